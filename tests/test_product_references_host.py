"""The two cheap references behind the full-output matrix-product tests (tests/helpers.py) bite: the projection check accepts a
correct product and rejects every kind of damage a plane / limb / tile kernel can do, and the float64 prime-field product equals the
oracle's.  Host only: the oracle is the checker here, no device code runs."""
import numpy as np
import pytest

from oracle import gf_oracle as O
from tests import helpers as H

GF13E5 = 13**5


def _fields():
    ext = O.OracleField(13, 5, 13**5 + 4 * 13 + 11, 13)  # x^5 + 4 x + 11 (Conway), primitive element x
    yield "GF(13^5)", GF13E5, ext.matmul
    yield "GF(2^64 - 2^32 + 1)", H.GOLDILOCKS, H.python_int_matmul(H.GOLDILOCKS)


def _corruptions(A, B, C, q, mul_mat):
    M, N = C.shape
    K = A.shape[1]
    c = C.copy(); c[M // 2, N // 3] = (int(c[M // 2, N // 3]) + 1) % q
    yield "one entry off by one", c
    c = C.copy(); c[M - 1, 5] = (int(c[M - 1, 5]) + 1) % q; c[M - 1, N - 2] = (int(c[M - 1, N - 2]) + q - 1) % q
    yield "+1 and -1 in one row", c
    c = C.copy(); c[[3, M - 4]] = c[[M - 4, 3]]
    yield "two rows swapped", c
    c = C.copy(); c[M - 8:, N - 8:] = 0
    yield "last 8 x 8 corner zeroed", c
    yield "B read as if it were stored transposed", np.asarray(mul_mat(A, B.reshape(N, K).T))


@pytest.mark.parametrize("name,q,mul_mat", list(_fields()), ids=["gf13e5", "goldilocks"])
def test_projection_check_accepts_the_product_and_rejects_damage(name, q, mul_mat):
    rng = np.random.default_rng(41)
    M, K, N = 96, 80, 72
    A, B = rng.integers(0, q, (M, K), dtype=np.uint64), rng.integers(0, q, (K, N), dtype=np.uint64)
    C = np.asarray(mul_mat(A, B))
    assert H.projection_width(q) == (2 if q == GF13E5 else 1)
    H.assert_product_by_projection(mul_mat, A, B, C, q, np.random.default_rng(7), name)
    for what, bad in _corruptions(A, B, C, q, mul_mat):
        assert bad.shape == C.shape and not H.as_int_list(bad) == H.as_int_list(C), what
        with pytest.raises(AssertionError):
            H.assert_product_by_projection(mul_mat, A, B, bad, q, np.random.default_rng(7), f"{name} {what}")
    out_of_field = C.copy().astype(object)
    out_of_field[0, 0] = int(out_of_field[0, 0]) + q  # congruent, but not a field element
    with pytest.raises(AssertionError):
        H.assert_product_by_projection(mul_mat, A, B, out_of_field, q, np.random.default_rng(7), name)


def test_projection_width_keeps_the_error_bound_below_2_to_minus_32():
    for q, want in ((2**16 + 1, 2), (13**5, 2), (3**11, 2), (3**16, 2), (5**8, 2), (2**31 - 1, 2), (2**32, 1), (2**61 - 1, 1), (H.GOLDILOCKS, 1)):
        nvec = H.projection_width(q)
        assert nvec == want and q**nvec >= 2**32 and (nvec == 1 or q ** (nvec - 1) < 2**32)


@pytest.mark.parametrize("p", [2, 3, 127, 251])
def test_exact_prime_matmul_equals_the_oracle(p):
    rng = np.random.default_rng(p)
    A, B = rng.integers(0, p, (70, 300)), rng.integers(0, p, (300, 50))
    A[0], B[:, 0] = p - 1, p - 1  # the largest sum
    alpha = {2: 1, 3: 2, 127: 3, 251: 6}[p]
    H.assert_equal_ints(H.exact_prime_matmul(A, B, p), O.OracleField(p, 1, None, alpha).matmul(A, B), f"GF({p})")
    with pytest.raises(AssertionError):
        H.exact_prime_matmul(A + 1, B, p)  # an entry equal to p is no residue
    with pytest.raises(AssertionError):
        H.exact_prime_matmul(A, B, 243)  # the order of a field, but no prime: its product is not the integers' mod 243
