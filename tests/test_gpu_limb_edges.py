"""The multi-limb kernels (csrc/gfa_wide.hip: 2 limbs; csrc/gfa_big.hip: 4 / 8 / 16 limbs) where carries, borrows and the final
conditional subtraction decide the answer: moduli that fill the top limb (a + b carries out of it, a + p wraps in the borrow
branch of the subtraction, the Montgomery accumulator's overflow word is set), every (limb count, kind) pair of the dispatch, the
masking branches of the binary product (m = 64, m a multiple of 64 below 64 NL, m = 64 NL), the extension kernels at their largest
degree and characteristic, a second pass of the grid-stride loop, and a zero stride on every operand.  The fields are those of
tests/limb_fields.py (their moduli are verified by tests/test_limb_params_host.py); the reference is oracle/wide_oracle.py, Python's
own integers."""
import random
import zlib

import numpy as np
import pytest
import torch

from oracle.wide_oracle import WideOracle
from tests import helpers as H
from tests import limb_fields as LF

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
N_RANDOM = 300


class _Oracle(WideOracle):
    """WideOracle with its inversions remembered: an inversion in a 1024-bit binary field is an exponentiation that takes the oracle
    more than half a second, and the tests of one field share their divisors.  Every formula is the oracle's own."""

    def __init__(self, *a):
        super().__init__(*a)
        self._inverses = {}

    def inv(self, a):
        if a not in self._inverses:
            self._inverses[a] = super().inv(a)
        return self._inverses[a]


_CTX = {}


def _ctx(tag):
    if tag not in _CTX:
        f = LF.FIELDS[tag]
        GF = LF.make_field(tag)
        assert GF._NL == f["nl"] and GF.dtypes == [np.object_] and GF.order == f["p"] ** f["m"]
        _CTX[tag] = (GF, _Oracle(f["p"], f["m"], LF.irr_coeffs(f)), f)
    return _CTX[tag]


def _rng(tag, salt):
    return random.Random(zlib.crc32(f"{tag}/{salt}".encode()))


def _obj(v):
    return np.array([int(x) for x in v], dtype=object)


def _obj2(rows):
    out = np.empty((len(rows), len(rows[0])), dtype=object)
    for i, r in enumerate(rows):
        for j, v in enumerate(r):
            out[i, j] = int(v)
    return out


def _slow(f):
    """Fields whose oracle spends more than 0.1 s per exponentiation by a full-size exponent (measured: 0.14 s in GF(2^512), 0.2 s in
    GF(2^576), 0.5 s in GF((2^32-5)^25), 0.65 s in GF(2^1024); at most 0.06 s in every other field of the table)."""
    return f["m"] > 1 and (f["p"] ** f["m"]).bit_length() > 512


def _n_quotients(f):
    """Random quotient cases per field: the oracle inverts in microseconds in a prime field and by an exponentiation elsewhere
    (0.05 s at 130 bits, 0.06 s at 320, 0.14 s at 512, 0.65 s at 1024 bits); never fewer than 8."""
    bits = (f["p"] ** f["m"]).bit_length()
    return 100 if f["m"] == 1 else 40 if bits <= 200 else 24 if bits <= 400 else 12 if bits <= 520 else 8


def _edge_operands(f):
    p, m, nl = f["p"], f["m"], f["nl"]
    q, N = p**m, 64 * nl
    e = [0, 1, 2, q - 1, q - 2, p - 1, p]  # p: the element "x" of an extension field
    for i in range(nl):  # every limb boundary of this limb count
        e += [(1 << (64 * i)) - 1, 1 << (64 * i), (1 << (64 * i)) + 1]
    e += [q // 2, q // 2 + 1]
    if m == 1:
        e.append(1 << (N - 1))  # with itself: the sum is exactly 2^N when p is full width
        r = _rng("edge", N).randrange(p // 3, p // 2)
        e += [r, p - r, p - r + 1, p - r - 1]  # a + b = p, p + 1, p - 1 (as are 1 + (q - 1), 2 + (q - 1), 1 + (q - 2))
        if p >> (N - 1):  # full width: a + p reaches 2^N from a = 2^N - p on
            d = (1 << N) - p
            e += [d - 1, d, d + 1]
    out = []
    for v in e:
        if v % q not in out:
            out.append(v % q)
    return out


def _divisors(tag):
    """The divisors every test of one field shares (the oracle inverts each of them once): the edge divisors 1, q - 1, p - 1 and
    p, then random ones."""
    GF, W, f = _ctx(tag)
    q, p = W.q, W.p
    rng = _rng(tag, "divisors")
    out = [v for v in dict.fromkeys([1, q - 1, p - 1, p % q]) if v]
    return out + [rng.randrange(1, q) for _ in range(_n_quotients(f))]


@pytest.mark.parametrize("tag", LF.TAGS)
def test_random_operands_and_named_carry_pairs_against_the_oracle(tag):
    GF, W, f = _ctx(tag)
    q, p, N = W.q, W.p, 64 * f["nl"]
    rng = _rng(tag, "random")
    a = [rng.randrange(q) for _ in range(N_RANDOM)]
    b = [rng.randrange(q) for _ in range(N_RANDOM)]
    if tag in LF.FULL_WIDTH_PRIMES:
        # the carry branches are really taken: computed from the Python integers alone.  Uniform operands below a full-width p
        # give about one half each, a quarter is asserted.
        n_carry = sum(x + y >= 1 << N for x, y in zip(a, b))
        n_wrap = sum(x < y and x + p >= 1 << N for x, y in zip(a, b))
        print(f"{tag}: {n_carry} of {N_RANDOM} pairs with a + b >= 2^{N}, {n_wrap} with a < b and a + p >= 2^{N}")
        assert n_carry >= N_RANDOM // 4 and n_wrap >= N_RANDOM // 4, (tag, n_carry, n_wrap)
    if f["m"] == 1:
        h = (1 << (N - 1)) % p
        pairs = [(h, h)]
        for _ in range(6):
            r = rng.randrange(1, p - 1)
            pairs += [(r, p - r), (r, (p - r + 1) % p), (r, p - r - 1)]  # a + b = p, p + 1, p - 1
        if p >> (N - 1):
            d = (1 << N) - p
            for x in (d - 1, d, d + 1, rng.randrange(d, p - 1), rng.randrange(d, p - 1)):
                pairs += [(x, x + 1), (x, p - 1)]  # a < b; a + p = 2^N - 1, 2^N, 2^N + 1, beyond
            assert any(x + y == 1 << N for x, y in pairs) and any(x < y and x + p == 1 << N for x, y in pairs)
        assert all(0 <= x < p and 0 <= y < p for x, y in pairs) and any(x + y == p for x, y in pairs)
        a += [x for x, _ in pairs]
        b += [y for _, y in pairs]
    A, B = GF(_obj(a)), GF(_obj(b))
    assert type(A + B) is GF and (A + B).dtype == np.dtype(object)
    H.assert_equal_ints((A + B).numpy(), _obj(W.add(x, y) for x, y in zip(a, b)), f"{tag} add")
    H.assert_equal_ints((A - B).numpy(), _obj(W.sub(x, y) for x, y in zip(a, b)), f"{tag} sub")
    H.assert_equal_ints((B - A).numpy(), _obj(W.sub(y, x) for x, y in zip(a, b)), f"{tag} sub, operands swapped")
    H.assert_equal_ints((A * B).numpy(), _obj(W.mul(x, y) for x, y in zip(a, b)), f"{tag} mul")
    H.assert_equal_ints((-A).numpy(), _obj(W.neg(x) for x in a), f"{tag} neg")
    H.assert_equal_ints(np.square(B).numpy(), _obj(W.mul(y, y) for y in b), f"{tag} square")


@pytest.mark.parametrize("tag", LF.TAGS)
def test_every_pair_of_edge_operands_against_the_oracle(tag):
    GF, W, f = _ctx(tag)
    e = _edge_operands(f)
    assert len(set(e)) == len(e) and all(0 <= v < W.q for v in e)
    assert {0, 1, 2, W.q - 1, W.q - 2, W.q // 2, W.q // 2 + 1, W.p - 1, W.p % W.q} <= set(e)  # (the 2^(64 i) at or above q wrap to small values)
    E = GF(_obj(e))
    col, row = E.reshape((len(e), 1)), E.reshape((1, len(e)))
    for name, got, fn in (("add", col + row, W.add), ("sub", col - row, W.sub), ("mul", col * row, W.mul)):
        assert got.shape == (len(e), len(e))
        H.assert_equal_ints(got.numpy(), _obj2([[fn(x, y) for y in e] for x in e]), f"{tag} {name} of every pair of edge operands")
    H.assert_equal_ints((-E).numpy(), _obj(W.neg(x) for x in e), f"{tag} neg of the edge operands")


@pytest.mark.parametrize("tag", LF.TAGS)
def test_quotients_and_reciprocals_against_the_oracle(tag):
    GF, W, f = _ctx(tag)
    q = W.q
    rng = _rng(tag, "dividends")
    d = _divisors(tag)
    assert len(d) >= 8 + 2 and {1, q - 1, W.p - 1} <= set(d) and (f["m"] == 1 or W.p in d)
    a = [0, 1, q - 1] + [rng.randrange(q) for _ in range(len(d) - 3)]
    A, D = GF(_obj(a)), GF(_obj(d))
    H.assert_equal_ints(np.reciprocal(D).numpy(), _obj(W.inv(y) for y in d), f"{tag} reciprocal")
    H.assert_equal_ints((A / D).numpy(), _obj(W.div(x, y) for x, y in zip(a, d)), f"{tag} div")
    H.assert_equal_ints((D ** -1).numpy(), _obj(W.inv(y) for y in d), f"{tag} ** -1")
    # many more inversions than the oracle has time for, checked by the product (itself checked against the oracle above)
    r = [rng.randrange(1, q) for _ in range(N_RANDOM)] + [v for v in _edge_operands(f) if v]
    R = GF(_obj(r))
    H.assert_equal_ints((R * np.reciprocal(R)).numpy(), _obj([1] * len(r)), f"{tag} x * (1 / x)")
    H.assert_equal_ints((R / R).numpy(), _obj([1] * len(r)), f"{tag} x / x")
    with pytest.raises(ZeroDivisionError):
        A / GF(_obj([1] * (len(a) - 1) + [0]))
    with pytest.raises(ZeroDivisionError):
        np.reciprocal(GF(_obj([1, 0])))


@pytest.mark.parametrize("tag", LF.TAGS)
def test_powers_with_one_exponent_per_element_against_the_oracle(tag):
    GF, W, f = _ctx(tag)
    q = W.q
    rng = _rng(tag, "powers")
    n_rand = 3 if _slow(f) else 12
    es = [0, 1, 2, -1, -2, q - 1, q, -(q - 1), 3 * q + 5] + [rng.randrange(-q, q) for _ in range(n_rand)]
    d = _divisors(tag)  # bases whose inverses the oracle already holds (a negative exponent inverts the base first)
    base = [d[(3 + i) % len(d)] for i in range(len(es))]
    got = GF(_obj(base)) ** np.array(es, dtype=object)
    H.assert_equal_ints(got.numpy(), _obj(W.pow(x, e) for x, e in zip(base, es)), f"{tag} power")
    assert int(GF(0) ** 0) == 1 and int(GF(0) ** 5) == 0 and int(GF(0) ** (q - 1)) == 0 and int(GF(0) ** q) == 0
    with pytest.raises(ZeroDivisionError):
        GF(_obj([2, 0])) ** np.array([3, -3], dtype=object)


@pytest.mark.parametrize("tag", LF.TAGS)
def test_zero_stride_on_either_operand_and_on_the_exponent(tag):
    """A scalar on the LEFT (sa = 0 in the binary and power kernels) and one exponent for a whole array (se = 0)."""
    GF, W, f = _ctx(tag)
    q = W.q
    rng = _rng(tag, "stride")
    c = rng.randrange(q // 2, q)
    C = GF(c)
    assert C.shape == ()
    a = _edge_operands(f) + [rng.randrange(q) for _ in range(70)]  # more than one wavefront of lanes
    A = GF(_obj(a))
    H.assert_equal_ints((C * A).numpy(), _obj(W.mul(c, x) for x in a), f"{tag} scalar * array")
    H.assert_equal_ints((C - A).numpy(), _obj(W.sub(c, x) for x in a), f"{tag} scalar - array")
    H.assert_equal_ints((C + A).numpy(), _obj(W.add(c, x) for x in a), f"{tag} scalar + array")
    H.assert_equal_ints((A - C).numpy(), _obj(W.sub(x, c) for x in a), f"{tag} array - scalar")
    d = _divisors(tag)
    H.assert_equal_ints((C / GF(_obj(d))).numpy(), _obj(W.div(c, y) for y in d), f"{tag} scalar / array")
    # scalar base, array of exponents: small ones, and a few of full size (one of them negative: the base is a shared divisor)
    g = d[-1]
    big = [q - 2, -1, rng.randrange(q)] if _slow(f) else [q - 2, -1, q - 1, -(q - 2)] + [rng.randrange(-q, q) for _ in range(8)]
    es = [0, 1, 2, 3, 65537, -2] + [rng.randrange(1 << 20) for _ in range(70)] + big
    got = GF(g) ** np.array(es, dtype=object)
    assert got.shape == (len(es),)
    H.assert_equal_ints(got.numpy(), _obj(W.pow(g, e) for e in es), f"{tag} scalar ** array of exponents")
    # one exponent for the whole array
    H.assert_equal_ints((A ** 65537).numpy(), _obj(W.pow(x, 65537) for x in a), f"{tag} array ** 65537")
    e = (1 << 64) + 3  # (an exponent with a second limb; the oracle's 66 products per element are paid for the last 70 elements only)
    H.assert_equal_ints((A[-70:] ** e).numpy(), _obj(W.pow(x, e) for x in a[-70:]), f"{tag} array ** (2^64 + 3)")
    D = GF(_obj(d))
    H.assert_equal_ints((D ** -3).numpy(), _obj(W.pow(y, -3) for y in d), f"{tag} array ** -3")


# the launches cap the grid at 2048 blocks of 256 lanes (two limbs) and 4096 blocks of 64 lanes (k limbs): longer arrays make a
# second pass of the grid-stride loop
@pytest.mark.parametrize("tag, lanes, tail", [("p_2e128_m159", 2048 * 256, 300), ("p_2e256_m189", 4096 * 64, 100)])
def test_second_pass_of_the_grid_stride_loop(tag, lanes, tail):
    GF, W, f = _ctx(tag)
    p, nl = W.p, f["nl"]
    n = lanes + tail
    rng = np.random.default_rng(n)

    def limbs():
        v = rng.integers(0, 1 << 64, (n, nl), dtype=np.uint64, endpoint=False)
        v[:, nl - 1] = rng.integers(0, M64, n, dtype=np.uint64)  # top limb below 2^64 - 1: the value is below 2^(64 nl) - 2^(64 nl - 64) < p
        return v

    def ints(v):
        return [sum(x << (64 * k) for k, x in enumerate(r)) for r in v.tolist()]

    la, lb = limbs(), limbs()
    a, b = ints(la), ints(lb)
    assert max(a) < p and max(b) < p
    x = GF._wrap(torch.from_numpy(la.view(np.int64)).cuda())
    y = GF._wrap(torch.from_numpy(lb.view(np.int64)).cuda())
    assert x.shape == (n,)
    for name, got, fn in (("add", x + y, W.add), ("mul", x * y, W.mul)):
        want = np.array([[(v >> (64 * k)) & M64 for k in range(nl)] for v in map(fn, a, b)], dtype=np.uint64)
        have = got._t.cpu().numpy().view(np.uint64)
        assert have.shape == want.shape
        bad = np.flatnonzero((have != want).any(axis=1))
        assert bad.size == 0, (f"{tag} {name}: {bad.size} of {n} elements differ, first at {bad[:5].tolist()}; {int(np.count_nonzero(bad >= lanes))} of them "
                               f"among the last {tail} (index >= {lanes}), which only the second pass of the grid-stride loop computes")


# ---- kernels with their own loops over the same device functions (two-limb fields only): folds, convolution, matrix product,
# elimination -- on the full-width fields of each kind
LOOP_TAGS = ["p_2e128_m159", "gf65521e8", "gf2e64"]


def _left_fold(fn, row):
    acc = int(row[0])
    for v in row[1:]:
        acc = fn(acc, int(v))
    return acc


@pytest.mark.parametrize("tag", LOOP_TAGS)
def test_folds_convolution_and_matrix_product_of_the_full_width_two_limb_fields(tag):
    GF, W, f = _ctx(tag)
    q = W.q
    rng = _rng(tag, "loops")
    h = np.array([rng.randrange(1, q) for _ in range(5 * 700)], dtype=object).reshape(5, 700)
    h[0, 0], h[1, 5], h[4, 699] = q - 1, 1, q - 2
    x = GF(h)
    for uf, fn in ((np.add, W.add), (np.multiply, W.mul)):
        H.assert_equal_ints(uf.reduce(x, axis=1).numpy(), _obj(_left_fold(fn, r) for r in h), f"{tag} {uf.__name__}.reduce along rows")
        H.assert_equal_ints(uf.reduce(x, axis=0).numpy(), _obj(_left_fold(fn, c) for c in h.T), f"{tag} {uf.__name__}.reduce along columns")
    u, v = [int(t) for t in h[2, :40]], [int(t) for t in h[3, :33]]
    want = [0] * (40 + 33 - 1)
    for i, s in enumerate(u):
        for j, t in enumerate(v):
            want[i + j] = W.add(want[i + j], W.mul(s, t))
    H.assert_equal_ints(np.convolve(GF(_obj(u)), GF(_obj(v))).numpy(), _obj(want), f"{tag} convolve 40 x 33")
    a, b = h[0, :9 * 17].reshape(9, 17), h[1, :17 * 6].reshape(17, 6)
    wm = [[_left_fold(W.add, [0] + [W.mul(int(a[i, k]), int(b[k, j])) for k in range(17)]) for j in range(6)] for i in range(9)]
    H.assert_equal_ints((GF(a) @ GF(b)).numpy(), _obj2(wm), f"{tag} (9, 17) @ (17, 6)")


def _row_reduce(W, rows, ncols):
    """row_reduce_jit of the reference on the oracle's scalars: the first non-zero entry at or below the pivot row, swap, scale to a
    leading 1, clear the column."""
    A = [list(map(int, r)) for r in rows]
    m, piv = len(A), 0
    for j in range(ncols):
        nz = [i for i in range(piv, m) if A[i][j]]
        if not nz:
            continue
        A[piv], A[nz[0]] = A[nz[0]], A[piv]
        inv = W.inv(A[piv][j])
        A[piv] = [W.mul(v, inv) for v in A[piv]]
        for i in range(m):
            if i != piv and A[i][j]:
                fct = A[i][j]
                A[i] = [W.sub(v, W.mul(fct, t)) for v, t in zip(A[i], A[piv])]
        piv += 1
        if piv == m:
            break
    return A, piv


@pytest.mark.parametrize("tag", LOOP_TAGS)
def test_elimination_of_12_by_12_matrices_over_the_full_width_two_limb_fields(tag):
    GF, W, f = _ctx(tag)
    q = W.q
    rng = _rng(tag, "elimination")
    n = 12
    a = [[rng.randrange(q) for _ in range(n)] for _ in range(n)]
    a[0][0], a[1][0], a[3][3] = 0, 0, q - 1  # the first pivot is found two rows down
    inv_want, rank = _row_reduce(W, [r + [int(i == j) for j in range(n)] for i, r in enumerate(a)], n)
    assert rank == n and all(inv_want[i][j] == int(i == j) for i in range(n) for j in range(n))
    inv_want = [r[n:] for r in inv_want]
    A = GF(_obj2(a))
    Ai = np.linalg.inv(A)
    H.assert_equal_ints(Ai.numpy(), _obj2(inv_want), f"{tag} inverse of a 12 x 12 matrix")
    eye = _obj2([[int(i == j) for j in range(n)] for i in range(n)])
    H.assert_equal_ints((A @ Ai).numpy(), eye, f"{tag} A @ inv(A)")
    H.assert_equal_ints((Ai @ A).numpy(), eye, f"{tag} inv(A) @ A")
    H.assert_equal_ints(A.row_reduce().numpy(), eye, f"{tag} row_reduce of an invertible matrix")
    # rank 10: two rows are combinations of others, so the reduced form keeps two free columns and two zero rows
    s = [list(r) for r in a]
    s[5] = [W.add(x, y) for x, y in zip(s[2], s[7])]
    s[11] = [W.sub(W.mul(x, q - 2), y) for x, y in zip(s[0], s[4])]
    rr_want, rank = _row_reduce(W, s, n)
    assert rank == 10
    H.assert_equal_ints(GF(_obj2(s)).row_reduce().numpy(), _obj2(rr_want), f"{tag} row_reduce of a rank-10 matrix")
    assert np.linalg.matrix_rank(GF(_obj2(s))) == 10
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.inv(GF(_obj2(s)))
