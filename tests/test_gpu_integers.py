"""The integer kernels of galois_amd/csrc/gfa_integers.hip on the device, against the host routes of galois_amd/_integers.py, the Sage
vectors and the reference's answers (tests/golden/{sage,reference}_numtheory.json), and against each other where two kernels
answer the same question.  All comparisons are exact."""
import ctypes
import json
import math
import os
import random

import numpy as np
import pytest
import torch

import galois_amd as ga
from galois_amd import _integers as gi
from galois_amd import _lib as L

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TWO64 = 1 << 64

# composites that fool short base sets, squares and semiprimes above 2^63, and the primes next to the top
EDGE = [0, 1, 2, 3, 4, 561, 41041, 3215031751, 341550071728321, 3825123056546413051, 4294967291**2, 4294967291 * 4294967279, 2**61 - 1,
        2**64 - 59, 2**64 - 1]
EDGE_PRIME = [False, False, True, True, False, False, False, False, False, False, False, False, True, True, False]


@pytest.fixture(scope="module")
def sage():
    with open(os.path.join(GOLDEN, "sage_numtheory.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLDEN, "reference_numtheory.json")) as fh:
        return json.load(fh)


def _dev_u64(values):
    return torch.from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).cuda()


def _u64_list(t: torch.Tensor) -> list:
    return [v % TWO64 for v in t.cpu().tolist()]


# ---- is_prime_batched ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_is_prime_batched_sizes(count):
    rnd = random.Random(count)
    for start, step in ((0, 1), (10**12 + 1, 2), (2**63 - 100, 3)):
        want = [ga.is_prime(start + i * step) for i in range(count)]
        values = [start + i * step for i in range(count)]
        got_list = ga.is_prime_batched(values)
        got_range = ga.is_prime_batched(range(start, start + count * step, step))
        assert got_list.dtype == bool and got_list.shape == (count,) and got_range.shape == (count,)
        assert got_list.tolist() == want and got_range.tolist() == want
    values = [rnd.getrandbits(rnd.choice((8, 32, 63, 64))) | 1 for _ in range(count)]
    t = _dev_u64(values)
    before = t.clone()
    assert ga.is_prime_batched(t).tolist() == [ga.is_prime(v) for v in values]
    assert torch.equal(t, before)


def test_is_prime_batched_edges_and_sage(sage):
    assert [ga.is_prime(n) for n in EDGE] == EDGE_PRIME  # the list itself, on the host
    assert ga.is_prime_batched(EDGE).tolist() == EDGE_PRIME
    assert ga.is_prime_batched(np.array(EDGE, dtype=np.uint64)).tolist() == EDGE_PRIME
    assert ga.is_prime_batched(torch.from_numpy(np.array(EDGE, dtype=np.uint64).view(np.int64))).tolist() == EDGE_PRIME
    X = [x for x in sage["is_prime"]["X"] if x >= 0]
    Z = [z for x, z in zip(sage["is_prime"]["X"], sage["is_prime"]["Z"]) if x >= 0]
    assert len(X) > 10 and ga.is_prime_batched(X).tolist() == Z
    with pytest.raises(ValueError):
        ga.is_prime_batched([3, -1])
    with pytest.raises(ValueError):
        ga.is_prime_batched([2**64])


def test_is_prime_range_at_the_top_of_the_word():
    top = 2**64 - 1
    got = ga.is_prime_batched(range(top - 2 * 99, top + 1, 2))  # ends exactly at 2^64 - 1
    assert got.shape == (100,) and got.tolist() == [ga.is_prime(top - 2 * (99 - i)) for i in range(100)]
    assert got[70] and top - 2 * 29 == 2**64 - 59
    flags = torch.zeros(101, dtype=torch.uint8, device="cuda")
    rc = L.lib().gfa_int_is_prime(None, 101, top - 2 * 99, 2, flags.data_ptr(), None)  # one step past it
    assert rc == L.ERR_INVALID and "2^64" in L.last_error()
    torch.cuda.synchronize()
    assert not flags.any()
    with pytest.raises(ValueError):
        ga.is_prime_batched(range(top - 2 * 99, top + 3, 2))


# ---- primes_in_range ------------------------------------------------------------------------------------------------------------------------
def _both_routes(start, stop):
    a = _u64_list(ga.primes_in_range(start, stop, _route="sieve"))
    b = _u64_list(ga.primes_in_range(start, stop, _route="test"))
    assert a == b, (start, stop)
    return a


def test_primes_in_range_small_and_counts(sage):
    got = ga.primes_in_range(0, 1000)
    assert got.dtype == torch.int64 and got.is_cuda
    below_1000 = got.tolist()
    assert below_1000 == _both_routes(0, 1000) == ga.primes(999, _route="host") and len(below_1000) == 168
    assert any(x < 1000 for x in sage["primes"]["X"])
    for x, z in zip(sage["primes"]["X"], sage["primes"]["Z"]):
        assert ga.primes(x, _route="device") == z
        if x < 1000:
            assert [p for p in below_1000 if p <= x] == z
    million = ga.primes_in_range(0, 10**6, _route="sieve")
    assert million.numel() == 78498 and million.tolist() == ga.primes(10**6, _route="host")
    ten_million = ga.primes_in_range(0, 10**7, _route="sieve")
    assert ten_million.numel() == 664579 and int(ten_million[-1]) == 9999991
    assert bool((ten_million[1:] > ten_million[:-1]).all())
    assert torch.equal(ten_million[:78498], million)


def test_primes_in_range_segment_edges():
    S = ga.sieve_segment_span()
    assert S == L.lib().gfa_int_sieve_segment_span() and S > 0 and S & (S - 1) == 0
    windows = [(S - 50, S + 50), (3 * S - 1, 3 * S + 1), (S, S + 1), (2, 3), (S + 1, S + 1), (0, 0), (0, 1), (0, 2), (0, 3), (1, 4), (2, 4), (3, 4),
               (S - 51, S + 51), (S - 1, S + 2), (2 * S - 7, 2 * S + 8), (S - 50, 2 * S + 51), (1, 2 * S + 2)]
    for start, stop in windows:
        got = _both_routes(start, stop)
        if stop - start <= 200:
            assert got == [n for n in range(start, stop) if ga.is_prime(n)], (start, stop)
    assert _both_routes(2, 3) == [2] and _both_routes(S, S + 1) == [] and _both_routes(0, 2 * S)[-1] == ga.prev_prime(2 * S)


def test_primes_in_range_at_and_above_the_sieve_bound(monkeypatch):
    lo, hi = 2**40 - 2**20, 2**40
    got = _both_routes(lo, hi)
    assert len(got) > 30000 and got[0] == ga.next_prime(lo - 1) and got[-1] == ga.prev_prime(hi - 1) == 2**40 - 87
    calls = []
    sieve = gi._sieve_window
    monkeypatch.setattr(gi, "_sieve_window", lambda *a: calls.append(a) or sieve(*a))
    above = ga.primes_in_range(2**40 - 1000, 2**40 + 1000)  # crosses the bound: the primality kernel
    assert not calls and _u64_list(above) == [n for n in range(2**40 - 1000, 2**40 + 1000) if ga.is_prime(n)]
    top = ga.primes_in_range(2**64 - 1000, 2**64)  # bit patterns of values above 2^63
    assert _u64_list(top) == [n for n in range(2**64 - 1000, 2**64) if ga.is_prime(n)] and _u64_list(top)[-1] == 2**64 - 59
    assert ga.primes_in_range(10**6, 10**6 + 10**5).numel() and len(calls) == 1  # a wide window below it: the sieve
    with pytest.raises(ValueError):
        ga.primes_in_range(0, 2**40 + 1, _route="sieve")
    with pytest.raises(ValueError):
        ga.primes_in_range(5, 4)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    bitmap = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert L.lib().gfa_int_sieve(2**40 - 100, 2**40 + 1, None, 0, bitmap.data_ptr(), counts.data_ptr(), None) == L.ERR_INVALID
    assert L.lib().gfa_int_sieve(100, 50, None, 0, bitmap.data_ptr(), counts.data_ptr(), None) == L.ERR_INVALID


# ---- jacobi_symbol_batched -------------------------------------------------------------------------------------------------------------------
JACOBI_MODULI = [3, 9, 15, 2**32 - 5, 2**63 + 29, 2**64 - 1, 2**64 - 59]


def _jacobi_arguments(n, rnd):
    fixed = [-(2**63), -1, 0, 1, n - 1, n, n + 1, 2**63 - 1]
    fixed = [a for a in fixed if -(2**63) <= a < 2**63]
    return fixed + [rnd.randrange(-(2**63), 2**63) for _ in range(57)] + [rnd.randrange(-50, 50) for _ in range(8)]


def test_jacobi_symbol_batched_shared_and_per_element():
    rnd = random.Random(7)
    all_a, all_n = [], []
    for n in JACOBI_MODULI:
        a = _jacobi_arguments(n, rnd)
        want = [ga.jacobi_symbol(v, n) for v in a]
        got = ga.jacobi_symbol_batched(a, n)
        assert got.dtype == np.int8 and got.tolist() == want, n
        assert set(want) <= {-1, 0, 1} and 0 in want and 1 in want and (-1 in want or n == 9)  # (a / 9) is a square
        all_a += a
        all_n += [n] * len(a)
    order = list(range(len(all_a)))
    rnd.shuffle(order)
    all_a, all_n = [all_a[i] for i in order], [all_n[i] for i in order]
    got = ga.jacobi_symbol_batched(all_a, all_n)
    assert got.tolist() == [ga.jacobi_symbol(a, n) for a, n in zip(all_a, all_n)]
    assert ga.jacobi_symbol_batched([], 9).shape == (0,)
    for bad in (8, 1, -7, 0):
        with pytest.raises(ValueError):
            ga.jacobi_symbol_batched([1, 2], bad)
    with pytest.raises(ValueError):
        ga.jacobi_symbol_batched([1, 2], [9, 10])
    with pytest.raises(ValueError):
        ga.jacobi_symbol_batched([1, 2], [9])


def test_jacobi_symbol_is_eulers_criterion_at_a_full_width_prime():
    p = 2**64 - 59
    rnd = random.Random(11)
    a = [0, 1, 2, p - 1, p - 2] + [rnd.randrange(p) for _ in range(59)]
    GF = ga.GF(p)
    powers = (GF(np.array(a, dtype=object)) ** ((p - 1) // 2)).numpy().tolist()  # the package's own GF(p) power
    want = [0 if v == 0 else (1 if v == 1 else -1) for v in powers]
    assert set(powers) <= {0, 1, p - 1}
    signed = [v if v < 2**63 else v - p for v in a]  # the same residues inside int64
    assert ga.jacobi_symbol_batched(signed, p).tolist() == want


# ---- the unit classifier -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 30, 2**16, 510510])
def test_totatives_on_the_device(n):
    want = [0] if n == 1 else [t for t in range(1, n) if math.gcd(t, n) == 1]
    assert ga.totatives(n, _route="device") == want
    assert ga.totatives(n) == want and len(want) == ga.euler_phi(n)


@pytest.mark.parametrize("n", [9, 18, 25, 27, 50, 31, 22, 2 * 3**9, 7**5])
def test_primitive_root_counts(ref, n):
    roots = list(ga.primitive_roots(n, _route="device"))
    assert len(roots) == ga.euler_phi(ga.euler_phi(n)) and roots == sorted(roots)
    if n <= 200:
        assert roots == ref["per_n"]["primitive_roots"][n - 1]
        assert list(ga.primitive_roots(n, reverse=True, _route="device")) == ref["per_n"]["primitive_roots_reversed"][n - 1]
    assert list(ga.primitive_roots(n)) == roots  # host first chunk, then the device
    root_set = set(roots)
    assert ga.is_primitive_root_batched(list(range(1, n)), n).tolist() == [g in root_set for g in range(1, n)]
    assert ga.primitive_root(n, _route="device") == roots[0] and ga.primitive_root(n, method="max", _route="device") == roots[-1]


def test_primitive_roots_of_65537_are_the_non_residues():
    n = 65537
    g = list(range(1, n))
    flags = ga.is_primitive_root_batched(g, n)
    assert int(flags.sum()) == 32768
    assert flags.tolist() == (ga.jacobi_symbol_batched(g, n) == -1).tolist()  # an independent kernel
    assert list(ga.primitive_roots(n)) == [v for v, f in zip(g, flags.tolist()) if f]


@pytest.mark.parametrize("n", [2**61 - 1, 2**64 - 59])
def test_classifier_at_full_width_moduli(n):
    rnd = random.Random(n)
    g = [1, 2, 3, 37, n - 1, n - 2] + [rnd.randrange(1, n) for _ in range(251)]
    phi, exps = gi._phi_exponents(n)
    want = [all(pow(v, e, n) != 1 for e in exps) for v in g]
    assert phi == n - 1 and any(want) and not all(want)
    t = _dev_u64(g)
    before = t.clone()
    assert ga.is_primitive_root_batched(t, n).tolist() == want
    assert torch.equal(t, before)
    assert ga.is_primitive_root_batched(g, n).tolist() == want
    assert ga.primitive_root(n, _route="device") == ga.primitive_root(n, _route="host")


def test_primitive_roots_across_chunk_edges(ref):
    n = 2 * 7**5
    phi, exps = gi._phi_exponents(n)
    every = [g for g in range(1, n) if gi._is_root(g, n, phi, exps)]  # 16807 odd candidates: chunks of 256, 1024, 4096, 16384
    assert list(ga.primitive_roots(n, _route="device")) == every
    assert list(ga.primitive_roots(n, reverse=True, _route="device")) == every[::-1]
    assert list(ga.primitive_roots(n, reverse=True)) == every[::-1] and list(ga.primitive_roots(n)) == every
    window = ref["misc"]["primitive_roots(2*7^5)[start, stop)"]
    assert list(ga.primitive_roots(n, start=1000, stop=1100, _route="device")) == window
    assert list(ga.primitive_roots(n, start=1000, stop=1100, reverse=True, _route="device")) == window[::-1]
    for n_big, method, want in ref["primitive_root"]:
        if n_big < TWO64:
            assert ga.primitive_root(n_big, method=method, _route="device") == want
    assert not list(ga.primitive_roots(2**20 + 4)) and not list(ga.primitive_roots(15 * 2**30))  # no roots: no launch needed
    assert ga.is_primitive_root_batched([1, 3, 5], 8).tolist() == [False] * 3 and ga.is_primitive_root_batched([1, 3], 4).tolist() == [False, True]


def test_polymorphic_functions_on_polynomials():
    GF = ga.GF(7)
    a, b, c = ga.Poly([1, 3], field=GF), ga.Poly([1, 5], field=GF), ga.Poly([1, 0, 1], field=GF)
    assert ga.are_coprime(a, b, c) and not ga.are_coprime(a, a * b)
    assert ga.is_square_free(a * b * c) and not ga.is_square_free(a * a * c)
    with pytest.raises(TypeError):
        ga.are_coprime(a, 3)
    with pytest.raises(TypeError):
        ga.is_square_free("x")


# ---- the C entry points' contract ------------------------------------------------------------------------------------------------------------------
def test_entry_points_reject_and_accept():
    lib = L.lib()
    flags = torch.zeros(8, dtype=torch.uint8, device="cuda")
    vals = _dev_u64([1, 2, 3, 4, 5, 6, 7, 8])
    a = torch.arange(8, dtype=torch.int64, device="cuda")
    out8 = torch.zeros(8, dtype=torch.int8, device="cuda")
    exps = (ctypes.c_uint64 * 2)(3, 2)
    one_n = ctypes.c_uint64(9)
    # even moduli that are not twice an odd number have no Montgomery form: with exponents, unsupported
    for n in (4, 8, 12, 2**40):
        assert lib.gfa_int_unit_classify(n, vals.data_ptr(), 8, 0, 0, exps, 2, flags.data_ptr(), None) == L.ERR_UNSUPPORTED
        assert lib.gfa_int_unit_classify(n, vals.data_ptr(), 8, 0, 0, None, 0, flags.data_ptr(), None) == L.OK  # units alone are served
    torch.cuda.synchronize()
    assert (flags & 1).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    # null pointers and bad counts
    assert lib.gfa_int_is_prime(vals.data_ptr(), 8, 0, 0, None, None) == L.ERR_INVALID
    assert lib.gfa_int_is_prime(vals.data_ptr(), -1, 0, 0, flags.data_ptr(), None) == L.ERR_INVALID
    assert lib.gfa_int_unit_classify(7, vals.data_ptr(), 6, 0, 0, exps, 2, None, None) == L.ERR_INVALID
    assert lib.gfa_int_unit_classify(7, vals.data_ptr(), 6, 0, 0, None, 2, flags.data_ptr(), None) == L.ERR_INVALID
    assert lib.gfa_int_unit_classify(0, vals.data_ptr(), 6, 0, 0, None, 0, flags.data_ptr(), None) == L.ERR_INVALID
    assert lib.gfa_int_unit_classify(7, None, 6, 2**64 - 3, 1, None, 0, flags.data_ptr(), None) == L.ERR_INVALID  # the range passes 2^64
    assert lib.gfa_int_unit_classify(7, vals.data_ptr(), 6, 0, 0, exps, 17, flags.data_ptr(), None) == L.ERR_INVALID
    assert lib.gfa_int_jacobi(None, ctypes.addressof(one_n), 8, 0, out8.data_ptr(), None) == L.ERR_INVALID
    assert lib.gfa_int_jacobi(a.data_ptr(), ctypes.addressof(one_n), 8, 0, None, None) == L.ERR_INVALID
    assert lib.gfa_int_jacobi(a.data_ptr(), None, 8, 0, out8.data_ptr(), None) == L.ERR_INVALID
    for bad in (0, 1, 2, 8, 2**64 - 2):
        bad_n = ctypes.c_uint64(bad)
        assert lib.gfa_int_jacobi(a.data_ptr(), ctypes.addressof(bad_n), 8, 0, out8.data_ptr(), None) == L.ERR_INVALID
    bitmap = torch.zeros(4, dtype=torch.int32, device="cuda")
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    primes = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert lib.gfa_int_sieve(0, 100, None, 0, None, counts.data_ptr(), None) == L.ERR_INVALID
    assert lib.gfa_int_sieve(0, 100, None, 0, bitmap.data_ptr(), None, None) == L.ERR_INVALID
    assert lib.gfa_int_sieve(0, 100, None, 3, bitmap.data_ptr(), counts.data_ptr(), None) == L.ERR_INVALID
    assert lib.gfa_int_sieve_expand(0, 100, None, counts.data_ptr(), primes.data_ptr(), None) == L.ERR_INVALID
    assert lib.gfa_int_sieve_expand(0, 100, bitmap.data_ptr(), None, primes.data_ptr(), None) == L.ERR_INVALID
    assert lib.gfa_int_sieve_expand(0, 100, bitmap.data_ptr(), counts.data_ptr(), None, None) == L.ERR_INVALID
    # nothing to do is a success, whatever the pointers
    assert lib.gfa_int_is_prime(None, 0, 0, 0, None, None) == L.OK
    assert lib.gfa_int_unit_classify(7, None, 0, 0, 0, None, 0, None, None) == L.OK
    assert lib.gfa_int_jacobi(None, ctypes.addressof(one_n), 0, 0, None, None) == L.OK
    assert lib.gfa_int_sieve(5, 5, None, 0, None, None, None) == L.OK and lib.gfa_int_sieve_expand(4, 5, None, None, None, None) == L.OK
    torch.cuda.synchronize()
    assert not out8.any() and not primes.any() and not bitmap.any() and vals.tolist() == [1, 2, 3, 4, 5, 6, 7, 8] and a.tolist() == list(range(8))
    # the sieve with the base primes of the caller, by hand: [0, 100) needs 3, 5 and 7
    base = torch.tensor([3, 5, 7], dtype=torch.int32, device="cuda")
    assert lib.gfa_int_sieve(0, 100, base.data_ptr(), 3, bitmap.data_ptr(), counts.data_ptr(), None) == L.OK
    offsets = torch.ones(1, dtype=torch.int64, device="cuda")
    assert lib.gfa_int_sieve_expand(0, 100, bitmap.data_ptr(), offsets.data_ptr(), primes.data_ptr(), None) == L.OK
    torch.cuda.synchronize()
    assert int(counts[0]) == 24 and primes[:25].tolist() == ga.primes(100, _route="host") and not primes[25:].any()
    assert base.tolist() == [3, 5, 7]
