"""Integer number theory without a device: every public name of galois_amd/_integers.py on its host route against the Sage vectors
of the reference's own tests (tests/golden/sage_numtheory.json) and live answers of the reference
(tests/golden/reference_numtheory.json, written by tests/golden/generate_numtheory_golden.py), and the per-lane routines of the
kernels (galois_amd/csrc/gfa_integers.h) compiled with g++ -- once plain, once under AddressSanitizer and UBSan.  All
comparisons are exact."""
import json
import math
import os
import random
import subprocess

import pytest

import galois_amd as ga
from galois_amd import _integers as gi
from galois_amd import _numtheory as nt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def sage():
    with open(os.path.join(GOLDEN, "sage_numtheory.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLDEN, "reference_numtheory.json")) as fh:
        return json.load(fh)


def _plain(v):
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def _answer(fn, *args, **kwargs):
    """The fixture's form of an answer: lists for tuples and generators, {"error": [type, message]} for a rejection."""
    try:
        out = fn(*args, **kwargs)
        if hasattr(out, "__next__"):
            out = list(out)
        return _plain(out)
    except Exception as e:
        return {"error": [type(e).__name__, str(e)]}


NAMES = ["primes", "kth_prime", "prev_prime", "next_prime", "random_prime", "mersenne_exponents", "mersenne_primes", "fermat_primality_test",
         "miller_rabin_primality_test", "legendre_symbol", "jacobi_symbol", "kronecker_symbol", "perfect_power", "trial_division", "pollard_p1",
         "pollard_rho", "divisors", "divisor_sigma", "is_prime", "is_composite", "is_prime_power", "is_perfect_power", "is_smooth",
         "is_powersmooth", "isqrt", "iroot", "ilog", "totatives", "euler_phi", "mobius", "carmichael_lambda", "is_cyclic", "is_primitive_root",
         "primitive_root", "primitive_roots", "are_coprime", "is_square_free", "is_prime_batched", "primes_in_range", "jacobi_symbol_batched",
         "is_primitive_root_batched", "gcd", "egcd", "lcm", "prod", "crt", "factors"]


def test_every_name_is_exported():
    for name in NAMES:
        assert callable(getattr(ga, name)), name
        assert name in ga.__all__, name
    assert ga.is_prime is gi.is_prime and ga.primitive_root is gi.primitive_root and ga.is_primitive_root is gi.is_primitive_root


# ---- Sage ---------------------------------------------------------------------------------------------------------------------------
def test_sage_single_argument_vectors(sage):
    for name in ("kth_prime", "prev_prime", "next_prime", "is_prime", "is_prime_power", "is_perfect_power", "is_square_free", "euler_phi",
                 "carmichael_lambda", "is_cyclic", "isqrt"):
        fn = getattr(ga, name)
        X, Z = sage[name]["X"], sage[name]["Z"]
        assert len(X) == len(Z) > 0
        for x, z in zip(X, Z):
            got = fn(x)
            assert got == z and type(got) is type(z), (name, x, got, z)


def test_sage_primes(sage):
    for x, z in zip(sage["primes"]["X"], sage["primes"]["Z"]):
        assert ga.primes(x, _route="host") == z, x


def test_sage_two_argument_vectors(sage):
    for name, a, b in (("is_smooth", "N", "B"), ("is_powersmooth", "N", "B"), ("iroot", "X", "R"), ("ilog", "X", "B")):
        fn = getattr(ga, name)
        for x, y, z in zip(sage[name][a], sage[name][b], sage[name]["Z"]):
            got = fn(x, y)
            assert got == z and type(got) is type(z), (name, x, y, got, z)


# ---- the reference, live -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["totatives", "euler_phi", "mobius", "carmichael_lambda", "is_cyclic", "divisors", "divisor_sigma", "perfect_power",
                                  "trial_division"])
def test_reference_answers_up_to_200(ref, name):
    fn = getattr(ga, name)
    kwargs = {"_route": "host"} if name == "totatives" else {}
    for n, want in enumerate(ref["per_n"][name], start=1):
        assert _answer(fn, n, **kwargs) == want, (name, n)


def test_reference_primitive_roots_up_to_200(ref):
    for n in range(1, 201):
        assert list(ga.primitive_roots(n, _route="host")) == ref["per_n"]["primitive_roots"][n - 1], n
        assert list(ga.primitive_roots(n, reverse=True, _route="host")) == ref["per_n"]["primitive_roots_reversed"][n - 1], n
        roots = ref["per_n"]["primitive_roots"][n - 1]
        if n > 2:
            for g in range(1, n):
                assert ga.is_primitive_root(g, n) == (g in roots), (g, n)
        if roots:
            assert ga.primitive_root(n, _route="host") == roots[0] and ga.primitive_root(n, method="max", _route="host") == roots[-1]
            assert ga.primitive_root(n, method="random") in roots
    # the host chunks of the generator (64 candidates) across several chunk edges, both directions, with a window
    n = 2 * 7**5
    window = ref["misc"]["primitive_roots(2*7^5)[start, stop)"]
    assert list(ga.primitive_roots(n, start=1000, stop=1100, _route="host")) == window
    assert list(ga.primitive_roots(n, start=1000, stop=1100, reverse=True, _route="host")) == window[::-1]
    phi, exps = gi._phi_exponents(n)
    every = [g for g in range(1, 2000) if gi._is_root(g, n, phi, exps)]
    assert list(ga.primitive_roots(n, stop=2000, _route="host")) == every
    assert list(ga.primitive_roots(n, stop=2000, reverse=True, _route="host")) == every[::-1]
    assert ref["misc"]["primitive_roots(18, reverse)"] == [11, 5] == list(ga.primitive_roots(18, reverse=True, _route="host"))
    assert ref["misc"]["primitive_roots(4)"] == [3] == list(ga.primitive_roots(4, _route="host"))
    assert ref["misc"]["totatives(1)"] == [0] == ga.totatives(1)


def test_reference_primitive_root_of_large_moduli(ref):
    for n, method, want in ref["primitive_root"]:
        assert ga.primitive_root(n, method=method, _route="host") == want, (n, method)
    by = {(n, m): w for n, m, w in ref["primitive_root"]}
    assert by[(2**61 - 1, "min")] == 37 and by[(2 * 7**5, "max")] == 33605


def test_reference_symbols(ref):
    for a, n, want in ref["jacobi"]:
        assert _answer(ga.jacobi_symbol, a, n) == want, (a, n)
    for a, n, want in ref["kronecker"]:
        assert _answer(ga.kronecker_symbol, a, n) == want, (a, n)
    for a, p, want in ref["legendre"]:
        assert _answer(ga.legendre_symbol, a, p) == want, (a, p)
    assert len(ref["jacobi"]) > 200 and any(a < 0 for a, _, _ in ref["jacobi"]) and any(n < 0 for _, n, _ in ref["kronecker"])


def test_reference_pollard(ref):
    for (n, c), want in ref["pollard_rho"]:
        assert _answer(ga.pollard_rho, n, c=c) == want, (n, c)
    for (n, B, B2), want in ref["pollard_p1"]:
        assert _answer(ga.pollard_p1, n, B, B2=B2) == want, (n, B, B2)


def test_reference_rejections(ref):
    assert len(ref["errors"]) > 80
    for name, args, kwargs, kind, message in ref["errors"]:
        got = _answer(getattr(ga, name), *args, **kwargs)
        assert got == {"error": [kind, message]}, (name, args, kwargs, got)


def test_reference_single_values(ref):
    misc = ref["misc"]
    assert ga.kth_prime(664579) == misc["kth_prime(664579)"] == 9999991
    for n, want in misc["perfect_power"]:
        if n == -729:  # the reference answers (-6, 3), and (-6)^3 is -216: its step to an odd exponent doubles the base where it
            continue   # has to square it (for the base 2 the two agree)
        assert list(ga.perfect_power(n)) == want, n
    assert ga.perfect_power(-729) == (-9, 3) and (-9) ** 3 == -729
    for n in list(range(-300, 300)) + [2**64, 3**40, 6**12, -(2**63), 10**30, -(10**30), 12**35]:
        c, e = ga.perfect_power(n)
        assert c**e == n, n
        if n > 1:
            assert e == math.gcd(*nt.factors(n)[1]), n
    assert ga.mersenne_exponents(2000) == misc["mersenne_exponents(2000)"]
    assert ga.mersenne_primes(31) == [3, 7, 31, 127, 8191, 131071, 524287, 2147483647]
    assert len(ga.mersenne_exponents()) == 51 and all(ga.is_prime(e) for e in ga.mersenne_exponents())
    for values, want in misc["are_coprime"]:
        assert ga.are_coprime(*values) == want, values
    for n, want in misc["is_square_free"]:
        assert ga.is_square_free(n) == want, n


# ---- the rebinding of is_prime / primitive_root / is_primitive_root ---------------------------------------------------------------------
def test_rebinding_keeps_every_answer_for_primes_below_2000():
    ps = [p for p in range(2, 2000) if nt.is_prime(p)]
    assert len(ps) == 303
    for n in range(-5, 2000):
        assert ga.is_prime(n) == nt.is_prime(n)
    for p in ps:
        assert ga.primitive_root(p) == nt.primitive_root(p), p
        for g in range(1, p):
            assert ga.is_primitive_root(g, p) == nt.is_primitive_root(g, p), (g, p)
    # what the reference rejects now raises; composite moduli, answered before as if they were prime, are answered right
    with pytest.raises(ValueError):
        ga.is_primitive_root(0, 7)
    with pytest.raises(ValueError):
        ga.is_primitive_root(7, 7)
    assert nt.is_primitive_root(2, 9) is True and ga.is_primitive_root(2, 9) is True
    assert ga.is_primitive_root(3, 8) is False and ga.is_primitive_root(5, 18) is True
    for n in (2**61 - 1, 2**64 - 59, 1000000000000000035000061):
        assert ga.is_prime(n)
    for n in (561, 41041, 3215031751, 341550071728321, 3825123056546413051, 4294967291**2, 4294967291 * 4294967279, 2**64 - 1):
        assert not ga.is_prime(n) and ga.is_composite(n)


# ---- what has no fixture ------------------------------------------------------------------------------------------------------------------
def test_random_prime_properties():
    for bits in (1, 2, 8, 64, 200):
        for seed in (1, 2, 3):
            p = ga.random_prime(bits, seed=seed)
            assert 2**bits <= p < 2 ** (bits + 1) and ga.is_prime(p)
            assert ga.random_prime(bits, seed=seed) == p
    assert len({ga.random_prime(64, seed=s) for s in range(8)}) > 1
    state = random.getstate()
    ga.random_prime(64, seed=5)
    assert random.getstate() == state  # the global generator is left alone
    assert ga.is_prime(ga.random_prime(16))


def test_prime_walks_and_tests():
    small = ga.primes(10000, _route="host")
    assert small == [n for n in range(10001) if nt.is_prime(n)]
    assert ga.primes(1) == [] and ga.primes(2) == [2] and ga.primes(-3) == []
    for n in range(-3, 2000):
        assert ga.next_prime(n) == small[next(i for i, p in enumerate(small) if p > n)]
        if n >= 2:
            assert ga.prev_prime(n) == [p for p in small if p <= n][-1]
    assert ga.next_prime(2**64) == 2**64 + 13 and ga.prev_prime(2**64) == 2**64 - 59
    assert [ga.kth_prime(k) for k in (1, 2, 3, 1000)] == [2, 3, 5, 7919]
    for n in range(5, 400, 2):
        assert ga.miller_rabin_primality_test(n) == (nt.is_prime(n) or n == 2047), n  # no strong pseudoprime to 2 below 2047
        if n > 5:  # the later rounds use the bases 2, 3, 5, which must not be n itself
            assert ga.miller_rabin_primality_test(n, rounds=4) == nt.is_prime(n)
        assert ga.fermat_primality_test(n, a=2) == (nt.is_prime(n) or n == 341), n
        if nt.is_prime(n):
            assert ga.fermat_primality_test(n, rounds=3)
    assert ga.miller_rabin_primality_test(3) is True
    assert ga.miller_rabin_primality_test(3215031751, a=7, rounds=4) and not ga.miller_rabin_primality_test(3215031751, a=7, rounds=6)


def test_floors_at_large_arguments():
    for n in (0, 1, 2, 10**40, 2**200 - 1, 2**200, 2**200 + 1):
        r = ga.isqrt(n)
        assert r * r <= n < (r + 1) ** 2
        for k in (1, 2, 3, 7, 64):
            x = ga.iroot(n, k)
            assert x**k <= n < (x + 1) ** k, (n, k)
        if n:
            for b in (2, 3, 10, 2**70):
                k = ga.ilog(n, b)
                assert b**k <= n < b ** (k + 1), (n, b)


def test_divisor_functions_beyond_the_fixture():
    n = 2**5 * 3**3 * 101 * 1000003
    d = ga.divisors(n)
    assert len(d) == 6 * 4 * 2 * 2 and d[0] == 1 and d[-1] == n and all(n % x == 0 for x in d) and d == sorted(set(d))
    assert ga.divisors(-12) == [1, 2, 3, 4, 6, 12] and ga.divisors(0) == [] and ga.divisor_sigma(0) == 0
    assert ga.divisor_sigma(n, 0) == len(d) and ga.divisor_sigma(28) == 56 and ga.divisor_sigma(6, 2) == 50
    assert ga.euler_phi(n) == 2**4 * 3**2 * 2 * 100 * 1000002 and ga.mobius(2 * 3 * 5) == -1 and ga.mobius(n) == 0
    assert ga.carmichael_lambda(2**10) == 2**8 and ga.is_cyclic(2 * 3**40) and not ga.is_cyclic(4 * 3**40)
    assert ga.trial_division(n, B=100) == ([2, 3], [5, 3], 101 * 1000003)


# ---- the kernels' arithmetic on the host ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_integers_header_on_the_host(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "integers_host_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-I", os.path.join(repo_root, "galois_amd", "csrc"),
                    os.path.join(repo_root, "tests", "csrc", "integers_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "integers host model ok" in r.stdout, r.stdout + r.stderr
    # phi(phi(n)) roots for every n with a cyclic unit group that the powers serve (odd or twice odd)
    roots = sum(ga.euler_phi(ga.euler_phi(n)) for n in range(3, 2001) if n % 4 and ga.is_cyclic(n))
    for line in ("miller-rabin: 82025 primes below 2^20", "jacobi: 94 odd primes below 500", "sieve: 648 small windows",
                 f"units: {roots} primitive roots over the moduli up to 2000"):
        assert line in r.stdout, line
