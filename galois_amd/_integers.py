"""
Integer number theory: the reference's _prime.py, _math.py, _modular.py, _primitive_root.py and the integer halves of
_polymorphic.py (paths relative to the reference's src/galois), with its signatures, return types, argument checks and error
types, written from the mathematics.

Scalars are plain Python integers of any size and never launch a kernel.  The array-shaped work -- which the reference does one
integer at a time -- runs in galois_amd/csrc/gfa_integers.hip for values and moduli below 2^64:

  * is_prime_batched ............ gfa_int_is_prime: deterministic Miller-Rabin, one candidate per lane
  * primes_in_range, primes ..... gfa_int_sieve + gfa_int_sieve_expand: a segmented sieve of the odd numbers (stop <= 2^40), or
                                  gfa_int_is_prime over the odd candidates when the window is narrow or lies above 2^40
  * jacobi_symbol_batched ....... gfa_int_jacobi
  * totatives, primitive_roots, primitive_root, is_primitive_root_batched ... gfa_int_unit_classify over ranges of candidates,
                                  in chunks that grow geometrically for the searches (as galois_amd/_polysearch.py)

Every routed function takes a private `_route` ("host", "device" or None for the crossover) so that both routes can be run on
the same input.  The crossovers are tuning, not correctness; tools/bench_integers.py measures both routes.
"""
from __future__ import annotations

import bisect
import ctypes
import itertools
import math
import random

import numpy as np
import torch

from . import _lib as L
from . import _numtheory as nt

_TWO64 = 1 << 64
SIEVE_MAX_STOP = 1 << 40

# Crossovers between the host and device routes, measured on an MI355X with tools/bench_integers.py ("Integer number
# theory", has the figures).
PRIMES_DEVICE_FROM = 1 << 20      # primes(n): host 0.32 ms | device 0.34 ms at 2^18, 1.17 | 0.80 ms at 2^20 (the list's copy back dominates)
TOTATIVES_DEVICE_FROM = 1 << 12   # totatives(n): host 0.064 | device 0.104 ms at 2^10, 0.26 | 0.13 ms at 2^12, 4.3 | 0.64 ms at 2^16
SIEVE_WINDOW_FACTOR = 1           # primes_in_range: sieve when (stop - start) * this >= isqrt(stop), else test the candidates: below
                                  # 2^40 the two meet at a window of 2^20 (0.40 | 0.41 ms); narrower, the base primes cost more
ROOTS_HOST_CHUNK = 64             # primitive_roots: candidates tested on the host before the first launch (not tuned: a launch and
                                  # its read-back cost 0.1 ms, 64 host tests of a 64-bit modulus about as much)

_TEST_CHUNK = 1 << 24             # candidates per gfa_int_is_prime / gfa_int_unit_classify launch
_SIEVE_CHUNK = 1 << 32            # integers per sieve call: a bitmap of 256 MiB


def _verify_int(name: str, value, optional: bool = False, kind=int):
    """The reference's verify_isinstance(value, int) with its message (numpy integers are rejected, bools pass, as there)."""
    if optional and value is None:
        return
    if not isinstance(value, kind):
        raise TypeError(f"Argument {name!r} must be an instance of {kind}, not {type(value)}.")


def _verify_route(route):
    if route not in (None, "host", "device"):
        raise ValueError(f"Argument '_route' must be None, 'host' or 'device', not {route!r}.")


# ---- floors (_math.py) ------------------------------------------------------------------------------------------------------------
def isqrt(n: int) -> int:
    """galois.isqrt (_math.py:78-122): the largest x with x^2 <= n.  On every Python this package runs on the reference hands
    the call to math.isqrt, whose argument checks and messages are therefore the ones to keep."""
    return math.isqrt(n)


def iroot(n: int, k: int) -> int:
    """galois.iroot (_math.py:126-171): the largest x with x^k <= n."""
    _verify_int("n", n)
    _verify_int("k", k)
    if not n >= 0:
        raise ValueError(f"Argument 'n' must be non-negative, not {n}.")
    if not k >= 1:
        raise ValueError(f"Argument 'k' must be at least 1, not {k}.")
    if n < 2 or k == 1:
        return n
    lo, hi = 1, 1 << (n.bit_length() // k + 1)  # lo^k <= n < hi^k
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid**k <= n:
            lo = mid
        else:
            hi = mid
    return lo


def ilog(n: int, b: int) -> int:
    """galois.ilog (_math.py:175-222): the largest k with b^k <= n."""
    _verify_int("n", n)
    _verify_int("b", b)
    if not n > 0:
        raise ValueError(f"Argument 'n' must be positive, not {n}.")
    if not b >= 2:
        raise ValueError(f"Argument 'b' must be at least 2, not {b}.")
    k = max((n.bit_length() - 1) // b.bit_length(), 0)  # b < 2^bits(b), so b^k <= 2^(bits(n) - 1) <= n
    power = b**k
    while power * b <= n:
        power *= b
        k += 1
    return k


# ---- primes on the host -------------------------------------------------------------------------------------------------------------
def _host_sieve(n: int) -> np.ndarray:
    """The primes <= n as an int64 array: a sieve of the odd numbers, index i standing for 2 i + 1."""
    if n < 2:
        return np.zeros(0, dtype=np.int64)
    half = (n + 1) // 2  # odd numbers 1, 3, .., <= n
    alive = np.ones(half, dtype=bool)
    alive[0] = False
    for i in range(1, (math.isqrt(n) + 1) // 2):
        if alive[i]:
            p = 2 * i + 1
            alive[(p * p) // 2::p] = False
    out = 2 * np.flatnonzero(alive).astype(np.int64) + 1
    return np.concatenate((np.array([2], dtype=np.int64), out))


KTH_PRIME_LIMIT = 10_000_000
_TABLE: list | None = None          # the primes <= KTH_PRIME_LIMIT, built on first use
_SMALL: np.ndarray = np.zeros(0, dtype=np.int64)  # a growing prefix of the primes for the routines that walk them
_SMALL_LIMIT = 0


def _prime_table() -> list:
    global _TABLE
    if _TABLE is None:
        _TABLE = _host_sieve(KTH_PRIME_LIMIT).tolist()
    return _TABLE


def _small_primes(n: int) -> np.ndarray:
    """The primes <= n from a cache that doubles; for trial division, base primes and the smoothness tests."""
    global _SMALL, _SMALL_LIMIT
    if n > _SMALL_LIMIT:
        _SMALL_LIMIT = max(n, 2 * _SMALL_LIMIT, 1 << 12)
        _SMALL = _host_sieve(_SMALL_LIMIT)
    return _SMALL[: int(np.searchsorted(_SMALL, n, side="right"))]


def primes(n: int, _route=None) -> list:
    """galois.primes (_prime.py:31-97): all primes <= n, ascending.  Large n runs the device sieve (primes_in_range)."""
    _verify_int("n", n)
    _verify_route(_route)
    if n < 2:
        return []
    if _route == "device" or (_route is None and PRIMES_DEVICE_FROM <= n < _TWO64):
        return primes_in_range(0, n + 1).tolist()
    return _host_sieve(n).tolist()


def kth_prime(k: int) -> int:
    """galois.kth_prime (_prime.py:108-139): the k-th prime, 1-based, from the table of the 664579 primes up to 10^7 (built on first
    use)."""
    _verify_int("k", k)
    table_size = 664579  # pi(10^7)
    if not 1 <= k <= table_size:
        raise ValueError(
            f"Argument 'k' is out of range of the prime lookup table. "
            f"The lookup table only contains the first {table_size} primes (up to {KTH_PRIME_LIMIT})."
        )
    return _prime_table()[k - 1]


_WHEEL = (1, 7, 11, 13, 17, 19, 23, 29)  # the residues modulo 30 coprime to 2, 3 and 5


def is_prime(n: int) -> bool:
    """galois.is_prime (_prime.py:1401-1458).  Miller-Rabin: deterministic below 3.3e24 (the first thirteen primes as bases),
    with 24 further bases drawn from n itself above."""
    _verify_int("n", n)
    return nt.is_prime(n)


def prev_prime(n: int) -> int:
    """galois.prev_prime (_prime.py:143-184): the nearest prime p <= n."""
    _verify_int("n", n)
    if not n >= 2:
        raise ValueError("There are no primes less than 2.")
    if n < 7:
        return (2, 3, 3, 5, 5)[n - 2]
    base = n // 30 * 30
    while True:
        for shift in reversed(_WHEEL):
            if base + shift <= n and nt.is_prime(base + shift):
                return base + shift
        base -= 30


def next_prime(n: int) -> int:
    """galois.next_prime (_prime.py:188-227): the nearest prime p > n."""
    _verify_int("n", n)
    if n < 7:
        return 2 if n < 2 else (3, 5, 5, 7, 7)[n - 2]
    base = n // 30 * 30
    while True:
        for shift in _WHEEL:
            if base + shift > n and nt.is_prime(base + shift):
                return base + shift
        base += 30


def random_prime(bits: int, seed: int | None = None) -> int:
    """galois.random_prime (_prime.py:231-282): a prime in [2^bits, 2^(bits + 1)), the same one for the same seed.

    The value for a given seed is NOT the reference's: there the candidates come from the global generator, and is_prime draws
    from the same generator between two candidates (its Fermat test picks a random base), so the sequence depends on the
    reference's own test.  Here the candidates come from a private random.Random(seed) and the global generator is untouched."""
    _verify_int("bits", bits)
    _verify_int("seed", seed, optional=True)
    if not bits > 0:
        raise ValueError(f"Argument 'bits' must be positive, not {bits}.")
    rnd = random.Random(seed)
    while True:
        p = rnd.randint(2**bits, 2 ** (bits + 1) - 1)
        if nt.is_prime(p):
            return p


# The exponents e of the known Mersenne primes 2^e - 1, from the published list of the Great Internet Mersenne Prime Search
# (https://www.mersenne.org/primes/, OEIS A000043) up to the 2018 discovery -- the reference's cut.
_MERSENNE_EXPONENTS = (
    2, 3, 5, 7, 13, 17, 19, 31, 61, 89, 107, 127, 521, 607, 1279, 2203, 2281, 3217, 4253, 4423, 9689, 9941, 11213, 19937, 21701, 23209,
    44497, 86243, 110503, 132049, 216091, 756839, 859433, 1257787, 1398269, 2976221, 3021377, 6972593, 13466917, 20996011, 24036583,
    25964951, 30402457, 32582657, 37156667, 42643801, 43112609, 57885161, 74207281, 77232917, 82589933,
)


def mersenne_exponents(n: int | None = None) -> list:
    """galois.mersenne_exponents (_prime.py:342-381): the known exponents e <= n with 2^e - 1 prime (all of them for n = None)."""
    if n is None:
        return list(_MERSENNE_EXPONENTS)
    _verify_int("n", n)
    if not n > 0:
        raise ValueError(f"Argument 'n' must be positive, not {n}.")
    return list(_MERSENNE_EXPONENTS[: bisect.bisect_right(_MERSENNE_EXPONENTS, n)])


def mersenne_primes(n: int | None = None) -> list:
    """galois.mersenne_primes (_prime.py:385-414): the known Mersenne primes p <= 2^n - 1."""
    return [2**e - 1 for e in mersenne_exponents(n)]


# ---- primality tests with a chosen base -------------------------------------------------------------------------------------------
def fermat_primality_test(n: int, a: int | None = None, rounds: int = 1) -> bool:
    """galois.fermat_primality_test (_prime.py:423-511): False when a^(n - 1) != 1 (mod n) proves n composite; the rounds after
    the first draw their bases at random."""
    _verify_int("n", n)
    _verify_int("a", a, optional=True)
    _verify_int("rounds", rounds)
    if not (n > 2 and n % 2 == 1):
        raise ValueError(f"Argument 'n' must be odd and greater than 2, not {n}.")
    if a is None:
        a = random.randint(2, max(n - 2, 2))
    if not 2 <= a <= n - 2:
        raise ValueError(f"Argument 'a' must satisfy 2 <= a <= {n - 2}, not {a}.")
    if not rounds >= 1:
        raise ValueError(f"Argument 'rounds' must be at least 1, not {rounds}.")
    for _ in range(rounds):
        if pow(a, n - 1, n) != 1:
            return False
        a = random.randint(2, n - 2)
    return True


def miller_rabin_primality_test(n: int, a: int = 2, rounds: int = 1) -> bool:
    """galois.miller_rabin_primality_test (_prime.py:515-616): the strong test to base a, then to the primes 2, 3, 5, .. for the
    rounds after the first."""
    _verify_int("n", n)
    _verify_int("a", a)
    _verify_int("rounds", rounds)
    if n == 3:
        return True
    if not (n > 2 and n % 2 == 1):
        raise ValueError(f"Argument 'n' must be odd and greater than 2, not {n}.")
    if not 2 <= a <= n - 2:
        raise ValueError(f"Argument 'a' must satisfy 2 <= a <= {n - 2}, not {a}.")
    if not rounds >= 1:
        raise ValueError(f"Argument 'rounds' must be at least 1, not {rounds}.")
    s = ((n - 1) & -(n - 1)).bit_length() - 1
    d = (n - 1) >> s
    later = iter(_small_primes(max(64, 20 * rounds)).tolist())  # the k-th prime is below 20 k for every k that can be run
    for _ in range(rounds):
        x = pow(a, d, n)
        if x != 1 and x != n - 1:
            for _ in range(s - 1):
                x = x * x % n
                if x == n - 1:
                    break
            else:
                return False
        a = next(later)
    return True


# ---- quadratic-residue symbols -----------------------------------------------------------------------------------------------------
def _jacobi(a: int, n: int) -> int:
    """(a / n) for odd n >= 3 by quadratic reciprocity."""
    a %= n
    t = 1
    while a:
        z = (a & -a).bit_length() - 1
        a >>= z
        if z & 1 and n & 7 in (3, 5):
            t = -t
        if a & 3 == 3 and n & 3 == 3:
            t = -t
        a, n = n % a, a
    return t if n == 1 else 0


def legendre_symbol(a: int, p: int) -> int:
    """galois.legendre_symbol (_prime.py:625-675): 1 when a is a non-zero square modulo the odd prime p, -1 when it is a
    non-square, 0 when p | a."""
    _verify_int("a", a)
    _verify_int("p", p)
    if not (p > 2 and nt.is_prime(p)):
        raise ValueError(f"Argument 'p' must be an odd prime greater than 2, not {p}.")
    return _jacobi(a, p)


def jacobi_symbol(a: int, n: int) -> int:
    """galois.jacobi_symbol (_prime.py:679-748): the product of the Legendre symbols of a over the prime factors of odd n >= 3."""
    _verify_int("a", a)
    _verify_int("n", n)
    if not (n > 2 and n % 2 == 1):
        raise ValueError(f"Argument 'n' must be an odd integer greater than 2, not {n}.")
    return _jacobi(a, n)


def kronecker_symbol(a: int, n: int) -> int:
    """galois.kronecker_symbol (_prime.py:752-803): the Jacobi symbol extended to every integer n through (a / -1), (a / 2) and
    (a / 0)."""
    _verify_int("a", a)
    _verify_int("n", n)
    if n == 0:
        return 1 if a in (1, -1) else 0
    sign = -1 if (n < 0 and a < 0) else 1
    n = abs(n)
    e = (n & -n).bit_length() - 1
    n >>= e
    if e:
        if a % 2 == 0:
            return 0
        if e & 1 and a % 8 in (3, 5):
            sign = -sign
    return sign * (_jacobi(a, n) if n >= 3 else 1)


# ---- factoring ---------------------------------------------------------------------------------------------------------------------
def perfect_power(n: int) -> tuple:
    """galois.perfect_power (_prime.py:895-991): (c, e) with n = c^e and e as large as possible; (n, 1) when n is no perfect power.
    A negative n needs an odd exponent: with |n| = c^e and e = 2^k o, o odd, the answer is (-(c^(2^k)), o) when o > 1."""
    _verify_int("n", n)
    if n == 0:
        return 0, 1
    size = abs(n)
    if size == 1:
        # the reference's search starts at the base 2: 1 = 2^0, and -1 is left alone
        return (2, 0) if n > 0 else (n, 1)
    base, exponent = size, 1
    k = 2
    while k <= base.bit_length():  # a k-th root of at least 2 needs k <= log2(base); prime k suffice
        x = iroot(base, k)
        if x**k == base:
            base, exponent = x, exponent * k
        else:
            k = k + 1 if k == 2 else k + 2
            while any(k % r == 0 for r in range(3, math.isqrt(k) + 1, 2)):
                k += 2
    if n > 0:
        return base, exponent
    while exponent % 2 == 0:
        base, exponent = base * base, exponent // 2
    return (-base, exponent) if exponent > 1 else (n, 1)


def trial_division(n: int, B: int | None = None) -> tuple:
    """galois.trial_division (_prime.py:1015-1071): (p, e, residual) with n = residual prod p_i^e_i over the primes p_i <= B that
    divide n; B defaults to, and is capped at, isqrt(n)."""
    _verify_int("n", n)
    _verify_int("B", B, optional=True)
    if not n > 1:
        raise ValueError(f"Argument 'n' must be greater than 1, not {n}.")
    B = math.isqrt(n) if B is None else B
    if not B > 2:
        raise ValueError(f"Argument 'B' must be greater than 2, not {B}.")
    B = min(math.isqrt(n), B)
    p, e = [], []
    for prime in _small_primes(B).tolist():
        if n % prime == 0:
            degree = 0
            while n % prime == 0:
                degree += 1
                n //= prime
            p.append(prime)
            e.append(degree)
            if n == 1:
                break
    return p, e, n


def pollard_p1(n: int, B: int, B2: int | None = None) -> int:
    """galois.pollard_p1 (_prime.py:1075-1198): a non-trivial factor of odd n by Pollard's p - 1 method with smoothness bound B
    and, optionally, one further prime in (B, B2].  The gcd is looked at after every tenth prime, as in the reference, so the
    factor found is the same."""
    _verify_int("n", n)
    _verify_int("B", B)
    _verify_int("B2", B2, optional=True)
    if not (n % 2 == 1 and n > 2):
        raise ValueError(f"Argument 'n' must be odd and greater than 2, not {n}.")
    if not B > 2:
        raise ValueError(f"Argument 'B' must be greater than 2, not {B}.")
    failure = RuntimeError(
        f"A non-trivial factor of {n} could not be found using the Pollard p-1 algorithm "
        f"with smoothness bound {B} and secondary bound {B2}."
    )
    a = 2
    for i, p in enumerate(_small_primes(B).tolist()):
        a = pow(a, p ** ilog(n, p), n)
        if i % 10 == 0:
            d = math.gcd(a - 1, n)
            if d not in (1, n):
                return d
    d = math.gcd(a - 1, n)
    if d not in (1, n):
        return d
    if d == n:
        raise failure
    if B2 is not None:
        for i, p in enumerate(q for q in _small_primes(B2).tolist() if q > B):
            a = pow(a, p, n)
            if i % 10 == 0:
                d = math.gcd(a - 1, n)
                if d not in (1, n):
                    return d
        d = math.gcd(a - 1, n)
        if d not in (1, n):
            return d
    raise failure


def pollard_rho(n: int, c: int = 1) -> int:
    """galois.pollard_rho (_prime.py:1203-1273): a non-trivial factor of n from Floyd's cycle search on x -> x^2 + c, started at
    2."""
    _verify_int("n", n)
    _verify_int("c", c)
    if not n > 1:
        raise ValueError(f"Argument 'n' must be greater than 1, not {n}.")
    if c in (0, -2):
        raise ValueError("Argument 'c' cannot be -2 or 0.")
    slow = fast = 2
    d = 1
    while d == 1:
        slow = (slow * slow + c) % n
        fast = (fast * fast + c) % n
        fast = (fast * fast + c) % n
        d = math.gcd(abs(slow - fast), n)
    if d == n:
        raise RuntimeError(f"A non-trivial factor of {n} could not be found using the Pollard Rho algorithm with f(x) = x^2 + {c}.")
    return d


def divisors(n: int) -> list:
    """galois.divisors (_prime.py:1292-1350): the positive divisors of n, ascending ([] for 0)."""
    _verify_int("n", n)
    n = abs(n)
    if n == 0:
        return []
    out = [1]
    if n > 1:
        for p, e in zip(*nt.factors(n)):
            out = [d * p**j for d in out for j in range(e + 1)]
    return sorted(out)


def divisor_sigma(n: int, k: int = 1) -> int:
    """galois.divisor_sigma (_prime.py:1354-1392): the sum of the k-th powers of the positive divisors of n."""
    _verify_int("n", n)
    d = divisors(n)
    if n == 0:
        return len(d)
    return sum(di**k for di in d)


# ---- tests of one integer ------------------------------------------------------------------------------------------------------------
def is_composite(n: int) -> bool:
    """galois.is_composite (_prime.py:1462-1489)."""
    _verify_int("n", n)
    return n >= 2 and not nt.is_prime(n)


def is_prime_power(n: int) -> bool:
    """galois.is_prime_power (_prime.py:1493-1531): n = p^k for a prime p and k >= 1."""
    _verify_int("n", n)
    if n < 2:
        return False
    return nt.is_prime(n) or nt.is_prime(perfect_power(n)[0])


def is_perfect_power(n: int) -> bool:
    """galois.is_perfect_power (_prime.py:1535-1602): n = c^e with e > 1; -1, 0 and 1 count."""
    _verify_int("n", n)
    if n in (-1, 0, 1):
        return True
    return perfect_power(n)[0] != n


def _int_is_square_free(n: int) -> bool:
    n = abs(n)
    if n == 0:
        return False
    if n == 1:
        return True
    return all(e == 1 for e in nt.factors(n)[1])


def is_smooth(n: int, B: int) -> bool:
    """galois.is_smooth (_prime.py:1624-1678): every prime factor of n is at most B."""
    _verify_int("n", n)
    _verify_int("B", B)
    if not B >= 2:
        raise ValueError(f"Argument 'B' must be at least 2, not {B}.")
    n = abs(n)
    if n == 0:
        return False
    for p in _small_primes(B).tolist():
        if n == 1:
            break
        while n % p == 0:
            n //= p
    return n == 1


def is_powersmooth(n: int, B: int) -> bool:
    """galois.is_powersmooth (_prime.py:1682-1742): every prime power p^e that divides n exactly is at most B."""
    _verify_int("n", n)
    _verify_int("B", B)
    if not B >= 2:
        raise ValueError(f"Argument 'B' must be at least 2, not {B}.")
    n = abs(n)
    if n == 0:
        return False
    for p in _small_primes(B).tolist():
        if n == 1:
            break
        power = 1
        while n % p == 0:
            n //= p
            power *= p
        if power > B:
            return False
    return n == 1


# ---- the unit group (_modular.py) --------------------------------------------------------------------------------------------------
def _verify_modulus(n):
    _verify_int("n", n)
    if not n > 0:
        raise ValueError(f"Argument 'n' must be a positive integer, not {n}.")


def euler_phi(n: int) -> int:
    """galois.euler_phi (_modular.py:86-197): the number of residues coprime to n; phi(1) = 1."""
    _verify_modulus(n)
    if n == 1:
        return 1
    phi = 1
    for p, e in zip(*nt.factors(n)):
        phi *= p ** (e - 1) * (p - 1)
    return phi


def mobius(n: int) -> int:
    """galois.mobius (_modular.py:201-328): 0 when a square divides n, else (-1)^(number of prime factors)."""
    _verify_modulus(n)
    if n == 1:
        return 1
    p, e = nt.factors(n)
    if any(ei > 1 for ei in e):
        return 0
    return -1 if len(p) % 2 else 1


def carmichael_lambda(n: int) -> int:
    """galois.carmichael_lambda (_modular.py:332-471): the exponent of the unit group modulo n."""
    _verify_modulus(n)
    if n == 1:
        return 1
    parts = []
    for p, e in zip(*nt.factors(n)):
        phi = p ** (e - 1) * (p - 1)
        parts.append(phi // 2 if (p == 2 and e > 2) else phi)
    return math.lcm(*parts)


def is_cyclic(n: int) -> bool:
    """galois.is_cyclic (_modular.py:475-673): the unit group modulo n is cyclic -- n is 1, 2, 4, p^k or 2 p^k for an odd prime p."""
    _verify_modulus(n)
    if n in (1, 2, 4):
        return True
    if n % 4 == 0:
        return False
    odd = n // 2 if n % 2 == 0 else n
    return len(nt.factors(odd)[0]) == 1


def totatives(n: int, _route=None) -> list:
    """galois.totatives (_modular.py:16-82): the t in [1, n) coprime to n ([0] for n = 1).  Large n keeps the unit flags of
    gfa_int_unit_classify over 1 .. n - 1."""
    _verify_modulus(n)
    _verify_route(_route)
    if n == 1:
        return [0]
    if n < _TWO64 and (_route == "device" or (_route is None and n >= TOTATIVES_DEVICE_FROM)):
        out = []
        for k0 in range(1, n, _TEST_CHUNK):
            count = min(_TEST_CHUNK, n - k0)
            idx = torch.nonzero(_classify_range(n, k0, 1, count, ()) & 1).reshape(-1).tolist()
            out.extend(k0 + i for i in idx)
        return out
    return [t for t in range(1, n) if math.gcd(n, t) == 1]


# ---- primitive roots (_primitive_root.py) ------------------------------------------------------------------------------------------
def _phi_exponents(n: int) -> tuple:
    """phi(n) and phi(n) / r for the primes r | phi(n)."""
    phi = euler_phi(n)
    return phi, tuple(phi // r for r in nt.factors(phi)[0]) if phi > 1 else ()


def _is_root(g: int, n: int, phi: int, exps: tuple) -> bool:
    if n == 2:
        return g == 1
    return pow(g, phi, n) == 1 and all(pow(g, e, n) != 1 for e in exps)


def is_primitive_root(g: int, n: int) -> bool:
    """galois.is_primitive_root (_primitive_root.py:18-116): does g generate the unit group modulo n?  Any n >= 1; 1 is the root
    modulo 2."""
    _verify_int("g", g)
    _verify_int("n", n)
    if not n > 0:
        raise ValueError(f"Argument 'n' must be a positive integer, not {n}.")
    if not 0 < g < n:
        raise ValueError(f"Argument 'g' must be a positive integer less than 'n', not {g}.")
    return _is_root(g, n, *_phi_exponents(n))


def _device_serves(n: int) -> bool:
    """Moduli gfa_int_unit_classify raises powers under: below 2^64, odd or twice an odd number."""
    return n < _TWO64 and n % 4 != 0


def primitive_roots(n: int, start: int = 1, stop: int | None = None, reverse: bool = False, _route=None):
    """galois.primitive_roots (_primitive_root.py:319-453): a generator of the primitive roots modulo n in [start, stop), ascending
    (descending with reverse).  n = 1 yields 0 and n = 2 yields 1.  A first short run of candidates is tested on the host, so the
    first next() stays cheap; after it, chunks of candidates that grow geometrically go through gfa_int_unit_classify.  For even n
    only odd candidates are looked at."""
    _verify_int("n", n)
    _verify_int("start", start)
    _verify_int("stop", stop, optional=True)
    _verify_int("reverse", reverse, kind=bool)
    _verify_route(_route)
    if n in (1, 2):
        yield n - 1
        return
    stop = n if stop is None else stop
    if not 1 <= start < stop <= n:
        raise ValueError(f"Arguments must satisfy 1 <= start < stop <= n, not 1 <= {start} < {stop} <= {n}.")
    if not is_cyclic(n):
        return
    phi, exps = _phi_exponents(n)
    step = 1
    if n % 2 == 0:
        start += 1 - start % 2
        step = 2
    total = max(0, (stop - start + step - 1) // step)  # candidates start, start + step, ..
    device = _route == "device" or (_route is None and _device_serves(n))
    if device and not _device_serves(n):
        raise NotImplementedError(f"gfa_int_unit_classify does not serve the modulus {n}.")
    done, chunk = 0, (256 if _route == "device" else ROOTS_HOST_CHUNK)
    while done < total:
        count = min(chunk, total - done)
        first = start + step * (total - done - count if reverse else done)
        if device and (done > 0 or _route == "device"):
            hits = torch.nonzero(_classify_range(n, first, step, count, exps) & 2).reshape(-1).tolist()
            roots = [first + step * i for i in hits]
        else:
            roots = [g for g in range(first, first + step * count, step) if _is_root(g, n, phi, exps)]
        yield from (reversed(roots) if reverse else roots)
        done += count
        chunk = min(4 * chunk, 1 << 20) if device else chunk
    return


def primitive_root(n: int, start: int = 1, stop: int | None = None, method: str = "min", _route=None) -> int:
    """galois.primitive_root (_primitive_root.py:120-315): the smallest ("min"), largest ("max") or a random primitive root modulo
    n in [start, stop).  0 for n = 1 and 1 for n = 2; RuntimeError when the range holds none."""
    _verify_int("n", n)
    _verify_int("start", start)
    _verify_int("stop", stop, optional=True)
    if n in (1, 2):
        return n - 1
    stop = n if stop is None else stop
    if not 1 <= start < stop <= n:
        raise ValueError(f"Arguments must satisfy 1 <= start < stop <= n, not 1 <= {start} < {stop} <= {n}.")
    if method not in ["min", "max", "random"]:
        raise ValueError(f"Argument 'method' must be in ['min', 'max', 'random'], not {method!r}.")
    if method in ("min", "max"):
        for root in primitive_roots(n, start, stop, reverse=method == "max", _route=_route):
            return root
    elif is_cyclic(n):
        phi, exps = _phi_exponents(n)
        for _ in range(2 * (stop - start) + 1):
            g = random.randint(start, stop - 1)
            if _is_root(g, n, phi, exps):
                return g
        # unlucky, or a range without roots: look at all of it, so that the error below is raised only when it is true
        roots = list(primitive_roots(n, start, stop, _route=_route))
        if roots:
            return random.choice(roots)
    raise RuntimeError(f"No primitive roots modulo {n} exist in the range [{start}, {stop}).")


# ---- ints or polynomials (_polymorphic.py) -----------------------------------------------------------------------------------------
def _all_ints(values) -> bool:
    return all(isinstance(v, (int, np.integer)) for v in values)


def are_coprime(*values) -> bool:
    """galois.are_coprime (_polymorphic.py:313-370): do the integers, or the polynomials, share no factor pairwise -- is their
    least common multiple their product?"""
    from ._poly import Poly
    from ._polygcd import lcm, prod

    if not (_all_ints(values) or all(isinstance(v, Poly) for v in values)):
        raise TypeError(f"All arguments must be either int or galois.Poly, not {[type(value) for value in values]}.")
    if not len(values) > 0:
        raise ValueError("At least one argument must be provided.")
    return lcm(*values) == prod(*values)


def is_square_free(value) -> bool:
    """galois.is_square_free (_polymorphic.py:652-720): no square of a prime (of an irreducible polynomial) divides the value."""
    from ._poly import Poly

    if isinstance(value, (int, np.integer)):
        return _int_is_square_free(int(value))
    if isinstance(value, Poly):
        return value.is_square_free()
    raise TypeError(f"Argument 'value' must be either int or Poly, not {type(value)}.")


# ---- the device forms ----------------------------------------------------------------------------------------------------------------
def _u64_tensor(values, name: str) -> torch.Tensor:
    """A contiguous 1-D device tensor of 64-bit patterns (int64 storage) of integers in [0, 2^64)."""
    from ._array import _device

    if isinstance(values, torch.Tensor):
        if values.dtype not in (torch.int64, torch.uint64):
            raise TypeError(f"Argument {name!r} must be a uint64 or int64 tensor, not {values.dtype}.")
        t = values.view(torch.int64) if values.dtype == torch.uint64 else values
        return t.reshape(-1).contiguous().to(_device())
    arr = values if isinstance(values, np.ndarray) else np.array(list(values), dtype=object)
    if arr.dtype == object or arr.size == 0:
        ints = [int(v) for v in arr.reshape(-1).tolist()]
        if any(not 0 <= v < _TWO64 for v in ints):
            raise ValueError(f"Argument {name!r} must hold integers in [0, 2^64).")
        arr = np.array(ints, dtype=np.uint64)
    elif arr.dtype.kind == "i":
        if arr.size and arr.min() < 0:
            raise ValueError(f"Argument {name!r} must hold integers in [0, 2^64).")
        arr = arr.astype(np.uint64)
    elif arr.dtype.kind in "ub":
        arr = arr.astype(np.uint64)
    else:
        raise TypeError(f"Argument {name!r} must hold integers, not {arr.dtype}.")
    return torch.from_numpy(np.ascontiguousarray(arr.reshape(-1)).view(np.int64)).to(_device())


def _range_args(r: range, name: str) -> tuple:
    if len(r) and not (r.step > 0 and 0 <= r.start < _TWO64 and r.step < _TWO64):
        raise ValueError(f"Argument {name!r} as a range must ascend from a start in [0, 2^64).")
    return (r.start, r.step, len(r)) if len(r) else (0, 1, 0)


def _is_prime_range(start: int, step: int, count: int) -> torch.Tensor:
    from ._array import _device, _ptr, _stream

    flags = torch.empty(count, dtype=torch.uint8, device=_device())
    L.check(L.lib().gfa_int_is_prime(None, count, start, step, _ptr(flags), _stream()), "gfa_int_is_prime")
    return flags


def is_prime_batched(values) -> np.ndarray:
    """Device extension: is_prime of every integer of an array-like of Python ints below 2^64, of a uint64 / int64 tensor (64-bit
    patterns), or of a `range`, whose candidates start + i step are formed in the kernel and never stored.  Returns a NumPy bool
    array.  Deterministic Miller-Rabin, exact below 2^64."""
    from ._array import _ptr, _stream

    if isinstance(values, range):
        flags = _is_prime_range(*_range_args(values, "values"))
    else:
        t = _u64_tensor(values, "values")
        flags = torch.empty(t.numel(), dtype=torch.uint8, device=t.device)
        L.check(L.lib().gfa_int_is_prime(_ptr(t), t.numel(), 0, 0, _ptr(flags), _stream()), "gfa_int_is_prime")
    return flags.cpu().numpy().astype(bool)


def sieve_segment_span() -> int:
    """The integers one workgroup of the device sieve owns."""
    return int(L.lib().gfa_int_sieve_segment_span())


_BASE_PRIMES: dict = {}


def _base_primes(limit: int) -> torch.Tensor:
    """The odd primes <= limit as uint32 patterns on the device, kept per power-of-two ceiling of the limit."""
    from ._array import _device

    dev = _device()
    key = (dev, max(limit, 2).bit_length())
    if key not in _BASE_PRIMES:
        if len(_BASE_PRIMES) > 64:
            _BASE_PRIMES.clear()
        p = _small_primes((1 << key[1]) - 1)[1:].astype(np.uint32)
        _BASE_PRIMES[key] = (p, torch.from_numpy(p.view(np.int32).copy()).to(dev))
    host, t = _BASE_PRIMES[key]
    return t[: int(np.searchsorted(host, limit, side="right"))]


def _to_i64(v: int) -> int:
    return v - _TWO64 if v >= 1 << 63 else v


def _sieve_window(start: int, stop: int) -> torch.Tensor:
    from ._array import _device, _ptr, _stream

    dev = _device()
    first_odd = start | 1
    bits = (stop - first_odd + 1) // 2 if stop > first_odd else 0
    has_two = 1 if start <= 2 < stop else 0
    if bits == 0:
        return torch.full((has_two,), 2, dtype=torch.int64, device=dev)
    segments = -(-2 * bits // sieve_segment_span())
    base = _base_primes(math.isqrt(stop - 1))
    bitmap = torch.empty((bits + 31) // 32, dtype=torch.int32, device=dev)
    counts = torch.empty(segments, dtype=torch.int64, device=dev)
    lib, st = L.lib(), _stream()
    L.check(lib.gfa_int_sieve(start, stop, _ptr(base) if base.numel() else None, base.numel(), _ptr(bitmap), _ptr(counts), st), "gfa_int_sieve")
    ends = torch.cumsum(counts, 0)
    total = int(ends[-1].item()) + has_two  # the one read-back
    offsets = (ends - counts + has_two).contiguous()
    out = torch.empty(total, dtype=torch.int64, device=dev)
    if total == 0:
        return out
    L.check(lib.gfa_int_sieve_expand(start, stop, _ptr(bitmap), _ptr(offsets), _ptr(out), st), "gfa_int_sieve_expand")
    return out


def _test_window(start: int, stop: int) -> torch.Tensor:
    """The primes of [start, stop) from gfa_int_is_prime over the odd candidates; only flags and primes reach memory."""
    from ._array import _device

    dev = _device()
    parts = [torch.full((1,), 2, dtype=torch.int64, device=dev)] if start <= 2 < stop else []
    first_odd = start | 1
    total = (stop - first_odd + 1) // 2 if stop > first_odd else 0
    for k0 in range(0, total, _TEST_CHUNK):
        count = min(_TEST_CHUNK, total - k0)
        first = first_odd + 2 * k0
        idx = torch.nonzero(_is_prime_range(first, 2, count)).reshape(-1)
        parts.append(idx * 2 + _to_i64(first))  # int64 arithmetic wraps: the 64-bit pattern of first + 2 idx
    return torch.cat(parts) if parts else torch.empty(0, dtype=torch.int64, device=dev)


def primes_in_range(start: int, stop: int, _route=None) -> torch.Tensor:
    """Device extension: the primes of [start, stop), 0 <= start <= stop <= 2^64, increasing, as an int64 tensor on the device
    (64-bit patterns for values from 2^63 on, as elsewhere in the package).  Up to stop = 2^40 a segmented sieve of the odd numbers
    runs (`_route="sieve"`), unless the window is narrow compared with sqrt(stop); then, and above 2^40, the odd candidates go
    through the primality kernel (`_route="test"`).  The candidates never exist as an array: only the bitmap (or the flags) and
    the primes do."""
    _verify_int("start", start)
    _verify_int("stop", stop)
    if _route not in (None, "sieve", "test"):
        raise ValueError(f"Argument '_route' must be None, 'sieve' or 'test', not {_route!r}.")
    if not 0 <= start <= stop <= _TWO64:
        raise ValueError(f"Arguments must satisfy 0 <= start <= stop <= 2^64, not 0 <= {start} <= {stop}.")
    if _route == "sieve" and stop > SIEVE_MAX_STOP:
        raise ValueError(f"The sieve serves windows up to 2^40, not {stop}.")
    sieve = _route == "sieve" or (_route is None and stop <= SIEVE_MAX_STOP and (stop - start) * SIEVE_WINDOW_FACTOR >= math.isqrt(stop))
    if not sieve:
        return _test_window(start, stop)
    parts = [_sieve_window(lo, min(lo + _SIEVE_CHUNK, stop)) for lo in range(start, max(stop, start + 1), _SIEVE_CHUNK)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def jacobi_symbol_batched(a, n) -> np.ndarray:
    """Device extension: jacobi_symbol(a[i], n) for one odd n >= 3, or jacobi_symbol(a[i], n[i]) for an array-like n of the same
    length; a int8 NumPy array.  a holds Python ints (or an int64 array / tensor).  Values of a outside the int64 range, and moduli
    from 2^64 on, are answered on the host."""
    from ._array import _device, _ptr, _stream

    shared = isinstance(n, (int, np.integer)) and not isinstance(n, bool)
    a_list = a.reshape(-1).tolist() if isinstance(a, (torch.Tensor, np.ndarray)) else [int(v) for v in a]
    n_list = [int(n)] if shared else (n.reshape(-1).tolist() if isinstance(n, (torch.Tensor, np.ndarray)) else [int(v) for v in n])
    if isinstance(n, torch.Tensor) and n.dtype in (torch.int64, torch.uint64):
        n_list = [v % _TWO64 for v in n_list]
    for m in n_list:
        if not (m > 2 and m % 2 == 1):
            raise ValueError(f"Argument 'n' must be an odd integer greater than 2, not {m}.")
    if not shared and len(n_list) != len(a_list):
        raise ValueError(f"Arguments 'a' and 'n' must have the same length, not {len(a_list)} and {len(n_list)}.")
    if any(m >= _TWO64 for m in n_list) or any(not -(1 << 63) <= v < 1 << 63 for v in a_list):
        return np.array([_jacobi(v, n_list[0] if shared else n_list[i]) for i, v in enumerate(a_list)], dtype=np.int8)
    dev = _device()
    a_t = torch.tensor(a_list, dtype=torch.int64, device=dev)
    out = torch.empty(len(a_list), dtype=torch.int8, device=dev)
    if shared:
        n_arg, keep = ctypes.c_uint64(n_list[0]), None
        n_ptr = ctypes.addressof(n_arg)  # one modulus: an argument in host memory
    else:
        keep = torch.from_numpy(np.array(n_list, dtype=np.uint64).view(np.int64)).to(dev)
        n_ptr = _ptr(keep)
    L.check(L.lib().gfa_int_jacobi(_ptr(a_t), n_ptr, len(a_list), 0 if shared else 1, _ptr(out), _stream()), "gfa_int_jacobi")
    return out.cpu().numpy()


def _exps_arg(exps: tuple):
    arr = (ctypes.c_uint64 * max(len(exps), 1))(*exps)
    return arr, len(exps)


def _classify_range(n: int, start: int, step: int, count: int, exps: tuple) -> torch.Tensor:
    """Flags (uint8, on the device) of the candidates start + i step, i < count, modulo n < 2^64: bit 1 unit, bit 2 no power
    g^e is 1."""
    from ._array import _device, _ptr, _stream

    flags = torch.empty(count, dtype=torch.uint8, device=_device())
    arr, n_exps = _exps_arg(exps)
    L.check(L.lib().gfa_int_unit_classify(n, None, count, start, step, arr, n_exps, _ptr(flags), _stream()), "gfa_int_unit_classify")
    return flags


def is_primitive_root_batched(g, n: int) -> np.ndarray:
    """Device extension: is_primitive_root(g[i], n) for an array-like of integers 0 < g[i] < n (or a uint64 / int64 tensor) and one
    modulus, as a NumPy bool array.  Moduli without primitive roots answer False without a launch; n = 4 and moduli from 2^64 on
    are answered on the host."""
    from ._array import _ptr, _stream

    _verify_int("n", n)
    if not n > 0:
        raise ValueError(f"Argument 'n' must be a positive integer, not {n}.")
    if n >= _TWO64 or not _device_serves(n) or n <= 2:
        values = g.reshape(-1).tolist() if isinstance(g, (torch.Tensor, np.ndarray)) else [int(v) for v in g]
        if any(not 0 < v < n for v in values):
            raise ValueError(f"Argument 'g' must hold positive integers less than 'n' = {n}.")
        if not is_cyclic(n):
            return np.zeros(len(values), dtype=bool)
        phi, exps = _phi_exponents(n)
        return np.array([_is_root(v, n, phi, exps) for v in values], dtype=bool)
    t = _u64_tensor(g, "g")
    if t.numel() and bool(((t == 0) | ((t ^ (-1 << 63)) >= (_to_i64(n) ^ (-1 << 63)))).any().item()):  # unsigned order on int64 patterns
        raise ValueError(f"Argument 'g' must hold positive integers less than 'n' = {n}.")
    if not is_cyclic(n):
        return np.zeros(t.numel(), dtype=bool)
    arr, n_exps = _exps_arg(_phi_exponents(n)[1])
    flags = torch.empty(t.numel(), dtype=torch.uint8, device=t.device)
    L.check(L.lib().gfa_int_unit_classify(n, _ptr(t), t.numel(), 0, 0, arr, n_exps, _ptr(flags), _stream()), "gfa_int_unit_classify")
    return (flags.cpu().numpy() & 2) != 0
