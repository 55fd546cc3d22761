"""Host side of the multi-limb fields of tests/limb_fields.py (no GPU): the parameter words that galois_amd/_wide.py and
galois_amd/_big.py hand to gfa_wfield_create / gfa_bfield_create satisfy their definitions, every modulus of the table is what the
table claims (Miller-Rabin for the primes, Rabin's irreducibility test for the polynomials, both written here on Python
integers and not imported from the code under test), and the oracle that tests/test_gpu_limb_edges.py compares the kernels with
is a field for each of them (a typo in a polynomial shows up here rather than as a device mismatch)."""
import random

import pytest

from galois_amd._big import big_params, limbs_for
from galois_amd._wide import wide_params
from tests import limb_fields as LF

M64 = (1 << 64) - 1


# ---- primality and irreducibility on plain Python integers -----------------------------------------------------------
def _miller_rabin(n, rounds=32):
    if n < 2 or n % 2 == 0:
        return n == 2
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    rnd = random.Random(n)
    for a in [2, 3, 5, 7, 11, 13] + [rnd.randrange(2, n - 1) for _ in range(rounds)]:
        if a % n == 0:
            continue
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _prime_divisors(n):
    out, d = [], 2
    while d * d <= n:
        if n % d == 0:
            out.append(d)
            while n % d == 0:
                n //= d
        d += 1
    return out + ([n] if n > 1 else [])


# GF(2)[x]: a polynomial is the integer of its coefficient bits
def _b_mod(a, f):
    df = f.bit_length()
    while a.bit_length() >= df:
        a ^= f << (a.bit_length() - df)
    return a


def _b_sqr_mod(a, f, m, low):
    """a^2 mod f, f = x^m + sum_{e in low} x^e: the square spreads the bits (binary digits read as base-4 digits); the part at
    x^m and above folds down through x^m = sum x^e."""
    a = int(bin(a)[2:], 4)
    mask = (1 << m) - 1
    while a >> m:
        h = a >> m
        a &= mask
        for e in low:
            a ^= h << e
    return a


def _b_gcd(a, b):
    while b:
        a, b = b, _b_mod(a, b)
    return a


def _rabin_binary(f, m):
    """Rabin: f of degree m is irreducible over GF(2) iff x^(2^m) = x mod f and gcd(x^(2^(m/r)) - x, f) = 1 for every prime r | m."""
    if f.bit_length() - 1 != m:
        return False
    low = [e for e in range(m) if (f >> e) & 1]
    stops = {m // r for r in _prime_divisors(m)}
    x = 2
    for k in range(1, m + 1):
        x = _b_sqr_mod(x, f, m, low)
        if k in stops and _b_gcd(f, x ^ 2) != 1:
            return False
    return x == 2


# GF(p)[x], p odd: coefficient lists, lowest degree first, no trailing zeros
def _trim(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _p_mod(a, f, p):
    a = list(a)
    inv = pow(f[-1], -1, p)
    while len(a) >= len(f):
        c = a[-1] * inv % p
        if c:
            off = len(a) - len(f)
            for i, fi in enumerate(f):
                a[off + i] = (a[off + i] - c * fi) % p
        a.pop()
    return _trim(a)


def _p_mulmod(a, b, f, p):
    if not a or not b:
        return []
    c = [0] * (len(a) + len(b) - 1)
    for i, ai in enumerate(a):
        if ai:
            for j, bj in enumerate(b):
                c[i + j] += ai * bj
    return _p_mod([v % p for v in c], f, p)


def _p_powmod(a, e, f, p):
    r = [1]
    while e:
        if e & 1:
            r = _p_mulmod(r, a, f, p)
        a = _p_mulmod(a, a, f, p)
        e >>= 1
    return r


def _p_gcd_is_one(a, b, p):
    while b:
        a, b = b, _p_mod(a, b, p)
    return len(a) == 1


def _rabin_odd(coeffs_high_first, p):
    f = coeffs_high_first[::-1]
    m = len(f) - 1
    if f[-1] != 1:
        return False
    stops = {m // r for r in _prime_divisors(m)}
    x = [0, 1]
    g = x
    for k in range(1, m + 1):
        g = _p_powmod(g, p, f, p)  # x^(p^k)
        d = list(g) + [0] * max(0, 2 - len(g))
        d[1] = (d[1] - 1) % p
        if k in stops and not _p_gcd_is_one(f, _trim(d), p):
            return False
    return g == x


def test_the_helpers_reject_composites_and_reducible_polynomials():
    assert not _miller_rabin(2**128 - 157) and not _miller_rabin(2**64 + 1) and _miller_rabin(2**61 - 1)
    assert _rabin_binary(0b10011, 4) and not _rabin_binary(0b10101, 4) and not _rabin_binary((1 << 64) | 0b111, 64)
    assert not _rabin_binary(LF.FIELDS["gf2e192"]["irr"] ^ 2, 192)  # x^192 + x^7 + x^2 + 1 has the root 1
    assert _rabin_odd([1, 0, 1], 3) and not _rabin_odd([1, 0, 2], 3) and not _rabin_odd([1, 0, 0, 0, 1], 17)  # x^4 + 1 = (x^2 - 4)(x^2 + 4) over GF(17)
    assert not _rabin_odd([1] + [0] * 15 + [17 - 2], 17)  # x^16 - 2: ord(2) = 8 mod 17, the binomial criterion fails


@pytest.mark.parametrize("tag", LF.TAGS)
def test_modulus_is_what_the_table_claims(tag):
    f = LF.FIELDS[tag]
    p, m, nl = f["p"], f["m"], f["nl"]
    q = p**m
    assert _miller_rabin(p), f"{tag}: the characteristic is not prime"
    assert 2**64 <= q and (q - 1).bit_length() <= 64 * nl and (nl == 2 or (q - 1).bit_length() > 64 * (nl // 2)), f"{tag}: not a {nl}-limb order"
    if LF.kind(f) == "binary":
        assert f["irr"] >> m == 1 and _rabin_binary(f["irr"], m), f"{tag}: the polynomial is reducible"
    elif LF.kind(f) == "extension":
        co = LF.irr_coeffs(f)
        assert len(co) == m + 1 and all(0 <= c < p for c in co) and _rabin_odd(co, p), f"{tag}: the polynomial is reducible"
    if tag in LF.FULL_WIDTH_PRIMES:
        assert p >> (64 * nl - 1) == 1


def _group(words, at, n=16):
    return sum(w << (64 * k) for k, w in enumerate(words[at:at + n]))


@pytest.mark.parametrize("tag", LF.TAGS)
def test_parameter_words_satisfy_their_definitions(tag):
    f = LF.FIELDS[tag]
    p, m, nl = f["p"], f["m"], f["nl"]
    q = p**m
    kd = LF.kind(f)
    irr = LF.irr_int(f) if m > 1 else 2 * p - 2  # (a prime field's "polynomial" x - alpha is not a parameter of the kernels)
    if nl == 2:
        assert not (q > 2**128 or (q == 2**128 and p != 2)), "a two-limb field of the factory's routing rule"
        k, w = wide_params(p, m, irr)
        assert len(w) == 27
        P, nprime, r2, einv, red, itr, digits = _group(w, 0, 2), w[2], _group(w, 3, 2), _group(w, 5, 2), _group(w, 7, 2), _group(w, 9, 2), w[11:27]
        maxd = 16
    else:
        assert limbs_for(q) == nl and (q > 2**128 or (q == 2**128 and p != 2))
        k, w = big_params(p, m, irr, nl)
        assert len(w) == 113
        P, nprime, r2, einv, red, itr, digits = _group(w, 0), w[16], _group(w, 17), _group(w, 33), _group(w, 49), _group(w, 65), w[81:113]
        maxd = 32
        for at in (0, 17, 33, 49, 65):  # every word above the limb count is zero
            assert all(v == 0 for v in w[at + nl:at + 16]), f"{tag}: words above limb {nl} of the group at {at}"
    assert all(0 <= v <= M64 for v in w)
    assert k == {"prime": 1, "binary": 2, "extension": 3}[kd]
    if kd == "prime":
        assert P == p and (nprime * p) % 2**64 == 2**64 - 1
        assert r2 == pow(2, 128 * nl, p) and einv == p - 2
        assert red == 0 and itr == 0 and not any(digits)
    elif kd == "binary":
        assert P == 2 and einv == 2**m - 2 and red == f["irr"] ^ (1 << m) and red < 2**m
        assert nprime == 0 and r2 == 0 and itr == 0 and not any(digits)
    else:
        assert P == p and p < 2**32 and m <= maxd
        assert itr == (q - 1) // (p - 1) - 1 and (itr + 1) * (p - 1) == q - 1
        assert digits[:m] == LF.irr_coeffs(f)[1:] and not any(digits[m:])  # f - x^m from degree m - 1 down
        assert nprime == 0 and r2 == 0 and einv == 0 and red == 0


@pytest.mark.parametrize("tag", LF.TAGS)
def test_the_oracle_is_a_field_for_every_modulus(tag):
    """mul(a, inv(a)) == 1 and pow(a, q - 1) == 1 on a few elements (two for the fields of 512 bits and more, whose binary
    oracle spends a second per exponentiation), and the linear operations undo each other."""
    f = LF.FIELDS[tag]
    W = LF.oracle(tag)
    q, p = W.q, W.p
    rnd = random.Random(len(tag) + f["nl"])
    picks = [q - 1] + [rnd.randrange(2, q) for _ in range(1 if q.bit_length() >= 512 else 3)]
    for a in picks:
        ia = W.inv(a)
        assert 0 < ia < q and W.mul(a, ia) == 1 and W.mul(ia, a) == 1, f"{tag}: a * a^-1"
        assert W.pow(a, q - 1) == 1, f"{tag}: a^(q-1)"
        b = rnd.randrange(q)
        assert W.sub(W.add(a, b), b) == a and W.add(a, W.neg(a)) == 0 and W.mul(a, 1) == a and W.mul(a, 0) == 0
    assert f["m"] == 1 or W.pow(p, f["m"]) == W.neg(_tail(f)), f"{tag}: x^m = -(f - x^m)"


def _tail(f):
    """f - x^m as a field element: x^m = -(f - x^m)."""
    v = 0
    for c in LF.irr_coeffs(f)[1:]:
        v = v * f["p"] + c
    return v


def test_field_classes_construct_with_the_limb_count_of_the_table():
    """Every field of the table is built with an explicit primitive element and verify=False (no device is needed for that).  The
    two-limb binary and extension fields still have the primitivity of their polynomial computed, which factors q - 1: 2^64 - 1,
    17^16 - 1 and 65521^8 - 1 split into small factors at once."""
    for tag in LF.TAGS:
        GF = LF.make_field(tag)
        f = LF.FIELDS[tag]
        assert GF._NL == f["nl"] and GF.order == f["p"] ** f["m"] and GF.characteristic == f["p"] and GF.degree == f["m"], tag
        assert LF.make_field(tag) is GF
