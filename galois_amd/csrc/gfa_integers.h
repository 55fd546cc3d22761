// gfa_integers.h -- per-lane arithmetic of the integer number-theory kernels (gfa_integers.hip), written as
// __host__ __device__ functions so that tests/csrc/integers_host_test.cpp compiles the same code with g++.
//
//   is_prime64 ........ deterministic Miller-Rabin below 2^64 (the seven bases of Jaeschke / Sinclair), Montgomery form with the
//                       constants of the candidate itself; Prime64::redc serves every odd modulus below 2^64.
//   jacobi ............ the binary algorithm: halve, swap with the reciprocity sign, subtract.  No division after the first
//                       reduction of a.
//   unit_flags ........ bit 1: gcd(g, n) == 1 (binary gcd).  bit 2: g is a unit and g^e != 1 (mod n) for every one of the
//                       launch's exponents -- with e = phi(n) / r over the primes r | phi(n), g is a primitive root.
//   mark_segment ...... one segment of the sieve of the odd numbers: bit j of a word array stands for first + 2 j; the
//                       multiples of the base primes from p^2 on are set.  Small primes are marked by all lanes together,
//                       the others one prime per lane, so two lanes can meet in one word: the caller passes the `or`.
#pragma once
#include "gfa_arith.h"

namespace gfa {
namespace integers {

enum : uint8_t { INT_UNIT = 1, INT_PRIMITIVE = 2 };

constexpr int MAX_EXPS = 16;       // phi(n) < 2^64 has at most 15 distinct prime factors
constexpr int SEG_WORDS = 8192;    // 32 KiB of LDS per segment
constexpr int SEG_BITS = SEG_WORDS * 32;
constexpr u64 SEG_SPAN = 2ull * SEG_BITS; // integers covered by one segment (odd numbers only are stored)
constexpr u32 COOP_PRIME = 1024;   // base primes below this are marked by all lanes of the workgroup together

GFA_HD int ctz64(u64 x) { return __builtin_ctzll(x); } // x != 0

// ---- Montgomery form modulo any odd n >= 3 ----------------------------------------------------------------------------
struct Mont {
    FieldDev fd; // p and nprime are what Prime64 reads
    u64 one;     // 2^64 mod n
    u64 r2;      // 2^128 mod n
};

GFA_HD u64 addmod(u64 a, u64 b, u64 n)
{
    u64 c = a + b;
    if (c < a || c >= n) c -= n;
    return c;
}

GFA_HD Mont mont_setup(u64 n)
{
    Mont m;
    m.fd = FieldDev();
    m.fd.p = n;
    u64 inv = n; // n n = 1 (mod 8); every step doubles the correct bits
    for (int i = 0; i < 5; i++) inv *= 2 - n * inv;
    m.fd.nprime = (u64)0 - inv;
    m.one = ((u64)0 - n) % n;
    u64 x = m.one;
    for (int i = 0; i < 64; i++) x = addmod(x, x, n);
    m.r2 = x;
    return m;
}

GFA_HD u64 mont_mul(const Mont &m, u64 a, u64 b) { return Prime64::montmul(m.fd, a, b); }
GFA_HD u64 to_mont(const Mont &m, u64 a) { return mont_mul(m, a, m.r2); } // a < n

// base^e in Montgomery form, left to right over the bits of e; e = 0 gives one
GFA_HD u64 mont_pow(const Mont &m, u64 base, u64 e)
{
    u64 r = m.one;
    for (int b = 63 - clz64(e | 1); b >= 0; b--) {
        r = mont_mul(m, r, r);
        if ((e >> b) & 1) r = mont_mul(m, r, base);
    }
    return r;
}

// ---- primality --------------------------------------------------------------------------------------------------------
GFA_HD bool is_prime64(u64 n)
{
    if (n < 2) return false;
    if (n < 4) return true;
    if ((n & 1) == 0) return false;
    const Mont m = mont_setup(n);
    const u64 minus_one = n - m.one;
    const int s = ctz64(n - 1);
    const u64 d = (n - 1) >> s;
    const u64 bases[7] = {2, 325, 9375, 28178, 450775, 9780504, 1795265022};
    for (int i = 0; i < 7; i++) {
        const u64 a = bases[i] % n;
        if (a == 0) continue;
        u64 x = mont_pow(m, to_mont(m, a), d);
        if (x == m.one || x == minus_one) continue;
        bool witness = true;
        for (int k = 1; k < s; k++) {
            x = mont_mul(m, x, x);
            if (x == minus_one) { witness = false; break; }
        }
        if (witness) return false;
    }
    return true;
}

// ---- the Jacobi symbol (a / n), n odd and >= 3 ---------------------------------------------------------------------------
GFA_HD int jacobi(i64 a_signed, u64 n)
{
    u64 a;
    if (a_signed >= 0) a = (u64)a_signed % n;
    else {
        const u64 r = ((u64)0 - (u64)a_signed) % n;
        a = r ? n - r : 0;
    }
    int t = 1;
    while (a != 0) {
        const int z = ctz64(a);
        a >>= z;
        if ((z & 1) && ((n & 7) == 3 || (n & 7) == 5)) t = -t;
        if (a < n) {
            if ((a & 3) == 3 && (n & 3) == 3) t = -t;
            const u64 s = a;
            a = n;
            n = s;
        }
        a -= n; // both odd: the difference is even, and (a - n / n) = (a / n)
    }
    return n == 1 ? t : 0;
}

// ---- units and primitive roots -------------------------------------------------------------------------------------------
GFA_HD u64 gcd64(u64 a, u64 b)
{
    if (a == 0) return b;
    if (b == 0) return a;
    const int shift = ctz64(a | b);
    a >>= ctz64(a);
    do {
        b >>= ctz64(b);
        if (a > b) {
            const u64 s = a;
            a = b;
            b = s;
        }
        b -= a;
    } while (b != 0);
    return a << shift;
}

// The modulus the powers run under: n itself when odd, n / 2 for n = 2 odd (a unit of n is odd there, the groups agree), 0
// for every other even n (no Montgomery form; such n > 4 has no primitive root).
GFA_HD u64 power_modulus(u64 n) { return (n & 1) ? n : ((n & 3) == 2 ? n >> 1 : 0); }

// `mont` is the form of power_modulus(n), set up by the caller when that modulus is >= 3 and n_exps > 0.
GFA_HD uint8_t unit_flags(u64 g, u64 n, const Mont &mont, u64 modulus, const u64 *exps, int n_exps)
{
    if (gcd64(g, n) != 1) return 0;
    if (n_exps == 0) return INT_UNIT | INT_PRIMITIVE;
    if (modulus < 3) return INT_UNIT; // every power is 1 modulo 1
    const u64 base = to_mont(mont, g % modulus);
    for (int c = 0; c < n_exps; c++) // the same exponents in every lane: uniform branches
        if (mont_pow(mont, base, exps[c]) == mont.one) return INT_UNIT;
    return INT_UNIT | INT_PRIMITIVE;
}

// ---- the segmented sieve -----------------------------------------------------------------------------------------------------
// Index of the first bit that p sets in a segment whose bit 0 is the odd integer `first`: the smallest odd multiple of p that
// is >= max(p p, first).  p odd, p < 2^32, first < 2^63.
GFA_HD u64 first_mark(u64 first, u64 p)
{
    const u64 sq = p * p;
    if (sq >= first) return (sq - first) >> 1;
    const u64 r = first % p;
    u64 m = r ? first + (p - r) : first;
    if ((m & 1) == 0) m += p;
    return (m - first) >> 1;
}

// Sets the composites among first, first + 2, .., first + 2 (n_bits - 1) in `words` (bit j of the array = bit j & 31 of word
// j >> 5), as lane `lane` of `n_lanes`.  `primes` are ascending; 2 is skipped.  `set_bits(word index, mask)` is the caller's or.
template <class Or>
GFA_HD void mark_segment(u64 first, u32 n_bits, const u32 *primes, int n_primes, int lane, int n_lanes, Or set_bits)
{
    const u64 end = first + 2ull * n_bits; // one past the last integer of the segment
    int i = 0;
    for (; i < n_primes; i++) { // all lanes walk the multiples of one small prime
        const u64 p = primes[i];
        if (p < 3) continue;
        if (p >= COOP_PRIME || p * p >= end) break;
        for (u64 j = first_mark(first, p) + (u64)lane * p; j < n_bits; j += (u64)n_lanes * p) set_bits((u32)(j >> 5), 1u << (j & 31));
    }
    for (i += lane; i < n_primes; i += n_lanes) { // one prime per lane
        const u64 p = primes[i];
        if (p * p >= end) break;
        for (u64 j = first_mark(first, p); j < n_bits; j += p) set_bits((u32)(j >> 5), 1u << (j & 31));
    }
}

// Word w of a segment as the device writes it: a set bit is a prime.  `marked` is the composite word; bits at or beyond n_bits
// are cleared, and so is the bit of the integer 1.
GFA_HD u32 survivors_word(u32 marked, u32 w, u64 first, u32 n_bits)
{
    u32 v = ~marked;
    const u32 lo = w * 32;
    if (lo >= n_bits) return 0;
    if (n_bits - lo < 32) v &= (1u << (n_bits - lo)) - 1;
    if (first == 1 && w == 0) v &= ~1u;
    return v;
}

} // namespace integers
} // namespace gfa
