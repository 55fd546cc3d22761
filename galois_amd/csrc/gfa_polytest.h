// gfa_polytest.h -- per-candidate arithmetic of the irreducibility / primitivity tests (gfa_polytest.hip), written as
// __host__ __device__ templates so that tests/csrc/polytest_host_test.cpp compiles the same code with g++.
//
// Every power the tests need is a power of x modulo the candidate f, so all there is are three operations on a residue
// r(x) of degree < m:  r <- r x,  r <- r^2  and  gcd(f, r - x) == 1.
//
// General fields.  `F` is a field policy of gfa_arith.h (F::add / sub / mul / inv / one on F::elem).  Polynomials are views
// `V` with operator[](int) returning a reference to coefficient i (ascending degree): on the device a lane-strided column of
// LDS (index i * blockDim.x + lane, see Col), on the host a plain array -- never a per-lane array indexed at run time, which
// the compiler would put in scratch memory.  f is held monic with all m + 1 coefficients.
//
// GF(2).  Polynomials are W 64-bit words held LEFT-ALIGNED: the candidate's x^m sits at bit 64 W - 1 and every residue is
// shifted by the same s = 64 W - 1 - m (multiplying both sides of a congruence by x^s changes nothing).  The bit that
// decides a reduction is then always the top bit of the top word, so no word is ever indexed by a run-time value.
#pragma once
#include "gfa_arith.h"

namespace gfa {
namespace polytest {

// flags written per candidate
enum : uint8_t { PT_IRREDUCIBLE = 1, PT_PRIMITIVE = 2, PT_BAD_DEGREE = 0x80 };

// coefficient i of a polynomial whose coefficients are `stride` elements apart
template <class E>
struct Col {
    E *p;
    int stride;
    GFA_HD E &operator[](int i) const { return p[(size_t)i * (size_t)stride]; }
};

// number of significant bits of a little-endian limb array (0 for the value 0)
GFA_HD int limb_bits(const u64 *e, int limbs)
{
    for (int l = limbs - 1; l >= 0; l--)
        if (e[l]) return 64 * l + 64 - clz64(e[l]);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// GF(p^M), p odd, on compile-time digit arrays: the policy the kernels use for KIND_EXT (Ext itself indexes its digit
// arrays at run time, which would put them in scratch memory).  Same values as Ext for every operation.
//   M <= 8 : Ext::mul_m<M>, as the element-wise kernels -- except M = 2 with p >= 2^31, where its unreduced middle
//            coefficient a1 b0 + a0 b1 no longer fits 64 bits: there every product is reduced before it is added.
//   M >= 9 : q < 2^64 leaves p <= 137 (M = 9) down to p <= 13 (M = 16).  Ext::mul_m_small applies: it reduces between its
//            folds for these degrees (FieldDev::r2 is only ever set for M <= 8), so every partial sum stays below
//            (2 M - 1) p^2 + M p^2 < 2^20.
// ---------------------------------------------------------------------------------------------------------------------
template <int M>
struct ExtP {
    typedef u64 elem;
    static GFA_HD u64 add(const FieldDev &f, u64 a, u64 b) { return Ext::lin_m<M, 0>(f, a, b); }
    static GFA_HD u64 sub(const FieldDev &f, u64 a, u64 b) { return Ext::lin_m<M, 1>(f, a, b); }
    // (a1 x + a0)(b1 x + b0) with x^2 = -(irr), any p < 2^32
    static GFA_HD u64 mul2_reduced(const FieldDev &f, u64 a, u64 b)
    {
        u32 av[2], bv[2];
        Ext::to_vec_m<2>(f, a, av);
        Ext::to_vec_m<2>(f, b, bv);
        const u32 n1 = Prime32::neg(f, f.ext_irr[0]), n0 = Prime32::neg(f, f.ext_irr[1]); // x^2 = n1 x + n0
        const u32 hi = Prime32::mul(f, av[0], bv[0]);
        u32 out[2];
        out[0] = Prime32::add(f, Prime32::add(f, Prime32::mul(f, av[0], bv[1]), Prime32::mul(f, av[1], bv[0])), Prime32::mul(f, hi, n1));
        out[1] = Prime32::add(f, Prime32::mul(f, av[1], bv[1]), Prime32::mul(f, hi, n0));
        return Ext::from_vec_m<2>(f, out);
    }
    static GFA_HD u64 mul(const FieldDev &f, u64 a, u64 b)
    {
        if constexpr (M == 2) return (f.p >> 31) ? mul2_reduced(f, a, b) : Ext::mul_m<2>(f, a, b); // uniform over the launch
        else if constexpr (M <= 8) return Ext::mul_m<M>(f, a, b);
        else return Ext::mul_m_small<M>(f, a, b);
    }
    static GFA_HD u64 one(const FieldDev &) { return 1; }
    static GFA_HD u64 inv(const FieldDev &f, u64 a)
    { // Itoh-Tsujii as Ext::inv
        const u64 e = (f.q - 1) / (f.p - 1) - 1;
        u64 r = 1, s = a;
        for (u64 k = e; k; k >>= 1) {
            if (k & 1) r = mul(f, r, s);
            s = mul(f, s, s);
        }
        const u32 norm_inv = Prime32::inv(f, (u32)mul(f, r, a));
        return mul(f, (u64)norm_inv, r);
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// general fields
// ---------------------------------------------------------------------------------------------------------------------
// r <- x mod f
template <class F, class V>
GFA_HD void set_x(const FieldDev &fd, V r, V f, int m)
{
    for (int j = 0; j < m; j++) r[j] = 0;
    if (m == 1) r[0] = F::sub(fd, 0, f[0]);
    else r[1] = F::one(fd);
}

// r <- r x mod f  (f monic of degree m)
template <class F, class V>
GFA_HD void mulx(const FieldDev &fd, V r, V f, int m)
{
    typedef typename F::elem E;
    const E c = r[m - 1];
    for (int j = m - 1; j >= 1; j--) r[j] = F::sub(fd, r[j - 1], F::mul(fd, c, f[j]));
    r[0] = F::sub(fd, 0, F::mul(fd, c, f[0]));
}

// r <- r^2 mod f by Horner's rule over the coefficients of r: t <- t x + r_i r for i = m - 1 .. 0; t is work space
template <class F, class V>
GFA_HD void sqr(const FieldDev &fd, V r, V t, V f, int m)
{
    typedef typename F::elem E;
    for (int j = 0; j < m; j++) t[j] = 0;
    for (int i = m - 1; i >= 0; i--) {
        const E ri = r[i], c = t[m - 1];
        for (int j = m - 1; j >= 1; j--)
            t[j] = F::add(fd, F::sub(fd, t[j - 1], F::mul(fd, c, f[j])), F::mul(fd, ri, r[j]));
        t[0] = F::sub(fd, F::mul(fd, ri, r[0]), F::mul(fd, c, f[0]));
    }
    for (int j = 0; j < m; j++) r[j] = t[j];
}

// r <- x^e mod f, e >= 1 as `limbs` little-endian words: left-to-right square, then multiply by x on a set bit.  The
// exponent is the same for every candidate of a launch, so these branches are uniform.
template <class F, class V>
GFA_HD void pow_x(const FieldDev &fd, V r, V t, V f, int m, const u64 *e, int limbs)
{
    set_x<F, V>(fd, r, f, m);
    for (int b = limb_bits(e, limbs) - 2; b >= 0; b--) {
        sqr<F, V>(fd, r, t, f, m);
        if ((e[b >> 6] >> (b & 63)) & 1) mulx<F, V>(fd, r, f, m);
    }
}

// r <- r - x  (mod f)
template <class F, class V>
GFA_HD void sub_x(const FieldDev &fd, V r, V f, int m)
{
    if (m == 1) r[0] = F::add(fd, r[0], f[0]);
    else r[1] = F::sub(fd, r[1], F::one(fd));
}

template <class V>
GFA_HD bool is_zero(V r, int m)
{
    bool z = true;
    for (int j = 0; j < m; j++) z = z && r[j] == 0;
    return z;
}

template <class F, class V>
GFA_HD bool is_one(const FieldDev &fd, V r, int m)
{
    bool z = r[0] == F::one(fd);
    for (int j = 1; j < m; j++) z = z && r[j] == 0;
    return z;
}

template <class V>
GFA_HD int degree_below(V a, int d)
{ // largest i < d with a[i] != 0, or -1
    int i = d - 1;
    while (i >= 0 && a[i] == 0) i--;
    return i;
}

// gcd(f, b) == 1 ?  b has degree < m.  Destroys b and t (t has room for m + 1 coefficients and receives f).  Euclid with
// pseudo-remainders (a <- lead(b) a - lead(a) x^k b), which needs no inverse; the gcd is only defined up to a unit anyway.
template <class F, class V>
GFA_HD bool gcd_is_one(const FieldDev &fd, V b, V t, V f, int m)
{
    typedef typename F::elem E;
    for (int j = 0; j <= m; j++) t[j] = f[j];
    V a = t;
    int da = m, db = degree_below(b, m);
    if (db < 0) return false; // gcd = f
    for (;;) {
        while (da >= db) { // a <- a mod b, up to a unit
            const E la = a[da], lb = b[db];
            const int k = da - db;
            for (int j = 0; j < k; j++) a[j] = F::mul(fd, lb, a[j]);
            for (int j = k; j < da; j++) a[j] = F::sub(fd, F::mul(fd, lb, a[j]), F::mul(fd, la, b[j - k]));
            a[da] = 0;
            da = degree_below(a, da);
            if (da < 0) return db == 0; // b divides a: the gcd is b
        }
        const V v = a; a = b; b = v;
        const int d = da; da = db; db = d;
    }
}

// f(x) of degree m >= 1 (monic, f[m] = 1) over GF(q).  `frob` holds n_frob exponents of `limbs` words each: q^(m / r) for
// the prime divisors r of m in ascending order of the exponent, then q^m.  Rabin: gcd(f, x^(q^(m/r)) - x) = 1 for every r,
// and x^(q^m) = x.  r and t are work space of m + 1 coefficients.
template <class F, class V>
GFA_HD bool irreducible(const FieldDev &fd, V f, V r, V t, int m, const u64 *frob, int n_frob, int limbs)
{
    for (int c = 0; c < n_frob; c++) {
        pow_x<F, V>(fd, r, t, f, m, frob + (size_t)c * limbs, limbs);
        sub_x<F, V>(fd, r, f, m);
        if (c + 1 < n_frob) {
            if (!gcd_is_one<F, V>(fd, r, t, f, m)) return false;
        } else if (!is_zero(r, m)) return false;
    }
    return true;
}

// an irreducible f with f(0) != 0 is primitive iff x^((q^m - 1) / r) != 1 for every prime r | q^m - 1 (the exponents in `exps`)
template <class F, class V>
GFA_HD bool primitive_given_irreducible(const FieldDev &fd, V f, V r, V t, int m, const u64 *exps, int n_exps, int limbs)
{
    if (f[0] == 0) return false;
    for (int c = 0; c < n_exps; c++) {
        pow_x<F, V>(fd, r, t, f, m, exps + (size_t)c * limbs, limbs);
        if (is_one<F, V>(fd, r, m)) return false;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// GF(2), bit-packed and left-aligned: W words, word W - 1 is the most significant
// ---------------------------------------------------------------------------------------------------------------------
template <int W>
struct Bits {
    u64 w[W];
};

template <int W>
GFA_HD Bits<W> bzero()
{
    Bits<W> z;
#pragma unroll
    for (int i = 0; i < W; i++) z.w[i] = 0;
    return z;
}

template <int W>
GFA_HD bool bis_zero(const Bits<W> &a)
{
    u64 o = 0;
#pragma unroll
    for (int i = 0; i < W; i++) o |= a.w[i];
    return o == 0;
}

template <int W>
GFA_HD bool beq(const Bits<W> &a, const Bits<W> &b)
{
    u64 o = 0;
#pragma unroll
    for (int i = 0; i < W; i++) o |= a.w[i] ^ b.w[i];
    return o == 0;
}

template <int W>
GFA_HD void bxor_masked(Bits<W> &a, const Bits<W> &b, u64 mask)
{
#pragma unroll
    for (int i = 0; i < W; i++) a.w[i] ^= b.w[i] & mask;
}

template <int W>
GFA_HD void bshl1(Bits<W> &a)
{
#pragma unroll
    for (int i = W - 1; i >= 1; i--) a.w[i] = (a.w[i] << 1) | (a.w[i - 1] >> 63);
    a.w[0] <<= 1;
}

// a << k, 0 <= k < 64 W: whole words in stages of 128 and 64, then the bits -- every index is a constant
template <int W>
GFA_HD Bits<W> bshl(Bits<W> a, int k)
{
    if (W > 2 && (k & 128)) {
#pragma unroll
        for (int i = W - 1; i >= 0; i--) a.w[i] = i >= 2 ? a.w[i - 2] : 0;
    }
    if (W > 1 && (k & 64)) {
#pragma unroll
        for (int i = W - 1; i >= 0; i--) a.w[i] = i >= 1 ? a.w[i - 1] : 0;
    }
    const int s = k & 63;
    if (s) {
#pragma unroll
        for (int i = W - 1; i >= 1; i--) a.w[i] = (a.w[i] << s) | (a.w[i - 1] >> (64 - s));
        a.w[0] <<= s;
    }
    return a;
}

template <int W>
GFA_HD int bclz(const Bits<W> &a)
{ // leading zeros of the 64 W-bit value; 64 W for zero
    int n = 0;
    bool open = true;
#pragma unroll
    for (int i = W - 1; i >= 0; i--) {
        const int c = clz64(a.w[i]);
        if (open) n += c;
        open = open && c == 64;
    }
    return n;
}

template <int W>
GFA_HD u64 btop_mask(const Bits<W> &a) { return (u64)((i64)a.w[W - 1] >> 63); } // all-ones iff the top bit is set

// x^0 in the shifted representation: bit s = 64 W - 1 - m
template <int W>
GFA_HD Bits<W> bone(int m)
{
    Bits<W> o = bzero<W>();
    o.w[0] = 1;
    return bshl<W>(o, 64 * W - 1 - m);
}

// r <- r x mod f
template <int W>
GFA_HD void bmulx(Bits<W> &r, const Bits<W> &f)
{
    bshl1<W>(r);
    bxor_masked<W>(r, f, btop_mask<W>(r));
}

// r^2 mod f: t <- t x + (bit i of r) r for i = m - 1 .. 0, the bits of r read off the top of a shifted copy
template <int W>
GFA_HD Bits<W> bsqr(const Bits<W> &r, const Bits<W> &f, int m)
{
    Bits<W> t = bzero<W>(), bits = r;
    bshl1<W>(bits); // coefficient m - 1 at the top bit
    for (int i = 0; i < m; i++) {
        bmulx<W>(t, f);
        bxor_masked<W>(t, r, btop_mask<W>(bits));
        bshl1<W>(bits);
    }
    return t;
}

template <int W>
GFA_HD Bits<W> bpow_x(const Bits<W> &f, int m, const u64 *e, int limbs)
{
    Bits<W> r = bone<W>(m);
    bmulx<W>(r, f);
    for (int b = limb_bits(e, limbs) - 2; b >= 0; b--) {
        r = bsqr<W>(r, f, m);
        if ((e[b >> 6] >> (b & 63)) & 1) bmulx<W>(r, f);
    }
    return r;
}

// gcd(a, b) == 1 in the shifted representation (both are multiples of x^s, so is their gcd: it is 1 iff it equals x^s)
template <int W>
GFA_HD bool bgcd_is_one(Bits<W> a, Bits<W> b, int m)
{
    for (;;) {
        if (bis_zero<W>(b)) return bclz<W>(a) == m;
        if (bis_zero<W>(a)) return bclz<W>(b) == m;
        const int za = bclz<W>(a), zb = bclz<W>(b); // fewer leading zeros = higher degree
        if (za <= zb) bxor_masked<W>(a, bshl<W>(b, zb - za), ~(u64)0);
        else bxor_masked<W>(b, bshl<W>(a, za - zb), ~(u64)0);
    }
}

// Rabin's test over GF(2).  x^(2^k) is k squarings of x, so the checks share one chain: `steps` holds n_steps ascending
// values m / r (r the prime divisors of m, largest first) and then m itself.
template <int W>
GFA_HD bool birreducible(const Bits<W> &f, int m, const int *steps, int n_steps)
{
    Bits<W> x = bone<W>(m);
    bmulx<W>(x, f);
    Bits<W> h = x;
    int done = 0;
    for (int c = 0; c < n_steps; c++) {
        for (; done < steps[c]; done++) h = bsqr<W>(h, f, m);
        Bits<W> d = h;
        bxor_masked<W>(d, x, ~(u64)0);
        if (c + 1 < n_steps) {
            if (!bgcd_is_one<W>(f, d, m)) return false;
        } else if (!bis_zero<W>(d)) return false;
    }
    return true;
}

template <int W>
GFA_HD bool bprimitive_given_irreducible(const Bits<W> &f, int m, const u64 *exps, int n_exps, int limbs)
{
    const Bits<W> one = bone<W>(m);
    Bits<W> c0 = bzero<W>(); // the constant term of f
    bxor_masked<W>(c0, f, ~(u64)0);
#pragma unroll
    for (int i = 0; i < W; i++) c0.w[i] &= one.w[i];
    if (bis_zero<W>(c0)) return false;
    for (int c = 0; c < n_exps; c++)
        if (beq<W>(bpow_x<W>(f, m, exps + (size_t)c * limbs, limbs), one)) return false;
    return true;
}

} // namespace polytest
} // namespace gfa
