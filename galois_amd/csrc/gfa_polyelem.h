// gfa_polyelem.h -- per-candidate arithmetic of the primitive / normal element tests (gfa_polyelem.hip), written as
// __host__ __device__ templates so that tests/csrc/polyelem_host_test.cpp compiles the same code with g++.
//
// f is irreducible and monic of degree m over GF(q); a candidate g is a residue of degree < m.
//
//   primitive:  g != 0 and g^((q^m - 1) / r) != 1 (mod f) for every prime r | q^m - 1.
//   normal:     the conjugates g, g^q, .., g^(q^(m-1)) are linearly independent over GF(q).  With Phi the matrix of the
//               q-th power on residues, GF(q^m) is a cyclic GF(q)[x]-module through Phi with annihilator x^m - 1, so g is normal
//               iff c_i(Phi) g != 0 for c_i = (x^m - 1) / P_i and every distinct irreducible factor P_i of x^m - 1.  The host
//               supplies the matrices c_i(Phi); a candidate costs one matrix-vector product per factor, cut short at the first
//               non-zero entry, and no elimination.
//
// The layouts are those of gfa_polytest.h, which this header builds on.  General fields: a polynomial is a view `V` with
// operator[](int) on ascending coefficients (a lane-strided column of LDS on the device, a plain array on the host; the one
// modulus of a launch is a view of stride 1 that every lane reads).  GF(2): Bits<W>, left-aligned -- coefficient j of a residue
// sits at bit 64 W - 1 - m + j, and so does column j of a packed matrix row.
#pragma once
#include "gfa_polytest.h"

namespace gfa {
namespace polyelem {

using polytest::Bits;
using polytest::Col;

// flags written per candidate
enum : uint8_t { PE_PRIMITIVE = 1, PE_NORMAL = 2 };

// ---------------------------------------------------------------------------------------------------------------------
// general fields
// ---------------------------------------------------------------------------------------------------------------------
// r <- a b mod f by Horner's rule over the coefficients of a: t <- t x + a_i b for i = m - 1 .. 0.  t is work space; r may be
// a or b (it is written last).  polytest::sqr is the case a = b.
template <class F, class V>
GFA_HD void mulmod(const FieldDev &fd, V r, V a, V b, V t, V f, int m)
{
    typedef typename F::elem E;
    for (int j = 0; j < m; j++) t[j] = 0;
    for (int i = m - 1; i >= 0; i--) {
        const E ai = a[i], c = t[m - 1];
        for (int j = m - 1; j >= 1; j--)
            t[j] = F::add(fd, F::sub(fd, t[j - 1], F::mul(fd, c, f[j])), F::mul(fd, ai, b[j]));
        t[0] = F::sub(fd, F::mul(fd, ai, b[0]), F::mul(fd, c, f[0]));
    }
    for (int j = 0; j < m; j++) r[j] = t[j];
}

// r <- g^e mod f, left to right over the bits of e (`limbs` little-endian words, the same for every candidate of a launch, so
// the branches are uniform).  e = 0 leaves r = g: the host never sends it, and the chain still ends.
template <class F, class V>
GFA_HD void pow_g(const FieldDev &fd, V r, V t, V g, V f, int m, const u64 *e, int limbs)
{
    for (int j = 0; j < m; j++) r[j] = g[j];
    for (int b = polytest::limb_bits(e, limbs) - 2; b >= 0; b--) {
        mulmod<F, V>(fd, r, r, r, t, f, m);
        if ((e[b >> 6] >> (b & 63)) & 1) mulmod<F, V>(fd, r, r, g, t, f, m);
    }
}

// `exps` holds the n_exps cofactor exponents (q^m - 1) / r.  The zero residue is not primitive (0^e = 0 != 1 would pass).
template <class F, class V>
GFA_HD bool primitive_element(const FieldDev &fd, V g, V r, V t, V f, int m, const u64 *exps, int n_exps, int limbs)
{
    if (polytest::is_zero(g, m)) return false;
    for (int c = 0; c < n_exps; c++) {
        pow_g<F, V>(fd, r, t, g, f, m, exps + (size_t)c * limbs, limbs);
        if (polytest::is_one<F, V>(fd, r, m)) return false;
    }
    return true;
}

// M g == 0 ?  M is m x m, row-major, acting on the ascending coefficients of g; `M` is any view with operator[](int).
// Stops at the first non-zero entry of the product.
template <class F, class VM, class V>
GFA_HD bool mat_kills(const FieldDev &fd, VM M, V g, int m)
{
    typedef typename F::elem E;
    for (int r = 0; r < m; r++) {
        E acc = 0;
        for (int j = 0; j < m; j++) acc = F::add(fd, acc, F::mul(fd, M[r * m + j], g[j]));
        if (acc != 0) return false;
    }
    return true;
}

// true iff none of the n matrices at `mats` (m m elements each) sends g to zero.  g is normal iff this holds for all the
// cofactor matrices, which may be fed in any number of pieces.
template <class F, class V>
GFA_HD bool survives(const FieldDev &fd, const typename F::elem *mats, int n, V g, int m)
{
    for (int k = 0; k < n; k++)
        if (mat_kills<F, const typename F::elem *, V>(fd, mats + (size_t)k * m * m, g, m)) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// GF(2), bit-packed and left-aligned
// ---------------------------------------------------------------------------------------------------------------------
// sets bit `pos` (0 <= pos < 64 W) when `on`; every word index is a constant
template <int W>
GFA_HD void bset(Bits<W> &a, int pos, bool on)
{
    const u64 bit = (u64)(on ? 1 : 0) << (pos & 63);
#pragma unroll
    for (int i = 0; i < W; i++) a.w[i] |= (pos >> 6) == i ? bit : 0;
}

// a b mod f: t <- t x + (bit i of a) b for i = m - 1 .. 0; polytest::bsqr is the case a = b
template <int W>
GFA_HD Bits<W> bmulmod(const Bits<W> &a, const Bits<W> &b, const Bits<W> &f, int m)
{
    Bits<W> t = polytest::bzero<W>(), bits = a;
    polytest::bshl1<W>(bits); // coefficient m - 1 at the top bit
    for (int i = 0; i < m; i++) {
        polytest::bmulx<W>(t, f);
        polytest::bxor_masked<W>(t, b, polytest::btop_mask<W>(bits));
        polytest::bshl1<W>(bits);
    }
    return t;
}

template <int W>
GFA_HD Bits<W> bpow_g(const Bits<W> &g, const Bits<W> &f, int m, const u64 *e, int limbs)
{
    Bits<W> r = g;
    for (int b = polytest::limb_bits(e, limbs) - 2; b >= 0; b--) {
        r = bmulmod<W>(r, r, f, m);
        if ((e[b >> 6] >> (b & 63)) & 1) r = bmulmod<W>(r, g, f, m);
    }
    return r;
}

template <int W>
GFA_HD bool bprimitive_element(const Bits<W> &g, const Bits<W> &f, int m, const u64 *exps, int n_exps, int limbs)
{
    if (polytest::bis_zero<W>(g)) return false;
    const Bits<W> one = polytest::bone<W>(m);
    for (int c = 0; c < n_exps; c++)
        if (polytest::beq<W>(bpow_g<W>(g, f, m, exps + (size_t)c * limbs, limbs), one)) return false;
    return true;
}

GFA_HD u64 parity64(u64 x)
{
    x ^= x >> 32;
    x ^= x >> 16;
    x ^= x >> 8;
    x ^= x >> 4;
    x ^= x >> 2;
    x ^= x >> 1;
    return x & 1;
}

// M g == 0 ?  `rows` holds the m rows of M as W words each (word 0 first), packed like a residue:
// (M g)_r = parity(popcount(row_r & g)).  Stops at the first non-zero entry.
template <int W>
GFA_HD bool bmat_kills(const u64 *rows, const Bits<W> &g, int m)
{
    for (int r = 0; r < m; r++) {
        u64 acc = 0;
#pragma unroll
        for (int i = 0; i < W; i++) acc ^= rows[(size_t)r * W + i] & g.w[i];
        if (parity64(acc)) return false;
    }
    return true;
}

template <int W>
GFA_HD bool bsurvives(const u64 *rows, int n, const Bits<W> &g, int m)
{
    for (int k = 0; k < n; k++)
        if (bmat_kills<W>(rows + (size_t)k * m * W, g, m)) return false;
    return true;
}

} // namespace polyelem
} // namespace gfa
