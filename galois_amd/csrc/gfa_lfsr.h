// gfa_lfsr.h -- linear-feedback shift registers (gfa_lfsr.hip), written as __host__ __device__ templates so that
// tests/csrc/lfsr_host_test.cpp compiles the same code with g++.
//
// Stepping.  clock() runs the reference's four loops (_lfsr.py:763-777, 826-843, 1398-1415, 1463-1477) for ONE register by
// ONE thread: registers do not talk to each other, so a kernel gives every lane a register of its own.  A Fibonacci
// register is kept as a circular buffer -- its shift is a move of `head`, not of n elements; a Galois register changes every
// element each clock anyway and stays in place.  The values are canonical field elements, so the reference's f == 0 branch
// of the Galois loop (shift only) is the general branch with f = 0 and needs no test.
//
// Jumping.  One clock of a Galois register with characteristic polynomial P multiplies its state polynomial
// G(x) = S[0] + S[1] x + ... + S[n-1] x^(n-1) by x modulo P and puts out the quotient digit.  So
//   (1) the T outputs of T clocks are the quotient of G x^T by P, the new state is the remainder;
//   (2) the state e clocks ahead is x^e G mod P: a modular power and a modular product (polydiv::mulmod);
//   (3) a Fibonacci register with state S is the Galois register G0 = floor(Y P / x^n), Y(x) = S[0] + S[1] x + ..., and its
//       state is its next n outputs reversed (FLFSR.to_galois_lfsr, _lfsr.py:552-575).
// jump() runs (2) for a whole team of threads, with (3) on the way in and (1) for n clocks on the way out.
//
//   F  field policy of gfa_arith.h / polytest::ExtP<M>          V  state view, operator[](int) -> reference
//   T  taps view, operator[](int) -> element                     Y  output sink, set(int, element)
//   B  view of P's n + 1 coefficients, highest degree first      G  the team of threads (gfa_polydiv.h)
#pragma once
#include "gfa_polydiv.h"

namespace gfa {
namespace lfsr {

using polydiv::Lin;

constexpr int KIND_FIBONACCI = 0, KIND_GALOIS = 1;

// the state of a register whose elements are `stride` apart (lane-interleaved in LDS: consecutive lanes on consecutive banks)
template <class E>
struct Strided {
    E *p;
    int stride;
    GFA_HD E &operator[](int j) const { return p[(size_t)j * stride]; }
};

// the tap a backward clock divides by: 1 / t (0 for t == 0, a caller error -- the outputs are then zeros)
template <class F>
GFA_HD typename F::elem backward_inverse(const FieldDev &fd, typename F::elem t)
{
    return polydiv::lead_inverse<F>(fd, t);
}

// `count` clocks of one register of order n.  For KIND_FIBONACCI the logical state element j sits at s[(head + j) % n] and
// head is updated; a Galois register does not use it.  Output i of the call goes to y.set(i, .).  tinv = backward_inverse of
// taps[n - 1] (Fibonacci) or taps[0] (Galois); forward clocks do not use it.
template <class F, class V, class T, class Y>
GFA_HD void clock(const FieldDev &fd, int kind, bool forward, V s, T taps, int n, int &head, typename F::elem tinv, int count, Y y)
{
    typedef typename F::elem E;
    if (kind == KIND_FIBONACCI && forward) {
        for (int i = 0; i < count; i++) {
            E f = 0;
            int j = 0;
            for (int p = head; p < n; p++, j++) f = F::add(fd, f, F::mul(fd, s[p], (E)taps[j]));
            for (int p = 0; p < head; p++, j++) f = F::add(fd, f, F::mul(fd, s[p], (E)taps[j]));
            const int last = head == 0 ? n - 1 : head - 1; // the element that leaves; its slot takes the feedback
            y.set(i, s[last]);
            s[last] = f;
            head = last;
        }
    } else if (kind == KIND_FIBONACCI) {
        const E tn = (E)taps[n - 1];
        for (int i = 0; i < count; i++) {
            E acc = s[head]; // the feedback value that entered last; every other element moves one place left
            int j = 0;
            for (int p = head + 1; p < n; p++, j++) acc = F::sub(fd, acc, F::mul(fd, s[p], (E)taps[j]));
            for (int p = 0; p < head; p++, j++) acc = F::sub(fd, acc, F::mul(fd, s[p], (E)taps[j]));
            acc = polydiv::quotient_digit<F>(fd, acc, tn, tinv);
            y.set(i, acc);
            s[head] = acc;
            head = head + 1 == n ? 0 : head + 1;
        }
    } else if (forward) {
        for (int i = 0; i < count; i++) {
            const E f = s[n - 1];
            y.set(i, f);
            for (int j = n - 1; j > 0; j--) s[j] = F::add(fd, s[j - 1], F::mul(fd, f, (E)taps[j]));
            s[0] = F::mul(fd, f, (E)taps[0]);
        }
    } else {
        const E t0 = (E)taps[0];
        for (int i = 0; i < count; i++) {
            const E f = polydiv::quotient_digit<F>(fd, s[0], t0, tinv);
            for (int j = 0; j < n - 1; j++) s[j] = F::sub(fd, s[j + 1], F::mul(fd, f, (E)taps[j + 1]));
            s[n - 1] = f;
            y.set(i, f);
        }
    }
}

// GF(2), n <= 64: the state is one word (bit j = S[j]), `taps` the taps as a word, mask = the low n bits.  Returns the
// `count` <= 64 outputs, output i in bit i.
GFA_HD u64 clock_bits(int kind, u64 &s, u64 taps, int n, int count)
{
    const u64 mask = n == 64 ? ~(u64)0 : (((u64)1 << n) - 1);
    u64 out = 0;
    if (kind == KIND_FIBONACCI) {
        for (int i = 0; i < count; i++) {
            u64 par = s & taps; // parity of the tapped bits
            par ^= par >> 32;
            par ^= par >> 16;
            par ^= par >> 8;
            par ^= par >> 4;
            par ^= par >> 2;
            par ^= par >> 1;
            out |= ((s >> (n - 1)) & 1) << i;
            s = ((s << 1) | (par & 1)) & mask;
        }
    } else {
        for (int i = 0; i < count; i++) {
            const u64 f = (s >> (n - 1)) & 1;
            out |= f << i;
            s = ((s << 1) & mask) ^ (taps & (0 - f));
        }
    }
    return out;
}

// r <- x r mod c for a residue of n coefficients, highest degree first: one register clock.  t is work space for n coefficients.
template <class F, class B, class G>
GFA_HD void mulx(const FieldDev &fd, Lin<typename F::elem> r, Lin<typename F::elem> t, B c, int n, const G &g)
{
    typedef typename F::elem E;
    const E f = r[0];
    for (int i = g.tid; i < n; i += g.n) t[i] = F::sub(fd, i + 1 < n ? r[i + 1] : (E)0, F::mul(fd, f, (E)c[i + 1]));
    g.sync();
    for (int i = g.tid; i < n; i += g.n) r[i] = t[i];
    g.sync();
}

// LDS elements of a jump: c, r, g0 and the 2 n coefficients of w
constexpr size_t jump_elems(int n) { return (size_t)(n + 1) + 2 * (size_t)n + 2 * (size_t)n; }

// The state e clocks ahead of the state S that w[0 .. n) holds (S[0] first); it arrives in g0[0 .. n), S[0] first.
// c = the characteristic polynomial (n + 1 coefficients, monic); r, g0: n coefficients each; w: 2 n.  e >= 0 is `limbs`
// little-endian words, the same for every thread of the team.
template <class F, class B, class G>
GFA_HD void jump(const FieldDev &fd, int kind, Lin<typename F::elem> w, Lin<typename F::elem> r, Lin<typename F::elem> g0, B c, int n,
                 const u64 *e, int limbs, const G &g)
{
    typedef typename F::elem E;
    // G0, highest degree first: the state reversed, or identity (3): g_j = sum over k <= n - 1 - j of S[j + k] a_k
    for (int j = g.tid; j < n; j += g.n) {
        E acc = w[j];
        if (kind == KIND_FIBONACCI)
            for (int k = 1; k < n - j; k++) acc = F::add(fd, acc, F::mul(fd, w[j + k], (E)c[k]));
        g0[n - 1 - j] = acc;
    }
    // x^e mod c, left to right over the bits of e: a square is a product, a set bit is one clock
    for (int j = g.tid; j < n; j += g.n) r[j] = j == n - 1 ? F::one(fd) : (E)0;
    g.sync();
    const int bits = polytest::limb_bits(e, limbs);
    for (int b = bits - 1; b >= 0; b--) {
        if (b != bits - 1) polydiv::mulmod<F, B, G>(fd, r, r, r, w, c, n, g);
        if ((e[b >> 6] >> (b & 63)) & 1) mulx<F, B, G>(fd, r, w, c, n, g);
    }
    polydiv::mulmod<F, B, G>(fd, r, r, g0, w, c, n, g);
    if (kind == KIND_FIBONACCI) { // identity (1): the next n outputs are the quotient of r x^n by c
        for (int j = g.tid; j < 2 * n; j += g.n) w[j] = j < n ? r[j] : (E)0;
        polydiv::divide<F, Lin<E>, B, polydiv::NoSource, polydiv::NoQuotient, G>(fd, w, c, polydiv::NoSource(), 2 * n, n + 1, polydiv::NoQuotient(),
                                                                                false, false, g);
        for (int j = g.tid; j < n; j += g.n) g0[j] = w[n - 1 - j];
    } else {
        for (int j = g.tid; j < n; j += g.n) g0[j] = r[n - 1 - j];
    }
    g.sync();
}

} // namespace lfsr
} // namespace gfa
