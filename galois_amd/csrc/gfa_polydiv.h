// gfa_polydiv.h -- polynomial division with remainder and modular powers (gfa_polydiv.hip), written as __host__ __device__
// templates so that tests/csrc/polydiv_host_test.cpp compiles the same code with g++.
//
// Coefficients are in degree-descending order, as in the interface.  Division is synthetic division on a copy W of the
// dividend: for i = 0 .. nq - 1, W[i] <- W[i] / b[0] (quotient coefficient i) and W[i + j] -= W[i] b[j] for 1 <= j < nb; the
// last nb - 1 coefficients are then the remainder (divmod_jit.implementation, _polys/_dense.py:183-198).  Here it is BLOCKED
// with block K: for the K quotient coefficients of a block,
//   triangle()  solves the K x K triangular part -- it needs the top K window coefficients and b[0 .. K) only and is one
//               dependent chain, run by ONE wave with a wave-level ordering point per quotient coefficient;
//   tail()      then gives every other window coefficient t in [K, K + nb - 1) its K updates at once,
//               W[t] -= sum over s < K, 1 <= t - s <= nb - 1 of W[s] b[t - s] -- independent of each other, all threads.
// Values are canonical field elements, so the order of the subtractions does not show in the result.
//
//   F   field policy of gfa_arith.h (F::add / sub / mul / inv on F::elem), polytest::ExtP<M> for KIND_EXT
//   V   window view: operator[](int) -> reference to the coefficient `i` places behind the block's first; advanced(k) slides it.
//       Lin = consecutive memory that holds the whole dividend; Ring = a circular buffer of nb - 1 + 2 K coefficients that is
//       refilled from the source as it slides (the next block's K new coefficients arrive while tail() runs, in slots no
//       live coefficient occupies).  Never a per-lane array indexed at run time.
//   B   divisor view: operator[](int) -> coefficient, b[0] leading
//   G   the threads that run the call: g.tid of g.n, G::wave lanes in the wave that runs triangle(), g.sync() orders
//       the memory of all of them, g.wave_sync() that of the first G::wave.  On the host one thread plays them all in turn.
#pragma once
#include <type_traits>

#include "gfa_polytest.h"

namespace gfa {
namespace polydiv {

constexpr int PD_K = 64; // block: one wavefront wide

template <class E>
struct Lin {
    E *p;
    static constexpr bool ring = false;
    GFA_HD E &operator[](int i) const { return p[i]; }
    GFA_HD Lin advanced(int k) const { return Lin{p + k}; }
};

template <class E>
struct Ring {
    E *p;
    int cap, off; // 0 <= off < cap; indices stay below cap
    static constexpr bool ring = true;
    GFA_HD E &operator[](int i) const
    {
        int j = off + i;
        if (j >= cap) j -= cap;
        return p[j];
    }
    GFA_HD Ring advanced(int k) const
    {
        int o = off + k;
        if (o >= cap) o -= cap;
        return Ring{p, cap, o};
    }
};

// one thread in place of the workgroup: the host model
struct Solo {
    int tid = 0, n = 1;
    static constexpr int wave = 1;
    void sync() const {}
    void wave_sync() const {}
};

// how far the two inner product loops are unrolled (independent LDS reads in flight per lane); the long digit-vector
// products gain nothing from it
template <class F>
struct Unroll {
    static constexpr int n = 4;
};
template <int M>
struct Unroll<polytest::ExtP<M>> {
    static constexpr int n = 1;
};

GFA_HD int imin(int a, int b) { return a < b ? a : b; }
GFA_HD int imax(int a, int b) { return a > b ? a : b; }

// 1 / b0 for the whole division; 0 for b0 == 0 (a caller error: the quotient is then all zero, nothing else happens)
template <class F>
GFA_HD typename F::elem lead_inverse(const FieldDev &fd, typename F::elem b0)
{
    if constexpr (std::is_same<F, Lut>::value) return 0; // div_nz is used instead
    else return b0 == 0 ? (typename F::elem)0 : F::inv(fd, b0);
}

template <class F>
GFA_HD typename F::elem quotient_digit(const FieldDev &fd, typename F::elem w, typename F::elem b0, typename F::elem binv)
{
    if constexpr (std::is_same<F, Lut>::value) return b0 == 0 ? 0 : Lut::div_nz(fd, w, b0);
    else return F::mul(fd, w, binv);
}

// the k <= K quotient coefficients of a block: W[s] <- W[s] / b0, then W[t] -= W[s] b[t - s] for s < t < min(k, s + nb).
// Run by the G::wave lanes `lane`; lane t % G::wave owns W[t], so one ordering point per s -- between the owner's division
// and everybody's read of the quotient -- is all it takes.
template <class F, class V, class B, class G>
GFA_HD void triangle(const FieldDev &fd, V W, B b, int k, int nb, typename F::elem b0, typename F::elem binv, int lane, const G &g)
{
    typedef typename F::elem E;
    for (int s = 0; s < k; s++) {
        if (s % G::wave == lane) W[s] = quotient_digit<F>(fd, W[s], b0, binv);
        g.wave_sync();
        const E q = W[s];
        if (q == 0) continue; // uniform; the reference skips these too
        const int hi = imin(k, s + nb);
        for (int t = s + 1 + (lane + G::wave - (s + 1) % G::wave) % G::wave; t < hi; t += G::wave)
            W[t] = F::sub(fd, W[t], F::mul(fd, q, (E)b[t - s]));
    }
}

// the other nb - 1 window coefficients, each with all of the block's updates
template <class F, class V, class B, class G>
GFA_HD void tail(const FieldDev &fd, V W, B b, int k, int nb, const G &g)
{
    typedef typename F::elem E;
    for (int t = k + g.tid; t < k + nb - 1; t += g.n) {
        E w = W[t];
#pragma unroll(Unroll<F>::n)
        for (int s = imax(0, t - (nb - 1)); s < k; s++) w = F::sub(fd, w, F::mul(fd, W[s], (E)b[t - s]));
        W[t] = w;
    }
}

// Divides the na coefficients of a by b (nb coefficients, 1 <= nb <= na) through the window W.  With `load` the window is
// first filled from a -- all of a for a Lin view, nb - 1 + K coefficients for a Ring --, without it W holds the dividend
// already (Lin only).  With `want_q` quotient coefficient i goes to q.set(i, .).  Returns the view of the nb - 1
// remainder coefficients; every thread's writes are ordered (g.sync()) when it returns.
template <class F, class V, class B, class A, class Q, class G>
GFA_HD V divide(const FieldDev &fd, V W, B b, A a, int na, int nb, Q q, bool want_q, bool load, const G &g)
{
    typedef typename F::elem E;
    const int nq = na - nb + 1;
    if (load) {
        const int first = V::ring ? imin(na, nb - 1 + PD_K) : na;
        for (int t = g.tid; t < first; t += g.n) W[t] = (E)a[t];
    }
    g.sync();
    const E b0 = (E)b[0], binv = lead_inverse<F>(fd, b0);
    for (int i = 0; i < nq; i += PD_K) {
        const int k = imin(PD_K, nq - i);
        if (g.tid < G::wave) triangle<F, V, B, G>(fd, W, b, k, nb, b0, binv, g.tid, g);
        g.sync();
        tail<F, V, B, G>(fd, W, b, k, nb, g);
        if (want_q)
            for (int t = g.tid; t < k; t += g.n) q.set(i + t, W[t]);
        if (V::ring) { // only after a full block is there a next one: its new coefficients take the slots behind the window
            const int k2 = imin(PD_K, nq - i - k);
            for (int t = g.tid; t < k2; t += g.n) W[k + nb - 1 + t] = (E)a[i + k + nb - 1 + t];
        }
        g.sync();
        W = W.advanced(k);
    }
    return W;
}

struct NoSource {
    GFA_HD u64 operator[](int) const { return 0; }
};
struct NoQuotient {
    GFA_HD void set(int, u64) const {}
};

// z <- x y mod c for residues of d = nc - 1 coefficients (z may be x or y).  P is work space for max(2 d - 1, 1)
// coefficients: the product is 2 d - 1 independent dot products, reduced in place by the blocked division.
template <class F, class B, class G>
GFA_HD void mulmod(const FieldDev &fd, Lin<typename F::elem> z, Lin<typename F::elem> x, Lin<typename F::elem> y,
                   Lin<typename F::elem> P, B c, int d, const G &g)
{
    typedef typename F::elem E;
    for (int k = g.tid; k < 2 * d - 1; k += g.n) {
        E acc = 0;
#pragma unroll(Unroll<F>::n)
        for (int i = imax(0, k - (d - 1)); i <= imin(k, d - 1); i++) acc = F::add(fd, acc, F::mul(fd, x[i], y[k - i]));
        P[k] = acc;
    }
    Lin<E> R = P;
    if (d > 1) R = divide<F, Lin<E>, B, NoSource, NoQuotient, G>(fd, P, c, NoSource(), 2 * d - 1, d + 1, NoQuotient(), false, false, g);
    else g.sync();
    for (int j = g.tid; j < d; j += g.n) z[j] = R[j];
    g.sync();
}

// r <- base^e mod c, e >= 0 as `limbs` little-endian words: left to right over the bits, as polytest::pow_x.  The exponent
// is the same for every row of a launch, so the branches are uniform.  e == 0 gives 1 (also for base == 0, as pow_jit).
template <class F, class B, class G>
GFA_HD void power(const FieldDev &fd, Lin<typename F::elem> r, Lin<typename F::elem> base, Lin<typename F::elem> P, B c, int d,
                  const u64 *e, int limbs, const G &g)
{
    typedef typename F::elem E;
    const int bits = polytest::limb_bits(e, limbs);
    for (int j = g.tid; j < d; j += g.n) r[j] = bits ? base[j] : (j == d - 1 ? F::one(fd) : (E)0);
    g.sync();
    for (int step = 2 * (bits - 1) - 1; step >= 0; step--) { // per bit below the top one: square, then multiply if it is set
        const int bit = step >> 1;
        const bool square = step & 1;
        if (!square && !((e[bit >> 6] >> (bit & 63)) & 1)) continue;
        mulmod<F, B, G>(fd, r, r, square ? r : base, P, c, d, g); // one call site: the kernels inline it once
    }
}

} // namespace polydiv
} // namespace gfa
