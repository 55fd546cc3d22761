// gfa_polyroots.h -- what happens to the hits of a root search (gfa_polyroots.hip): taking a slot, sorting a row's slots and
// counting how often (x - r) divides the row, written as __host__ __device__ templates so that
// tests/csrc/polyroots_host_test.cpp compiles the same code with g++ and polydiv::Solo.
//
// A row is ncoef >= 2 coefficients, highest degree first, leading zeros allowed; it has at most cap = ncoef - 1 roots unless it
// is the zero polynomial, which the callers detect from the coefficients (row_is_zero) and never from a count of hits.
//
//   take_slot     a hit owns the slot an atomic counter handed it; it is stored only below the row's capacity, so neither the
//                 zero polynomial (q hits) nor a wrapped counter can write outside the row
//   sort_slots    rank sort: element j goes to the place (number of elements before it in the order (value, index)) -- a
//                 permutation of [0, n) whatever the values, n (n - 1) independent comparisons spread over the threads
//   multiplicity  synthetic division by (x - r), b_0 = c_0, b_i = c_i + r b_(i-1), whose last value is the remainder f(r) and
//                 whose others are the quotient, repeated on the quotient while the remainder is 0.  Exact in every
//                 characteristic: it is the definition of the multiplicity (the reference's rule on derivatives, with its
//                 reset after p of them, _polys/_poly.py:1672-1698, computes the same number).  One thread per root; the
//                 quotient is kept in a work column of ncoef elements the thread owns, a strided view (polytest::Col) of
//                 LDS on the device -- never a per-lane array indexed at run time.
//   finish_row    the three in turn for one row, by the thread group G
#pragma once
#include "gfa_polydiv.h"

namespace gfa {
namespace polyroots {

using polytest::Col;

// is every one of the n coefficients zero?  (one thread's share; the group combines the shares with any())
template <class E, class G>
GFA_HD bool share_is_zero(const E *c, int n, const G &g)
{
    bool z = true;
    for (int i = g.tid; i < n; i += g.n) z = z && c[i] == 0;
    return z;
}

// the slot an atomic counter handed to a hit: used only below the capacity
GFA_HD bool slot_in_row(u32 slot, int cap) { return slot < (u32)cap; }

template <class S>
GFA_HD void take_slot(S out, int cap, u32 slot, u64 r)
{
    if (slot_in_row(slot, cap)) out.set((int)slot, r);
}

// how many slots of a row hold a hit, given the counter's final value
GFA_HD int slots_taken(u32 counter, int cap) { return counter < (u32)cap ? (int)counter : cap; }

// sorted[rank] = r[j] for the n values at r, in increasing order; equal values keep their order.  r and sorted do not overlap;
// the caller orders the threads' memory before and after.
template <class E, class G>
GFA_HD void sort_slots(const E *r, int n, E *sorted, const G &g)
{
    for (int j = g.tid; j < n; j += g.n) {
        const E v = r[j];
        int rank = 0;
        for (int i = 0; i < n; i++) rank += (r[i] < v || (r[i] == v && i < j)) ? 1 : 0;
        sorted[rank] = v;
    }
}

// the largest m with (x - r)^m | c, for c != 0 with ncoef >= 1 coefficients (leading zeros allowed); 0 when r is no root.
// w: ncoef elements of work space.  At most ncoef - 1 divisions of shrinking length, so at most ncoef^2 / 2 steps.
template <class F, class W>
GFA_HD int multiplicity(const FieldDev &fd, const typename F::elem *c, int ncoef, typename F::elem r, W w)
{
    typedef typename F::elem E;
    E b = c[0];
    w[0] = b;
    for (int i = 1; i < ncoef; i++) { // the first division reads the row itself
        b = F::add(fd, F::mul(fd, b, r), c[i]);
        w[i] = b;
    }
    int m = 0, n = ncoef;
    while (b == 0 && n >= 2) { // w[0 .. n - 1) is the quotient; a zero quotient cannot occur for c != 0
        m++;
        n--;
        b = w[0];
        for (int i = 1; i < n; i++) {
            b = F::add(fd, F::mul(fd, b, r), w[i]);
            w[i] = b;
        }
    }
    return m;
}

struct NoMultiplicity {
    GFA_HD void set(int, int) const {}
};

// multiplicities of the n roots at r in the non-zero row c: root j by thread j % lanes in work column j % lanes of the
// lanes x ncoef elements at work (lanes <= g.n on the device, so that a column has one owner)
template <class F, class M, class G>
GFA_HD void multiplicities(const FieldDev &fd, const typename F::elem *c, int ncoef, const typename F::elem *r, int n, typename F::elem *work, int lanes,
                           M mult, const G &g)
{
    typedef typename F::elem E;
    for (int t = g.tid; t < lanes; t += g.n)
        for (int j = t; j < n; j += lanes) mult.set(j, multiplicity<F, Col<E>>(fd, c, ncoef, r[j], Col<E>{work + t, lanes}));
}

// One row after the search: `counter` hits were claimed and those below the capacity stand, in any order, in slots[0 .. cap).
// Returns the number of roots, -1 for the zero row (`zero`, from the coefficients); sorted[0 .. count) then holds them in
// increasing order and mult (unless `want_mult` is false) has received their multiplicities.  Every thread returns the count.
template <class F, class M, class G>
GFA_HD int finish_row(const FieldDev &fd, const typename F::elem *c, int ncoef, bool zero, const typename F::elem *slots, u32 counter,
                      typename F::elem *sorted, typename F::elem *work, int lanes, bool want_mult, M mult, const G &g)
{
    if (zero) return -1;
    const int n = slots_taken(counter, ncoef - 1);
    sort_slots(slots, n, sorted, g);
    g.sync();
    if (want_mult) multiplicities<F, M, G>(fd, c, ncoef, sorted, n, work, lanes, mult, g);
    return n;
}

} // namespace polyroots
} // namespace gfa
