// gfa_polygcd.h -- Euclid's algorithm and its extended form for one pair of polynomials (gfa_polygcd.hip), written as
// __host__ __device__ templates over the parameters of gfa_polydiv.h (field policy F, Lin views, thread group G) so that
// tests/csrc/polygcd_host_test.cpp compiles the same code with g++ and polydiv::Solo.
//
// The remainder sequence r2, r1 <- r1, r2 mod r1 (gcd / egcd, _polys/_functions.py:10-57) runs on two buffers that never move:
// polydiv::divide on a Lin view leaves the quotient in the first nq = len r2 - len r1 + 1 places of the dividend's buffer and
// the remainder behind it, so the next r1 is the tail of the old r2 (behind its leading zeros, found by leading()) and the next
// r2 is the old r1 where it stands -- the two pointers swap roles, nothing is copied.  The quotient of a step has ANY length
// (the degree may drop by more than one) and stays where divide() left it while the cofactors are updated with it.
//
// Cofactors s, t (a s + b t = r) are stored RIGHT-ALIGNED in buffers of fixed width (coefficient of x^j at index width - 1 - j,
// zeros in front), so that s2 <- s2 - q s1 is in place: coefficient j of the result needs s2[j] and one dot product of q with
// s1, independent of every other coefficient and spread over all threads as polydiv::mulmod's.  deg s <= deg b - 1 and
// deg t <= deg a - 1 for every cofactor that is returned (the update of the step whose remainder is zero is never needed and
// is skipped), so widths nb and na hold them.
//
// Control flow depends on the pair (true degrees, degree drops), so it is uniform within the thread group only: every branch
// below is taken on values all threads of the group hold alike.
#pragma once
#include "gfa_polydiv.h"

namespace gfa {
namespace polygcd {

using polydiv::imax;
using polydiv::imin;
using polydiv::Lin;

// the smallest value of v over the group's threads, through the word `slot` all of them can reach; every thread returns it.
// One thread is its own group; gfa_polygcd.hip specialises it for the workgroup.
template <class G>
struct GroupMin;
template <>
struct GroupMin<polydiv::Solo> {
    GFA_HD static int run(const polydiv::Solo &, int v, int *) { return v; }
};

// the number of leading zero coefficients of the n at p (n for the zero polynomial); the threads' writes to p are ordered before
template <class E, class G>
GFA_HD int leading(const E *p, int n, int *slot, const G &g)
{
    int first = n;
    for (int i = g.tid; i < n; i += g.n)
        if (p[i] != 0) {
            first = i;
            break;
        }
    return GroupMin<G>::run(g, first, slot);
}

// c2 <- c2 - q c1 for right-aligned cofactors of width w: q has nq coefficients, highest degree first; c1 has at most l1
// significant coefficients.  Returns the (bound on the) length of the result, at most w.  No ordering point inside.
template <class F, class G>
GFA_HD int cofactor_step(const FieldDev &fd, typename F::elem *c2, int l2, const typename F::elem *c1, int l1, const typename F::elem *q, int nq,
                         int w, const G &g)
{
    typedef typename F::elem E;
    if (l1 == 0) return l2;
    const int len = imin(w, imax(l2, nq + l1 - 1));
    for (int j = g.tid; j < len; j += g.n) { // the coefficient of x^j
        E acc = c2[w - 1 - j];
#pragma unroll(polydiv::Unroll<F>::n)
        for (int i = imax(0, j - (l1 - 1)); i <= imin(j, nq - 1); i++) acc = F::sub(fd, acc, F::mul(fd, q[nq - 1 - i], c1[w - 1 - (j - i)]));
        c2[w - 1 - j] = acc;
    }
    return len;
}

template <class E>
struct Result {
    E *r; // the monic gcd: len coefficients, highest degree first; len == 0 for gcd(0, 0) = 0
    int len;
    E *s, *t; // extended form only: right-aligned in widths nb and na, ls / lt significant coefficients at most
    int ls, lt;
};

// Euclid on ra (na >= 1 coefficients, leading zeros allowed) and rb (nb >= 1), both overwritten.  With `extended`, s2 and s1
// are buffers of nb and t2 and t1 of na coefficients (contents ignored).  `slot` is one word for GroupMin.  The last non-zero
// remainder -- and s and t with it -- is divided by its leading coefficient (_functions.py:21-26, 50-55).
template <class F, class G>
GFA_HD Result<typename F::elem> euclid(const FieldDev &fd, typename F::elem *ra, int na, typename F::elem *rb, int nb, typename F::elem *s2, typename F::elem *s1,
                                       typename F::elem *t2, typename F::elem *t1, bool extended, int *slot, const G &g)
{
    typedef typename F::elem E;
    g.sync();
    int z = leading(ra, na, slot, g);
    E *p2 = ra + z;
    int l2 = na - z;
    z = leading(rb, nb, slot, g);
    E *p1 = rb + z;
    int l1 = nb - z;
    int ls2 = 1, ls1 = 0, lt2 = 0, lt1 = 1;
    if (extended) { // s2 = 1, s1 = 0, t2 = 0, t1 = 1
        for (int i = g.tid; i < nb; i += g.n) {
            s2[i] = i == nb - 1 ? F::one(fd) : (E)0;
            s1[i] = 0;
        }
        for (int i = g.tid; i < na; i += g.n) {
            t2[i] = 0;
            t1[i] = i == na - 1 ? F::one(fd) : (E)0;
        }
        g.sync();
    }
    while (l1 > 0) {
        E *p;
        int l;
        if (l2 >= l1) {
            const int nq = l2 - l1 + 1;
            const Lin<E> R = polydiv::divide<F, Lin<E>, Lin<E>, polydiv::NoSource, polydiv::NoQuotient, G>(fd, Lin<E>{p2}, Lin<E>{p1}, polydiv::NoSource(), l2, l1,
                                                                                                     polydiv::NoQuotient(), false, false, g);
            z = leading(R.p, l1 - 1, slot, g);
            p = R.p + z;
            l = l1 - 1 - z;
            if (extended && l > 0) { // the quotient is p2[0 .. nq)
                ls2 = cofactor_step<F, G>(fd, s2, ls2, s1, ls1, p2, nq, nb, g);
                lt2 = cofactor_step<F, G>(fd, t2, lt2, t1, lt1, p2, nq, na, g);
                g.sync();
            }
        } else { // a shorter dividend: the quotient is zero and the remainder the dividend itself
            p = p2;
            l = l2;
        }
        p2 = p1, l2 = l1, p1 = p, l1 = l;
        E *c = s2;
        s2 = s1, s1 = c;
        c = t2, t2 = t1, t1 = c;
        int n = ls2;
        ls2 = ls1, ls1 = n;
        n = lt2, lt2 = lt1, lt1 = n;
    }
    if (l2 > 0) {
        const E c = p2[0], cinv = polydiv::lead_inverse<F>(fd, c);
        g.sync(); // everybody has read the leading coefficient
        for (int i = g.tid; i < l2; i += g.n) p2[i] = polydiv::quotient_digit<F>(fd, p2[i], c, cinv);
        if (extended) {
            for (int j = g.tid; j < ls2; j += g.n) s2[nb - 1 - j] = polydiv::quotient_digit<F>(fd, s2[nb - 1 - j], c, cinv);
            for (int j = g.tid; j < lt2; j += g.n) t2[na - 1 - j] = polydiv::quotient_digit<F>(fd, t2[na - 1 - j], c, cinv);
        }
        g.sync();
    }
    return Result<E>{p2, l2, s2, t2, ls2, lt2};
}

} // namespace polygcd
} // namespace gfa
