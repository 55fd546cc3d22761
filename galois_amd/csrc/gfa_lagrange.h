// gfa_lagrange.h -- one row of Lagrange interpolation (gfa_lagrange.hip): the unique L with deg L < k and L(x_i) = y_i, written
// as __host__ __device__ templates so that tests/csrc/lagrange_host_test.cpp compiles the same code with g++.
//
// A row is worked by a team G of g.n threads (g.tid of g.n; fewer threads than points stride over them) on six arrays of k
// elements of the field policy and one flag, all the team's own:
//   x[k] c[k] a[2][k] m[2][k] dup
// Coefficients in a and m stand lowest degree first (index j is the coefficient of x^j); the interface is highest degree first,
// so store() reverses them.
//
//   load     x and y arrive in x and c; a = 0, m = 1 (both buffers cleared: a sweep writes only the coefficients that can be
//            non-zero, the others keep this zero), dup = 0
//   weights  thread i: w_i = prod over m != i of (x_i - x_m), the x_m read by every thread at the same address.  w_i == 0 exactly
//            when x_i occurs twice: the thread raises the row's flag (every writer stores the same 1), and c_i = 0.
//            Otherwise c_i = y_i / w_i, one inversion per point.
//   sweep s  with M = prod over m < s of (x - x_m) and A = sum over i < s of c_i prod over m < s, m != i of (x - x_m):
//              A'_j = A_(j-1) - x_s A_j + c_s M_j        M'_j = M_(j-1) - x_s M_j        for j <= s + 1
//            read from buffer s % 2 and written to the other, so that one ordering point per sweep is enough.  After sweep
//            k - 1, A is L.  No powers, no reductions across threads.
//   store    out[k - 1 - j] = A_j, or 0 for a row whose flag is up
//   row      the four in turn.  `live` is false for a team without a row (the last workgroup of a launch): it only keeps the
//            ordering points, whose number depends on k alone.
#pragma once
#include "gfa_polydiv.h"

namespace gfa {
namespace lagrange {

constexpr int LG_ARRAYS = 6; // x c a[2] m[2]

template <class E>
struct Row {
    E *x, *c, *a0, *a1, *m0, *m1, *dup;
};

// the row's arrays in `mem`, LG_ARRAYS * k + 1 elements
template <class E>
GFA_HD Row<E> carve(E *mem, int k)
{
    return Row<E>{mem, mem + k, mem + 2 * (size_t)k, mem + 3 * (size_t)k, mem + 4 * (size_t)k, mem + 5 * (size_t)k, mem + 6 * (size_t)k};
}

template <class F, class X, class Y, class G>
GFA_HD void load(const FieldDev &fd, const Row<typename F::elem> &r, int k, X xs, Y ys, const G &g)
{
    typedef typename F::elem E;
    for (int i = g.tid; i < k; i += g.n) {
        r.x[i] = (E)xs[i];
        r.c[i] = (E)ys[i];
        r.a0[i] = r.a1[i] = r.m1[i] = 0;
        r.m0[i] = i == 0 ? F::one(fd) : (E)0;
    }
    if (g.tid == 0) *r.dup = 0;
}

template <class F, class G>
GFA_HD void weights(const FieldDev &fd, const Row<typename F::elem> &r, int k, const G &g)
{
    typedef typename F::elem E;
    for (int i = g.tid; i < k; i += g.n) {
        const E xi = r.x[i];
        E w = F::one(fd);
        for (int m = 0; m < k; m++) {
            const E d = F::sub(fd, xi, r.x[m]);
            w = F::mul(fd, w, m == i ? F::one(fd) : d);
        }
        if (w == 0) {
            *r.dup = 1;
            r.c[i] = 0;
        } else r.c[i] = F::mul(fd, r.c[i], F::inv(fd, w));
    }
}

template <class F, class G>
GFA_HD void sweep(const FieldDev &fd, const Row<typename F::elem> &r, int k, int s, const G &g)
{
    typedef typename F::elem E;
    const bool odd = s & 1; // (selected, not indexed: the pointers stay in registers)
    const E *a = odd ? r.a1 : r.a0, *m = odd ? r.m1 : r.m0;
    E *a2 = odd ? r.a0 : r.a1, *m2 = odd ? r.m0 : r.m1;
    const E xs = r.x[s], cs = r.c[s];
    const int top = polydiv::imin(k, s + 2);
    for (int j = g.tid; j < top; j += g.n) {
        const E al = j ? a[j - 1] : (E)0, ml = j ? m[j - 1] : (E)0, mj = m[j];
        a2[j] = F::add(fd, F::sub(fd, al, F::mul(fd, xs, a[j])), F::mul(fd, cs, mj));
        m2[j] = F::sub(fd, ml, F::mul(fd, xs, mj));
    }
}

template <class E, class O, class G>
GFA_HD void store(const Row<E> &r, int k, bool dup, O out, const G &g)
{
    const E *a = (k & 1) ? r.a1 : r.a0;
    for (int j = g.tid; j < k; j += g.n) out.set(k - 1 - j, dup ? 0 : (u64)a[j]);
}

// Interpolates one row; returns whether its x has a repeated entry (to every thread of a live team).
template <class F, class X, class Y, class O, class G>
GFA_HD bool row(const FieldDev &fd, const Row<typename F::elem> &r, int k, X xs, Y ys, O out, bool live, const G &g)
{
    if (live) load<F, X, Y, G>(fd, r, k, xs, ys, g);
    g.sync();
    if (live) weights<F, G>(fd, r, k, g);
    g.sync();
    for (int s = 0; s < k; s++) {
        if (live) sweep<F, G>(fd, r, k, s, g);
        g.sync();
    }
    if (!live) return false;
    const bool dup = *r.dup != 0;
    store<typename F::elem, O, G>(r, k, dup, out, g);
    return dup;
}

} // namespace lagrange
} // namespace gfa
