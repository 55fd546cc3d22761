// Host model of galois_amd/csrc/gfa_polytest.h: the per-candidate routines the device kernels run, compiled with g++.
//
// For GF(2) up to degree 12, GF(3) up to degree 6, GF(5) and GF(4) up to degree 4 every monic polynomial is sieved (all
// products of two monic polynomials of lower degree are marked reducible) and the header's Rabin test must agree on each
// one; its primitivity routine must agree with the order of x found by stepping through the powers of x.  GF(2) runs
// through the bit-packed routines with one, two and four words (a low-degree f sits left-aligned in the wider forms), the
// other fields through the general routines on strided columns, as the device lays them out in LDS.  The compile-time digit
// policy ExtP<2> is compared with the run-time Ext over GF(p^2) for the largest primes below 2^31 and below 2^32.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_polytest.h"

using namespace gfa;
using namespace gfa::polytest;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            std::exit(1);                                  \
        }                                                  \
    } while (0)

// GF(4) = GF(2)[a] / (a^2 + a + 1) on a product table: a field policy that is not one of gfa_arith.h
struct GF4 {
    typedef u32 elem;
    static u32 add(const FieldDev &, u32 a, u32 b) { return a ^ b; }
    static u32 sub(const FieldDev &, u32 a, u32 b) { return a ^ b; }
    static u32 mul(const FieldDev &, u32 a, u32 b)
    {
        static const u32 T[4][4] = {{0, 0, 0, 0}, {0, 1, 2, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}};
        return T[a][b];
    }
    static u32 inv(const FieldDev &, u32 a)
    {
        static const u32 I[4] = {0, 1, 3, 2};
        return I[a];
    }
    static u32 one(const FieldDev &) { return 1; }
};

static FieldDev prime_field(u64 p)
{
    FieldDev fd = {};
    fd.p = fd.q = p;
    fd.m = 1;
    fd.kind = KIND_PRIME32;
    fd.mu = (u64)((((unsigned __int128)1) << 64) / p);
    return fd;
}

static u64 ipow(u64 q, int k)
{
    u64 v = 1;
    while (k--) v *= q;
    return v;
}

static std::vector<u64> prime_divisors(u64 n)
{
    std::vector<u64> out;
    for (u64 r = 2; r * r <= n; r++)
        if (n % r == 0) {
            out.push_back(r);
            while (n % r == 0) n /= r;
        }
    if (n > 1) out.push_back(n);
    return out;
}

// the schedule the library's host side builds: m / r ascending, then m
static std::vector<int> rabin_steps(int m)
{
    std::vector<int> out;
    for (u64 r : prime_divisors((u64)m)) out.insert(out.begin(), m / (int)r); // divisors ascend, so m / r descends
    out.push_back(m);
    return out;
}

// ---- general fields ------------------------------------------------------------------------------------------------
template <class F>
static int sweep(const FieldDev &fd, u64 q, int max_degree, const char *name)
{
    typedef typename F::elem E;
    // polynomials as integers in radix q; digits ascending
    auto digits = [&](u64 v, int n) {
        std::vector<E> d((size_t)n);
        for (int i = 0; i < n; i++) { d[i] = (E)(v % q); v /= q; }
        return d;
    };
    const u64 total = 2 * ipow(q, max_degree);
    std::vector<char> reducible((size_t)total, 0);
    for (int a = 1; a <= max_degree; a++)
        for (int b = a; a + b <= max_degree; b++)
            for (u64 g = ipow(q, a); g < 2 * ipow(q, a); g++)
                for (u64 h = ipow(q, b); h < 2 * ipow(q, b); h++) {
                    const std::vector<E> dg = digits(g, a + 1), dh = digits(h, b + 1);
                    std::vector<E> pr((size_t)(a + b + 1), 0);
                    for (int i = 0; i <= a; i++)
                        for (int k = 0; k <= b; k++) pr[i + k] = F::add(fd, pr[i + k], F::mul(fd, dg[i], dh[k]));
                    u64 v = 0;
                    for (int i = a + b; i >= 0; i--) v = v * q + pr[i];
                    reducible[(size_t)v] = 1;
                }
    int n_irr = 0, n_prim = 0, checked = 0;
    for (int m = 1; m <= max_degree; m++) {
        const std::vector<int> steps = rabin_steps(m);
        const int limbs = 2; // the values fit one word; the second exercises the limb scan
        std::vector<u64> frob;
        for (int s : steps) { frob.push_back(ipow(q, s)); frob.push_back(0); }
        const u64 group = ipow(q, m) - 1;
        std::vector<u64> cof;
        if (group > 1)
            for (u64 r : prime_divisors(group)) { cof.push_back(group / r); cof.push_back(0); }
        const int stride = 3; // three interleaved columns, as lanes interleave in LDS
        std::vector<E> store((size_t)(3 * (m + 1) * stride), 0);
        for (u64 v = ipow(q, m); v < 2 * ipow(q, m); v++) {
            for (int lane = 0; lane < stride; lane += 2) { // the first and the last column
                std::fill(store.begin(), store.end(), (E)0);
                E *base = store.data() + lane;
                const Col<E> f{base, stride}, r{base + (m + 1) * stride, stride}, t{base + 2 * (m + 1) * stride, stride};
                const std::vector<E> d = digits(v, m + 1);
                for (int i = 0; i <= m; i++) f[i] = d[i];
                const bool irr = irreducible<F, Col<E>>(fd, f, r, t, m, frob.data(), (int)steps.size(), limbs);
                CHECK(irr == !reducible[(size_t)v], "%s: irreducibility of %llu (degree %d): header says %d", name, (unsigned long long)v, m, (int)irr);
                for (int i = 0; i <= m; i++) CHECK(f[i] == d[i], "%s: f modified", name);
                for (size_t i = 0; i < store.size(); i++)
                    CHECK((int)(i % stride) == lane || store[i] == 0, "%s: a neighbouring column was written", name);
                if (!irr) continue;
                // order of x by stepping: x^k for k = 1, 2, ... (independent of the header: plain shift and subtract)
                bool expect = d[0] != 0;
                if (expect) {
                    std::vector<E> pw((size_t)m, 0);
                    if (m == 1) pw[0] = F::sub(fd, 0, d[0]); else pw[1] = F::one(fd);
                    u64 order = 1;
                    for (;;) {
                        bool one = pw[0] == F::one(fd);
                        for (int i = 1; i < m; i++) one = one && pw[i] == 0;
                        if (one) break;
                        const E c = pw[m - 1];
                        for (int i = m - 1; i >= 1; i--) pw[i] = F::sub(fd, pw[i - 1], F::mul(fd, c, d[i]));
                        pw[0] = F::sub(fd, 0, F::mul(fd, c, d[0]));
                        order++;
                        CHECK(order <= group, "%s: x has no order modulo %llu", name, (unsigned long long)v);
                    }
                    expect = order == group;
                }
                const bool prim = primitive_given_irreducible<F, Col<E>>(fd, f, r, t, m, cof.data(), (int)cof.size() / 2, limbs);
                CHECK(prim == expect, "%s: primitivity of %llu (degree %d): header says %d", name, (unsigned long long)v, m, (int)prim);
                if (lane == 0) { n_irr++; n_prim += prim; }
            }
            checked++;
        }
    }
    std::printf("%s: %d polynomials up to degree %d, %d irreducible, %d primitive\n", name, checked, max_degree, n_irr, n_prim);
    return checked;
}

// ---- GF(2), bit-packed ---------------------------------------------------------------------------------------------
template <int W>
static void sweep_gf2(int max_degree, const std::vector<char> &reducible, int *n_irr_out, int *n_prim_out)
{
    int n_irr = 0, n_prim = 0;
    for (int m = 1; m <= max_degree; m++) {
        const std::vector<int> steps = rabin_steps(m);
        const u64 group = ((u64)1 << m) - 1;
        std::vector<u64> cof;
        if (group > 1)
            for (u64 r : prime_divisors(group)) { cof.push_back(group / r); cof.push_back(0); }
        for (u64 v = (u64)1 << m; v < (u64)2 << m; v++) {
            Bits<W> f = bzero<W>();
            f.w[0] = v;
            f = bshl<W>(f, 64 * W - 1 - m);
            CHECK((f.w[W - 1] >> 63) == 1, "left alignment");
            const bool irr = birreducible<W>(f, m, steps.data(), (int)steps.size());
            CHECK(irr == !reducible[(size_t)v], "GF(2), W = %d: irreducibility of %llu: header says %d", W, (unsigned long long)v, (int)irr);
            if (!irr) continue;
            bool expect = (v & 1) != 0;
            if (expect) {
                u64 pw = m == 1 ? 1 : 2, order = 1; // x mod (x + 1) = 1
                while (pw != 1) {
                    pw <<= 1;
                    if (pw >> m) pw ^= v;
                    order++;
                    CHECK(order <= group, "no order");
                }
                expect = order == group;
            }
            const bool prim = bprimitive_given_irreducible<W>(f, m, cof.data(), (int)cof.size() / 2, 2);
            CHECK(prim == expect, "GF(2), W = %d: primitivity of %llu: header says %d", W, (unsigned long long)v, (int)prim);
            n_irr++;
            n_prim += prim;
        }
    }
    *n_irr_out = n_irr;
    *n_prim_out = n_prim;
}

// a few full-width cases: the lexicographically first irreducible polynomials of minimal weight, and reducible neighbours
template <int W>
static void wide_case(int m, std::vector<int> lower, bool expect)
{
    Bits<W> f = bzero<W>();
    lower.push_back(m);
    for (int d : lower) {
        Bits<W> b = bzero<W>();
        b.w[0] = 1;
        bxor_masked<W>(f, bshl<W>(b, 64 * W - 1 - m + d), ~(u64)0);
    }
    const std::vector<int> steps = rabin_steps(m);
    CHECK(birreducible<W>(f, m, steps.data(), (int)steps.size()) == expect, "degree %d, W = %d", m, W);
}

// ---- the digit-vector policy of the kernels against the run-time Ext --------------------------------------------------
// GF(p^2) = GF(p)[x] / (x^2 - a), a a non-residue: ExtP<2> must give Ext's values, below 2^31 (unreduced 64-bit sums) and
// just below 2^32 (where those sums would overflow and every product is reduced first)
static void ext2_case(u64 p)
{
    FieldDev fd = prime_field(p);
    u32 a = 2;
    while (Prime32::pow_barrett(fd, a, (p - 1) / 2) == 1) a++; // Euler's criterion
    fd.q = p * p;
    fd.m = 2;
    fd.kind = KIND_EXT;
    fd.ext_irr[0] = 0;
    fd.ext_irr[1] = (u32)(p - a);
    u64 s = 88172645463325252ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s % fd.q; };
    for (int i = 0; i < 20000; i++) {
        u64 x = rnd(), y = rnd();
        if (i == 0) { x = fd.q - 1; y = fd.q - 1; } // both digits p - 1: the largest middle coefficient
        if (i == 1) { x = fd.q - 1; y = p * (p - 1); }
        CHECK(ExtP<2>::mul(fd, x, y) == Ext::mul(fd, x, y), "GF(%llu^2): product of %llu and %llu", (unsigned long long)p, (unsigned long long)x, (unsigned long long)y);
        CHECK(ExtP<2>::add(fd, x, y) == Ext::add(fd, x, y) && ExtP<2>::sub(fd, x, y) == Ext::sub(fd, x, y), "GF(%llu^2): sum / difference", (unsigned long long)p);
        if (i < 200 && x) CHECK(ExtP<2>::mul(fd, x, ExtP<2>::inv(fd, x)) == 1, "GF(%llu^2): inverse of %llu", (unsigned long long)p, (unsigned long long)x);
    }
    // x^2 - c over GF(p^2) is irreducible iff c is a non-square: c^((q - 1) / 2) != 1, the power taken with Ext
    const int m = 2, limbs = 3;
    std::vector<u64> frob;
    const unsigned __int128 q2 = (unsigned __int128)fd.q * fd.q;
    frob.insert(frob.end(), {fd.q, 0, 0, (u64)q2, (u64)(q2 >> 64), 0}); // q^(2/2), q^2
    int n_irr = 0;
    for (int i = 0; i < 40; i++) {
        const u64 c = rnd() | 1;
        u64 store[9] = {ExtP<2>::sub(fd, 0, c % fd.q), 0, 1};
        const Col<u64> f{store, 1}, r{store + 3, 1}, t{store + 6, 1};
        const bool irr = irreducible<ExtP<2>, Col<u64>>(fd, f, r, t, m, frob.data(), 2, limbs);
        const bool expect = Ext::pow_u(fd, c % fd.q, (fd.q - 1) / 2) != 1;
        CHECK(irr == expect, "GF(%llu^2): x^2 - %llu", (unsigned long long)p, (unsigned long long)(c % fd.q));
        n_irr += irr;
    }
    CHECK(n_irr > 5 && n_irr < 35, "GF(%llu^2): %d of 40 irreducible", (unsigned long long)p, n_irr);
    std::printf("GF(%llu^2): ExtP<2> agrees with Ext; %d of 40 x^2 - c irreducible\n", (unsigned long long)p, n_irr);
}

int main()
{
    const int D2 = 12;
    std::vector<char> red2((size_t)2 << D2, 0);
    for (u64 g = 2; g < ((u64)2 << D2); g++)
        for (u64 h = g; h < ((u64)2 << D2); h++) {
            const int dg = 63 - __builtin_clzll(g), dh = 63 - __builtin_clzll(h);
            if (dg + dh > D2) break;
            u64 pr = 0;
            for (int i = 0; i <= dh; i++)
                if ((h >> i) & 1) pr ^= g << i;
            red2[(size_t)pr] = 1;
        }
    int irr1, prim1, irr2, prim2, irr4, prim4;
    sweep_gf2<1>(D2, red2, &irr1, &prim1);
    sweep_gf2<2>(D2, red2, &irr2, &prim2);
    sweep_gf2<4>(8, red2, &irr4, &prim4);
    CHECK(irr1 == irr2 && prim1 == prim2, "W = 1 and W = 2 disagree");
    std::printf("GF(2): degrees 1..%d, %d irreducible, %d primitive (W = 1, 2); degrees 1..8 with W = 4: %d, %d\n", D2, irr1, prim1, irr4, prim4);
    wide_case<1>(63, {1, 0}, true);
    wide_case<1>(63, {2, 1, 0}, false);         // an even number of terms: divisible by x + 1
    wide_case<2>(64, {4, 3, 1, 0}, true);
    wide_case<2>(64, {4, 3, 0}, false);
    wide_case<2>(127, {1, 0}, true);
    wide_case<4>(128, {7, 2, 1, 0}, true);
    wide_case<4>(255, {52, 0}, true);
    wide_case<4>(255, {52, 1}, false);          // no constant term

    sweep<Prime32>(prime_field(3), 3, 6, "GF(3)");
    sweep<Prime32>(prime_field(5), 5, 4, "GF(5)");
    FieldDev fd4 = {};
    fd4.p = 2; fd4.q = 4; fd4.m = 2;
    sweep<GF4>(fd4, 4, 4, "GF(4)");
    ext2_case(2147483629);  // the largest prime below 2^31
    ext2_case(4294967291);  // the largest prime below 2^32
    std::printf("polytest host model ok\n");
    return 0;
}
