// Host model of galois_amd/csrc/gfa_polyelem.h: the per-candidate routines of the primitive / normal element kernels, compiled
// with g++.
//
// Every residue of GF(2)[x] / f up to degree 10, GF(3)[x] / f up to degree 5, GF(5)[x] / f up to degree 4 and GF(4)[x] / f at
// degrees 2 and 3 (f the first monic irreducible polynomial of the degree, found here by trial division) goes through the
// header's routines on strided columns, as the device lays them out in LDS, and through the bit-packed routines over GF(2).
// The references are written here and share nothing with the header: normality is the rank of the matrix of conjugates by
// elimination (products are schoolbook products reduced afterwards, not Horner's rule), primitivity is the multiplicative
// order found by stepping through the powers.  The counts must be q^m prod (1 - q^(-deg P_i)) and phi(q^m - 1).  The cofactor
// matrices c_i(Phi) are built here the way the library's Python layer builds them (Phi from x^q, x^m - 1 factored by trial
// division, Horner with matrix products), and are also fed in pieces, as the kernels stage them in slabs.  The packed path
// runs at m = 63, 64, 65, 127, 128 and 129 on samples against an elimination on std::bitset.
#include <algorithm>
#include <bitset>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_polyelem.h"

using namespace gfa;
using namespace gfa::polytest;
using namespace gfa::polyelem;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            std::exit(1);                                  \
        }                                                  \
    } while (0)

// field policies that are not among gfa_arith.h's
struct GF4 { // GF(2)[a] / (a^2 + a + 1)
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

struct GF2P {
    typedef u32 elem;
    static u32 add(const FieldDev &, u32 a, u32 b) { return a ^ b; }
    static u32 sub(const FieldDev &, u32 a, u32 b) { return a ^ b; }
    static u32 mul(const FieldDev &, u32 a, u32 b) { return a & b; }
    static u32 inv(const FieldDev &, u32 a) { return a; }
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

// ---- reference arithmetic on plain vectors, ascending coefficients ---------------------------------------------------
template <class F>
struct Ref {
    typedef typename F::elem E;
    typedef std::vector<E> P;
    FieldDev fd;
    u64 q;

    P digits(u64 v, int n) const
    {
        P d((size_t)n);
        for (int i = 0; i < n; i++) { d[i] = (E)(v % q); v /= q; }
        return d;
    }
    static int deg(const P &a)
    {
        int d = (int)a.size() - 1;
        while (d >= 0 && a[d] == 0) d--;
        return d;
    }
    // a mod b and, when quo is given, a / b; b monic
    P rem(P a, const P &b, P *quo = nullptr) const
    {
        const int db = deg(b);
        if (quo) quo->assign(a.size(), 0);
        for (int d = deg(a); d >= db; d--) {
            const E c = a[d];
            if (c == 0) continue;
            if (quo) (*quo)[d - db] = c;
            for (int k = 0; k <= db; k++) a[d - db + k] = F::sub(fd, a[d - db + k], F::mul(fd, c, b[k]));
        }
        a.resize((size_t)db);
        return a;
    }
    // schoolbook product, reduced afterwards
    P mulmod(const P &a, const P &b, const P &f) const
    {
        P pr(a.size() + b.size(), 0);
        for (size_t i = 0; i < a.size(); i++)
            for (size_t k = 0; k < b.size(); k++) pr[i + k] = F::add(fd, pr[i + k], F::mul(fd, a[i], b[k]));
        return rem(pr, f);
    }
    P powmod(const P &a, u64 e, const P &f) const
    {
        P r((size_t)deg(f), 0), s = a;
        r[0] = 1;
        for (; e; e >>= 1) {
            if (e & 1) r = mulmod(r, s, f);
            s = mulmod(s, s, f);
        }
        return r;
    }
    bool is_one(const P &a) const
    {
        for (size_t i = 1; i < a.size(); i++)
            if (a[i]) return false;
        return a[0] == 1;
    }
    // rank of the rows by elimination
    int rank(std::vector<P> rows) const
    {
        const int n = (int)rows.size(), w = n ? (int)rows[0].size() : 0;
        int rk = 0;
        for (int c = 0; c < w && rk < n; c++) {
            int piv = -1;
            for (int r = rk; r < n; r++)
                if (rows[r][c]) { piv = r; break; }
            if (piv < 0) continue;
            std::swap(rows[rk], rows[piv]);
            const E iv = F::inv(fd, rows[rk][c]);
            for (int r = rk + 1; r < n; r++) {
                const E k = F::mul(fd, rows[r][c], iv);
                if (k == 0) continue;
                for (int j = c; j < w; j++) rows[r][j] = F::sub(fd, rows[r][j], F::mul(fd, k, rows[rk][j]));
            }
            rk++;
        }
        return rk;
    }
    // the first monic irreducible polynomial of degree m in integer order: no monic polynomial of degree 1 .. m / 2 divides it
    P first_irreducible(int m) const
    {
        for (u64 v = ipow(q, m); v < 2 * ipow(q, m); v++) {
            const P f = digits(v, m + 1);
            bool irr = true;
            for (int d = 1; d <= m / 2 && irr; d++)
                for (u64 h = ipow(q, d); h < 2 * ipow(q, d) && irr; h++)
                    if (deg(rem(f, digits(h, d + 1))) < 0) irr = false;
            if (irr) return f;
        }
        CHECK(false, "no irreducible polynomial of degree %d", m);
        return P();
    }
    // the distinct monic irreducible factors of x^m - 1, by trial division in ascending order: once every smaller factor is
    // divided out completely, a divisor of what is left is irreducible
    std::vector<P> factors_of_xm_minus_1(int m) const
    {
        P left((size_t)(m + 1), 0);
        left[m] = 1;
        left[0] = F::sub(fd, 0, 1);
        std::vector<P> out;
        for (int d = 1; deg(left) > 0; d++)
            for (u64 h = ipow(q, d); h < 2 * ipow(q, d) && deg(left) >= d; h++) {
                const P b = digits(h, d + 1);
                bool found = false;
                for (;;) {
                    P quo;
                    if (deg(rem(left, b, &quo)) >= 0) break;
                    left = quo;
                    found = true;
                }
                if (found) out.push_back(b);
            }
        return out;
    }
    // c_i(Phi) for every factor, row-major on ascending coefficients, one after the other
    std::vector<E> cofactor_matrices(const P &f, const std::vector<P> &factors) const
    {
        const int m = deg(f);
        P x((size_t)m, 0);
        if (m == 1) x[0] = F::sub(fd, 0, f[0]); else x[1] = 1;
        const P xq = powmod(x, q, f);
        std::vector<E> phi((size_t)m * m, 0); // column j = x^(q j) mod f
        P col((size_t)m, 0);
        col[0] = 1;
        for (int j = 0; j < m; j++) {
            for (int r = 0; r < m; r++) phi[(size_t)r * m + j] = col[r];
            col = mulmod(col, xq, f);
        }
        P xm1((size_t)(m + 1), 0);
        xm1[m] = 1;
        xm1[0] = F::sub(fd, 0, 1);
        std::vector<E> out;
        for (const P &pi : factors) {
            P c;
            CHECK(deg(rem(xm1, pi, &c)) < 0, "a factor does not divide x^m - 1");
            std::vector<E> acc((size_t)m * m, 0);
            for (int k = deg(c); k >= 0; k--) { // Horner: acc <- acc Phi + c_k I
                std::vector<E> nx((size_t)m * m, 0);
                for (int r = 0; r < m; r++)
                    for (int j = 0; j < m; j++) {
                        const E a = acc[(size_t)r * m + j];
                        if (a == 0) continue;
                        for (int s = 0; s < m; s++) nx[(size_t)r * m + s] = F::add(fd, nx[(size_t)r * m + s], F::mul(fd, a, phi[(size_t)j * m + s]));
                    }
                for (int r = 0; r < m; r++) nx[(size_t)r * m + r] = F::add(fd, nx[(size_t)r * m + r], c[k]);
                acc = nx;
            }
            out.insert(out.end(), acc.begin(), acc.end());
        }
        return out;
    }
};

static u64 expected_normal_count(u64 q, int m, const std::vector<int> &degrees)
{
    u64 n = ipow(q, m);
    for (int d : degrees) n = n / ipow(q, d) * (ipow(q, d) - 1);
    return n;
}

static u64 euler_phi(u64 n)
{
    u64 phi = n;
    for (u64 r : prime_divisors(n)) phi = phi / r * (r - 1);
    return phi;
}

// packs m ascending coefficients (0 / 1) where the kernels put them: coefficient j at bit 64 W - 1 - m + j
template <int W, class T>
static Bits<W> pack_residue(const T &c, int m)
{
    Bits<W> b = bzero<W>();
    for (int j = 0; j < m; j++) bset<W>(b, 64 * W - 1 - m + j, c[j] != 0);
    return b;
}

template <int W, class T>
static Bits<W> pack_modulus(const T &f, int m)
{
    Bits<W> b = bzero<W>();
    for (int j = 0; j <= m; j++) bset<W>(b, 64 * W - 1 - m + j, f[j] != 0);
    return b;
}

// ---- every residue of one field ------------------------------------------------------------------------------------
// returns (normal count, primitive count); W > 0 also runs the packed routines (GF(2) only)
template <class F, int W>
static void field_case(const FieldDev &fd, u64 q, int m, const char *name, int *totals)
{
    typedef typename F::elem E;
    typedef std::vector<E> P;
    const Ref<F> R{fd, q};
    const P f = R.first_irreducible(m);
    const std::vector<P> factors = R.factors_of_xm_minus_1(m);
    const std::vector<E> mats = R.cofactor_matrices(f, factors);
    const int n_mats = (int)factors.size();
    std::vector<int> degrees;
    int total_degree = 0;
    for (const P &p : factors) { degrees.push_back(Ref<F>::deg(p)); total_degree += degrees.back(); }
    CHECK(total_degree <= m && total_degree >= 1, "%s, m = %d: factor degrees", name, m);
    if (m % (int)fd.p) CHECK(total_degree == m, "%s, m = %d: x^m - 1 is square-free", name, m);

    const u64 group = ipow(q, m) - 1;
    const int limbs = 2; // the values fit one word; the second exercises the limb scan
    std::vector<u64> cof;
    if (group > 1)
        for (u64 r : prime_divisors(group)) { cof.push_back(group / r); cof.push_back(0); }
    const int n_exps = (int)cof.size() / limbs;

    // packed copies (GF(2))
    std::vector<u64> rows;
    Bits<(W > 0 ? W : 1)> fb = bzero<(W > 0 ? W : 1)>();
    if constexpr (W > 0) {
        fb = pack_modulus<W>(f, m);
        CHECK((fb.w[W - 1] >> 63) == 1, "left alignment");
        for (int k = 0; k < n_mats * m; k++) {
            const Bits<W> b = pack_residue<W>(mats.data() + (size_t)k * m, m);
            for (int w = 0; w < W; w++) rows.push_back(b.w[w]);
        }
    }

    const int stride = 3; // three interleaved columns, as lanes interleave in LDS; f has stride 1
    std::vector<E> store((size_t)(3 * m * stride), 0), fs(f);
    u64 n_normal = 0, n_primitive = 0;
    for (u64 v = 0; v <= group; v++) {
        const P gd = R.digits(v, m);
        // the references
        std::vector<P> conj;
        P cj = gd;
        for (int k = 0; k < m; k++) { conj.push_back(cj); cj = R.powmod(cj, q, f); }
        CHECK(cj == gd, "%s: g^(q^m) != g", name);
        const bool ref_normal = R.rank(conj) == m;
        bool ref_primitive = false;
        if (v != 0) {
            u64 order = 1;
            for (P h = gd; !R.is_one(h); h = R.mulmod(h, gd, f)) {
                order++;
                CHECK(order <= group, "%s: %llu has no order", name, (unsigned long long)v);
            }
            ref_primitive = order == group;
        }
        n_normal += ref_normal;
        n_primitive += ref_primitive;

        for (int lane = 0; lane < stride; lane += 2) { // the first and the last column
            std::fill(store.begin(), store.end(), (E)0);
            E *base = store.data() + lane;
            const Col<E> fv{fs.data(), 1}, g{base, stride}, r{base + m * stride, stride}, t{base + 2 * m * stride, stride};
            for (int j = 0; j < m; j++) g[j] = gd[j];
            const bool prim = primitive_element<F, Col<E>>(fd, g, r, t, fv, m, cof.data(), n_exps, limbs);
            CHECK(prim == ref_primitive, "%s, m = %d: primitivity of %llu: header says %d", name, m, (unsigned long long)v, (int)prim);
            const bool whole = v != 0 && survives<F, Col<E>>(fd, mats.data(), n_mats, g, m);
            CHECK(whole == ref_normal, "%s, m = %d: normality of %llu: header says %d", name, m, (unsigned long long)v, (int)whole);
            // the matrices in pieces of one and of two, as the kernels stage them
            for (int piece = 1; piece <= 2; piece++) {
                bool alive = v != 0;
                for (int b = 0; b < n_mats; b += piece)
                    if (alive) alive = survives<F, Col<E>>(fd, mats.data() + (size_t)b * m * m, std::min(piece, n_mats - b), g, m);
                CHECK(alive == ref_normal, "%s, m = %d: normality of %llu in slabs of %d", name, m, (unsigned long long)v, piece);
            }
            for (int j = 0; j < m; j++) CHECK(g[j] == gd[j] && fs[j] == f[j], "%s: an input was modified", name);
            for (size_t i = 0; i < store.size(); i++)
                CHECK((int)(i % stride) == lane || store[i] == 0, "%s: a neighbouring column was written", name);
        }
        if constexpr (W > 0) {
            const Bits<W> gb = pack_residue<W>(gd, m);
            CHECK(bprimitive_element<W>(gb, fb, m, cof.data(), n_exps, limbs) == ref_primitive, "GF(2), m = %d, W = %d: primitivity of %llu", m, W, (unsigned long long)v);
            CHECK((v != 0 && bsurvives<W>(rows.data(), n_mats, gb, m)) == ref_normal, "GF(2), m = %d, W = %d: normality of %llu", m, W, (unsigned long long)v);
            bool alive = v != 0;
            for (int b = 0; b < n_mats; b++)
                if (alive) alive = bsurvives<W>(rows.data() + (size_t)b * m * W, 1, gb, m);
            CHECK(alive == ref_normal, "GF(2), m = %d, W = %d: normality of %llu in slabs", m, W, (unsigned long long)v);
            if (v > 1) { // products: the header's Horner against the schoolbook product
                const P hd = R.digits((v * 2654435761u) % (group + 1), m);
                const Bits<W> pb = bmulmod<W>(gb, pack_residue<W>(hd, m), fb, m);
                CHECK(beq<W>(pb, pack_residue<W>(R.mulmod(gd, hd, f), m)), "GF(2), m = %d, W = %d: product", m, W);
            }
        }
    }
    CHECK(n_normal == expected_normal_count(q, m, degrees), "%s, m = %d: %llu normal elements", name, m, (unsigned long long)n_normal);
    CHECK(n_primitive == euler_phi(group), "%s, m = %d: %llu primitive elements", name, m, (unsigned long long)n_primitive);
    std::printf("%s, m = %d: %d factors of x^m - 1, %llu normal, %llu primitive\n", name, m, n_mats, (unsigned long long)n_normal,
                (unsigned long long)n_primitive);
    totals[0] += (int)n_normal;
    totals[1] += (int)n_primitive;
}

// ---- GF(2), full width -----------------------------------------------------------------------------------------------
typedef std::bitset<320> BS; // products of two residues of degree 128 have degree 256

static BS bs_mulmod(const BS &a, const BS &b, const BS &f, int m)
{
    BS pr;
    for (int i = 0; i < m; i++)
        if (a[i]) pr ^= b << i;
    for (int d = 2 * m - 2; d >= m; d--)
        if (pr[d]) pr ^= f << (d - m);
    return pr;
}

static int bs_deg(const BS &a)
{
    for (int d = 319; d >= 0; d--)
        if (a[d]) return d;
    return -1;
}

// a mod b (b != 0); quo receives a / b
static BS bs_rem(BS a, const BS &b, BS *quo)
{
    const int db = bs_deg(b);
    quo->reset();
    for (int d = bs_deg(a); d >= db; d--)
        if (a[d]) { a ^= b << (d - db); quo->set(d - db); }
    return a;
}

template <int W>
static void wide_case(int m)
{
    // the first irreducible trinomial, or else pentanomial, of the degree (gfa_polytest.h's Rabin test, which has a host test of its own)
    std::vector<int> steps;
    for (u64 r : prime_divisors((u64)m)) steps.insert(steps.begin(), m / (int)r);
    steps.push_back(m);
    BS f;
    Bits<W> fb = bzero<W>();
    bool found = false;
    auto try_poly = [&](std::vector<int> terms) {
        BS c;
        for (int d : terms) c.set(d);
        Bits<W> b = bzero<W>();
        for (int d : terms) bset<W>(b, 64 * W - 1 - m + d, true);
        if (!birreducible<W>(b, m, steps.data(), (int)steps.size())) return false;
        f = c;
        fb = b;
        return true;
    };
    for (int k = 1; k < m && !found; k++) found = try_poly({m, k, 0});
    for (int a = 3; a < 16 && !found; a++)
        for (int b = 2; b < a && !found; b++)
            for (int c = 1; c < b && !found; c++) found = try_poly({m, a, b, c, 0});
    CHECK(found, "no sparse irreducible polynomial of degree %d", m);

    // Phi: row r holds the coefficients of x^r over the columns; column j = x^(2 j) mod f
    BS x2;
    x2.set(m == 1 ? 0 : 1);
    x2 = bs_mulmod(x2, x2, f, m);
    std::vector<BS> phi((size_t)m);
    BS col;
    col.set(0);
    for (int j = 0; j < m; j++) {
        for (int r = 0; r < m; r++)
            if (col[r]) phi[r].set(j);
        col = bs_mulmod(col, x2, f, m);
    }
    // the factors of x^m + 1 by trial division in ascending order
    BS left;
    left.set(m);
    left.set(0);
    const BS xm1 = left;
    std::vector<BS> factors;
    for (u64 h = 3; bs_deg(left) > 0; h += 2) { // x does not divide x^m + 1: odd h only
        const BS b(h);
        bool hit = false;
        for (;;) {
            BS quo;
            if (bs_rem(left, b, &quo).any()) break;
            left = quo;
            hit = true;
        }
        if (hit) factors.push_back(b);
        CHECK(h < (1u << 20), "degree %d: the factors of x^m - 1 were not found", m);
    }
    const int n_mats = (int)factors.size();
    // c_i(Phi) by Horner on rows: (A Phi)_r = xor of the rows j of Phi with A_rj set
    std::vector<u64> rows;
    for (const BS &pi : factors) {
        BS c;
        CHECK(bs_rem(xm1, pi, &c).none(), "a factor does not divide");
        std::vector<BS> acc((size_t)m);
        for (int k = bs_deg(c); k >= 0; k--) {
            std::vector<BS> nx((size_t)m);
            for (int r = 0; r < m; r++)
                for (int j = 0; j < m; j++)
                    if (acc[r][j]) nx[r] ^= phi[j];
            if (c[k])
                for (int r = 0; r < m; r++) nx[r].flip(r);
            acc = nx;
        }
        for (int r = 0; r < m; r++) {
            const Bits<W> b = pack_residue<W>(acc[r], m);
            for (int w = 0; w < W; w++) rows.push_back(b.w[w]);
        }
    }

    u64 s = 88172645463325252ull + (u64)m;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    // 2^m as an exponent: g^(2^m) = g
    std::vector<u64> e2m((size_t)(m / 64 + 1), 0);
    e2m[m / 64] = (u64)1 << (m % 64);
    int n_normal = 0;
    const int samples = 96;
    BS prev;
    for (int it = 0; it < samples; it++) {
        BS g;
        if (it == 1) g.set(0);                         // 1
        else if (it == 2) g.set(m > 1 ? 1 : 0);        // x
        else if (it == 3) for (int j = 0; j < m; j++) g.set(j);
        else if (it > 3) for (int j = 0; j < m; j++) if (rnd() & 1) g.set(j);
        const Bits<W> gb = pack_residue<W>(g, m);
        // the reference: eliminate the conjugates
        std::vector<BS> conj;
        BS cj = g;
        for (int k = 0; k < m; k++) { conj.push_back(cj); cj = bs_mulmod(cj, cj, f, m); }
        CHECK(cj == g, "degree %d: g^(2^m) != g in the reference", m);
        int rk = 0;
        for (int c = 0; c < m; c++) {
            int piv = -1;
            for (int r = rk; r < m; r++)
                if (conj[r][c]) { piv = r; break; }
            if (piv < 0) continue;
            std::swap(conj[rk], conj[piv]);
            for (int r = rk + 1; r < m; r++)
                if (conj[r][c]) conj[r] ^= conj[rk];
            rk++;
        }
        const bool ref_normal = rk == m;
        n_normal += ref_normal;
        CHECK((g.any() && bsurvives<W>(rows.data(), n_mats, gb, m)) == ref_normal, "degree %d: normality of sample %d", m, it);
        bool alive = g.any();
        for (int b = 0; b < n_mats; b += 3)
            if (alive) alive = bsurvives<W>(rows.data() + (size_t)b * m * W, std::min(3, n_mats - b), gb, m);
        CHECK(alive == ref_normal, "degree %d: normality of sample %d in slabs", m, it);
        CHECK(beq<W>(bmulmod<W>(gb, pack_residue<W>(prev, m), fb, m), pack_residue<W>(bs_mulmod(g, prev, f, m), m)), "degree %d: product of sample %d", m, it);
        if (it < 8) CHECK(beq<W>(bpow_g<W>(gb, fb, m, e2m.data(), (int)e2m.size()), gb), "degree %d: g^(2^m) of sample %d", m, it);
        prev = g;
    }
    CHECK(n_normal > 0 && n_normal < samples, "degree %d: %d of %d samples normal", m, n_normal, samples);
    if (m == 127) { // 2^127 - 1 is prime: the one cofactor exponent is 1, and every residue but 0 and 1 is primitive
        const u64 one_exp[2] = {1, 0};
        for (int it = 0; it < 6; it++) {
            BS g;
            if (it == 1) g.set(0);
            if (it > 1) for (int j = 0; j < m; j++) if (rnd() & 1) g.set(j);
            CHECK(bprimitive_element<W>(pack_residue<W>(g, m), fb, m, one_exp, 1, 2) == (it > 1), "degree 127: primitivity of sample %d", it);
        }
    }
    std::printf("GF(2), m = %d, W = %d: %d factors of x^m - 1, %d of %d samples normal\n", m, W, n_mats, n_normal, samples);
}

int main()
{
    int t2[2] = {0, 0}, t2w[2] = {0, 0}, t3[2] = {0, 0}, t5[2] = {0, 0}, t4[2] = {0, 0};
    const FieldDev fd2 = prime_field(2);
    for (int m = 1; m <= 10; m++) field_case<GF2P, 1>(fd2, 2, m, "GF(2)", t2);
    for (int m = 1; m <= 8; m++) field_case<GF2P, 2>(fd2, 2, m, "GF(2), two words", t2w);
    for (int m = 1; m <= 6; m++) field_case<GF2P, 4>(fd2, 2, m, "GF(2), four words", t2w);
    for (int m = 1; m <= 5; m++) field_case<Prime32, 0>(prime_field(3), 3, m, "GF(3)", t3);
    for (int m = 1; m <= 4; m++) field_case<Prime32, 0>(prime_field(5), 5, m, "GF(5)", t5);
    FieldDev fd4 = {};
    fd4.p = 2; fd4.q = 4; fd4.m = 2;
    for (int m = 2; m <= 3; m++) field_case<GF4, 0>(fd4, 4, m, "GF(4)", t4);
    std::printf("GF(2): degrees 1..10, %d normal, %d primitive\n", t2[0], t2[1]);
    wide_case<1>(63);
    wide_case<2>(64);
    wide_case<2>(65);
    wide_case<2>(127);
    wide_case<4>(128);
    wide_case<4>(129);
    std::printf("polyelem host model ok\n");
    return 0;
}
