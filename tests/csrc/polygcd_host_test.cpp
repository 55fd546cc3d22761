// Host model of galois_amd/csrc/gfa_polygcd.h: Euclid's algorithm and its extended form as the device kernel runs them, compiled
// with g++ (polydiv::Solo, one thread in place of the workgroup), against the schoolbook Euclid below (the reference's loop,
// _polys/_functions.py:40-57, on vectors).
//
// Pairs: every (deg a, deg b) in {0, 1, 63, 64, 65, 130}^2, dense and with zeroed interior coefficients, each also with leading
// zeros in front of both rows; a = 0, b = 0 and both; b | a, a = b; deg a < deg b (part of the grid); and remainder sequences
// built BACKWARDS from chosen quotients of 1, 64, 65 and 66 coefficients (the degree drops by 0, 63, 64 and 65), whose lengths the
// schoolbook loop is checked to reproduce.  Guard words surround every buffer.  Fields: a 32-bit prime and GF(5) (Prime32), and
// GF(p^2) for the largest prime below 2^32 (ExtP<2>).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_polygcd.h"

using namespace gfa;
using namespace gfa::polydiv;
using gfa::polytest::ExtP;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            std::exit(1);                                  \
        }                                                  \
    } while (0)

static FieldDev prime_field(u64 p)
{
    FieldDev fd = {};
    fd.p = fd.q = p;
    fd.m = 1;
    fd.kind = KIND_PRIME32;
    fd.mu = (u64)((((unsigned __int128)1) << 64) / p);
    return fd;
}

static FieldDev ext2_field(u64 p)
{
    FieldDev fd = prime_field(p);
    u32 a = 2;
    while (Prime32::pow_barrett(fd, a, (p - 1) / 2) == 1) a++; // a non-residue: x^2 - a is irreducible
    fd.q = p * p;
    fd.m = 2;
    fd.kind = KIND_EXT;
    fd.ext_irr[0] = 0;
    fd.ext_irr[1] = (u32)(p - a);
    return fd;
}

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u64 rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// ---- schoolbook polynomials: coefficients highest degree first, trimmed; the zero polynomial is empty -------------------------
template <class F>
struct Ref {
    typedef typename F::elem E;
    typedef std::vector<E> P;
    const FieldDev &fd;
    u64 q;

    P random(int degree, int zero_percent) const
    { // degree < 0: zero
        P v((size_t)(degree + 1));
        for (auto &x : v) x = (int)(rnd() % 100) < zero_percent ? (E)0 : (E)(rnd() % q);
        if (!v.empty())
            while (v[0] == 0) v[0] = (E)(rnd() % q);
        return v;
    }
    static P trim(P v)
    {
        size_t z = 0;
        while (z < v.size() && v[z] == 0) z++;
        return P(v.begin() + (long)z, v.end());
    }
    P sub(const P &x, const P &y) const
    {
        const size_t n = std::max(x.size(), y.size());
        P out(n, 0);
        for (size_t i = 0; i < n; i++) {
            const E a = i < n - x.size() ? (E)0 : x[i - (n - x.size())], b = i < n - y.size() ? (E)0 : y[i - (n - y.size())];
            out[i] = F::sub(fd, a, b);
        }
        return trim(out);
    }
    P add(const P &x, const P &y) const { return sub(x, sub(P(), y)); }
    P mul(const P &x, const P &y) const
    {
        if (x.empty() || y.empty()) return P();
        P out(x.size() + y.size() - 1, 0);
        for (size_t i = 0; i < x.size(); i++)
            for (size_t k = 0; k < y.size(); k++) out[i + k] = F::add(fd, out[i + k], F::mul(fd, x[i], y[k]));
        return trim(out);
    }
    void divmod(const P &x, const P &y, P &quo, P &rem) const
    { // y != 0
        if (x.size() < y.size()) {
            quo = P();
            rem = x;
            return;
        }
        P w = x;
        const size_t nq = x.size() - y.size() + 1;
        const E yinv = F::inv(fd, y[0]);
        for (size_t i = 0; i < nq; i++) {
            const E c = F::mul(fd, w[i], yinv);
            w[i] = c;
            for (size_t j = 1; j < y.size(); j++) w[i + j] = F::sub(fd, w[i + j], F::mul(fd, c, y[j]));
        }
        quo = trim(P(w.begin(), w.begin() + (long)nq));
        rem = trim(P(w.begin() + (long)nq, w.end()));
    }
    P scale_inv(const P &x, E c) const
    {
        P out = x;
        const E cinv = F::inv(fd, c);
        for (auto &v : out) v = F::mul(fd, v, cinv);
        return out;
    }
    // the reference's egcd; the quotient lengths of the steps go to `steps`
    void egcd(const P &a, const P &b, P &g, P &s, P &t, std::vector<int> *steps = nullptr) const
    {
        P r2 = a, r1 = b, s2 = {F::one(fd)}, s1, t2, t1 = {F::one(fd)};
        while (!r1.empty()) {
            P quo, rem;
            divmod(r2, r1, quo, rem);
            if (steps) steps->push_back((int)quo.size());
            P ns = sub(s2, mul(quo, s1)), nt = sub(t2, mul(quo, t1));
            r2 = r1, r1 = rem;
            s2 = s1, s1 = ns;
            t2 = t1, t1 = nt;
        }
        if (!r2.empty()) {
            const E c = r2[0];
            r2 = scale_inv(r2, c), s2 = scale_inv(s2, c), t2 = scale_inv(t2, c);
        }
        g = r2, s = s2, t = t2;
    }
};

// runs gfa_polygcd.h on (a, b) stored behind `pa` and `pb` leading zeros and compares with the schoolbook answer
template <class F>
static void one_pair(const Ref<F> &R, const typename Ref<F>::P &a, const typename Ref<F>::P &b, int pa, int pb, const char *name, const char *what)
{
    typedef typename F::elem E;
    typedef typename Ref<F>::P P;
    const int GUARD = 5;
    const E MARK = (E)0x5a5a5a5a;
    P g, s, t;
    R.egcd(a, b, g, s, t);
    CHECK(R.add(R.mul(a, s), R.mul(b, t)) == g, "%s %s: the schoolbook cofactors do not give the gcd", name, what);
    const int na = std::max((int)a.size() + pa, 1), nb = std::max((int)b.size() + pb, 1);
    for (int extended = 0; extended < 2; extended++) {
        // one allocation, in the kernel's order, with guard words between the buffers
        const int widths[6] = {na, nb, nb, nb, na, na};
        std::vector<E> mem;
        int off[6];
        for (int k = 0; k < 6; k++) {
            mem.insert(mem.end(), (size_t)GUARD, MARK);
            off[k] = (int)mem.size();
            mem.insert(mem.end(), (size_t)widths[k], k < 2 ? (E)0 : (E)0x33);
        }
        mem.insert(mem.end(), (size_t)GUARD, MARK);
        for (size_t i = 0; i < a.size(); i++) mem[(size_t)off[0] + (size_t)na - a.size() + i] = a[i];
        for (size_t i = 0; i < b.size(); i++) mem[(size_t)off[1] + (size_t)nb - b.size() + i] = b[i];
        int slot = -7;
        E *m = mem.data();
        const polygcd::Result<E> res = polygcd::euclid<F, Solo>(R.fd, m + off[0], na, m + off[1], nb, extended ? m + off[2] : nullptr, extended ? m + off[3] : nullptr,
                                                              extended ? m + off[4] : nullptr, extended ? m + off[5] : nullptr, extended != 0, &slot, Solo());
        CHECK(res.len == (int)g.size(), "%s %s: gcd of degree %d, expected %d (extended %d)", name, what, res.len - 1, (int)g.size() - 1, extended);
        for (int i = 0; i < res.len; i++) CHECK(res.r[i] == g[(size_t)i], "%s %s: gcd coefficient %d (extended %d)", name, what, i, extended);
        if (extended) {
            CHECK(res.ls <= nb && res.lt <= na, "%s %s: cofactor lengths", name, what);
            for (int j = 0; j < nb; j++) {
                const E got = j < res.ls ? res.s[nb - 1 - j] : (E)0, want = j < (int)s.size() ? s[s.size() - 1 - (size_t)j] : (E)0;
                CHECK(got == want, "%s %s: s, coefficient of x^%d", name, what, j);
            }
            for (int j = 0; j < na; j++) {
                const E got = j < res.lt ? res.t[na - 1 - j] : (E)0, want = j < (int)t.size() ? t[t.size() - 1 - (size_t)j] : (E)0;
                CHECK(got == want, "%s %s: t, coefficient of x^%d", name, what, j);
            }
        }
        size_t at = 0;
        for (int k = 0; k <= 6; k++) {
            for (int gd = 0; gd < GUARD; gd++) CHECK(mem[at + (size_t)gd] == MARK, "%s %s: guard %d (extended %d)", name, what, k, extended);
            if (k < 6) {
                at += (size_t)GUARD + (size_t)widths[k];
                if (!extended && k >= 2)
                    for (int i = 0; i < widths[k]; i++) CHECK(mem[(size_t)off[k] + (size_t)i] == (E)0x33, "%s %s: a cofactor buffer was written without being asked for", name, what);
            }
        }
    }
}

template <class F>
static void field_cases(const FieldDev &fd, u64 q, const char *name)
{
    typedef typename Ref<F>::P P;
    const Ref<F> R{fd, q};
    int cases = 0;
    const int degs[6] = {0, 1, 63, 64, 65, 130};
    for (int da : degs)
        for (int db : degs)
            for (int rep = 0; rep < 3; rep++) { // dense; sparse; sparse behind leading zeros
                const P a = R.random(da, rep ? 50 : 0), b = R.random(db, rep ? 50 : 0);
                one_pair<F>(R, a, b, rep == 2 ? 3 : 0, rep == 2 ? 66 : 0, name, "grid");
                cases++;
            }
    // zero operands
    for (int d : {0, 1, 64, 130}) {
        one_pair<F>(R, P(), R.random(d, 30), d + 1, 0, name, "a = 0");
        one_pair<F>(R, R.random(d, 30), P(), 0, d + 1, name, "b = 0");
        one_pair<F>(R, P(), P(), d + 1, 1, name, "a = b = 0");
        one_pair<F>(R, R.random(d, 30), P(), 2, 1, name, "b = 0, short");
        cases += 4;
    }
    // b | a, a = b, a = c b, and a common factor of degree 64 in both
    for (int d : {1, 63, 64, 65}) {
        const P b = R.random(d, 30), u = R.random(67, 30), v = R.random(3, 0), c = R.random(0, 0);
        one_pair<F>(R, R.mul(b, u), b, 0, 0, name, "b | a");
        one_pair<F>(R, b, R.mul(b, u), 1, 0, name, "a | b");
        one_pair<F>(R, b, b, 0, 2, name, "a = b");
        one_pair<F>(R, R.mul(b, c), b, 0, 0, name, "a = c b");
        one_pair<F>(R, R.mul(b, u), R.mul(b, v), 0, 0, name, "planted");
        cases += 5;
    }
    // remainder sequences with chosen quotients: r[i-1] = q[i] r[i] + r[i+1], backwards from the gcd
    const std::vector<std::vector<int>> plans = {{1, 2, 66, 2, 65, 3, 64, 2}, {64, 64}, {65, 2, 2, 66}, {1, 66, 65, 64, 2}, {66}};
    for (const auto &plan : plans) {
        P next, cur = R.random(2, 0); // the last non-zero remainder
        for (size_t i = plan.size(); i-- > 0;) {
            const P prev = R.add(R.mul(R.random(plan[i] - 1, 40), cur), next);
            next = cur, cur = prev;
        }
        P g, s, t;
        std::vector<int> steps;
        R.egcd(cur, next, g, s, t, &steps);
        CHECK(steps == plan && g.size() == 3, "%s: the built sequence does not have the chosen quotients", name);
        one_pair<F>(R, cur, next, 0, 0, name, "chosen quotients");
        one_pair<F>(R, next, cur, 1, 0, name, "chosen quotients, swapped");
        cases += 2;
    }
    std::printf("%s: %d euclid cases\n", name, cases);
}

int main()
{
    field_cases<Prime32>(prime_field(5), 5, "GF(5)");
    field_cases<Prime32>(prime_field(4294967291ull), 4294967291ull, "GF(4294967291)");
    const FieldDev e2 = ext2_field(4294967291ull);
    field_cases<ExtP<2>>(e2, e2.q, "GF(4294967291^2)");
    std::printf("polygcd host model ok\n");
    return 0;
}
