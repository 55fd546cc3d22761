// Host model of galois_amd/csrc/gfa_polyroots.h: the slot rule, the rank sort and the repeated synthetic division of the finishing
// kernel, compiled with g++ (polydiv::Solo, one thread in place of the workgroup), against a schoolbook count of the factors
// (x - r): long division by x - r on vectors, repeated while it is exact.
//
// Per field: products of (x - r)^m over chosen roots with every multiplicity in {1, p - 1, p, p + 1, 2 p} (p the characteristic;
// capped for the 32-bit prime), times a cofactor without roots, with and without leading zeros; a row whose capacity is exactly
// full (x^q - x over the small fields: q roots in q slots; a product of cap distinct linear factors over the large one); a row
// with no roots, a constant row and the zero row; elements that are no roots (multiplicity 0); slots claimed in scrambled order,
// with more claims than the capacity, and with a counter that has wrapped.  Guard words surround every buffer.
// Fields: GF(2), GF(3), GF(5), GF(4294967291) (Prime32) and GF(4) (Bin).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_polyroots.h"

using namespace gfa;
using gfa::polydiv::Solo;

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

static FieldDev gf4()
{
    FieldDev fd = {};
    fd.p = 2;
    fd.q = 4;
    fd.m = 2;
    fd.kind = KIND_BIN;
    fd.irr = 7; // x^2 + x + 1
    return fd;
}

static u64 rng_state = 0x2545f4914f6cdd1dull;
static u64 rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// ---- schoolbook: coefficients highest degree first ------------------------------------------------------------------------------
template <class F>
struct Ref {
    typedef typename F::elem E;
    typedef std::vector<E> P;
    const FieldDev &fd;
    u64 q;

    P mul(const P &x, const P &y) const
    {
        P out(x.size() + y.size() - 1, 0);
        for (size_t i = 0; i < x.size(); i++)
            for (size_t k = 0; k < y.size(); k++) out[i + k] = F::add(fd, out[i + k], F::mul(fd, x[i], y[k]));
        return out;
    }
    P linear(E r) const { return P{F::one(fd), F::sub(fd, 0, r)}; }
    E eval(const P &f, E x) const
    {
        E acc = 0;
        for (E c : f) acc = F::add(fd, F::mul(fd, acc, x), c);
        return acc;
    }
    static bool is_zero(const P &f) { return std::all_of(f.begin(), f.end(), [](E c) { return c == 0; }); }
    // how often x - r divides f != 0: long division by the monic x - r, column by column, while the remainder is zero
    int count_factors(P f, E r) const
    {
        const P d = linear(r);
        int m = 0;
        for (;;) {
            P w = f;
            for (size_t i = 0; i + 1 < w.size(); i++) w[i + 1] = F::sub(fd, w[i + 1], F::mul(fd, w[i], d[1]));
            if (w.size() < 2 || w.back() != 0) return m;
            m++;
            w.pop_back();
            f = w;
        }
    }
    // a polynomial of the degree without roots in the field, found by trying (degree >= 2; small q) or x^2 - (non-residue)
    P rootless(int degree) const
    {
        if (q > 1000) {
            E a = 2;
            while (Prime32::pow_barrett(fd, (u32)a, (q - 1) / 2) == 1) a++;
            return P{F::one(fd), 0, F::sub(fd, 0, a)};
        }
        for (;;) {
            P f((size_t)degree + 1);
            for (auto &c : f) c = (E)(rnd() % q);
            f[0] = F::one(fd);
            bool none = true;
            for (u64 x = 0; x < q; x++) none = none && eval(f, (E)x) != 0;
            if (none) return f;
        }
    }
};

struct VecStore {
    std::vector<u64> *v;
    int off;
    void set(int i, u64 r) const { (*v)[(size_t)(off + i)] = r; }
};
struct VecMult {
    int *p;
    void set(int i, int m) const { p[i] = m; }
};

// One row through the header as the two kernels use it: the hits of f among `candidates` (every element for the small fields)
// claim slots in scrambled order, `extra` further claims arrive beyond them, finish_row sorts and counts.
template <class F>
static void one_row(const Ref<F> &R, const typename Ref<F>::P &f, std::vector<typename F::elem> candidates, int extra, u32 counter_start, const char *name,
                    const char *what)
{
    typedef typename F::elem E;
    const int GUARD = 4, ncoef = (int)f.size(), cap = ncoef - 1;
    const u64 MARK = 0x5a5a5a5a5a5a5a5aull;
    const bool zero = Ref<F>::is_zero(f);
    // expected
    std::sort(candidates.begin(), candidates.end());
    candidates.erase(std::unique(candidates.begin(), candidates.end()), candidates.end());
    std::vector<E> want_r;
    std::vector<int> want_m;
    if (!zero)
        for (E x : candidates)
            if (R.eval(f, x) == 0) {
                want_r.push_back(x);
                want_m.push_back(R.count_factors(f, x));
            }
    CHECK((int)want_r.size() <= cap || zero, "%s %s: more roots than the degree", name, what);
    // the search's side: slots in a guarded row
    std::vector<u64> row((size_t)(cap + 2 * GUARD), MARK);
    for (int i = 0; i < cap; i++) row[(size_t)(GUARD + i)] = 0;
    std::vector<E> hits;
    for (E x : candidates)
        if (R.eval(f, x) == 0) hits.push_back(x);
    for (size_t i = hits.size(); i > 1; i--) std::swap(hits[i - 1], hits[rnd() % i]);
    u32 counter = counter_start;
    const VecStore store{&row, GUARD};
    for (E x : hits) polyroots::take_slot(store, cap, counter++, (u64)x);
    for (int i = 0; i < extra; i++) polyroots::take_slot(store, cap, counter++, (u64)0x77);
    for (int gd = 0; gd < GUARD; gd++) CHECK(row[(size_t)gd] == MARK && row[(size_t)(GUARD + cap + gd)] == MARK, "%s %s: a slot outside the row was written", name, what);
    if (counter_start != 0) { // a wrapped counter: nothing below the capacity was handed out, nothing may be stored
        for (int i = 0; i < cap; i++) CHECK(row[(size_t)(GUARD + i)] == 0, "%s %s: a slot at or above the capacity was stored", name, what);
        return;
    }
    // the finishing side: c | slots | sorted | work, guard words between
    const int lanes = 3;
    const int widths[4] = {ncoef, cap, cap, lanes * ncoef};
    std::vector<E> mem;
    int off[4];
    for (int k = 0; k < 4; k++) {
        mem.insert(mem.end(), (size_t)GUARD, (E)MARK);
        off[k] = (int)mem.size();
        mem.insert(mem.end(), (size_t)widths[k], (E)0x33);
    }
    mem.insert(mem.end(), (size_t)GUARD, (E)MARK);
    for (int i = 0; i < ncoef; i++) mem[(size_t)(off[0] + i)] = f[(size_t)i];
    for (int i = 0; i < cap; i++) mem[(size_t)(off[1] + i)] = (E)row[(size_t)(GUARD + i)];
    std::vector<int> mult((size_t)(cap + 2 * GUARD), -9);
    E *m = mem.data();
    const Solo g;
    CHECK(polyroots::share_is_zero(m + off[0], ncoef, g) == zero, "%s %s: zero row", name, what);
    for (int want_mult = 0; want_mult < 2; want_mult++) {
        const int n = polyroots::finish_row<F, VecMult, Solo>(R.fd, m + off[0], ncoef, zero, m + off[1], counter, m + off[2], m + off[3], lanes, want_mult != 0,
                                                             VecMult{mult.data() + GUARD}, g);
        if (zero) {
            CHECK(n == -1, "%s %s: the zero row must report -1, not %d", name, what, n);
            for (int i = 0; i < cap; i++) CHECK(m[off[2] + i] == (E)0x33 && mult[(size_t)(GUARD + i)] == -9, "%s %s: the zero row was written to", name, what);
            continue;
        }
        CHECK(n == (int)want_r.size(), "%s %s: %d roots, expected %d", name, what, n, (int)want_r.size());
        for (int i = 0; i < n; i++) {
            CHECK(m[off[2] + i] == want_r[(size_t)i], "%s %s: root %d", name, what, i);
            if (want_mult) CHECK(mult[(size_t)(GUARD + i)] == want_m[(size_t)i], "%s %s: multiplicity of root %d is %d, expected %d", name, what, i, mult[(size_t)(GUARD + i)], want_m[(size_t)i]);
            else CHECK(mult[(size_t)(GUARD + i)] == -9, "%s %s: a multiplicity was written without being asked for", name, what);
        }
        for (int i = n; i < cap; i++) CHECK(mult[(size_t)(GUARD + i)] == -9, "%s %s: a multiplicity behind the roots", name, what);
    }
    for (int gd = 0; gd < GUARD; gd++) CHECK(mult[(size_t)gd] == -9 && mult[(size_t)(GUARD + cap + gd)] == -9, "%s %s: multiplicity guard", name, what);
    size_t at = 0;
    for (int k = 0; k <= 4; k++) {
        for (int gd = 0; gd < GUARD; gd++) CHECK(mem[at + (size_t)gd] == (E)MARK, "%s %s: guard %d", name, what, k);
        if (k < 4) at += (size_t)GUARD + (size_t)widths[k];
    }
    for (int i = 0; i < ncoef; i++) CHECK(mem[(size_t)(off[0] + i)] == f[(size_t)i], "%s %s: the row was modified", name, what);
    // elements that are no roots have multiplicity 0, roots given unsorted and twice keep theirs
    std::vector<E> given = want_r;
    given.insert(given.end(), want_r.rbegin(), want_r.rend());
    for (E x : candidates)
        if (R.eval(f, x) != 0 && given.size() < want_r.size() * 2 + 3) given.push_back(x);
    std::vector<int> gm(given.size(), -9);
    polyroots::multiplicities<F, VecMult, Solo>(R.fd, m + off[0], ncoef, given.data(), (int)given.size(), m + off[3], lanes, VecMult{gm.data()}, g);
    for (size_t i = 0; i < given.size(); i++) CHECK(gm[i] == R.count_factors(f, given[i]), "%s %s: given element %zu", name, what, i);
}

template <class F>
static void field_cases(const FieldDev &fd, u64 q, const char *name)
{
    typedef typename F::elem E;
    typedef typename Ref<F>::P P;
    const Ref<F> R{fd, q};
    const bool small = q <= 1000;
    const int p = (int)std::min<u64>(fd.p, 5); // multiplicities around the characteristic; around 5 for the 32-bit prime
    std::vector<E> all;
    if (small)
        for (u64 x = 0; x < q; x++) all.push_back((E)x);
    const std::vector<E> picks = small ? all : std::vector<E>{0, 1, 2, (E)(q - 1), (E)(q - 2), (E)(q / 2), 64, 65};
    int cases = 0;
    const P cof = R.rootless(small ? 2 : 2);
    for (int m : {1, p - 1, p, p + 1, 2 * p}) {
        if (m < 1) continue;
        // one root of multiplicity m beside the others with multiplicity 1 and 2, times a cofactor without roots
        for (size_t lead = 0; lead < picks.size() && lead < 4; lead++) {
            P f = cof;
            std::vector<E> cand = small ? all : picks;
            for (size_t i = 0; i < picks.size() && i < 4; i++) {
                const int mi = i == lead ? m : 1 + (int)(i % 2);
                for (int k = 0; k < mi; k++) f = R.mul(f, R.linear(picks[i]));
            }
            one_row<F>(R, f, cand, 0, 0, name, "multiplicities");
            P padded(3, 0);
            padded.insert(padded.end(), f.begin(), f.end());
            one_row<F>(R, padded, cand, 0, 0, name, "multiplicities behind leading zeros");
            cases += 2;
        }
        // a single root of multiplicity m and nothing else: the quotient shrinks to a constant
        P f{F::one(fd)};
        for (int k = 0; k < m; k++) f = R.mul(f, R.linear(picks[1]));
        one_row<F>(R, f, small ? all : picks, 0, 0, name, "(x - r)^m");
        cases++;
    }
    // capacity exactly full: as many distinct roots as slots
    {
        P f{F::one(fd)};
        for (E r : picks) f = R.mul(f, R.linear(r));
        one_row<F>(R, f, small ? all : picks, 0, 0, name, "capacity full");
        one_row<F>(R, f, small ? all : picks, 5, 0, name, "capacity full and five claims more");
        one_row<F>(R, f, small ? all : picks, 0, 0xfffffff0u, name, "a counter above 2^31");
        cases += 3;
    }
    // no roots, a constant behind leading zeros, the zero row (every candidate claims a slot)
    one_row<F>(R, cof, small ? all : picks, 0, 0, name, "no roots");
    one_row<F>(R, P{0, 0, 0, F::one(fd)}, small ? all : picks, 0, 0, name, "constant");
    one_row<F>(R, P{0, 0, 0}, small ? all : picks, 0, 0, name, "zero row");
    one_row<F>(R, P{0, 0}, small ? all : picks, 7, 0, name, "zero row, one slot");
    cases += 4;
    std::printf("%s: %d root cases\n", name, cases);
}

int main()
{
    field_cases<Prime32>(prime_field(2), 2, "GF(2)");
    field_cases<Prime32>(prime_field(3), 3, "GF(3)");
    field_cases<Prime32>(prime_field(5), 5, "GF(5)");
    field_cases<Bin>(gf4(), 4, "GF(4)");
    field_cases<Prime32>(prime_field(4294967291ull), 4294967291ull, "GF(4294967291)");
    std::printf("polyroots host model ok\n");
    return 0;
}
