// Host model of galois_amd/csrc/gfa_polydiv.h: the blocked division and the modular power the device kernels run, compiled
// with g++ (one thread in place of the workgroup).
//
// Division: every combination of quotient length in {1, K-1, K, K+1, 2K+3} and divisor length in {1, 2, K, K+1, 3K+5}, several
// sparse operands each (zero quotient digits, zero interior divisor coefficients, leading zeros in the dividend), against the
// schoolbook loop below -- through the linear view and through the circular window (with guard words on both sides), with and
// without quotients.  Power: against repeated multiply-and-reduce, and right-to-left binary powers for two-word exponents.
// Fields: GF(3), GF(5) and a 32-bit prime (Prime32), GF(4) on a table, GF(p^2) for the largest prime below 2^32 (ExtP<2>).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_polydiv.h"

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

static u64 rng_state = 88172645463325252ull;
static u64 rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

template <class E>
struct Arr {
    const E *p;
    E operator[](int i) const { return p[i]; }
};
template <class E>
struct QOut {
    E *p;
    void set(int i, E v) const { p[i] = v; }
};

template <class E>
static std::vector<E> sparse(u64 q, int n, int zero_percent)
{
    std::vector<E> v((size_t)n);
    for (auto &x : v) x = (int)(rnd() % 100) < zero_percent ? (E)0 : (E)(rnd() % q);
    return v;
}

// the reference's loop (divmod_jit.implementation), in place: quotient in w[0 .. nq), remainder behind it
template <class F>
static void schoolbook(const FieldDev &fd, std::vector<typename F::elem> &w, const std::vector<typename F::elem> &b)
{
    typedef typename F::elem E;
    const int nq = (int)w.size() - (int)b.size() + 1;
    const E binv = F::inv(fd, b[0]);
    for (int i = 0; i < nq; i++) {
        if (w[i] == 0) continue;
        const E q = F::mul(fd, w[i], binv);
        for (size_t j = 1; j < b.size(); j++) w[i + j] = F::sub(fd, w[i + j], F::mul(fd, q, b[j]));
        w[i] = q;
    }
}

template <class F>
static std::vector<typename F::elem> product(const FieldDev &fd, const std::vector<typename F::elem> &x, const std::vector<typename F::elem> &y)
{
    std::vector<typename F::elem> out(x.size() + y.size() - 1, 0);
    for (size_t i = 0; i < x.size(); i++)
        for (size_t k = 0; k < y.size(); k++) out[i + k] = F::add(fd, out[i + k], F::mul(fd, x[i], y[k]));
    return out;
}

template <class F>
static int division_cases(const FieldDev &fd, u64 q, const char *name)
{
    typedef typename F::elem E;
    const int K = PD_K, GUARD = 7;
    const E MARK = (E)0x5a5a5a5a;
    const int nqs[5] = {1, K - 1, K, K + 1, 2 * K + 3}, nbs[5] = {1, 2, K, K + 1, 3 * K + 5};
    int cases = 0;
    for (int nq : nqs)
        for (int nb : nbs)
            for (int rep = 0; rep < 4; rep++) {
                const int na = nq + nb - 1;
                // a = quo b + rem with sparse parts; rep 1: the quotient starts with zeros, so the dividend has leading zeros
                std::vector<E> b = sparse<E>(q, nb, rep == 3 ? 0 : 60), quo = sparse<E>(q, nq, rep == 2 ? 85 : 50), rem = sparse<E>(q, nb - 1, 50);
                while (b[0] == 0) b[0] = (E)(rnd() % q);
                if (rep == 1)
                    for (int i = 0; i < (nq + 1) / 2; i++) quo[i] = 0;
                std::vector<E> a = product<F>(fd, quo, b);
                for (int j = 0; j < nb - 1; j++) a[nq + j] = F::add(fd, a[nq + j], rem[j]);
                std::vector<E> expect = a;
                schoolbook<F>(fd, expect, b);
                for (int i = 0; i < nq; i++) CHECK(expect[i] == quo[i], "%s: schoolbook quotient, nq %d nb %d", name, nq, nb);
                for (int j = 0; j < nb - 1; j++) CHECK(expect[nq + j] == rem[j], "%s: schoolbook remainder, nq %d nb %d", name, nq, nb);

                for (int want_q = 0; want_q < 2; want_q++) {
                    // linear view, loaded from a
                    std::vector<E> lin((size_t)(na + 2 * GUARD), MARK), qo((size_t)(nq + 2 * GUARD), MARK);
                    const Lin<E> R = divide<F, Lin<E>, Arr<E>, Arr<E>, QOut<E>, Solo>(fd, Lin<E>{lin.data() + GUARD}, Arr<E>{b.data()}, Arr<E>{a.data()}, na, nb,
                                                                                  QOut<E>{qo.data() + GUARD}, want_q != 0, true, Solo());
                    CHECK(R.p == lin.data() + GUARD + nq, "%s: linear view not advanced by nq", name);
                    for (int j = 0; j < nb - 1; j++) CHECK(R[j] == rem[j], "%s: linear remainder %d, nq %d nb %d rep %d", name, j, nq, nb, rep);
                    for (int i = 0; i < nq; i++) CHECK(lin[GUARD + i] == quo[i], "%s: linear quotient in place %d, nq %d nb %d rep %d", name, i, nq, nb, rep);
                    for (int i = 0; i < nq; i++) CHECK(qo[GUARD + i] == (want_q ? quo[i] : MARK), "%s: linear quotient out %d, nq %d nb %d", name, i, nq, nb);
                    for (int gd = 0; gd < GUARD; gd++)
                        CHECK(lin[gd] == MARK && lin[GUARD + na + gd] == MARK && qo[gd] == MARK && qo[GUARD + nq + gd] == MARK, "%s: linear guard, nq %d nb %d", name, nq, nb);

                    // circular window of nb - 1 + 2 K coefficients, started at an offset so that it wraps early
                    const int cap = nb - 1 + 2 * K;
                    std::vector<E> ring((size_t)(cap + 2 * GUARD), MARK);
                    std::fill(qo.begin(), qo.end(), MARK);
                    const Ring<E> W{ring.data() + GUARD, cap, (int)(rnd() % (u64)cap)};
                    const Ring<E> RR = divide<F, Ring<E>, Arr<E>, Arr<E>, QOut<E>, Solo>(fd, W, Arr<E>{b.data()}, Arr<E>{a.data()}, na, nb, QOut<E>{qo.data() + GUARD},
                                                                                     want_q != 0, true, Solo());
                    for (int j = 0; j < nb - 1; j++) CHECK(RR[j] == rem[j], "%s: ring remainder %d, nq %d nb %d rep %d", name, j, nq, nb, rep);
                    for (int i = 0; i < nq; i++) CHECK(qo[GUARD + i] == (want_q ? quo[i] : MARK), "%s: ring quotient %d, nq %d nb %d rep %d", name, i, nq, nb, rep);
                    for (int gd = 0; gd < GUARD; gd++)
                        CHECK(ring[gd] == MARK && ring[GUARD + cap + gd] == MARK && qo[gd] == MARK && qo[GUARD + nq + gd] == MARK, "%s: ring guard, nq %d nb %d", name, nq, nb);
                }
                // in place, nothing loaded (the form the power uses)
                std::vector<E> w = a;
                const Lin<E> R2 = divide<F, Lin<E>, Arr<E>, NoSource, NoQuotient, Solo>(fd, Lin<E>{w.data()}, Arr<E>{b.data()}, NoSource(), na, nb, NoQuotient(), false,
                                                                                   false, Solo());
                for (int j = 0; j < nb - 1; j++) CHECK(R2[j] == rem[j], "%s: in-place remainder %d, nq %d nb %d", name, j, nq, nb);
                cases++;
            }
    // a zero leading coefficient is a caller error: the call ends, inside its buffers
    {
        std::vector<E> b = sparse<E>(q, K + 1, 0), a = sparse<E>(q, 3 * K, 0), lin((size_t)(3 * K + 2), MARK);
        b[0] = 0;
        divide<F, Lin<E>, Arr<E>, Arr<E>, NoQuotient, Solo>(fd, Lin<E>{lin.data() + 1}, Arr<E>{b.data()}, Arr<E>{a.data()}, 3 * K, K + 1, NoQuotient(), false, true, Solo());
        CHECK(lin[0] == MARK && lin[3 * K + 1] == MARK, "%s: zero leading coefficient", name);
    }
    std::printf("%s: %d division cases\n", name, cases);
    return cases;
}

// x mod c for a polynomial of any length (zero-padded to d coefficients when shorter)
template <class F>
static std::vector<typename F::elem> reduce(const FieldDev &fd, std::vector<typename F::elem> x, const std::vector<typename F::elem> &c)
{
    typedef typename F::elem E;
    const size_t d = c.size() - 1;
    if (x.size() < c.size()) {
        std::vector<E> out(d - x.size(), 0);
        out.insert(out.end(), x.begin(), x.end());
        return out;
    }
    schoolbook<F>(fd, x, c);
    return std::vector<E>(x.end() - (long)d, x.end());
}

template <class F>
static int power_cases(const FieldDev &fd, u64 q, const char *name)
{
    typedef typename F::elem E;
    const int K = PD_K;
    int cases = 0;
    for (int d : {1, 2, 5, K, K + 1}) {
        std::vector<E> c = sparse<E>(q, d + 1, 40), base = sparse<E>(q, d, 30);
        while (c[0] == 0) c[0] = (E)(rnd() % q);
        std::vector<E> one((size_t)d, 0);
        one[d - 1] = F::one(fd);
        // repeated multiply-and-reduce for e = 0 .. 9
        std::vector<std::vector<E>> by_steps = {one};
        for (int e = 1; e < 10; e++) by_steps.push_back(reduce<F>(fd, product<F>(fd, by_steps.back(), base), c));
        auto run = [&](const std::vector<E> &bs, const u64 *e, int limbs) {
            std::vector<E> r((size_t)d, (E)7), bb = bs, P((size_t)(2 * d + 1), (E)0x77);
            power<F, Arr<E>, Solo>(fd, Lin<E>{r.data()}, Lin<E>{bb.data()}, Lin<E>{P.data()}, Arr<E>{c.data()}, d, e, limbs, Solo());
            CHECK(bb == bs, "%s: the base was modified", name);
            CHECK(P[2 * d - 1] == (E)0x77 && P[2 * d] == (E)0x77, "%s: the product buffer was overrun, degree %d", name, d);
            return r;
        };
        for (int e = 0; e < 10; e++) {
            const u64 limbs[2] = {(u64)e, 0};
            CHECK(run(base, limbs, 1) == by_steps[e], "%s: degree %d, exponent %d", name, d, e);
            CHECK(run(base, limbs, 2) == by_steps[e], "%s: degree %d, exponent %d with an empty high word", name, d, e);
            cases += 2;
        }
        const u64 zero = 0;
        CHECK(run(std::vector<E>((size_t)d, 0), &zero, 1) == one, "%s: 0^0", name);
        // right-to-left binary powers for exponents of one and two words
        const u64 big[3][2] = {{1000003, 0}, {1234, 1}, {0x8000000000000001ull, 0x41}};
        for (const auto &e : big) {
            std::vector<E> acc = one, sq = base;
            for (int bit = 0; bit < 128; bit++) {
                if ((e[bit >> 6] >> (bit & 63)) & 1) acc = reduce<F>(fd, product<F>(fd, acc, sq), c);
                sq = reduce<F>(fd, product<F>(fd, sq, sq), c);
            }
            CHECK(run(base, e, 2) == acc, "%s: degree %d, exponent %llu + 2^64 %llu", name, d, (unsigned long long)e[0], (unsigned long long)e[1]);
            cases++;
        }
    }
    std::printf("%s: %d power cases\n", name, cases);
    return cases;
}

template <class F>
static void field_cases(const FieldDev &fd, u64 q, const char *name)
{
    CHECK(division_cases<F>(fd, q, name) == 100, "%s: case count", name);
    power_cases<F>(fd, q, name);
}

int main()
{
    field_cases<Prime32>(prime_field(3), 3, "GF(3)");
    field_cases<Prime32>(prime_field(5), 5, "GF(5)");
    field_cases<Prime32>(prime_field(4294967291ull), 4294967291ull, "GF(4294967291)");
    FieldDev fd4 = {};
    fd4.p = 2; fd4.q = 4; fd4.m = 2;
    field_cases<GF4>(fd4, 4, "GF(4)");
    const FieldDev e2 = ext2_field(4294967291ull);
    field_cases<ExtP<2>>(e2, e2.q, "GF(4294967291^2)");
    std::printf("polydiv host model ok\n");
    return 0;
}
