// Host model of galois_amd/csrc/gfa_lagrange.h: the weights, the duplicate flag and the sweeps of the interpolation kernel,
// compiled with g++, against a schoolbook solve of the Vandermonde system V c = y, V[i][j] = x_i^(k - 1 - j), by Gauss-Jordan
// elimination written here (and against Horner evaluation of the result at every point).
//
// Per field: every k from 1 to min(q, 9) and k = q (k = 33 over the 32-bit prime, whose q points do not fit), each with random,
// all-zero and constant y, with x drawn with and without 0; each row once by lagrange::row on polydiv::Solo (one thread strides
// over all points) and once phase by phase on teams of 2, 3, k and k + 3 threads whose threads run in increasing and in
// decreasing order between the ordering points (fewer threads than points stride); a repeated x in the first, middle and last
// position, which must raise the flag and give a zero row.  Guard words surround the row's memory and the output.
// Fields: GF(2), GF(3), GF(5), GF(4294967291) (Prime32) and GF(4) (Bin).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_lagrange.h"

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

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u64 rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// ---- schoolbook ---------------------------------------------------------------------------------------------------------------
// the coefficients (highest degree first) of the polynomial of degree < k through the points, x distinct: Gauss-Jordan on [V | y]
template <class F>
static std::vector<typename F::elem> vandermonde_solve(const FieldDev &fd, const std::vector<typename F::elem> &x, const std::vector<typename F::elem> &y)
{
    typedef typename F::elem E;
    const size_t k = x.size();
    std::vector<std::vector<E>> A(k, std::vector<E>(k + 1));
    for (size_t i = 0; i < k; i++) {
        E pw = F::one(fd);
        for (size_t j = k; j-- > 0;) {
            A[i][j] = pw;
            pw = F::mul(fd, pw, x[i]);
        }
        A[i][k] = y[i];
    }
    for (size_t col = 0; col < k; col++) {
        size_t piv = col;
        while (piv < k && A[piv][col] == 0) piv++;
        CHECK(piv < k, "singular Vandermonde matrix: the test's own x repeat");
        std::swap(A[piv], A[col]);
        const E inv = F::inv(fd, A[col][col]);
        for (size_t j = col; j <= k; j++) A[col][j] = F::mul(fd, A[col][j], inv);
        for (size_t i = 0; i < k; i++) {
            if (i == col || A[i][col] == 0) continue;
            const E f = A[i][col];
            for (size_t j = col; j <= k; j++) A[i][j] = F::sub(fd, A[i][j], F::mul(fd, f, A[col][j]));
        }
    }
    std::vector<E> c(k);
    for (size_t i = 0; i < k; i++) c[i] = A[i][k];
    return c;
}

template <class F>
static typename F::elem horner(const FieldDev &fd, const std::vector<typename F::elem> &c, typename F::elem x)
{
    typename F::elem acc = 0;
    for (auto v : c) acc = F::add(fd, F::mul(fd, acc, x), v);
    return acc;
}

// ---- the header ------------------------------------------------------------------------------------------------------------------
struct VecOut {
    std::vector<u64> *v;
    int off;
    void set(int i, u64 c) const { (*v)[(size_t)(off + i)] = c; }
};

struct Member { // one thread of a team of n; the caller is the ordering point
    int tid, n;
    void sync() const {}
};

// One row through the header on a team of `n` threads (0: lagrange::row on Solo).  Returns the flag; `got` receives the k
// coefficients.
template <class F>
static bool interpolate(const FieldDev &fd, const std::vector<typename F::elem> &x, const std::vector<typename F::elem> &y, int n, bool reverse,
                        std::vector<typename F::elem> *got, const char *name, const char *what)
{
    typedef typename F::elem E;
    const int GUARD = 4, k = (int)x.size(), len = lagrange::LG_ARRAYS * k + 1;
    const E MARK = (E)0x5a5a5a5a5a5a5a5aull;
    std::vector<E> mem((size_t)(len + 2 * GUARD), MARK);
    std::vector<u64> out((size_t)(k + 2 * GUARD), 0x7777);
    const lagrange::Row<E> r = lagrange::carve(mem.data() + GUARD, k);
    const VecOut store{&out, GUARD};
    bool dup;
    if (n == 0) {
        dup = lagrange::row<F, const E *, const E *, VecOut, Solo>(fd, r, k, x.data(), y.data(), store, true, Solo());
    } else {
        auto each = [&](auto phase) {
            for (int t = 0; t < n; t++) phase(Member{reverse ? n - 1 - t : t, n});
        };
        each([&](Member g) { lagrange::load<F, const E *, const E *, Member>(fd, r, k, x.data(), y.data(), g); });
        each([&](Member g) { lagrange::weights<F, Member>(fd, r, k, g); });
        for (int s = 0; s < k; s++) each([&](Member g) { lagrange::sweep<F, Member>(fd, r, k, s, g); });
        dup = *r.dup != 0;
        each([&](Member g) { lagrange::store<E, VecOut, Member>(r, k, dup, store, g); });
    }
    for (int gd = 0; gd < GUARD; gd++) {
        CHECK(mem[(size_t)gd] == MARK && mem[(size_t)(GUARD + len + gd)] == MARK, "%s %s: the row's memory was left (team %d)", name, what, n);
        CHECK(out[(size_t)gd] == 0x7777 && out[(size_t)(GUARD + k + gd)] == 0x7777, "%s %s: the output row was left (team %d)", name, what, n);
    }
    for (int i = 0; i < k; i++) CHECK(mem[(size_t)(GUARD + i)] == x[(size_t)i], "%s %s: x was modified", name, what);
    got->resize((size_t)k);
    for (int i = 0; i < k; i++) (*got)[(size_t)i] = (E)out[(size_t)(GUARD + i)];
    return dup;
}

// every team size on one point set; returns the number of runs
template <class F>
static int one_set(const FieldDev &fd, const std::vector<typename F::elem> &x, const std::vector<typename F::elem> &y, bool repeated, const char *name, const char *what)
{
    typedef typename F::elem E;
    const int k = (int)x.size();
    std::vector<E> want((size_t)k, 0);
    if (!repeated) {
        want = vandermonde_solve<F>(fd, x, y);
        for (int i = 0; i < k; i++) CHECK(horner<F>(fd, want, x[(size_t)i]) == y[(size_t)i], "%s %s: the schoolbook solution misses point %d", name, what, i);
    }
    int runs = 0;
    for (int n : {0, 2, 3, k, k + 3})
        for (int reverse = 0; reverse < (n ? 2 : 1); reverse++) {
            std::vector<E> got;
            const bool dup = interpolate<F>(fd, x, y, n, reverse != 0, &got, name, what);
            CHECK(dup == repeated, "%s %s: k = %d, team %d: flag %d, expected %d", name, what, k, n, (int)dup, (int)repeated);
            for (int i = 0; i < k; i++)
                CHECK(got[(size_t)i] == want[(size_t)i], "%s %s: k = %d, team %d: coefficient %d is %llu, expected %llu", name, what, k, n, i,
                      (unsigned long long)got[(size_t)i], (unsigned long long)want[(size_t)i]);
            runs++;
        }
    return runs;
}

template <class F>
static void field_cases(const FieldDev &fd, u64 q, const char *name)
{
    typedef typename F::elem E;
    const bool small = q <= 1000;
    std::vector<int> ks;
    for (int k = 1; k <= (int)std::min<u64>(q, 9); k++) ks.push_back(k);
    if (small && q > 9) ks.push_back((int)q);
    if (!small) ks.push_back(33);
    int sets = 0, runs = 0;
    for (int k : ks) {
        for (int with_zero = 0; with_zero < 2; with_zero++) {
            // k distinct elements, with or (where the field has room) without 0
            std::vector<E> x;
            if (small) {
                for (u64 v = 0; v < q; v++) x.push_back((E)v);
                for (size_t i = x.size(); i > 1; i--) std::swap(x[i - 1], x[rnd() % i]);
                if (with_zero) std::swap(*std::find(x.begin(), x.end(), (E)0), x[rnd() % (u64)k]);
                else if ((u64)k < q) std::swap(*std::find(x.begin(), x.end(), (E)0), x[q - 1]);
                x.resize((size_t)k);
            } else {
                x.push_back(with_zero ? 0 : (E)(q - 1));
                while ((int)x.size() < k) {
                    const E v = (E)(1 + rnd() % (q - 2));
                    if (std::find(x.begin(), x.end(), v) == x.end()) x.push_back(v);
                }
                std::swap(x[0], x[rnd() % (u64)k]);
            }
            std::vector<E> y((size_t)k);
            for (auto &v : y) v = (E)(rnd() % q);
            runs += one_set<F>(fd, x, y, false, name, "random y");
            runs += one_set<F>(fd, x, std::vector<E>((size_t)k, 0), false, name, "all-zero y");
            runs += one_set<F>(fd, x, std::vector<E>((size_t)k, (E)(q - 1)), false, name, "constant y");
            sets += 3;
            if (k >= 2) { // a repeated x in the first, the middle and the last position
                std::vector<int> places{0, k / 2, k - 1};
                places.erase(std::unique(places.begin(), places.end()), places.end());
                for (int pos : places) {
                    std::vector<E> xr = x;
                    xr[(size_t)pos] = x[(size_t)(pos == 0 ? k - 1 : 0)];
                    runs += one_set<F>(fd, xr, y, true, name, "repeated x");
                    sets++;
                }
            }
        }
    }
    std::printf("%s: %d lagrange cases, %d runs\n", name, sets, runs);
}

int main()
{
    field_cases<Prime32>(prime_field(2), 2, "GF(2)");
    field_cases<Prime32>(prime_field(3), 3, "GF(3)");
    field_cases<Prime32>(prime_field(5), 5, "GF(5)");
    field_cases<Bin>(gf4(), 4, "GF(4)");
    field_cases<Prime32>(prime_field(4294967291ull), 4294967291ull, "GF(4294967291)");
    std::printf("lagrange host model ok\n");
    return 0;
}
