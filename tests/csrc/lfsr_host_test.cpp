// Host model of galois_amd/csrc/gfa_lfsr.h: the register clocks and the jump-ahead the device kernels run, compiled with g++
// (one thread in place of the workgroup).
//
// Reference: a schoolbook transcription of the four step loops (shifts and the Galois f == 0 branch written out), and a
// schoolbook x^e mod P by right-to-left binary powers.  Orders n in {1, 2, 63, 64, 65, 130}; steps in {1, n-1, n, n+1, 3n+1};
// both kinds, forward and backward; a_n = 0 (forward only); Galois states whose top elements are zero (the branch that only
// shifts); jump(e) for e in {0, 1, n} against stepping and for e = 2^40 + 3 against the schoolbook power; the Fibonacci <->
// Galois conversion.  The clocks run through the lane-interleaved view in tiles of 64, as the kernel runs them, with guard words.
// Fields: GF(5) and a 32-bit prime (Prime32), GF(p^2) for the largest prime below 2^32 (ExtP<2>); the one-word GF(2) clock
// against the generic one over GF(2).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_lfsr.h"

using namespace gfa;
using namespace gfa::lfsr;
using gfa::polydiv::Solo;
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

static u64 rng_state = 88172645463325252ull;
static u64 rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

template <class E>
static std::vector<E> sparse(u64 q, int n, int zero_percent)
{
    std::vector<E> v((size_t)n);
    for (auto &x : v) x = (int)(rnd() % 100) < zero_percent ? (E)0 : (E)(rnd() % q);
    return v;
}

// ---- the reference's loops, as written there ---------------------------------------------------------------------------
template <class F>
static std::vector<typename F::elem> school_step(const FieldDev &fd, int kind, bool forward, const std::vector<typename F::elem> &taps,
                                                 std::vector<typename F::elem> &state, int steps)
{
    typedef typename F::elem E;
    const int n = (int)taps.size();
    std::vector<E> y((size_t)steps, 0);
    for (int i = 0; i < steps; i++) {
        if (kind == KIND_FIBONACCI && forward) {
            E f = 0;
            for (int j = 0; j < n; j++) f = F::add(fd, f, F::mul(fd, state[j], taps[j]));
            y[i] = state[n - 1];
            for (int j = n - 1; j > 0; j--) state[j] = state[j - 1];
            state[0] = f;
        } else if (kind == KIND_FIBONACCI) {
            const E f = state[0];
            for (int j = 0; j < n - 1; j++) state[j] = state[j + 1];
            E s = f;
            for (int j = 0; j < n - 1; j++) s = F::sub(fd, s, F::mul(fd, state[j], taps[j]));
            s = F::mul(fd, s, F::inv(fd, taps[n - 1]));
            y[i] = s;
            state[n - 1] = s;
        } else if (forward) {
            const E f = state[n - 1];
            y[i] = f;
            if (f == 0) {
                for (int j = n - 1; j > 0; j--) state[j] = state[j - 1];
                state[0] = 0;
            } else {
                for (int j = n - 1; j > 0; j--) state[j] = F::add(fd, state[j - 1], F::mul(fd, f, taps[j]));
                state[0] = F::mul(fd, f, taps[0]);
            }
        } else {
            const E f = F::mul(fd, state[0], F::inv(fd, taps[0]));
            for (int j = 0; j < n - 1; j++) state[j] = F::sub(fd, state[j + 1], F::mul(fd, f, taps[j + 1]));
            state[n - 1] = f;
            y[i] = f;
        }
    }
    return y;
}

// a b mod c, all highest degree first, c monic with n + 1 coefficients; a and b have n coefficients
template <class F>
static std::vector<typename F::elem> school_mulmod(const FieldDev &fd, const std::vector<typename F::elem> &a, const std::vector<typename F::elem> &b,
                                                   const std::vector<typename F::elem> &c)
{
    typedef typename F::elem E;
    const int n = (int)a.size();
    std::vector<E> w((size_t)(2 * n - 1), 0);
    for (int i = 0; i < n; i++)
        for (int k = 0; k < n; k++) w[i + k] = F::add(fd, w[i + k], F::mul(fd, a[i], b[k]));
    for (int i = 0; i < n - 1; i++) { // n - 1 quotient digits
        const E q = w[i];
        for (int k = 0; k <= n; k++) w[i + k] = F::sub(fd, w[i + k], F::mul(fd, q, c[k]));
    }
    return std::vector<E>(w.end() - n, w.end());
}

// the characteristic polynomial (highest degree first) of a register with the given taps
template <class F>
static std::vector<typename F::elem> char_poly(const FieldDev &fd, int kind, const std::vector<typename F::elem> &taps)
{
    typedef typename F::elem E;
    const int n = (int)taps.size();
    std::vector<E> c((size_t)(n + 1), 0);
    c[0] = F::one(fd);
    for (int k = 1; k <= n; k++) c[k] = F::sub(fd, (E)0, kind == KIND_FIBONACCI ? taps[k - 1] : taps[n - k]); // a_k
    return c;
}

template <class E>
static std::vector<E> galois_taps(const std::vector<E> &fib_taps)
{
    return std::vector<E>(fib_taps.rbegin(), fib_taps.rend());
}

// FLFSR.to_galois_lfsr: G0 = floor(Y P / x^n), Y = sum S[i] x^i; returned as a Galois state (g_0 first)
template <class F>
static std::vector<typename F::elem> school_to_galois(const FieldDev &fd, const std::vector<typename F::elem> &S, const std::vector<typename F::elem> &c)
{
    typedef typename F::elem E;
    const int n = (int)S.size();
    std::vector<E> prod((size_t)(2 * n + 1), 0); // coefficient of x^k at k
    for (int i = 0; i < n; i++)
        for (int k = 0; k <= n; k++) prod[i + k] = F::add(fd, prod[i + k], F::mul(fd, S[i], c[n - k]));
    return std::vector<E>(prod.begin() + n, prod.begin() + 2 * n);
}

// ---- the header under test, as the kernel drives it --------------------------------------------------------------------
template <class E>
struct YOut {
    E *p;
    void set(int i, E v) const { p[i] = v; }
};

template <class F>
static std::vector<typename F::elem> run_step(const FieldDev &fd, int kind, bool forward, const std::vector<typename F::elem> &taps,
                                              std::vector<typename F::elem> &state, int steps)
{
    typedef typename F::elem E;
    const int n = (int)taps.size(), STRIDE = 3, TILE = 64;
    const E MARK = (E)0x5a5a5a5a;
    std::vector<E> lds((size_t)n * STRIDE, MARK), y((size_t)steps + 2, MARK), tile((size_t)TILE + 2, MARK);
    const Strided<E> s{lds.data() + 1, STRIDE};
    for (int j = 0; j < n; j++) s[j] = state[j];
    const E tinv = forward ? (E)0 : backward_inverse<F>(fd, kind == KIND_FIBONACCI ? taps[n - 1] : taps[0]);
    int head = 0;
    for (int i0 = 0; i0 < steps; i0 += TILE) {
        const int count = steps - i0 < TILE ? steps - i0 : TILE;
        clock<F>(fd, kind, forward, s, Lin<const E>{taps.data()}, n, head, tinv, count, YOut<E>{tile.data() + 1});
        CHECK(tile[0] == MARK && tile[TILE + 1] == MARK, "tile guard");
        for (int t = 0; t < count; t++) y[1 + i0 + t] = tile[1 + t];
    }
    for (size_t k = 0; k < lds.size(); k++)
        if (k % STRIDE != 1) CHECK(lds[k] == MARK, "another lane's state was touched");
    for (int j = 0; j < n; j++) state[j] = s[(head + j) % n];
    CHECK(y[0] == MARK && y[steps + 1] == MARK, "output guard");
    return std::vector<E>(y.begin() + 1, y.end() - 1);
}

template <class F>
static std::vector<typename F::elem> run_jump(const FieldDev &fd, int kind, const std::vector<typename F::elem> &c, const std::vector<typename F::elem> &state,
                                              const u64 *e, int limbs)
{
    typedef typename F::elem E;
    const int n = (int)state.size();
    const E MARK = (E)0x5a5a5a5a;
    std::vector<E> buf(jump_elems(n) - (size_t)(n + 1) + 2, MARK); // r, g0, w between two guards
    E *r = buf.data() + 1, *g0 = r + n, *w = g0 + n;
    for (int j = 0; j < n; j++) w[j] = state[j];
    jump<F, Lin<const E>, Solo>(fd, kind, Lin<E>{w}, Lin<E>{r}, Lin<E>{g0}, Lin<const E>{c.data()}, n, e, limbs, Solo());
    CHECK(buf.front() == MARK && buf.back() == MARK, "jump guard, n %d", n);
    return std::vector<E>(g0, g0 + n);
}

template <class F>
static void field_cases(const FieldDev &fd, u64 q, const char *name)
{
    typedef typename F::elem E;
    int step_cases = 0, jump_cases = 0, conv_cases = 0;
    for (int n : {1, 2, 63, 64, 65, 130}) {
        std::vector<int> steps_list;
        for (int s : {1, n - 1, n, n + 1, 3 * n + 1}) {
            bool seen = s <= 0;
            for (int t : steps_list) seen = seen || t == s;
            if (!seen) steps_list.push_back(s);
        }
        for (int kind : {KIND_FIBONACCI, KIND_GALOIS}) {
            const int an = kind == KIND_FIBONACCI ? n - 1 : 0; // where the tap -a_n sits
            // forward and backward, a_n != 0
            for (int steps : steps_list)
                for (int fwd = 1; fwd >= 0; fwd--) {
                    std::vector<E> taps = sparse<E>(q, n, 40), state = sparse<E>(q, n, 30);
                    while (taps[an] == 0) taps[an] = (E)(rnd() % q);
                    std::vector<E> expect_state = state, got_state = state;
                    const std::vector<E> expect = school_step<F>(fd, kind, fwd != 0, taps, expect_state, steps);
                    const std::vector<E> got = run_step<F>(fd, kind, fwd != 0, taps, got_state, steps);
                    CHECK(got == expect, "%s: outputs, kind %d fwd %d n %d steps %d", name, kind, fwd, n, steps);
                    CHECK(got_state == expect_state, "%s: state, kind %d fwd %d n %d steps %d", name, kind, fwd, n, steps);
                    if (fwd) { // and back again: the reference's own round trip
                        std::vector<E> back = run_step<F>(fd, kind, false, taps, got_state, steps);
                        CHECK(got_state == state && std::vector<E>(back.rbegin(), back.rend()) == got, "%s: round trip, kind %d n %d steps %d", name, kind, n, steps);
                    }
                    step_cases++;
                }
            { // a_n = 0, forward
                std::vector<E> taps = sparse<E>(q, n, 40), state = sparse<E>(q, n, 30);
                taps[an] = 0;
                std::vector<E> expect_state = state, got_state = state;
                const std::vector<E> expect = school_step<F>(fd, kind, true, taps, expect_state, 3 * n + 1);
                CHECK(run_step<F>(fd, kind, true, taps, got_state, 3 * n + 1) == expect && got_state == expect_state, "%s: a_n = 0, kind %d n %d", name, kind, n);
                step_cases++;
            }
            // jump(e) against stepping, and against the schoolbook power
            std::vector<E> taps = sparse<E>(q, n, 40), state = sparse<E>(q, n, 30);
            if (n == 64 || n == 130) taps[an] = 0; // characteristic polynomials with a_n = 0 too
            const std::vector<E> c = char_poly<F>(fd, kind, taps);
            for (u64 e : {(u64)0, (u64)1, (u64)n, ((u64)1 << 40) + 3}) {
                const u64 limbs[2] = {e, 0}; // (odd exponents also with an empty high word)
                const std::vector<E> got = run_jump<F>(fd, kind, c, state, limbs, 1 + (int)(e & 1));
                std::vector<E> expect = state;
                if (e <= (u64)n) {
                    school_step<F>(fd, kind, true, taps, expect, (int)e);
                } else {
                    std::vector<E> acc((size_t)n, 0), sq((size_t)n, 0); // x^e mod c
                    acc[n - 1] = F::one(fd);
                    if (n == 1) sq[0] = F::sub(fd, (E)0, c[1]);
                    else sq[n - 2] = F::one(fd);
                    for (int bit = 0; bit < 41; bit++) {
                        if ((e >> bit) & 1) acc = school_mulmod<F>(fd, acc, sq, c);
                        sq = school_mulmod<F>(fd, sq, sq, c);
                    }
                    const std::vector<E> gtaps = kind == KIND_FIBONACCI ? galois_taps(taps) : taps;
                    std::vector<E> G = kind == KIND_FIBONACCI ? school_to_galois<F>(fd, state, c) : state;
                    G = school_mulmod<F>(fd, acc, std::vector<E>(G.rbegin(), G.rend()), c);
                    expect = std::vector<E>(G.rbegin(), G.rend());
                    if (kind == KIND_FIBONACCI) { // its next n outputs, reversed
                        const std::vector<E> y = school_step<F>(fd, KIND_GALOIS, true, gtaps, expect, n);
                        expect = std::vector<E>(y.rbegin(), y.rend());
                    }
                }
                CHECK(got == expect, "%s: jump, kind %d n %d e %llu", name, kind, n, (unsigned long long)e);
                jump_cases++;
            }
        }
        { // the Galois branch that only shifts: the top half of the state is zero
            std::vector<E> taps = sparse<E>(q, n, 40), state = sparse<E>(q, n, 30);
            for (int j = n / 2; j < n; j++) state[j] = 0;
            std::vector<E> expect_state = state, got_state = state;
            const std::vector<E> expect = school_step<F>(fd, KIND_GALOIS, true, taps, expect_state, n + 1);
            CHECK(run_step<F>(fd, KIND_GALOIS, true, taps, got_state, n + 1) == expect && got_state == expect_state, "%s: f = 0 steps, n %d", name, n);
            step_cases++;
        }
        { // conversion: the Galois register at to_galois(S) puts out what the Fibonacci register at S does
            std::vector<E> taps = sparse<E>(q, n, 40), state = sparse<E>(q, n, 30);
            const std::vector<E> c = char_poly<F>(fd, KIND_FIBONACCI, taps);
            std::vector<E> fs = state, gs = school_to_galois<F>(fd, state, c);
            const std::vector<E> yf = run_step<F>(fd, KIND_FIBONACCI, true, taps, fs, 2 * n + 3);
            const std::vector<E> yg = run_step<F>(fd, KIND_GALOIS, true, galois_taps(taps), gs, 2 * n + 3);
            CHECK(yf == yg, "%s: conversion, n %d", name, n);
            conv_cases++;
        }
    }
    std::printf("%s: %d step cases, %d jump cases, %d conversion cases\n", name, step_cases, jump_cases, conv_cases);
}

// the one-word clock of GF(2) against the generic clock over GF(2)
static void bits_cases()
{
    const FieldDev fd = prime_field(2);
    int cases = 0;
    for (int n : {1, 2, 31, 63, 64})
        for (int kind : {KIND_FIBONACCI, KIND_GALOIS})
            for (int steps : {1, n, 63, 64, 65, 3 * n + 1}) {
                std::vector<u32> taps = sparse<u32>(2, n, 0), state = sparse<u32>(2, n, 0);
                u64 t = 0, s = 0;
                for (int j = 0; j < n; j++) {
                    t |= (u64)taps[j] << j;
                    s |= (u64)state[j] << j;
                }
                const std::vector<u32> expect = school_step<Prime32>(fd, kind, true, taps, state, steps);
                for (int i0 = 0; i0 < steps; i0 += 64) {
                    const int count = steps - i0 < 64 ? steps - i0 : 64;
                    const u64 out = clock_bits(kind, s, t, n, count);
                    for (int i = 0; i < count; i++) CHECK(((out >> i) & 1) == expect[i0 + i], "GF(2) words: output %d, kind %d n %d steps %d", i0 + i, kind, n, steps);
                    if (count < 64) CHECK((out >> count) == 0, "GF(2) words: bits beyond the count");
                }
                for (int j = 0; j < n; j++) CHECK(((s >> j) & 1) == state[j], "GF(2) words: state, kind %d n %d steps %d", kind, n, steps);
                if (n < 64) CHECK((s >> n) == 0, "GF(2) words: bits beyond the order");
                cases++;
            }
    std::printf("GF(2) words: %d cases\n", cases);
}

int main()
{
    field_cases<Prime32>(prime_field(5), 5, "GF(5)");
    field_cases<Prime32>(prime_field(4294967291ull), 4294967291ull, "GF(4294967291)");
    const FieldDev e2 = ext2_field(4294967291ull);
    field_cases<ExtP<2>>(e2, e2.q, "GF(4294967291^2)");
    bits_cases();
    std::printf("lfsr host model ok\n");
    return 0;
}
