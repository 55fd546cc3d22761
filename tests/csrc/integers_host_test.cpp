// Host model of galois_amd/csrc/gfa_integers.h: the per-lane routines of the integer kernels, compiled with g++ and checked
// against the definitions -- trial division, Euler's criterion, a naive sieve and the order found by stepping.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_integers.h"

using namespace gfa;
using namespace gfa::integers;

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                printf("FAIL: ");         \
                printf(__VA_ARGS__);      \
                printf("\n");             \
            }                             \
        }                                 \
    } while (0)

static bool naive_prime(u64 n)
{
    if (n < 2) return false;
    for (u64 d = 2; d * d <= n; d++)
        if (n % d == 0) return false;
    return true;
}

static u64 powmod(u64 a, u64 e, u64 n)
{
    unsigned __int128 r = 1, b = a % n;
    while (e) {
        if (e & 1) r = r * b % n;
        b = b * b % n;
        e >>= 1;
    }
    return (u64)r;
}

static u64 naive_gcd(u64 a, u64 b)
{
    while (b) {
        const u64 t = a % b;
        a = b;
        b = t;
    }
    return a;
}

static void test_miller_rabin()
{
    u64 count = 0;
    for (u64 n = 0; n < (1u << 20); n++) {
        const bool want = naive_prime(n);
        count += want;
        CHECK(is_prime64(n) == want, "is_prime64(%llu)", (unsigned long long)n);
    }
    CHECK(count == 82025, "pi(2^20) = %llu", (unsigned long long)count);
    struct { u64 n; bool prime; } edge[] = {
        {0, false}, {1, false}, {2, true}, {3, true}, {4, false}, {561, false}, {41041, false}, {3215031751ull, false},
        {341550071728321ull, false}, {3825123056546413051ull, false}, {4294967291ull * 4294967291ull, false},
        {4294967291ull * 4294967279ull, false}, {(1ull << 61) - 1, true}, {0xffffffffffffffffull - 58, true}, {0xffffffffffffffffull, false},
        {4294967291ull, true}, {4294967279ull, true},
    };
    for (auto &e : edge) CHECK(is_prime64(e.n) == e.prime, "is_prime64(%llu) edge", (unsigned long long)e.n);
    // Montgomery arithmetic itself, on moduli of every size class
    const u64 moduli[] = {3, 9, 15, 4294967291ull, (1ull << 63) + 29, 0xffffffffffffffffull, 0xffffffffffffffffull - 58};
    for (u64 n : moduli) {
        const Mont m = mont_setup(n);
        u64 x = 0x9e3779b97f4a7c15ull;
        for (int i = 0; i < 200; i++) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const u64 a = x % n, e = (x >> 7) | 1;
            const u64 got = mont_mul(m, mont_pow(m, to_mont(m, a), e), 1); // out of Montgomery form
            CHECK(got == powmod(a, e, n), "mont_pow modulo %llu", (unsigned long long)n);
        }
    }
    printf("miller-rabin: %llu primes below 2^20\n", (unsigned long long)count);
}

static void test_jacobi()
{
    int primes = 0;
    for (u64 p = 3; p < 500; p += 2) {
        if (!naive_prime(p)) continue;
        primes++;
        for (u64 a = 0; a < p; a++) {
            const u64 e = powmod(a, (p - 1) / 2, p);
            const int want = e == 0 ? 0 : (e == 1 ? 1 : -1);
            CHECK(jacobi((i64)a, p) == want, "jacobi(%llu, %llu)", (unsigned long long)a, (unsigned long long)p);
            CHECK(jacobi((i64)a - (i64)p, p) == want, "jacobi(%lld, %llu)", (long long)a - (long long)p, (unsigned long long)p);
        }
    }
    // multiplicativity in the lower argument: (a / n1 n2) = (a / n1) (a / n2)
    const u64 odd[] = {3, 5, 9, 15, 21, 49, 105, 1001, 4294967291ull, 4294967279ull};
    const i64 as[] = {INT64_MIN, -1000003, -2, -1, 0, 1, 2, 3, 5, 6, 1000003, INT64_MAX};
    for (u64 n1 : odd)
        for (u64 n2 : odd)
            for (i64 a : as)
                CHECK(jacobi(a, n1 * n2) == jacobi(a, n1) * jacobi(a, n2), "jacobi(%lld, %llu * %llu)", (long long)a, (unsigned long long)n1,
                      (unsigned long long)n2);
    // and in the upper one, at full-width moduli
    const u64 wide[] = {(1ull << 63) + 29, 0xffffffffffffffffull, 0xffffffffffffffffull - 58};
    for (u64 n : wide)
        for (i64 a : as)
            for (i64 b : {(i64)3, (i64)-7, (i64)65537})
                if (a > INT64_MIN / 65537 && a < INT64_MAX / 65537)
                    CHECK(jacobi(a * b, n) == jacobi(a, n) * jacobi(b, n), "jacobi(%lld * %lld, %llu)", (long long)a, (long long)b, (unsigned long long)n);
    printf("jacobi: %d odd primes below 500\n", primes);
}

// the window [start, stop) sieved as `segments of seg_bits bits`, with n_lanes lanes, against trial division
static void sieve_window(u64 start, u64 stop, int n_lanes)
{
    const u64 first = start | 1;
    const u64 n_bits64 = stop > first ? (stop - first + 1) / 2 : 0;
    if (n_bits64 == 0) return;
    const u32 n_bits = (u32)n_bits64;
    std::vector<u32> base;
    u64 limit = 2;
    while (limit * limit < stop) limit++;
    std::vector<char> composite(limit + 1, 0);
    for (u64 p = 2; p * p < stop; p++) {
        if (composite[p]) continue;
        base.push_back((u32)p);
        for (u64 k = p * p; k <= limit; k += p) composite[k] = 1;
    }
    const u32 n_words = (n_bits + 31) / 32;
    std::vector<u32> words(n_words, 0); // exactly the words of the window: AddressSanitizer sees a mark past them
    for (int lane = 0; lane < n_lanes; lane++)
        mark_segment(first, n_bits, base.data(), (int)base.size(), lane, n_lanes, [&](u32 w, u32 mask) {
            CHECK(w < n_words, "mark outside the segment");
            if (w < n_words) words[w] |= mask;
        });
    for (u32 w = 0; w < n_words; w++) {
        const u32 v = survivors_word(words[w], w, first, n_bits);
        for (u32 b = 0; b < 32; b++) {
            const u64 k = (u64)w * 32 + b, value = first + 2 * k;
            const bool want = k < n_bits && naive_prime(value);
            CHECK((((v >> b) & 1) != 0) == want, "sieve [%llu, %llu): %llu with %d lanes", (unsigned long long)start, (unsigned long long)stop,
                  (unsigned long long)value, n_lanes);
        }
    }
}

static void test_sieve()
{
    int windows = 0;
    const u64 widths[] = {1, 63, 64, 65}; // in odd numbers
    std::vector<u64> starts = {0, 1, 2, 3};
    for (u64 p : {3, 5, 7, 11, 13, 31, 61, 127, 1021, 1031, 1049}) // windows that straddle p^2
        for (u64 back : {0, 1, 2, 3, 60, 64, 126}) starts.push_back(p * p > back ? p * p - back : 0);
    for (u64 s : starts)
        for (u64 w : widths)
            for (u64 parity = 0; parity < 2; parity++) { // the stop of either parity
                const u64 first = s | 1, stop = first + 2 * (w - 1) + 1 + parity;
                for (int lanes : {1, 4, 256}) sieve_window(s, stop, lanes);
                windows++;
            }
    sieve_window(0, 70000, 256);             // several words per small prime, primes beyond sqrt left alone
    sieve_window(1024 * 1024 - 5000, 1024 * 1024 + 90000, 64); // base primes on both sides of COOP_PRIME
    sieve_window((1ull << 40) - 4096, 1ull << 40, 256);        // the bound of the entry point (base primes up to 2^20)
    sieve_window(5, 5, 4);
    sieve_window(2, 3, 4);
    printf("sieve: %d small windows\n", windows);
}

static void test_units()
{
    u64 roots_total = 0;
    for (u64 n = 1; n <= 2000; n++) {
        u64 phi = 0;
        for (u64 g = 0; g < n; g++) phi += naive_gcd(g, n) == 1;
        if (n == 1) phi = 1;
        std::vector<u64> exps;
        for (u64 r = 2, rest = phi; rest > 1; r++)
            if (rest % r == 0) {
                exps.push_back(phi / r);
                while (rest % r == 0) rest /= r;
            }
        const u64 modulus = power_modulus(n);
        const bool powers = modulus != 0; // the entry point refuses exponents for the other moduli
        Mont mont = Mont();
        if (modulus >= 3) mont = mont_setup(modulus);
        for (u64 g = 0; g < n; g++) {
            const bool unit = naive_gcd(g, n) == 1;
            const uint8_t plain = unit_flags(g, n, mont, modulus, nullptr, 0);
            CHECK(((plain & INT_UNIT) != 0) == unit, "unit flag of %llu modulo %llu", (unsigned long long)g, (unsigned long long)n);
            CHECK(gcd64(g, n) == naive_gcd(g, n), "gcd64(%llu, %llu)", (unsigned long long)g, (unsigned long long)n);
            if (!powers || n < 3) continue;
            u64 order = 0;
            if (unit) {
                u64 x = g % n;
                order = 1;
                while (x != 1) {
                    x = x * g % n;
                    order++;
                }
            }
            const bool root = unit && order == phi;
            const uint8_t f = unit_flags(g, n, mont, modulus, exps.data(), (int)exps.size());
            CHECK(((f & INT_UNIT) != 0) == unit && ((f & INT_PRIMITIVE) != 0) == root, "flags %d of %llu modulo %llu (order %llu, phi %llu)", (int)f,
                  (unsigned long long)g, (unsigned long long)n, (unsigned long long)order, (unsigned long long)phi);
            roots_total += root;
        }
    }
    CHECK(power_modulus(4) == 0 && power_modulus(8) == 0 && power_modulus(6) == 3 && power_modulus(2) == 1 && power_modulus(9) == 9,
          "power_modulus");
    printf("units: %llu primitive roots over the moduli up to 2000\n", (unsigned long long)roots_total);
}

int main()
{
    test_miller_rabin();
    test_jacobi();
    test_sieve();
    test_units();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("integers host model ok\n");
    return 0;
}
