// Host test of galois_amd/csrc/gfa_elim_plan.h: the integer arithmetic that sends a gfa_row_reduce call to the one-workgroup kernel or to
// the two-kernels-per-column route, and the shapes gfa_row_reduce / gfa_plu_decompose refuse.  Sweeps m and n around 256, 4096, 2^24 and
// the row limit of the two-kernel grid, m * n around 131072 (including products past 32 bits), and the batch around 32 and 65535, against
// the rules restated here in 128-bit arithmetic.  Prints the route of a fixed list of calls, which tests/test_elim_plan_host.py compares
// with tests/elim_plan.py line for line.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_elim_plan.h"

using namespace gfa::elim_plan;

static long g_checks = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        g_checks++;                                                                       \
        if (!(cond)) {                                                                    \
            std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);               \
            std::printf(__VA_ARGS__);                                                     \
            std::printf("\n");                                                            \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

static const char *name(Route r) { return r == ONE_WORKGROUP ? "ONE_WORKGROUP" : r == TWO_KERNELS ? "TWO_KERNELS" : "UNSUPPORTED"; }

static std::vector<i64> around(std::vector<i64> centres)
{
    std::vector<i64> out;
    for (i64 c : centres)
        for (i64 d = -2; d <= 2; d++)
            if (c + d >= 1) out.push_back(c + d);
    return out;
}

int main()
{
    static_assert(GJ_THREADS == 256 && GJ_MAX_ROWS == 4096 && GJ_WIDE_MIN_ELEMS == 131072 && GJ_WIDE_MAX_BATCH == 32, "thresholds the tests name");
    static_assert(GJ_MAX_DIM == (i64)1 << 24 && GJ_WIDE_MAX_ROWS == 2097120, "limits the tests name");
    static_assert((GJ_WIDE_MAX_ROWS + GJ_WIDE_ROW_TILE - 1) / GJ_WIDE_ROW_TILE == 65535, "the row tiles of the tallest matrix fill gridDim.y exactly");
    static_assert(GJ_MAX_ROWS % GJ_THREADS == 0 && GJ_MAX_ROWS < GJ_WIDE_MAX_ROWS && GJ_WIDE_MAX_ROWS < GJ_MAX_DIM, "order of the limits");

    // dimensions: every threshold itself, the divisors of 131072 that pair with them, and sizes whose product passes 2^32 and 2^47
    const std::vector<i64> dims = around({1, 3, 8, 32, 256, 257, 362, 363, 510, 511, 512, 4096, 8192, 16384, 32768, 65536, 131072, 2097120,
                                          (i64)1 << 22, (i64)1 << 24});
    const std::vector<i64> batches = around({1, 32, 33, 4096, 65535, 65536, 0x7fffffff});
    for (i64 b : batches)
        for (i64 m : dims)
            for (i64 n : dims) {
                const Route r = elim_route(b, m, n);
                const unsigned __int128 elems = (unsigned __int128)m * (unsigned __int128)n;
                const bool in_range = m <= ((i64)1 << 24) && n <= ((i64)1 << 24);
                const bool few_and_large = b <= 32 && (elems >= 131072 || m > 4096);
                // the product the header computes in 64 bits is the true one
                CHECK(!in_range || (unsigned __int128)(m * n) == elems, "m=%lld n=%lld", (long long)m, (long long)n);
                if (!in_range) CHECK(r == UNSUPPORTED, "b=%lld m=%lld n=%lld", (long long)b, (long long)m, (long long)n);
                else if (few_and_large) CHECK(r == (m <= 2097120 ? TWO_KERNELS : UNSUPPORTED), "b=%lld m=%lld n=%lld", (long long)b, (long long)m, (long long)n);
                else CHECK(r == (m <= 4096 ? ONE_WORKGROUP : UNSUPPORTED), "b=%lld m=%lld n=%lld", (long long)b, (long long)m, (long long)n);
                // what each route relies on
                if (r == ONE_WORKGROUP) CHECK(m <= GJ_MAX_ROWS, "the LDS factor array holds %d rows, m=%lld", GJ_MAX_ROWS, (long long)m);
                if (r == TWO_KERNELS) {
                    CHECK((m + GJ_WIDE_ROW_TILE - 1) / GJ_WIDE_ROW_TILE <= 65535 && b <= 65535, "grid of gj_eliminate_kernel: b=%lld m=%lld", (long long)b, (long long)m);
                    CHECK((unsigned __int128)b * (unsigned __int128)m <= ((unsigned __int128)1 << 30), "factor buffer of b=%lld m=%lld", (long long)b, (long long)m);
                    CHECK((unsigned __int128)b * elems < ((unsigned __int128)1 << 60), "byte offset of b=%lld m=%lld n=%lld in 64 bits", (long long)b, (long long)m, (long long)n);
                }
                CHECK(plu_supported(m, n) == (m <= 4096 && n <= ((i64)1 << 24)), "plu m=%lld n=%lld", (long long)m, (long long)n);
                std::printf("row_reduce batch=%lld m=%lld n=%lld -> %s\n", (long long)b, (long long)m, (long long)n, name(r));
            }
    for (i64 m : dims)
        for (i64 n : {(i64)1, (i64)4, (i64)300, (i64)4096, (i64)1 << 24, ((i64)1 << 24) + 1})
            std::printf("plu m=%lld n=%lld -> %s\n", (long long)m, (long long)n, plu_supported(m, n) ? "yes" : "no");
    CHECK(elim_route(0, 5, 5) == UNSUPPORTED && elim_route(1, 0, 5) == UNSUPPORTED && elim_route(1, 5, 0) == UNSUPPORTED && !plu_supported(0, 1) && !plu_supported(1, 0),
          "empty shapes are not routed");
    std::printf("elim plan host model ok: %ld checks\n", g_checks);
    return 0;
}
