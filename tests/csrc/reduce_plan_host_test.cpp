// Host test of galois_amd/csrc/gfa_reduce_plan.h: the arithmetic that cuts a gfa_reduce / gfa_accumulate call into segments and picks the
// first-phase kernel, swept over CU counts, row counts and lengths around every threshold.  Prints the plan of a fixed list of shapes, which
// tests/test_reduce_plan_host.py compares with tests/fold_plan.py line for line.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_reduce_plan.h"

using namespace gfa::reduce_plan;

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

struct Field {
    u64 p;
    unsigned m;
    u64 q;
};

static bool holds(int size, u64 q) { return size == 8 || q - 1 <= (((u64)1 << (8 * size)) - 1); }

// segments [s seg_len, min((s + 1) seg_len, len)) of the len folded columns: none empty, together every column exactly once (they are
// consecutive, so that is: the last one ends at len)
static void check_cover(const Segments &sg, i64 len, const char *what, int cus, i64 n_outer)
{
    CHECK(sg.nseg >= 1 && sg.nseg <= MAX_SEGMENTS, "%s cus=%d rows=%lld len=%lld nseg=%lld", what, cus, (long long)n_outer, (long long)len, (long long)sg.nseg);
    if (sg.seg_len == 0) { // the whole-row scan
        CHECK(sg.nseg == 1, "%s", what);
        return;
    }
    CHECK(sg.seg_len >= 1, "%s", what);
    const unsigned __int128 last_lo = (unsigned __int128)(sg.nseg - 1) * (u64)sg.seg_len, end = (unsigned __int128)sg.nseg * (u64)sg.seg_len;
    CHECK(last_lo < (unsigned __int128)(len > 0 ? len : 1), "%s cus=%d rows=%lld len=%lld: an empty segment (nseg=%lld seg_len=%lld)", what, cus, (long long)n_outer,
          (long long)len, (long long)sg.nseg, (long long)sg.seg_len);
    CHECK(end >= (unsigned __int128)len, "%s cus=%d rows=%lld len=%lld: columns left over (nseg=%lld seg_len=%lld)", what, cus, (long long)n_outer, (long long)len,
          (long long)sg.nseg, (long long)sg.seg_len);
}

// the bound each streaming form relies on, from the widest element it can meet
static void check_guards(int mode, int size, i64 seg_len)
{
    if (mode == STREAM_SUM) { // seg_len addends below 2^(8 size) in 64 bits
        CHECK(size <= 4, "size %d", size);
        CHECK((unsigned __int128)seg_len * ((((u64)1) << (8 * size)) - 1) < ((unsigned __int128)1 << 64), "seg_len %lld", (long long)seg_len);
        CHECK(seg_len < ((i64)1 << 32), "seg_len %lld", (long long)seg_len);
    }
    if (mode == STREAM_LOG) { // seg_len logarithms below 2^8 in 64 bits
        CHECK(size == 1, "size %d", size);
        CHECK((unsigned __int128)seg_len * 255 < ((unsigned __int128)1 << 64) && seg_len < ((i64)1 << 40), "seg_len %lld", (long long)seg_len);
    }
    if (mode == STREAM_TAB) CHECK(size == 1, "size %d", size);
}

static const Field FIELDS[] = {{2, 1, 2}, {2, 8, 256}, {2, 16, 65536}, {2, 40, (u64)1 << 40}, {3, 1, 3}, {31, 1, 31}, {65521, 1, 65521},
                               {4294967291ull, 1, 4294967291ull}, {3, 2, 9}, {3, 5, 243}, {3, 10, 59049}, {0xffffffff00000001ull, 1, 0xffffffff00000001ull}};

// (a field of at most 256 elements has its byte tables on the device whenever a call gets as far as planning: gfa_field::ensure_device)
static int mode_of(const Field &f, bool is_mul, bool lut, int size, i64 seg_len)
{
    const bool tab8 = f.q <= 256;
    return stream_mode(is_mul, f.p, f.m, f.q, lut, size, tab8, tab8, seg_len);
}

static void sweep()
{
    const int cus_list[] = {1, 64, 256, 304};
    const i64 rows_list[] = {1, 2, 3, 255, 256, 257, 511, 512, 2047, 2048, 2049, (i64)1 << 20, MAX_GRID - 1, MAX_GRID};
    std::vector<i64> lens = {1, 2, 4095, 4096, 4097, 8191, 8192, 8193, 65535, 65536, 65537, 8192 * 256 - 1, 8192 * 256, 8192 * 256 + 1,
                             4096 * 4096 - 1, 4096 * 4096, 4096 * 4096 + 1, ((i64)1 << 32) - 1, (i64)1 << 32, ((i64)1 << 32) + 1, (i64)1 << 40};
    for (int cus : cus_list)
        for (i64 n_outer : rows_list)
            for (i64 len : lens)
                for (int tab_add = 0; tab_add < 2; tab_add++) {
                    const Segments r = reduce_segments(n_outer, len, cus, tab_add != 0);
                    check_cover(r, len, "reduce", cus, n_outer);
                    CHECK(r.seg_len > 0, "reduce");
                    CHECK((unsigned __int128)n_outer * (u64)r.nseg <= (unsigned __int128)MAX_GRID, "reduce grid: rows=%lld nseg=%lld", (long long)n_outer, (long long)r.nseg);
                    CHECK(r.nseg == 1 || (len > 8192 && n_outer < (i64)cus * 8), "reduce: segments for a short row or many rows");
                    const Segments a = accumulate_segments(n_outer, len, cus);
                    check_cover(a, len, "accumulate", cus, n_outer);
                    CHECK(a.seg_len % 256 == 0, "accumulate seg_len %lld", (long long)a.seg_len);
                    CHECK((a.nseg == 1) == (a.seg_len == 0), "accumulate: nseg %lld with seg_len %lld", (long long)a.nseg, (long long)a.seg_len);
                    CHECK((unsigned __int128)n_outer * (u64)a.nseg <= (unsigned __int128)MAX_GRID, "accumulate grid: rows=%lld nseg=%lld", (long long)n_outer, (long long)a.nseg);
                    CHECK(carry_runs(a.nseg) >= 1 && carry_runs(a.nseg) * 256 >= a.nseg && (carry_runs(a.nseg) - 1) * 256 < a.nseg, "carry runs");
                    for (const Field &f : FIELDS)
                        for (int size = 1; size <= 8; size *= 2) {
                            if (!holds(size, f.q)) continue;
                            for (int lut = 0; lut < (f.q <= ((u64)1 << 20) ? 2 : 1); lut++)
                                for (int is_mul = 0; is_mul < 2; is_mul++) {
                                    const bool ta = table_sum(is_mul != 0, lut != 0, size, f.q, f.m, f.q <= 256);
                                    if (ta == (tab_add != 0)) check_guards(mode_of(f, is_mul != 0, lut != 0, size, r.seg_len), size, r.seg_len);
                                    if (a.nseg > 1) check_guards(mode_of(f, is_mul != 0, lut != 0, size, a.seg_len), size, a.seg_len);
                                }
                        }
                }
    CHECK(!block_join(1) && !block_join(8) && block_join(9) && block_join(MAX_SEGMENTS), "block_join");
    CHECK(rows_fit_grid(0) && rows_fit_grid(MAX_GRID) && !rows_fit_grid(MAX_GRID + 1) && !rows_fit_grid((i64)1 << 32) && !rows_fit_grid(INT64_MAX), "rows_fit_grid");
    // the guards themselves, at the lengths they cut at
    const Field gf31 = {31, 1, 31}, gf256 = {2, 8, 256}, gf243 = {3, 5, 243};
    CHECK(mode_of(gf31, false, true, 4, ((i64)1 << 32) - 1) == STREAM_SUM && mode_of(gf31, false, true, 4, (i64)1 << 32) == GENERIC, "sum guard");
    CHECK(mode_of(gf31, false, false, 8, 100) == GENERIC, "8-byte prime elements");
    CHECK(mode_of(gf256, true, true, 1, ((i64)1 << 40) - 1) == STREAM_LOG && mode_of(gf256, true, true, 1, (i64)1 << 40) == GENERIC, "log guard");
    CHECK(mode_of(gf256, true, false, 1, 100) == GENERIC && mode_of(gf256, true, true, 2, 100) == GENERIC, "log form needs the table field in bytes");
    CHECK(mode_of(gf256, false, false, 8, (i64)1 << 40) == STREAM_XOR, "xor");
    CHECK(mode_of(gf243, false, true, 1, 100) == STREAM_TAB && mode_of(gf243, false, true, 2, 100) == GENERIC && mode_of(gf243, false, false, 1, 100) == GENERIC, "table sums");
}

static const char *form_name(int mode, char *buf)
{
    std::snprintf(buf, 16, "%d", mode);
    return buf;
}

static void print_plans()
{
    const int cus_list[] = {64, 256, 304};
    const i64 shapes[][2] = {{5, 8192}, {5, 8193}, {5, 8194}, {3, 40003}, {3, 40004}, {1, 32768}, {1, 32769}, {1, 32770}, {2, 65535}, {2, 65536}, {2, 65537},
                             {3, 70001}, {1, 2200001}, {1, 2200002}, {100000, 3}, {4096, 1}, {1025, 9001}, {300, 9001}, {1, (i64)1 << 24}, {7, 1000003}};
    char buf[16];
    for (const Field &f : FIELDS)
        for (int size = 1; size <= 8; size *= 2) {
            if (!holds(size, f.q)) continue;
            for (int lut = 0; lut < (f.q <= ((u64)1 << 20) ? 2 : 1); lut++)
                for (int op = 0; op < 4; op++) // GFA_OP_ADD, SUB, MUL, DIV
                    for (int cus : cus_list)
                        for (const auto &sh : shapes) {
                            const bool is_mul = op >= 2, tab8 = f.q <= 256;
                            const i64 n_outer = sh[0], n_inner = sh[1], len = n_inner - (op == 1 || op == 3 ? 1 : 0);
                            const Segments r = reduce_segments(n_outer, len, cus, table_sum(is_mul, lut != 0, size, f.q, f.m, tab8));
                            std::printf("reduce op=%d cus=%d rows=%lld cols=%lld size=%d p=%llu m=%u lut=%d -> nseg=%lld seg_len=%lld form=%s join=%s c=0\n", op, cus,
                                        (long long)n_outer, (long long)n_inner, size, (unsigned long long)f.p, f.m, lut, (long long)r.nseg, (long long)r.seg_len,
                                        form_name(mode_of(f, is_mul, lut != 0, size, r.seg_len), buf), block_join(r.nseg) ? "block" : "thread");
                            const Segments a = accumulate_segments(n_outer, len, cus);
                            std::printf("accumulate op=%d cus=%d rows=%lld cols=%lld size=%d p=%llu m=%u lut=%d -> nseg=%lld seg_len=%lld form=%s join=%s c=%lld\n", op, cus,
                                        (long long)n_outer, (long long)n_inner, size, (unsigned long long)f.p, f.m, lut, (long long)a.nseg, (long long)a.seg_len,
                                        a.nseg > 1 ? form_name(mode_of(f, is_mul, lut != 0, size, a.seg_len), buf) : "none", a.nseg > 1 ? "carries" : "row",
                                        a.nseg > 1 ? (long long)carry_runs(a.nseg) : 0ll);
                        }
        }
}

int main()
{
    sweep();
    print_plans();
    std::printf("reduce plan host model ok: %ld checks\n", g_checks);
    return 0;
}
