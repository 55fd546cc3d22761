// gfa_reduce_plan.h -- how gfa_reduce / gfa_accumulate cut a call into segments and which first-phase kernel folds a segment.
// Plain integer arithmetic on plain integers: no HIP types, the CU count is a parameter, so that the same functions compile for the host
// alone (tests/csrc/reduce_plan_host_test.cpp sweeps them; tests/fold_plan.py mirrors them for the GPU tests).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GFA_PLAN_HD __host__ __device__
#else
#define GFA_PLAN_HD
#endif

namespace gfa {
namespace reduce_plan {

typedef int64_t i64;
typedef uint64_t u64;

// first-phase forms of reduce_stream_kernel (its MODE); GENERIC is reduce_segments_kernel
enum { GENERIC = -1, STREAM_XOR = 0, STREAM_SUM = 1, STREAM_LOG = 2, STREAM_TAB = 3 };

// A launch's grid is cast to `unsigned`; 2^31 - 1 workgroups along x is the documented limit of a HIP grid.  Whether the runtime at hand
// launches every grid below it has NOT been measured (runtimes have refused grids of more than 2^32 - 1 threads in all, 2^24 - 1 workgroups
// of 256): the bound only keeps the cast from wrapping.  A launch the runtime refuses comes back as GFA_ERR_HIP, never as wrong values.
constexpr i64 MAX_GRID = 0x7fffffff;
constexpr i64 MAX_SEGMENTS = 4096;

struct Segments {
    i64 nseg;    // segments per row; 1: the whole row
    i64 seg_len; // columns per segment (the last one may be shorter); 0 for the whole-row scan
};

// the byte-table sum fold (STREAM_TAB) stages the field's 64 KiB sum table per workgroup: table field of odd characteristic and degree > 1 with
// at most 256 elements, in 1-byte storage
inline bool table_sum(bool is_mul, bool is_lut, int elem_size, u64 q, unsigned m, bool has_add8)
{
    return !is_mul && is_lut && elem_size == 1 && q <= 256 && m > 1 && has_add8;
}

// which kernel folds a segment of seg_len elements (p, m, q: the field; is_lut: the table arithmetic is in use; has_log8 / has_add8: the
// byte LOG + EXP / sum tables are on the device -- gfa_field::ensure_device uploads them for every field of at most 256 elements, in either
// arithmetic mode, or fails the call; tests/fold_plan.py and the host sweep therefore write q <= 256 for them)
inline int stream_mode(bool is_mul, u64 p, unsigned m, u64 q, bool is_lut, int elem_size, bool has_log8, bool has_add8, i64 seg_len)
{
    if (!is_mul && p == 2) return STREAM_XOR;
    if (!is_mul && m == 1 && elem_size <= 4 && seg_len < ((i64)1 << 32)) return STREAM_SUM; // at most 2^32 addends below 2^32: a 64-bit sum
    if (is_mul && is_lut && elem_size == 1 && q <= 256 && has_log8 && seg_len < ((i64)1 << 40)) return STREAM_LOG; // 2^40 logarithms below 2^8
    if (table_sum(is_mul, is_lut, elem_size, q, m, has_add8)) return STREAM_TAB;
    return GENERIC;
}

// gfa_reduce: enough segments to fill the chip when there are few rows, at least 4096 elements each.  len = n_inner - col_begin columns are
// folded (col_begin = 1 for subtract / divide); tab_add: table_sum() above, two workgroups per CU instead of eight.
inline Segments reduce_segments(i64 n_outer, i64 len, int cus, bool tab_add)
{
    i64 nseg = 1;
    const i64 want_blocks = (i64)cus * (tab_add ? 2 : 8);
    if (n_outer < want_blocks && len > 8192) {
        const i64 by_rows = (want_blocks + n_outer - 1) / n_outer, by_len = (len + 4095) / 4096;
        nseg = by_rows < by_len ? by_rows : by_len;
        if (nseg > MAX_SEGMENTS) nseg = MAX_SEGMENTS;
    }
    if (nseg < 1) nseg = 1;
    return {nseg, len > 0 ? (len + nseg - 1) / nseg : 1};
}

// gfa_accumulate: few long rows are cut into segments of a multiple of 256 elements (segment folds -> carries -> segment scans); {1, 0}: one
// workgroup scans the whole row
inline Segments accumulate_segments(i64 n_outer, i64 len, int cus)
{
    const i64 want_blocks = (i64)cus * 8;
    if (n_outer < want_blocks / 4 && len >= ((i64)1 << 16)) {
        const i64 by_rows = (want_blocks + n_outer - 1) / n_outer, by_len = len / 8192;
        i64 nseg = by_rows < by_len ? by_rows : by_len;
        if (nseg > MAX_SEGMENTS) nseg = MAX_SEGMENTS;
        if (nseg >= 2) {
            const i64 seg_len = ((len + nseg - 1) / nseg + 255) / 256 * 256;
            return {(len + seg_len - 1) / seg_len, seg_len};
        }
    }
    return {1, 0};
}

// gfa_reduce joins the segment folds of a row with one thread per row (reduce_finalize_kernel), or -- few rows, many segments -- with one
// workgroup per row (reduce_finalize_block_kernel)
inline bool block_join(i64 nseg) { return nseg > 8; }

// runs of segment folds per thread in accumulate_carries_kernel (the kernel calls it too)
GFA_PLAN_HD inline i64 carry_runs(i64 nseg) { return (nseg + 255) / 256; }

// the entry points refuse a row count whose grid would wrap in the cast, see MAX_GRID (with nseg > 1 the planners keep n_outer * nseg below
// 2 * 8 * cus + n_outer, so the row count alone decides)
inline bool rows_fit_grid(i64 n_outer) { return n_outer <= MAX_GRID; }

} // namespace reduce_plan
} // namespace gfa
