// gfa_elim_plan.h -- which kernels run a gfa_row_reduce call, and which shapes gfa_row_reduce / gfa_plu_decompose accept.
// Plain integer arithmetic on plain integers, no HIP types, so that the same functions compile for the host alone
// (tests/csrc/elim_plan_host_test.cpp sweeps them; tests/elim_plan.py mirrors them for the GPU tests, which assert the route of every
// shape they name before they launch it).
#pragma once
#include <cstdint>

namespace gfa {
namespace elim_plan {

typedef int64_t i64;

constexpr int GJ_THREADS = 256;             // row_reduce_kernel, plu_kernel: one workgroup per matrix
constexpr int GJ_MAX_ROWS = 4096;           // their column factors are staged in LDS: one entry per row
constexpr i64 GJ_MAX_DIM = (i64)1 << 24;    // rows, columns: the kernels index a row or a column with an int, an element with 64 bits
constexpr i64 GJ_WIDE_MIN_ELEMS = 131072;   // m * n from which a matrix is worth two launches per column ...
constexpr i64 GJ_WIDE_MAX_BATCH = 32;       // ... when there are too few matrices to fill the chip with one workgroup each
constexpr i64 GJ_WIDE_ROW_TILE = 32;        // rows per workgroup of gj_eliminate_kernel, on gridDim.y (<= 65535)
constexpr i64 GJ_WIDE_MAX_ROWS = 65535 * GJ_WIDE_ROW_TILE;

enum Route { ONE_WORKGROUP = 0, TWO_KERNELS = 1, UNSUPPORTED = 2 };

// batch >= 1 matrices of m x n, m, n >= 1 (empty calls return before they are routed).
//   TWO_KERNELS ..... gj_pivot_kernel + gj_eliminate_kernel per column, the factors in global memory: few large matrices, and few
//                     matrices of more rows than the LDS array of the other route holds, whatever their size
//   ONE_WORKGROUP ... row_reduce_kernel, one workgroup per matrix
// m and n are at most 2^24, so m * n stays below 2^48: no overflow in 64 bits.
inline Route elim_route(i64 batch, i64 m, i64 n)
{
    if (batch < 1 || m < 1 || n < 1 || m > GJ_MAX_DIM || n > GJ_MAX_DIM) return UNSUPPORTED;
    if (batch <= GJ_WIDE_MAX_BATCH && (m * n >= GJ_WIDE_MIN_ELEMS || m > GJ_MAX_ROWS))
        return m <= GJ_WIDE_MAX_ROWS ? TWO_KERNELS : UNSUPPORTED;
    return m <= GJ_MAX_ROWS ? ONE_WORKGROUP : UNSUPPORTED;
}

// plu_kernel is the one-workgroup kind only
inline bool plu_supported(i64 m, i64 n) { return m >= 1 && n >= 1 && m <= GJ_MAX_ROWS && n <= GJ_MAX_DIM; }

} // namespace elim_plan
} // namespace gfa
