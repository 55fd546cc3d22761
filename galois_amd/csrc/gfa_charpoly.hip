// gfa_charpoly.hip -- characteristic polynomials det(xI - A) of square matrices on the device.
//
//   gfa_charpoly ...... replaces _characteristic_poly_matrix (_fields/_array.py:2409-2430), which expands the determinant of an
//                       n x n array of Python Poly objects.  Here: an O(n^3) elimination in two steps that need nothing but
//                       the inverses of the pivots, so every characteristic is served (Faddeev-LeVerrier divides by 1 .. n).
//
// Step 1, similarity reduction to upper Hessenberg form.  For m = 1 .. n-2: the first row i >= m with H[i][m-1] != 0 is
// exchanged with row m (rows AND columns i <-> m); with u_r = H[r][m-1] / H[m][m-1] every row r > m gets row_r -= u_r row_m
// (row phase, a rank-1 update), then col_m += sum_{r>m} u_r col_r over all n rows (column phase, a matrix-vector product).
// The u_r sit in one column of the transform, so all row operations of one m commute and may precede its column operation.
//
// Step 2, the Hessenberg recurrence.  p_0 = 1 and for m = 1 .. n
//     p_m(x) = (x - H[m-1][m-1]) p_{m-1}(x) - sum_{a=1}^{m-1} H[a-1][m-1] T_a p_{a-1}(x),   T_a = prod_{k=a}^{m-1} H[k][k-1].
// T is kept as an array: going from m-1 to m every T_a is multiplied by H[m-1][m-2] and T_{m-1} = H[m-1][m-2] is appended,
// so no step has a serial product chain.  All p_k live in a lower-triangular table (p_k at offset k (k + 1) / 2, ascending
// degree); threads own coefficient indices d and loop over a, so the reads of p_{a-1}[d] are contiguous across lanes.
//
// Two launch regimes, chosen as gfa_row_reduce chooses: one workgroup per matrix for stacks, and for few large matrices a
// handful of kernels per column with the row phase, the column phase and each recurrence step spread over all CUs and the
// per-matrix state (pivot found or not, factors, T) passed through device memory -- the host reads nothing back.
#include "gfa_internal.h"

using namespace gfa;

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_MAX_N = 4096;                   // factors / recurrence coefficients are staged in LDS
constexpr size_t CP_SCRATCH_BYTES = 1ull << 30;  // work buffers of one slice of the batch

__host__ __device__ __forceinline__ i64 tri(i64 k) { return k * (k + 1) / 2; } // offset of p_k in the table

template <class E>
__device__ __forceinline__ E shfl_down_e(E v, int off, int width)
{
    if constexpr (sizeof(E) == 8) {
        const u32 lo = __shfl_down((u32)v, (unsigned)off, width), hi = __shfl_down((u32)((u64)v >> 32), (unsigned)off, width);
        return (E)(((u64)hi << 32) | lo);
    } else {
        return (E)__shfl_down((u32)v, (unsigned)off, width);
    }
}

// sum_{r = r0 + lane, step g}^{n-1} u[r] row[r], folded over the g lanes of a group (g a power of two <= 64); lane 0 holds it
template <class F, typename T, typename U>
__device__ __forceinline__ typename F::elem group_dot(const FieldDev &fd, const T *row, const U *u, int r0, int n,
                                                      int lane, int g)
{
    typedef typename F::elem E;
    E acc = 0;
    for (int r = r0 + lane; r < n; r += g) acc = F::add(fd, acc, F::mul(fd, (E)u[r], (E)row[r]));
    for (int off = g >> 1; off > 0; off >>= 1) acc = F::add(fd, acc, shfl_down_e<E>(acc, off, g));
    return acc;
}

// sum_{a = d+1}^{m-1} c[a] p_{a-1}[d].  Every lane of a wave walks the same a (from the wave's first d) so that the reads
// of p_{a-1}[d] stay contiguous; d must be wave-aligned: lane l of a wave holds d0 + l with d0 a multiple of 64.
template <class F, typename T, typename C>
__device__ __forceinline__ typename F::elem rec_sum(const FieldDev &fd, const T *P, const C *c, int m, int d)
{
    typedef typename F::elem E;
    E acc = 0;
    int a = (d & ~63) + 1;
    i64 base = tri(a - 1);
    for (; a < m; base += a, a++) {
        if (d >= a) continue;
        const E ca = (E)c[a];
        if (ca != 0) acc = F::add(fd, acc, F::mul(fd, ca, (E)P[base + d]));
    }
    return acc;
}

// p_m[d] from p_{m-1} and the sum above
template <class F, typename T>
__device__ __forceinline__ typename F::elem rec_coeff(const FieldDev &fd, const T *P, typename F::elem diag,
                                                      typename F::elem sum, int m, int d)
{
    typedef typename F::elem E;
    const T *prev = P + tri(m - 1);
    E v = d >= 1 ? (E)prev[d - 1] : (E)0;
    if (d < m) v = F::sub(fd, v, F::mul(fd, diag, (E)prev[d]));
    return F::sub(fd, v, sum);
}

// ------------------------------------------------------------------------------------------------
// one workgroup per matrix.  H: scratch copies (batch, n, n); P: (batch, tri(n + 1)); Tall: (batch, n + 1)
// ------------------------------------------------------------------------------------------------
template <class F, typename T>
__global__ __launch_bounds__(CP_THREADS) void charpoly_wg_kernel(FieldDev fd, T *__restrict__ Hall, T *__restrict__ Pall,
                                                                 u64 *__restrict__ Tall, T *__restrict__ out_all, int n)
{
    typedef typename F::elem E;
    __shared__ E fac[CP_MAX_N]; // step 1: the factors u_r; step 2: c_a = H[a-1][m-1] T_a
    __shared__ int piv_row;
    __shared__ E piv_inv;
    T *H = Hall + (i64)blockIdx.x * n * n;
    T *P = Pall + (i64)blockIdx.x * tri(n + 1);
    u64 *Tp = Tall + (i64)blockIdx.x * (n + 1);
    T *out = out_all + (i64)blockIdx.x * (n + 1);
    const int tid = threadIdx.x;
    int g = 64; // lanes per row in the column phase
    while (g > 1 && (g >> 1) >= n) g >>= 1;

    for (int m = 1; m + 1 < n; m++) {
        if (tid == 0) piv_row = n;
        __syncthreads();
        for (int i = m + tid; i < n; i += CP_THREADS)
            if (H[(i64)i * n + m - 1] != 0) { atomicMin(&piv_row, i); break; } // rows ascend per thread: first hit is its minimum
        __syncthreads();
        const int pr = piv_row;
        if (pr == n) { __syncthreads(); continue; }
        if (pr != m) {
            // rows m and pr are zero left of column m-1
            for (int c = m - 1 + tid; c < n; c += CP_THREADS) {
                const T t = H[(i64)m * n + c]; H[(i64)m * n + c] = H[(i64)pr * n + c]; H[(i64)pr * n + c] = t;
            }
            __syncthreads();
            for (int k = tid; k < n; k += CP_THREADS) {
                const T t = H[(i64)k * n + m]; H[(i64)k * n + m] = H[(i64)k * n + pr]; H[(i64)k * n + pr] = t;
            }
            __syncthreads();
        }
        if (tid == 0) piv_inv = F::inv(fd, (E)H[(i64)m * n + m - 1]);
        __syncthreads();
        const E inv = piv_inv;
        for (int r = m + 1 + tid; r < n; r += CP_THREADS) {
            fac[r] = F::mul(fd, (E)H[(i64)r * n + m - 1], inv);
            H[(i64)r * n + m - 1] = 0; // what row_r -= u_r row_m leaves in column m-1
        }
        __syncthreads();
        // row phase: H[r, m:] -= u_r H[m, m:] for r > m.  Threads tile (rows x columns) with a power-of-two column count.
        {
            const int width = n - m;
            int tcols = CP_THREADS;
            while (tcols > 1 && (tcols >> 1) >= width) tcols >>= 1;
            const int lc = tid & (tcols - 1), r0 = tid / tcols, rstep = CP_THREADS / tcols;
            for (int c = m + lc; c < n; c += tcols) {
                const E pv = (E)H[(i64)m * n + c];
                if (pv == 0) continue;
                for (int r = m + 1 + r0; r < n; r += rstep) {
                    const E f = fac[r];
                    if (f != 0) H[(i64)r * n + c] = (T)F::sub(fd, (E)H[(i64)r * n + c], F::mul(fd, f, pv));
                }
            }
        }
        __syncthreads();
        // column phase: H[k, m] += sum_{r > m} u_r H[k, r] for every row k, g lanes per row
        {
            const int lane = tid & (g - 1), grp = tid / g, ngrp = CP_THREADS / g;
            for (int k = grp; k < n; k += ngrp) {
                const E s = group_dot<F, T, E>(fd, H + (i64)k * n, fac, m + 1, n, lane, g);
                if (lane == 0) H[(i64)k * n + m] = (T)F::add(fd, (E)H[(i64)k * n + m], s);
            }
        }
        __syncthreads();
    }

    if (tid == 0) P[0] = (T)F::one(fd);
    __syncthreads();
    for (int m = 1; m <= n; m++) {
        if (m >= 2) {
            const E h = (E)H[(i64)(m - 1) * n + m - 2];
            for (int a = 1 + tid; a < m; a += CP_THREADS) {
                const E Ta = a == m - 1 ? h : F::mul(fd, (E)Tp[a], h);
                Tp[a] = (u64)Ta;
                fac[a] = F::mul(fd, (E)H[(i64)(a - 1) * n + m - 1], Ta);
            }
        }
        __syncthreads();
        const E diag = (E)H[(i64)(m - 1) * n + m - 1];
        T *cur = P + tri(m);
        for (int d = tid; d <= m; d += CP_THREADS)
            cur[d] = (T)rec_coeff<F, T>(fd, P, diag, rec_sum<F, T, E>(fd, P, fac, m, d), m, d);
        __syncthreads();
    }
    const T *pn = P + tri(n);
    for (int j = tid; j <= n; j += CP_THREADS) out[j] = pn[n - j];
}

// ------------------------------------------------------------------------------------------------
// few large matrices: four kernels per column
// ------------------------------------------------------------------------------------------------
// pivot search in column m-1, the row and column exchange, the factors u_r.  One workgroup per matrix.
template <class F, typename T>
__global__ __launch_bounds__(1024) void hz_pivot_kernel(FieldDev fd, T *__restrict__ Hall, int n, int m, int *__restrict__ has_all,
                                                        u64 *__restrict__ factor_all)
{
    typedef typename F::elem E;
    __shared__ int piv_row;
    __shared__ E piv_inv;
    T *H = Hall + (i64)blockIdx.x * n * n;
    u64 *factor = factor_all + (i64)blockIdx.x * n;
    const int tid = threadIdx.x;
    if (tid == 0) piv_row = n;
    __syncthreads();
    for (int i = m + tid; i < n; i += 1024)
        if (H[(i64)i * n + m - 1] != 0) { atomicMin(&piv_row, i); break; }
    __syncthreads();
    const int pr = piv_row;
    if (pr >= n) {
        if (tid == 0) has_all[blockIdx.x] = 0;
        return;
    }
    if (pr != m) {
        for (int c = m - 1 + tid; c < n; c += 1024) {
            const T t = H[(i64)m * n + c]; H[(i64)m * n + c] = H[(i64)pr * n + c]; H[(i64)pr * n + c] = t;
        }
        __syncthreads();
        for (int k = tid; k < n; k += 1024) {
            const T t = H[(i64)k * n + m]; H[(i64)k * n + m] = H[(i64)k * n + pr]; H[(i64)k * n + pr] = t;
        }
        __syncthreads();
    }
    if (tid == 0) piv_inv = F::inv(fd, (E)H[(i64)m * n + m - 1]);
    __syncthreads();
    const E inv = piv_inv;
    for (int r = m + 1 + tid; r < n; r += 1024) {
        factor[r] = (u64)F::mul(fd, (E)H[(i64)r * n + m - 1], inv);
        H[(i64)r * n + m - 1] = 0;
    }
    if (tid == 0) has_all[blockIdx.x] = 1;
}

// row phase.  grid: (column tiles of 64 from column m, row tiles of 32 from row m+1, batch)
template <class F, typename T>
__global__ __launch_bounds__(256) void hz_row_kernel(FieldDev fd, T *__restrict__ Hall, int n, int m, const int *__restrict__ has_all,
                                                     const u64 *__restrict__ factor_all)
{
    typedef typename F::elem E;
    if (!has_all[blockIdx.z]) return;
    T *H = Hall + (i64)blockIdx.z * n * n;
    const u64 *factor = factor_all + (i64)blockIdx.z * n;
    const int c = m + blockIdx.x * 64 + (threadIdx.x & 63);
    if (c >= n) return;
    const E pv = (E)H[(i64)m * n + c];
    if (pv == 0) return;
    const int r_beg = m + 1 + blockIdx.y * 32;
    const int r_end = min(n, r_beg + 32);
    for (int r = r_beg + (threadIdx.x >> 6); r < r_end; r += 4) {
        const E f = (E)factor[r];
        if (f != 0) H[(i64)r * n + c] = (T)F::sub(fd, (E)H[(i64)r * n + c], F::mul(fd, f, pv));
    }
}

// column phase: one wave per row.  grid: (ceil(n / 4), batch)
template <class F, typename T>
__global__ __launch_bounds__(256) void hz_col_kernel(FieldDev fd, T *__restrict__ Hall, int n, int m, const int *__restrict__ has_all,
                                                     const u64 *__restrict__ factor_all)
{
    typedef typename F::elem E;
    if (!has_all[blockIdx.y]) return;
    T *H = Hall + (i64)blockIdx.y * n * n;
    const u64 *factor = factor_all + (i64)blockIdx.y * n;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= n) return; // the whole wave leaves together
    const E s = group_dot<F, T, u64>(fd, H + (i64)k * n, factor, m + 1, n, lane, 64);
    if (lane == 0) H[(i64)k * n + m] = (T)F::add(fd, (E)H[(i64)k * n + m], s);
}

// one recurrence step, a grid over d.  grid: (ceil((m + 1) / 256), batch).  Every workgroup rebuilds the c_a it needs in
// LDS from the previous step's T (T_old); workgroup 0 needs them all and writes the new T into the other buffer (T_new).
template <class F, typename T>
__global__ __launch_bounds__(256) void hz_rec_kernel(FieldDev fd, const T *__restrict__ Hall, T *__restrict__ Pall,
                                                     const u64 *__restrict__ Told_all, u64 *__restrict__ Tnew_all, int n, int m)
{
    typedef typename F::elem E;
    __shared__ E c[CP_MAX_N];
    const T *H = Hall + (i64)blockIdx.y * n * n;
    T *P = Pall + (i64)blockIdx.y * tri(n + 1);
    const u64 *Told = Told_all + (i64)blockIdx.y * (n + 1);
    u64 *Tnew = Tnew_all + (i64)blockIdx.y * (n + 1);
    const int tid = threadIdx.x;
    if (m == 1 && blockIdx.x == 0 && tid == 0) P[0] = (T)F::one(fd); // p_0, read after the barrier by d = 0 and d = 1
    if (m >= 2) {
        const E h = (E)H[(i64)(m - 1) * n + m - 2];
        for (int a = blockIdx.x * 256 + 1 + tid; a < m; a += 256) {
            const E Ta = a == m - 1 ? h : F::mul(fd, (E)Told[a], h);
            if (blockIdx.x == 0) Tnew[a] = (u64)Ta;
            c[a] = F::mul(fd, (E)H[(i64)(a - 1) * n + m - 1], Ta);
        }
    }
    __syncthreads();
    const int d = blockIdx.x * 256 + tid;
    if (d > m) return;
    const E diag = (E)H[(i64)(m - 1) * n + m - 1];
    P[tri(m) + d] = (T)rec_coeff<F, T>(fd, P, diag, rec_sum<F, T, E>(fd, P, c, m, d), m, d);
}

// out[b][j] = p_n[n - j].  grid: (ceil((n + 1) / 256), batch)
template <typename T>
__global__ void cp_write_kernel(const T *__restrict__ Pall, T *__restrict__ out_all, int n)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    out_all[(i64)blockIdx.y * (n + 1) + j] = Pall[(i64)blockIdx.y * tri(n + 1) + tri(n) + n - j];
}

template <typename T>
__global__ void cp_fill_kernel(T *__restrict__ out, i64 count, T value)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = value;
}

template <class F, typename T>
int launch_charpoly_ft(const FieldDev &fd, const void *a, void *out, i64 batch, i64 n, bool chip_wide, hipStream_t st)
{
    if (n == 0) { // det of the empty matrix: the constant 1
        hipLaunchKernelGGL((cp_fill_kernel<T>), dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, (T *)out, batch, (T)1);
        GFA_HIP(hipGetLastError());
        return GFA_OK;
    }
    // work buffers of one slice: the copy of A, the table of p_k, T (two copies: the chip-wide steps ping-pong), factors, flags
    const size_t per_matrix = sizeof(T) * (size_t)(n * n + tri(n + 1)) + sizeof(u64) * (size_t)(2 * (n + 1) + n) + sizeof(int);
    i64 slice = (i64)(CP_SCRATCH_BYTES / per_matrix);
    if (slice < 1) slice = 1;
    if (slice > 65535) slice = 65535; // the batch rides on a grid dimension
    if (slice > batch) slice = batch;
    T *H = nullptr, *P = nullptr;
    u64 *Tb = nullptr, *factor = nullptr;
    int *has = nullptr;
    Scratch ws(st);
    GFA_HIP(ws.get(&H, (size_t)(slice * n * n)));
    GFA_HIP(ws.get(&P, (size_t)(slice * tri(n + 1))));
    GFA_HIP(ws.get(&Tb, (size_t)(2 * slice * (n + 1))));
    GFA_HIP(ws.get(&factor, (size_t)(slice * n)));
    GFA_HIP(ws.get(&has, (size_t)slice));
    u64 *Tbuf[2] = {Tb, Tb + slice * (n + 1)};
    for (i64 b0 = 0; b0 < batch; b0 += slice) {
        const i64 nb = batch - b0 < slice ? batch - b0 : slice;
        T *o = (T *)out + b0 * (n + 1);
        GFA_HIP(hipMemcpyAsync(H, (const T *)a + b0 * n * n, sizeof(T) * (size_t)(nb * n * n), hipMemcpyDeviceToDevice, st));
        if (!chip_wide) {
            hipLaunchKernelGGL((charpoly_wg_kernel<F, T>), dim3((unsigned)nb), dim3(CP_THREADS), 0, st, fd, H, P, Tbuf[0], o, (int)n);
            GFA_HIP(hipGetLastError());
            continue;
        }
        for (i64 m = 1; m + 1 < n; m++) {
            hipLaunchKernelGGL((hz_pivot_kernel<F, T>), dim3((unsigned)nb), dim3(1024), 0, st, fd, H, (int)n, (int)m, has, factor);
            const dim3 rgrid((unsigned)((n - m + 63) / 64), (unsigned)((n - m - 1 + 31) / 32), (unsigned)nb);
            hipLaunchKernelGGL((hz_row_kernel<F, T>), rgrid, dim3(256), 0, st, fd, H, (int)n, (int)m, has, factor);
            hipLaunchKernelGGL((hz_col_kernel<F, T>), dim3((unsigned)((n + 3) / 4), (unsigned)nb), dim3(256), 0, st, fd, H, (int)n,
                               (int)m, has, factor);
        }
        GFA_HIP(hipGetLastError());
        for (i64 m = 1; m <= n; m++)
            hipLaunchKernelGGL((hz_rec_kernel<F, T>), dim3((unsigned)((m + 1 + 255) / 256), (unsigned)nb), dim3(256), 0, st, fd, H, P,
                               Tbuf[m & 1], Tbuf[(m & 1) ^ 1], (int)n, (int)m);
        hipLaunchKernelGGL((cp_write_kernel<T>), dim3((unsigned)((n + 1 + 255) / 256), (unsigned)nb), dim3(256), 0, st, P, o, (int)n);
        GFA_HIP(hipGetLastError());
    }
    return GFA_OK;
}

int dispatch_charpoly(const FieldDev &fd, int dtype, const void *a, void *out, i64 batch, i64 n, bool chip_wide, hipStream_t st)
{
    GFA_DISPATCH_FT(launch_charpoly_ft, fd, dtype, fd, a, out, batch, n, chip_wide, st);
}

} // namespace

extern "C" {

int gfa_charpoly(gfa_field_t *f, const void *a, void *coeffs_out, int64_t batch, int64_t n, int dtype, gfa_stream_t stream)
{
    if (!f || batch < 0 || n < 0) { set_error("gfa_charpoly: bad arguments"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0) return GFA_OK;
    if (!coeffs_out || (n > 0 && !a)) { set_error("gfa_charpoly: bad arguments"); return GFA_ERR_INVALID; }
    if (n > CP_MAX_N) { set_error("gfa_charpoly: matrix too large (at most 4096 rows)"); return GFA_ERR_UNSUPPORTED; }
    FieldDeviceState *ds;
    int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    const FieldDev fd = f->use_lookup() ? f->lut_desc(*ds) : f->calc;
    // few large matrices: kernels per column spread over all CUs; otherwise one workgroup per matrix
    const bool chip_wide = n * n >= 131072 && batch <= 32;
    return dispatch_charpoly(fd, dtype, a, coeffs_out, batch, n, chip_wide, (hipStream_t)stream);
}

} // extern "C"
