// gfa_reduce.hip -- ufunc.reduce / reduceat / accumulate over the last axis (the reference's _ufunc.py reduce / accumulate seams).
// add / multiply fold as trees; subtract / divide are the reference's left folds a0 - fold(rest), a0 / fold(rest).
#include <algorithm>
#include <map>

#include "gfa_internal.h"
#include "gfa_reduce_plan.h"

using namespace gfa;

namespace {

template <class F, typename T, bool IS_MUL>
__global__ __launch_bounds__(256) void reduce_segments_kernel(FieldDev fd, const T *__restrict__ in, i64 n_inner,
                                                              i64 col_begin, i64 seg_len, i64 nseg,
                                                              u64 *__restrict__ partial)
{
    typedef typename F::elem E;
    __shared__ u64 sh[256];
    const i64 row = blockIdx.x / nseg, seg = blockIdx.x % nseg;
    const i64 lo = col_begin + seg * seg_len;
    i64 hi = lo + seg_len;
    if (hi > n_inner) hi = n_inner;
    const T *x = in + row * n_inner;
    E acc = IS_MUL ? F::one(fd) : (E)0;
    for (i64 i = lo + threadIdx.x; i < hi; i += 256) {
        E v = (E)x[i];
        acc = IS_MUL ? F::mul(fd, acc, v) : F::add(fd, acc, v);
    }
    sh[threadIdx.x] = (u64)acc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            E a = (E)sh[threadIdx.x], b = (E)sh[threadIdx.x + off];
            sh[threadIdx.x] = (u64)(IS_MUL ? F::mul(fd, a, b) : F::add(fd, a, b));
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// mode 0: out = reduce(partials); 1: out = a0 - sum(partials); 2: out = a0 / prod(partials)
template <class F, typename T, bool IS_MUL>
__global__ void reduce_finalize_kernel(FieldDev fd, const T *__restrict__ in, i64 n_inner, const u64 *__restrict__ partial,
                                       i64 nseg, T *__restrict__ out, i64 n_outer, int mode, int32_t *err)
{
    typedef typename F::elem E;
    const i64 row = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (row < n_outer) {
        E acc = IS_MUL ? F::one(fd) : (E)0;
        for (i64 s = 0; s < nseg; s++) {
            E v = (E)partial[row * nseg + s];
            acc = IS_MUL ? F::mul(fd, acc, v) : F::add(fd, acc, v);
        }
        if (mode == 1) acc = F::sub(fd, (E)in[row * n_inner], acc);
        if (mode == 2) {
            E a0 = (E)in[row * n_inner];
            if (acc == 0) { bad = true; acc = 0; }
            else if (a0 == 0) acc = 0;
            else {
                if constexpr (std::is_same<F, Lut>::value) acc = Lut::div_nz(fd, a0, acc);
                else acc = F::mul(fd, a0, F::inv(fd, acc));
            }
        }
        out[row] = (T)acc;
    }
    flag_error(err, bad);
}

// ufunc.reduceat: out[s] = fold(a[starts[s] : ends[s]]) with NumPy's convention that an empty or reversed slice yields
// a[starts[s]].  One 64-lane workgroup per segment; subtract / divide are left folds a0 - sum(rest), a0 / prod(rest).
template <class F, typename T, bool IS_MUL>
__global__ __launch_bounds__(64) void reduce_ragged_kernel(FieldDev fd, const T *__restrict__ in, const i64 *__restrict__ starts,
                                                           const i64 *__restrict__ ends, T *__restrict__ out, int mode, int32_t *err)
{
    typedef typename F::elem E;
    __shared__ u64 sh[64];
    const i64 lo = starts[blockIdx.x];
    i64 hi = ends[blockIdx.x];
    if (hi <= lo) hi = lo + 1;
    const i64 first = mode ? lo + 1 : lo;
    E acc = IS_MUL ? F::one(fd) : (E)0;
    for (i64 i = first + threadIdx.x; i < hi; i += 64) {
        const E v = (E)in[i];
        acc = IS_MUL ? F::mul(fd, acc, v) : F::add(fd, acc, v);
    }
    sh[threadIdx.x] = (u64)acc;
    __syncthreads();
    for (int off = 32; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const E x = (E)sh[threadIdx.x], y = (E)sh[threadIdx.x + off];
            sh[threadIdx.x] = (u64)(IS_MUL ? F::mul(fd, x, y) : F::add(fd, x, y));
        }
        __syncthreads();
    }
    bool bad = false;
    if (threadIdx.x == 0) {
        E r = (E)sh[0];
        if (mode == 1) r = F::sub(fd, (E)in[lo], r);
        if (mode == 2) {
            const E a0 = (E)in[lo];
            if (r == 0) { bad = true; r = 0; }
            else if (a0 == 0) r = 0;
            else {
                if constexpr (std::is_same<F, Lut>::value) r = Lut::div_nz(fd, a0, r);
                else r = F::mul(fd, a0, F::inv(fd, r));
            }
        }
        out[blockIdx.x] = (T)r;
    }
    flag_error(err, bad);
}

template <class F, typename T>
int launch_reduceat_ft(const FieldDev &fd, int op, const void *a, const i64 *starts, const i64 *ends, i64 nseg, void *out,
                       hipStream_t st, int32_t *err)
{
    const bool is_mul = op == GFA_OP_MUL || op == GFA_OP_DIV;
    const int mode = op == GFA_OP_SUB ? 1 : op == GFA_OP_DIV ? 2 : 0;
    if (is_mul)
        hipLaunchKernelGGL((reduce_ragged_kernel<F, T, true>), dim3((unsigned)nseg), dim3(64), 0, st, fd, (const T *)a, starts, ends,
                           (T *)out, mode, err);
    else
        hipLaunchKernelGGL((reduce_ragged_kernel<F, T, false>), dim3((unsigned)nseg), dim3(64), 0, st, fd, (const T *)a, starts, ends,
                           (T *)out, mode, err);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}
int dispatch_reduceat(const FieldDev &fd, int dtype, int op, const void *a, const i64 *starts, const i64 *ends, i64 nseg, void *out,
                      hipStream_t st, int32_t *err)
{
    GFA_DISPATCH_FT(launch_reduceat_ft, fd, dtype, fd, op, a, starts, ends, nseg, out, st, err);
}

// ---- r06: streaming forms of the folds a 1-D array of 1e8 elements asks for (the generic kernel above reads one element per lane and load:
// 0.04 of the roofline for np.add.reduce over GF(2^8)) ----
// MODE 0: xor of the words (every field of characteristic 2: the fold of the elements is the fold of the packed words, folded once more
//         across the word at the end).  MODE 1: plain integer sums in 64 bits, reduced mod p once per block (prime fields, elements of at
//         most 32 bits: a block adds at most 2^32 of them).  MODE 2: np.multiply.reduce of a table field of at most 256 elements: sum of
//         LOG[x] from a 256-entry LDS table, EXP once per block, zero if any element is zero.
// Each block covers [lo, hi) of one row: 16-byte loads over the aligned middle, the unaligned head and tail element by element.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void reduce_stream_kernel(const T *__restrict__ in, i64 n_inner, i64 col_begin, i64 seg_len, i64 nseg, u64 *__restrict__ partial,
                                                            u64 p, const uint8_t *__restrict__ log8, const uint8_t *__restrict__ exp8, u32 qm1)
{
    __shared__ u64 sh[256];
    __shared__ uint8_t lg[256];
    __shared__ int any_zero;
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_add8[]; // MODE 3: the field's 64 KiB sum table (log8 points at it)
    if (MODE == 3) {
        const uint4 *s0 = reinterpret_cast<const uint4 *>(log8);
        uint4 *d0 = reinterpret_cast<uint4 *>(rs_add8);
        for (int i = threadIdx.x; i < 4096; i += 256) d0[i] = s0[i];
        __syncthreads();
    }
    if (MODE == 2) {
        lg[threadIdx.x] = log8[threadIdx.x];
        if (threadIdx.x == 0) any_zero = 0;
        __syncthreads();
    }
    constexpr int V = 16 / (int)sizeof(T);
    const i64 row = blockIdx.x / nseg, seg = blockIdx.x % nseg;
    const i64 lo = col_begin + seg * seg_len;
    i64 hi = lo + seg_len;
    if (hi > n_inner) hi = n_inner;
    const T *x = in + row * n_inner;
    u64 acc = 0;
    u32 a4[4] = {0, 0, 0, 0}; // MODE 3: four chains of table additions per lane (independent gathers in flight)
    bool zero = false;
    auto one = [&](T v) {
        if (MODE == 0) acc ^= (u64)v;
        else if (MODE == 1) acc += (u64)v;
        else if (MODE == 2) { zero |= v == 0; acc += (u64)lg[(uint8_t)v]; }
        else a4[0] = rs_add8[(a4[0] << 8) | (u32)(uint8_t)v];
    };
    if (hi > lo) {
        const uintptr_t addr = reinterpret_cast<uintptr_t>(x + lo);
        i64 head = (i64)(((16 - (addr & 15)) & 15) / sizeof(T));
        if (head > hi - lo) head = hi - lo;
        const i64 a_lo = lo + head, nvec = (hi - a_lo) / V, a_hi = a_lo + nvec * V;
        if ((i64)threadIdx.x < head) one(x[lo + threadIdx.x]);
        if (a_hi + (i64)threadIdx.x < hi) one(x[a_hi + threadIdx.x]);
        const uint4 *xv = reinterpret_cast<const uint4 *>(x + a_lo);
        if (MODE == 0) {
            u32 w0 = 0, w1 = 0, w2 = 0, w3 = 0;
            for (i64 v = threadIdx.x; v < nvec; v += 256) { const uint4 w = xv[v]; w0 ^= w.x; w1 ^= w.y; w2 ^= w.z; w3 ^= w.w; }
            u32 w = w0 ^ w1 ^ w2 ^ w3; // the elements of the four words sit at the same offsets inside a word (sizeof(T) divides 4), or T is 8 bytes
            if (sizeof(T) == 8) acc ^= ((u64)(w1 ^ w3) << 32) | (u64)(w0 ^ w2);
            else {
                if (sizeof(T) <= 2) w ^= w >> 16;
                if (sizeof(T) == 1) w ^= w >> 8;
                acc ^= (u64)(w & (sizeof(T) == 1 ? 0xffu : sizeof(T) == 2 ? 0xffffu : 0xffffffffu));
            }
        } else {
            for (i64 v = threadIdx.x; v < nvec; v += 256) {
                const uint4 w = xv[v];
                const u32 ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (sizeof(T) == 4) one((T)ww[j]);
                    else if (sizeof(T) == 2) { one((T)(ww[j] & 0xffffu)); one((T)(ww[j] >> 16)); }
                    else if (sizeof(T) == 1) {
                        if (MODE == 3) { // static chain per byte lane of the word
#pragma unroll
                            for (int b = 0; b < 4; b++) a4[b] = rs_add8[(a4[b] << 8) | ((ww[j] >> (8 * b)) & 0xffu)];
                        } else { one((T)(ww[j] & 0xffu)); one((T)((ww[j] >> 8) & 0xffu)); one((T)((ww[j] >> 16) & 0xffu)); one((T)(ww[j] >> 24)); }
                    }
                }
                if (sizeof(T) == 8) { one((T)(((u64)w.y << 32) | w.x)); one((T)(((u64)w.w << 32) | w.z)); }
            }
        }
    }
    if (MODE == 2 && zero) any_zero = 1; // (benign race: every writer stores 1)
    if (MODE == 3) {
        u32 r = rs_add8[(a4[0] << 8) | a4[1]];
        r = rs_add8[(r << 8) | a4[2]];
        acc = rs_add8[(r << 8) | a4[3]];
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            if (MODE == 3) sh[threadIdx.x] = rs_add8[(sh[threadIdx.x] << 8) | sh[threadIdx.x + off]];
            else sh[threadIdx.x] = MODE == 0 ? sh[threadIdx.x] ^ sh[threadIdx.x + off] : sh[threadIdx.x] + sh[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        u64 r = sh[0];
        if (MODE == 1) r %= p;
        if (MODE == 2) r = any_zero ? 0 : (u64)exp8[r % qm1];
        partial[blockIdx.x] = r;
    }
}

// the same finalisation with ONE WORKGROUP per row: a 1-D array is cut into up to 4096 segments, and one thread walking their partial results
// was 180 of the 196 us np.add.reduce took over 1e8 bytes (r06)
template <class F, typename T, bool IS_MUL>
__global__ __launch_bounds__(256) void reduce_finalize_block_kernel(FieldDev fd, const T *__restrict__ in, i64 n_inner, const u64 *__restrict__ partial,
                                                                    i64 nseg, T *__restrict__ out, int mode, int32_t *err)
{
    typedef typename F::elem E;
    __shared__ u64 sh[256];
    const i64 row = blockIdx.x;
    E acc = IS_MUL ? F::one(fd) : (E)0;
    for (i64 sg = threadIdx.x; sg < nseg; sg += 256) {
        const E v = (E)partial[row * nseg + sg];
        acc = IS_MUL ? F::mul(fd, acc, v) : F::add(fd, acc, v);
    }
    sh[threadIdx.x] = (u64)acc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const E a = (E)sh[threadIdx.x], b = (E)sh[threadIdx.x + off];
            sh[threadIdx.x] = (u64)(IS_MUL ? F::mul(fd, a, b) : F::add(fd, a, b));
        }
        __syncthreads();
    }
    bool bad = false;
    if (threadIdx.x == 0) {
        acc = (E)sh[0];
        if (mode == 1) acc = F::sub(fd, (E)in[row * n_inner], acc);
        if (mode == 2) {
            const E a0 = (E)in[row * n_inner];
            if (acc == 0) { bad = true; acc = 0; }
            else if (a0 == 0) acc = 0;
            else {
                if constexpr (std::is_same<F, Lut>::value) acc = Lut::div_nz(fd, a0, acc);
                else acc = F::mul(fd, a0, F::inv(fd, acc));
            }
        }
        out[row] = (T)acc;
    }
    flag_error(err, bad);
}

// byte LOG / EXP / sum table of the field a gfa_reduce / gfa_accumulate call is for (q <= 256; null otherwise)
struct ByteTables {
    const uint8_t *log8 = nullptr, *exp8 = nullptr, *add8 = nullptr;
};

// The segment folds of a call go to a buffer of the stream's own, taken from the pool (gfa::scratch_alloc) and kept for the next call on
// that stream: calls on one stream are ordered by the stream, calls on two streams never share a buffer.  (With a pool allocation and
// release per call, each call returned only once the device had caught up: 3-8 us more per np.add.reduce / np.multiply.reduce of a long
// row.)  The lock is held until the launches that use the buffer are queued, so that a concurrent call on the same stream cannot release
// it in between.
std::mutex g_partials_mu;
std::map<std::pair<int, hipStream_t>, std::pair<u64 *, size_t>> g_partials; // (device, stream) -> (buffer, entries)

template <class Launch>
int with_partials(hipStream_t st, size_t n, const Launch &launch)
{
    int d = 0;
    GFA_HIP(hipGetDevice(&d));
    std::lock_guard<std::mutex> lock(g_partials_mu);
    std::pair<u64 *, size_t> &b = g_partials[{d, st}];
    if (b.second < n) {
        if (b.first) GFA_HIP(scratch_free(b.first, st));
        b = {nullptr, 0};
        GFA_HIP(scratch_alloc((void **)&b.first, n * sizeof(u64), st));
        b.second = n;
    }
    launch(b.first);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

// the fold of each of nseg segments of every row into partial[row * nseg + seg]: the streaming kernels where the fold is an xor of words / an
// integer sum / a sum of byte logarithms (r06), else the generic kernel
template <class F, typename T>
void reduce_phase1(const FieldDev &fd, const ByteTables &bt, bool is_mul, const void *a, i64 n_inner, i64 col_begin, i64 seg_len, i64 nseg, i64 n_outer, u64 *partial,
                   hipStream_t st)
{
    const unsigned grid = (unsigned)(n_outer * nseg);
    // (gfa_reduce_plan.h; 3: odd-characteristic table fields, the sum table in LDS)
    const int stream_mode = reduce_plan::stream_mode(is_mul, fd.p, fd.m, fd.q, std::is_same<F, Lut>::value, (int)sizeof(T), bt.log8 && bt.exp8, bt.add8 != nullptr, seg_len);
    if (stream_mode == 0)
        hipLaunchKernelGGL((reduce_stream_kernel<T, 0>), dim3(grid), dim3(256), 0, st, (const T *)a, n_inner, col_begin, seg_len, nseg, partial, (u64)fd.p, nullptr, nullptr, 0u);
    else if (stream_mode == 1)
        hipLaunchKernelGGL((reduce_stream_kernel<T, 1>), dim3(grid), dim3(256), 0, st, (const T *)a, n_inner, col_begin, seg_len, nseg, partial, (u64)fd.p, nullptr, nullptr, 0u);
    else if (stream_mode == 2)
        hipLaunchKernelGGL((reduce_stream_kernel<T, 2>), dim3(grid), dim3(256), 0, st, (const T *)a, n_inner, col_begin, seg_len, nseg, partial, (u64)fd.p, bt.log8,
                           bt.exp8, (u32)(fd.q - 1));
    else if (stream_mode == 3) {
        static bool attr = false;
        auto k3 = reduce_stream_kernel<T, 3>;
        if (!attr) { (void)hipFuncSetAttribute((const void *)k3, hipFuncAttributeMaxDynamicSharedMemorySize, 65536); attr = true; }
        hipLaunchKernelGGL(k3, dim3(grid), dim3(256), 65536, st, (const T *)a, n_inner, col_begin, seg_len, nseg, partial, (u64)fd.p, bt.add8, nullptr, 0u);
    } else if (is_mul)
        hipLaunchKernelGGL((reduce_segments_kernel<F, T, true>), dim3(grid), dim3(256), 0, st, fd, (const T *)a, n_inner, col_begin, seg_len, nseg, partial);
    else
        hipLaunchKernelGGL((reduce_segments_kernel<F, T, false>), dim3(grid), dim3(256), 0, st, fd, (const T *)a, n_inner, col_begin, seg_len, nseg, partial);
}

template <class F, typename T>
int launch_reduce_ft(const FieldDev &fd, const ByteTables &bt, int op, const void *a, void *out, i64 n_outer, i64 n_inner, hipStream_t st,
                     int32_t *err)
{
    const bool is_mul = op == GFA_OP_MUL || op == GFA_OP_DIV;
    const int mode = op == GFA_OP_SUB ? 1 : op == GFA_OP_DIV ? 2 : 0;
    const i64 col_begin = mode ? 1 : 0;
    const i64 len = n_inner - col_begin;
    // enough segments to fill the chip when there are few rows, at least 4096 elements each (gfa_reduce_plan.h)
    // (the sum-table fold of reduce_phase1 stages 64 KiB per workgroup: two workgroups per CU, long segments)
    const bool tab_add = reduce_plan::table_sum(is_mul, std::is_same<F, Lut>::value, (int)sizeof(T), fd.q, fd.m, bt.add8 != nullptr);
    const reduce_plan::Segments sg = reduce_plan::reduce_segments(n_outer, len, num_cus(), tab_add);
    const i64 nseg = sg.nseg, seg_len = sg.seg_len;
    return with_partials(st, (size_t)(n_outer * nseg), [&](u64 *partial) {
        reduce_phase1<F, T>(fd, bt, is_mul, a, n_inner, col_begin, seg_len, nseg, n_outer, partial, st);
        if (reduce_plan::block_join(nseg)) { // few rows, many segments: a workgroup per row
            if (is_mul)
                hipLaunchKernelGGL((reduce_finalize_block_kernel<F, T, true>), dim3((unsigned)n_outer), dim3(256), 0, st, fd, (const T *)a, n_inner, partial, nseg, (T *)out, mode, err);
            else
                hipLaunchKernelGGL((reduce_finalize_block_kernel<F, T, false>), dim3((unsigned)n_outer), dim3(256), 0, st, fd, (const T *)a, n_inner, partial, nseg, (T *)out, mode, err);
        } else if (is_mul)
            hipLaunchKernelGGL((reduce_finalize_kernel<F, T, true>), dim3((unsigned)((n_outer + 255) / 256)), dim3(256), 0, st, fd, (const T *)a, n_inner, partial, nseg,
                               (T *)out, n_outer, mode, err);
        else
            hipLaunchKernelGGL((reduce_finalize_kernel<F, T, false>), dim3((unsigned)((n_outer + 255) / 256)), dim3(256), 0, st, fd, (const T *)a, n_inner, partial, nseg,
                               (T *)out, n_outer, mode, err);
    });
}

int dispatch_reduce(const FieldDev &fd, const ByteTables &bt, int dtype, int op, const void *a, void *out, i64 n_outer, i64 n_inner,
                    hipStream_t st, int32_t *err)
{
    GFA_DISPATCH_FT(launch_reduce_ft, fd, dtype, fd, bt, op, a, out, n_outer, n_inner, st, err);
}

// ufunc.accumulate over the last axis: one workgroup per row, 256-element chunks scanned in LDS with a running carry.
// mode 0: inclusive scan with the op; 1: out[i] = a0 - (a1 + ... + ai); 2: out[i] = a0 / (a1 * ... * ai)
// r06: a row may be cut into nseg segments of seg_len elements, one workgroup each, that start from carry_in[row * nseg + seg] -- the fold of
// everything before the segment (accumulate_carries_kernel) -- so that ONE long row fills the chip; nseg = 1, carry_in = nullptr: the whole row.
template <class F, typename T, bool IS_MUL>
__global__ __launch_bounds__(256) void accumulate_kernel(FieldDev fd, const T *__restrict__ in, T *__restrict__ out, i64 n_inner,
                                                         int mode, int32_t *err, i64 nseg, i64 seg_len, const u64 *__restrict__ carry_in)
{
    typedef typename F::elem E;
    __shared__ u64 sh[256];
    const i64 row = (i64)blockIdx.x / nseg, seg = (i64)blockIdx.x % nseg;
    const T *x = in + row * n_inner;
    T *y = out + row * n_inner;
    const E ident = IS_MUL ? F::one(fd) : (E)0;
    const E a0 = (E)x[0];
    E carry = carry_in ? (E)carry_in[blockIdx.x] : ident;
    bool bad = false;
    const i64 start = (mode ? 1 : 0) + seg * seg_len;
    i64 stop = nseg == 1 ? n_inner : start + seg_len;
    if (stop > n_inner) stop = n_inner;
    if (mode && seg == 0 && threadIdx.x == 0) y[0] = (T)a0;
    constexpr int PER = 8; // consecutive elements per thread and iteration: one LDS scan (16 barriers) per 2048 elements instead of per 256
    for (i64 base = start; base < stop; base += 256 * PER) {
        const i64 i0 = base + (i64)threadIdx.x * PER;
        E w[PER];
        E v = ident; // running fold of this thread's elements
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const E e = i0 + j < stop ? (E)x[i0 + j] : ident;
            v = IS_MUL ? F::mul(fd, v, e) : F::add(fd, v, e);
            w[j] = v; // inclusive scan inside the thread
        }
        sh[threadIdx.x] = (u64)v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            E o = ident;
            if ((int)threadIdx.x >= off) o = (E)sh[threadIdx.x - off];
            __syncthreads();
            if ((int)threadIdx.x >= off) {
                v = IS_MUL ? F::mul(fd, o, v) : F::add(fd, o, v);
                sh[threadIdx.x] = (u64)v;
            }
            __syncthreads();
        }
        const E before = threadIdx.x ? (E)sh[threadIdx.x - 1] : ident;               // the threads before this one, in this chunk
        const E lead = IS_MUL ? F::mul(fd, carry, before) : F::add(fd, carry, before); // everything before this thread's elements
        const E total = IS_MUL ? F::mul(fd, carry, (E)sh[255]) : F::add(fd, carry, (E)sh[255]);
#pragma unroll
        for (int j = 0; j < PER; j++) {
            if (i0 + j < stop) {
                const E r = IS_MUL ? F::mul(fd, lead, w[j]) : F::add(fd, lead, w[j]);
                E o = r;
                if (mode == 1) o = F::sub(fd, a0, r);
                if (mode == 2) {
                    if (r == 0) { bad = true; o = 0; }
                    else if (a0 == 0) o = 0;
                    else {
                        if constexpr (std::is_same<F, Lut>::value) o = Lut::div_nz(fd, a0, r);
                        else o = F::mul(fd, a0, F::inv(fd, r));
                    }
                }
                y[i0 + j] = (T)o;
            }
        }
        carry = total;
        __syncthreads();
    }
    flag_error(err, bad);
}

// partial[row * nseg + seg] (the fold of segment seg) -> the fold of the segments before it.  One workgroup per row: every thread folds
// its run of ceil(nseg / 256) partials, the 256 run totals are scanned in LDS, the runs are rewritten from their prefix
template <class F, bool IS_MUL>
__global__ __launch_bounds__(256) void accumulate_carries_kernel(FieldDev fd, u64 *__restrict__ partial, i64 nseg, i64 n_outer)
{
    typedef typename F::elem E;
    __shared__ u64 sh[256];
    const i64 row = blockIdx.x;
    const E ident = IS_MUL ? F::one(fd) : (E)0;
    const i64 c = reduce_plan::carry_runs(nseg), lo = (i64)threadIdx.x * c;
    i64 hi = lo + c;
    if (hi > nseg) hi = nseg;
    u64 *pr = partial + row * nseg;
    E loc = ident;
    for (i64 sg = lo; sg < hi; sg++) { const E v = (E)pr[sg]; loc = IS_MUL ? F::mul(fd, loc, v) : F::add(fd, loc, v); }
    E v = loc;
    sh[threadIdx.x] = (u64)v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        E o = ident;
        if ((int)threadIdx.x >= off) o = (E)sh[threadIdx.x - off];
        __syncthreads();
        if ((int)threadIdx.x >= off) { v = IS_MUL ? F::mul(fd, o, v) : F::add(fd, o, v); sh[threadIdx.x] = (u64)v; }
        __syncthreads();
    }
    E run = threadIdx.x ? (E)sh[threadIdx.x - 1] : ident; // the fold of every run before this one
    for (i64 sg = lo; sg < hi; sg++) {
        const E x = (E)pr[sg];
        pr[sg] = (u64)run;
        run = IS_MUL ? F::mul(fd, run, x) : F::add(fd, run, x);
    }
    (void)n_outer;
}

template <class F, typename T>
int launch_accumulate_ft(const FieldDev &fd, const ByteTables &bt, int op, const void *a, void *out, i64 n_outer, i64 n_inner, hipStream_t st,
                         int32_t *err)
{
    const int mode = op == GFA_OP_SUB ? 1 : op == GFA_OP_DIV ? 2 : 0;
    const bool is_mul = op == GFA_OP_MUL || op == GFA_OP_DIV;
    // r06: few long rows (np.cumsum of a 1-D array): segment folds -> carries -> segment scans, instead of one workgroup for the whole row
    const i64 col_begin = mode ? 1 : 0, len = n_inner - col_begin;
    const reduce_plan::Segments sg = reduce_plan::accumulate_segments(n_outer, len, num_cus()); // gfa_reduce_plan.h
    if (sg.nseg >= 2) {
        const i64 nseg = sg.nseg, seg_len = sg.seg_len;
        return with_partials(st, (size_t)(n_outer * nseg), [&](u64 *partial) {
            reduce_phase1<F, T>(fd, bt, is_mul, a, n_inner, col_begin, seg_len, nseg, n_outer, partial, st);
            if (is_mul) {
                hipLaunchKernelGGL((accumulate_carries_kernel<F, true>), dim3((unsigned)n_outer), dim3(256), 0, st, fd, partial, nseg, n_outer);
                hipLaunchKernelGGL((accumulate_kernel<F, T, true>), dim3((unsigned)(n_outer * nseg)), dim3(256), 0, st, fd, (const T *)a, (T *)out, n_inner, mode, err,
                                   nseg, seg_len, (const u64 *)partial);
            } else {
                hipLaunchKernelGGL((accumulate_carries_kernel<F, false>), dim3((unsigned)n_outer), dim3(256), 0, st, fd, partial, nseg, n_outer);
                hipLaunchKernelGGL((accumulate_kernel<F, T, false>), dim3((unsigned)(n_outer * nseg)), dim3(256), 0, st, fd, (const T *)a, (T *)out, n_inner, mode, err,
                                   nseg, seg_len, (const u64 *)partial);
            }
        });
    }
    if (is_mul)
        hipLaunchKernelGGL((accumulate_kernel<F, T, true>), dim3((unsigned)n_outer), dim3(256), 0, st, fd, (const T *)a, (T *)out,
                           n_inner, mode, err, (i64)1, (i64)0, (const u64 *)nullptr);
    else
        hipLaunchKernelGGL((accumulate_kernel<F, T, false>), dim3((unsigned)n_outer), dim3(256), 0, st, fd, (const T *)a, (T *)out,
                           n_inner, mode, err, (i64)1, (i64)0, (const u64 *)nullptr);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

int dispatch_accumulate(const FieldDev &fd, const ByteTables &bt, int dtype, int op, const void *a, void *out, i64 n_outer, i64 n_inner,
                        hipStream_t st, int32_t *err)
{
    GFA_DISPATCH_FT(launch_accumulate_ft, fd, dtype, fd, bt, op, a, out, n_outer, n_inner, st, err);
}

} // namespace

extern "C" {

int gfa_reduce(gfa_field_t *f, int op, const void *a, void *out, int64_t n_outer, int64_t n_inner, int dtype,
               gfa_stream_t stream, int32_t *dev_err)
{
    if (!f || n_outer < 0 || n_inner < 1 || op < GFA_OP_ADD || op > GFA_OP_DIV) {
        set_error("gfa_reduce: bad arguments");
        return GFA_ERR_INVALID;
    }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (n_outer == 0) return GFA_OK; // (no rows: nothing is read or written, the buffers may be null)
    if (!a || !out) { set_error("gfa_reduce: bad arguments"); return GFA_ERR_INVALID; }
    if (!reduce_plan::rows_fit_grid(n_outer)) { set_error("gfa_reduce: more than 2^31 - 1 rows"); return GFA_ERR_INVALID; } // the launch grids
    FieldDeviceState *ds;
    int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    ByteTables bt;
    bt.log8 = ds->log8; bt.exp8 = ds->exp8; bt.add8 = ds->add8;
    if (f->use_lookup()) return dispatch_reduce(f->lut_desc(*ds), bt, dtype, op, a, out, n_outer, n_inner, (hipStream_t)stream, dev_err);
    return dispatch_reduce(f->calc, bt, dtype, op, a, out, n_outer, n_inner, (hipStream_t)stream, dev_err);
}

int gfa_reduceat(gfa_field_t *f, int op, const void *a, const int64_t *starts, const int64_t *ends, int64_t nseg, void *out, int dtype,
                 gfa_stream_t stream, int32_t *dev_err)
{
    if (!f || nseg < 0 || op < GFA_OP_ADD || op > GFA_OP_DIV) { set_error("gfa_reduceat: bad arguments"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (nseg == 0) return GFA_OK;
    if (!a || !starts || !ends || !out || nseg > 0x7fffffff) { set_error("gfa_reduceat: bad arguments"); return GFA_ERR_INVALID; }
    FieldDeviceState *ds;
    int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    if (f->use_lookup())
        return dispatch_reduceat(f->lut_desc(*ds), dtype, op, a, (const i64 *)starts, (const i64 *)ends, nseg, out, (hipStream_t)stream, dev_err);
    return dispatch_reduceat(f->calc, dtype, op, a, (const i64 *)starts, (const i64 *)ends, nseg, out, (hipStream_t)stream, dev_err);
}

int gfa_accumulate(gfa_field_t *f, int op, const void *a, void *out, int64_t n_outer, int64_t n_inner, int dtype,
                   gfa_stream_t stream, int32_t *dev_err)
{
    if (!f || n_outer < 0 || n_inner < 0 || op < GFA_OP_ADD || op > GFA_OP_DIV) {
        set_error("gfa_accumulate: bad arguments");
        return GFA_ERR_INVALID;
    }
    if (n_outer == 0 || n_inner == 0) return GFA_OK;
    if (!a || !out) { set_error("gfa_accumulate: bad arguments"); return GFA_ERR_INVALID; }
    if (!reduce_plan::rows_fit_grid(n_outer)) { set_error("gfa_accumulate: more than 2^31 - 1 rows"); return GFA_ERR_INVALID; } // the launch grids
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    FieldDeviceState *ds;
    int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    ByteTables bt;
    bt.log8 = ds->log8; bt.exp8 = ds->exp8; bt.add8 = ds->add8;
    if (f->use_lookup()) return dispatch_accumulate(f->lut_desc(*ds), bt, dtype, op, a, out, n_outer, n_inner, (hipStream_t)stream, dev_err);
    return dispatch_accumulate(f->calc, bt, dtype, op, a, out, n_outer, n_inner, (hipStream_t)stream, dev_err);
}

} // extern "C"
