// gfa_integers.hip -- integer number theory on whole arrays, one integer (or one pair) per lane; no gfa_field_t.
//
//   gfa_int_is_prime ........ replaces a loop over is_prime (_prime.py:1401-1458): deterministic Miller-Rabin below 2^64.
//   gfa_int_sieve / _expand . replaces primes (_prime.py:31-97) for a window: a segmented sieve of the odd numbers, one segment
//                             per workgroup as a bit array in LDS, then the survivors written out in increasing order.
//   gfa_int_jacobi .......... replaces a loop over jacobi_symbol (_prime.py:679-748).
//   gfa_int_unit_classify ... replaces the loops over range(n) of totatives (_modular.py:16-82) and primitive_roots
//                             (_primitive_root.py:319-464).
//
// The per-lane arithmetic is gfa_integers.h.  Nothing here allocates or synchronises: outputs belong to the caller, the
// exponents of the classifier travel as kernel arguments.
#include "gfa_internal.h"
#include "gfa_integers.h"

using namespace gfa;
using namespace gfa::integers;

namespace {

constexpr int INT_THREADS = 256;
constexpr u64 SIEVE_MAX_STOP = 1ull << 40;

struct Exps {
    u64 v[MAX_EXPS];
};

__global__ __launch_bounds__(INT_THREADS) void int_is_prime_kernel(const u64 *__restrict__ values, i64 count, u64 start, u64 step,
                                                                   uint8_t *__restrict__ flags)
{
    const i64 i = (i64)blockIdx.x * INT_THREADS + threadIdx.x;
    if (i >= count) return;
    const u64 n = values ? values[i] : start + (u64)i * step;
    flags[i] = is_prime64(n) ? 1 : 0;
}

__global__ __launch_bounds__(INT_THREADS) void int_jacobi_kernel(const i64 *__restrict__ a, const u64 *__restrict__ n, u64 shared_n,
                                                                 i64 count, int8_t *__restrict__ out)
{
    const i64 i = (i64)blockIdx.x * INT_THREADS + threadIdx.x;
    if (i >= count) return;
    const u64 m = n ? n[i] : shared_n;
    // the per-element moduli are validated before upload; a bad one must still not hang the loop
    out[i] = (m >= 3 && (m & 1)) ? (int8_t)jacobi(a[i], m) : (int8_t)0;
}

__global__ __launch_bounds__(INT_THREADS) void int_classify_kernel(u64 n, const u64 *__restrict__ values, i64 count, u64 start, u64 step,
                                                                   Exps exps, int n_exps, uint8_t *__restrict__ flags)
{
    const i64 i = (i64)blockIdx.x * INT_THREADS + threadIdx.x;
    if (i >= count) return;
    const u64 g = values ? values[i] : start + (u64)i * step;
    const u64 modulus = power_modulus(n);
    Mont mont;
    if (n_exps > 0 && modulus >= 3) mont = mont_setup(modulus);
    else mont = Mont();
    flags[i] = unit_flags(g, n, mont, modulus, exps.v, n_exps);
}

// Segment s of the window: bit j of its words is the odd integer first_odd + 2 (s SEG_BITS + j).
__global__ __launch_bounds__(INT_THREADS) void int_sieve_kernel(u64 first_odd, u64 total_bits, const u32 *__restrict__ primes, int n_primes,
                                                                u32 *__restrict__ bitmap, i64 *__restrict__ counts)
{
    __shared__ u32 words[SEG_WORDS];
    __shared__ u32 wave_sums[INT_THREADS / 64];
    const u64 bit0 = (u64)blockIdx.x * SEG_BITS;
    const u64 left = total_bits - bit0; // the grid has no empty segment
    const u32 n_bits = left < (u64)SEG_BITS ? (u32)left : (u32)SEG_BITS;
    const u32 n_words = (n_bits + 31) / 32;
    const u64 first = first_odd + 2 * bit0;

    for (int w = threadIdx.x; w < SEG_WORDS; w += INT_THREADS) words[w] = 0;
    __syncthreads();
    mark_segment(first, n_bits, primes, n_primes, (int)threadIdx.x, INT_THREADS, [&](u32 w, u32 mask) { atomicOr(&words[w], mask); });
    __syncthreads();

    u32 mine = 0;
    u32 *dst = bitmap + (size_t)blockIdx.x * SEG_WORDS;
    for (u32 w = threadIdx.x; w < n_words; w += INT_THREADS) {
        const u32 v = survivors_word(words[w], w, first, n_bits);
        dst[w] = v;
        mine += __popc(v);
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 total = 0;
        for (int k = 0; k < INT_THREADS / 64; k++) total += wave_sums[k];
        counts[blockIdx.x] = (i64)total;
    }
}

// One workgroup per segment: lane t owns words t K .. t K + K - 1 (K = SEG_WORDS / INT_THREADS), so the lanes' runs are in
// increasing order and an exclusive scan of their counts places them.
__global__ __launch_bounds__(INT_THREADS) void int_sieve_expand_kernel(u64 first_odd, u64 total_bits, const u32 *__restrict__ bitmap,
                                                                       const i64 *__restrict__ offsets, i64 *__restrict__ primes_out)
{
    constexpr int K = SEG_WORDS / INT_THREADS;
    __shared__ u32 scan[INT_THREADS];
    const u64 bit0 = (u64)blockIdx.x * SEG_BITS;
    const u64 left = total_bits - bit0;
    const u32 n_bits = left < (u64)SEG_BITS ? (u32)left : (u32)SEG_BITS;
    const u32 n_words = (n_bits + 31) / 32;
    const u32 *src = bitmap + (size_t)blockIdx.x * SEG_WORDS;
    const u32 w0 = threadIdx.x * K;

    u32 mine = 0;
    for (u32 w = w0; w < w0 + K && w < n_words; w++) mine += __popc(src[w]);
    scan[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < INT_THREADS; off <<= 1) { // inclusive scan, Hillis-Steele
        const u32 add = threadIdx.x >= (unsigned)off ? scan[threadIdx.x - off] : 0;
        __syncthreads();
        scan[threadIdx.x] += add;
        __syncthreads();
    }
    i64 at = offsets[blockIdx.x] + (i64)(scan[threadIdx.x] - mine);
    const u64 first = first_odd + 2 * bit0;
    for (u32 w = w0; w < w0 + K && w < n_words; w++) {
        u32 v = src[w];
        while (v) {
            const int b = __ffs((int)v) - 1;
            v &= v - 1;
            primes_out[at++] = (i64)(first + 2ull * (w * 32 + b));
        }
    }
}

__global__ void int_store_two_kernel(i64 *primes_out) { primes_out[0] = 2; }

unsigned blocks_for(i64 count) { return (unsigned)((count + INT_THREADS - 1) / INT_THREADS); }

// does start + (count - 1) step stay below 2^64?
bool range_fits(u64 start, u64 step, i64 count)
{
    if (count <= 1) return true;
    const unsigned __int128 last = (unsigned __int128)start + (unsigned __int128)step * (u64)(count - 1);
    return (last >> 64) == 0;
}

// the window [start, stop) as bits of odd numbers: the first odd integer >= start and how many odd integers are below stop
void odd_window(u64 start, u64 stop, u64 *first_odd, u64 *total_bits)
{
    *first_odd = start | 1;
    *total_bits = stop > *first_odd ? (stop - *first_odd + 1) / 2 : 0;
}

int check_sieve_window(const char *who, u64 start, u64 stop)
{
    if (start > stop || stop > SIEVE_MAX_STOP) {
        set_error(std::string(who) + ": the window must satisfy start <= stop <= 2^40");
        return GFA_ERR_INVALID;
    }
    return GFA_OK;
}

} // namespace

extern "C" {

int gfa_int_is_prime(const uint64_t *values, int64_t count, uint64_t start, uint64_t step, uint8_t *flags_out, gfa_stream_t stream)
{
    if (count < 0 || count > 0x7fffffffll * INT_THREADS) { set_error("gfa_int_is_prime: bad count"); return GFA_ERR_INVALID; }
    if (!values && !range_fits(start, step, count)) {
        set_error("gfa_int_is_prime: the range passes 2^64 - 1");
        return GFA_ERR_INVALID;
    }
    if (count == 0) return GFA_OK;
    if (!flags_out) { set_error("gfa_int_is_prime: flags_out is NULL"); return GFA_ERR_INVALID; }
    hipLaunchKernelGGL(int_is_prime_kernel, dim3(blocks_for(count)), dim3(INT_THREADS), 0, (hipStream_t)stream, values, (i64)count, start, step,
                       flags_out);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

int64_t gfa_int_sieve_segment_span(void) { return (int64_t)SEG_SPAN; }

int gfa_int_sieve(uint64_t start, uint64_t stop, const uint32_t *base_primes, int64_t n_base, uint32_t *bitmap_out,
                  int64_t *segment_counts_out, gfa_stream_t stream)
{
    int rc = check_sieve_window("gfa_int_sieve", start, stop);
    if (rc) return rc;
    if (n_base < 0 || n_base > 0x7fffffffll) { set_error("gfa_int_sieve: bad n_base"); return GFA_ERR_INVALID; }
    u64 first_odd, total_bits;
    odd_window(start, stop, &first_odd, &total_bits);
    if (total_bits == 0) return GFA_OK;
    if (!bitmap_out || !segment_counts_out || (n_base > 0 && !base_primes)) { set_error("gfa_int_sieve: NULL pointer"); return GFA_ERR_INVALID; }
    const unsigned segments = (unsigned)((total_bits + SEG_BITS - 1) / SEG_BITS); // at most 2^21
    hipLaunchKernelGGL(int_sieve_kernel, dim3(segments), dim3(INT_THREADS), 0, (hipStream_t)stream, first_odd, total_bits, base_primes,
                       (int)n_base, bitmap_out, (i64 *)segment_counts_out);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

int gfa_int_sieve_expand(uint64_t start, uint64_t stop, const uint32_t *bitmap, const int64_t *segment_offsets, int64_t *primes_out,
                         gfa_stream_t stream)
{
    int rc = check_sieve_window("gfa_int_sieve_expand", start, stop);
    if (rc) return rc;
    u64 first_odd, total_bits;
    odd_window(start, stop, &first_odd, &total_bits);
    const bool has_two = start <= 2 && stop > 2;
    if (total_bits == 0 && !has_two) return GFA_OK;
    if (!primes_out || (total_bits > 0 && (!bitmap || !segment_offsets))) { set_error("gfa_int_sieve_expand: NULL pointer"); return GFA_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    if (has_two) {
        hipLaunchKernelGGL(int_store_two_kernel, dim3(1), dim3(1), 0, st, (i64 *)primes_out);
        GFA_HIP(hipGetLastError());
    }
    if (total_bits == 0) return GFA_OK;
    const unsigned segments = (unsigned)((total_bits + SEG_BITS - 1) / SEG_BITS);
    hipLaunchKernelGGL(int_sieve_expand_kernel, dim3(segments), dim3(INT_THREADS), 0, st, first_odd, total_bits, bitmap,
                       (const i64 *)segment_offsets, (i64 *)primes_out);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

int gfa_int_jacobi(const int64_t *a, const uint64_t *n, int64_t count, int64_t n_stride, int8_t *out, gfa_stream_t stream)
{
    if (count < 0 || count > 0x7fffffffll * INT_THREADS || (n_stride != 0 && n_stride != 1)) {
        set_error("gfa_int_jacobi: bad arguments");
        return GFA_ERR_INVALID;
    }
    if (!n) { set_error("gfa_int_jacobi: n is NULL"); return GFA_ERR_INVALID; }
    // a shared modulus is read on the HOST (n_stride == 0: n points to one value in host memory)
    u64 shared_n = 0;
    if (n_stride == 0) {
        shared_n = n[0];
        if (shared_n < 3 || (shared_n & 1) == 0) {
            set_error("gfa_int_jacobi: n must be odd and greater than 2");
            return GFA_ERR_INVALID;
        }
    }
    if (count == 0) return GFA_OK;
    if (!a || !out) { set_error("gfa_int_jacobi: NULL pointer"); return GFA_ERR_INVALID; }
    hipLaunchKernelGGL(int_jacobi_kernel, dim3(blocks_for(count)), dim3(INT_THREADS), 0, (hipStream_t)stream, (const i64 *)a,
                       n_stride ? (const u64 *)n : (const u64 *)nullptr, shared_n, (i64)count, out);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

int gfa_int_unit_classify(uint64_t n, const uint64_t *values, int64_t count, uint64_t start, uint64_t step, const uint64_t *exps,
                          int64_t n_exps, uint8_t *flags_out, gfa_stream_t stream)
{
    if (n < 1 || count < 0 || count > 0x7fffffffll * INT_THREADS || n_exps < 0 || n_exps > MAX_EXPS || (n_exps > 0 && !exps)) {
        set_error("gfa_int_unit_classify: bad arguments");
        return GFA_ERR_INVALID;
    }
    if (!values && !range_fits(start, step, count)) {
        set_error("gfa_int_unit_classify: the range passes 2^64 - 1");
        return GFA_ERR_INVALID;
    }
    if (n_exps > 0 && power_modulus(n) == 0) {
        set_error("gfa_int_unit_classify: the powers need n odd or n = 2 odd (every other n > 4 has no primitive root)");
        return GFA_ERR_UNSUPPORTED;
    }
    if (count == 0) return GFA_OK;
    if (!flags_out) { set_error("gfa_int_unit_classify: flags_out is NULL"); return GFA_ERR_INVALID; }
    Exps e{};
    for (int i = 0; i < (int)n_exps; i++) e.v[i] = exps[i]; // host memory
    hipLaunchKernelGGL(int_classify_kernel, dim3(blocks_for(count)), dim3(INT_THREADS), 0, (hipStream_t)stream, n, values, (i64)count, start,
                       step, e, (int)n_exps, flags_out);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

} // extern "C"
