// gfa_lfsr.hip -- linear-feedback shift registers over GF(q), q < 2^64: stepping a stack of registers, and jumping ahead.
//
//   gfa_lfsr_step ... replaces fibonacci_lfsr_step_forward_jit / _backward_jit and galois_lfsr_step_forward_jit / _backward_jit
//                     (_lfsr.py:718-843, 1354-1477) for `batch` registers with the same taps, one launch
//   gfa_lfsr_jump ... the states exp0 + k stride clocks ahead of one register, k < count, one launch: what lets a caller cut one
//                     long sequence into `count` chunks that gfa_lfsr_step then produces side by side
//
// ls_step_kernel   ONE LANE PER REGISTER (gfa_lfsr.h clock()), LS_ROWS = 64 registers per workgroup of one wavefront.  The
//                  states sit in LDS lane-interleaved (element j of lane l at j * rows + l: a wave's access is one bank row, no
//                  conflicts), the taps once per workgroup (every lane reads the same address: a broadcast).  A lane's outputs
//                  are consecutive in memory, so a lane storing its own would scatter 64 lines per instruction; instead LS_TILE
//                  = 64 clocks of outputs are staged in LDS (rows padded to 65) and written out one register per instruction:
//                  64 consecutive elements.  Long registers leave room for fewer rows: rows = (LDS - taps) / (n + 65), so
//                    n <= LS_STEP_MAX(sizeof element) = (150 KiB / sizeof element - 65) / 2 = 19167 / 9567.
// ls_bits_kernel   GF(2), n <= 64, forward: the state is one 64-bit word in registers (clock_bits()), 256 registers per
//                  workgroup; the 64 outputs of a tile are one word per lane, passed through LDS and written as 64 consecutive
//                  elements per register (one uint8 per bit in the storage GF(2) arrays have).
// ls_jump_kernel   one workgroup per row runs gfa_lfsr.h jump(): x^e mod P by squarings (polydiv::mulmod) and single clocks,
//                  then the product with the register's state polynomial.  P, the residue, the state polynomial and 2 n
//                  coefficients of work space sit in LDS, 5 n + 1 elements of 150 KiB less the exponent's words:
//                    n <= LS_JUMP_MAX(sizeof element) = ((150 KiB - 1 KiB) / sizeof element - 1) / 5 = 7628 / 3814.
//                  The row's exponent exp0 + k stride is formed in LDS by one thread; exp0 arrives as kernel arguments.
#include <algorithm>

#include "gfa_poly_launch.h"
#include "gfa_lfsr.h"

using namespace gfa;
using namespace gfa::lfsr;
using namespace gfa::polykit;

namespace {

constexpr int LS_ROWS = 64;       // registers per workgroup of ls_step_kernel: one wavefront
constexpr int LS_TILE = 64;       // clocks between two flushes of the staged outputs
constexpr int LS_BITS_ROWS = 256; // registers per workgroup of ls_bits_kernel
constexpr size_t LS_LDS_BYTES = 150 * 1024;
constexpr int LS_EXP_WORDS = 126; // words of exp0 at most; the row's exponent has two more
constexpr size_t LS_EXP_BYTES = (LS_EXP_WORDS + 2) * sizeof(u64);

constexpr i64 LS_STEP_MAX(size_t elem) { return (i64)((LS_LDS_BYTES / elem - (LS_TILE + 1)) / 2); }
constexpr i64 LS_JUMP_MAX(size_t elem) { return (i64)(((LS_LDS_BYTES - LS_EXP_BYTES) / elem - 1) / 5); }
static_assert(jump_elems((int)LS_JUMP_MAX(4)) * 4 + LS_EXP_BYTES <= LS_LDS_BYTES && jump_elems((int)LS_JUMP_MAX(8)) * 8 + LS_EXP_BYTES <= LS_LDS_BYTES, "cap");

template <class E>
struct Staged { // a lane's row of the output tile
    E *p;
    __device__ __forceinline__ void set(int i, E v) const { p[i] = v; }
};
struct Dropped {
    template <class E>
    __device__ __forceinline__ void set(int, E) const {}
};

struct ExpWords {
    u64 v[LS_EXP_WORDS];
};

// rows registers per workgroup (rows <= blockDim.x = LS_ROWS); LDS: taps[n], states[n][rows], tile[rows][LS_TILE + 1]
template <class F>
__global__ __launch_bounds__(LS_ROWS) void ls_step_kernel(FieldDev fd, int kind, int forward, const void *__restrict__ taps, int n, void *__restrict__ states,
                                                          i64 batch, i64 steps, int rows, void *__restrict__ y_out, int dtype)
{
    typedef typename F::elem E;
    extern __shared__ u64 ls_lds[];
    E *ts = (E *)ls_lds, *ss = ts + n, *tile = ss + (size_t)n * rows;
    const int lane = (int)threadIdx.x;
    const i64 row0 = (i64)blockIdx.x * rows, row = row0 + lane;
    const bool owner = lane < rows, live = owner && row < batch;
    for (int j = lane; j < n; j += (int)blockDim.x) ts[j] = (E)load_coeff(taps, dtype, j);
    const Strided<E> s{ss + (owner ? lane : 0), rows};
    if (owner)
        for (int j = 0; j < n; j++) s[j] = live ? (E)load_coeff(states, dtype, row * n + j) : (E)0;
    __syncthreads();
    const Lin<E> T{ts};
    const E tinv = forward ? (E)0 : backward_inverse<F>(fd, kind == KIND_FIBONACCI ? T[n - 1] : T[0]);
    int head = 0;
    const Staged<E> mine{tile + (size_t)(owner ? lane : 0) * (LS_TILE + 1)};
    for (i64 i0 = 0; i0 < steps; i0 += LS_TILE) { // the same trips for every lane: the barriers are the workgroup's
        const int count = (int)(steps - i0 < LS_TILE ? steps - i0 : LS_TILE);
        if (!y_out) {
            if (owner) clock<F>(fd, kind, forward != 0, s, T, n, head, tinv, count, Dropped());
            continue;
        }
        if (owner) clock<F>(fd, kind, forward != 0, s, T, n, head, tinv, count, mine);
        __syncthreads();
        for (int r = 0; r < rows && row0 + r < batch; r++)
            if (lane < count) store_coeff(y_out, dtype, (row0 + r) * steps + i0 + lane, tile[(size_t)r * (LS_TILE + 1) + lane]);
        __syncthreads();
    }
    if (live)
        for (int j = 0; j < n; j++) {
            int p = head + j;
            if (p >= n) p -= n;
            store_coeff(states, dtype, row * n + j, s[p]);
        }
}

__global__ __launch_bounds__(LS_BITS_ROWS) void ls_bits_kernel(int kind, const void *__restrict__ taps, int n, void *__restrict__ states, i64 batch, i64 steps,
                                                              void *__restrict__ y_out, int dtype)
{
    __shared__ u64 words[LS_BITS_ROWS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave0 = tid & ~63;
    const i64 row = (i64)blockIdx.x * LS_BITS_ROWS + tid;
    const bool live = row < batch;
    u64 t = 0, s = 0;
    for (int j = 0; j < n; j++) {
        t |= (load_coeff(taps, dtype, j) & 1) << j;
        if (live) s |= (load_coeff(states, dtype, row * n + j) & 1) << j;
    }
    for (i64 i0 = 0; i0 < steps; i0 += 64) {
        const int count = (int)(steps - i0 < 64 ? steps - i0 : 64);
        const u64 out = clock_bits(kind, s, t, n, count);
        if (!y_out) continue;
        words[tid] = out;
        __syncthreads();
        const i64 wrow0 = (i64)blockIdx.x * LS_BITS_ROWS + wave0; // a wavefront writes out its own 64 registers
        for (int r = 0; r < 64 && wrow0 + r < batch; r++)
            if (lane < count) store_coeff(y_out, dtype, (wrow0 + r) * steps + i0 + lane, (words[wave0 + r] >> lane) & 1);
        __syncthreads();
    }
    if (live)
        for (int j = 0; j < n; j++) store_coeff(states, dtype, row * n + j, (s >> j) & 1);
}

template <class F>
__global__ __launch_bounds__(MaxThreads<F>::most) void ls_jump_kernel(FieldDev fd, int kind, const void *__restrict__ P, int n, const void *__restrict__ state,
                                                                      ExpWords exp0, int limbs, u64 stride, void *__restrict__ states_out, int dtype)
{
    typedef typename F::elem E;
    extern __shared__ u64 ls_lds[];
    u64 *ew = ls_lds; // the row's exponent: limbs + 2 words
    E *cs = (E *)(ls_lds + LS_EXP_WORDS + 2), *rs = cs + n + 1, *gs = rs + n, *ws = gs + n;
    const Team g{(int)threadIdx.x, (int)blockDim.x};
    const u64 k = blockIdx.x;
    for (int t = g.tid; t <= n; t += g.n) cs[t] = (E)load_coeff(P, dtype, t);
    for (int t = g.tid; t < n; t += g.n) ws[t] = (E)load_coeff(state, dtype, t);
    if (g.tid == 0) { // exp0 + k stride
        const u64 lo = k * stride, hi = mulhi64(k, stride);
        u64 carry = 0;
        for (int l = 0; l < limbs + 2; l++) {
            const u64 a = l < limbs ? exp0.v[l] : 0, b = l == 0 ? lo : l == 1 ? hi : 0;
            const u64 s1 = a + b, s2 = s1 + carry;
            carry = (u64)(s1 < a) + (u64)(s2 < s1);
            ew[l] = s2;
        }
    }
    g.sync();
    jump<F, Lin<E>, Team>(fd, kind, Lin<E>{ws}, Lin<E>{rs}, Lin<E>{gs}, Lin<E>{cs}, n, ew, limbs + 2, g);
    for (int t = g.tid; t < n; t += g.n) store_coeff(states_out, dtype, (i64)k * n + t, gs[t]);
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct StepJob {
    int kind, forward;
    const void *taps;
    int n;
    void *states;
    i64 batch, steps;
    void *y;
    int dtype;
    hipStream_t st;
};

template <class F>
int launch_step(const FieldDev &fd, const StepJob &j)
{
    typedef typename F::elem E;
    const size_t elems = LS_LDS_BYTES / sizeof(E);
    const int rows = (int)std::min<size_t>(LS_ROWS, (elems - (size_t)j.n) / ((size_t)j.n + LS_TILE + 1));
    const size_t lds = ((size_t)j.n + (size_t)rows * ((size_t)j.n + LS_TILE + 1)) * sizeof(E);
    const int rc = allow_large_lds<ls_step_kernel<F>>(LS_LDS_BYTES);
    if (rc) return rc;
    const i64 groups = (j.batch + rows - 1) / rows;
    hipLaunchKernelGGL((ls_step_kernel<F>), dim3((unsigned)groups), dim3(LS_ROWS), lds, j.st, fd, j.kind, j.forward, j.taps, j.n, j.states, j.batch, j.steps, rows, j.y, j.dtype);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

struct JumpJob {
    int kind;
    const void *P;
    int n;
    const void *state;
    ExpWords exp0;
    int limbs;
    u64 stride;
    i64 count;
    void *out;
    int dtype;
    hipStream_t st;
};

template <class F>
int launch_jump(const FieldDev &fd, const JumpJob &j)
{
    typedef typename F::elem E;
    const int rc = allow_large_lds<ls_jump_kernel<F>>(LS_LDS_BYTES);
    if (rc) return rc;
    const int threads = wave_threads(2 * j.n - 1, MaxThreads<F>::most);
    const size_t lds = LS_EXP_BYTES + jump_elems(j.n) * sizeof(E);
    hipLaunchKernelGGL((ls_jump_kernel<F>), dim3((unsigned)j.count), dim3(threads), lds, j.st, fd, j.kind, j.P, j.n, j.state, j.exp0, j.limbs, j.stride, j.out, j.dtype);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

bool bad_kind(int kind) { return kind != KIND_FIBONACCI && kind != KIND_GALOIS; }

} // namespace

extern "C" {

int gfa_lfsr_step(gfa_field_t *f, int kind, int direction, const void *taps, int64_t n, void *states, int64_t batch, int64_t steps, void *y_out, int dtype,
                  gfa_stream_t stream)
{
    if (!f) { set_error("gfa_lfsr_step: no field handle (fields of order >= 2^64 are not served: run the four loops on whole arrays)"); return GFA_ERR_UNSUPPORTED; }
    if (bad_kind(kind) || (direction != 1 && direction != -1) || n < 1 || batch < 0 || steps < 0) {
        set_error("gfa_lfsr_step: bad arguments (kind 0 Fibonacci or 1 Galois, direction 1 or -1, n >= 1, batch >= 0, steps >= 0)");
        return GFA_ERR_INVALID;
    }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0 || steps == 0) return GFA_OK;
    if (!taps || !states) { set_error("gfa_lfsr_step: bad arguments"); return GFA_ERR_INVALID; }
    if (batch > 0x7fffffff) { set_error("gfa_lfsr_step: at most 2^31 - 1 registers"); return GFA_ERR_UNSUPPORTED; }
    FieldDev fd;
    const int rc = field_desc(f, &fd);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (f->calc.q == 2 && n <= 64 && direction == 1) {
        const i64 groups = (batch + LS_BITS_ROWS - 1) / LS_BITS_ROWS;
        hipLaunchKernelGGL(ls_bits_kernel, dim3((unsigned)groups), dim3(LS_BITS_ROWS), 0, st, kind, taps, (int)n, states, (i64)batch, (i64)steps, y_out, dtype);
        GFA_HIP(hipGetLastError());
        return GFA_OK;
    }
    const i64 cap = LS_STEP_MAX(elem_bytes(fd));
    if (n > cap) {
        set_error("gfa_lfsr_step: order " + std::to_string(n) + ", the kernel holds a register, its taps and a tile of outputs in LDS up to order " +
                  std::to_string(cap) + " over this field");
        return GFA_ERR_UNSUPPORTED;
    }
    const StepJob j{kind, direction == 1 ? 1 : 0, taps, (int)n, states, batch, steps, y_out, dtype, st};
    return for_policy(fd, dtype, "gfa_lfsr", [&](auto p) { return launch_step<typename decltype(p)::type>(fd, j); });
}

int64_t gfa_lfsr_max_order(gfa_field_t *f)
{
    if (!f) return 0;
    FieldDev fd;
    if (field_desc(f, &fd)) return 0;
    return LS_JUMP_MAX(elem_bytes(fd));
}

int gfa_lfsr_jump(gfa_field_t *f, int kind, const void *P, int64_t n, const void *state, const uint64_t *exp0_limbs, int64_t n_limbs, uint64_t stride,
                  int64_t count, void *states_out, int dtype, gfa_stream_t stream)
{
    if (!f) { set_error("gfa_lfsr_jump: no field handle (fields of order >= 2^64 are not served)"); return GFA_ERR_UNSUPPORTED; }
    if (bad_kind(kind) || n < 1 || count < 0 || n_limbs < 1 || !exp0_limbs) {
        set_error("gfa_lfsr_jump: bad arguments (kind 0 Fibonacci or 1 Galois, n >= 1, count >= 0, an exponent of n_limbs >= 1 words)");
        return GFA_ERR_INVALID;
    }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (count == 0) return GFA_OK;
    if (!P || !state || !states_out) { set_error("gfa_lfsr_jump: bad arguments"); return GFA_ERR_INVALID; }
    while (n_limbs > 1 && exp0_limbs[n_limbs - 1] == 0) n_limbs--;
    if (n_limbs > LS_EXP_WORDS || count > 0x7fffffff) {
        set_error("gfa_lfsr_jump: at most 2^31 - 1 rows, and exponents of at most " + std::to_string(LS_EXP_WORDS) + " words");
        return GFA_ERR_UNSUPPORTED;
    }
    FieldDev fd;
    const int rc = field_desc(f, &fd);
    if (rc) return rc;
    const i64 cap = LS_JUMP_MAX(elem_bytes(fd));
    if (n > cap) {
        set_error("gfa_lfsr_jump: order " + std::to_string(n) + ", the kernel holds the characteristic polynomial, two residues and a product in LDS up to order " +
                  std::to_string(cap) + " over this field (gfa_lfsr_max_order)");
        return GFA_ERR_UNSUPPORTED;
    }
    JumpJob j{kind, P, (int)n, state, {}, (int)n_limbs, stride, count, states_out, dtype, (hipStream_t)stream};
    for (int l = 0; l < (int)n_limbs; l++) j.exp0.v[l] = exp0_limbs[l];
    return for_policy(fd, dtype, "gfa_lfsr", [&](auto p) { return launch_jump<typename decltype(p)::type>(fd, j); });
}

} // extern "C"
