// gfa_polydiv.hip -- polynomial division with remainder and modular powers over GF(q), q < 2^64, one workgroup per row.
//
//   gfa_poly_divmod ... replaces divmod_jit / floordiv_jit / mod_jit (_polys/_dense.py:126-320) for a batch of dividends and one divisor
//   gfa_poly_powmod ... replaces pow_jit with a modulus (_polys/_dense.py:323-401) for a batch of bases, one exponent, one modulus
//
// Both run the blocked synthetic division of gfa_polydiv.h (block PD_K = 64 quotient coefficients: a triangular solve by one
// wave, then every other window coefficient updated independently by all threads).
//
// Division.  The divisor and a circular window of nb - 1 + 2 K coefficients sit in LDS when (2 nb - 1 + 2 K) elements fit
// PD_DIV_LDS_BYTES = 64 KiB (nb <= 8128 on 32-bit elements, 4032 on 64-bit ones); longer divisors run the same code on a
// stream-ordered work copy of the rows in global memory (__syncthreads() orders a workgroup's global writes between the
// phases).  There is no degree cap.  A single long division is quadratic work on one compute unit.
//
// Power.  The whole square-and-multiply chain is one launch: the residue, the base, the 2 d - 1 product coefficients and the
// modulus live in LDS (5 d + 2 K + 1 elements at most, of the 150 KiB berlekamp_massey_kernel also asks for), so
//   d = nc - 1 <= PD_POWMOD_MAX(sizeof element) = (150 KiB / sizeof element - 2 K - 1) / 5 = 7654 (32-bit) / 3814 (64-bit elements);
// above it the entry point returns GFA_ERR_UNSUPPORTED and the caller loops over gfa_convolve and gfa_poly_divmod.
//
// The element type is the field policy's (32 bits for Prime32 and Lut, 64 bits otherwise) whatever the storage type, which
// is read and written through a switch that is uniform over the launch -- so the kernels are instantiated per policy only.
#include <algorithm>

#include "gfa_internal.h"
#include "gfa_polydiv.h"

using namespace gfa;
using namespace gfa::polydiv;
using gfa::polytest::ExtP;

namespace {

// threads of a workgroup at most (a launch takes as many whole waves as it has independent coefficients, up to this): 1024,
// but 512 for the digit-vector products of GF(p^M), M >= 11, which need more than the 128 registers a 1024-thread workgroup
// leaves each lane (they would spill to scratch memory)
constexpr int PD_THREADS = 1024;
template <class F>
struct MaxThreads {
    static constexpr int most = PD_THREADS;
};
template <int M>
struct MaxThreads<ExtP<M>> {
    static constexpr int most = M >= 11 ? PD_THREADS / 2 : PD_THREADS;
};
constexpr size_t PD_DIV_LDS_BYTES = 64 * 1024;
constexpr size_t PD_POW_LDS_BYTES = 150 * 1024;
constexpr int PD_ARG_WORDS = 256;

constexpr int PD_POWMOD_MAX(size_t elem) { return (int)((PD_POW_LDS_BYTES / elem - 2 * PD_K - 1) / 5); }

// LDS elements of a division (divisor + window) and of a power (modulus, residue, base, product / first window)
constexpr size_t div_lds_elems(int nb) { return (size_t)nb + (size_t)(nb - 1 + 2 * PD_K); }
constexpr size_t pow_lds_elems(int d) { return (size_t)(d + 1) + 2 * (size_t)d + (size_t)std::max(2 * d - 1, d + 2 * PD_K); }
static_assert(pow_lds_elems(PD_POWMOD_MAX(4)) * 4 <= PD_POW_LDS_BYTES && pow_lds_elems(PD_POWMOD_MAX(8)) * 8 <= PD_POW_LDS_BYTES, "cap");

__device__ __forceinline__ u64 load_coeff(const void *p, int dtype, i64 i)
{
    switch (dtype) { // uniform over the launch
    case GFA_U8: return ((const uint8_t *)p)[i];
    case GFA_U16: return ((const uint16_t *)p)[i];
    case GFA_U32: return ((const uint32_t *)p)[i];
    default: return ((const uint64_t *)p)[i];
    }
}

__device__ __forceinline__ void store_coeff(void *p, int dtype, i64 i, u64 v)
{
    switch (dtype) {
    case GFA_U8: ((uint8_t *)p)[i] = (uint8_t)v; break;
    case GFA_U16: ((uint16_t *)p)[i] = (uint16_t)v; break;
    case GFA_U32: ((uint32_t *)p)[i] = (uint32_t)v; break;
    default: ((uint64_t *)p)[i] = v; break;
    }
}

struct Source { // coefficients base + i of a storage array
    const void *p;
    int dtype;
    i64 base;
    __device__ __forceinline__ u64 operator[](int i) const { return load_coeff(p, dtype, base + i); }
};

struct Sink {
    void *p;
    int dtype;
    i64 base;
    __device__ __forceinline__ void set(int i, u64 v) const { store_coeff(p, dtype, base + i, v); }
};

// the workgroup; triangle() runs on its first wave, whose lanes order their LDS and global accesses among themselves
struct Team {
    int tid, n;
    static constexpr int wave = 64;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ void wave_sync() const
    {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
};

struct ArgWords {
    u64 v[PD_ARG_WORDS];
};

// the exponent reaches the device as kernel arguments: ordered on the stream, no synchronous copy
__global__ void pd_store_kernel(ArgWords a, u64 *dst, int n)
{
    const int i = threadIdx.x;
    if (i < n) dst[i] = a.v[i];
}

// divisor and window in LDS
template <class F>
__global__ __launch_bounds__(MaxThreads<F>::most) void pd_divmod_lds_kernel(FieldDev fd, const void *__restrict__ a, int na, const void *__restrict__ b, int nb,
                                                                      void *__restrict__ q_out, void *__restrict__ r_out, int dtype)
{
    typedef typename F::elem E;
    extern __shared__ u64 pd_lds[];
    E *bs = (E *)pd_lds, *win = bs + nb;
    const Team g{(int)threadIdx.x, (int)blockDim.x};
    const i64 row = blockIdx.x;
    const int nq = na - nb + 1;
    for (int t = g.tid; t < nb; t += g.n) bs[t] = (E)load_coeff(b, dtype, t);
    const Ring<E> W{win, nb - 1 + 2 * PD_K, 0};
    const Ring<E> R = divide<F, Ring<E>, Lin<E>, Source, Sink, Team>(fd, W, Lin<E>{bs}, Source{a, dtype, row * na}, na, nb, Sink{q_out, dtype, row * nq},
                                                                   q_out != nullptr, true, g);
    if (r_out)
        for (int t = g.tid; t < nb - 1; t += g.n) store_coeff(r_out, dtype, row * (nb - 1) + t, R[t]);
}

// divisor (bw, widened to elements) and the rows' work copies (ws, na elements each) in global memory
template <class F>
__global__ __launch_bounds__(MaxThreads<F>::most) void pd_divmod_global_kernel(FieldDev fd, const void *__restrict__ a, int na,
                                                                         const typename F::elem *__restrict__ bw, int nb, typename F::elem *__restrict__ ws,
                                                                         void *__restrict__ q_out, void *__restrict__ r_out, int dtype)
{
    typedef typename F::elem E;
    const Team g{(int)threadIdx.x, (int)blockDim.x};
    const i64 row = blockIdx.x;
    const int nq = na - nb + 1;
    const Lin<E> W{ws + row * na};
    const Lin<E> R = divide<F, Lin<E>, Lin<const E>, Source, Sink, Team>(fd, W, Lin<const E>{bw}, Source{a, dtype, row * na}, na, nb,
                                                                       Sink{q_out, dtype, row * nq}, q_out != nullptr, true, g);
    if (r_out)
        for (int t = g.tid; t < nb - 1; t += g.n) store_coeff(r_out, dtype, row * (nb - 1) + t, R[t]);
}

template <class E>
__global__ void pd_widen_kernel(const void *__restrict__ src, int dtype, E *__restrict__ dst, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = (E)load_coeff(src, dtype, i);
}

template <class F>
__global__ __launch_bounds__(MaxThreads<F>::most) void pd_powmod_kernel(FieldDev fd, const void *__restrict__ a, int na, const u64 *__restrict__ e, int limbs,
                                                                  const void *__restrict__ c, int nc, void *__restrict__ out, int dtype)
{
    typedef typename F::elem E;
    extern __shared__ u64 pd_lds[];
    const int d = nc - 1;
    E *cs = (E *)pd_lds, *rs = cs + nc, *as = rs + d, *ps = as + d;
    const Team g{(int)threadIdx.x, (int)blockDim.x};
    const i64 row = blockIdx.x;
    for (int t = g.tid; t < nc; t += g.n) cs[t] = (E)load_coeff(c, dtype, t);
    const Lin<E> C{cs}, r{rs}, base{as}, P{ps};
    // the row modulo c
    if (na < nc) {
        for (int j = g.tid; j < d; j += g.n) base[j] = j < d - na ? (E)0 : (E)load_coeff(a, dtype, row * na + j - (d - na));
    } else {
        const Ring<E> W{ps, d + 2 * PD_K, 0};
        const Ring<E> R = divide<F, Ring<E>, Lin<E>, Source, NoQuotient, Team>(fd, W, C, Source{a, dtype, row * na}, na, nc, NoQuotient(), false, true, g);
        for (int j = g.tid; j < d; j += g.n) base[j] = R[j];
    }
    g.sync();
    power<F, Lin<E>, Team>(fd, r, base, P, C, d, e, limbs, g);
    for (int j = g.tid; j < d; j += g.n) store_coeff(out, dtype, row * d + j, r[j]);
}

// ---- host ------------------------------------------------------------------------------------------------------------
int round_up_threads(int work, int most)
{
    const int t = (std::max(work, 1) + 63) / 64 * 64;
    return std::min(t, most);
}

struct DivJob {
    const void *a, *b;
    i64 batch;
    int na, nb, dtype;
    void *q, *r;
    hipStream_t st;
};

template <class F>
int launch_div(const FieldDev &fd, const DivJob &j)
{
    typedef typename F::elem E;
    const int threads = round_up_threads(j.nb - 1, MaxThreads<F>::most);
    const size_t lds = div_lds_elems(j.nb) * sizeof(E);
    if (lds <= PD_DIV_LDS_BYTES) {
        hipLaunchKernelGGL((pd_divmod_lds_kernel<F>), dim3((unsigned)j.batch), dim3(threads), lds, j.st, fd, j.a, j.na, j.b, j.nb, j.q, j.r, j.dtype);
        GFA_HIP(hipGetLastError());
        return GFA_OK;
    }
    Scratch ws(j.st);
    E *bw = nullptr;
    GFA_HIP(ws.get(&bw, (size_t)j.batch * (size_t)j.na + (size_t)j.nb));
    E *rows = bw + j.nb;
    hipLaunchKernelGGL((pd_widen_kernel<E>), dim3((unsigned)std::min(256, (j.nb + 255) / 256)), dim3(256), 0, j.st, j.b, j.dtype, bw, j.nb);
    GFA_HIP(hipGetLastError());
    hipLaunchKernelGGL((pd_divmod_global_kernel<F>), dim3((unsigned)j.batch), dim3(threads), 0, j.st, fd, j.a, j.na, (const E *)bw, j.nb, rows, j.q, j.r, j.dtype);
    GFA_HIP(hipGetLastError());
    return GFA_OK; // the buffer goes back to the pool in stream order
}

struct PowJob {
    const void *a, *c;
    i64 batch;
    int na, nc, dtype;
    const u64 *e; // device
    int limbs;
    void *out;
    hipStream_t st;
};

template <class F>
int launch_pow(const FieldDev &fd, const PowJob &j)
{
    typedef typename F::elem E;
    const int d = j.nc - 1;
    if (d > PD_POWMOD_MAX(sizeof(E))) {
        set_error("gfa_poly_powmod: the modulus has degree " + std::to_string(d) + ", the kernel holds its operands in LDS up to degree " +
                  std::to_string(PD_POWMOD_MAX(sizeof(E))) + " over this field");
        return GFA_ERR_UNSUPPORTED;
    }
    auto k = pd_powmod_kernel<F>;
    static bool attr = false;
    if (!attr) { GFA_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PD_POW_LDS_BYTES)); attr = true; }
    const int threads = round_up_threads(2 * d - 1, MaxThreads<F>::most);
    hipLaunchKernelGGL(k, dim3((unsigned)j.batch), dim3(threads), pow_lds_elems(d) * sizeof(E), j.st, fd, j.a, j.na, j.e, j.limbs, j.c, j.nc, j.out, j.dtype);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

template <int M, class J>
int launch_ext(const FieldDev &fd, const J &j)
{
    if constexpr (M > GFA_MAX_EXT_DEGREE) {
        set_error("gfa_polydiv: unsupported extension degree");
        return GFA_ERR_UNSUPPORTED;
    } else {
        if ((int)fd.m == M) {
            if constexpr (std::is_same<J, DivJob>::value) return launch_div<ExtP<M>>(fd, j);
            else return launch_pow<ExtP<M>>(fd, j);
        }
        return launch_ext<M + 1, J>(fd, j);
    }
}

// the storage type is read through load_coeff, so the kernels are instantiated per field policy only
template <class F, typename T>
int launch_div_ft(const FieldDev &fd, const DivJob &j)
{
    if constexpr (std::is_same<F, Ext>::value) return launch_ext<2, DivJob>(fd, j);
    else return launch_div<F>(fd, j);
}

template <class F, typename T>
int launch_pow_ft(const FieldDev &fd, const PowJob &j)
{
    if constexpr (std::is_same<F, Ext>::value) return launch_ext<2, PowJob>(fd, j);
    else return launch_pow<F>(fd, j);
}

int dispatch_div(const FieldDev &fd, int dtype, const DivJob &j) { GFA_DISPATCH_FT(launch_div_ft, fd, dtype, fd, j); }
int dispatch_pow(const FieldDev &fd, int dtype, const PowJob &j) { GFA_DISPATCH_FT(launch_pow_ft, fd, dtype, fd, j); }

int upload(const uint64_t *h, size_t n, u64 *d, hipStream_t st)
{
    for (size_t off = 0; off < n; off += PD_ARG_WORDS) {
        ArgWords a;
        const int m = (int)std::min<size_t>(PD_ARG_WORDS, n - off);
        for (int i = 0; i < m; i++) a.v[i] = h[off + i];
        hipLaunchKernelGGL(pd_store_kernel, dim3(1), dim3(PD_ARG_WORDS), 0, st, a, d + off, m);
    }
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

} // namespace

extern "C" {

int gfa_poly_divmod(gfa_field_t *f, const void *a, int64_t batch, int64_t na, const void *b, int64_t nb, void *q_out, void *r_out, int dtype,
                    gfa_stream_t stream)
{
    if (!f || batch < 0 || nb < 1 || nb > na) { set_error("gfa_poly_divmod: bad arguments"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0) return GFA_OK;
    if (!a || !b) { set_error("gfa_poly_divmod: bad arguments"); return GFA_ERR_INVALID; }
    if (batch > 0x7fffffff || na > 0x7fffffff) { set_error("gfa_poly_divmod: at most 2^31 - 1 rows of at most 2^31 - 1 coefficients"); return GFA_ERR_UNSUPPORTED; }
    if (nb == 1) r_out = nullptr; // no remainder coefficients
    if (!q_out && !r_out) return GFA_OK;
    FieldDeviceState *ds;
    int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    const FieldDev fd = f->use_lookup() ? f->lut_desc(*ds) : f->calc;
    const DivJob j{a, b, batch, (int)na, (int)nb, dtype, q_out, r_out, (hipStream_t)stream};
    return dispatch_div(fd, dtype, j);
}

int gfa_poly_powmod(gfa_field_t *f, const void *a, int64_t batch, int64_t na, const uint64_t *exp_limbs, int64_t n_limbs, const void *c, int64_t nc,
                    void *out, int dtype, gfa_stream_t stream)
{
    if (!f || batch < 0 || na < 1 || nc < 2 || n_limbs < 1 || n_limbs > (1 << 20) || !exp_limbs) { set_error("gfa_poly_powmod: bad arguments"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0) return GFA_OK;
    if (!a || !c || !out) { set_error("gfa_poly_powmod: bad arguments"); return GFA_ERR_INVALID; }
    if (batch > 0x7fffffff || na > 0x7fffffff || nc > 0x7fffffff) { set_error("gfa_poly_powmod: at most 2^31 - 1 rows of at most 2^31 - 1 coefficients"); return GFA_ERR_UNSUPPORTED; }
    FieldDeviceState *ds;
    int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    const FieldDev fd = f->use_lookup() ? f->lut_desc(*ds) : f->calc;
    hipStream_t st = (hipStream_t)stream;
    Scratch ws(st);
    u64 *exps = nullptr;
    GFA_HIP(ws.get(&exps, (size_t)n_limbs));
    rc = upload(exp_limbs, (size_t)n_limbs, exps, st);
    if (rc) return rc;
    const PowJob j{a, c, batch, (int)na, (int)nc, dtype, exps, (int)n_limbs, out, st};
    return dispatch_pow(fd, dtype, j);
}

} // extern "C"
