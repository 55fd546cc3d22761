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
// The element type is the field policy's (32 bits for Prime32 and Lut, 64 bits otherwise) whatever the storage type, which is
// read and written through load_coeff / store_coeff.  Those, the workgroup (Team), the thread limits, the policy dispatch and
// the word upload are the family's: gfa_poly_launch.h.
#include <algorithm>

#include "gfa_poly_launch.h"
#include "gfa_polydiv.h"

using namespace gfa;
using namespace gfa::polydiv;
using namespace gfa::polykit;

namespace {

constexpr size_t PD_DIV_LDS_BYTES = 64 * 1024;
constexpr size_t PD_POW_LDS_BYTES = 150 * 1024;

constexpr int PD_POWMOD_MAX(size_t elem) { return (int)((PD_POW_LDS_BYTES / elem - 2 * PD_K - 1) / 5); }

// LDS elements of a division (divisor + window) and of a power (modulus, residue, base, product / first window)
constexpr size_t div_lds_elems(int nb) { return (size_t)nb + (size_t)(nb - 1 + 2 * PD_K); }
constexpr size_t pow_lds_elems(int d) { return (size_t)(d + 1) + 2 * (size_t)d + (size_t)std::max(2 * d - 1, d + 2 * PD_K); }
static_assert(pow_lds_elems(PD_POWMOD_MAX(4)) * 4 <= PD_POW_LDS_BYTES && pow_lds_elems(PD_POWMOD_MAX(8)) * 8 <= PD_POW_LDS_BYTES, "cap");

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
    const Ring<E> R = divide<F, Ring<E>, Lin<E>, RowLoad, RowStore, Team>(fd, W, Lin<E>{bs}, RowLoad{a, dtype, row * na}, na, nb, RowStore{q_out, dtype, row * nq},
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
    const Lin<E> R = divide<F, Lin<E>, Lin<const E>, RowLoad, RowStore, Team>(fd, W, Lin<const E>{bw}, RowLoad{a, dtype, row * na}, na, nb,
                                                                       RowStore{q_out, dtype, row * nq}, q_out != nullptr, true, g);
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
        const Ring<E> R = divide<F, Ring<E>, Lin<E>, RowLoad, NoQuotient, Team>(fd, W, C, RowLoad{a, dtype, row * na}, na, nc, NoQuotient(), false, true, g);
        for (int j = g.tid; j < d; j += g.n) base[j] = R[j];
    }
    g.sync();
    power<F, Lin<E>, Team>(fd, r, base, P, C, d, e, limbs, g);
    for (int j = g.tid; j < d; j += g.n) store_coeff(out, dtype, row * d + j, r[j]);
}

// ---- host ------------------------------------------------------------------------------------------------------------
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
    const int threads = wave_threads(j.nb - 1, MaxThreads<F>::most);
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
    const int rc = allow_large_lds<pd_powmod_kernel<F>>(PD_POW_LDS_BYTES);
    if (rc) return rc;
    const int threads = wave_threads(2 * d - 1, MaxThreads<F>::most);
    hipLaunchKernelGGL((pd_powmod_kernel<F>), dim3((unsigned)j.batch), dim3(threads), pow_lds_elems(d) * sizeof(E), j.st, fd, j.a, j.na, j.e, j.limbs, j.c, j.nc, j.out, j.dtype);
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
    FieldDev fd;
    int rc = field_desc(f, &fd);
    if (rc) return rc;
    const DivJob j{a, b, batch, (int)na, (int)nb, dtype, q_out, r_out, (hipStream_t)stream};
    return for_policy(fd, dtype, "gfa_polydiv", [&](auto p) { return launch_div<typename decltype(p)::type>(fd, j); });
}

int gfa_poly_powmod(gfa_field_t *f, const void *a, int64_t batch, int64_t na, const uint64_t *exp_limbs, int64_t n_limbs, const void *c, int64_t nc,
                    void *out, int dtype, gfa_stream_t stream)
{
    if (!f || batch < 0 || na < 1 || nc < 2 || n_limbs < 1 || n_limbs > (1 << 20) || !exp_limbs) { set_error("gfa_poly_powmod: bad arguments"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0) return GFA_OK;
    if (!a || !c || !out) { set_error("gfa_poly_powmod: bad arguments"); return GFA_ERR_INVALID; }
    if (batch > 0x7fffffff || na > 0x7fffffff || nc > 0x7fffffff) { set_error("gfa_poly_powmod: at most 2^31 - 1 rows of at most 2^31 - 1 coefficients"); return GFA_ERR_UNSUPPORTED; }
    FieldDev fd;
    int rc = field_desc(f, &fd);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    Scratch ws(st);
    u64 *exps = nullptr;
    GFA_HIP(ws.get(&exps, (size_t)n_limbs));
    rc = upload_words(exp_limbs, (size_t)n_limbs, exps, st);
    if (rc) return rc;
    const PowJob j{a, c, batch, (int)na, (int)nc, dtype, exps, (int)n_limbs, out, st};
    return for_policy(fd, dtype, "gfa_polydiv", [&](auto p) { return launch_pow<typename decltype(p)::type>(fd, j); });
}

} // extern "C"
