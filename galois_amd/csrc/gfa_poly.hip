// gfa_poly.hip -- polynomial functions over a field: the direct-form product (np.convolve), Horner evaluation at many points and
// the Berlekamp-Massey shortest LFSR, on the arithmetic of gfa_arith.h.  Long prime-field products go through gfa_conv_crt.hip.
#include <algorithm>

#include "gfa_internal.h"

using namespace gfa;

namespace {

// np.convolve(a, b) = polynomial product, direct form (convolve_jit.implementation, _domains/_function.py:141-167):
// out[k] = sum_i a[i] * b[k - i].  One output coefficient per thread; large prime-field products go through the NTT
// on the host side (galois_amd/_ntt.py) instead.
template <class F, typename T>
__global__ __launch_bounds__(256) void convolve_kernel(FieldDev fd, const T *__restrict__ a, i64 na, const T *__restrict__ b,
                                                       i64 nb, T *__restrict__ out)
{
    typedef typename F::elem E;
    const i64 n = na + nb - 1;
    for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (i64)gridDim.x * blockDim.x) {
        const i64 lo = k - (nb - 1) > 0 ? k - (nb - 1) : 0;
        const i64 hi = k < na - 1 ? k : na - 1;
        E acc = 0;
        for (i64 i = lo; i <= hi; i++) acc = F::add(fd, acc, F::mul(fd, (E)a[i], (E)b[k - i]));
        out[k] = (T)acc;
    }
}

template <class F, typename T>
int launch_convolve_ft(const FieldDev &fd, const void *a, i64 na, const void *b, i64 nb, void *out, hipStream_t st)
{
    const int grid = grid_for(na + nb - 1, 256, 8);
    hipLaunchKernelGGL((convolve_kernel<F, T>), dim3(grid), dim3(256), 0, st, fd, (const T *)a, na, (const T *)b, nb, (T *)out);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

int dispatch_convolve(const FieldDev &fd, int dtype, const void *a, i64 na, const void *b, i64 nb, void *out, hipStream_t st)
{
    GFA_DISPATCH_FT(launch_convolve_ft, fd, dtype, fd, a, na, b, nb, out, st);
}


// evaluate_elementwise_jit (_polys/_dense.py:432-440): y[i] = Horner(coeffs, x[i]), coefficients highest degree first.
// The coefficient index is uniform across the wave, so the compiler keeps the coefficient stream in scalar loads.
template <class F, typename T>
__global__ __launch_bounds__(256) void poly_eval_kernel(FieldDev fd, const T *__restrict__ coeffs, i64 ncoef,
                                                        const T *__restrict__ x, T *__restrict__ out, i64 n)
{
    typedef typename F::elem E;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        const E xv = (E)x[i];
        E acc = (E)coeffs[0];
        for (i64 j = 1; j < ncoef; j++) acc = F::add(fd, F::mul(fd, acc, xv), (E)coeffs[j]);
        out[i] = (T)acc;
    }
}

template <class F, typename T>
int launch_poly_eval_ft(const FieldDev &fd, const void *coeffs, i64 ncoef, const void *x, void *out, i64 n, hipStream_t st)
{
    const int grid = grid_for(n, 256, 8);
    hipLaunchKernelGGL((poly_eval_kernel<F, T>), dim3(grid), dim3(256), 0, st, fd, (const T *)coeffs, ncoef, (const T *)x, (T *)out, n);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

// r06: Horner's rule for the fields of at most 256 elements on uint8 arrays with the full 64 KiB PRODUCT table in LDS (row = the point x, fixed
// per lane; column = the running value: random banks) -- one LDS gather per coefficient where the generic kernel does two or three gathers
// from L2 (and two more through Zech logarithms per addition in odd characteristic; here the 64 KiB SUM table, row = the coefficient).
// Four points per lane: four independent chains cover the gather latency.  One persistent 1024-thread workgroup per CU.
template <bool ODD>
__global__ __launch_bounds__(1024) void poly_eval_tab8_kernel(const uint8_t *__restrict__ mul8, const uint8_t *__restrict__ add8, const uint8_t *__restrict__ coeffs,
                                                              i64 ncoef, const uint8_t *__restrict__ x, uint8_t *__restrict__ out, i64 n)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t pe_lds[];
    {
        const uint4 *s0 = reinterpret_cast<const uint4 *>(mul8);
        uint4 *d0 = reinterpret_cast<uint4 *>(pe_lds);
        for (int i = threadIdx.x; i < 4096; i += 1024) d0[i] = s0[i];
        if (ODD) {
            const uint4 *s1 = reinterpret_cast<const uint4 *>(add8);
            for (int i = threadIdx.x; i < 4096; i += 1024) d0[4096 + i] = s1[i];
        }
    }
    __syncthreads();
    const uint8_t *mt = pe_lds, *at = pe_lds + 65536;
    const i64 stride = (i64)gridDim.x * 1024;
    for (i64 i0 = (i64)blockIdx.x * 1024 + threadIdx.x; i0 < n; i0 += 4 * stride) {
        u32 row[4], acc[4];
        const u32 c0 = coeffs[0];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const i64 i = i0 + k * stride;
            row[k] = (i < n ? (u32)x[i] : 0u) << 8;
            acc[k] = c0;
        }
        for (i64 j = 1; j < ncoef; j++) {
            const u32 c = coeffs[j]; // uniform: a scalar load
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u32 prod = mt[row[k] | acc[k]];
                acc[k] = ODD ? (u32)at[(c << 8) | prod] : (prod ^ c);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const i64 i = i0 + k * stride;
            if (i < n) out[i] = (uint8_t)acc[k];
        }
    }
}

int launch_poly_eval_tab8(const uint8_t *mul8, const uint8_t *add8, bool odd, const void *coeffs, i64 ncoef, const void *x, void *out, i64 n, hipStream_t st)
{
    static bool attr[2] = {false, false};
    const size_t lds = odd ? 131072 : 65536;
    const void *k = odd ? (const void *)poly_eval_tab8_kernel<true> : (const void *)poly_eval_tab8_kernel<false>;
    if (!attr[odd]) { GFA_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); attr[odd] = true; }
    const i64 blocks = (n + 4095) / 4096;
    const int grid = (int)std::min<i64>(blocks, (i64)num_cus());
    if (odd)
        hipLaunchKernelGGL(poly_eval_tab8_kernel<true>, dim3(grid), dim3(1024), lds, st, mul8, add8, (const uint8_t *)coeffs, ncoef, (const uint8_t *)x, (uint8_t *)out, n);
    else
        hipLaunchKernelGGL(poly_eval_tab8_kernel<false>, dim3(grid), dim3(1024), lds, st, mul8, add8, (const uint8_t *)coeffs, ncoef, (const uint8_t *)x, (uint8_t *)out, n);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

int dispatch_poly_eval(const FieldDev &fd, int dtype, const void *coeffs, i64 ncoef, const void *x, void *out, i64 n, hipStream_t st)
{
    GFA_DISPATCH_FT(launch_poly_eval_ft, fd, dtype, fd, coeffs, ncoef, x, out, n, st);
}

// berlekamp_massey_jit.implementation (_lfsr.py:1647-1702): shortest LFSR (connection polynomial C, ascending) of each of
// `batch` sequences of length n.  One 64-lane workgroup per sequence, C / B / T in LDS; the discrepancy is a strided
// partial sum folded in LDS.  out_c: (batch, n) ascending coefficients, zero padded; out_len: trimmed length (>= 1).
template <class F, typename T>
__global__ __launch_bounds__(64) void berlekamp_massey_kernel(FieldDev fd, const T *__restrict__ seq, i64 n, T *__restrict__ out_c,
                                                              i64 *__restrict__ out_len)
{
    typedef typename F::elem E;
    extern __shared__ __attribute__((aligned(16))) unsigned char bm_raw[];
    E *C = reinterpret_cast<E *>(bm_raw), *B = C + n, *Tm = B + n;
    __shared__ u64 part[64];
    const T *S = seq + (i64)blockIdx.x * n;
    const int tid = threadIdx.x;
    for (i64 i = tid; i < n; i += 64) { C[i] = i == 0 ? F::one(fd) : (E)0; B[i] = C[i]; }
    __syncthreads();
    i64 L = 0, m = 1;
    E b = F::one(fd);
    for (i64 k = 0; k < n; k++) {
        E acc = 0;
        for (i64 i = tid; i <= L; i += 64) acc = F::add(fd, acc, F::mul(fd, (E)S[k - i], C[i]));
        part[tid] = (u64)acc;
        __syncthreads();
        for (int off = 32; off >= 1; off >>= 1) {
            if (tid < off) part[tid] = (u64)F::add(fd, (E)part[tid], (E)part[tid + off]);
            __syncthreads();
        }
        const E d = (E)part[0];
        __syncthreads();
        if (d == 0) { m++; continue; }
        E coef;
        if constexpr (std::is_same<F, Lut>::value) coef = Lut::div_nz(fd, d, b);
        else coef = F::mul(fd, d, F::inv(fd, b));
        const bool grow = !(2 * L > k);
        if (grow) for (i64 i = tid; i < n; i += 64) Tm[i] = C[i];
        __syncthreads();
        for (i64 i = m + tid; i < n; i += 64) C[i] = F::sub(fd, C[i], F::mul(fd, coef, B[i - m]));
        __syncthreads();
        if (grow) {
            for (i64 i = tid; i < n; i += 64) B[i] = Tm[i];
            L = k + 1 - L; b = d; m = 1;
        } else {
            m++;
        }
        __syncthreads();
    }
    // C[: L + 1], trailing zeros trimmed (at least one coefficient)
    const i64 clen = L + 1 < n ? L + 1 : n;
    if (tid == 0) {
        i64 last = 0;
        for (i64 i = 0; i < clen; i++) if (C[i] != 0) last = i;
        out_len[blockIdx.x] = last + 1;
    }
    for (i64 i = tid; i < n; i += 64) out_c[(i64)blockIdx.x * n + i] = i < clen ? (T)C[i] : (T)0;
}

template <class F, typename T>
int launch_bm_ft(const FieldDev &fd, const void *seq, i64 n, i64 batch, void *out_c, i64 *out_len, hipStream_t st)
{
    typedef typename F::elem E;
    const size_t lds = 3 * (size_t)n * sizeof(E);
    auto k = berlekamp_massey_kernel<F, T>;
    static bool attr = false;
    if (!attr) { GFA_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024)); attr = true; }
    hipLaunchKernelGGL(k, dim3((unsigned)batch), dim3(64), lds, st, fd, (const T *)seq, n, (T *)out_c, out_len);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}
int dispatch_bm(const FieldDev &fd, int dtype, const void *seq, i64 n, i64 batch, void *out_c, i64 *out_len, hipStream_t st)
{
    GFA_DISPATCH_FT(launch_bm_ft, fd, dtype, fd, seq, n, batch, out_c, out_len, st);
}

} // namespace

extern "C" {

int gfa_convolve(gfa_field_t *f, const void *a, int64_t na, const void *b, int64_t nb, void *out, int dtype,
                 gfa_stream_t stream)
{
    if (!f || !a || !b || !out || na < 1 || nb < 1) { set_error("gfa_convolve: bad arguments"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    FieldDeviceState *ds;
    int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    if (convolve_crt_eligible(f->calc, na, nb)) return convolve_crt(f, dtype, a, na, b, nb, out, (hipStream_t)stream);
    if (f->use_lookup()) return dispatch_convolve(f->lut_desc(*ds), dtype, a, na, b, nb, out, (hipStream_t)stream);
    return dispatch_convolve(f->calc, dtype, a, na, b, nb, out, (hipStream_t)stream);
}

int gfa_berlekamp_massey(gfa_field_t *f, const void *seq, int64_t n, int64_t batch, void *out_coeffs, int64_t *out_len, int dtype,
                          gfa_stream_t stream)
{
    if (!f || n < 1 || batch < 0) { set_error("gfa_berlekamp_massey: bad arguments"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0) return GFA_OK;
    if (!seq || !out_coeffs || !out_len) { set_error("gfa_berlekamp_massey: bad arguments"); return GFA_ERR_INVALID; }
    if (n > 6000 || batch > 0x7fffffff) { set_error("gfa_berlekamp_massey: sequences are limited to 6000 terms"); return GFA_ERR_UNSUPPORTED; }
    FieldDeviceState *ds;
    int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    if (f->use_lookup()) return dispatch_bm(f->lut_desc(*ds), dtype, seq, n, batch, out_coeffs, (i64 *)out_len, (hipStream_t)stream);
    return dispatch_bm(f->calc, dtype, seq, n, batch, out_coeffs, (i64 *)out_len, (hipStream_t)stream);
}

int gfa_poly_evaluate(gfa_field_t *f, const void *coeffs, int64_t ncoef, const void *x, void *out, int64_t n, int dtype,
                      gfa_stream_t stream)
{
    if (!f || !coeffs || ncoef < 1 || n < 0) { set_error("gfa_poly_evaluate: bad arguments"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (n == 0) return GFA_OK;
    if (!x || !out) { set_error("gfa_poly_evaluate: bad arguments"); return GFA_ERR_INVALID; }
    FieldDeviceState *ds;
    int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    if (f->has_tab8 && f->use_lookup() && dtype == GFA_U8 && ds->mul8 && (f->calc.p == 2 || ds->add8) && n >= 65536 && ncoef >= 4) // r06: product (and sum) table in LDS
        return launch_poly_eval_tab8(ds->mul8, ds->add8, f->calc.p != 2, coeffs, ncoef, x, out, n, (hipStream_t)stream);
    if (f->use_lookup()) return dispatch_poly_eval(f->lut_desc(*ds), dtype, coeffs, ncoef, x, out, n, (hipStream_t)stream);
    return dispatch_poly_eval(f->calc, dtype, coeffs, ncoef, x, out, n, (hipStream_t)stream);
}

} // extern "C"
