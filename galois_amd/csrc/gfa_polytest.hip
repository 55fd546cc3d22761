// gfa_polytest.hip -- irreducibility and primitivity of whole batches of polynomials over GF(q), one candidate per lane.
//
//   gfa_poly_classify ... replaces Poly.is_irreducible / Poly.is_primitive (_polys/_irreducible.py:101-124, _primitive.py:70-104)
//                         called once per candidate by the searches of _polys/_search.py.
//
// Irreducibility is Rabin's test as in the reference: x^(q^m) = x (mod f) and gcd(f, x^(q^(m/r)) - x) = 1 for every prime
// r | m.  Primitivity adds f(0) != 0 and x^((q^m - 1)/r) != 1 for every prime r | q^m - 1.  Every power is a power of x, so
// the arithmetic (gfa_polytest.h) is squaring modulo f and multiplication by x, driven by exponent bits that are the same for
// the whole launch (scalar control flow); only the gcd -- a per-candidate Euclid -- lets lanes diverge.
//
// Two launches.  The first classifies every row and appends the indices of the irreducible ones to a list in device memory;
// the second runs the primitivity powers on that list only (about one row in m), sized for the worst case and bounded by the
// count the first left behind -- the host reads nothing back in between.
//
// Two regimes.  GF(2): the candidate and the residue are W in {1, 2, 4} 64-bit words in registers (degrees 1 .. 255).  Every
// other field served by polykit::for_policy (order < 2^64): f, the residue and one work polynomial are lane-strided columns of
// LDS sized by the launch for the degree at hand (degrees 1 .. 32; 3 (m + 1) elements per lane, 50 KiB at m = 32 on 64-bit
// elements), so nothing is indexed per lane in registers and no kernel needs scratch memory.
//
// Storage access (load_coeff), the policy dispatch and the word upload are the family's: gfa_poly_launch.h.
#include <algorithm>

#include "gfa_poly_launch.h"

using namespace gfa;
using namespace gfa::polytest;
using namespace gfa::polykit;

namespace {

constexpr int PT_THREADS = 64;        // one wave per workgroup: a lane only ever touches its own LDS column
constexpr int PT_MAX_DEGREE = 32;     // general fields
constexpr int PT_MAX_DEGREE_GF2 = 255;

typedef unsigned long long ull;

// ---- general fields ------------------------------------------------------------------------------------------------
// row `i` of coeffs -> monic f (f[m] = 1) in the lane's LDS column; false when the leading coefficient is zero
template <class F>
__device__ __forceinline__ bool load_monic(const FieldDev &fd, const void *coeffs, int dtype, i64 i, int m, bool valid,
                                           Col<typename F::elem> f)
{
    typedef typename F::elem E;
    const E one = F::one(fd);
    const E lead = valid ? (E)load_coeff(coeffs, dtype, i * (m + 1)) : (E)0;
    const bool ok = lead != 0;
    f[m] = one;
    if (!ok) { // x^m: the arithmetic below stays defined, the result is discarded
        for (int j = 0; j < m; j++) f[j] = 0;
        return false;
    }
    for (int j = 0; j < m; j++) f[j] = (E)load_coeff(coeffs, dtype, i * (m + 1) + (m - j));
    if (lead != one) {
        const E li = F::inv(fd, lead);
        for (int j = 0; j < m; j++) f[j] = F::mul(fd, f[j], li);
    }
    return true;
}

template <class F>
__global__ __launch_bounds__(PT_THREADS) void pt_irreducible_kernel(FieldDev fd, const void *__restrict__ coeffs, int dtype, i64 batch,
                                                                    int m, const u64 *__restrict__ frob, int n_frob, int limbs,
                                                                    uint8_t *__restrict__ flags, i64 *__restrict__ list,
                                                                    ull *__restrict__ count)
{
    typedef typename F::elem E;
    extern __shared__ u64 pt_lds[];
    E *base = (E *)pt_lds + threadIdx.x;
    const int stride = PT_THREADS, col = (m + 1) * PT_THREADS;
    const Col<E> f{base, stride}, r{base + col, stride}, t{base + 2 * col, stride};
    const i64 i = (i64)blockIdx.x * PT_THREADS + threadIdx.x;
    const bool valid = i < batch;
    const bool ok = load_monic<F>(fd, coeffs, dtype, i, m, valid, f);
    const bool irr = irreducible<F, Col<E>>(fd, f, r, t, m, frob, n_frob, limbs);
    if (!valid) return;
    flags[i] = !ok ? PT_BAD_DEGREE : irr ? PT_IRREDUCIBLE : 0;
    if (ok && irr && list) list[atomicAdd(count, 1ull)] = i;
}

template <class F>
__global__ __launch_bounds__(PT_THREADS) void pt_primitive_kernel(FieldDev fd, const void *__restrict__ coeffs, int dtype, int m,
                                                                  const u64 *__restrict__ exps, int n_exps, int limbs,
                                                                  uint8_t *__restrict__ flags, const i64 *__restrict__ list,
                                                                  const ull *__restrict__ count)
{
    typedef typename F::elem E;
    extern __shared__ u64 pt_lds[];
    const ull n = *count;
    if ((ull)blockIdx.x * PT_THREADS >= n) return;
    E *base = (E *)pt_lds + threadIdx.x;
    const int stride = PT_THREADS, col = (m + 1) * PT_THREADS;
    const Col<E> f{base, stride}, r{base + col, stride}, t{base + 2 * col, stride};
    const ull k = (ull)blockIdx.x * PT_THREADS + threadIdx.x;
    const bool valid = k < n;
    const i64 i = valid ? list[k] : 0;
    load_monic<F>(fd, coeffs, dtype, i, m, valid, f);
    const bool prim = primitive_given_irreducible<F, Col<E>>(fd, f, r, t, m, exps, n_exps, limbs);
    if (valid && prim) flags[i] |= PT_PRIMITIVE;
}

// ---- GF(2) ---------------------------------------------------------------------------------------------------------
// row `i` -> W left-aligned words (coefficient of x^(m - j) at bit 64 W - 1 - j); false when the leading coefficient is zero
template <int W>
__device__ __forceinline__ bool load_bits(const void *coeffs, int dtype, i64 i, int m, bool valid, Bits<W> &f)
{
    f = bzero<W>();
    if (valid) {
#pragma unroll
        for (int wi = 0; wi < W; wi++) {
            const int j0 = wi * 64, n = min(64, m + 1 - j0);
            u64 acc = 0;
            for (int k = 0; k < n; k++) acc |= (load_coeff(coeffs, dtype, i * (m + 1) + j0 + k) & 1) << (63 - k);
            f.w[W - 1 - wi] = acc;
        }
    }
    const bool ok = (f.w[W - 1] >> 63) != 0;
    if (!ok) {
        f = bzero<W>();
        f.w[W - 1] = (u64)1 << 63;
    }
    return ok;
}

template <int W>
__global__ __launch_bounds__(256) void pt_irreducible_gf2_kernel(const void *__restrict__ coeffs, int dtype, i64 batch, int m,
                                                                 const int *__restrict__ steps, int n_steps, uint8_t *__restrict__ flags,
                                                                 i64 *__restrict__ list, ull *__restrict__ count)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < batch;
    Bits<W> f;
    const bool ok = load_bits<W>(coeffs, dtype, i, m, valid, f);
    const bool irr = birreducible<W>(f, m, steps, n_steps);
    if (!valid) return;
    flags[i] = !ok ? PT_BAD_DEGREE : irr ? PT_IRREDUCIBLE : 0;
    if (ok && irr && list) list[atomicAdd(count, 1ull)] = i;
}

template <int W>
__global__ __launch_bounds__(256) void pt_primitive_gf2_kernel(const void *__restrict__ coeffs, int dtype, int m, const u64 *__restrict__ exps,
                                                               int n_exps, int limbs, uint8_t *__restrict__ flags, const i64 *__restrict__ list,
                                                               const ull *__restrict__ count)
{
    const ull n = *count;
    if ((ull)blockIdx.x * blockDim.x >= n) return;
    const ull k = (ull)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = k < n;
    const i64 i = valid ? list[k] : 0;
    Bits<W> f;
    load_bits<W>(coeffs, dtype, i, m, valid, f);
    const bool prim = bprimitive_given_irreducible<W>(f, m, exps, n_exps, limbs);
    if (valid && prim) flags[i] |= PT_PRIMITIVE;
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct Job {
    const void *coeffs;
    i64 batch;
    int m, dtype;
    const u64 *sched; // device: the Frobenius exponents (general fields) or the squaring counts (GF(2))
    int n_sched, sched_limbs;
    const u64 *exps; // device: the cofactor exponents
    int n_exps, exp_limbs;
    bool want_primitive;
    uint8_t *flags;
    i64 *list;
    ull *count;
    hipStream_t st;
};

template <class F>
int launch_general(const FieldDev &fd, const Job &j)
{
    const size_t lds = sizeof(typename F::elem) * 3 * (size_t)(j.m + 1) * PT_THREADS;
    const unsigned grid = (unsigned)((j.batch + PT_THREADS - 1) / PT_THREADS);
    hipLaunchKernelGGL((pt_irreducible_kernel<F>), dim3(grid), dim3(PT_THREADS), lds, j.st, fd, j.coeffs, j.dtype, j.batch, j.m, j.sched,
                       j.n_sched, j.sched_limbs, j.flags, j.list, j.count);
    GFA_HIP(hipGetLastError());
    if (j.want_primitive) {
        hipLaunchKernelGGL((pt_primitive_kernel<F>), dim3(grid), dim3(PT_THREADS), lds, j.st, fd, j.coeffs, j.dtype, j.m, j.exps, j.n_exps,
                           j.exp_limbs, j.flags, (const i64 *)j.list, (const ull *)j.count);
        GFA_HIP(hipGetLastError());
    }
    return GFA_OK;
}

template <int W>
int launch_gf2(const Job &j)
{
    const unsigned grid = (unsigned)((j.batch + 255) / 256);
    hipLaunchKernelGGL((pt_irreducible_gf2_kernel<W>), dim3(grid), dim3(256), 0, j.st, j.coeffs, j.dtype, j.batch, j.m, (const int *)j.sched,
                       j.n_sched, j.flags, j.list, j.count);
    GFA_HIP(hipGetLastError());
    if (j.want_primitive) {
        hipLaunchKernelGGL((pt_primitive_gf2_kernel<W>), dim3(grid), dim3(256), 0, j.st, j.coeffs, j.dtype, j.m, j.exps, j.n_exps, j.exp_limbs,
                           j.flags, (const i64 *)j.list, (const ull *)j.count);
        GFA_HIP(hipGetLastError());
    }
    return GFA_OK;
}

// q^k as little-endian limbs
std::vector<u64> big_pow(u64 q, int k, int limbs)
{
    std::vector<u64> v((size_t)limbs, 0);
    v[0] = 1;
    for (int s = 0; s < k; s++) {
        u64 carry = 0;
        for (int l = 0; l < limbs; l++) {
            const unsigned __int128 t = (unsigned __int128)v[l] * q + carry;
            v[l] = (u64)t;
            carry = (u64)(t >> 64);
        }
    }
    return v;
}

// m / r for the prime divisors r of m, ascending
std::vector<int> rabin_steps(int m)
{
    std::vector<int> out;
    int v = m;
    for (int r = 2; r <= v; r++)
        if (v % r == 0) {
            out.push_back(m / r);
            while (v % r == 0) v /= r;
        }
    std::sort(out.begin(), out.end());
    return out;
}

} // namespace

extern "C" {

int gfa_poly_classify(gfa_field_t *f, const void *coeffs, int64_t batch, int64_t degree, int dtype, const uint64_t *cofactor_exps,
                      int64_t n_exps, int64_t exp_limbs, uint8_t *flags_out, gfa_stream_t stream)
{
    if (!f || batch < 0 || degree < 1 || n_exps < 0 || n_exps > 4096 || (n_exps > 0 && (!cofactor_exps || exp_limbs < 1 || exp_limbs > 4096))) {
        set_error("gfa_poly_classify: bad arguments");
        return GFA_ERR_INVALID;
    }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0) return GFA_OK;
    if (!coeffs || !flags_out) { set_error("gfa_poly_classify: bad arguments"); return GFA_ERR_INVALID; }
    const bool gf2 = f->calc.q == 2;
    if (gf2 && degree > PT_MAX_DEGREE_GF2) { set_error("gfa_poly_classify: degree too large (at most 255 over GF(2))"); return GFA_ERR_UNSUPPORTED; }
    if (!gf2 && degree > PT_MAX_DEGREE) { set_error("gfa_poly_classify: degree too large (at most 32 over fields other than GF(2))"); return GFA_ERR_UNSUPPORTED; }
    FieldDev fd;
    int rc = field_desc(f, &fd);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int m = (int)degree;

    // the schedule of Rabin's test, then the cofactor exponents, in one device buffer
    std::vector<u64> host;
    Job j{};
    const std::vector<int> steps = rabin_steps(m);
    j.n_sched = (int)steps.size() + 1;
    if (gf2) {
        host.resize((size_t)(j.n_sched + 1) / 2 + 1, 0);
        int *s = (int *)host.data();
        for (size_t c = 0; c < steps.size(); c++) s[c] = steps[c];
        s[steps.size()] = m;
    } else {
        int qbits = 64 - clz64(f->calc.q);
        j.sched_limbs = (qbits * m + 63) / 64 + 1;
        for (int c = 0; c < j.n_sched; c++) {
            const std::vector<u64> e = big_pow(f->calc.q, c + 1 < j.n_sched ? steps[c] : m, j.sched_limbs);
            host.insert(host.end(), e.begin(), e.end());
        }
    }
    const size_t exps_at = host.size();
    host.insert(host.end(), cofactor_exps, cofactor_exps + (size_t)(n_exps * exp_limbs));
    j.want_primitive = n_exps > 0 || cofactor_exps != nullptr;

    Scratch ws(st);
    u64 *dev = nullptr;
    i64 *list = nullptr;
    GFA_HIP(ws.get(&dev, host.size()));
    rc = upload_words(host.data(), host.size(), dev, st);
    if (rc) return rc;
    if (j.want_primitive) { // list[0] is the count, the indices follow
        GFA_HIP(ws.get(&list, (size_t)(batch + 1)));
        GFA_HIP(hipMemsetAsync(list, 0, sizeof(i64), st));
    }
    {
        j.coeffs = coeffs; j.batch = batch; j.m = m; j.dtype = dtype;
        j.sched = dev; j.exps = dev + exps_at; j.n_exps = (int)n_exps; j.exp_limbs = (int)exp_limbs;
        j.flags = flags_out; j.list = list ? list + 1 : nullptr; j.count = (ull *)list; j.st = st;
        if (gf2) rc = m <= 63 ? launch_gf2<1>(j) : m <= 127 ? launch_gf2<2>(j) : launch_gf2<4>(j);
        else rc = for_policy(fd, dtype, "gfa_poly_classify", [&](auto p) { return launch_general<typename decltype(p)::type>(fd, j); });
    }
    return rc; // the buffers go back to the pool in stream order
}

} // extern "C"
