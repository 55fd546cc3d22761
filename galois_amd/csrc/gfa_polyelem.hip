// gfa_polyelem.hip -- primitive and normal elements of GF(q^m) = GF(q)[x] / (f), whole batches of residues, one per lane.
//
//   gfa_poly_element_classify ... replaces is_primitive_element / is_normal_element (_fields/_primitive_element.py:137-166,
//                                 _fields/_normal_element.py:143-185), which the reference calls once per candidate from its
//                                 searches and enumerations.
//
// Primitivity is the reference's order test: g != 0 and g^((q^m - 1) / r) != 1 for every prime r | q^m - 1.  Normality is the
// rank test in the form of gfa_polyelem.h: c_i(Phi) g != 0 for the cofactors c_i = (x^m - 1) / P_i of the distinct irreducible
// factors of x^m - 1, with the matrices c_i(Phi) built once per field by the caller -- a few rows of a matrix-vector product per
// candidate in place of an elimination.  One modulus serves the whole launch, and the exponent bits are uniform over it.
//
// Two regimes, as gfa_polytest.hip.  GF(2): the residue is W in {1, 2, 4} 64-bit words in registers (degrees 1 .. 255); matrix
// rows are packed into the same words by a first launch and staged through a 32 KiB slab of LDS.  Every other field served by
// polykit::for_policy: one wave per workgroup; f once (stride 1, read by every lane at the same address), then the lane-strided
// columns g, r and t.  After the powers the space of r and t holds the slab of cofactor matrices -- every lane reads the same
// entry, each its own column of g.  The slab is sized from a 64 KiB budget: with 64-bit elements at m = 32 that is 5 of up to 32
// matrices per pass.
//
// Storage access (load_elem), the policy dispatch and the word upload are the family's: gfa_poly_launch.h.
#include <algorithm>

#include "gfa_poly_launch.h"
#include "gfa_polyelem.h"

using namespace gfa;
using namespace gfa::polytest;
using namespace gfa::polyelem;
using namespace gfa::polykit;

namespace {

constexpr int PE_THREADS = 64; // one wave per workgroup: a lane only ever writes its own LDS column
constexpr int PE_MAX_DEGREE = 32;
constexpr int PE_MAX_DEGREE_GF2 = 255;
constexpr size_t PE_LDS_BUDGET = 64 * 1024;
constexpr int PE_GF2_THREADS = 256;
constexpr int PE_GF2_SLAB_WORDS = 4096; // 32 KiB: at least 4 matrices (255 rows of 4 words)

// ---- general fields ------------------------------------------------------------------------------------------------
template <class F>
__global__ __launch_bounds__(PE_THREADS) void pe_general_kernel(FieldDev fd, u64 q, const void *__restrict__ elems,
                                                                const void *__restrict__ modulus, int dtype, i64 batch, int m,
                                                                const u64 *__restrict__ exps, int n_exps, int limbs, int want_primitive,
                                                                const void *__restrict__ mats, int n_mats, int slab_mats,
                                                                uint8_t *__restrict__ flags)
{
    typedef typename F::elem E;
    extern __shared__ u64 pe_lds[];
    E *fs = (E *)pe_lds;                      // m + 1 coefficients of f, ascending
    E *cols = fs + (m + 1) + threadIdx.x;     // this lane's entry of coefficient 0 of g
    E *work = fs + (m + 1) + m * PE_THREADS;  // r and t, then the slab of matrices
    const int stride = PE_THREADS, col = m * PE_THREADS;
    const Col<E> f{fs, 1}, g{cols, stride}, r{cols + col, stride}, t{cols + 2 * col, stride};
    const i64 i = (i64)blockIdx.x * PE_THREADS + threadIdx.x;
    const bool valid = i < batch;

    for (int j = threadIdx.x; j <= m; j += PE_THREADS) fs[j] = (E)load_elem(modulus, dtype, m - j, q);
    for (int j = 0; j < m; j++) g[j] = valid ? (E)load_elem(elems, dtype, i * m + (m - 1 - j), q) : (E)0;
    __syncthreads();

    uint8_t out = 0;
    const bool nonzero = !is_zero(g, m);
    if (want_primitive) {
        bool alive = nonzero;
        for (int c = 0; c < n_exps && __any(alive); c++) {
            pow_g<F, Col<E>>(fd, r, t, g, f, m, exps + (size_t)c * limbs, limbs);
            alive = alive && !is_one<F, Col<E>>(fd, r, m);
        }
        if (alive) out |= PE_PRIMITIVE;
    }
    if (mats) {
        bool alive = nonzero;
        const int mm = m * m;
        for (int base = 0; base < n_mats && __any(alive); base += slab_mats) { // one wave: the trip count is the workgroup's
            const int n = min(slab_mats, n_mats - base);
            __syncthreads();
            for (int k = threadIdx.x; k < n * mm; k += PE_THREADS) work[k] = (E)load_elem(mats, dtype, (i64)base * mm + k, q);
            __syncthreads();
            if (alive) alive = survives<F, Col<E>>(fd, work, n, g, m);
        }
        if (alive) out |= PE_NORMAL;
    }
    if (valid) flags[i] = out;
}

// ---- GF(2) ---------------------------------------------------------------------------------------------------------
// One launch packs what the classifier reads as words: thread `n_rows` the modulus (x^(m - k) at bit 64 W - 1 - k; the top bit
// is set whatever the buffer holds, so that a reduction always clears it), thread r < n_rows row r of the stacked matrices
// (column j at bit 64 W - 1 - m + j, where coefficient j of a residue sits).  packed = f, then the rows.
template <int W>
__global__ void pe_pack_gf2_kernel(const void *__restrict__ modulus, const void *__restrict__ mats, int dtype, int m, int n_rows,
                                   u64 *__restrict__ packed)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row > n_rows) return;
    Bits<W> b = bzero<W>();
    if (row == n_rows) {
        for (int k = 1; k <= m; k++) bset<W>(b, 64 * W - 1 - k, load_elem(modulus, dtype, k, 2) != 0);
        b.w[W - 1] |= (u64)1 << 63;
#pragma unroll
        for (int w = 0; w < W; w++) packed[w] = b.w[w];
    } else {
        const int s = 64 * W - 1 - m;
        for (int j = 0; j < m; j++) bset<W>(b, s + j, load_elem(mats, dtype, (i64)row * m + j, 2) != 0);
#pragma unroll
        for (int w = 0; w < W; w++) packed[(size_t)W + (size_t)row * W + w] = b.w[w];
    }
}

template <int W>
__global__ __launch_bounds__(PE_GF2_THREADS) void pe_gf2_kernel(const void *__restrict__ elems, int dtype, i64 batch, int m,
                                                                const u64 *__restrict__ packed, const u64 *__restrict__ exps, int n_exps,
                                                                int limbs, int want_primitive, int n_mats, int slab_mats,
                                                                uint8_t *__restrict__ flags)
{
    __shared__ u64 slab[PE_GF2_SLAB_WORDS];
    const i64 i = (i64)blockIdx.x * PE_GF2_THREADS + threadIdx.x;
    const bool valid = i < batch;
    Bits<W> f, g = bzero<W>();
#pragma unroll
    for (int w = 0; w < W; w++) f.w[w] = packed[w];
    if (valid)
        for (int k = 0; k < m; k++) bset<W>(g, 64 * W - 2 - k, load_elem(elems, dtype, i * m + k, 2) != 0); // x^(m - 1 - k)

    uint8_t out = 0;
    if (want_primitive && bprimitive_element<W>(g, f, m, exps, n_exps, limbs)) out |= PE_PRIMITIVE;
    if (n_mats > 0) {
        bool alive = !bis_zero<W>(g);
        const u64 *rows = packed + W;
        const int words = m * W; // per matrix
        for (int base = 0; base < n_mats; base += slab_mats) {
            const int n = min(slab_mats, n_mats - base);
            __syncthreads();
            for (int k = threadIdx.x; k < n * words; k += PE_GF2_THREADS) slab[k] = rows[(size_t)base * words + k];
            __syncthreads();
            if (alive) alive = bsurvives<W>(slab, n, g, m);
        }
        if (alive) out |= PE_NORMAL;
    }
    if (valid) flags[i] = out;
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct Job {
    const void *elems, *modulus, *mats;
    i64 batch;
    int m, dtype, n_mats;
    u64 q;
    const u64 *exps; // device
    int n_exps, limbs;
    bool want_primitive;
    u64 *packed; // GF(2): device words of f and of the matrix rows
    uint8_t *flags;
    hipStream_t st;
};

template <class F>
int launch_general(const FieldDev &fd, const Job &j)
{
    typedef typename F::elem E;
    const size_t fixed = (size_t)(j.m + 1) + (size_t)j.m * PE_THREADS, mm = (size_t)j.m * j.m;
    size_t work = j.want_primitive ? 2 * (size_t)j.m * PE_THREADS : 0;
    int slab_mats = 1;
    if (j.mats) {
        const size_t room = PE_LDS_BUDGET / sizeof(E) - fixed; // at m = 32 on 64-bit elements: 6111 elements, 5 matrices
        slab_mats = (int)std::max<size_t>(1, std::min<size_t>(room / mm, (size_t)j.n_mats));
        work = std::max(work, (size_t)slab_mats * mm);
    }
    const size_t lds = (fixed + work) * sizeof(E);
    const unsigned grid = (unsigned)((j.batch + PE_THREADS - 1) / PE_THREADS);
    hipLaunchKernelGGL((pe_general_kernel<F>), dim3(grid), dim3(PE_THREADS), lds, j.st, fd, j.q, j.elems, j.modulus, j.dtype, j.batch, j.m,
                       j.exps, j.n_exps, j.limbs, (int)j.want_primitive, j.mats, j.n_mats, slab_mats, j.flags);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

template <int W>
int launch_gf2(const Job &j)
{
    const int n_rows = j.mats ? j.n_mats * j.m : 0;
    hipLaunchKernelGGL((pe_pack_gf2_kernel<W>), dim3((unsigned)(n_rows / 256 + 1)), dim3(256), 0, j.st, j.modulus, j.mats, j.dtype, j.m, n_rows,
                       j.packed);
    GFA_HIP(hipGetLastError());
    const int slab_mats = PE_GF2_SLAB_WORDS / (j.m * W);
    const unsigned grid = (unsigned)((j.batch + PE_GF2_THREADS - 1) / PE_GF2_THREADS);
    hipLaunchKernelGGL((pe_gf2_kernel<W>), dim3(grid), dim3(PE_GF2_THREADS), 0, j.st, j.elems, j.dtype, j.batch, j.m, (const u64 *)j.packed,
                       j.exps, j.n_exps, j.limbs, (int)j.want_primitive, j.mats ? j.n_mats : 0, slab_mats, j.flags);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

} // namespace

extern "C" {

int gfa_poly_element_classify(gfa_field_t *f, const void *elements, int64_t batch, const void *modulus, int64_t degree, int dtype,
                              const uint64_t *cofactor_exps, int64_t n_exps, int64_t exp_limbs, const void *normal_mats, int64_t n_mats,
                              uint8_t *flags_out, gfa_stream_t stream)
{
    if (!f) {
        set_error("gfa_poly_element_classify: fields of order 2^64 and above are not served (no gfa_field_t)");
        return GFA_ERR_UNSUPPORTED;
    }
    if (batch < 0 || batch > 0x7fffffffll || degree < 1 || n_exps < 0 || n_exps > 4096 ||
        (n_exps > 0 && (!cofactor_exps || exp_limbs < 1 || exp_limbs > 4096)) || n_mats < 0 || n_mats > 4096) {
        set_error("gfa_poly_element_classify: bad arguments");
        return GFA_ERR_INVALID;
    }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    const bool gf2 = f->calc.q == 2;
    if (gf2 && degree > PE_MAX_DEGREE_GF2) { set_error("gfa_poly_element_classify: degree too large (at most 255 over GF(2))"); return GFA_ERR_UNSUPPORTED; }
    if (!gf2 && degree > PE_MAX_DEGREE) { set_error("gfa_poly_element_classify: degree too large (at most 32 over fields other than GF(2))"); return GFA_ERR_UNSUPPORTED; }
    if (batch == 0) return GFA_OK;
    if (!elements || !modulus || !flags_out) { set_error("gfa_poly_element_classify: bad arguments"); return GFA_ERR_INVALID; }
    FieldDev fd;
    int rc = field_desc(f, &fd);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;

    Job j{};
    j.elems = elements; j.modulus = modulus; j.batch = batch; j.m = (int)degree; j.dtype = dtype; j.q = f->calc.q;
    j.mats = n_mats > 0 ? normal_mats : nullptr; j.n_mats = j.mats ? (int)n_mats : 0;
    j.want_primitive = n_exps > 0 || cofactor_exps != nullptr;
    j.n_exps = (int)n_exps; j.limbs = n_exps > 0 ? (int)exp_limbs : 1;
    j.flags = flags_out; j.st = st;

    Scratch ws(st);
    u64 *dev = nullptr;
    const size_t n_words = (size_t)j.n_exps * j.limbs;
    GFA_HIP(ws.get(&dev, std::max<size_t>(n_words, 1)));
    if (n_words) {
        rc = upload_words(cofactor_exps, n_words, dev, st);
        if (rc) return rc;
    }
    j.exps = dev;
    if (gf2) {
        const int W = j.m <= 63 ? 1 : j.m <= 127 ? 2 : 4;
        GFA_HIP(ws.get(&j.packed, (size_t)W * (1 + (size_t)j.n_mats * j.m)));
        return W == 1 ? launch_gf2<1>(j) : W == 2 ? launch_gf2<2>(j) : launch_gf2<4>(j);
    }
    // the buffers go back to the pool in stream order
    return for_policy(fd, dtype, "gfa_poly_element_classify", [&](auto p) { return launch_general<typename decltype(p)::type>(fd, j); });
}

} // extern "C"
