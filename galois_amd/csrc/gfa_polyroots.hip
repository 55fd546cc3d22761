// gfa_polyroots.hip -- the roots in GF(q), q < 2^64, of a stack of polynomials, and their multiplicities.
//
//   gfa_poly_roots ................ replaces roots_jit (Chien search over all q elements, _polys/_dense.py:443-513) and the
//                                   loop of _root_multiplicity over the roots (_polys/_poly.py:1672-1698)
//   gfa_poly_root_multiplicity .... the second half on its own: multiplicities of GIVEN elements (roots found algebraically)
//
// pr_search_kernel   the candidates are the integers 0 .. q - 1, made from the index and never read from memory; every lane runs
//                    Horner's rule on Chains<F>::n independent candidates over the row's coefficients, which the workgroup holds
//                    in LDS as elements of the field policy (one broadcast read per coefficient, whatever the storage type).
//                    The grid is rows x chunks: workgroup b works on row b / chunks and on the candidates
//                    (b % chunks) * 256 + lane, + chunks * 256, ...; `chunks` is picked from batch and q so that one polynomial
//                    over a large field and many short rows over a small one both fill the device.  Candidate indices are
//                    64 bits wide.  A hit takes a slot of its row with one atomicAdd on the row's counter and stores the
//                    candidate if the slot is below the row's capacity (polyroots::slot_in_row); nothing loops on the value an
//                    atomic returned.  A workgroup that finds its row all zero leaves at once: every candidate would hit.
// pr_finish_kernel   one workgroup per row (gfa_polyroots.h): zero row from the coefficients, rank sort of the slots in LDS,
//                    multiplicities by repeated synthetic division, one thread per root.  The slots are the row of roots_out
//                    itself, zeroed before the search, so the result does not depend on the order the hits arrived in.
//
// LDS of pr_finish_kernel, in elements of the field policy (32 bits for Prime32 and Lut, 64 bits otherwise):
//   c[ncoef] slots[nroots] sorted[nroots] work[lanes * ncoef]     lanes = roots whose divisions run at the same time
// of 150 KiB.  With nroots = ncoef - 1 and lanes >= 1 that is 4 ncoef - 2 elements at least, so
//   ncoef <= PR_MAX_TERMS(sizeof element) = 150 KiB / sizeof element / 4 = 9600 / 4800;
// above it the entry points return GFA_ERR_UNSUPPORTED and the caller takes the algebraic route (galois_amd/_polyroots.py).
#include <algorithm>

#include "gfa_poly_launch.h"
#include "gfa_polyroots.h"

using namespace gfa;
using namespace gfa::polykit;

namespace {

constexpr int PR_SEARCH_THREADS = 256;
// independent candidates per lane: four chains cover the latency of a product; a digit-vector product is M^2 independent
// multiplications already
template <class F>
struct Chains {
    static constexpr int n = 4;
};
template <int M>
struct Chains<ExtP<M>> {
    static constexpr int n = 1;
};
constexpr size_t PR_LDS_BYTES = 150 * 1024;
constexpr i64 PR_MAX_TERMS(size_t elem) { return (i64)(PR_LDS_BYTES / elem / 4); }
// q (ncoef - 1) batch Horner steps at most in one search: minutes of one launch on a device others share is a hang to them
constexpr unsigned __int128 PR_MAX_WORK = (unsigned __int128)1 << 42;

struct RowMult { // a row of mult_out
    int32_t *p;
    __device__ __forceinline__ void set(int i, int m) const { p[i] = m; }
};

template <class F>
__global__ __launch_bounds__(PR_SEARCH_THREADS) void pr_search_kernel(FieldDev fd, const void *__restrict__ coeffs, int ncoef, u32 chunks,
                                                                      void *__restrict__ roots_out, u32 *__restrict__ counter, int dtype)
{
    typedef typename F::elem E;
    constexpr int K = Chains<F>::n;
    extern __shared__ u64 pr_lds[];
    E *c = (E *)pr_lds;
    const int tid = threadIdx.x;
    const i64 row = blockIdx.x / chunks;
    const u32 chunk = blockIdx.x % chunks;
    bool nz = false;
    for (int i = tid; i < ncoef; i += PR_SEARCH_THREADS) {
        const E v = (E)load_coeff(coeffs, dtype, row * ncoef + i);
        c[i] = v;
        nz = nz || v != 0;
    }
    if (!__syncthreads_or(nz)) return; // the zero row: pr_finish_kernel reports it
    const int cap = ncoef - 1;
    const RowStore out{roots_out, dtype, row * cap};
    const u64 q = fd.q, sub = (u64)chunks * PR_SEARCH_THREADS, step = sub * K; // sub: between the chains of a lane
    u64 x0 = (u64)chunk * PR_SEARCH_THREADS + tid;
    if (x0 >= q) return;
    const u64 iters = (q - 1 - x0) / step + 1; // counted, so that x0 + step may wrap behind the last one
    for (u64 it = 0; it < iters; it++, x0 += step) {
        E x[K], acc[K];
        bool live[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            live[k] = (u64)k * sub <= q - 1 - x0;
            x[k] = (E)(live[k] ? x0 + (u64)k * sub : x0);
            acc[k] = c[0];
        }
        for (int j = 1; j < ncoef; j++) {
            const E cj = c[j]; // the same address in every lane
#pragma unroll
            for (int k = 0; k < K; k++) acc[k] = F::add(fd, F::mul(fd, acc[k], x[k]), cj);
        }
#pragma unroll
        for (int k = 0; k < K; k++)
            if (live[k] && acc[k] == 0) polyroots::take_slot(out, cap, atomicAdd(&counter[row], 1u), (u64)x[k]);
    }
}

// counter != null: after a search -- roots is the row of slots, sorted in place; count_out and (nullable) mult_out are written.
// counter == null: roots holds nroots given elements per row and only mult_out is written (0 for an element that is no root
// and for every element of a zero row).
template <class F>
__global__ __launch_bounds__(MaxThreads<F>::most) void pr_finish_kernel(FieldDev fd, const void *__restrict__ coeffs, int ncoef, void *roots, int nroots,
                                                                  const u32 *__restrict__ counter, int64_t *__restrict__ count_out,
                                                                  int32_t *__restrict__ mult_out, int lanes, int dtype)
{
    typedef typename F::elem E;
    extern __shared__ u64 pr_lds[];
    E *c = (E *)pr_lds, *slots = c + ncoef, *sorted = slots + nroots, *work = sorted + nroots;
    const Team g{(int)threadIdx.x, (int)blockDim.x};
    const i64 row = blockIdx.x;
    for (int i = g.tid; i < ncoef; i += g.n) c[i] = (E)load_coeff(coeffs, dtype, row * ncoef + i);
    for (int i = g.tid; i < nroots; i += g.n) slots[i] = (E)load_coeff(roots, dtype, row * nroots + i);
    const bool zero = !__syncthreads_or(!polyroots::share_is_zero(c, ncoef, g)); // (a thread's share is what it loaded; the barrier orders the rest)
    const RowMult mult{mult_out ? mult_out + row * nroots : nullptr};
    if (!counter) {
        if (zero)
            for (int i = g.tid; i < nroots; i += g.n) mult.set(i, 0);
        else polyroots::multiplicities<F, RowMult, Team>(fd, c, ncoef, slots, nroots, work, lanes, mult, g);
        return;
    }
    const int n = polyroots::finish_row<F, RowMult, Team>(fd, c, ncoef, zero, slots, counter[row], sorted, work, lanes, mult_out != nullptr, mult, g);
    const int roots_n = n > 0 ? n : 0;
    for (int i = g.tid; i < nroots; i += g.n) {
        store_coeff(roots, dtype, row * nroots + i, i < roots_n ? (u64)sorted[i] : 0);
        if (mult_out && i >= roots_n) mult.set(i, 0); // the places of the roots have their owners
    }
    if (g.tid == 0) count_out[row] = n;
}

// ---- host ------------------------------------------------------------------------------------------------------------
// does a row with its roots and one quotient fit the finishing kernel's LDS?  Checked before anything is written.
bool fits_lds(const FieldDev &fd, const char *who, i64 ncoef, i64 nroots)
{
    const i64 cap = PR_MAX_TERMS(elem_bytes(fd));
    if (ncoef <= cap && 2 * ncoef + 2 * nroots <= (i64)(PR_LDS_BYTES / elem_bytes(fd))) return true;
    set_error(std::string(who) + ": ncoef = " + std::to_string(ncoef) + ", the finishing kernel holds a row, its roots and one quotient in LDS up to ncoef = " +
              std::to_string(cap) + " over this field");
    return false;
}

struct RootsJob {
    const void *coeffs;
    i64 batch;
    int ncoef, nroots, dtype;
    void *roots;
    u32 *counter; // null: the roots are given
    int64_t *count;
    int32_t *mult;
    hipStream_t st;
};

template <class F>
int launch_roots(const FieldDev &fd, const RootsJob &j)
{
    typedef typename F::elem E;
    const char *who = j.counter ? "gfa_poly_roots" : "gfa_poly_root_multiplicity";
    const i64 fixed = (i64)j.ncoef + 2 * (i64)j.nroots, room = (i64)(PR_LDS_BYTES / sizeof(E));
    if (j.ncoef > PR_MAX_TERMS(sizeof(E)) || fixed + j.ncoef > room) {
        set_error(std::string(who) + ": ncoef = " + std::to_string(j.ncoef) + ", the finishing kernel holds a row, its roots and one quotient in LDS up to ncoef = " +
                  std::to_string(PR_MAX_TERMS(sizeof(E))) + " over this field");
        return GFA_ERR_UNSUPPORTED;
    }
    if (j.counter) {
        // enough workgroups for 8 per compute unit, no more per row than it has candidates for
        const u64 per_row = (fd.q - 1) / ((u64)PR_SEARCH_THREADS * Chains<F>::n) + 1;
        const i64 want = ((i64)num_cus() * 8 + j.batch - 1) / j.batch;
        const u64 chunks = std::max<u64>(1, std::min<u64>({(u64)want, per_row, (u64)(0x7fffffff / j.batch)}));
        hipLaunchKernelGGL(pr_search_kernel<F>, dim3((unsigned)(j.batch * (i64)chunks)), dim3(PR_SEARCH_THREADS), (size_t)j.ncoef * sizeof(E), j.st, fd, j.coeffs, j.ncoef,
                           (u32)chunks, j.roots, j.counter, j.dtype);
        GFA_HIP(hipGetLastError());
    }
    const int rc = allow_large_lds<pr_finish_kernel<F>>(PR_LDS_BYTES);
    if (rc) return rc;
    const int threads = wave_threads(j.nroots, MaxThreads<F>::most);
    const int lanes = j.mult ? (int)std::min<i64>({(i64)threads, (i64)j.nroots, (room - fixed) / j.ncoef}) : 0;
    hipLaunchKernelGGL((pr_finish_kernel<F>), dim3((unsigned)j.batch), dim3(threads), (size_t)(fixed + (i64)lanes * j.ncoef) * sizeof(E), j.st, fd, j.coeffs, j.ncoef, j.roots, j.nroots,
                       j.counter, j.count, j.mult, lanes, j.dtype);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

} // namespace

extern "C" {

int gfa_poly_roots(gfa_field_t *f, const void *coeffs, int64_t batch, int64_t ncoef, void *roots_out, int32_t *mult_out, int64_t *count_out, int dtype,
                   gfa_stream_t stream)
{
    if (!f) { // fields of order >= 2^64 have no gfa_field_t
        set_error("gfa_poly_roots: no field handle (fields of order >= 2^64 are not served: their roots are found algebraically)");
        return GFA_ERR_UNSUPPORTED;
    }
    if (batch < 0 || ncoef < 2) { set_error("gfa_poly_roots: bad arguments (batch >= 0 rows of ncoef >= 2 coefficients)"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0) return GFA_OK;
    if (!coeffs || !roots_out || !count_out) { set_error("gfa_poly_roots: bad arguments"); return GFA_ERR_INVALID; }
    if (batch > 0x7fffffff || ncoef > 0x7fffffff) { set_error("gfa_poly_roots: at most 2^31 - 1 rows of at most 2^31 - 1 coefficients"); return GFA_ERR_UNSUPPORTED; }
    if ((unsigned __int128)f->calc.q * (u64)(ncoef - 1) * (u64)batch > PR_MAX_WORK) {
        set_error("gfa_poly_roots: q (ncoef - 1) batch exceeds 2^42 evaluation steps: too many for a search over every element, find these roots algebraically");
        return GFA_ERR_UNSUPPORTED;
    }
    FieldDev fd;
    int rc = field_desc(f, &fd);
    if (rc) return rc;
    if (!fits_lds(fd, "gfa_poly_roots", ncoef, ncoef - 1)) return GFA_ERR_UNSUPPORTED;
    const hipStream_t st = (hipStream_t)stream;
    Scratch scratch(st);
    u32 *counter;
    GFA_HIP(scratch.get(&counter, (size_t)batch));
    GFA_HIP(hipMemsetAsync(counter, 0, (size_t)batch * sizeof(u32), st));
    GFA_HIP(hipMemsetAsync(roots_out, 0, ((size_t)batch * (size_t)(ncoef - 1)) << dtype, st)); // the slots; GFA_U8 .. GFA_U64 = 0 .. 3
    const RootsJob j{coeffs, batch, (int)ncoef, (int)ncoef - 1, dtype, roots_out, counter, count_out, mult_out, st};
    return for_policy(fd, dtype, "gfa_poly_roots", [&](auto p) { return launch_roots<typename decltype(p)::type>(fd, j); });
}

int gfa_poly_root_multiplicity(gfa_field_t *f, const void *coeffs, int64_t batch, int64_t ncoef, const void *roots, int64_t nroots, int32_t *mult_out, int dtype,
                               gfa_stream_t stream)
{
    if (!f) {
        set_error("gfa_poly_root_multiplicity: no field handle (fields of order >= 2^64 are not served: divide by x - r instead)");
        return GFA_ERR_UNSUPPORTED;
    }
    if (batch < 0 || ncoef < 1 || nroots < 0) { set_error("gfa_poly_root_multiplicity: bad arguments"); return GFA_ERR_INVALID; }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0 || nroots == 0) return GFA_OK;
    if (!coeffs || !roots || !mult_out) { set_error("gfa_poly_root_multiplicity: bad arguments"); return GFA_ERR_INVALID; }
    if (batch > 0x7fffffff || ncoef > 0x7fffffff || nroots > 0x7fffffff) {
        set_error("gfa_poly_root_multiplicity: at most 2^31 - 1 rows, coefficients and elements");
        return GFA_ERR_UNSUPPORTED;
    }
    FieldDev fd;
    int rc = field_desc(f, &fd);
    if (rc) return rc;
    if (!fits_lds(fd, "gfa_poly_root_multiplicity", ncoef, nroots)) return GFA_ERR_UNSUPPORTED;
    const RootsJob j{coeffs, batch, (int)ncoef, (int)nroots, dtype, const_cast<void *>(roots), nullptr, nullptr, mult_out, (hipStream_t)stream};
    return for_policy(fd, dtype, "gfa_poly_roots", [&](auto p) { return launch_roots<typename decltype(p)::type>(fd, j); });
}

} // extern "C"
