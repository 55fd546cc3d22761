// gfa_polygcd.hip -- greatest common divisors of a stack of polynomial pairs over GF(q), q < 2^64: the whole Euclidean remainder
// sequence of a pair in ONE launch, one workgroup per pair.
//
//   gfa_poly_gcd ... replaces gcd / egcd (_polys/_functions.py:10-57), whose loop is one remainder (a launch and a read-back of
//                    `r1 != 0`) per step, for `batch` pairs (a_k, b_k) or (a_k, b)
//
// Every step is polydiv::divide (gfa_polydiv.h: blocked triangle + tail) on Lin views of the two running remainders, which stay
// in LDS from the load to the normalised result (gfa_polygcd.h).  Nothing is read back between the steps; rows with different
// true degrees simply run different numbers of steps, so the control flow is uniform within a workgroup only.
//
// LDS (elements of the field policy: 32 bits for Prime32 and Lut, 64 bits otherwise):
//   plain     ra[na] rb[nb]                                   na + nb      elements
//   extended  ra[na] rb[nb] s2[nb] s1[nb] t2[na] t1[na]       3 (na + nb)  elements
// plus one word for the workgroup reduction, of the 150 KiB gfa_poly_powmod also asks for (PG_LDS_BYTES - 8 bytes hold them):
//   na + nb <= PG_MAX_TERMS(sizeof element, extended) = (150 KiB - 8) / sizeof element / (extended ? 3 : 1)
//            = 38398 / 12799 (32-bit elements),  19199 / 6399 (64-bit elements);
// above it the entry point returns GFA_ERR_UNSUPPORTED and the caller runs Euclid over gfa_poly_divmod (galois_amd/_polygcd.py).
//
// Threads follow the independent work of a step, rounded to whole waves: min(na, nb) tail coefficients of a division, and with
// cofactors max(na, nb) product coefficients -- a pair of degree <= 63 is one wave, so many pairs share a compute unit.
#include <algorithm>

#include "gfa_poly_launch.h"
#include "gfa_polygcd.h"

using namespace gfa;
using namespace gfa::polydiv;
using namespace gfa::polykit;

namespace {

constexpr size_t PG_LDS_BYTES = 150 * 1024;
constexpr size_t PG_SLOT_BYTES = 8; // the reduction word, in front of the coefficients (keeps 64-bit elements aligned)

constexpr i64 PG_MAX_TERMS(size_t elem, bool extended) { return (i64)((PG_LDS_BYTES - PG_SLOT_BYTES) / elem / (extended ? 3 : 1)); }
constexpr size_t lds_bytes(i64 terms, size_t elem, bool extended) { return PG_SLOT_BYTES + (size_t)terms * (extended ? 3 : 1) * elem; }
static_assert(lds_bytes(PG_MAX_TERMS(4, false), 4, false) <= PG_LDS_BYTES && lds_bytes(PG_MAX_TERMS(8, true), 8, true) <= PG_LDS_BYTES, "cap");

} // namespace

namespace gfa {
namespace polygcd {
// minimum over the workgroup: within each wave by shuffles, across the waves by one LDS atomic each.  The three barriers order
// the reset, the atomics, and the last read before the next reset.
template <>
struct GroupMin<Team> {
    static __device__ __forceinline__ int run(const Team &g, int v, int *slot)
    {
        for (int d = 32; d >= 1; d >>= 1) {
            const int o = __shfl_xor(v, d, 64);
            v = o < v ? o : v;
        }
        if (g.tid == 0) *slot = v; // the first wave's
        g.sync();
        if ((g.tid & 63) == 0 && g.tid != 0) atomicMin(slot, v);
        g.sync();
        const int r = *slot;
        g.sync();
        return r;
    }
};
} // namespace polygcd
} // namespace gfa

namespace {

// g, s, t: (batch, n) with n = max(na, nb), right-aligned; s, t and deg may be null (s and t together)
template <class F>
__global__ __launch_bounds__(MaxThreads<F>::most) void pg_gcd_kernel(FieldDev fd, const void *__restrict__ a, int na, const void *__restrict__ b, int b_shared, int nb,
                                                               void *__restrict__ g_out, void *__restrict__ s_out, void *__restrict__ t_out,
                                                               int32_t *__restrict__ deg_out, int dtype)
{
    typedef typename F::elem E;
    extern __shared__ u64 pg_lds[];
    int *slot = (int *)pg_lds;
    E *ra = (E *)(pg_lds + 1), *rb = ra + na;
    const bool extended = s_out != nullptr;
    E *s2 = rb + nb, *s1 = s2 + nb, *t2 = s1 + nb, *t1 = t2 + na; // inside the allocation only when extended
    const Team g{(int)threadIdx.x, (int)blockDim.x};
    const i64 row = blockIdx.x;
    const int n = na > nb ? na : nb;
    for (int i = g.tid; i < na; i += g.n) ra[i] = (E)load_coeff(a, dtype, row * na + i);
    for (int i = g.tid; i < nb; i += g.n) rb[i] = (E)load_coeff(b, dtype, (b_shared ? 0 : row * nb) + i);
    const polygcd::Result<E> res = polygcd::euclid<F, Team>(fd, ra, na, rb, nb, s2, s1, t2, t1, extended, slot, g);
    for (int i = g.tid; i < n; i += g.n) { // column i holds the coefficient of x^(n - 1 - i)
        const int j = n - 1 - i;
        store_coeff(g_out, dtype, row * n + i, j < res.len ? (u64)res.r[res.len - 1 - j] : 0);
        if (extended) {
            store_coeff(s_out, dtype, row * n + i, j < res.ls ? (u64)res.s[nb - 1 - j] : 0);
            store_coeff(t_out, dtype, row * n + i, j < res.lt ? (u64)res.t[na - 1 - j] : 0);
        }
    }
    if (deg_out && g.tid == 0) deg_out[row] = res.len - 1;
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct GcdJob {
    const void *a, *b;
    i64 batch;
    int na, nb, b_shared, dtype;
    void *g, *s, *t;
    int32_t *deg;
    hipStream_t st;
};

template <class F>
int launch_gcd(const FieldDev &fd, const GcdJob &j)
{
    typedef typename F::elem E;
    const bool extended = j.s != nullptr;
    const i64 terms = (i64)j.na + j.nb, cap = PG_MAX_TERMS(sizeof(E), extended);
    if (terms > cap) {
        set_error("gfa_poly_gcd: na + nb = " + std::to_string(terms) + ", the kernel holds the remainders" + (extended ? " and cofactors" : "") +
                  " in LDS up to na + nb = " + std::to_string(cap) + " over this field");
        return GFA_ERR_UNSUPPORTED;
    }
    const int rc = allow_large_lds<pg_gcd_kernel<F>>(PG_LDS_BYTES);
    if (rc) return rc;
    const int threads = wave_threads(extended ? std::max(j.na, j.nb) : std::min(j.na, j.nb), MaxThreads<F>::most);
    hipLaunchKernelGGL((pg_gcd_kernel<F>), dim3((unsigned)j.batch), dim3(threads), lds_bytes(terms, sizeof(E), extended), j.st, fd, j.a, j.na, j.b, j.b_shared, j.nb, j.g, j.s, j.t,
                       j.deg, j.dtype);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

} // namespace

extern "C" {

int gfa_poly_gcd(gfa_field_t *f, const void *a, int64_t batch, int64_t na, const void *b, int64_t b_rows, int64_t nb, void *g_out, void *s_out, void *t_out,
                 int32_t *deg_out, int dtype, gfa_stream_t stream)
{
    if (!f) { // fields of order >= 2^64 have no gfa_field_t
        set_error("gfa_poly_gcd: no field handle (fields of order >= 2^64 are not served: run Euclid over their own division)");
        return GFA_ERR_UNSUPPORTED;
    }
    if (batch < 0 || na < 1 || nb < 1 || (b_rows != 1 && b_rows != batch) || (s_out == nullptr) != (t_out == nullptr)) {
        set_error("gfa_poly_gcd: bad arguments (b_rows is 1 or batch; s_out and t_out are given together)");
        return GFA_ERR_INVALID;
    }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0) return GFA_OK;
    if (!a || !b || !g_out) { set_error("gfa_poly_gcd: bad arguments"); return GFA_ERR_INVALID; }
    if (batch > 0x7fffffff || na > 0x3fffffff || nb > 0x3fffffff) { set_error("gfa_poly_gcd: at most 2^31 - 1 rows of at most 2^30 - 1 coefficients"); return GFA_ERR_UNSUPPORTED; }
    FieldDev fd;
    int rc = field_desc(f, &fd);
    if (rc) return rc;
    const GcdJob j{a, b, batch, (int)na, (int)nb, b_rows == 1 ? 1 : 0, dtype, g_out, s_out, t_out, deg_out, (hipStream_t)stream};
    return for_policy(fd, dtype, "gfa_poly_gcd", [&](auto p) { return launch_gcd<typename decltype(p)::type>(fd, j); });
}

} // extern "C"
