// gfa_lagrange.hip -- Lagrange interpolation over GF(q), q < 2^64, of a stack of point sets.
//
//   gfa_poly_lagrange ... replaces lagrange_poly_jit (a doubly nested loop of polynomial products on one core,
//                         _polys/_lagrange.py:118-133) for `batch` rows of `npts` points at once
//
// lg_kernel   one launch, no work buffer, no atomics.  A row is worked by a TEAM of lanes (gfa_lagrange.h: weights, duplicate
//             flag, npts sweeps) and a workgroup carries blockDim.x / team rows side by side, so that the short rows this is
//             mostly for (Shamir shares, k = 3 .. 32) fill its wavefronts:
//               npts <= LG_PACK_THREADS   team = the power of two >= npts, workgroup = LG_PACK_THREADS threads (fewer when the
//                                         whole batch needs fewer), rows per workgroup = threads / team; the last workgroup is
//                                         partly filled and its spare teams only keep the barriers
//               above                     one row per workgroup of min(1024, npts rounded up to 64) threads, which stride over
//                                         the coefficients when npts is larger still
//             Every row of a launch has the same npts, so the number of barriers (npts + 2) is the same for every thread and
//             the barriers are workgroup-wide.  x is read per row, or from row 0 for every row (x_rows == 1).
//
// LDS, per row a workgroup carries, in elements of the field policy (32 bits for Prime32 and Lut, 64 bits otherwise):
//   x[npts] c[npts] a[2][npts] m[2][npts] dup                 6 npts + 1 elements
// of 150 KiB for the workgroup.  One row must fit, so
//   npts <= LG_MAX_POINTS(sizeof element) = (150 KiB / sizeof element - 1) / 6 = 6399 / 3199;
// above it the entry point returns GFA_ERR_UNSUPPORTED and the caller runs the same weights and sweeps on whole arrays
// (galois_amd/_lagrange.py).
#include <algorithm>

#include "gfa_poly_launch.h"
#include "gfa_lagrange.h"

using namespace gfa;
using namespace gfa::polykit;

namespace {

constexpr int LG_THREADS = 1024;
// rows of up to this many points share a workgroup of this many threads (tools/bench_lagrange.py)
constexpr int LG_PACK_THREADS = 256;
// This kernel's own limits, tighter than polykit::MaxThreads: it also inverts.  The digit-vector products and the inversion of
// GF(p^M) fit 128 registers up to M = 7, 256 up to M = 14
template <class F>
struct LgThreads {
    static constexpr int most = LG_THREADS;
};
template <int M>
struct LgThreads<ExtP<M>> {
    static constexpr int most = M >= 15 ? LG_THREADS / 4 : M >= 8 ? LG_THREADS / 2 : LG_THREADS;
};
constexpr size_t LG_LDS_BYTES = 150 * 1024;
constexpr i64 LG_MAX_POINTS(size_t elem) { return (i64)((LG_LDS_BYTES / elem - 1) / lagrange::LG_ARRAYS); }

int lg_pack_threads = LG_PACK_THREADS; // gfa_debug_lagrange_tune

template <class F>
__global__ __launch_bounds__(LgThreads<F>::most) void lg_kernel(FieldDev fd, const void *__restrict__ x, const void *__restrict__ y, i64 batch, int npts, int x_shared,
                                                                 int team, void *__restrict__ coeffs_out, int32_t *__restrict__ status_out, int dtype)
{
    typedef typename F::elem E;
    extern __shared__ u64 lg_lds[];
    const int slot = (int)threadIdx.x / team; // the workgroup's rows: slot < blockDim.x / team
    const Team g{(int)threadIdx.x % team, team};
    const i64 row = (i64)blockIdx.x * ((int)blockDim.x / team) + slot;
    const bool live = row < batch;
    const lagrange::Row<E> r = lagrange::carve((E *)lg_lds + (size_t)slot * ((size_t)lagrange::LG_ARRAYS * npts + 1), npts);
    const RowLoad xs{x, dtype, x_shared || !live ? 0 : row * npts}, ys{y, dtype, live ? row * npts : 0};
    const RowStore out{coeffs_out, dtype, live ? row * npts : 0};
    const bool dup = lagrange::row<F, RowLoad, RowLoad, RowStore, Team>(fd, r, npts, xs, ys, out, live, g);
    if (live && g.tid == 0) status_out[row] = dup ? 1 : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct LagrangeJob {
    const void *x, *y;
    i64 batch;
    int npts, x_shared, dtype;
    void *coeffs;
    int32_t *status;
    hipStream_t st;
};

template <class F>
int launch_lagrange(const FieldDev &fd, const LagrangeJob &j)
{
    typedef typename F::elem E;
    const int most = LgThreads<F>::most, pack = std::min(lg_pack_threads, most);
    int team, threads;
    if (j.npts <= pack) {
        team = 1;
        while (team < j.npts) team *= 2;
        threads = (int)std::min<i64>(pack, (j.batch * team + 63) / 64 * 64); // a small batch does not need the whole workgroup
        threads = std::max(threads, team);
    } else {
        team = threads = wave_threads(j.npts, most);
    }
    const int rows = threads / team;
    const size_t lds = (size_t)rows * ((size_t)lagrange::LG_ARRAYS * j.npts + 1) * sizeof(E);
    const int rc = allow_large_lds<lg_kernel<F>>(LG_LDS_BYTES);
    if (rc) return rc;
    const i64 groups = (j.batch + rows - 1) / rows;
    hipLaunchKernelGGL((lg_kernel<F>), dim3((unsigned)groups), dim3(threads), lds, j.st, fd, j.x, j.y, j.batch, j.npts, j.x_shared, team, j.coeffs, j.status, j.dtype);
    GFA_HIP(hipGetLastError());
    return GFA_OK;
}

} // namespace

extern "C" {

int gfa_poly_lagrange(gfa_field_t *f, const void *x, const void *y, int64_t batch, int64_t npts, int64_t x_rows, void *coeffs_out, int32_t *status_out, int dtype,
                      gfa_stream_t stream)
{
    if (!f) { // fields of order >= 2^64 have no gfa_field_t
        set_error("gfa_poly_lagrange: no field handle (fields of order >= 2^64 are not served: interpolate on whole arrays)");
        return GFA_ERR_UNSUPPORTED;
    }
    if (batch < 0 || npts < 1 || !(x_rows == 1 || x_rows == batch)) {
        set_error("gfa_poly_lagrange: bad arguments (batch >= 0 rows of npts >= 1 points; x_rows is batch, or 1 for shared abscissae)");
        return GFA_ERR_INVALID;
    }
    if (!dtype_holds(dtype, f->calc.q)) { set_error("dtype cannot hold the field's elements"); return GFA_ERR_INVALID; }
    if (batch == 0) return GFA_OK;
    if (!x || !y || !coeffs_out || !status_out) { set_error("gfa_poly_lagrange: bad arguments"); return GFA_ERR_INVALID; }
    if (batch > 0x7fffffff) { set_error("gfa_poly_lagrange: at most 2^31 - 1 rows"); return GFA_ERR_UNSUPPORTED; }
    FieldDev fd;
    const int rc = field_desc(f, &fd);
    if (rc) return rc;
    const i64 cap = LG_MAX_POINTS(elem_bytes(fd));
    if (npts > cap) {
        set_error("gfa_poly_lagrange: npts = " + std::to_string(npts) + ", the kernel holds a row's points, weights and two pairs of polynomials in LDS up to npts = " +
                  std::to_string(cap) + " over this field");
        return GFA_ERR_UNSUPPORTED;
    }
    const LagrangeJob j{x, y, batch, (int)npts, x_rows == 1 && batch > 1 ? 1 : 0, dtype, coeffs_out, status_out, (hipStream_t)stream};
    return for_policy(fd, dtype, "gfa_poly_lagrange", [&](auto p) { return launch_lagrange<typename decltype(p)::type>(fd, j); });
}

void gfa_debug_lagrange_tune(int pack_threads)
{
    const bool ok = pack_threads >= 64 && pack_threads <= LG_THREADS && (pack_threads & (pack_threads - 1)) == 0;
    lg_pack_threads = ok ? pack_threads : LG_PACK_THREADS;
}

} // extern "C"
