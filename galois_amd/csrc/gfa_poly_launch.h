// gfa_poly_launch.h -- the launch toolkit of the batched polynomial kernel files (gfa_polytest.hip, gfa_polyelem.hip, gfa_polydiv.hip,
// gfa_polygcd.hip, gfa_polyroots.hip, gfa_lagrange.hip, gfa_lfsr.hip): what stands between a __host__ __device__ algorithm header
// (gfa_polydiv.h, gfa_polygcd.h, ...) and an extern "C" entry point, and is the same for every file of the family.
//
//   device   load_coeff / store_coeff / load_elem, the row views RowLoad / RowStore over them, and Team, the workgroup
//   host     MaxThreads, wave_threads, elem_bytes, field_desc, for_policy, allow_large_lds
//
// HIP only: included by .hip files, never by an algorithm header (those are also compiled by a host compiler in tests/csrc).
// A kernel file of this family keeps its constants and LDS caps, its kernels, its Job structs, its launch_x<F> functions and its
// entry points with their argument checks.
#pragma once
#include <algorithm>

#include "gfa_internal.h"
#include "gfa_polytest.h"

namespace gfa {
namespace polykit {

using gfa::polytest::ExtP;

// ---- storage -----------------------------------------------------------------------------------------------------------
// The element type of a kernel is the field policy's (32 bits for Prime32 and Lut, 64 bits otherwise) whatever the storage type,
// which is read and written through a switch that is uniform over the launch -- so the kernels are instantiated per policy only.
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

// load_coeff where a value that is no field element reads as 0, so that table-driven arithmetic stays inside its tables
// whatever the buffers hold
__device__ __forceinline__ u64 load_elem(const void *p, int dtype, i64 i, u64 q)
{
    const u64 v = load_coeff(p, dtype, i);
    return v < q ? v : 0;
}

// elements base + i of an array in the caller's storage
struct RowLoad {
    const void *p;
    int dtype;
    i64 base;
    __device__ __forceinline__ u64 operator[](int i) const { return load_coeff(p, dtype, base + i); }
};
struct RowStore {
    void *p;
    int dtype;
    i64 base;
    __device__ __forceinline__ void set(int i, u64 v) const { store_coeff(p, dtype, base + i, v); }
};

// ---- the workgroup -----------------------------------------------------------------------------------------------------
// The lanes that work one row: a whole workgroup, or a slice of one whose rows all keep the same barriers.  polydiv::triangle()
// runs on the first wave, whose lanes order their LDS and global accesses among themselves with wave_sync().
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

// threads of a workgroup at most: 1024, but 512 for the digit-vector products of GF(p^M), M >= 11, which need more than the 128
// registers a 1024-thread workgroup leaves each lane (they would spill to scratch memory)
template <class F>
struct MaxThreads {
    static constexpr int most = 1024;
};
template <int M>
struct MaxThreads<ExtP<M>> {
    static constexpr int most = M >= 11 ? 512 : 1024;
};

// a launch takes as many whole waves as it has independent items of work, up to `most` threads
inline int wave_threads(int work, int most) { return std::min((std::max(work, 1) + 63) / 64 * 64, most); }

// ---- host --------------------------------------------------------------------------------------------------------------
// size of an element of the field policy the descriptor dispatches to (F::elem)
inline size_t elem_bytes(const FieldDev &fd) { return fd.kind == KIND_PRIME32 || fd.kind == KIND_LUT ? 4 : 8; }

// the descriptor to launch with on the current device: the lookup tables (uploaded on first use) or explicit calculation
inline int field_desc(gfa_field_t *f, FieldDev *fd)
{
    FieldDeviceState *ds;
    const int rc = f->ensure_device(nullptr, &ds);
    if (rc) return rc;
    *fd = f->use_lookup() ? f->lut_desc(*ds) : f->calc;
    return GFA_OK;
}

// what for_policy hands to its callee: the field policy as a type
template <class F>
struct Policy {
    typedef F type;
};

template <int M, class Fn>
int for_ext_degree(const FieldDev &fd, const char *who, Fn &&fn)
{
    if constexpr (M > GFA_MAX_EXT_DEGREE) {
        set_error(std::string(who) + ": unsupported extension degree");
        return GFA_ERR_UNSUPPORTED;
    } else {
        if ((int)fd.m == M) return fn(Policy<ExtP<M>>());
        return for_ext_degree<M + 1>(fd, who, fn);
    }
}

// fn(Policy<F>()) for the policy F the descriptor asks for: Prime32, Lut, Bin, Prime64, Goldilocks, or ExtP<M> of the descriptor's
// degree, M = 2 .. GFA_MAX_EXT_DEGREE.  The kernels read storage through load_coeff, so the storage type selects nothing; the
// entry points have checked it with dtype_holds, which leaves the 64-bit-only kinds asked with a narrower one to refuse here.
template <class Fn>
int for_policy(const FieldDev &fd, int dtype, const char *who, Fn &&fn)
{
    switch (fd.kind) {
    case KIND_PRIME32: return fn(Policy<Prime32>());
    case KIND_LUT: return fn(Policy<Lut>());
    case KIND_BIN: return fn(Policy<Bin>());
    case KIND_EXT: return for_ext_degree<2>(fd, who, fn);
    case KIND_PRIME64:
        if (dtype == GFA_U64) return fn(Policy<Prime64>());
        break;
    case KIND_GOLDILOCKS:
        if (dtype == GFA_U64) return fn(Policy<Goldilocks>());
        break;
    }
    set_error("unsupported (field kind, dtype) combination");
    return GFA_ERR_UNSUPPORTED;
}

// Lets `Kernel` be launched with up to `bytes` of dynamic LDS (more than the 64 KiB a kernel gets unasked).  Asked once per
// process and kernel instantiation, whatever device was current then: the flag takes no account of the device.  Whether that
// matters has not been measured; the flag lives here alone, so keying it by device is a change to this function only.
template <auto Kernel>
int allow_large_lds(size_t bytes)
{
    static bool done = false;
    if (!done) {
        GFA_HIP(hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        done = true;
    }
    return GFA_OK;
}

} // namespace polykit
} // namespace gfa
