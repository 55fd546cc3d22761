// Micro-benchmark (r07): in which ORDER should the persistent workgroups of the 64 KiB-table kernel walk the arrays?
// out = TABLE[a][b] over n uint8 elements (default 1e8), GF(2^8)/0x11D product table in LDS, against the flat a ^ b launch.
// The question stream3.hip left open: its k_dyn (two barriers per block, nothing in flight across them) lost to static
// striding at 1e8, but the overlapped claim loop of the library (claim a block ahead, next loads before current stores) was
// never timed at this size, nor were non-temporal accesses.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/stream4.hip -o tools/ubench/stream4
//   tools/ubench/stream4 [n] [rounds] [launches]
//
// Protocol: ~0.1 s of untimed launches, then `rounds` (default 7) passes over the whole variant list in order -- so the
// variants are interleaved in time -- each pass timing `launches` (default 100) back-to-back launches of a variant between
// two HIP events.  Per variant: median, min and max of the per-pass averages.  A memset that a variant needs per launch is
// inside its timed region.  Every table variant's output is compared byte for byte (on the device) with variant A's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "tab8_sched.h"

typedef unsigned int u32;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef long long i64;
using gfa::Tab8Sched;

#define CK(x)                                                                                                              \
    do {                                                                                                                   \
        hipError_t e_ = (x);                                                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(2); } \
    } while (0)

template <bool NT> __device__ __forceinline__ u32x4 ld(const u32x4 *p) { if constexpr (NT) return __builtin_nontemporal_load(p); else return *p; }
template <bool NT> __device__ __forceinline__ void st(u32x4 v, u32x4 *p) { if constexpr (NT) __builtin_nontemporal_store(v, p); else *p = v; }

// R0: flat launch, one vector per thread
__global__ __launch_bounds__(256) void k_flat_xor(const u32x4 *a, const u32x4 *b, u32x4 *o, i64 nvec)
{
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < nvec) o[i] = a[i] ^ b[i];
}
// R1: grid-stride, the library's launch shape
__global__ __launch_bounds__(1024) void k_stride_xor(const u32x4 *a, const u32x4 *b, u32x4 *o, i64 nvec)
{
    const i64 stride = (i64)gridDim.x * 1024;
    for (i64 i = (i64)blockIdx.x * 1024 + threadIdx.x; i < nvec; i += stride) o[i] = a[i] ^ b[i];
}

__device__ __forceinline__ u32 lookup4(const unsigned char *lds, u32 aw, u32 bw)
{
    u32 i0 = __builtin_amdgcn_perm(aw, bw, 0x0c0c0400u);
    u32 i1 = __builtin_amdgcn_perm(aw, bw, 0x0c0c0501u);
    u32 i2 = __builtin_amdgcn_perm(aw, bw, 0x0c0c0602u);
    u32 i3 = __builtin_amdgcn_perm(aw, bw, 0x0c0c0703u);
    u32 r0 = lds[i0], r1 = lds[i1], r2 = lds[i2], r3 = lds[i3];
    return r0 | (r1 << 8) | (r2 << 16) | (r3 << 24);
}
__device__ __forceinline__ u32x4 lookup16(const unsigned char *lds, u32x4 x, u32x4 y)
{
    u32x4 r;
    r.x = lookup4(lds, x.x, y.x); r.y = lookup4(lds, x.y, y.y);
    r.z = lookup4(lds, x.z, y.z); r.w = lookup4(lds, x.w, y.w);
    return r;
}
__device__ __forceinline__ void stage_table(unsigned char *lds, const unsigned char *table)
{
    for (int t = threadIdx.x; t < 4096; t += 1024) ((uint4 *)lds)[t] = ((const uint4 *)table)[t];
}

// A / B: the r06 library kernel (static stride, one vector per thread re-armed before the lookups), with optional
// non-temporal loads / stores
template <bool NTL, bool NTS>
__global__ __launch_bounds__(1024) void k_static(const unsigned char *table, const u32x4 *av, const u32x4 *bv, u32x4 *ov, i64 nvec)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const i64 stride = (i64)gridDim.x * 1024;
    i64 i = (i64)blockIdx.x * 1024 + threadIdx.x;
    u32x4 x = {0, 0, 0, 0}, y = {0, 0, 0, 0};
    if (i < nvec) { x = ld<NTL>(av + i); y = ld<NTL>(bv + i); }
    stage_table(lds, table);
    __syncthreads();
    for (; i < nvec; i += stride) {
        const u32x4 cx = x, cy = y;
        const i64 nxt = i + stride;
        if (nxt < nvec) { x = ld<NTL>(av + nxt); y = ld<NTL>(bv + nxt); }
        st<NTS>(lookup16(lds, cx, cy), ov + i);
    }
}

// C / C' / D / E: blocks of U * 1024 vectors; blocks below s.nstatic strided statically (no atomics, next loads issued before
// the lookups), the rest claimed a block ahead (thread 0 atomicAdd -> LDS word -> barrier; next loads before current stores).
// Every loop is bounded by s.nblk and no workgroup waits on another.
// SELF_RESET: ctr[1] counts workgroups that are done; the last one out zeroes both words, so no memset per launch.
template <int U, bool NTL, bool NTS, bool SELF_RESET>
__global__ __launch_bounds__(1024) void k_sched(const unsigned char *table, const u32x4 *av, const u32x4 *bv, u32x4 *ov,
                                                 Tab8Sched s, unsigned *ctr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ unsigned s_next;
    i64 blk = blockIdx.x;
    u32x4 x[U], y[U];
    if (blk < s.nblk) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const i64 i = gfa::tab8_block_first(s, blk) + u * 1024 + threadIdx.x;
            if (i < s.nvec) { x[u] = ld<NTL>(av + i); y[u] = ld<NTL>(bv + i); }
        }
    }
    stage_table(lds, table);
    __syncthreads();
    while (blk < s.nblk) {
        const i64 base = gfa::tab8_block_first(s, blk) + threadIdx.x;
        i64 nxt;
        if (!gfa::tab8_next_is_claimed(s, blk)) {
            nxt = blk + s.grid;
            const i64 nbase = gfa::tab8_block_first(s, nxt) + threadIdx.x;
#pragma unroll
            for (int u = 0; u < U; u++) {
                const i64 i = base + u * 1024;
                if (i < s.nvec) {
                    const u32x4 cx = x[u], cy = y[u];
                    const i64 j = nbase + u * 1024;
                    if (nxt < s.nblk && j < s.nvec) { x[u] = ld<NTL>(av + j); y[u] = ld<NTL>(bv + j); }
                    st<NTS>(lookup16(lds, cx, cy), ov + i);
                }
            }
        } else {
            if (threadIdx.x == 0) s_next = atomicAdd(ctr, 1u);
            u32x4 r[U];
#pragma unroll
            for (int u = 0; u < U; u++) r[u] = lookup16(lds, x[u], y[u]);
            __syncthreads();
            nxt = gfa::tab8_claimed_block(s, s_next);
            __syncthreads();
            if (nxt < s.nblk) {
                const i64 nbase = gfa::tab8_block_first(s, nxt) + threadIdx.x;
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const i64 j = nbase + u * 1024;
                    if (j < s.nvec) { x[u] = ld<NTL>(av + j); y[u] = ld<NTL>(bv + j); }
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const i64 i = base + u * 1024;
                if (i < s.nvec) st<NTS>(r[u], ov + i);
            }
        }
        blk = nxt;
    }
    if constexpr (SELF_RESET) {
        // Thread 0 made all of this workgroup's claims and has consumed the last one's result, so they precede this increment;
        // whoever reads grid - 1 knows that every claim of the launch is done and may zero the words for the next launch.
        if (threadIdx.x == 0 && s.nstatic < s.nblk) {
            if (atomicAdd(ctr + 1, 1u) == (unsigned)s.grid - 1) { atomicExch(ctr, 0u); atomicExch(ctr + 1, 0u); }
        }
    }
}

__global__ void k_diff(const u32x4 *p, const u32x4 *q, i64 nvec, unsigned long long *cnt)
{
    unsigned long long c = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (i64)gridDim.x * blockDim.x) {
        const u32x4 d = p[i] ^ q[i];
        c += (d.x | d.y | d.z | d.w) != 0;
    }
    if (c) atomicAdd(cnt, c);
}

struct Variant {
    std::string name;
    bool table;                  // output is compared with variant A's
    std::function<void()> launch;
    std::vector<float> us;
};

int main(int argc, char **argv)
{
    const i64 n = argc > 1 ? atoll(argv[1]) : 100000000, nvec = n / 16;
    const int rounds = argc > 2 ? atoi(argv[2]) : 7, launches = argc > 3 ? atoi(argv[3]) : 100;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    u32x4 *a, *b, *o, *oref;
    CK(hipMalloc(&a, n)); CK(hipMalloc(&b, n)); CK(hipMalloc(&o, n)); CK(hipMalloc(&oref, n));
    // two counter pairs: the self-resetting variants need theirs at zero between launches, the memset variant leaves its own dirty
    unsigned *ctr, *ctr_ms;
    CK(hipMalloc(&ctr, 8)); CK(hipMemset(ctr, 0, 8));
    CK(hipMalloc(&ctr_ms, 8)); CK(hipMemset(ctr_ms, 0, 8));
    unsigned long long *dcnt;
    CK(hipMalloc(&dcnt, 8));
    unsigned char *htab = (unsigned char *)malloc(65536), *dtab;
    for (int x = 0; x < 256; x++)
        for (int y = 0; y < 256; y++) {
            unsigned r = 0, aa = x;
            for (int k = 0; k < 8; k++) { if (y >> k & 1) r ^= aa; aa <<= 1; if (aa & 0x100) aa ^= 0x11d; }
            htab[x * 256 + y] = (unsigned char)r;
        }
    CK(hipMalloc(&dtab, 65536)); CK(hipMemcpy(dtab, htab, 65536, hipMemcpyHostToDevice));
    {
        unsigned char *h = (unsigned char *)malloc(n);
        unsigned long long st = 88172645463325252ull;
        for (i64 i = 0; i < n; i++) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; h[i] = (unsigned char)(st >> 24); }
        CK(hipMemcpy(a, h, n, hipMemcpyHostToDevice));
        for (i64 i = 0; i < n; i++) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; h[i] = (unsigned char)(st >> 24); }
        CK(hipMemcpy(b, h, n, hipMemcpyHostToDevice));
        free(h);
    }

    std::vector<Variant> V;
    const unsigned flat_grid = (unsigned)((nvec + 255) / 256);
    V.push_back({"R0 flat xor 256thr", false, [=]() { hipLaunchKernelGGL(k_flat_xor, dim3(flat_grid), dim3(256), 0, 0, a, b, o, nvec); }, {}});
    V.push_back({"R1 gridstride xor 2/CU x 1024", false, [=]() { hipLaunchKernelGGL(k_stride_xor, dim3(cus * 2), dim3(1024), 0, 0, a, b, o, nvec); }, {}});
#define ADD_STATIC(NAME, NTL, NTS)                                                                                         \
    {                                                                                                                      \
        auto k = k_static<NTL, NTS>;                                                                                       \
        CK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));                       \
        const i64 blocks = (nvec + 1023) / 1024;                                                                           \
        const int g = (int)std::max<i64>(1, std::min<i64>(blocks, cus * 2));                                               \
        V.push_back({NAME, true, [=]() { hipLaunchKernelGGL(k, dim3(g), dim3(1024), 65536, 0, dtab, a, b, o, nvec); }, {}}); \
    }
    ADD_STATIC("A  static pipelined (library r06)", false, false)
    ADD_STATIC("B  A + nt loads", true, false)
    ADD_STATIC("B  A + nt stores", false, true)
    ADD_STATIC("B  A + nt loads + nt stores", true, true)
    // PER_CU workgroups per CU, U vectors per thread per block, CLAIM_ROUNDS as in tab8_sched (1 << 40: all but the first block)
#define ADD_SCHED(NAME, PER_CU, U, NT, SELF_RESET, CLAIM_ROUNDS)                                                           \
    {                                                                                                                      \
        auto k = k_sched<U, NT, NT, SELF_RESET>;                                                                           \
        CK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));                       \
        const Tab8Sched s = gfa::tab8_sched(n, cus * PER_CU, U * 1024, CLAIM_ROUNDS);                                      \
        V.push_back({NAME, true, [=]() {                                                                                   \
                         if (!SELF_RESET) (void)hipMemsetAsync(ctr_ms, 0, 8, 0);                                           \
                         hipLaunchKernelGGL(k, dim3(s.grid), dim3(1024), 65536, 0, dtab, a, b, o, s, SELF_RESET ? ctr : ctr_ms); \
                     }, {}});                                                                                              \
    }
    const i64 ALL = (i64)1 << 40;
    ADD_SCHED("C  claim 32K nt, memset per launch (library >= 2^28)", 2, 2, true, false, ALL)
    ADD_SCHED("C' claim 16K    self-reset", 2, 1, false, true, ALL)
    ADD_SCHED("C' claim 16K nt self-reset", 2, 1, true, true, ALL)
    ADD_SCHED("C' claim 32K    self-reset", 2, 2, false, true, ALL)
    ADD_SCHED("C' claim 32K nt self-reset", 2, 2, true, true, ALL)
    ADD_SCHED("C' claim 64K    self-reset", 2, 4, false, true, ALL)
    ADD_SCHED("C' claim 64K nt self-reset", 2, 4, true, true, ALL)
    ADD_SCHED("D  static, last 2 rounds claimed 16K    self-reset", 2, 1, false, true, 2)
    ADD_SCHED("D  static, last 2 rounds claimed 16K nt self-reset", 2, 1, true, true, 2)
    ADD_SCHED("D4 static, last 4 rounds claimed 16K    self-reset", 2, 1, false, true, 4)
    ADD_SCHED("S  k_sched all static 16K (A through the schedule)", 2, 1, false, true, 0)
    ADD_SCHED("E  1/CU claim 32K    self-reset", 1, 2, false, true, ALL)
    ADD_SCHED("E  1/CU claim 32K nt self-reset", 1, 2, true, true, ALL)
    ADD_SCHED("E  1/CU static, last 2 rounds claimed 32K    self-reset", 1, 2, false, true, 2)
    ADD_SCHED("E  1/CU static, last 2 rounds claimed 32K nt self-reset", 1, 2, true, true, 2)

    // correctness first: every table variant against A, one launch each (also the first warm-up)
    int bad_variants = 0;
    for (size_t v = 0; v < V.size(); v++) {
        if (!V[v].table) continue;
        CK(hipMemset(o, 0xA5, n));
        V[v].launch();
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        if (V[v].name[0] == 'A') { CK(hipMemcpy(oref, o, n, hipMemcpyDeviceToDevice)); continue; }
        CK(hipMemset(dcnt, 0, 8));
        hipLaunchKernelGGL(k_diff, dim3(1024), dim3(256), 0, 0, o, oref, nvec, dcnt);
        unsigned long long c = 0;
        CK(hipMemcpy(&c, dcnt, 8, hipMemcpyDeviceToHost));
        if (c) { printf("MISMATCH %-60s %llu vectors differ from A\n", V[v].name.c_str(), c); bad_variants++; }
    }
    {
        unsigned h[2] = {1, 1};
        CK(hipMemcpy(h, ctr, 8, hipMemcpyDeviceToHost));
        if (h[0] || h[1]) { printf("counter not back at zero after the self-resetting variants: %u %u\n", h[0], h[1]); bad_variants++; }
    }
    {   // spot check of A against the host table
        std::vector<unsigned char> ha(4096), hb(4096), ho(4096);
        CK(hipMemcpy(ha.data(), a, 4096, hipMemcpyDeviceToHost)); CK(hipMemcpy(hb.data(), b, 4096, hipMemcpyDeviceToHost));
        CK(hipMemcpy(ho.data(), oref, 4096, hipMemcpyDeviceToHost));
        for (int i = 0; i < 4096 && i < n / 16 * 16; i++)
            if (ho[i] != htab[ha[i] * 256 + hb[i]]) { printf("A differs from the host table at %d\n", i); bad_variants++; break; }
    }
    printf("n = %lld, %d CUs, %d rounds x %d launches; table variants that differ from A: %d\n", n, cus, rounds, launches, bad_variants);
    if (bad_variants) return 1;

    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    {   // ~0.1 s of untimed load so that the clocks are up
        float total = 0.f;
        while (total < 100.f) {
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < 200; i++) V[2].launch();
            CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            total += ms;
        }
    }
    for (int r = 0; r < rounds; r++)
        for (auto &v : V) {
            for (int i = 0; i < 3; i++) v.launch();
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < launches; i++) v.launch();
            CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            v.us.push_back(ms * 1e3f / launches);
        }
    CK(hipGetLastError());
    printf("%-62s %9s %9s %9s %8s\n", "variant (3 n bytes moved)", "median us", "min us", "max us", "TB/s");
    for (auto &v : V) {
        std::sort(v.us.begin(), v.us.end());
        const float med = v.us[v.us.size() / 2];
        printf("%-62s %9.2f %9.2f %9.2f %8.3f\n", v.name.c_str(), med, v.us.front(), v.us.back(), 3.0 * n / med / 1e6);
    }
    return 0;
}
