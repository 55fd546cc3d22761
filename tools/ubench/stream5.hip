// Micro-benchmark (r08): what is left between the 64 KiB-table kernel and the device copy rate once walk order, claimed blocks
// and non-temporal accesses are settled (stream4.hip, r07)?  The PROLOGUE: the table copy loop of the r07 kernel is not unrolled,
// so a workgroup pays four dependent L2 round trips before its barrier with no HBM request in flight after the first.
// out = TABLE[a][b] over n uint8 elements, GF(2^8)/0x11D product table in LDS.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/stream5.hip -o tools/ubench/stream5      (from the repository root)
//   tools/ubench/stream5 [n] [nt stores: 1 | 0] [rounds] [launches]
//
// Rows:
//   A      the r07 library kernel: static striding, two workgroups per CU, prologue as it was (one load, one wait, one write, x4)
//   P      A with the table staged by stage_table_lds (gfa_internal.h, included): four loads issued together, then four writes
//   P1     P with ONE workgroup per CU and two operand vector pairs per lane and round: the same bytes in flight per CU, half the
//          waves to launch, half the table bytes staged per launch
//   P2     P at two workgroups per CU with the loads TWO rounds ahead (128 KiB instead of 64 KiB of loads in flight per CU)
//   R1     a ^ b in the library's launch shape: the floor for a table-free kernel of this shape
//   copy2  a 16-byte copy of 1.5 n bytes in the same launch shape (one stream in, one out: the same 3 n bytes cross the memory system)
// The table rows and R1 store non-temporally when the second argument is 1 (the library does from 2^26 elements).
//
// Protocol (stream4.hip's): ~0.1 s of untimed launches, then `rounds` (default 7) passes over the whole variant list in order -- so
// the variants are interleaved in time -- each pass timing `launches` (default 100) back-to-back launches of a variant between
// two HIP events.  Per variant: median, min and max of the per-pass averages.  Every table variant's output is compared byte for
// byte (on the device) with variant A's.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "../../galois_amd/csrc/gfa_internal.h" // stage_table_lds: the library's own helper, not a copy

using gfa::stage_table_lds;
typedef unsigned int u32;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef long long i64;

#define CK(x)                                                                                                              \
    do {                                                                                                                   \
        hipError_t e_ = (x);                                                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(2); } \
    } while (0)

template <bool NT> __device__ __forceinline__ void st(u32x4 v, u32x4 *p) { if constexpr (NT) __builtin_nontemporal_store(v, p); else *p = v; }

template <bool NTS>
__global__ __launch_bounds__(1024) void k_stride_xor(const u32x4 *a, const u32x4 *b, u32x4 *o, i64 nvec)
{
    const i64 stride = (i64)gridDim.x * 1024;
    for (i64 i = (i64)blockIdx.x * 1024 + threadIdx.x; i < nvec; i += stride) st<NTS>(a[i] ^ b[i], o + i);
}
template <bool NTS>
__global__ __launch_bounds__(1024) void k_stride_copy(const u32x4 *a, u32x4 *o, i64 nvec)
{
    const i64 stride = (i64)gridDim.x * 1024;
    for (i64 i = (i64)blockIdx.x * 1024 + threadIdx.x; i < nvec; i += stride) st<NTS>(a[i], o + i);
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
// the r07 prologue
__device__ __forceinline__ void stage_r07(unsigned char *lds, const unsigned char *table)
{
    for (int t = threadIdx.x; t < 4096; t += 1024) ((uint4 *)lds)[t] = ((const uint4 *)table)[t];
}
// A / P: static stride, one vector pair per lane re-armed before the lookups
template <bool NEW_STAGING, bool NTS>
__global__ __launch_bounds__(1024) void k_static(const unsigned char *table, const u32x4 *av, const u32x4 *bv, u32x4 *ov, i64 nvec)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const i64 stride = (i64)gridDim.x * 1024;
    i64 i = (i64)blockIdx.x * 1024 + threadIdx.x;
    u32x4 x = {0, 0, 0, 0}, y = {0, 0, 0, 0};
    if (i < nvec) { x = av[i]; y = bv[i]; }
    if constexpr (NEW_STAGING) stage_table_lds<1024>(lds, table, 4096);
    else stage_r07(lds, table);
    __syncthreads();
    for (; i < nvec; i += stride) {
        const u32x4 cx = x, cy = y;
        const i64 nxt = i + stride;
        if (nxt < nvec) { x = av[nxt]; y = bv[nxt]; }
        st<NTS>(lookup16(lds, cx, cy), ov + i);
    }
}

// P1: one workgroup per CU, two vector pairs per lane and round (vectors i and i + 1024 of a 2048-vector block)
template <bool NTS>
__global__ __launch_bounds__(1024) void k_p1(const unsigned char *table, const u32x4 *av, const u32x4 *bv, u32x4 *ov, i64 nvec)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const i64 stride = (i64)gridDim.x * 2048;
    i64 i = (i64)blockIdx.x * 2048 + threadIdx.x;
    u32x4 x0 = {0, 0, 0, 0}, y0 = {0, 0, 0, 0}, x1 = {0, 0, 0, 0}, y1 = {0, 0, 0, 0};
    if (i < nvec) { x0 = av[i]; y0 = bv[i]; }
    if (i + 1024 < nvec) { x1 = av[i + 1024]; y1 = bv[i + 1024]; }
    stage_table_lds<1024>(lds, table, 4096);
    __syncthreads();
    for (; i < nvec; i += stride) {
        const u32x4 cx0 = x0, cy0 = y0, cx1 = x1, cy1 = y1;
        const i64 nxt = i + stride;
        if (nxt < nvec) { x0 = av[nxt]; y0 = bv[nxt]; }
        if (nxt + 1024 < nvec) { x1 = av[nxt + 1024]; y1 = bv[nxt + 1024]; }
        st<NTS>(lookup16(lds, cx0, cy0), ov + i);
        if (i + 1024 < nvec) st<NTS>(lookup16(lds, cx1, cy1), ov + i + 1024);
    }
}

// P2: two workgroups per CU, loads two rounds ahead (registers 0 carry the even rounds, registers 1 the odd ones)
template <bool NTS>
__global__ __launch_bounds__(1024) void k_p2(const unsigned char *table, const u32x4 *av, const u32x4 *bv, u32x4 *ov, i64 nvec)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const i64 stride = (i64)gridDim.x * 1024;
    i64 i = (i64)blockIdx.x * 1024 + threadIdx.x;
    u32x4 x0 = {0, 0, 0, 0}, y0 = {0, 0, 0, 0}, x1 = {0, 0, 0, 0}, y1 = {0, 0, 0, 0};
    if (i < nvec) { x0 = av[i]; y0 = bv[i]; }
    if (i + stride < nvec) { x1 = av[i + stride]; y1 = bv[i + stride]; }
    stage_table_lds<1024>(lds, table, 4096);
    __syncthreads();
    for (; i < nvec; i += 2 * stride) {
        {
            const u32x4 cx = x0, cy = y0;
            const i64 nxt = i + 2 * stride;
            if (nxt < nvec) { x0 = av[nxt]; y0 = bv[nxt]; }
            st<NTS>(lookup16(lds, cx, cy), ov + i);
        }
        const i64 i1 = i + stride;
        if (i1 < nvec) {
            const u32x4 cx = x1, cy = y1;
            const i64 nxt = i1 + 2 * stride;
            if (nxt < nvec) { x1 = av[nxt]; y1 = bv[nxt]; }
            st<NTS>(lookup16(lds, cx, cy), ov + i1);
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

template <bool NTS>
static void add_variants(std::vector<Variant> &V, int cus, const unsigned char *dtab, const u32x4 *a, const u32x4 *b, u32x4 *o,
                         i64 nvec, const u32x4 *csrc, u32x4 *cdst, i64 cvec)
{
    const i64 blocks = (nvec + 1023) / 1024;
    const int g2 = (int)std::max<i64>(1, std::min<i64>(blocks, (i64)cus * 2));          // the library's tab8_grid
    const int g1 = (int)std::max<i64>(1, std::min<i64>((nvec + 2047) / 2048, (i64)cus)); // P1
    auto kA = k_static<false, NTS>;
    auto kP = k_static<true, NTS>;
    auto kP1 = k_p1<NTS>;
    auto kP2 = k_p2<NTS>;
    // P1 asks for 96 KiB of LDS (it uses the first 64) so that no CU can take two of its workgroups and leave another CU idle
    const int lds1 = 96 * 1024;
    CK(hipFuncSetAttribute((const void *)kA, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    CK(hipFuncSetAttribute((const void *)kP, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    CK(hipFuncSetAttribute((const void *)kP1, hipFuncAttributeMaxDynamicSharedMemorySize, lds1));
    CK(hipFuncSetAttribute((const void *)kP2, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    V.push_back({"A  static, r07 prologue (parent library)", true, [=]() { hipLaunchKernelGGL(kA, dim3(g2), dim3(1024), 65536, 0, dtab, a, b, o, nvec); }, {}});
    V.push_back({"P  A + batched staging", true, [=]() { hipLaunchKernelGGL(kP, dim3(g2), dim3(1024), 65536, 0, dtab, a, b, o, nvec); }, {}});
    V.push_back({"P1 P, 1 workgroup/CU x 2 vector pairs per lane", true, [=]() { hipLaunchKernelGGL(kP1, dim3(g1), dim3(1024), lds1, 0, dtab, a, b, o, nvec); }, {}});
    V.push_back({"P2 P, 2 workgroups/CU, loads two rounds ahead", true, [=]() { hipLaunchKernelGGL(kP2, dim3(g2), dim3(1024), 65536, 0, dtab, a, b, o, nvec); }, {}});
    V.push_back({"R1 a ^ b, 2/CU x 1024", false, [=]() { hipLaunchKernelGGL(k_stride_xor<NTS>, dim3(g2), dim3(1024), 0, 0, a, b, o, nvec); }, {}});
    const int gc = (int)std::max<i64>(1, std::min<i64>((cvec + 1023) / 1024, (i64)cus * 2));
    V.push_back({"copy2 1.5 n bytes in, 1.5 n out, 2/CU x 1024", false, [=]() { hipLaunchKernelGGL(k_stride_copy<NTS>, dim3(gc), dim3(1024), 0, 0, csrc, cdst, cvec); }, {}});
}

int main(int argc, char **argv)
{
    const i64 n = argc > 1 ? atoll(argv[1]) : 100000000, nvec = n / 16;
    const bool nts = argc > 2 ? atoi(argv[2]) != 0 : true;
    const int rounds = argc > 3 ? atoi(argv[3]) : 7, launches = argc > 4 ? atoi(argv[4]) : 100;
    if (n < 16) { fprintf(stderr, "n must be at least 16\n"); return 2; }
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const i64 cvec = 3 * nvec / 2; // vectors of the copy: 1.5 n bytes in, 1.5 n bytes out
    u32x4 *a, *b, *o, *oref, *csrc, *cdst;
    CK(hipMalloc(&a, n)); CK(hipMalloc(&b, n)); CK(hipMalloc(&o, n)); CK(hipMalloc(&oref, n));
    CK(hipMalloc(&csrc, (cvec + 1) * 16)); CK(hipMalloc(&cdst, (cvec + 1) * 16));
    CK(hipMemset(csrc, 0x5A, (cvec + 1) * 16));
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
        unsigned long long s = 88172645463325252ull;
        for (i64 i = 0; i < n; i++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; h[i] = (unsigned char)(s >> 24); }
        CK(hipMemcpy(a, h, n, hipMemcpyHostToDevice));
        for (i64 i = 0; i < n; i++) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; h[i] = (unsigned char)(s >> 24); }
        CK(hipMemcpy(b, h, n, hipMemcpyHostToDevice));
        free(h);
    }

    std::vector<Variant> V;
    if (nts) add_variants<true>(V, cus, dtab, a, b, o, nvec, csrc, cdst, cvec);
    else add_variants<false>(V, cus, dtab, a, b, o, nvec, csrc, cdst, cvec);

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
    {   // spot check of A against the host table
        std::vector<unsigned char> ha(4096), hb(4096), ho(4096);
        const i64 m = std::min<i64>(4096, nvec * 16);
        CK(hipMemcpy(ha.data(), a, m, hipMemcpyDeviceToHost)); CK(hipMemcpy(hb.data(), b, m, hipMemcpyDeviceToHost));
        CK(hipMemcpy(ho.data(), oref, m, hipMemcpyDeviceToHost));
        for (i64 i = 0; i < m; i++)
            if (ho[i] != htab[ha[i] * 256 + hb[i]]) { printf("A differs from the host table at %lld\n", i); bad_variants++; break; }
    }
    printf("n = %lld, %s stores, %d CUs, %d rounds x %d launches; table variants that differ from A: %d\n", n,
           nts ? "non-temporal" : "ordinary", cus, rounds, launches, bad_variants);
    if (bad_variants) return 1;

    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    {   // ~0.1 s of untimed load so that the clocks are up
        float total = 0.f;
        while (total < 100.f) {
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < 200; i++) V[0].launch();
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
    printf("%-50s %9s %9s %9s %9s %8s\n", "variant (3 n bytes moved)", "median us", "min us", "max us", "max-min", "TB/s");
    for (auto &v : V) {
        std::sort(v.us.begin(), v.us.end());
        const float med = v.us[v.us.size() / 2];
        printf("%-50s %9.2f %9.2f %9.2f %9.2f %8.3f\n", v.name.c_str(), med, v.us.front(), v.us.back(), v.us.back() - v.us.front(),
               3.0 * n / med / 1e6);
    }
    return 0;
}
