// scratch_host_test.cpp -- gfa::Scratch (galois_amd/csrc/gfa_scratch.h) against an allocator of this file: malloc / free that
// log every call with its stream and can refuse the k-th allocation.  Built plain and under ASan + UBSan by
// tests/test_scratch_host.py; with ASan a leaked or doubly freed buffer ends the run.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gfa_scratch.h"

namespace {
struct Call {
    void *p;
    hipStream_t st;
};
std::vector<Call> g_allocs, g_frees;
int g_alloc_calls = 0, g_refuse_at = -1; // g_refuse_at: index of the allocation call to refuse (-1: none)
int g_failures = 0;

void reset(int refuse_at)
{
    g_allocs.clear();
    g_frees.clear();
    g_alloc_calls = 0;
    g_refuse_at = refuse_at;
}

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                     \
            g_failures++;                                                        \
        }                                                                        \
    } while (0)
} // namespace

namespace gfa {
hipError_t scratch_alloc(void **p, size_t bytes, hipStream_t st)
{
    if (g_alloc_calls++ == g_refuse_at) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    g_allocs.push_back({*p, st});
    return hipSuccess;
}
hipError_t scratch_free(void *p, hipStream_t st)
{
    g_frees.push_back({p, st});
    free(p); // a second free of the same pointer is an ASan report
    return hipErrorUnknown; // the guard ignores the result
}
} // namespace gfa

namespace {
hipStream_t stream_a() { return reinterpret_cast<hipStream_t>(0x1000); }

// every logged allocation freed exactly once, last taken first, on `st`
void check_all_freed(hipStream_t st)
{
    CHECK(g_frees.size() == g_allocs.size());
    for (size_t i = 0; i < g_frees.size() && i < g_allocs.size(); i++) {
        CHECK(g_frees[i].p == g_allocs[g_allocs.size() - 1 - i].p);
        CHECK(g_frees[i].st == st);
    }
    for (const Call &a : g_allocs) CHECK(a.st == st);
}

// takes n buffers of mixed element types, leaves by an early return after the last one when `early`
int take(hipStream_t st, int n, bool early, int *first_failed)
{
    gfa::Scratch ws(st);
    *first_failed = -1;
    for (int i = 0; i < n; i++) {
        hipError_t e;
        void *got;
        if (i & 1) { double *d = reinterpret_cast<double *>(8); e = ws.get(&d, (size_t)i + 3); got = d; if (e == hipSuccess) d[i + 2] = 1.0; }
        else { unsigned char *c = reinterpret_cast<unsigned char *>(8); e = ws.get(&c, (size_t)i + 3); got = c; if (e == hipSuccess) c[i + 2] = 1; }
        if (e != hipSuccess) {
            CHECK(got == nullptr);
            *first_failed = i;
            return 1; // the k earlier buffers go back here
        }
        CHECK(got != nullptr && got == g_allocs.back().p);
        CHECK(g_frees.empty()); // nothing is freed while the scope lives
    }
    if (early) return 2;
    CHECK(g_frees.empty());
    return 0;
}
} // namespace

int main()
{
    int failed_at;
    for (int n : {0, 1, 5, 8})
        for (bool early : {false, true}) {
            reset(-1);
            CHECK(take(stream_a(), n, early, &failed_at) == (early ? 2 : 0));
            CHECK((int)g_allocs.size() == n && g_alloc_calls == n);
            check_all_freed(stream_a());
        }
    for (int n : {1, 5, 8})
        for (int k = 0; k < n; k++) {
            reset(k);
            CHECK(take(stream_a(), n, false, &failed_at) == 1);
            CHECK(failed_at == k);
            CHECK((int)g_allocs.size() == k && g_alloc_calls == k + 1); // nothing was asked for after the refusal
            check_all_freed(stream_a());
        }
    { // the null stream is a stream like any other
        reset(-1);
        CHECK(take(nullptr, 2, false, &failed_at) == 0);
        check_all_freed(nullptr);
    }
    { // a ninth buffer: refused without a call of the allocator, the eight stay owned
        reset(-1);
        {
            gfa::Scratch ws(stream_a());
            int *p[9];
            for (int i = 0; i < 8; i++) CHECK(ws.get(&p[i], 4) == hipSuccess && p[i] != nullptr);
            p[8] = reinterpret_cast<int *>(8);
            CHECK(ws.get(&p[8], 4) == hipErrorInvalidValue);
            CHECK(p[8] == nullptr);
            CHECK(g_alloc_calls == 8 && g_frees.empty());
        }
        CHECK(g_allocs.size() == 8);
        check_all_freed(stream_a());
    }
    if (g_failures) return 1;
    printf("scratch guard ok\n");
    return 0;
}
