// gfa_scratch.h -- the stream-ordered work buffers of one call, and the one guard that owns them.
#pragma once
#include <hip/hip_runtime_api.h>

namespace gfa {

// Stream-ordered work buffers of one call (hipMallocFromPoolAsync / hipFreeAsync) from a pool the library owns, one per
// device, with a release threshold of 256 MiB (GFA_SCRATCH_KEEP_MB): freed blocks up to that total stay in the pool across
// synchronisations instead of going back to the driver (the device's default pool releases at every synchronisation --
// 0.05 ms per Reed-Solomon decode); gfa_trim_scratch() returns the rest on demand.
hipError_t scratch_alloc(void **p, size_t bytes, hipStream_t st);
hipError_t scratch_free(void *p, hipStream_t st);

// The work buffers of one call: every buffer taken through get() goes back to the pool, last taken first, on the call's
// stream, on every way out of the scope -- after the launches already enqueued there, so a failed launch in the middle
// leaves nothing in the pool's books.  At most 8 buffers, no heap allocation; the result of the free is ignored.
class Scratch {
public:
    explicit Scratch(hipStream_t st) : st_(st) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { while (n_ > 0) (void)scratch_free(p_[--n_], st_); }
    template <class T>
    hipError_t get(T **out, size_t count)
    {
        *out = nullptr;
        if (n_ == kSlots) return hipErrorInvalidValue;
        void *p = nullptr;
        const hipError_t e = scratch_alloc(&p, count * sizeof(T), st_);
        if (e != hipSuccess) return e;
        p_[n_++] = p;
        *out = static_cast<T *>(p);
        return hipSuccess;
    }

private:
    static constexpr int kSlots = 8;
    hipStream_t st_;
    void *p_[kSlots];
    int n_ = 0;
};

} // namespace gfa
