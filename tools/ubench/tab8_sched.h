// tab8_sched.h -- BENCHMARK-ONLY code: the block schedules that tools/ubench/stream4.hip (k_sched) times for the 64 KiB-table
// kernel -- static striding, claimed blocks, and hybrids of the two -- as plain integer arithmetic that compiles for the host too.
// The library does not include this file: every schedule that claims blocks lost at 1e8 elements (profiles/r07_stream_order_1e8.txt),
// so tab8_binary_kernel kept its own grid-stride loop and tab8_binary_claim_kernel its own inline arithmetic (gfa_elementwise.hip).
// tests/csrc/tab8_sched_host_test.cpp replays these schedules with claims handed out in a shuffled order and checks that every
// vector is covered exactly once: that is what makes the benchmark's timings comparable (every variant does all of the work), and
// it is the starting point should a claimed schedule ever move into the library.
//
// The n >> 4 whole vectors are cut into blocks of `bvec` vectors (the last one partial).  Blocks [0, nstatic) are walked
// statically -- workgroup g takes g, g + grid, g + 2 grid, ... -- and blocks [nstatic, nblk) are handed out in completion
// order by a global counter: claim number c (the value atomicAdd returned) is block nstatic + c.  The first block of every
// workgroup is always static, so nstatic >= min(nblk, grid).  The n & 15 tail elements belong to workgroup 0.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GFA_SCHED_HD __host__ __device__
#else
#define GFA_SCHED_HD
#endif

namespace gfa {

struct Tab8Sched {
    int64_t nvec;    // whole vectors, n >> 4
    int64_t nblk;    // blocks, ceil(nvec / bvec)
    int64_t nstatic; // blocks [0, nstatic) are strided statically, [nstatic, nblk) are claimed
    int bvec;        // vectors per block
    int grid;        // workgroups
};

// claim_rounds: how many of the last floor(nblk / grid) rounds (plus the ragged remainder) are claimed instead of strided;
// 0 = everything static, a huge value = everything but the first block of each workgroup claimed.
// A grid that does not fill the device (fewer blocks than max_grid) has no ragged end to repair and stays static.
GFA_SCHED_HD inline Tab8Sched tab8_sched(int64_t n, int max_grid, int bvec, int64_t claim_rounds)
{
    Tab8Sched s;
    s.nvec = n >> 4;
    s.bvec = bvec;
    s.nblk = (s.nvec + bvec - 1) / bvec;
    s.grid = (int)(s.nblk < 1 ? 1 : s.nblk < max_grid ? s.nblk : max_grid);
    const int64_t rounds = s.nblk / s.grid;
    int64_t srounds = claim_rounds <= 0 ? rounds + 1 : rounds - claim_rounds;
    if (srounds < 1) srounds = 1;
    if (s.nblk <= max_grid) srounds = 1; // nblk == grid: one static block each, nothing left to claim
    s.nstatic = srounds * s.grid < s.nblk ? srounds * s.grid : s.nblk;
    return s;
}

GFA_SCHED_HD inline int64_t tab8_block_first(const Tab8Sched &s, int64_t blk) { return blk * s.bvec; }
GFA_SCHED_HD inline int64_t tab8_block_end(const Tab8Sched &s, int64_t blk)
{
    const int64_t e = (blk + 1) * s.bvec;
    return e < s.nvec ? e : s.nvec;
}
// the workgroup that holds block `blk`: is its next block a claimed one (true) or blk + grid (false)?  Once true it stays true,
// since claimed blocks are >= nstatic.  False with blk + grid >= nblk means the workgroup is done.
GFA_SCHED_HD inline bool tab8_next_is_claimed(const Tab8Sched &s, int64_t blk)
{
    return blk + s.grid >= s.nstatic && s.nstatic < s.nblk;
}
GFA_SCHED_HD inline int64_t tab8_claimed_block(const Tab8Sched &s, uint32_t claim) { return s.nstatic + (int64_t)claim; }
// claims a launch can take at most: every claimed block once, plus one failed claim per workgroup
GFA_SCHED_HD inline int64_t tab8_max_claims(const Tab8Sched &s) { return (s.nblk - s.nstatic) + s.grid; }
// the tail: elements [tail_first, n), fewer than 16, done by workgroup 0
GFA_SCHED_HD inline int64_t tab8_tail_first(const Tab8Sched &s) { return s.nvec << 4; }

} // namespace gfa
