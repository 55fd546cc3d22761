// Host replay of tools/ubench/tab8_sched.h: the block schedules that the micro-benchmark tools/ubench/stream4.hip times for the
// 64 KiB-table kernel (benchmark-only code; the library's kernels do not use that header), with the
// workgroups advanced in a shuffled order (so claims are handed out in an order no launch is promised), for a set of array
// sizes, grids, block sizes and static / claimed splits.  Every vector index in [0, n / 16) must be visited exactly once,
// nothing beyond it, the tail must be the n % 16 last elements, and the claim count must stay inside tab8_max_claims.
//   g++ -O2 -std=c++17 -I tools/ubench tests/csrc/tab8_sched_host_test.cpp -o tab8_sched_test && ./tab8_sched_test
// (also clean under -fsanitize=address,undefined)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tab8_sched.h"

using gfa::Tab8Sched;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static long fails = 0;
#define EXPECT(c, ...)                                                                                                     \
    do {                                                                                                                   \
        if (!(c)) { if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } }                    \
    } while (0)

static void replay(int64_t n, int max_grid, int bvec, int64_t claim_rounds)
{
    const Tab8Sched s = gfa::tab8_sched(n, max_grid, bvec, claim_rounds);
    const char *fmt = "n=%lld max_grid=%d bvec=%d claim_rounds=%lld";
#define WHERE fmt, (long long)n, max_grid, bvec, (long long)claim_rounds
    EXPECT(s.nvec == n / 16, WHERE);
    EXPECT(s.grid >= 1 && s.grid <= max_grid, WHERE);
    EXPECT(s.nblk == (s.nvec + bvec - 1) / bvec, WHERE);
    EXPECT(s.nstatic >= 0 && s.nstatic <= s.nblk, WHERE);
    EXPECT(s.nstatic >= (s.nblk < s.grid ? s.nblk : s.grid), WHERE);                 // first block of every workgroup is static
    if (claim_rounds == 0 || s.nblk <= max_grid) EXPECT(s.nstatic == s.nblk, WHERE); // nothing claimed
    EXPECT(gfa::tab8_tail_first(s) == s.nvec * 16 && n - gfa::tab8_tail_first(s) >= 0 && n - gfa::tab8_tail_first(s) < 16, WHERE);

    std::vector<uint8_t> seen((size_t)s.nvec, 0);
    std::vector<int64_t> cur((size_t)s.grid);
    std::vector<int> active;
    for (int g = 0; g < s.grid; g++) { cur[g] = g; if (g < s.nblk) active.push_back(g); }
    uint32_t counter = 0; // the global claim counter
    int64_t visited = 0, steps = 0;
    while (!active.empty()) {
        const size_t pick = (size_t)(rnd() % active.size());
        const int g = active[pick];
        const int64_t blk = cur[g];
        EXPECT(blk >= 0 && blk < s.nblk, WHERE);
        // the kernel: the claim for the next block is taken before this block is stored
        int64_t nxt;
        if (gfa::tab8_next_is_claimed(s, blk)) nxt = gfa::tab8_claimed_block(s, counter++);
        else nxt = blk + s.grid;
        const int64_t first = gfa::tab8_block_first(s, blk), end = gfa::tab8_block_end(s, blk);
        EXPECT(first >= 0 && first < end && end <= s.nvec && end - first <= bvec, WHERE);
        for (int64_t i = first; i < end && i < s.nvec; i++) { seen[(size_t)i]++; visited++; }
        EXPECT(nxt > blk, WHERE); // progress: the loop is bounded by the block count
        cur[g] = nxt;
        if (nxt >= s.nblk) { active[pick] = active.back(); active.pop_back(); }
        if (++steps > s.nblk + s.grid) { EXPECT(false, WHERE); break; }
    }
    EXPECT((int64_t)counter <= gfa::tab8_max_claims(s), WHERE);
    if (s.nstatic == s.nblk) EXPECT(counter == 0, WHERE); // a static schedule never touches the counter
    EXPECT(visited == s.nvec, WHERE);
    int64_t wrong = 0;
    for (int64_t i = 0; i < s.nvec; i++) wrong += seen[(size_t)i] != 1;
    EXPECT(wrong == 0, WHERE);
#undef WHERE
}

int main()
{
    long cases = 0;
    const int grids[] = {1, 2, 7, 256, 512};
    const int bvecs[] = {1024, 2048};
    const int64_t crs[] = {0, 1, 2, 4, (int64_t)1 << 40};
    for (int grid : grids)
        for (int bvec : bvecs)
            for (int64_t cr : crs) {
                const int64_t B = (int64_t)bvec * 16; // elements per block
                const int64_t ns[] = {0, 1, 15, 16, 17, B - 1, B, B + 1, grid * B - 16, grid * B, grid * B + 16,
                                      3 * grid * B + 5, 100000000};
                for (int64_t n : ns) { replay(n, grid, bvec, cr); cases++; }
            }
    printf("tab8 schedule: %ld cases, fails %ld\n", cases, fails);
    if (!fails) printf("tab8 schedule ok\n");
    return fails ? 1 : 0;
}
