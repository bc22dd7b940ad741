// tickets.h — work distribution of the persistent scan kernels (adc_scan.hip, plain_scan.hip):
// blocks of work are drawn from a few work counters, each counter a range of consecutive blocks.
// The plain scan starts a wave at the counter of the XCD it runs on, so that blocks which share
// inputs meet in one L2; the exact scan starts it at the counter of its wave number.
#pragma once
#include <stdint.h>

// work counters of the list-major scan: TK_TICKETS ints, 128 bytes apart, behind the
// (n_lists+1)-entry unit_prefix table in the same allocation
#define TK_TICKETS 8
#define TK_TICKET_OFF(n_lists) ((((n_lists) + 1 + 31) / 32 + 1) * 32)

// ---- the arithmetic of the handout (no GPU in it: tests/test_ticket_ranges_cpu.py) ----
// N blocks are cut into TK_TICKETS ranges of near-equal length, range r = [tk_range_lo(N, r),
// tk_range_lo(N, r + 1)): tk_range_lo(N, 0) == 0, tk_range_lo(N, TK_TICKETS) == N, non-decreasing in
// between, so the ranges partition [0, N) whatever N (some are empty when N < TK_TICKETS).
constexpr int tk_range_lo(int N, int r) { return (int)((int64_t)N * r / TK_TICKETS); }
// the i-th range (i = 0 .. TK_TICKETS - 1) of a wave that starts at `start` (any int, only its low
// bits count): every range once, cyclically
constexpr int tk_range_at(int start, int i) { return (start + i) & (TK_TICKETS - 1); }

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

// Where a wave starts, and what it starts with.
// TK_START_XCD (plain scan): the range numbered by the XCC id of the XCD the wave runs on
//   (HW_REG_XCC_ID = 20, bits 0..3, masked to the number of ranges).  Workgroups are dealt round-robin
//   over the eight XCDs and each XCD has its own L2; the waves of one XCD now drain one range of
//   consecutive units, and units are numbered list by list, tile by tile, range by range: the units of
//   a list read its codes, the ranges of a tile its table rows, once into that L2 instead of once per
//   XCD over the fabric.  The XCC id is a hint about locality and nothing else — HIP promises nothing
//   about placement — so EVERY block, a wave's first included, comes from the counters, and the ranges
//   split all NB blocks: no block is handed out twice or left out wherever the workgroups run.  On a
//   device that shows fewer XCDs (partitioned modes) all waves start on as few counters as there are
//   XCDs: the handout is still complete, the first draws queue up on those counters (same-address
//   atomics retire at ~60 M/s) and the other ranges are reached by the cyclic walk, in order.
// TK_START_WAVE (exact scan: its reuse is weak — the coarse codes are 28 KB and the table rows stay in
//   L1): wave w takes block w statically (by wave number, so placement cannot matter either), the
//   counters split the other NB - NW blocks, and a wave starts at range w mod TK_TICKETS — every range
//   is drained by waves of all XCDs at once.
enum { TK_START_WAVE = 0, TK_START_XCD = 1 };

// NB blocks of work (a unit of the plain scan, 64 consecutive units of the exact scan) drawn from
// TK_TICKETS work counters (behind the prefix table, a cache line each, zeroed by the kernel that
// wrote the table): counter r counts the blocks of range r handed out.  A wave draws from its range
// until the counter passes the range's length, then from the next range cyclically, and is done after
// TK_TICKETS ranges.  Only a wave's first draw (TK_START_XCD) and the search for a range with work
// left wait for their answer: the draw for the NEXT block is issued before the current block's work
// and looked at behind it.  With other batches' heap replays sharing some SIMDs a static split leaves
// the kernel waiting for its slowest waves.  One counter would not do: same-address atomics retire
// at ~60 M/s and this kernel wants 70 M blocks/s.
// `work(blk)` processes block blk of NB.
template <int START, typename F>
__device__ __forceinline__ void ticketed_blocks(int NB, int *ticket, F work)
{
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
    int NW = 0;                                     // blocks handed out statically
    if (START == TK_START_WAVE) NW = gridDim.x * 4 < NB ? gridDim.x * 4 : NB;
    const int dyn = NB - NW;
    int tried = 0;
    int tk = tk_range_at(START == TK_START_XCD ? (int)__builtin_amdgcn_s_getreg(20 | (3 << 11)) : wid, 0);
    // synchronous draw: the search through the ranges for one that has blocks left
    auto draw = [&]() -> int {
        while (tried < TK_TICKETS) {
            const int lo = tk_range_lo(dyn, tk);
            const int len = tk_range_lo(dyn, tk + 1) - lo;
            int got = len;
            if ((threadIdx.x & 63) == 0) {
                int *t = ticket + tk * 32;
                if (__atomic_load_n(t, __ATOMIC_RELAXED) < len) got = atomicAdd(t, 1);
            }
            got = __builtin_amdgcn_readfirstlane(got);
            if (got < len) return NW + lo + got;
            tried++;
            tk = tk_range_at(tk, 1);
        }
        return NB;
    };
    int blk = START == TK_START_WAVE ? (wid < NW ? wid : NB) : draw();
    while (blk < NB) {
        // draw the block after this one now; the answer is looked at after this block's work
        int nlo = 0, nlen = 0, ngot = 0;
        const bool drawn = dyn > 0 && tried < TK_TICKETS;
        if (drawn) {
            nlo = tk_range_lo(dyn, tk);
            nlen = tk_range_lo(dyn, tk + 1) - nlo;
            if ((threadIdx.x & 63) == 0) ngot = atomicAdd(ticket + tk * 32, 1);
        }
        work(__builtin_amdgcn_readfirstlane(blk));   // wave-uniform, and known to be
        // next block
        blk = NB;
        if (!drawn) break;
        ngot = __builtin_amdgcn_readfirstlane(ngot);
        if (ngot < nlen) {
            blk = NW + nlo + ngot;
            continue;
        }
        tried++;
        tk = tk_range_at(tk, 1);
        blk = draw();
    }
}
#endif
