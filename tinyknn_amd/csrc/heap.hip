// heap.hip — exact replay of the reference's bounded top-R "heap" on gfx950: the LANE-PER-QUERY replay.
//
// Replaces the selection half of query_pq_sse (_fast_pq.pyx:153-206) /
// query_pq_avx (_fast_pq_256.pyx:73-123) and the heap primitives init_heap,
// insert, insert_is (_fast_pq.pyx:240-307).
//
// The reference's result is a function of stream order and heap layout (SURVEY §0
// fact 2): per 16-code block it compares against the bound captured at block
// start, inserts EVERY passing lane without re-checking, and refreshes the bound
// once per block.  `insert` drops a label that is already present anywhere and
// otherwise replaces the root and sifts down (left child unless the right one is
// strictly greater).  The replays do exactly that from the int8 distances the scan
// kernels wrote.  All are bit-exact (tests compare heap arrays, layout included, with
// the compiled reference):
//
//   heap.hip (this file)
//     heap_replay_lanes_kernel      one query per LANE (64 per wave), packed 32-bit entries in LDS columns, block
//                                   minima, top heap levels in registers; fresh heaps, labels that cannot repeat:
//                                   every lane a RING of staged blocks of its own.  The batch path.
//     heap_replay_lanes_seg_kernel  the same heap over 16-block SEGMENTS the wave walks in step: DEDUPE / TWIN
//                                   (labels that can repeat) and LAZY (rows far longer than the heap).
//   heap_wave.hip
//     heap_replay_packed_kernel     one query per WAVE on the same packed entries (heaps too big for the lane
//                                   kernels' LDS budget, the queries a lane replay flags).
//     heap_replay_kernel            the general form: int64 labels, arbitrary incoming heaps (tk_query_pq
//                                   continues whatever the caller passes); heap_fill / heap_insert.
//   heap_pair.hip
//     heap_replay_pair_kernel       one query per wave, the heap in REGISTERS (up to 513 entries): one query per
//                                   call and small batches.
//   heap_flat.hip
//     flat_top_one_kernel           one query over one long array, one workgroup, heap of <= 64 entries in registers.
//   heap_common.h                   what they share: block compares, packed entries, position -> label.
#include <stdlib.h>

#include "heap_common.h"

// ---------------------------------------------------------------------------
// Lane-per-query replay (the throughput path of IVF.query batches).
//
// The wave-per-query kernels (heap_wave.hip) spend 64 lanes on one scalar heap.  When
//   (a) every heap starts fresh (ivf.py:137-138 / init_heap),
//   (b) no label can occur twice among the lists a query scans (ids are globally
//       unique, i.e. IVF.build(n_probes=1), or positions of one list), so the
//       duplicate test of `insert` can never fire,
// each LANE can replay one query: same blocks, same stale-bound test, same
// unconditional inserts, same sift-down — 64 queries per wave in SIMT.
//   * heap entry = one dword (value8 << 24 | flat position24) in LDS, laid out
//     [slot j][lane]: a lane only touches its own column and bank = lane % 32, so
//     the divergent sift-down addresses are conflict-free by construction;
//   * the distance rows are staged 16 blocks per lane at a time: the next segment is
//     fetched into registers while the current one is replayed and dropped into
//     ST[k][lane] at the switch, so that no lane ever waits on a dependent global
//     load; inside a segment lanes are decoupled: each walks to its next block with
//     a byte below its bound, then all lanes with a pending candidate perform one
//     insert together; a bound is refreshed when its block is done;
//   * (without a duplicate test: !DEDUPE && !TWIN && !LAZY) the lanes do not walk segments in step — a wave that does
//     pays, per segment, the LARGEST insert count among its 64 lanes: sum over segments of the maximum, 678 rounds per
//     wave for ~460 inserts per query — but each keeps a RING of staged blocks of its own: a cursor into its row's
//     block minima, a FIFO over its TK_RING_SLOTS rows ST[slot][lane], up to TK_RING_LOADS blocks in flight in
//     registers.  Every TK_RING_T rounds (and whenever no lane has a pending row) the wave REFILLS: the blocks
//     requested at the previous refill drop into the rings, each lane picks its next blocks whose minimum is below
//     its bound of now and requests them.  A lane without a pending row pops its ring.  Why the heaps are the same:
//       - a block whose minimum is >= a bound captured earlier is >= the bound at its own start (a bound only
//         falls): the reference enters it, inserts nothing, and the bound does not move — leaving it out is a no-op;
//       - the blocks that are staged are replayed in row order, each tested against the bound at its own start (a
//         lane pops only when its block is done and its bound refreshed) with the same strict `<`, the same
//         unconditional replace-root insert and the same sift;
//       - lanes never shared state.
//     (tests/test_ring_replay_lemma.py checks the first point on the reference's loop; scripts/sim_replay_rounds.py
//     is the model of the rounds per wave.)
//   * pad_fix_kernel has set the rows that pad a list's last chunk to the largest
//     value beforehand (`pos < n`, _fast_pq_256.pyx:111), so there is no row mask
//     and, with distinct labels, no slot cursor in the loop;
//   * the scan kernel also wrote each block's minimum (1 byte per block): a lane
//     tests 16 minima at once and touches only blocks that can contain a hit;
//   * the top three heap levels (nodes 0..6) are kept in registers;
//   * labels are resolved from the flat positions once, at the end.
// The form without a duplicate test (distinct labels, and the coarse replay of every index) stages its blocks in a
// per-lane RING instead of segments the wave walks in step (see the head of heap_replay_lanes_kernel):
#define TK_RING_SLOTS 8     // staging rows ST[slot][lane] of a lane's ring (the queue of block numbers below holds eight)
#ifndef TK_RING_T
#define TK_RING_T 4         // insert rounds between two refills of the rings
#endif
#ifndef TK_RING_LOADS
#define TK_RING_LOADS 4     // blocks a lane requests per refill at most (uint4 registers in flight)
#endif

// `pos < n` (_fast_pq_256.pyx:111) once, ahead of the replay: the rows that pad the last chunk
// of a probed list (code of the zero vector, fast_pq.py:165) get the largest distance value —
// nothing is ever below a bound with it, which is exactly what the reference's row test
// achieves — and the chunk's minimum is recomputed.  One thread per (query, slot).
template <bool SIGNED>
__global__ void pad_fix_kernel(uint4 *__restrict__ dist, int64_t cap, int64_t nq,
                               const int *__restrict__ slot_prefix, const int *__restrict__ slot_n,
                               int S, int slots_uniform, uint8_t *__restrict__ mins, int64_t cap_min,
                               int *__restrict__ flag_list)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && flag_list) flag_list[0] = 0;      // the lane replay behind this kernel appends the queries it flags
    if (i >= nq * S) return;
    const int64_t q = i / S;
    const int sl = (int)(i - q * S);
    const int64_t qs = slots_uniform ? 0 : q;
    const int f0 = slot_prefix[qs * (S + 1) + sl], f1 = slot_prefix[qs * (S + 1) + sl + 1];
    int n = slot_n[qs * S + sl];
    n = n < 0 ? 0 : n;
    const uint32_t fill = SIGNED ? 0x7f7f7f7fu : 0xffffffffu;
    for (int c = n >> 4; c < f1 - f0; c++) {
        const int keep = n - 16 * c;                   // valid rows of this chunk: 0..15
        uint4 v = dist[q * cap + f0 + c];
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        int m = SIGNED ? 127 : 255;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int km = keep - 4 * j;
            km = km < 0 ? 0 : (km > 4 ? 4 : km);
            const uint32_t kmask = km >= 4 ? 0xffffffffu : ((1u << (8 * km)) - 1u);
            w[j] = (w[j] & kmask) | (fill & ~kmask);
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const uint32_t b = (w[j] >> (8 * t)) & 0xffu;
                const int x = SIGNED ? (int)(int8_t)b : (int)b;
                m = x < m ? x : m;
            }
        }
        dist[q * cap + f0 + c] = make_uint4(w[0], w[1], w[2], w[3]);
        mins[q * cap_min + f0 + c] = (uint8_t)m;
    }
}

// ---------------------------------------------------------------------------
// LDS of one query-wave, written down ONCE: the kernels take their pointers from it, the launcher its launch size,
// tk_lanes_twin_fits / tk_lanes_dedupe_fits their budgets.  LW lanes of the wave carry a query (64, or 32: DEDUPE);
// a row of dword columns is CB = 4 LW bytes, regions in this order from the wave's base:
//   H   [R + 2][LW]            heap columns (+ 2 sentinel rows)
//   LAB [ceil(R / 4)][LW][4]   DEDUPE: the 32-bit label of every slot
//   TB  [64][LW] x uint4       DEDUPE: the labels in the heap as a two-choice hash set, 64 buckets of four
//   ST  [rows][LW] x uint4     staged blocks: none when LAZY, the TK_RING_SLOTS of a lane's ring without a duplicate
//                              test, 16 (one segment) otherwise
//   SE, SB [S][LW]             DEDUPE / TWIN: slot table of the lane's query (first flat chunk past slot s; label
//                              offset of slot s - 16 * its first flat chunk)
//   PL  [ceil(S / 4)][LW] x uint4   TWIN: the probed lists of the lane's query, four to a uint4
//   BM  [bm_words][LW]         TWIN: one bit per list of the index (tk_lanes_twin_bm_words), set for the lists replayed
// A launch smaller than this arithmetic does not fault on this hardware: it corrupts a neighbouring wave's heap.
// (T: uint32_t in the kernels — an LDS address is 32 bits, and as 64-bit values the offsets cost the segment kernels
// scalar registers they do not have — size_t on the host, where S is any int)
template <typename T>
struct TkLanesLds {
    T lab, tb, st, se, sb, pl, bm, bytes;     // byte offsets (H at 0), all of it
};
template <typename T = size_t>
__host__ __device__ constexpr TkLanesLds<T> tk_lanes_lds(bool dedupe, bool twin, bool lazy, int LW, int R, int S, int bm_words)
{
    const T CB = (T)LW * 4;
    const T R4 = (T)((R + 3) >> 2), S4 = (T)((S + 3) >> 2);
    const T st_rows = dedupe ? 16 : lazy ? 0 : twin ? 16 : TK_RING_SLOTS;
    const T slots = dedupe || twin ? (T)S : 0;
    TkLanesLds<T> L{};
    L.lab = (T)(R + 2) * CB;
    L.tb = L.lab + (dedupe ? R4 * CB * 4 : 0);
    L.st = L.tb + (dedupe ? (T)64 * CB * 4 : 0);
    L.se = L.st + st_rows * CB * 4;
    L.sb = L.se + slots * CB;
    L.pl = L.sb + slots * CB;
    L.bm = L.pl + (twin ? S4 * CB * 4 : 0);
    L.bytes = L.bm + (twin ? (T)bm_words * CB : 0);
    return L;
}
// What decides whether an index gets a lane replay (tk_lanes_*_fits, TK_LANES_MAX_R*) is not the launch size but a
// BUDGET: a 64-query wave with a 16-block segment (16 KiB) of staging, also for the forms that use less — the ring (8
// rows), LAZY (none), DEDUPE (32 queries: half of everything).  Which replay an index gets is behaviour: it stays.
constexpr size_t TK_LANES_LDS_MAX = 160 * 1024;
__host__ __device__ constexpr size_t tk_lanes_budget(bool dedupe, int R, int S, int bm_words)
{
    // (without the hash set this is the staged TWIN form's launch; S = 0: no slot table — the forms without a test)
    return tk_lanes_lds(dedupe, !dedupe, false, 64, R, S, bm_words).bytes;
}
// ring: TK_LANES_MAX_R is where the budget ends; the launch itself (8 staging rows) is 8 KiB below it
static_assert(tk_lanes_lds(false, false, false, 64, TK_LANES_MAX_R, 1, 0).bytes == 155648 &&
              tk_lanes_budget(false, TK_LANES_MAX_R, 0, 0) <= TK_LANES_LDS_MAX &&
              tk_lanes_budget(false, TK_LANES_MAX_R + 1, 0, 0) > TK_LANES_LDS_MAX, "ring form");
// TWIN: the LAZY form fits at TK_LANES_MAX_R; the staged form's launch IS the budget, over 160 KiB there beside even one
// list (165 376 B): tk_lanes_twin_fits is its limit, R <= 568 at S = 1 without a bitmap
static_assert(tk_lanes_lds(false, true, true, 64, TK_LANES_MAX_R, 1, 0).bytes <= TK_LANES_LDS_MAX &&
              tk_lanes_budget(false, 568, 1, 0) <= TK_LANES_LDS_MAX && tk_lanes_budget(false, 569, 1, 0) > TK_LANES_LDS_MAX, "TWIN form");
// DEDUPE: within the budget at 149, which is not where the budget ends (156 at S = 1; kernels.h)
static_assert(tk_lanes_budget(true, TK_LANES_MAX_R_DEDUPE, 1, 0) <= TK_LANES_LDS_MAX &&
              tk_lanes_budget(true, 156, 1, 0) <= TK_LANES_LDS_MAX && tk_lanes_budget(true, 157, 1, 0) > TK_LANES_LDS_MAX, "DEDUPE form");
// every region is whole rows of CB bytes, so every offset is a multiple of CB, and CB = 4 LW is a multiple of 16 for both
// LW: LAB, TB, ST and PL, which hold uint4, are 16-byte aligned at any R, S and bitmap (SE, SB and BM hold ints)
static_assert((32 * 4) % 16 == 0 && (64 * 4) % 16 == 0, "rows of the lane replay's LDS");

// ---------------------------------------------------------------------------
// What the two lane kernels share: a lane's query, its heap columns, the way out.

// The base of the query-wave's LDS (one wave per workgroup: the workgroup's) held in a VECTOR register, and with it every
// pointer into the regions above, as the multiply by the wave's number used to leave them.  This rests on what one
// compiler does (AMD clang 22.0.0git, ROCm 7.2.0) and on one box's numbers — measure again before relying on it.  As
// a link-time constant the base is added again at each use: one VALU more per level of the sift's dependent chain in
// LDS (v_lshlrev + v_add of the symbol for one v_lshl_add), the ring replay's isolated stage 0.605 ms against the parent
// commit's 0.602; with this it was 0.593 — faster than the parent's, not equal to it.  As scalars the region pointers
// also take the SGPRs of the kernel arguments that wait for the epilogue (DEDUPE: 44 parked in VGPR lanes instead of
// 42 / 40, TWIN: 23 instead of 21).
__device__ __forceinline__ unsigned char *lanes_lds_base()
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_wg[];
    uint32_t base = 0;
    asm volatile("" : "+v"(base));
    return smem_wg + base;
}

// The lane's query: q (valid: a query of the batch the replay may touch; `skip`: queries whose probe list may repeat a
// list, left to the wave kernel), its slot row, distance row and block minima.  A lane without a query reads the
// rows of the batch's last one and never writes.
struct LaneQuery {
    int64_t q, qc, qs;
    bool valid;
    const int *prefix;
    const uint4 *drow, *mrow;       // mrow: per-block minima, 16 per uint4
    int total;                      // flat chunks of this lane's query
    // plain_scan.hip: the blocks from flat chunk plain0 on carry clamp(plain sums), which equal the
    // reference's values below qlim[q] and are >= qlim[q] elsewhere: the replay over them is the
    // replay over the exact values iff the bound is <= qlim[q] when the first of their blocks is
    // reached.  b_plain follows the bound across the exact blocks; checked at the end.
    int plain0;
    // Blocks past the lane's row are clamped to its last valid address and never looked at.
    int last_blk, last_m;
    __device__ __forceinline__ uint4 block(int blk) const { return drow[blk < last_blk ? blk : last_blk]; }
    __device__ __forceinline__ uint4 mins16(int g) const { return mrow[g < last_m ? g : (last_m > 0 ? last_m : 0)]; }
};
template <int LW>
__device__ __forceinline__ LaneQuery lane_query(int lane, int64_t nq, const unsigned char *__restrict__ skip,
                                                int slots_uniform, const int *__restrict__ slot_prefix, int S,
                                                const uint4 *__restrict__ dist, int64_t cap,
                                                const uint8_t *__restrict__ mins, int64_t cap_min,
                                                const int *__restrict__ plain0_arr)
{
    LaneQuery Q;
    Q.q = (int64_t)blockIdx.x * LW + lane;          // one query-wave per workgroup
    Q.valid = Q.q < nq && !(skip && skip[Q.q]);
    Q.qc = Q.q < nq ? Q.q : nq - 1;
    Q.qs = slots_uniform ? 0 : Q.qc;
    Q.prefix = slot_prefix + Q.qs * (S + 1);
    Q.drow = dist + Q.qc * cap;
    Q.total = (Q.valid && S > 0) ? Q.prefix[S] : 0;
    Q.plain0 = (plain0_arr && Q.valid) ? plain0_arr[Q.qc] : 0x7fffffff;
    Q.mrow = (const uint4 *)(mins + Q.qc * cap_min);
    Q.last_blk = (int)(cap > 0 ? cap - 1 : 0);
    Q.last_m = (int)(cap_min / 16) - 1;
    return Q;
}

// The lane's heap: column `lane` of H[R + 2][LW], one packed entry per node, the top three levels (nodes 0..6) in
// registers; rows R and R + 1 and the registers of nodes >= R hold a value no entry is below (sentinels: never taken).
// SLOTS (DEDUPE): the low 24 bits of a fresh entry are its node's number — node j owns slot j.
template <bool SIGNED, bool SLOTS, int LW>
struct LaneHeap {
    uint32_t *H;
    int R, lane;
    uint32_t h0, h1, h2, h3, h4, h5, h6;
    __device__ __forceinline__ void init(uint32_t *H_, int R_, int lane_)
    {
        H = H_; R = R_; lane = lane_;
        const uint32_t fresh_val = SIGNED ? 0x7f000000u : 0xff000000u;
        const uint32_t fresh = fresh_val | 0x00ffffffu;
        const uint32_t lowest = SIGNED ? 0x80000000u : 0u;    // a value no entry is below
        for (int j = 0; j < R; j++)
            H[j * LW + lane] = SLOTS ? (fresh_val | (uint32_t)j) : fresh;   // node j owns slot j
        H[R * LW + lane] = H[(R + 1) * LW + lane] = lowest;   // sentinel rows: never taken
#define TK_FRESH(j) (R > (j) ? (SLOTS ? (fresh_val | (uint32_t)(j)) : fresh) : lowest)
        h0 = TK_FRESH(0); h1 = TK_FRESH(1); h2 = TK_FRESH(2); h3 = TK_FRESH(3);
        h4 = TK_FRESH(4); h5 = TK_FRESH(5); h6 = TK_FRESH(6);
#undef TK_FRESH
    }
    // `insert`, _fast_pq.pyx:291-307, levels 0-2 (registers).  -> 0: the entry has its place; j = 3..6: the sift goes
    // on below node j (lds_levels)
    __device__ __forceinline__ int reg_levels(const uint32_t entry, const int v)
    {
        // node 0, children 1 and 2
        const int v1 = entry_val<SIGNED>(h1), v2 = entry_val<SIGNED>(h2);
        const bool c1 = v1 > v;
        const int nv = c1 ? v1 : v;
        const bool c2 = v2 > nv;
        h0 = c2 ? h2 : (c1 ? h1 : entry);
        if (!(c1 | c2)) return 0;
        // node 1 or 2, children (3,4) or (5,6)
        const uint32_t a = c2 ? h5 : h3, b = c2 ? h6 : h4;
        const int va = entry_val<SIGNED>(a), vb = entry_val<SIGNED>(b);
        const bool ca = va > v;
        const int nv1 = ca ? va : v;
        const bool cb = vb > nv1;
        const uint32_t ne1 = cb ? b : (ca ? a : entry);
        if (c2) h2 = ne1; else h1 = ne1;
        return (ca | cb) ? (c2 ? 5 : 3) + (cb ? 1 : 0) : 0;
    }
    // `insert` below node j (3..6): children in LDS, branch-free per level — rows R and R+1 hold a value no entry
    // exceeds, so children beyond the heap (clamped to R) are never taken
    __device__ __forceinline__ void lds_levels(int j, const uint32_t entry, const int v)
    {
        bool first = true, go = true;
        do {
            const int l = 2 * j + 1;
            const int lc = l < R ? l : R;
            const uint32_t el = H[lc * LW + lane];
            const uint32_t er = H[(lc + 1) * LW + lane];
            const int vl = entry_val<SIGNED>(el), vr = entry_val<SIGNED>(er);
            const bool cl = vl > v;                 // vals[l] > nxt_val
            const int nvv = cl ? vl : v;
            uint32_t ne = cl ? el : entry;
            int nxt = cl ? l : j;
            const bool cr = vr > nvv;               // vals[r] > nxt_val
            ne = cr ? er : ne;
            nxt = cr ? l + 1 : nxt;
            if (first) {
                h3 = j == 3 ? ne : h3; h4 = j == 4 ? ne : h4;
                h5 = j == 5 ? ne : h5; h6 = j == 6 ? ne : h6;
                first = false;
            } else {
                H[j * LW + lane] = ne;              // entry itself when nxt == j
            }
            go = nxt != j;
            j = nxt;
        } while (go);
    }
    // registers back to their heap rows
    __device__ __forceinline__ void write_back()
    {
        if (R > 0) H[0 * LW + lane] = h0;
        if (R > 1) H[1 * LW + lane] = h1;
        if (R > 2) H[2 * LW + lane] = h2;
        if (R > 3) H[3 * LW + lane] = h3;
        if (R > 4) H[4 * LW + lane] = h4;
        if (R > 5) H[5 * LW + lane] = h5;
        if (R > 6) H[6 * LW + lane] = h6;
    }
};

// DEDUPE: the label of a slot
#define TK_LAB(slot) LAB[(((slot) >> 2) * LW + lane) * 4 + ((slot) & 3)]

// The way out of both kernels: counters, the heap's registers back to LDS, the queries left to the kernels behind,
// entries to (label, value) in the caller's arrays.  steps: segments walked, or refills of the rings.
template <bool SIGNED, bool DEDUPE, int LW>
__device__ __forceinline__ void lanes_finish(const LaneQuery &Q, LaneHeap<SIGNED, DEDUPE, LW> &hp, const uint32_t *LAB,
                                             uint32_t b_plain, int rounds, int steps,
                                             unsigned long long *__restrict__ dbg, int64_t nq,
                                             unsigned char *__restrict__ skip, int *__restrict__ flag_list,
                                             const int *__restrict__ plain0_arr, const int *__restrict__ qlim,
                                             const int64_t *__restrict__ slot_label_off, int S,
                                             const int64_t *__restrict__ labels, int64_t *__restrict__ heap_idx,
                                             int32_t *__restrict__ heap_val)
{
    const int lane = hp.lane, R = hp.R;
    const uint32_t *H = hp.H;
    const int64_t q = Q.q;
    if (dbg && lane == 0) {       // TK_OPT_REPLAY_COUNT: [0] += rounds, [1] = max rounds of a wave, [2] += waves, [3] += segments (RING: refills)
        atomicAdd(&dbg[0], (unsigned long long)rounds);
        atomicMax(&dbg[1], (unsigned long long)rounds);
        atomicAdd(&dbg[2], 1ull);
        atomicAdd(&dbg[3], (unsigned long long)steps);
    }
    hp.write_back();
    // flag_list: the queries left to the kernels behind this one — flagged before it (probe lists that name a list
    // twice) or by the check below — [0] = their count (zeroed by pad_fix_kernel), then their numbers in any order:
    // what a separate one-workgroup kernel over all nq flags used to compile (30 us of every batch's replay stream)
    if (!Q.valid) {
        if (flag_list && q < nq) flag_list[1 + atomicAdd(&flag_list[0], 1)] = (int)q;
        return;
    }
    // re-scan + replay again: flag 2 with distinct labels (no duplicate test needed then) and from the TWIN form, 1 otherwise
    if (plain0_arr && Q.plain0 < Q.total && (int)(int8_t)b_plain > qlim[Q.qc]) {
        skip[q] = DEDUPE ? 1 : 2;
        if (flag_list) flag_list[1 + atomicAdd(&flag_list[0], 1)] = (int)q;
    }
    // ---- resolve flat positions (or slots) to labels
    const int64_t *loffs = slot_label_off + Q.qs * S;
    for (int j = 0; j < R; j++) {
        const uint32_t e = H[j * LW + lane];
        const uint32_t pos = e & 0x00ffffffu;
        heap_idx[q * R + j] = DEDUPE ? (int64_t)(int32_t)TK_LAB(pos) : resolve_position(pos, Q.prefix, loffs, S, labels);
        heap_val[q * R + j] = entry_val<SIGNED>(e);
    }
}

// DEDUPE (labels may repeat, IVF.build(n_probes >= 2)): the low 24 bits of an entry are
// a SLOT, LAB[slot][lane] holds the slot's 32-bit label, `insert` first scans LAB for
// the candidate's label (the reference's duplicate test, _fast_pq.pyx:284-287) and a
// new entry inherits the slot of the root it evicts.  labels32 = the ids as int32.
// LAZY (rows far longer than the heap: _FastDistanceTable.top over a whole data set, 62 500 blocks per
// query at 1M rows): nothing is staged — a lane reads its row's block minima, 16 at a time and one
// segment ahead, and fetches a block from global memory only when its minimum passes the bound.
// A handful of blocks in 4 000 segments pass once the heap is warm; staging every block cost 16
// row-per-lane loads and 16 LDS writes per segment and lane (55 of the 90 ms per 10 000 queries).
// TWIN (labels may repeat AND every copy of a label carries ONE value: the lists of IVF.build(n_probes >= 2),
// ivf.py:53,77-102 — same code, same table): the duplicate test without a set of labels.  Entries stay
// POSITIONS as with distinct labels; the lane keeps f = the smallest value of any root it has evicted.  Every
// entry but the root is <= f (a root is the maximum when it leaves; a later insert above f stays at the root
// and is the next to leave).  A row that passes its block's bound (captured at block start, never rising from
// block to block) and has an EARLIER copy in the lists replayed so far: that copy passed too (same value, a
// bound no lower) and went in, or found a still earlier one in the heap.  So a copy is in the heap now
//     always                                         where v <  f  (nothing of value v has ever left),
//     iff the root is one of the earlier copies      where v >  f,
//     iff some entry is one of the earlier copies    where v == f  (the one case that scans the heap);
// and a row without an earlier copy never finds its label.  Checked at every passing row of random and
// adversarial streams against the reference's loop: tests/test_twin_dedupe_lemma.py.  Where the earlier
// copies are comes from twins.hip's table (list + offset of a stored row's other copies) and the query's
// probe list: one 4-byte load per candidate, fetched a candidate ahead; a 64-bit mask of the lists replayed
// so far answers "not probed" for most rows at once, the probe list in LDS answers exactly.  The hash set
// of the DEDUPE form (64 KB per 64 queries, its removal and insertion inside every round) is gone: 64
// queries per wave, three workgroups per CU, the LAZY form and pairs of calls apply as with distinct labels.

// The RING form: no duplicate test, every block staged through the lane's ring.  One query-wave per workgroup.
template <bool SIGNED>
__global__ __launch_bounds__(256) void heap_replay_lanes_kernel(
    const uint4 *__restrict__ dist, int64_t cap, int64_t nq, const int *__restrict__ slot_prefix,
    const int64_t *__restrict__ slot_label_off, int S, const int64_t *__restrict__ labels,
    int64_t *__restrict__ heap_idx, int32_t *__restrict__ heap_val, int R, int slots_uniform,
    unsigned char *__restrict__ skip, const uint8_t *__restrict__ mins, int64_t cap_min,
    unsigned long long *__restrict__ dbg, const int *__restrict__ plain0_arr, const int *__restrict__ qlim,
    int *__restrict__ flag_list)
{
    // the replay is a chain of dependent LDS round trips on 157 waves; when it shares SIMDs
    // with other batches' VALU-bound scan waves, let the arbiter issue its instructions first
    __builtin_amdgcn_s_setprio(3);
    constexpr int LW = 64;
    unsigned char *smem = lanes_lds_base();
    const TkLanesLds<uint32_t> L = tk_lanes_lds<uint32_t>(false, false, false, LW, R, S, 0);
    uint4 *ST = (uint4 *)(smem + L.st);
    const int lane = threadIdx.x & 63;
    const LaneQuery Q = lane_query<LW>(lane, nq, skip, slots_uniform, slot_prefix, S, dist, cap, mins, cap_min, plain0_arr);
    LaneHeap<SIGNED, false, LW> hp;
    hp.init((uint32_t *)smem, R, lane);
    uint32_t bound = SIGNED ? 0x7fu : 0xffu;
    uint32_t bb = bound_bytes<SIGNED>(bound);     // the bound's byte, biased, in all four bytes (mask_lt16_swar)
    uint32_t b_plain = SIGNED ? 0x7fu : 0xffu;
    int rounds = 0;               // wave-uniform: iterations of the insert loop (each a dependent chain: roofline.replay)
    int refills = 0;              // wave-uniform: refills of the rings (TK_OPT_REPLAY_COUNT)
    // ---- per-lane ring of staged blocks (the head of the file says why the heaps stay the same)
    const int nwin = (Q.total + 15) >> 4;          // windows of 16 block minima in the lane's row
    int win = -1;                                // the window the cursor is in
    uint32_t wmask = 0;                          // its blocks still to pick: minimum below the bound when it was entered
    uint4 m1 = make_uint4(0, 0, 0, 0), m2 = m1;  // minima of windows win + 1, win + 2, requested ahead
    // (a wave without any row touches neither its rows nor their minima; a lane without rows beside others
    // requests block 0 of its own row like them, and never looks at it)
    const bool wave_rows = __builtin_amdgcn_ballot_w64(nwin > 0) != 0;
    if (wave_rows) {
        m1 = Q.mins16(0);
        m2 = Q.mins16(1);
    }
    int head = 0, nst = 0, nfl = 0;              // ring: slot of the oldest staged block, blocks staged, blocks in flight
    // block numbers of the staged and in-flight blocks, oldest first: 16-bit steps from the block before (a window
    // that would put a step past 16 bits stages its first block whatever its minimum: a block nothing passes in)
    uint64_t qlo = 0, qhi = 0;
    int last_req = 0;                            // the block requested last
    uint4 fl[TK_RING_LOADS];                     // blocks in flight: fl[0 .. nfl)
#pragma unroll
    for (int k = 0; k < TK_RING_LOADS; k++) fl[k] = make_uint4(0, 0, 0, 0);
    uint32_t bits = 0;
    uint4 dd = make_uint4(0, 0, 0, 0);
    int cur = 0;                                 // the block popped last
    // One pass of this loop = one refill and up to TK_RING_T rounds behind it.  (The refill is not a branch inside
    // the round loop: what it requests is used at the head of the next pass and nowhere else, so each load keeps
    // ONE register from request to ring store, and the only vmcnt wait is in front of the ring stores.)
    while (wave_rows) {
        // ---- refill.  The blocks requested by the previous one: into the ring
        const bool more = nfl > 0 || wmask != 0 || win + 1 < nwin;
        refills += __builtin_amdgcn_ballot_w64(more) != 0;
#pragma unroll
        for (int k = 0; k < TK_RING_LOADS; k++)
            if (k < nfl) ST[((head + nst + k) & (TK_RING_SLOTS - 1)) * LW + lane] = fl[k];
        nst += nfl;
        nfl = 0;
        // the cursor: at most two windows per refill (their minima are in registers; those requested here arrive
        // while the rounds up to the next refill run)
#pragma unroll
        for (int a = 0; a < 2; a++) {   // (the second step only behind the first: wmask is unchanged otherwise)
            if (wmask == 0 && win + 1 < nwin) {
                win++;
                const int kn = Q.total - 16 * win;
                wmask = mask_lt16_swar<SIGNED>(a ? m2 : m1, bb) & (kn >= 16 ? 0xffffu : ((1u << kn) - 1u));
                if (16 * win - last_req > 0xffe0) wmask |= 1u;
            }
        }
        // pick and request: the next blocks of the window whose minimum passes, into the free slots.  No branch
        // around a load: every lane requests TK_RING_LOADS blocks and two rows of minima in every refill (a lane
        // with nothing to pick: the block it requested last)
        int room = TK_RING_SLOTS - nst;
        room = room > TK_RING_LOADS ? TK_RING_LOADS : room;
#pragma unroll
        for (int k = 0; k < TK_RING_LOADS; k++) {
            const bool take = k < room && wmask != 0;
            const int blk = take ? 16 * win + __builtin_ctz(wmask) : last_req;
            wmask &= take ? wmask - 1 : ~0u;
            fl[k] = Q.block(blk);
            const int p = nst + nfl;
            const uint64_t step = (uint64_t)(uint32_t)(blk - last_req) << (16 * (p & 3));
            qlo |= take && p < 4 ? step : 0;
            qhi |= take && p >= 4 ? step : 0;
            last_req = blk;
            nfl += take;
        }
        m1 = Q.mins16(win + 1);
        m2 = Q.mins16(win + 2);
        // (what is in flight or still in a row: if nothing is, in any lane, the last blocks are in the rings)
        const bool rest = __builtin_amdgcn_ballot_w64(nfl > 0 || wmask != 0 || win + 1 < nwin) != 0;
        // ---- rounds
        bool any = true;
        for (int t = 0; rest ? t < TK_RING_T : true; t++) {
            // a lane without a pending row pops its ring until a block has a row below the live bound (its block
            // is done and its bound refreshed: the bound at the popped block's own start)
            while (bits == 0 && nst > 0) {
                dd = ST[head * LW + lane];
                head = (head + 1) & (TK_RING_SLOTS - 1);
                nst--;
                cur += (int)((uint32_t)qlo & 0xffffu);
                qlo = (qlo >> 16) | (qhi << 48);
                qhi >>= 16;
                bits = mask_lt16_swar<SIGNED>(dd, bb);
            }
            any = __builtin_amdgcn_ballot_w64(bits != 0) != 0;
            if (!any) break;          // every ring is empty: refill at once
            rounds++;
            if (bits) {   // one insert per lane with a pending candidate
                const int r = __builtin_ctz(bits);
                bits &= bits - 1;
                const uint32_t by = block_byte(dd, r);
                const uint32_t entry = (by << 24) | (uint32_t)(16 * cur + r);
                const int v = entry_val<SIGNED>(entry);
                const int j = hp.reg_levels(entry, v);
                if (j) hp.lds_levels(j, entry, v);
                if (bits == 0) {  // refresh after the block, :123
                    bound = hp.h0 >> 24;
                    bb = bound_bytes<SIGNED>(bound);
                    b_plain = cur < Q.plain0 ? bound : b_plain;
                }
            }
        }
        if (!rest) break;             // no pending row, staged block, request in flight or row left in any lane
    }
    lanes_finish<SIGNED, false, LW>(Q, hp, nullptr, b_plain, rounds, refills, dbg, nq, skip, flag_list, plain0_arr, qlim,
                                    slot_label_off, S, labels, heap_idx, heap_val);
}

// The SEGMENT forms: DEDUPE, TWIN and LAZY (above).  One query-wave per workgroup.
template <bool SIGNED, bool DEDUPE, int LW, bool LAZY = false, bool TWIN = false>
__global__ __launch_bounds__(256) void heap_replay_lanes_seg_kernel(
    const uint4 *__restrict__ dist, int64_t cap, int64_t nq, const int *__restrict__ slot_prefix,
    const int64_t *__restrict__ slot_label_off, int S, const int64_t *__restrict__ labels,
    int64_t *__restrict__ heap_idx, int32_t *__restrict__ heap_val, int R, int slots_uniform,
    unsigned char *__restrict__ skip, const uint8_t *__restrict__ mins, int64_t cap_min,
    const int32_t *__restrict__ labels32, unsigned long long *__restrict__ dbg,
    const int *__restrict__ plain0_arr, const int *__restrict__ qlim, const TkTwins tw, int *__restrict__ flag_list)
{
    static_assert(!(TWIN && DEDUPE), "one form of the duplicate test");
    static_assert(DEDUPE || TWIN || LAZY, "without a duplicate test and with staged blocks: heap_replay_lanes_kernel");
    // the replay is a chain of dependent LDS round trips on 157 waves; when it shares SIMDs
    // with other batches' VALU-bound scan waves, let the arbiter issue its instructions first
    __builtin_amdgcn_s_setprio(3);
    // LW = queries per wave: 64, or 32 (lanes 32..63 idle) where the per-lane columns of the
    // duplicate test would otherwise leave room for only ONE workgroup per CU
    unsigned char *smem = lanes_lds_base();
    const int BMW = TWIN ? tw.bm_words : 0;
    const TkLanesLds<uint32_t> L = tk_lanes_lds<uint32_t>(DEDUPE, TWIN, LAZY, LW, R, S, BMW);
    const int R4 = (R + 3) >> 2, S4 = (S + 3) >> 2;
    uint32_t *H = (uint32_t *)smem;
    uint32_t *LAB = (uint32_t *)(smem + L.lab);
    uint4 *TB = (uint4 *)(smem + L.tb);
    uint4 *ST = (uint4 *)(smem + L.st);
    // label of row r of flat chunk c in slot s = labels32[SB[s] + 16 c + r]
    int *SE = (int *)(smem + L.se);
    int *SB = (int *)(smem + L.sb);
    uint4 *PL = (uint4 *)(smem + L.pl);
    // (BM where the index has few enough lists: tw.bm_words > 0; a 64-bit mask of list & 63 in front of a search of PL
    // otherwise)
    uint32_t *BM = (uint32_t *)(smem + L.bm);
    const int lane = threadIdx.x & 63;
    if (LW < 64 && lane >= LW) return;   // idle half-wave: no barrier follows, ballots see exec only
    const LaneQuery Q = lane_query<LW>(lane, nq, skip, slots_uniform, slot_prefix, S, dist, cap, mins, cap_min, plain0_arr);

    LaneHeap<SIGNED, DEDUPE, LW> hp;
    hp.init(H, R, lane);
    if (DEDUPE) {
        for (int g = 0; g < R4; g++)                                     // every label -1
            ((uint4 *)LAB)[g * LW + lane] = make_uint4(~0u, ~0u, ~0u, ~0u);
        for (int b = 0; b < 64; b++) TB[b * LW + lane] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    // DEDUPE: labels that found both their buckets full wait in a four-entry stash (registers);
    // only a lane whose stash is full too falls back to scanning LAB — with 64 lanes x ~1000
    // inserts per wave even a 1e-4 event per insert would otherwise put every wave on the scan
    uint32_t sh0 = ~0u, sh1 = ~0u, sh2 = ~0u, sh3 = ~0u;
    bool tb_ovf = false;
    uint32_t bound = SIGNED ? 0x7fu : 0xffu;
    uint32_t bb = bound_bytes<SIGNED>(bound);     // the bound's byte, biased, in all four bytes (mask_lt16_swar)
    uint32_t b_plain = SIGNED ? 0x7fu : 0xffu;
    // Blocks per staged segment.  The staging rows are LDS SPACE, which is what the pipelined
    // batch runs out of: the form without a duplicate test — every index with distinct labels, and the
    // coarse stage of all — has 8 rows per lane (8 KB per wave instead of 16), as a ring (heap_replay_lanes_kernel);
    // with the plain kernel on 256 instead of 512 workgroups beside it the batch's kernels fit
    // the chip's LDS.  The TWIN form keeps 16-block segments (replay-bound: 15.5 against 14.9 M).
    constexpr int SEG = 16;
    int nseg = (Q.total + SEG - 1) / SEG;
    int max_nseg = nseg;
    for (int o = LW / 2; o > 0; o >>= 1) {
        int other = __shfl_xor(max_nseg, o, 64);
        max_nseg = other > max_nseg ? other : max_nseg;
    }
    max_nseg = __builtin_amdgcn_readfirstlane(max_nseg);

    // DEDUPE / TWIN: slot cursor (monotonic) over the LDS slot table
    int s = 0;
    if (DEDUPE || TWIN) {
        for (int t = 0; t < S; t++) {
            const int e0 = Q.prefix[t], e1 = Q.prefix[t + 1];
            SE[t * LW + lane] = Q.valid ? e1 : 0x7fffffff;
            SB[t * LW + lane] = (int)(slot_label_off[Q.qs * S + t] - 16 * (int64_t)e0);
        }
    }
    // TWIN: f (see the head of the kernel), pm = bit (list & 63) of every list replayed before slot s
    int f = 0x7fffffff;
    uint64_t pm = 0;
    int se_cur = 0x7fffffff, sb_cur = 0;      // SE[s], SB[s] of the slot the cursor is in
    if (TWIN && S > 0) {
        se_cur = Q.valid ? Q.prefix[1] : 0x7fffffff;
        sb_cur = (int)(slot_label_off[Q.qs * S] - 16 * (int64_t)Q.prefix[0]);
    }
    if (TWIN) {
        const int64_t *pq = tw.probes + Q.qc * S;
        for (int g = 0; g < S4; g++) {
            uint4 pl;
            pl.x = (uint32_t)(int)pq[4 * g];                                    // (a probe of -1 flags its query: `skip`)
            pl.y = 4 * g + 1 < S ? (uint32_t)(int)pq[4 * g + 1] : 0x7fffffffu;
            pl.z = 4 * g + 2 < S ? (uint32_t)(int)pq[4 * g + 2] : 0x7fffffffu;
            pl.w = 4 * g + 3 < S ? (uint32_t)(int)pq[4 * g + 3] : 0x7fffffffu;
            PL[g * LW + lane] = pl;
        }
        for (int g = 0; g < BMW; g++) BM[g * LW + lane] = 0;
    }

    // Segment g + 1 (16 blocks per lane, each lane from its own row, + its 16 block minima) is
    // fetched into REGISTERS while segment g is replayed and dropped into the LDS staging rows
    // ST[k][lane] — from where the replay picks blocks by a run-time index — when segment g is
    // done.  (Round 1 staged by LDS-DMA, global_load_lds_dwordx4: the compiler must put
    // s_waitcnt vmcnt(0) in front of every LDS read that follows such an operation — it cannot
    // tell that the read does not alias the DMA's target — so the "next" segment was always
    // waited for before the current one was touched.  Fetching only the blocks whose minimum
    // passes the previous bound, predicated per lane, was measured slower: the exec-mask
    // handling costs more than the addresses it saves; profiles/r02_replay_phases.md.)
    uint4 nx[SEG];
    uint4 mins_nx = make_uint4(0, 0, 0, 0);
#define TK_FETCH_BLOCKS(g_)                                                       \
    {                                                                             \
        _Pragma("unroll") for (int k = 0; k < SEG; k++) nx[k] = Q.block(SEG * (g_) + k); \
    }
#pragma unroll
    for (int k = 0; k < SEG; k++) nx[k] = make_uint4(0, 0, 0, 0);
    // LAZY: the minima run TWO segments ahead, so that at the start of segment g those of g + 1 are in registers
    // and the FIRST block of g + 1 whose minimum passes the bound of now — a superset of what will pass then —
    // can be requested while segment g is replayed: on long lists ~1.3 blocks of a segment with any hit pass
    // (500 of 6 250 per query at 100M x 128), each was a dependent trip to memory of its own.
    uint4 mins_n2 = make_uint4(0, 0, 0, 0), pre = make_uint4(0, 0, 0, 0), pre_n = make_uint4(0, 0, 0, 0);
    int pre_blk = -1, pre_n_blk = -1;
    if (max_nseg > 0) {
        mins_nx = Q.mins16(0);
        if (LAZY && max_nseg > 1) mins_n2 = Q.mins16(1);
        if (!LAZY) TK_FETCH_BLOCKS(0)
    }
    int rounds = 0;               // wave-uniform: iterations of the insert loop (each a dependent chain: roofline.replay)
    for (int g = 0; g < max_nseg; g++) {
        if (!LAZY) {
#pragma unroll
            for (int k = 0; k < SEG; k++) ST[k * LW + lane] = nx[k];
        }
        const uint4 mins_cur = mins_nx;
        if (LAZY) {
            mins_nx = mins_n2;                              // segment g + 1: requested an iteration ago
            if (g + 2 < max_nseg) mins_n2 = Q.mins16(g + 2);
            pre = pre_n;
            pre_blk = pre_n_blk;
            pre_n_blk = -1;
            if (g + 1 < max_nseg) {
                int kn = Q.total - 16 * (g + 1);
                kn = kn < 0 ? 0 : (kn > 16 ? 16 : kn);
                uint32_t hn = mask_lt16_swar<SIGNED>(mins_nx, bb);
                hn &= kn >= 16 ? 0xffffu : ((1u << kn) - 1u);
                if (hn) {
                    pre_n_blk = 16 * (g + 1) + __builtin_ctz(hn);
                    pre_n = Q.block(pre_n_blk);
                }
            }
        } else if (g + 1 < max_nseg) {
            mins_nx = Q.mins16(g + 1);
            TK_FETCH_BLOCKS(g + 1)
        }
        int kmax = Q.total - SEG * g;
        kmax = kmax < 0 ? 0 : (kmax > SEG ? SEG : kmax);
        // blocks whose minimum is below the bound at segment start: a superset of the
        // blocks the reference enters (the bound only decreases)
        uint32_t hit = mask_lt16_swar<SIGNED>(mins_cur, bb);
        hit &= kmax >= SEG ? ((1u << SEG) - 1u) : ((1u << kmax) - 1u);
        uint32_t bits = 0;
        uint4 dd = make_uint4(0, 0, 0, 0);
        int cur = 0;
        uint32_t lab_next = 0;        // DEDUPE: label of the lowest pending row, fetched ahead
        int lab_base = 0;             //         labels32 index of row 0 of the current block
        int tw_next = -1;             // TWIN: list of the lowest pending row's first other copy, fetched ahead
        // next block of this segment with a byte below the live bound (a macro, not a lambda: inline at the head of the
        // round loop the compiler folds this loop into it; as a lambda it stayed a nested loop of its own and the form
        // without a duplicate test lost 7 % alone).  `pos < n` (:111): the rows that pad a list's last chunk were set to the
        // largest value by pad_fix_kernel and can never be below a bound — no row count, and with distinct labels no slot
        // cursor at all, is needed; cmp_mask: _fast_pq_256.pyx:81-90; DEDUPE / TWIN: the slot cursor steps over empty lists,
        // TWIN: the list left joins the set, rows of the first probed list have no earlier copy (nothing to ask)
#define TK_ADVANCE() \
            while (bits == 0 && hit) { \
                const int k = __builtin_ctz(hit); \
                hit &= hit - 1; \
                cur = SEG * g + k; \
                if (LAZY) { \
                    if (cur == pre_blk) dd = pre; \
                    else dd = Q.block(cur); \
                } else { \
                    dd = ST[k * LW + lane]; \
                } \
                bits = mask_lt16_swar<SIGNED>(dd, bb); \
                if (DEDUPE && bits) { \
                    while (cur >= SE[s * LW + lane]) s++; \
                    lab_base = SB[s * LW + lane] + 16 * cur; \
                    lab_next = (uint32_t)labels32[(int64_t)lab_base + __builtin_ctz(bits)]; \
                } \
                if (TWIN && bits) { \
                    while (cur >= se_cur) { \
                        const int cs = ((const int *)PL)[(((s >> 2) * LW + lane) << 2) + (s & 3)]; \
                        if (BMW) BM[(cs >> 5) * LW + lane] |= 1u << (cs & 31); \
                        else pm |= 1ull << (cs & 63); \
                        s++; \
                        se_cur = SE[s * LW + lane]; \
                        sb_cur = SB[s * LW + lane]; \
                    } \
                    lab_base = sb_cur + 16 * cur; \
                    if (s > 0) tw_next = tw.list[(lab_base + __builtin_ctz(bits)) * tw.w]; \
                } \
            }
        // One round: every lane without a pending candidate looks for its next block (`advance`, one call site); the
        // lanes with one take it through the duplicate test and `insert` — register levels, then LDS levels.  TWIN
        // with staged blocks (EARLY) looks between the two: the new root — the bound behind the block — is known
        // after the register levels, the block is in LDS, and the request for the next candidate's row of the twin
        // table is then in flight while the sift goes through the LDS levels (a trip to memory in every round
        // otherwise: 1.7 us per round against 1.0 of the form without the test; 1.35 this way).  Requesting a LAZY
        // form's next passing block ahead of the insert in the same manner was measured and is not kept (100M x 128:
        // 6.27 M queries/s with, 6.27 without, same box).
        constexpr bool EARLY = TWIN && !LAZY;
        for (;;) {
            if (!EARLY) {
                TK_ADVANCE()
                if (__builtin_amdgcn_ballot_w64(bits != 0) == 0) break;
                rounds++;
            }
            int j = 0;             // > 0: the sift goes on below node j (3..6), whose children are in LDS
            uint32_t entry = 0;
            int v = 0;
            if (bits) {   // one insert per lane with a pending candidate
                const int r = __builtin_ctz(bits);
                bits &= bits - 1;
                const uint32_t by = block_byte(dd, r);
                uint32_t low = (uint32_t)(16 * cur + r);
                bool dup = false;
                if (DEDUPE) {
                    const uint32_t label = lab_next;
                    if (bits) lab_next = (uint32_t)labels32[(int64_t)lab_base + __builtin_ctz(bits)];
                    // `if i == indices[j]: return` over every slot, _fast_pq.pyx:284-287, answered by
                    // a hash set of the labels in the heap instead of a scan of all R slots (with
                    // any cheaper pre-filter some lane of 64 passes it in every round, and the
                    // scan then runs for the whole wave: it was 1.0 of the kernel's 2.2 ms,
                    // profiles/r02_replay_phases.md).  Two candidate buckets of four labels per
                    // label, the emptier one takes it; a label that finds both full is only kept in
                    // LAB and switches its lane to the full scan (exactness never depends on the
                    // set: LAB always holds every slot's label).
                    const TkBucketPair lb = tk_label_bucket_pair(label);
                    const int b1 = lb.b1, b2 = lb.b2;
                    const uint4 x1 = TB[b1 * LW + lane], x2 = TB[b2 * LW + lane];
                    dup = (x1.x == label) | (x1.y == label) | (x1.z == label) | (x1.w == label) |
                          (x2.x == label) | (x2.y == label) | (x2.z == label) | (x2.w == label) |
                          (sh0 == label) | (sh1 == label) | (sh2 == label) | (sh3 == label);
                    if (tb_ovf) {
#pragma unroll 4
                        for (int g = 0; g < R4; g++) {
                            const uint4 lv = ((const uint4 *)LAB)[g * LW + lane];
                            dup |= (lv.x == label) | (lv.y == label) | (lv.z == label) | (lv.w == label);
                        }
                    }
                    low = hp.h0 & 0x00ffffffu;            // the evicted root's slot
                    const uint32_t gone = TK_LAB(low); // label leaving with the root
                    if (!dup) {
                        if (gone != 0xffffffffu) {     // out of its bucket (if it ever got into one)
                            const TkBucketPair gb = tk_label_bucket_pair(gone);
                            const int g1 = gb.b1, g2 = gb.b2;
                            const uint4 y1 = TB[g1 * LW + lane], y2 = TB[g2 * LW + lane];
                            const int p1 = y1.x == gone ? 0 : y1.y == gone ? 1 : y1.z == gone ? 2 : y1.w == gone ? 3 : -1;
                            const int p2 = y2.x == gone ? 0 : y2.y == gone ? 1 : y2.z == gone ? 2 : y2.w == gone ? 3 : -1;
                            if (p1 >= 0) ((uint32_t *)TB)[(g1 * LW + lane) * 4 + p1] = 0xffffffffu;
                            else if (p2 >= 0) ((uint32_t *)TB)[(g2 * LW + lane) * 4 + p2] = 0xffffffffu;
                            else {
                                sh0 = sh0 == gone ? ~0u : sh0; sh1 = sh1 == gone ? ~0u : sh1;
                                sh2 = sh2 == gone ? ~0u : sh2; sh3 = sh3 == gone ? ~0u : sh3;
                            }
                        }
                        // x1 / x2 were read before that removal: an entry it freed still looks taken,
                        // which can only cost an unnecessary overflow, never a wrong placement
                        const int e1 = (x1.x == ~0u) + (x1.y == ~0u) + (x1.z == ~0u) + (x1.w == ~0u);
                        const int e2 = (x2.x == ~0u) + (x2.y == ~0u) + (x2.z == ~0u) + (x2.w == ~0u);
                        const bool first = e1 >= e2;
                        const uint4 xs = first ? x1 : x2;
                        const int pe = xs.x == ~0u ? 0 : xs.y == ~0u ? 1 : xs.z == ~0u ? 2 : xs.w == ~0u ? 3 : -1;
                        if (pe >= 0) ((uint32_t *)TB)[((first ? b1 : b2) * LW + lane) * 4 + pe] = label;
                        else if (sh0 == ~0u) sh0 = label;
                        else if (sh1 == ~0u) sh1 = label;
                        else if (sh2 == ~0u) sh2 = label;
                        else if (sh3 == ~0u) sh3 = label;
                        else tb_ovf = true;
                        TK_LAB(low) = label;
                    }
                }
                entry = (by << 24) | low;
                v = entry_val<SIGNED>(entry);
                if (TWIN && s > 0) {
                    const int row = lab_base + r;                   // the candidate's row in the twin table
                    int c = tw_next;
                    if (bits) tw_next = tw.list[(lab_base + __builtin_ctz(bits)) * tw.w];
#pragma nounroll
                    for (int u = 0; u < tw.w && !dup; u++) {
                        if (u > 0) c = tw.list[row * tw.w + u];
                        if (c < 0) break;                           // no further copies
                        // was list c replayed before this one?
                        if (BMW) {
                            if (!((BM[(c >> 5) * LW + lane] >> (c & 31)) & 1u)) continue;
                        } else if (!((pm >> (c & 63)) & 1ull)) continue;
                        if (BMW && v < f) { dup = true; break; }    // nothing of this value has ever left
                        int t = -1;                                 // its slot (the mask: exactly; the bitmap: for the position)
#pragma nounroll
                        for (int g = 0; g < S4; g++) {
                            const uint4 pl = PL[g * LW + lane];
                            t = ((int)pl.x == c && 4 * g < s) ? 4 * g : t;
                            t = ((int)pl.y == c && 4 * g + 1 < s) ? 4 * g + 1 : t;
                            t = ((int)pl.z == c && 4 * g + 2 < s) ? 4 * g + 2 : t;
                            t = ((int)pl.w == c && 4 * g + 3 < s) ? 4 * g + 3 : t;
                        }
                        if (t < 0) continue;
                        if (v < f) { dup = true; break; }           // nothing of this value has ever left
                        // the earlier copy as an entry: same value, its position in this query's rows
                        const uint32_t E = (by << 24) | (uint32_t)(16 * Q.prefix[t] + tw.off[row * tw.w + u]);
                        if (v > f) {
                            dup = hp.h0 == E;                          // only the root can be above f
                        } else {
                            bool found = (hp.h0 == E) | (hp.h1 == E) | (hp.h2 == E) | (hp.h3 == E) | (hp.h4 == E) | (hp.h5 == E) | (hp.h6 == E);
#pragma nounroll
                            for (int jj = 7; jj < R; jj++) found |= H[jj * LW + lane] == E;
                            dup = found;
                        }
                    }
                }
                if (TWIN && !dup) {
                    const int root = entry_val<SIGNED>(hp.h0);
                    f = root < f ? root : f;
                }
                // insert, _fast_pq.pyx:291-307: levels 0-2 in registers, the rest in LDS
                if (!dup) {
                    j = hp.reg_levels(entry, v);
                    if (j && !EARLY) hp.lds_levels(j, entry, v);           // (EARLY: behind the look-ahead below)
                }
                // refresh after the block, :123 (EARLY: the new root is known behind the register levels — the bound
                // does not wait for the levels below)
                if (bits == 0) {
                    bound = hp.h0 >> 24;
                    bb = bound_bytes<SIGNED>(bound);
                    b_plain = cur < Q.plain0 ? bound : b_plain;
                }
            }
            if (EARLY) {
                TK_ADVANCE()
                if (j) hp.lds_levels(j, entry, v);
                if (__builtin_amdgcn_ballot_w64(bits != 0) == 0) break;
                rounds++;
            }
        }
    }
#undef TK_ADVANCE
#undef TK_FETCH_BLOCKS
    lanes_finish<SIGNED, DEDUPE, LW>(Q, hp, LAB, b_plain, rounds, max_nseg, dbg, nq, skip, flag_list, plain0_arr, qlim,
                                     slot_label_off, S, labels, heap_idx, heap_val);
}
#undef TK_LAB

// one bit per list and query where that is at most 32 KB per wave of 64 queries (4096 lists)
int tk_lanes_twin_bm_words(int64_t n_lists) { return n_lists <= 4096 ? (int)((n_lists + 31) / 32) : 0; }
// (both rules ask for the BUDGET above — a 64-query wave with 16 KiB of staging — not for the launch size of the
// form that will run: they decide which replay an index gets, and that is behaviour)
int tk_lanes_twin_fits(int R, int S, int64_t n_lists)
{
    return R <= TK_LANES_MAX_R && tk_lanes_budget(false, R, S, tk_lanes_twin_bm_words(n_lists)) <= TK_LANES_LDS_MAX;
}

int tk_lanes_dedupe_fits(int R, int S)
{
    return R <= TK_LANES_MAX_R_DEDUPE && tk_lanes_budget(true, R, S, 0) <= TK_LANES_LDS_MAX;
}

// pad_fix_kernel, then the form's kernel: one query-wave of LW queries per workgroup (multi-wave workgroups are placed
// only when a whole CU has room, which next to the persistent scan kernels means at their launch boundaries)
template <bool SIGNED>
static void launch_lanes(const TkReplayJob &j, const TkLanesOpts &o, const TkPlainCheck &c, const TkTwins &tw,
                         bool dedupe, bool twin, int LW, size_t lds, hipStream_t s)
{
    const int64_t nq = j.nq;
    {   // padding rows out of the way first (the kernels below no longer test `pos < n`)
        const int64_t items = nq * j.S;
        const unsigned pg = (unsigned)((items + 255) / 256);
        if (items > 0)
            hipLaunchKernelGGL(pad_fix_kernel<SIGNED>, dim3(pg), dim3(256), 0, s, (uint4 *)j.dist, j.cap, nq,
                               j.slot_prefix, j.slot_n, j.S, j.slots_uniform, (uint8_t *)j.mins, j.cap_min, c.flag_list);
    }
    const dim3 grid((unsigned)((nq + LW - 1) / LW));
#define TK_LAUNCH_SEG(...)                                                                                            \
    hipLaunchKernelGGL((heap_replay_lanes_seg_kernel<SIGNED, __VA_ARGS__>), grid, dim3(64), lds, s, j.dist, j.cap, nq, \
                       j.slot_prefix, j.slot_label_off, j.S, j.labels, j.heap_idx, j.heap_val, j.R, j.slots_uniform,  \
                       o.skip, j.mins, j.cap_min, o.labels32, o.counters, c.plain0, c.qlim, tw, c.flag_list)
    if (dedupe) TK_LAUNCH_SEG(true, 32);
    else if (twin && o.lazy) TK_LAUNCH_SEG(false, 64, true, true);
    else if (twin) TK_LAUNCH_SEG(false, 64, false, true);
    else if (o.lazy) TK_LAUNCH_SEG(false, 64, true);
    else
        hipLaunchKernelGGL(heap_replay_lanes_kernel<SIGNED>, grid, dim3(64), lds, s, j.dist, j.cap, nq, j.slot_prefix,
                           j.slot_label_off, j.S, j.labels, j.heap_idx, j.heap_val, j.R, j.slots_uniform, o.skip, j.mins,
                           j.cap_min, o.counters, c.plain0, c.qlim, c.flag_list);
#undef TK_LAUNCH_SEG
}

int tk_launch_heap_replay_lanes(const TkReplayJob &j, const TkLanesOpts &o, hipStream_t s)
{
    const int64_t nq = j.nq;
    const int R = j.R, S = j.S;
    if (nq == 0 || R == 0) return 0;
    TkPlainCheck c = o.check;
    if (!c.plain0 || !c.qlim || !o.skip || !j.signd) c.plain0 = c.qlim = nullptr;
    const int dedupe = o.labels32 != nullptr;
    const TkTwins *t = o.twins;
    const TkTwins tw = !dedupe && t && t->w > 0 && t->list && t->off && t->probes && !j.slots_uniform ? *t : TkTwins();
    const bool twin = tw.w > 0;
    // Queries per wave: 64, or 32 with the duplicate test — a 64-query wave then needs 140+ KB of
    // LDS at R = 111: one workgroup per CU, and the two replay kernels of the pipelined mode (2 x 157
    // workgroups on 256 CUs) waited for each other's CUs (1.6 ms alone became 2.9 ms in the
    // pipeline); half-filled waves (lanes 32..63 exit at once) halve every per-lane column: two
    // workgroups per CU.  (Measured and dropped, profiles/HISTORY.md: 32- and 16-query waves for
    // distinct labels and for the coarse replay, 2-4 query-waves per workgroup, blocks fetched only
    // where their minimum passes, s_setprio below 3.)
    const int LWr = dedupe ? 32 : 64;
    const size_t lds = tk_lanes_lds(dedupe, twin, o.lazy != 0, LWr, R, S, tw.bm_words).bytes;
    static bool attr_set = false;
    if (!attr_set) {
        const void *fns[] = {(const void *)heap_replay_lanes_kernel<true>,
                             (const void *)heap_replay_lanes_kernel<false>,
                             (const void *)heap_replay_lanes_seg_kernel<true, true, 32>,
                             (const void *)heap_replay_lanes_seg_kernel<false, true, 32>,
                             (const void *)heap_replay_lanes_seg_kernel<true, false, 64, true>,
                             (const void *)heap_replay_lanes_seg_kernel<false, false, 64, true>,
                             (const void *)heap_replay_lanes_seg_kernel<true, false, 64, false, true>,
                             (const void *)heap_replay_lanes_seg_kernel<false, false, 64, false, true>,
                             (const void *)heap_replay_lanes_seg_kernel<true, false, 64, true, true>,
                             (const void *)heap_replay_lanes_seg_kernel<false, false, 64, true, true>};
        for (const void *f : fns)
            if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
                hipSuccess)
                return -1;
        attr_set = true;
    }
    if (j.signd) launch_lanes<true>(j, o, c, tw, dedupe, twin, LWr, lds, s);
    else launch_lanes<false>(j, o, c, tw, dedupe, twin, LWr, lds, s);
    return 0;
}
