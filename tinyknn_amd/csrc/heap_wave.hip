// heap_wave.hip — the heap replays of ONE QUERY PER WAVE with the heap in LDS, general and packed, and the reference's heap
// primitives init_heap, insert, insert_is (_fast_pq.pyx:240-307).  heap.hip's head has the overview of all replays.
//
// The general kernel, one wavefront per query:
//
//   * the int8 distances were produced by adc_scan.hip (16 per chunk);
//   * a step covers 64 blocks (1024 codes): lane b holds block b's 16 bytes and
//     votes "some byte < bound" with the bound at step start.  The bound never
//     increases while the heap is a valid max-heap of 8-bit values, so the vote is
//     a superset of the blocks the reference would enter (when the caller hands
//     in arrays that are not such a heap, every block is examined instead);
//   * voted blocks are visited in ascending order; each is re-tested against the
//     live bound (= its true block-start bound, all earlier blocks being done),
//     passing lanes are inserted in lane order, the bound is refreshed after the
//     block, and the remaining votes are re-filtered;
//   * the heap (int64 id, int32 value) lives in LDS; the duplicate-label scan is a
//     64-lane compare + ballot, the sift-down runs wave-uniformly.
#include <stdlib.h>

#include "heap_common.h"

// The heap arrays are wave-uniform state; reading them through readfirstlane keeps
// the replay's control flow on the scalar unit.
__device__ __forceinline__ int32_t lds_i32(lds_vi32 *p)
{
    return __builtin_amdgcn_readfirstlane(*p);
}
__device__ __forceinline__ int64_t lds_i64(lds_vi64 *p)
{
    int64_t v = *p;
    uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// insert (_fast_pq.pyx:274-307).  Called by all 64 lanes with wave-uniform
// arguments.  Only lane 0 stores: 64 lanes storing to one address serialise in the
// LDS pipe (a 64-way same-bank write), and the accesses are volatile and
// in-order per wave, so every lane's later loads see lane 0's stores.
__device__ __forceinline__ void heap_insert(lds_vi64 *hidx, lds_vi32 *hval, int R,
                                            int64_t label, int32_t v, int lane)
{
    bool dup = false;
    for (int t = lane; t < R; t += 64) dup |= (hidx[t] == label);
    if (__builtin_amdgcn_ballot_w64(dup)) return;  // :284-287
    int j = 0;
    for (;;) {
        int nxt = j;
        int32_t nxt_val = v;
        int l = 2 * j + 1, r = 2 * j + 2;
        if (l < R) {
            int32_t vl = lds_i32(&hval[l]);
            if (vl > nxt_val) { nxt = l; nxt_val = vl; }
        }
        if (r < R) {
            int32_t vr = lds_i32(&hval[r]);
            if (vr > nxt_val) { nxt = r; nxt_val = vr; }
        }
        if (nxt == j) {
            if (lane == 0) { hval[j] = v; hidx[j] = label; }
            break;
        }
        const int64_t moved = lds_i64(&hidx[nxt]);
        if (lane == 0) { hval[j] = nxt_val; hidx[j] = moved; }
        j = nxt;
    }
}

// insert_is (_fast_pq.pyx:256-271)
__device__ __forceinline__ void heap_insert_is(lds_vi64 *hidx, lds_vi32 *hval,
                                               int R, int64_t label, int32_t v, int lane)
{
    bool dup = false;
    for (int t = lane; t < R; t += 64) dup |= (hidx[t] == label);
    if (__builtin_amdgcn_ballot_w64(dup)) return;
    int j = 0;
    while (j + 1 != R) {
        int32_t nv = lds_i32(&hval[j + 1]);
        if (!(nv > v)) break;
        const int64_t moved = lds_i64(&hidx[j + 1]);
        if (lane == 0) { hidx[j] = moved; hval[j] = nv; }
        j++;
    }
    if (lane == 0) { hidx[j] = label; hval[j] = v; }
}

// Workgroup = 4 independent waves (4 queries): gfx950 admits only ~8 workgroups
// per CU, so single-wave workgroups would cap residency at 2 waves per SIMD.
#define TK_HEAP_WAVES 4

template <bool SIGNED>
__global__ __launch_bounds__(64 * TK_HEAP_WAVES) void heap_replay_kernel(
    const uint4 *__restrict__ dist, int64_t cap, const int *__restrict__ slot_prefix,
    const int *__restrict__ slot_n, const int64_t *__restrict__ slot_label_off, int S,
    const int64_t *__restrict__ labels, int64_t *__restrict__ heap_idx,
    int32_t *__restrict__ heap_val, int R, int slots_uniform,
    const unsigned char *__restrict__ only_flagged, int64_t nq,
    const uint8_t *__restrict__ mins, int64_t cap_min)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = threadIdx.x >> 6;
    const size_t wstride = ((size_t)R * 12 + 15) & ~(size_t)15;
    lds_vi64 *hidx = LDS_PTR(lds_vi64, smem + wave * wstride);
    lds_vi32 *hval = LDS_PTR(lds_vi32, smem + wave * wstride + (size_t)R * 8);
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (q >= nq) return;   // wave-uniform; the kernel uses no workgroup barrier

    if (only_flagged) {
        // second pass behind the lane-per-query kernel: only the queries it skipped,
        // starting from a fresh heap
        if (!only_flagged[q]) return;
        for (int t = lane; t < R; t += 64) {
            hidx[t] = -1;
            hval[t] = SIGNED ? 127 : 255;
        }
    } else {
        for (int t = lane; t < R; t += 64) {
            hidx[t] = heap_idx[q * R + t];
            hval[t] = heap_val[q * R + t];
        }
    }
    // Is the incoming array a max-heap of values in the 8-bit range?  Then the
    // bound (low 8 bits of the root) can only go down and stale votes are safe.
    bool bad = false;
    for (int t = lane; t < R; t += 64) {
        int32_t v = hval[t];
        if (SIGNED ? (v < -128 || v > 127) : (v < 0 || v > 255)) bad = true;
        if (t > 0 && hval[(t - 1) >> 1] < v) bad = true;
    }
    const bool no_skip = __builtin_amdgcn_ballot_w64(bad) != 0;
    uint32_t bound = (uint32_t)lds_i32(&hval[0]) & 0xffu;  // _fast_pq_256.pyx:73

    const int64_t qs = slots_uniform ? 0 : q;  // one descriptor row shared by all queries
    const int *prefix = slot_prefix + qs * (S + 1);
    const uint4 *drow = dist + q * cap;
    const uint4 never = never16<SIGNED>();
    for (int s = 0; s < S; s++) {
        const int c0 = prefix[s];
        const int nchunks = prefix[s + 1] - c0;
        const int64_t n = slot_n[qs * S + s];
        const int64_t loff = slot_label_off[qs * S + s];
        const int64_t *lab = loff < 0 ? nullptr : labels + loff;
        // 64 blocks per step — or, with the scan's per-block minima and a heap whose bound can
        // only fall, 1024: lane j looks at the 16 minima of blocks [sbase + 16 j, +16) and only
        // groups that can hold a hit are entered, 16 blocks at a time (one long list against a
        // small heap, the flat DistanceTable.top: 977 steps of 1 KiB become 61 of 1 KiB of
        // minima plus the few groups that matter)
        const bool by_mins = mins != nullptr && !no_skip && (c0 & 15) == 0;
        const int width = by_mins ? 16 : 64;
        for (int sbase = 0; sbase < nchunks; sbase += by_mins ? 1024 : 64) {
          uint64_t groups = 1;
          if (by_mins) {
              const int gb = sbase + 16 * lane;
              bool gv = false;
              if (gb < nchunks) {
                  const uint4 m16 = *(const uint4 *)(mins + q * cap_min + c0 + gb);
                  gv = any_lt16<SIGNED>(m16, bound);
              }
              groups = __builtin_amdgcn_ballot_w64(gv);
          }
          while (groups) {
            const int gj = __builtin_ctzll(groups);
            groups &= groups - 1;
            const int base = by_mins ? sbase + 16 * gj : sbase;
            const int b = base + lane;
            const bool have = lane < width && b < nchunks;
            uint4 dd = never;
            if (have) dd = drow[c0 + b];
            bool vote = have && (no_skip || any_lt16<SIGNED>(dd, bound));
            uint64_t mask = __builtin_amdgcn_ballot_w64(vote);
            while (mask) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1;
                const uint32_t d0 = __builtin_amdgcn_readlane(dd.x, j);
                const uint32_t d1 = __builtin_amdgcn_readlane(dd.y, j);
                const uint32_t d2 = __builtin_amdgcn_readlane(dd.z, j);
                const uint32_t d3 = __builtin_amdgcn_readlane(dd.w, j);
                // the reference's cmp_mask of this block against the live bound
                uint32_t bits = 0;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    bits |= (uint32_t)byte_lt<SIGNED>(block_byte(d0, d1, d2, d3, r), bound) << r;
                }
                if (!bits) continue;
                const int64_t pos0 = 16 * (int64_t)(base + j);
                while (bits) {
                    const int r = __builtin_ctz(bits);
                    bits &= bits - 1;
                    const int64_t pos = pos0 + r;
                    if (pos < n) {  // _fast_pq_256.pyx:111
                        const int64_t label = lab ? lab[pos] : pos;
                        const uint32_t by = block_byte(d0, d1, d2, d3, r);
                        int32_t v = SIGNED ? (int32_t)(int8_t)by : (int32_t)by;
                        heap_insert(hidx, hval, R, label, v, lane);
                    }
                }
                bound = (uint32_t)lds_i32(&hval[0]) & 0xffu;  // :123
                if (!no_skip && mask) {
                    vote = vote && any_lt16<SIGNED>(dd, bound);
                    mask &= __builtin_amdgcn_ballot_w64(vote);
                }
            }
          }
        }
    }
    for (int t = lane; t < R; t += 64) {
        heap_idx[q * R + t] = hidx[t];
        heap_val[q * R + t] = hval[t];
    }
}

void tk_launch_heap_replay(const TkReplayJob &j, hipStream_t s)
{
    if (j.nq == 0 || j.R == 0) return;
    const size_t wstride = ((size_t)j.R * 12 + 15) & ~(size_t)15;
    int waves = (int)(64 * 1024 / wstride);   // large heaps: fewer query-waves per workgroup
    waves = waves < 1 ? 1 : (waves > TK_HEAP_WAVES ? TK_HEAP_WAVES : waves);
    size_t lds = wstride * waves;
    dim3 grid((unsigned)((j.nq + waves - 1) / waves)), block(64 * waves);
    const auto kernel = j.signd ? heap_replay_kernel<true> : heap_replay_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, lds, s, j.dist, j.cap, j.slot_prefix, j.slot_n, j.slot_label_off, j.S, j.labels,
                       j.heap_idx, j.heap_val, j.R, j.slots_uniform, /*only_flagged=*/(const unsigned char *)nullptr, j.nq,
                       j.mins, j.cap_min);
}

// ---------------------------------------------------------------------------
// Wave-per-query replay on packed entries: same preconditions as the
// lane-per-query kernel (fresh heap, labels cannot repeat), same entry format
// (value8 << 24 | flat position24), but the 64 lanes of a wave cooperate on ONE
// query: coalesced 1 KiB loads of 64 blocks, a ballot vote, the exact per-block
// mask from lanes 0..15, and a scalar-controlled sift-down over a heap that is R
// dwords of LDS (children l, l+1 are adjacent dwords).  Far fewer instructions per
// insert than heap_replay_kernel (no label array, no duplicate scan, one LDS word
// per node), which is what bounds that kernel at 10^4 concurrent queries.
// DEDUPE: labels may repeat among a query's lists (IVF.build(n_probes >= 2), or a
// wrapped probe id).  The low 24 bits of an entry are then a SLOT number instead of
// a position; lab[slot] holds the int64 label, `insert` first runs the reference's
// duplicate test over lab[] with all 64 lanes, and a new entry takes over the slot
// of the root it evicts.  `flags`/`run_if`: process query q iff flags[q] == run_if.
template <bool SIGNED, bool DEDUPE>
__global__ __launch_bounds__(64 * TK_HEAP_WAVES) void heap_replay_packed_kernel(
    const uint4 *__restrict__ dist, int64_t cap, const int *__restrict__ slot_prefix,
    const int *__restrict__ slot_n, const int64_t *__restrict__ slot_label_off, int S,
    const int64_t *__restrict__ labels, int64_t *__restrict__ heap_idx,
    int32_t *__restrict__ heap_val, int R, int slots_uniform,
    const unsigned char *__restrict__ flags, int run_if, int64_t nq, const int *__restrict__ flag_list,
    volatile int *host_count)
{
    // (the count of the flagged queries to the page-locked word the host polls: plain_scan's state machine)
    if (host_count && flag_list && blockIdx.x == 0 && threadIdx.x == 0) *host_count = flag_list[0];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = threadIdx.x >> 6;
    const size_t wstride = DEDUPE ? (((size_t)R * 12 + 15) & ~(size_t)15) : (size_t)R * 4;
    lds_vi64 *lab = LDS_PTR(lds_vi64, smem + wave * wstride);                       // [R] (DEDUPE)
    lds_vu32 *H = LDS_PTR(lds_vu32, smem + wave * wstride + (DEDUPE ? (size_t)R * 8 : 0));  // [R]
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (q >= nq) return;   // wave-uniform; no workgroup barrier below
    if (flags && (run_if < 0 ? flags[q] == 0 : (int)flags[q] != run_if)) return;      // run_if < 0: every flagged query
    const int64_t qs = slots_uniform ? 0 : q;
    const int *prefix = slot_prefix + qs * (S + 1);
    const uint4 *drow = dist + q * cap;

    const uint32_t fresh_val = SIGNED ? 0x7f000000u : 0xff000000u;
    for (int t = lane; t < R; t += 64) {
        H[t] = fresh_val | (DEDUPE ? (uint32_t)t : 0x00ffffffu);
        if (DEDUPE) lab[t] = -1;
    }
    uint32_t bound = SIGNED ? 0x7fu : 0xffu;
    const uint4 never = never16<SIGNED>();
    for (int s = 0; s < S; s++) {
        const int c0 = prefix[s];
        const int nchunks = prefix[s + 1] - c0;
        const int n = slot_n[qs * S + s];
        const int64_t loff = slot_label_off[qs * S + s];
        const int64_t *labp = loff < 0 ? nullptr : labels + loff;
        for (int base = 0; base < nchunks; base += 64) {
            const int b = base + lane;
            const bool have = b < nchunks;
            uint4 dd = never;
            if (have) dd = drow[c0 + b];
            bool vote = have && any_lt16<SIGNED>(dd, bound);
            uint64_t mask = __builtin_amdgcn_ballot_w64(vote);
            // DEDUPE: the 16 labels of a voted block are fetched by lanes 0..15 with one
            // vector load, one block ahead of the block being replayed
            auto load_labels = [&](int jb) -> int64_t {
                const int64_t inl = 16 * (int64_t)(base + jb) + lane;
                if (lane >= 16 || inl >= n) return -2;   // never a label
                return labp ? labp[inl] : inl;
            };
            int j_pref = -1;
            int64_t lab_pref = -2;
            if (DEDUPE && mask) {
                j_pref = __builtin_ctzll(mask);
                lab_pref = load_labels(j_pref);
            }
            while (mask) {
                const int j = __builtin_ctzll(mask);
                mask &= mask - 1;
                int64_t lab_cur = -2;
                if (DEDUPE) {
                    lab_cur = (j == j_pref) ? lab_pref : load_labels(j);
                    if (mask) {
                        j_pref = __builtin_ctzll(mask);
                        lab_pref = load_labels(j_pref);
                    }
                }
                const uint32_t d0 = __builtin_amdgcn_readlane(dd.x, j);
                const uint32_t d1 = __builtin_amdgcn_readlane(dd.y, j);
                const uint32_t d2 = __builtin_amdgcn_readlane(dd.z, j);
                const uint32_t d3 = __builtin_amdgcn_readlane(dd.w, j);
                // lane r < 16 tests row r against the live bound (= block-start bound)
                const uint32_t by = block_byte(d0, d1, d2, d3, lane);
                const int rows = n - 16 * (base + j);   // `pos < n`
                const bool lt = lane < 16 && lane < rows && byte_lt<SIGNED>(by, bound);
                uint32_t bits = (uint32_t)__builtin_amdgcn_ballot_w64(lt);
                if (!bits) continue;
                const uint32_t pos0 = (uint32_t)(16 * (c0 + base + j));
                while (bits) {
                    const int r = __builtin_ctz(bits);
                    bits &= bits - 1;
                    const uint32_t byr = __builtin_amdgcn_readlane(by, r);
                    uint32_t low = pos0 + (uint32_t)r;
                    if (DEDUPE) {
                        const uint32_t llo = __builtin_amdgcn_readlane((uint32_t)lab_cur, r);
                        const uint32_t lhi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)lab_cur >> 32), r);
                        const int64_t label = (int64_t)(((uint64_t)lhi << 32) | llo);
                        bool dup = false;   // `if i == indices[j]: return`, _fast_pq.pyx:284-287
                        for (int t = lane; t < R; t += 64) dup |= (lab[t] == label);
                        if (__builtin_amdgcn_ballot_w64(dup)) continue;
                        // the new entry inherits the slot of the root it replaces
                        low = __builtin_amdgcn_readfirstlane(H[0]) & 0x00ffffffu;
                        if (lane == 0) lab[low] = label;
                    }
                    const uint32_t entry = (byr << 24) | low;
                    const int v = entry_val<SIGNED>(entry);
                    int jn = 0;
                    for (;;) {  // insert, _fast_pq.pyx:291-307
                        const int l = 2 * jn + 1;
                        if (l >= R) { if (lane == 0) H[jn] = entry; break; }
                        uint32_t el = H[l];
                        uint32_t er = (l + 1 < R) ? H[l + 1] : 0u;
                        el = __builtin_amdgcn_readfirstlane(el);
                        er = __builtin_amdgcn_readfirstlane(er);
                        int nxt = jn, nv = v;
                        uint32_t ne = entry;
                        if (entry_val<SIGNED>(el) > nv) { nxt = l; nv = entry_val<SIGNED>(el); ne = el; }
                        if (l + 1 < R && entry_val<SIGNED>(er) > nv) { nxt = l + 1; ne = er; }
                        if (nxt == jn) { if (lane == 0) H[jn] = entry; break; }
                        if (lane == 0) H[jn] = ne;  // one lane: same-address stores serialise
                        jn = nxt;
                    }
                }
                bound = __builtin_amdgcn_readfirstlane(H[0]) >> 24;  // :123
                if (mask) {
                    vote = vote && any_lt16<SIGNED>(dd, bound);
                    mask &= __builtin_amdgcn_ballot_w64(vote);
                }
            }
        }
    }
    // heap arrays out
    const int64_t *loffs = slot_label_off + qs * S;
    for (int t = lane; t < R; t += 64) {
        const uint32_t e = H[t];
        const uint32_t pos = e & 0x00ffffffu;
        heap_idx[q * R + t] = DEDUPE ? (int64_t)lab[pos] : resolve_position(pos, prefix, loffs, S, labels);
        heap_val[q * R + t] = entry_val<SIGNED>(e);
    }
}

void tk_launch_heap_replay_packed(const TkReplayJob &j, const unsigned char *flags, int run_if, bool dedupe,
                                  hipStream_t s, const int *flag_list, int *host_count)
{
    if (j.nq == 0 || j.R == 0) return;
    const size_t wstride = dedupe ? (((size_t)j.R * 12 + 15) & ~(size_t)15) : (size_t)j.R * 4;
    int waves = (int)(64 * 1024 / wstride);
    waves = waves < 1 ? 1 : (waves > TK_HEAP_WAVES ? TK_HEAP_WAVES : waves);
    size_t lds = wstride * waves;
    dim3 grid((unsigned)((j.nq + waves - 1) / waves)), block(64 * waves);
    const auto kernel = j.signd ? (dedupe ? heap_replay_packed_kernel<true, true> : heap_replay_packed_kernel<true, false>)
                                : (dedupe ? heap_replay_packed_kernel<false, true> : heap_replay_packed_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, j.dist, j.cap, j.slot_prefix, j.slot_n, j.slot_label_off, j.S, j.labels,
                       j.heap_idx, j.heap_val, j.R, j.slots_uniform, flags, run_if, j.nq, flag_list, host_count);
}

// ---------------------------------------------------------------------------
__global__ void heap_fill_kernel(int64_t *heap_idx, int32_t *heap_val, int64_t count, int32_t v)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        heap_idx[i] = -1;
        heap_val[i] = v;
    }
}

void tk_launch_heap_fill(int64_t *heap_idx, int32_t *heap_val, int64_t count, int32_t v,
                         hipStream_t s)
{
    if (count == 0) return;
    hipLaunchKernelGGL(heap_fill_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s,
                       heap_idx, heap_val, count, v);
}

__global__ __launch_bounds__(64) void heap_insert_kernel(int64_t *heap_idx, int32_t *heap_val,
                                                         int R, int64_t i, int32_t v, int is)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lds_vi64 *hidx = LDS_PTR(lds_vi64, smem);
    lds_vi32 *hval = LDS_PTR(lds_vi32, smem + (size_t)R * 8);
    const int lane = threadIdx.x;
    for (int t = lane; t < R; t += 64) {
        hidx[t] = heap_idx[t];
        hval[t] = heap_val[t];
    }
    if (is)
        heap_insert_is(hidx, hval, R, i, v, lane);
    else
        heap_insert(hidx, hval, R, i, v, lane);
    for (int t = lane; t < R; t += 64) {
        heap_idx[t] = hidx[t];
        heap_val[t] = hval[t];
    }
}

void tk_launch_heap_insert(int64_t *heap_idx, int32_t *heap_val, int R, int64_t i, int32_t v,
                           int is, hipStream_t s)
{
    hipLaunchKernelGGL(heap_insert_kernel, dim3(1), dim3(64), (size_t)R * 12, s, heap_idx,
                       heap_val, R, i, v, is);
}
