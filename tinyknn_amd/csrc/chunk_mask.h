// chunk_mask.h — the device bodies the restricting passes share (allow.hip: one set per call; rows.hip: one excluded
// row per query; groups.hip: one group per query; tags.hip: one tag mask per query; between.hip: one interval per query
// and value column).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// keep: bit r set = row r of the chunk stays.  A chunk whose 16 bits are all set is not touched; one with none set is
// written without being read; else the bytes of the rows that leave take the heap's empty value (127 signed, 255
// unsigned) and the chunk's minimum byte is recomputed (the replays' LAZY form and the block-minimum skips read it).
template <bool SIGNED>
__device__ __forceinline__ void tk_mask_chunk(uint4 *__restrict__ d, uint8_t *__restrict__ m, uint32_t keep16)
{
    const uint32_t fill = SIGNED ? 0x7f7f7f7fu : 0xffffffffu;
    const uint32_t b = keep16;
    if (b == 0xffffu) return;
    if (b == 0) {
        *d = make_uint4(fill, fill, fill, fill);
        *m = (uint8_t)fill;
        return;
    }
    const uint4 v = *d;
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    int mn = SIGNED ? 127 : 255;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        // nibble j of the row bits -> 0xff in the bytes of the rows that stay
        const uint32_t keep = (((b >> (4 * j)) & 0xfu) * 0x00204081u & 0x01010101u) * 0xffu;
        w[j] = (w[j] & keep) | (fill & ~keep);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t y = (w[j] >> (8 * t)) & 0xffu;
            const int x = SIGNED ? (int)(int8_t)y : (int)y;
            mn = x < mn ? x : mn;
        }
    }
    *d = make_uint4(w[0], w[1], w[2], w[3]);
    *m = (uint8_t)mn;
}

// The query q that workgroup (or thread group) i of a pass works on: i itself, or entry i of only = [count, q_0, q_1,
// ...] (the exact re-scan of flagged queries rewrote just their rows: rescan_flagged).  false: none, the caller returns.
template <typename I>
__device__ __forceinline__ bool tk_pass_query(I i, const int *__restrict__ only, int64_t &q)
{
    q = i;
    if (!only) return true;
    if (i >= only[0]) return false;
    q = only[1 + i];
    return true;
}

// Batch row `row`'s entry of a per-query array: a holds rows [0, n_a) of the batch, b the rows behind them (a pair of
// calls).  false: that call named no array, the query is unrestricted.
template <typename T>
__device__ __forceinline__ bool tk_pass_entry(const T *__restrict__ a, const T *__restrict__ b, int64_t n_a,
                                              int64_t row, T &out)
{
    const T *p = row < n_a ? a : b;
    if (!p) return false;
    out = p[row < n_a ? row : row - n_a];
    return true;
}

// One workgroup on query q; threads stride over the query's contiguous chunk range [0, slot_prefix[S]) of dist / mins,
// the slot prefix in LDS (S + 1 ints of dynamic LDS), a binary search to the slot, slot_chunk0 to the global chunk c.
// keep(c): the chunk's 16-bit keep mask, applied by tk_mask_chunk.  Every thread of the workgroup comes here or none.
template <bool SIGNED, typename Keep>
__device__ __forceinline__ void tk_mask_probed(uint4 *__restrict__ dist, int64_t cap, uint8_t *__restrict__ mins,
                                               int64_t cap_min, const int *__restrict__ slot_prefix,
                                               const int64_t *__restrict__ slot_chunk0, int S, int64_t q, Keep keep)
{
    extern __shared__ int pre[];        // S + 1
    for (int s = threadIdx.x; s <= S; s += blockDim.x) pre[s] = slot_prefix[q * (S + 1) + s];
    __syncthreads();
    const int total = pre[S];
    for (int f = threadIdx.x; f < total; f += blockDim.x) {
        int lo = 0, hi = S;     // largest lo with pre[lo] <= f (pre is non-decreasing, pre[0] = 0)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pre[mid] <= f) lo = mid; else hi = mid;
        }
        const uint32_t b = keep(slot_chunk0[q * S + lo] + (f - pre[lo]));
        tk_mask_chunk<SIGNED>(dist + q * cap + f, mins + q * cap_min + f, b);
    }
}

// A per-row value in list-position order: one workgroup per list, threads striding over the list's rows padded to
// whole chunks (coalesced reads of the labels, coalesced writes of the table).  table[16 c + r] = by_row[label of row r
// of global chunk c]; `fill` for the rows that pad a list's last chunk and for labels outside [0, N).
template <typename T>
__device__ __forceinline__ void tk_row_table(const int64_t *__restrict__ list_chunk_off,
                                             const int64_t *__restrict__ list_n, const int64_t *__restrict__ ids_off,
                                             const int64_t *__restrict__ ids, const T *__restrict__ by_row, int64_t N,
                                             T fill, T *__restrict__ table)
{
    const int64_t l = blockIdx.x;
    const int64_t c0 = list_chunk_off[l];
    const int64_t rows = (list_chunk_off[l + 1] - c0) * 16;     // padded to whole chunks
    const int64_t n = list_n[l];
    const int64_t io = ids_off[l];
    for (int64_t r = threadIdx.x; r < rows; r += blockDim.x) {
        T v = fill;
        if (r < n) {
            const int64_t lab = ids[io + r];
            if (lab >= 0 && lab < N) v = by_row[lab];
        }
        table[c0 * 16 + r] = v;
    }
}
