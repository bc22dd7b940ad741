// cap_select.h — at most m rows of any group among a query's ranked candidates (per_group=; the epilogue of the capped
// rescoring kernels of rescore.hip).  Extends IVF.query, ivf.py:154-163: the ids that bottom_k would return are walked
// in rank order and a candidate is kept while fewer than m of its group have been kept, up to k of them.
//
// A candidate is kept iff fewer than m candidates of its group rank BEFORE it (within a group the first m in rank
// order are exactly the kept ones), so nothing is walked serially: a lane counts, for its rank, the earlier entries
// with its group, and a ballot over 64 ranks in order turns the kept flags into output positions.
#pragma once
#include <stddef.h>
#include <stdint.h>

// What a capped launch carries beside the uncapped one's arguments.  groups: one id per row, by row id (n_rows of
// them).  m: one cap per query, <= 0 for none; m_b (or NULL): the caps of a second call's queries, batch rows n_a on.
struct TkCap {
    const int32_t *groups = nullptr;
    const int32_t *m = nullptr;
    const int32_t *m_b = nullptr;
    int64_t n_a = 0;
};

// bytes of LDS the selection needs behind a body's own: by rank, id (int64) | distance (T) | group (int32)
static inline size_t cap_lds_bytes(int R, size_t dist_size) { return (size_t)R * (8 + dist_size + 4); }

#ifdef __HIPCC__
// query qi's cap as a count that every earlier-entries count is below when there is none
__device__ __forceinline__ unsigned cap_of(const TkCap &cap, int64_t qi)
{
    const int32_t *p = (cap.m_b && qi >= cap.n_a) ? cap.m_b + (qi - cap.n_a) : (cap.m ? cap.m + qi : nullptr);
    const int m = p ? *p : 0;
    return m > 0 ? (unsigned)m : 0xffffffffu;
}

// The three LDS arrays of a capped body behind `base` (8-byte aligned), R entries each
template <typename T>
struct CapRanked {
    int64_t *id;
    T *dist;
    int32_t *group;
    __device__ __forceinline__ CapRanked(unsigned char *base, int R)
        : id((int64_t *)base), dist((T *)(base + (size_t)R * 8)), group((int32_t *)(base + (size_t)R * (8 + sizeof(T))))
    {
    }
};

// Every thread of the workgroup calls this once its candidates stand in `by` at their ranks 0 .. nc - 1 (dist only
// where od is given).  Writes row o[0 .. k): the kept ids in rank order, then -1; od (or NULL) beside them, +inf beside
// a -1; *count (or NULL): the number kept.  The first wave does the work: ranks in chunks of 64, in order, until k are
// kept — with few groups exhausted that is the first chunk, k <= 64.
template <typename T>
__device__ __forceinline__ void cap_select(const CapRanked<T> &by, int nc, int k, unsigned cap, int64_t *__restrict__ o,
                                           T *__restrict__ od, int *__restrict__ count)
{
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    int kept = 0;
    const uint64_t lower = (1ull << lane) - 1ull;
    for (int r0 = 0; r0 < nc && kept < k; r0 += 64) {
        const int r = r0 + lane;
        const bool have = r < nc;
        const int32_t g = by.group[have ? r : nc - 1];
        // the earlier entries of its group: in the chunks walked so far (every lane reads one address: a broadcast) ...
        unsigned before = 0;
#pragma unroll 4
        for (int u = 0; u < r0; u++) before += by.group[u] == g;
        // ... and in this chunk, a group at a time: the lanes that hold it count the ones below them
        uint64_t todo = __builtin_amdgcn_ballot_w64(have);
        while (todo) {
            const int32_t gj = __builtin_amdgcn_readlane(g, __builtin_ctzll(todo));
            const uint64_t same = __builtin_amdgcn_ballot_w64(have && g == gj);
            if (g == gj) before += __builtin_popcountll(same & lower);
            todo &= ~same;
        }
        const bool keep = have && before < cap;
        const uint64_t mask = __builtin_amdgcn_ballot_w64(keep);
        const int pos = kept + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (keep && pos < k) {
            o[pos] = by.id[r];
            if (od) od[pos] = by.dist[r];
        }
        kept += __builtin_popcountll(mask);
    }
    if (kept > k) kept = k;
    for (int t = kept + lane; t < k; t += 64) {
        o[t] = -1;
        if (od) od[t] = (T)__builtin_huge_valf();
    }
    if (lane == 0 && count) *count = kept;
}
#endif
