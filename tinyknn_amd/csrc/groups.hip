// groups.hip — every query of a batch restricted to its own group of rows
// (tk_index_set_groups / tk_index_query_batch[_dev]_ex3).
//
// What a group means: rows carry a group id, groups[r] in [0, 2^31 - 1).  A query with group g >= 0
// returns what the reference's IVF.query (ivf.py:106-163) returns when `insert` in query_pq runs only for labels
// with groups[label] == g — the allowed set "groups == g" of §3.8, for that query alone, and so the allow pass's
// move: every probed row of another group gets the heap's empty value in the distance bytes, behind the list scans
// and every re-scan, in front of every replay that reads dist / mins.  g < 0: the query is unrestricted.  Every
// stored copy of a label has the label's group, so the copies are all in or all out (twin lemma); a masked byte is
// the empty value in both scans (plain-scan lemma).
//
// The group table in list-position order: 16 int32 per stored chunk, indexed like the allow bitmap (entry 16 c + r =
// the group of row r of global chunk c; -2, which equals no query group, for the rows that pad a list's last chunk
// and for labels outside [0, N)).  64 bytes per stored chunk: 0.4 GB for 100M rows stored once, beside the 4 N bytes
// of the groups by row id.  Made from the device-resident labels by the first call that names a group array, for one
// layout of the lists (lists_gen), as rows.hip's row-position table.
#include "api_internal.h"
#include "chunk_mask.h"

#define TK_NO_GROUP (-2)

// One workgroup per list, threads striding over the list's rows padded to whole chunks: coalesced reads of the
// labels, coalesced writes of the table.
__global__ __launch_bounds__(256) void group_table_kernel(const int64_t *__restrict__ list_chunk_off,
                                                          const int64_t *__restrict__ list_n,
                                                          const int64_t *__restrict__ ids_off,
                                                          const int64_t *__restrict__ ids,
                                                          const int32_t *__restrict__ row_group, int64_t N,
                                                          int32_t *__restrict__ table)
{
    const int64_t l = blockIdx.x;
    const int64_t c0 = list_chunk_off[l];
    const int64_t rows = (list_chunk_off[l + 1] - c0) * 16;     // padded to whole chunks
    const int64_t n = list_n[l];
    const int64_t io = ids_off[l];
    for (int64_t r = threadIdx.x; r < rows; r += blockDim.x) {
        int32_t g = TK_NO_GROUP;
        if (r < n) {
            const int64_t lab = ids[io + r];
            if (lab >= 0 && lab < N) g = row_group[lab];
        }
        table[c0 * 16 + r] = g;
    }
}

// One workgroup per query; threads stride over the query's contiguous chunk range [0, slot_prefix[S]) of dist / mins,
// the slot prefix in LDS: allow_pass_kernel's geometry, the 16-bit keep mask made from the chunk's 16 group ids
// (four 16-byte loads) instead of read from a bitmap.  g_a: the groups of rows [0, n_a) of the batch, g_b: of the
// rows behind them (a pair of calls); NULL, or an entry < 0: the query is unrestricted and its workgroup returns
// before it touches anything.  q0: the batch row the slot arrays start at.  only (or NULL): [count, q_0, q_1, ...] —
// just these queries (rescan_flagged).
template <bool SIGNED>
__global__ __launch_bounds__(256) void group_pass_kernel(uint4 *__restrict__ dist, int64_t cap,
                                                         uint8_t *__restrict__ mins, int64_t cap_min,
                                                         const int *__restrict__ slot_prefix,
                                                         const int64_t *__restrict__ slot_chunk0, int S,
                                                         const int4 *__restrict__ table,
                                                         const int32_t *__restrict__ g_a,
                                                         const int32_t *__restrict__ g_b, int64_t n_a, int64_t q0,
                                                         const int *__restrict__ only)
{
    extern __shared__ int pre[];        // S + 1
    int64_t q = blockIdx.x;
    if (only) {
        if ((int)blockIdx.x >= only[0]) return;
        q = only[1 + blockIdx.x];
    }
    const int64_t row = q0 + q;
    const int32_t *ga = row < n_a ? g_a : g_b;
    if (!ga) return;
    const int32_t g = ga[row < n_a ? row : row - n_a];
    if (g < 0) return;
    for (int s = threadIdx.x; s <= S; s += blockDim.x) pre[s] = slot_prefix[q * (S + 1) + s];
    __syncthreads();
    const int total = pre[S];
    for (int f = threadIdx.x; f < total; f += blockDim.x) {
        int lo = 0, hi = S;     // largest lo with pre[lo] <= f (pre is non-decreasing, pre[0] = 0)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pre[mid] <= f) lo = mid; else hi = mid;
        }
        const int4 *t = table + (slot_chunk0[q * S + lo] + (f - pre[lo])) * 4;
        uint32_t b = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int4 v = t[j];
            b |= (uint32_t)((v.x == g) | ((v.y == g) << 1) | ((v.z == g) << 2) | ((v.w == g) << 3)) << (4 * j);
        }
        tk_mask_chunk<SIGNED>(dist + q * cap + f, mins + q * cap_min + f, b);
    }
}

void tk_launch_group_pass(uint4 *dist, int64_t cap, uint8_t *mins, int64_t cap_min, int64_t nq,
                          const int *slot_prefix, const int64_t *slot_chunk0, int S, const int32_t *table,
                          const int32_t *g_a, TkSecond g_b, int64_t q0, int signd, const int *only, hipStream_t s)
{
    if (nq <= 0 || (!g_a && !g_b.b)) return;
    const int64_t n_a = g_b.n_a > 0 ? g_b.n_a : INT64_MAX;     // (no second call: every row is g_a's)
    const size_t lds = (size_t)(S + 1) * 4;
    if (signd)
        hipLaunchKernelGGL(group_pass_kernel<true>, dim3((unsigned)nq), dim3(256), lds, s, dist, cap, mins, cap_min,
                           slot_prefix, slot_chunk0, S, (const int4 *)table, g_a, (const int32_t *)g_b.b, n_a, q0,
                           only);
    else
        hipLaunchKernelGGL(group_pass_kernel<false>, dim3((unsigned)nq), dim3(256), lds, s, dist, cap, mins, cap_min,
                           slot_prefix, slot_chunk0, S, (const int4 *)table, g_a, (const int32_t *)g_b.b, n_a, q0,
                           only);
}

// What a call that names a group array needs: groups for every row the index has now, and the table for the index's
// current lists — made on the first such call, and again after the lists changed.  Synchronises the device (once per
// layout).
int group_table_ensure(tk_index *ix)
{
    if (ix->groups_n == 0) return fail(TK_ERR_STATE, "a group array was passed but the index has no groups: tk_index_set_groups first");
    if (ix->groups_n != ix->N)
        return fail(TK_ERR_STATE, "the groups cover " + std::to_string(ix->groups_n) + " rows, the index has " +
                                      std::to_string(ix->N) + " now: set them again (tk_index_set_groups)");
    if (ix->group_table_ok && ix->group_table_gen == ix->lists_gen) return TK_OK;
    ARGCHECK(ix->have_lists && ix->have_data, "index has no lists / data yet");
    ARGCHECK(!ix->capturing, "the group table cannot be made inside a stream capture: make one grouped call before "
                             "the capture");
    ix->group_table_ok = false;
    TRY(ix->group_table.ensure((size_t)(ix->total_chunks > 0 ? ix->total_chunks : 1) * 64));
    if (ix->n_lists > 0)
        hipLaunchKernelGGL(group_table_kernel, dim3((unsigned)ix->n_lists), dim3(256), 0, 0,
                           ix->list_chunk_off.as<int64_t>(), ix->list_n.as<int64_t>(), ix->ids_off.as<int64_t>(),
                           ix->ids.as<int64_t>(), ix->row_group.as<int32_t>(), ix->N, ix->group_table.as<int32_t>());
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    ix->group_table_ok = true;
    ix->group_table_gen = ix->lists_gen;
    ix->group_table_builds++;
    return TK_OK;
}

// ---- C ABI ----

extern "C" int tk_index_set_groups(tk_index *ix, const int32_t *groups, int64_t n)
{
    IXLOCK(ix);
    ARGCHECK(ix, "null index");
    ARGCHECK(n >= 0 && (n == 0 || groups), "groups: n ids, or NULL and 0");
    ARGCHECK(!ix->sharded, "list-sharded index: row groups are not supported");
    if (n > 0) {
        ARGCHECK(ix->have_data && n == ix->N, "groups: one id per row of the index (n == N)");
        for (int64_t i = 0; i < n; i++)
            ARGCHECK(groups[i] >= 0 && groups[i] < 0x7fffffff, "groups: ids must lie in [0, 2^31 - 1)");
    }
    TRY(flush_pending(ix));                 // calls still owed that read the old groups are enqueued ...
    HIPCHECK(hipDeviceSynchronize());       // ... and have run
    ix->group_table_ok = false;
    ix->groups_n = 0;
    if (n == 0) {
        ix->row_group.release();
        ix->group_table.release();
        return TK_OK;
    }
    TRY(ix->row_group.ensure((size_t)n * 4));
    HIPCHECK(hipMemcpy(ix->row_group.p, groups, (size_t)n * 4, hipMemcpyHostToDevice));
    ix->groups_n = n;
    return TK_OK;
}

extern "C" int64_t tk_index_groups(tk_index *ix)
{
    IXLOCK(ix);
    if (!ix) return fail(TK_ERR_ARG, "bad argument: null index");
    return ix->groups_n;
}

extern "C" int tk_index_group_table(tk_index *ix, int64_t *info4)
{
    IXLOCK(ix);
    ARGCHECK(ix && info4, "null index / buffer");
    const bool have = ix->group_table_ok && ix->group_table_gen == ix->lists_gen;
    info4[0] = have ? 1 : 0;
    info4[1] = have ? (ix->total_chunks > 0 ? ix->total_chunks : 1) * 64 : 0;
    info4[2] = ix->group_table_builds;
    info4[3] = ix->groups_n * 4;
    return TK_OK;
}
