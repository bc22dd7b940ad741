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

// One workgroup per list (tk_row_table, chunk_mask.h).
__global__ __launch_bounds__(256) void group_table_kernel(const int64_t *__restrict__ list_chunk_off,
                                                          const int64_t *__restrict__ list_n,
                                                          const int64_t *__restrict__ ids_off,
                                                          const int64_t *__restrict__ ids,
                                                          const int32_t *__restrict__ row_group, int64_t N,
                                                          int32_t *__restrict__ table)
{
    tk_row_table<int32_t>(list_chunk_off, list_n, ids_off, ids, row_group, N, TK_NO_GROUP, table);
}

// One workgroup per query over the query's probed chunks (tk_mask_probed, chunk_mask.h), a chunk's keep mask made from
// its 16 group ids (four 16-byte loads).  g_a: the groups of rows [0, n_a) of the batch, g_b: of the rows behind them
// (a pair of calls); NULL, or an entry < 0: the query is unrestricted and its workgroup returns before it touches
// anything.  q0: the batch row the slot arrays start at.  only (or NULL): [count, q_0, q_1, ...] — just these queries
// (tk_pass_query).
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
    int64_t q;
    int32_t g;
    if (!tk_pass_query(blockIdx.x, only, q) || !tk_pass_entry(g_a, g_b, n_a, q0 + q, g) || g < 0) return;
    tk_mask_probed<SIGNED>(dist, cap, mins, cap_min, slot_prefix, slot_chunk0, S, q, [=](int64_t c) -> uint32_t {
        const int4 *t = table + c * 4;
        uint32_t b = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int4 v = t[j];
            b |= (uint32_t)((v.x == g) | ((v.y == g) << 1) | ((v.z == g) << 2) | ((v.w == g) << 3)) << (4 * j);
        }
        return b;
    });
}

void tk_launch_group_pass(uint4 *dist, int64_t cap, uint8_t *mins, int64_t cap_min, int64_t nq,
                          const int *slot_prefix, const int64_t *slot_chunk0, int S, const int32_t *table,
                          const int32_t *g_a, TkSecond g_b, int64_t q0, int signd, const int *only, hipStream_t s)
{
    if (nq <= 0 || (!g_a && !g_b.b)) return;
    const int64_t n_a = g_b.n_a > 0 ? g_b.n_a : INT64_MAX;     // (no second call: every row is g_a's)
    const size_t lds = (size_t)(S + 1) * 4;
    const auto kernel = signd ? group_pass_kernel<true> : group_pass_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nq), dim3(256), lds, s, dist, cap, mins, cap_min, slot_prefix, slot_chunk0,
                       S, (const int4 *)table, g_a, (const int32_t *)g_b.b, n_a, q0, only);
}

// What a call that names a group array needs (row_table_ensure): groups for every row, the table of the current lists
int group_table_ensure(tk_index *ix)
{
    return row_table_ensure(ix, ix->groups, [](const tk_index *ix) {
        hipLaunchKernelGGL(group_table_kernel, dim3((unsigned)ix->n_lists), dim3(256), 0, 0,
                           ix->list_chunk_off.as<int64_t>(), ix->list_n.as<int64_t>(), ix->ids_off.as<int64_t>(),
                           ix->ids.as<int64_t>(), ix->groups.by_row.as<int32_t>(), ix->N,
                           ix->groups.table.as<int32_t>());
    });
}

// ---- C ABI ----

extern "C" int tk_index_set_groups(tk_index *ix, const int32_t *groups, int64_t n)
{
    IXLOCK(ix);
    ARGCHECK(ix, "null index");
    return row_table_set(ix, ix->groups, groups, n, [](const void *vals, int64_t n) -> int {
        const int32_t *g = (const int32_t *)vals;
        for (int64_t i = 0; i < n; i++)
            ARGCHECK(g[i] >= 0 && g[i] < 0x7fffffff, "groups: ids must lie in [0, 2^31 - 1)");
        return TK_OK;
    });
}

extern "C" int64_t tk_index_groups(tk_index *ix)
{
    IXLOCK(ix);
    if (!ix) return fail(TK_ERR_ARG, "bad argument: null index");
    return ix->groups.n;
}

extern "C" int tk_index_group_table(tk_index *ix, int64_t *info4)
{
    IXLOCK(ix);
    ARGCHECK(ix && info4, "null index / buffer");
    return row_table_info(ix, ix->groups, info4);
}
