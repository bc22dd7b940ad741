// tags.hip — every query of a batch restricted to the rows that carry its tags
// (tk_index_set_tags / tk_index_query_batch[_dev]_ex4).
//
// What tags mean: rows carry a 64-bit mask, tags[r], bit t set = row r carries tag t; a mask of 0 is a
// row without tags.  A query carries a mask m, the call one mode: "any" — a row passes iff (tags[r] & m) != 0; "all" —
// iff (tags[r] & m) == m.  A query with m != 0 returns what the reference's IVF.query (ivf.py:106-163) returns when
// `insert` in query_pq runs only for labels that pass — the allowed set of §3.8, for that query alone, and so the
// allow pass's move: every probed row that does not pass gets the heap's empty value in the distance bytes, behind the
// list scans and every re-scan, in front of every replay that reads dist / mins.  m == 0: the query is unrestricted
// in both modes (the truth of the formula in "all", the convention "no filter was given" in "any").  Every stored copy
// of a label has the label's tags, so the copies are all in or all out (twin lemma); a masked byte is the empty value
// in both scans (plain-scan lemma).
//
// The tag table in list-position order: 16 uint64 per stored chunk, indexed like the group table (entry 16 c + r = the
// tags of row r of global chunk c; 0, which passes no restricted query in either mode since m != 0 there, for the rows
// that pad a list's last chunk and for labels outside [0, N)).  128 bytes per stored chunk: 0.8 GB for 100M rows
// stored once, beside the 8 N bytes of the tags by row id.  Made from the device-resident labels by the first call
// that names a tag array, for one layout of the lists (lists_gen), as the group table.
#include "api_internal.h"
#include "chunk_mask.h"

// One workgroup per list (tk_row_table, chunk_mask.h).
__global__ __launch_bounds__(256) void tag_table_kernel(const int64_t *__restrict__ list_chunk_off,
                                                        const int64_t *__restrict__ list_n,
                                                        const int64_t *__restrict__ ids_off,
                                                        const int64_t *__restrict__ ids,
                                                        const uint64_t *__restrict__ row_tags, int64_t N,
                                                        uint64_t *__restrict__ table)
{
    tk_row_table<uint64_t>(list_chunk_off, list_n, ids_off, ids, row_tags, N, 0, table);
}

// One workgroup per query over the query's probed chunks (tk_mask_probed, chunk_mask.h), a chunk's keep mask made from
// its 16 tag masks (eight 16-byte loads) with 64-bit compares, ALL: (t & m) == m, else (t & m) != 0.  m_a: the masks of
// rows [0, n_a) of the batch, m_b: of the rows behind them (a pair of calls, both of one mode); NULL, or an entry of 0:
// the query is unrestricted and its workgroup returns before it touches anything.  q0, only: as group_pass_kernel.
template <bool SIGNED, bool ALL>
__global__ __launch_bounds__(256) void tag_pass_kernel(uint4 *__restrict__ dist, int64_t cap,
                                                       uint8_t *__restrict__ mins, int64_t cap_min,
                                                       const int *__restrict__ slot_prefix,
                                                       const int64_t *__restrict__ slot_chunk0, int S,
                                                       const ulonglong2 *__restrict__ table,
                                                       const uint64_t *__restrict__ m_a,
                                                       const uint64_t *__restrict__ m_b, int64_t n_a, int64_t q0,
                                                       const int *__restrict__ only)
{
    int64_t q;
    uint64_t m;
    if (!tk_pass_query(blockIdx.x, only, q) || !tk_pass_entry(m_a, m_b, n_a, q0 + q, m) || m == 0) return;
    tk_mask_probed<SIGNED>(dist, cap, mins, cap_min, slot_prefix, slot_chunk0, S, q, [=](int64_t c) -> uint32_t {
        const ulonglong2 *t = table + c * 8;
        uint32_t b = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const ulonglong2 v = t[j];
            const uint64_t x = (uint64_t)v.x & m, y = (uint64_t)v.y & m;
            const uint32_t px = ALL ? x == m : x != 0, py = ALL ? y == m : y != 0;
            b |= (px | (py << 1)) << (2 * j);
        }
        return b;
    });
}

void tk_launch_tag_pass(uint4 *dist, int64_t cap, uint8_t *mins, int64_t cap_min, int64_t nq,
                        const int *slot_prefix, const int64_t *slot_chunk0, int S, const uint64_t *table,
                        const uint64_t *m_a, TkSecond m_b, int all, int64_t q0, int signd, const int *only,
                        hipStream_t s)
{
    if (nq <= 0 || (!m_a && !m_b.b)) return;
    const int64_t n_a = m_b.n_a > 0 ? m_b.n_a : INT64_MAX;     // (no second call: every row is m_a's)
    const size_t lds = (size_t)(S + 1) * 4;
    const auto kernel = signd ? (all ? tag_pass_kernel<true, true> : tag_pass_kernel<true, false>)
                              : (all ? tag_pass_kernel<false, true> : tag_pass_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nq), dim3(256), lds, s, dist, cap, mins, cap_min, slot_prefix, slot_chunk0,
                       S, (const ulonglong2 *)table, m_a, (const uint64_t *)m_b.b, n_a, q0, only);
}

// What a call that names a tag array needs (row_table_ensure): tags for every row, the table of the current lists
int tag_table_ensure(tk_index *ix)
{
    return row_table_ensure(ix, ix->tags, [](const tk_index *ix) {
        hipLaunchKernelGGL(tag_table_kernel, dim3((unsigned)ix->n_lists), dim3(256), 0, 0,
                           ix->list_chunk_off.as<int64_t>(), ix->list_n.as<int64_t>(), ix->ids_off.as<int64_t>(),
                           ix->ids.as<int64_t>(), ix->tags.by_row.as<uint64_t>(), ix->N,
                           ix->tags.table.as<uint64_t>());
    });
}

// ---- C ABI ----

extern "C" int tk_index_set_tags(tk_index *ix, const uint64_t *tags, int64_t n)
{
    IXLOCK(ix);
    ARGCHECK(ix, "null index");
    return row_table_set(ix, ix->tags, tags, n);
}

extern "C" int64_t tk_index_tags(tk_index *ix)
{
    IXLOCK(ix);
    if (!ix) return fail(TK_ERR_ARG, "bad argument: null index");
    return ix->tags.n;
}

extern "C" int tk_index_tag_table(tk_index *ix, int64_t *info4)
{
    IXLOCK(ix);
    ARGCHECK(ix && info4, "null index / buffer");
    return row_table_info(ix, ix->tags, info4);
}
