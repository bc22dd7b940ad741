// between.hip — every query of a batch restricted to the rows whose values lie in its ranges
// (tk_index_set_values / tk_index_query_batch[_dev]_ex5).
//
// What ranges mean: rows carry C numeric columns, 1 <= C <= 4, as int64 KEYS (the host maps integers and
// floats to keys with one strictly monotone function, ivf.py: value_keys; the device compares int64 only).  A query
// carries one inclusive interval [lo_c, hi_c] per column; a row passes iff lo_c <= key[row, c] <= hi_c for every c.  An
// unbounded end is INT64_MIN / INT64_MAX: the comparison is simply true.  A query with a bounded column returns what the
// reference's IVF.query (ivf.py:106-163) returns when `insert` in query_pq runs only for labels that pass — the allowed
// set of §3.8, for that query alone, and so the allow pass's move: every probed row that does not pass gets the heap's
// empty value in the distance bytes, behind the list scans and every re-scan, in front of every replay that reads
// dist / mins.  Every bound unbounded: the query is unrestricted.  lo > hi: no row passes.  Every stored copy of a label
// has the label's values (twin lemma); a masked byte is the empty value in both scans (plain-scan lemma).
//
// The value table, column-major: by row id (C, N) int64, and in list-position order C planes of 16 x total_chunks
// int64, plane c indexed like the tag table (entry 16 ch + r = column c of row r of global chunk ch).  The rows that
// pad a list's last chunk and labels outside [0, N) get INT64_MIN; any value would do, their distance bytes are the
// empty value already (pad_fix_kernel).  128 bytes per stored chunk and column beside the 8 C N bytes by row id:
// 0.8 GB + 0.8 GB per column for 100M rows stored once, 1.6 GB + 0.8 GB per column stored twice (build(n_probes=2)).
// Made from the device-resident labels by the first call that names a range array, for one layout of the lists
// (lists_gen), as the tag table.
#include "api_internal.h"
#include "chunk_mask.h"

// One workgroup per list (tk_row_table, chunk_mask.h), one launch per column: a column's keys by row id -> its plane.
__global__ __launch_bounds__(256) void value_table_kernel(const int64_t *__restrict__ list_chunk_off,
                                                          const int64_t *__restrict__ list_n,
                                                          const int64_t *__restrict__ ids_off,
                                                          const int64_t *__restrict__ ids,
                                                          const int64_t *__restrict__ row_keys, int64_t N,
                                                          int64_t *__restrict__ plane)
{
    tk_row_table<int64_t>(list_chunk_off, list_n, ids_off, ids, row_keys, N, INT64_MIN, plane);
}

// bit r = lo <= key r of the chunk at t <= hi: the chunk's 16 keys as eight 16-byte loads, all issued before the first
// compare (one round trip to memory a chunk, as the tag pass: left to itself the compiler issued them in groups of 1, 4
// and 3 with a wait behind each), two 64-bit compares each.  A wave's compare result is an SGPR pair, so the compares
// go four at a time behind a scheduling barrier: 77 SGPRs, where all 32 results at once took 105 and a wave of occupancy.
__device__ __forceinline__ uint32_t range_mask16(const longlong2 *__restrict__ t, int64_t lo, int64_t hi)
{
    longlong2 v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = t[j];
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j % 2 == 0) __builtin_amdgcn_sched_barrier(0);
        const uint32_t px = (uint32_t)((int64_t)v[j].x >= lo) & (uint32_t)((int64_t)v[j].x <= hi);
        const uint32_t py = (uint32_t)((int64_t)v[j].y >= lo) & (uint32_t)((int64_t)v[j].y <= hi);
        m |= (px | (py << 1)) << (2 * j);
    }
    return m;
}

// One workgroup per query over the query's probed chunks (tk_mask_probed, chunk_mask.h).  The query's 2 C bounds
// (lo_0, hi_0, lo_1, ...) are entries [2 C row, 2 C row + 2 C) of b_a for the rows [0, n_a) of the batch, of b_b for
// the rows behind them (a pair of calls; n_a2 = 2 C n_a, the boundary in keys); NULL, or every bound the unbounded
// extreme: the query is unrestricted and its workgroup returns before it touches anything.  A chunk's keep mask: for
// every BOUNDED column (uniform over the workgroup) the 16 bits of range_mask16, anded.  The column loop is a runtime
// loop with one body; a column's two bounds are read again per chunk (scalar loads, uniform) and never held across
// columns.  plane: a column's plane in 16-byte units (8 per chunk).  q0, only: as tag_pass_kernel.
template <bool SIGNED>
__global__ __launch_bounds__(256) void between_pass_kernel(uint4 *__restrict__ dist, int64_t cap,
                                                           uint8_t *__restrict__ mins, int64_t cap_min,
                                                           const int *__restrict__ slot_prefix,
                                                           const int64_t *__restrict__ slot_chunk0, int S,
                                                           const longlong2 *__restrict__ table, int64_t plane, int C,
                                                           const int64_t *__restrict__ b_a,
                                                           const int64_t *__restrict__ b_b, int64_t n_a2, int64_t q0,
                                                           const int *__restrict__ only)
{
    int64_t q;
    if (!tk_pass_query(blockIdx.x, only, q)) return;
    const int64_t e0 = (q0 + q) * 2 * C;        // the query's first bound
    uint32_t bounded = 0;                       // bit c: column c has a bounded end
    for (int c = 0; c < C; c++) {
        int64_t l, h;
        if (!tk_pass_entry(b_a, b_b, n_a2, e0 + 2 * c, l) || !tk_pass_entry(b_a, b_b, n_a2, e0 + 2 * c + 1, h)) return;
        if (l != INT64_MIN || h != INT64_MAX) bounded |= 1u << c;
    }
    if (bounded == 0) return;
    tk_mask_probed<SIGNED>(dist, cap, mins, cap_min, slot_prefix, slot_chunk0, S, q, [=](int64_t ch) -> uint32_t {
        const longlong2 *t = table + ch * 8;
        uint32_t b = 0xffffu;
        for (int c = 0; c < C; c++) {
            if (!(bounded >> c & 1u)) continue;
            int64_t l = 0, h = 0;
            (void)tk_pass_entry(b_a, b_b, n_a2, e0 + 2 * c, l);
            (void)tk_pass_entry(b_a, b_b, n_a2, e0 + 2 * c + 1, h);
            b &= range_mask16(t + c * plane, l, h);
        }
        return b;
    });
}

void tk_launch_between_pass(uint4 *dist, int64_t cap, uint8_t *mins, int64_t cap_min, int64_t nq,
                            const int *slot_prefix, const int64_t *slot_chunk0, int S, const int64_t *table,
                            int64_t plane_keys, int cols, const int64_t *b_a, TkSecond b_b, int64_t q0, int signd,
                            const int *only, hipStream_t s)
{
    if (nq <= 0 || (!b_a && !b_b.b)) return;
    const int64_t n_a2 = b_b.n_a > 0 ? b_b.n_a * 2 * cols : INT64_MAX;     // (no second call: every row is b_a's)
    const size_t lds = (size_t)(S + 1) * 4;
    const auto kernel = signd ? between_pass_kernel<true> : between_pass_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nq), dim3(256), lds, s, dist, cap, mins, cap_min, slot_prefix, slot_chunk0,
                       S, (const longlong2 *)table, plane_keys / 2, cols, b_a, (const int64_t *)b_b.b, n_a2, q0, only);
}

// What a call that names a range array needs (row_table_ensure): values for every row, the table of the current lists
int value_table_ensure(tk_index *ix)
{
    return row_table_ensure(ix, ix->values, [](const tk_index *ix) {
        for (int c = 0; c < value_columns(ix); c++)
            hipLaunchKernelGGL(value_table_kernel, dim3((unsigned)ix->n_lists), dim3(256), 0, 0,
                               ix->list_chunk_off.as<int64_t>(), ix->list_n.as<int64_t>(), ix->ids_off.as<int64_t>(),
                               ix->ids.as<int64_t>(), ix->values.by_row.as<int64_t>() + c * ix->N, ix->N,
                               ix->values.table.as<int64_t>() + c * value_plane(ix));
    });
}

// ---- C ABI ----

extern "C" int tk_index_set_values(tk_index *ix, const int64_t *keys, int64_t n, int cols)
{
    IXLOCK(ix);
    ARGCHECK(ix, "null index");
    ARGCHECK(n == 0 ? cols == 0 || (cols >= 1 && cols <= 4) : cols >= 1 && cols <= 4, "values: 1 to 4 columns");
    return row_table_set(ix, ix->values, keys, n, nullptr, n > 0 ? (size_t)cols * 8 : 0);
}

extern "C" int64_t tk_index_values(tk_index *ix)
{
    IXLOCK(ix);
    if (!ix) return fail(TK_ERR_ARG, "bad argument: null index");
    return ix->values.n;
}

extern "C" int tk_index_value_columns(tk_index *ix)
{
    IXLOCK(ix);
    if (!ix) return fail(TK_ERR_ARG, "bad argument: null index");
    return value_columns(ix);
}

extern "C" int tk_index_value_table(tk_index *ix, int64_t *info4)
{
    IXLOCK(ix);
    ARGCHECK(ix && info4, "null index / buffer");
    return row_table_info(ix, ix->values, info4);
}
