// rows.hip — stored rows as queries, and one row per query that the query may not return
// (tk_index_query_batch[_dev]_ex2 / tk_index_gather_queries_dev / tk_index_query_rows).
//
// What an excluded row means: a query with excluded row e returns what the reference's IVF.query
// (ivf.py:106-163) returns when `insert` in query_pq runs only for labels != e — the allowed set "all rows but e" of
// §3.8, and so the allow pass's move: every stored copy of e that the query probes gets the heap's empty value in the
// distance bytes, behind the list scans and every re-scan, in front of every replay that reads dist / mins.  It is at
// most one byte per copy and probed slot instead of a bitmap over every probed chunk.
//
// Where a row is stored: the row-position table.  pos_off (N + 2 ints; entry r = first of row r's entries, entry N
// and N + 1 = their total) and pos (T ints): the positions of every stored copy of a row as indices into ix->ids,
// in no particular order.  4 (N + 2) + 4 T bytes: 0.8 GB for 100M rows stored once, 1.2 GB stored twice.  Made from
// the device-resident labels by the first call that names an exclude array, for one layout of the lists (lists_gen).
#include "api_internal.h"
#include "chunk_mask.h"

// cur[1 + r] = first entry of row r on entry (the exclusive scan of the copies per row) and, every copy placed,
// the first entry of row r + 1: the cursor of a row IS the next row's offset, so cur[0 .. N] (cur[0] = 0) ends as the
// table's pos_off.  Labels outside [0, N) are skipped, as the count skipped them.
__global__ __launch_bounds__(256) void row_pos_fill_kernel(const int64_t *__restrict__ ids, int64_t T, int64_t N,
                                                           int *__restrict__ cur, int *__restrict__ pos)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const int64_t id = ids[i];
    if (id < 0 || id >= N) return;
    const int at = atomicAdd(&cur[1 + id], 1);
    if (at >= 0 && at < T) pos[at] = (int)i;
}

// One thread per (query, slot): every copy t of the query's excluded row that lies in the slot's list gets the
// empty value in byte (t - off) % 16 of chunk slot_prefix + (t - off) / 16, and the chunk's byte in mins is taken
// again from the 16 bytes.  Every slot, not the first that holds t: a probe list can name a list twice.  A chunk
// belongs to one slot of one query, so no two threads touch the same one.  ex_a: the excluded rows of rows
// [0, n_a) of the batch, ex_b: of the rows behind them (a pair of calls); NULL or an entry outside [0, N): nothing
// excluded (tk_pass_entry, chunk_mask.h).  only (or NULL): [count, q_0, q_1, ...] — just these queries
// (tk_pass_query).  The probed lists' distance bytes are signed (list_replay_job), so the empty value is 127; there is
// no unsigned form.
__global__ __launch_bounds__(256) void exclude_pass_kernel(uint4 *__restrict__ dist, int64_t cap,
                                                           uint8_t *__restrict__ mins, int64_t cap_min, int64_t nq,
                                                           const int *__restrict__ slot_prefix,
                                                           const int *__restrict__ slot_n,
                                                           const int64_t *__restrict__ slot_label_off, int S,
                                                           const int *__restrict__ pos_off,
                                                           const int *__restrict__ pos, int64_t N, int64_t T,
                                                           const int64_t *__restrict__ ex_a,
                                                           const int64_t *__restrict__ ex_b, int64_t n_a, int64_t q0,
                                                           const int *__restrict__ only)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t qi = i / S;
    const int s = (int)(i - qi * S);
    if (qi >= nq) return;
    int64_t q, e;
    if (!tk_pass_query(qi, only, q) || !tk_pass_entry(ex_a, ex_b, n_a, q0 + q, e) || e < 0 || e >= N) return;
    const int n = slot_n[q * S + s];
    const int64_t off = slot_label_off[q * S + s];
    const int c0 = slot_prefix[q * (S + 1) + s];
    int t0 = pos_off[e], t1 = pos_off[e + 1];
    if (t0 < 0) t0 = 0;
    if (t1 > T) t1 = (int)T;
    const uint32_t fill = 0x7fu;
    for (int t = t0; t < t1; t++) {
        const int64_t r = (int64_t)pos[t] - off;
        if (r < 0 || r >= n) continue;
        const int64_t f = c0 + (r >> 4);
        uint4 *d = dist + q * cap + f;
        const uint4 v = *d;
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const int b = (int)(r & 15);
        int mn = 127;
#pragma unroll
        for (int j = 0; j < 4; j++) {       // (the word is picked by comparison: no indexed register array)
            if (j == (b >> 2)) w[j] = (w[j] & ~(0xffu << (8 * (b & 3)))) | (fill << (8 * (b & 3)));
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t y = (w[j] >> (8 * u)) & 0xffu;
                const int x = (int)(int8_t)y;
                mn = x < mn ? x : mn;
            }
        }
        *d = make_uint4(w[0], w[1], w[2], w[3]);
        mins[q * cap_min + f] = (uint8_t)mn;
    }
}

void tk_launch_exclude_pass(uint4 *dist, int64_t cap, uint8_t *mins, int64_t cap_min, int64_t nq,
                            const int *slot_prefix, const int *slot_n, const int64_t *slot_label_off, int S,
                            const TkRowPos &tab, const int64_t *ex_a, TkSecond ex_b, int64_t q0, const int *only,
                            hipStream_t s)
{
    if (nq <= 0 || S <= 0 || (!ex_a && !ex_b.b)) return;
    const int64_t n_a = ex_b.n_a > 0 ? ex_b.n_a : INT64_MAX;     // (no second call: every row is ex_a's)
    const dim3 grid((unsigned)((nq * S + 255) / 256)), block(256);
    hipLaunchKernelGGL(exclude_pass_kernel, grid, block, 0, s, dist, cap, mins, cap_min, nq, slot_prefix, slot_n,
                       slot_label_off, S, tab.pos_off, tab.pos, tab.N, tab.T, ex_a, (const int64_t *)ex_b.b, n_a, q0,
                       only);
}

// The table for the index's current lists: made on the first call, and again after the lists changed.  Count per row
// (row_copies_kernel), exclusive scan, fill.  Synchronises the device (once per layout).
int row_pos_ensure(tk_index *ix)
{
    if (ix->row_pos_state.current(ix->lists_gen)) return TK_OK;
    TRY(table_may_build(ix, "row-position", "excluding"));
    ARGCHECK(ix->total_ids < 0x7fffffffll && ix->N < 0x7ffffff0ll, "row-position table: more than 2^31 stored rows");
    const int64_t N = ix->N, T = ix->total_ids;
    ix->row_pos_state.ok = false;
    DevBuf summary, tmp;
    auto run = [&]() -> int {
        const int init[4] = {-1, 0, 0x7fffffff, 0};
        TRY(ix->row_pos_off.ensure((size_t)(N + 2) * 4));
        TRY(ix->row_pos.ensure((size_t)(T > 0 ? T : 1) * 4));
        TRY(summary.ensure(sizeof init));
        size_t tmp_bytes = 0;
        if (tk_scan_exclusive(nullptr, &tmp_bytes, nullptr, nullptr, N + 1, 0)) return fail(TK_ERR_HIP, "scan size query");
        TRY(tmp.ensure(tmp_bytes));
        int *off = ix->row_pos_off.as<int>();
        HIPCHECK(hipMemset(off, 0, (size_t)(N + 2) * 4));
        HIPCHECK(hipMemcpy(summary.p, init, sizeof init, hipMemcpyHostToDevice));
        // (the launcher also sums the counts up for its other callers; that summary is not read here)
        tk_launch_row_copies(ix->ids.as<int64_t>(), T, off + 1, N, summary.as<int>(), 0);
        if (tk_scan_exclusive(tmp.p, &tmp_bytes, off + 1, off + 1, N + 1, 0)) return fail(TK_ERR_HIP, "scan");
        if (T > 0)
            hipLaunchKernelGGL(row_pos_fill_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, 0,
                               ix->ids.as<int64_t>(), T, N, off, ix->row_pos.as<int>());
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        return TK_OK;
    };
    const int r = run();
    summary.release();
    tmp.release();
    if (r != TK_OK) return r;
    ix->row_pos_state.made(ix->lists_gen);
    return TK_OK;
}

// ---- C ABI ----

extern "C" int tk_index_row_table(tk_index *ix, int64_t *info4)
{
    IXLOCK(ix);
    ARGCHECK(ix && info4, "null index / buffer");
    const bool have = ix->row_pos_state.current(ix->lists_gen);
    info4[0] = have ? 1 : 0;
    info4[1] = have ? (ix->N + 2) * 4 + (ix->total_ids > 0 ? ix->total_ids : 1) * 4 : 0;
    info4[2] = ix->row_pos_state.builds;
    info4[3] = have ? ix->total_ids : 0;
    return TK_OK;
}

extern "C" int tk_index_coalesce(tk_index *ix)
{
    IXLOCK(ix);
    ARGCHECK(ix, "null index");
    return ix->coalesce;
}

extern "C" int tk_index_gather_queries_dev(tk_index *ix, const int64_t *rows_dev, int64_t nq, float *qn_dev,
                                           void *q_pq_dev, void *stream)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_pq && ix->have_centers && ix->have_data, "set_pq, set_centers and set_data first");
    ARGCHECK(nq >= 0 && (nq == 0 || (rows_dev && qn_dev && q_pq_dev)), "buffers");
    ARGCHECK(ix->rot_d_pad > 0 || ix->dq >= ix->d, "unrotated PQ: dq >= d");
    if (nq == 0) return TK_OK;
    hipStream_t st = (hipStream_t)stream;
    tk_launch_gather_rows(ix->data.p, ix->data_dtype, ix->d, rows_dev, nq, qn_dev, st);
    tk_launch_prepare_queries(qn_dev, nq, ix->d, ix->rot_d_pad ? ix->rot_t.as<double>() : nullptr, ix->dq,
                              ix->rot_d_pad ? ix->rot_d_pad : ix->dq, q_pq_dev, st);
    HIPCHECK(hipGetLastError());
    return TK_OK;
}

// the same with host buffers: what the device made of the rows, for inspection and tests
extern "C" int tk_index_gather_queries(tk_index *ix, const int64_t *rows, int64_t nq, float *qn, void *q_pq)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_pq && ix->have_centers && ix->have_data, "set_pq, set_centers and set_data first");
    ARGCHECK(nq >= 0 && (nq == 0 || (rows && qn && q_pq)), "buffers");
    for (int64_t i = 0; i < nq; i++) ARGCHECK(rows[i] >= 0 && rows[i] < ix->N, "row id out of range");
    if (nq == 0) return TK_OK;
    const size_t esz = ix->rot_d_pad > 0 ? 8 : 4;
    DevBuf r, a, b;
    auto run = [&]() -> int {
        TRY(r.ensure((size_t)nq * 8));
        TRY(a.ensure((size_t)nq * ix->d * 4));
        TRY(b.ensure((size_t)nq * ix->dq * esz));
        HIPCHECK(hipMemcpy(r.p, rows, (size_t)nq * 8, hipMemcpyHostToDevice));
        TRY(tk_index_gather_queries_dev(ix, r.as<int64_t>(), nq, a.as<float>(), b.p, nullptr));
        HIPCHECK(hipMemcpy(qn, a.p, (size_t)nq * ix->d * 4, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(q_pq, b.p, (size_t)nq * ix->dq * esz, hipMemcpyDeviceToHost));
        return TK_OK;
    };
    const int rc = run();
    r.release();
    a.release();
    b.release();
    return rc;
}
