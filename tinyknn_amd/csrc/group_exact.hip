// group_exact.hip — the exact k nearest rows inside a query's own group of rows (tk_index_knn_group).
//
// knn_brute(group=) multiplies every query with all N rows and keeps the products of one group; here a query reads the
// rows of its group and nothing else, so the cost follows the size of the group.  Three things make that possible:
//   rows by group   every row id gathered by group id (TkRowTable::span_*): span_rows[N] int32, the rows of one group
//                   one contiguous span in ascending order; span_gid[G] the sorted distinct group ids, span_off[G + 1]
//                   where the spans begin.  Group ids are sparse in [0, 2^31 - 1), so this is a sort by key — rocPRIM's
//                   radix sort over (group, row) pairs, 31 key bits, stable — then a run-length encoding of the sorted
//                   keys and tk_scan_exclusive over the run lengths (group_rows.hip: the library's kernels stay out
//                   of this file).  Made by the first call that needs it and again after tk_index_set_groups; it
//                   follows the groups, not the lists.
//   stored rows     tk_index_remove_rows leaves the vectors of removed rows in HBM; a row is stored when some list
//                   holds its id.  An N-bit map (bit r: label r occurs), made from the labels by one kernel per layout
//                   of the lists (lists_gen): N / 8 bytes, 32 times smaller than the row-position table of rows.hip,
//                   and one L2-resident word per row where that table costs two loads.
//   the kernel      (the walk itself is span_exact.h's, shared with value_exact.hip; group_exact_kernel hands it the
//                   group's span.)  One workgroup per query.  The span is walked in tiles of GX_TILE rows, a lane a row: rows that are
//                   not stored or fail a restriction (allowed bit, exclude, tags any / all, ranges — by row id, the
//                   formulas of brute.hip's restricted form; the query's own attributes sit in scalar registers) are
//                   dropped, the others get sqdist_row<T, TY> (sqdist_row.h: the rescoring's distance, numpy's einsum
//                   order bit for bit) and, where that is not above the query's bound, a slot in a candidate buffer in
//                   LDS: GX_CAP entries of (distance key, row id).  In front of a tile that could overflow the buffer
//                   it is cut back: sorted by (distance, row id) — a bitonic sort over the entries it holds — cut to its
//                   k best, the bound tightened to the k-th distance.  "Could": the count the decision uses is an upper
//                   bound kept in a register (entries after the last cut + GX_TILE per tile since), so the tile loop has
//                   no barrier and the waves of a workgroup stream through their rows independently.  The last cut is
//                   the result: ascending by (distance, row id), -1 / +inf behind fewer than k survivors.
// A group of any size is answered, the whole index in one group included, but one workgroup reads all of it: for large
// groups knn_brute(group=) on the matrix cores is the call (IVF.query_batch(exact_below=) routes by size).  Queries of
// one group share row reads only through L2.
#include "api_internal.h"
#include "sqdist_row.h"
#include "span_exact.h"

// (stated here as span_exact.h states them: the walk, GxKey and gx_lds_bytes live there, shared with value_exact.hip)
#define GX_TILE 256       // rows of the span per pass of the workgroup: a lane a row
#define GX_CAP 2048       // entries of the candidate buffer; k + GX_TILE <= GX_CAP for every k <= 1024

// r: the restriction's device arrays (TkBruteRestrict; its group fields are not read: the span IS the group).
// begin / len: the query's span of span_rows (len 0: an id no row carries).  stored: the N-bit map.
template <typename T, typename TY>
__global__ __launch_bounds__(GX_THREADS) void group_exact_kernel(const float *__restrict__ q, int d,
                                                                 const TY *__restrict__ rows,
                                                                 const int32_t *__restrict__ span_rows,
                                                                 const int32_t *__restrict__ begin,
                                                                 const int32_t *__restrict__ len,
                                                                 const uint32_t *__restrict__ stored,
                                                                 const TkBruteRestrict r, int k,
                                                                 int64_t *__restrict__ out, T *__restrict__ out_d)
{
    const int64_t qi = blockIdx.x;
    span_exact_body<T, TY, false>(q, d, rows, span_rows + begin[qi], len[qi], stored, r, k, out, out_d);
}

// group ids -> their spans: the lower bound of g among the sorted distinct ids; (0, 0) for an id no row carries
__global__ __launch_bounds__(256) void group_span_kernel(const int32_t *__restrict__ gid,
                                                         const int32_t *__restrict__ off, int64_t G,
                                                         const int32_t *__restrict__ group, int64_t n,
                                                         int32_t *__restrict__ begin, int32_t *__restrict__ len)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t g = group[i];
    int64_t lo = 0, hi = G;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (gid[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    const bool have = lo < G && gid[lo] == g;
    begin[i] = have ? off[lo] : 0;
    len[i] = have ? off[lo + 1] - off[lo] : 0;
}

// bit r of `bits` = some list holds label r (labels outside [0, N) are skipped, as rows.hip skips them)
__global__ __launch_bounds__(256) void stored_bits_kernel(const int64_t *__restrict__ ids, int64_t T, int64_t N,
                                                          uint32_t *__restrict__ bits)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const int64_t id = ids[i];
    if (id < 0 || id >= N) return;
    atomicOr(&bits[id >> 5], 1u << (id & 31));
}

// The stored-row map of the index's current lists: made on the first call, and again after the lists changed.
// call: the entry point that asks (tk_index_knn_group, tk_index_knn_between), named where the map cannot be made.
int stored_bits_ensure(tk_index *ix, const char *call)
{
    if (ix->stored_state.current(ix->lists_gen)) return TK_OK;
    TRY(table_may_build(ix, "stored-row", call));
    ix->stored_state.ok = false;
    const size_t bytes = (size_t)((ix->N + 31) / 32) * 4;
    TRY(ix->stored_bits.ensure(bytes));
    HIPCHECK(hipMemset(ix->stored_bits.p, 0, bytes));
    if (ix->total_ids > 0)
        hipLaunchKernelGGL(stored_bits_kernel, dim3((unsigned)((ix->total_ids + 255) / 256)), dim3(256), 0, 0,
                           ix->ids.as<int64_t>(), ix->total_ids, ix->N, ix->stored_bits.as<uint32_t>());
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    ix->stored_state.made(ix->lists_gen);
    return TK_OK;
}

// the spans of n group ids (device) -> begin / len (device, the index's gx_ buffers)
static int group_spans(tk_index *ix, const int32_t *group_dev, int64_t n)
{
    TRY(ix->gx_begin.ensure((size_t)n * 4));
    TRY(ix->gx_len.ensure((size_t)n * 4));
    hipLaunchKernelGGL(group_span_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0,
                       ix->groups.span_gid.as<int32_t>(), ix->groups.span_off.as<int32_t>(), ix->groups.span_groups,
                       group_dev, n, ix->gx_begin.as<int32_t>(), ix->gx_len.as<int32_t>());
    return TK_OK;
}

template <typename T, typename TY>
static void launch_group_exact(const tk_index *ix, const float *q, int64_t nq, int k, const TkBruteRestrict &r,
                               int64_t *out, void *out_d)
{
    const size_t lds = gx_lds_bytes(ix->d, sizeof(typename GxKey<T>::type), sizeof(T));
    hipLaunchKernelGGL((group_exact_kernel<T, TY>), dim3((unsigned)nq), dim3(GX_THREADS), lds, 0, q, ix->d,
                       ix->data.as<TY>(), ix->groups.span_rows.as<int32_t>(), ix->gx_begin.as<int32_t>(),
                       ix->gx_len.as<int32_t>(), ix->stored_bits.as<uint32_t>(), r, k, out, (T *)out_d);
}

// A host array of the call in its workspace buffer (NULL stays NULL)
template <typename T>
static int gx_upload(DevBuf &b, const T *host, size_t n, const T *&dev)
{
    dev = nullptr;
    if (!host) return TK_OK;
    TRY(b.ensure((n > 0 ? n : 1) * sizeof(T)));
    HIPCHECK(hipMemcpy(b.p, host, n * sizeof(T), hipMemcpyHostToDevice));
    dev = b.as<T>();
    return TK_OK;
}

// ---- C ABI ----

extern "C" int tk_index_knn_group(tk_index *ix, const float *q, int64_t nq, int k, const int32_t *group,
                                  const uint8_t *allowed_mask, const int64_t *exclude, const uint64_t *tags,
                                  int tag_mode, const int64_t *between, int64_t *out_ids, void *out_dist)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: knn_group is not supported");
    ARGCHECK(nq >= 0 && (nq == 0 || (q && out_ids)), "buffers");
    ARGCHECK(nq == 0 || group, "group: one group id per query is required");
    ARGCHECK(k >= 1 && k <= 1024 && k <= ix->N, "1 <= k <= min(1024, N)");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    ARGCHECK(ix->d <= 4096, "d <= 4096");
    ARGCHECK(tag_mode == 0 || tag_mode == 1, "tag_mode: 0 (any) or 1 (all)");
    for (int64_t i = 0; i < nq; i++) ARGCHECK(group[i] >= 0, "group: every entry must be a group id >= 0");
    TRY(row_table_covers(ix, ix->groups));
    if (tags) TRY(row_table_covers(ix, ix->tags));
    if (between) TRY(row_table_covers(ix, ix->values));
    if (exclude)
        for (int64_t i = 0; i < nq; i++) ARGCHECK(exclude[i] >= -1 && exclude[i] < ix->N, "exclude: entries in [-1, N)");
    if (nq == 0) return TK_OK;
    TRY(flush_pending(ix));
    TRY(group_rows_ensure(ix));
    TRY(stored_bits_ensure(ix, "tk_index_knn_group"));
    TkBruteRestrict r{};
    r.n_rows = ix->N;
    r.tag_mode = tag_mode;
    if (allowed_mask) {
        std::vector<uint32_t> bits((size_t)(ix->N + 31) / 32, 0u);
        for (int64_t j = 0; j < ix->N; j++) bits[(size_t)(j >> 5)] |= (uint32_t)(allowed_mask[j] != 0) << (j & 31);
        TRY(gx_upload(ix->br_mask, bits.data(), bits.size(), r.allowed));
    }
    const int32_t *group_dev = nullptr;
    TRY(gx_upload(ix->br_group, group, (size_t)nq, group_dev));
    TRY(gx_upload(ix->br_exclude, exclude, (size_t)nq, r.exclude));
    TRY(gx_upload(ix->br_tags, tags, (size_t)nq, r.tags));
    if (tags) r.row_tags = ix->tags.by_row.as<uint64_t>();
    if (between) {
        r.cols = value_columns(ix);
        r.row_keys = ix->values.by_row.as<int64_t>();
        TRY(gx_upload(ix->br_ranges, between, (size_t)nq * 2 * r.cols, r.ranges));
    }
    const size_t dsz = ix->data_dtype == TK_DATA_F64 ? 8 : 4;
    TRY(ix->br_q.ensure((size_t)nq * ix->d * 4));
    TRY(ix->br_out.ensure((size_t)nq * k * 8));
    if (out_dist) TRY(ix->br_dist.ensure((size_t)nq * k * dsz));
    HIPCHECK(hipMemcpy(ix->br_q.p, q, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice));
    TRY(group_spans(ix, group_dev, nq));
    void *dist = out_dist ? ix->br_dist.p : nullptr;
    const float *X = ix->br_q.as<float>();
    int64_t *out = ix->br_out.as<int64_t>();
    if (ix->data_dtype == TK_DATA_F64) launch_group_exact<double, double>(ix, X, nq, k, r, out, dist);
    else if (ix->data_dtype == TK_DATA_F16) launch_group_exact<float, _Float16>(ix, X, nq, k, r, out, dist);
    else launch_group_exact<float, float>(ix, X, nq, k, r, out, dist);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out_ids, ix->br_out.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    if (out_dist) HIPCHECK(hipMemcpy(out_dist, dist, (size_t)nq * k * dsz, hipMemcpyDeviceToHost));
    return TK_OK;
}

extern "C" int tk_index_group_sizes(tk_index *ix, const int32_t *group, int64_t n, int64_t *out)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: row groups are not supported");
    ARGCHECK(n >= 0 && (n == 0 || (group && out)), "buffers");
    TRY(row_table_covers(ix, ix->groups));
    if (n == 0) return TK_OK;
    TRY(flush_pending(ix));
    TRY(group_rows_ensure(ix));
    const int32_t *group_dev = nullptr;
    TRY(gx_upload(ix->br_group, group, (size_t)n, group_dev));
    TRY(group_spans(ix, group_dev, n));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    std::vector<int32_t> len((size_t)n);
    HIPCHECK(hipMemcpy(len.data(), ix->gx_len.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) out[i] = len[(size_t)i];
    return TK_OK;
}

extern "C" int tk_index_group_rows(tk_index *ix, int64_t *info4)
{
    IXLOCK(ix);
    ARGCHECK(ix && info4, "null index / buffer");
    const TkRowTable &t = ix->groups;
    const bool have = t.span_state.current(t.set_gen) && t.n == ix->N;
    info4[0] = have ? 1 : 0;
    info4[1] = have ? ix->N * 4 + t.span_groups * 4 + (t.span_groups + 1) * 4 : 0;
    info4[2] = t.span_state.builds;
    info4[3] = have ? t.span_groups : 0;
    return TK_OK;
}
