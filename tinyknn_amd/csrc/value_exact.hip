// value_exact.hip — the exact k nearest rows inside a query's value range (tk_index_knn_between).
//
// knn_brute(between=) multiplies every query with all N rows whatever the range admits, and the probed lists of
// query_batch(between=) hold too few rows of a narrow range.  A range over ONE column is a contiguous span of the rows
// sorted by that column, so here a query walks such a span and nothing else: the cost follows the span's length.
//   rows by value   value_rows.hip: per value column a plane of N row ids ascending by (key, row id), 4 N bytes; made
//                   by the first call that needs it and again after tk_index_set_values.
//   the span        range_span_kernel, a lane a query: for every column the query bounds, the lower bound of lo and
//                   the upper bound of hi in the column's order (two binary searches that read a key through its row
//                   id); the query walks the SHORTEST of them, ties to the lowest column.  lo > hi gives length 0.
//   the walk        span_exact.h's, group_exact.hip's too: one workgroup per query, every condition tested by row id —
//                   every bounded column (the span's own again: harmless), allowed bit, exclude, group, tags — the
//                   survivors ranked by sqdist_row.  The span is in value order, not ascending by row id; the walk's
//                   last sort by (distance key, row id) makes the answer the same.
// One workgroup reads a whole span: for wide ranges knn_brute(between=) on the matrix cores is the call
// (IVF.query_batch(between=, exact_below=) routes by length).
#include "api_internal.h"
#include "span_exact.h"

// ranges: (n, cols, 2) inclusive int64 keys, INT64_MIN / INT64_MAX for an end that is not bounded.  ord: cols planes
// of N row ids in the column's order; keys: cols planes of N keys by row id.  -> col (-1: no column is bounded, the
// span is every row: begin 0, len N), begin within the column's plane, len.
__global__ __launch_bounds__(256) void range_span_kernel(const int64_t *__restrict__ ranges, int64_t n, int cols,
                                                         const int32_t *__restrict__ ord,
                                                         const int64_t *__restrict__ keys, int64_t N,
                                                         int32_t *__restrict__ col, int32_t *__restrict__ begin,
                                                         int32_t *__restrict__ len)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t kmin = (int64_t)1 << 63, kmax = ~kmin;
    int best_c = -1;
    int64_t best_b = 0, best_len = N;
    for (int c = 0; c < cols; c++) {
        const int64_t lo = ranges[(i * cols + c) * 2], hi = ranges[(i * cols + c) * 2 + 1];
        if (lo == kmin && hi == kmax) continue;
        const int32_t *o = ord + (int64_t)c * N;
        const int64_t *kc = keys + (int64_t)c * N;
        int64_t b = 0, e = N;               // b: the first position whose key is >= lo
        while (b < e) {
            const int64_t mid = (b + e) >> 1;
            if (kc[o[mid]] < lo) b = mid + 1;
            else e = mid;
        }
        int64_t u = 0, v = N;               // u: the first position whose key is > hi
        while (u < v) {
            const int64_t mid = (u + v) >> 1;
            if (kc[o[mid]] <= hi) u = mid + 1;
            else v = mid;
        }
        const int64_t l = u > b ? u - b : 0;
        if (best_c < 0 || l < best_len) best_c = c, best_b = b, best_len = l;
    }
    col[i] = best_c;
    begin[i] = (int32_t)best_b;
    len[i] = (int32_t)best_len;
}

// r: the restriction's device arrays (TkBruteRestrict), all of them tested.  col / begin / len: the query's span of
// ord's planes of N row ids (range_span_kernel's; a query without a column walks nothing).  stored: the N-bit map.
template <typename T, typename TY>
__global__ __launch_bounds__(GX_THREADS) void range_exact_kernel(const float *__restrict__ q, int d,
                                                                 const TY *__restrict__ rows,
                                                                 const int32_t *__restrict__ ord, int64_t N,
                                                                 const int32_t *__restrict__ col,
                                                                 const int32_t *__restrict__ begin,
                                                                 const int32_t *__restrict__ len,
                                                                 const uint32_t *__restrict__ stored,
                                                                 const TkBruteRestrict r, int k,
                                                                 int64_t *__restrict__ out, T *__restrict__ out_d)
{
    const int64_t qi = blockIdx.x;
    const int c = col[qi];
    span_exact_body<T, TY, true>(q, d, rows, ord + (int64_t)(c < 0 ? 0 : c) * N + begin[qi], c < 0 ? 0 : len[qi],
                                 stored, r, k, out, out_d);
}

// the spans of n queries' ranges (device, (n, cols, 2)) -> col / begin / len (device, the index's gx_ buffers)
static int range_spans(tk_index *ix, const int64_t *ranges_dev, int64_t n)
{
    TRY(ix->gx_col.ensure((size_t)n * 4));
    TRY(ix->gx_begin.ensure((size_t)n * 4));
    TRY(ix->gx_len.ensure((size_t)n * 4));
    hipLaunchKernelGGL(range_span_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ranges_dev, n,
                       value_columns(ix), ix->values.span_rows.as<int32_t>(), ix->values.by_row.as<int64_t>(), ix->N,
                       ix->gx_col.as<int32_t>(), ix->gx_begin.as<int32_t>(), ix->gx_len.as<int32_t>());
    return TK_OK;
}

template <typename T, typename TY>
static void launch_range_exact(const tk_index *ix, const float *q, int64_t nq, int k, const TkBruteRestrict &r,
                               int64_t *out, void *out_d)
{
    const size_t lds = gx_lds_bytes(ix->d, sizeof(typename GxKey<T>::type), sizeof(T));
    hipLaunchKernelGGL((range_exact_kernel<T, TY>), dim3((unsigned)nq), dim3(GX_THREADS), lds, 0, q, ix->d,
                       ix->data.as<TY>(), ix->values.span_rows.as<int32_t>(), ix->N, ix->gx_col.as<int32_t>(),
                       ix->gx_begin.as<int32_t>(), ix->gx_len.as<int32_t>(), ix->stored_bits.as<uint32_t>(), r, k, out,
                       (T *)out_d);
}

// A host array of the call in its workspace buffer (NULL stays NULL)
template <typename T>
static int vx_upload(DevBuf &b, const T *host, size_t n, const T *&dev)
{
    dev = nullptr;
    if (!host) return TK_OK;
    TRY(b.ensure((n > 0 ? n : 1) * sizeof(T)));
    HIPCHECK(hipMemcpy(b.p, host, n * sizeof(T), hipMemcpyHostToDevice));
    dev = b.as<T>();
    return TK_OK;
}

// query i of (n, cols, 2) host keys bounds some column
static bool range_bounded(const int64_t *between, int64_t i, int cols)
{
    for (int c = 0; c < cols; c++)
        if (between[(i * cols + c) * 2] != INT64_MIN || between[(i * cols + c) * 2 + 1] != INT64_MAX) return true;
    return false;
}

// ---- C ABI ----

extern "C" int tk_index_knn_between(tk_index *ix, const float *q, int64_t nq, int k, const int64_t *between,
                                    const uint8_t *allowed_mask, const int64_t *exclude, const int32_t *group,
                                    const uint64_t *tags, int tag_mode, int64_t *out_ids, void *out_dist)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: knn_between is not supported");
    ARGCHECK(nq >= 0 && (nq == 0 || (q && out_ids)), "buffers");
    ARGCHECK(nq == 0 || between, "between: the ranges of every query are required");
    ARGCHECK(k >= 1 && k <= 1024 && k <= ix->N, "1 <= k <= min(1024, N)");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    ARGCHECK(ix->d <= 4096, "d <= 4096");
    ARGCHECK(tag_mode == 0 || tag_mode == 1, "tag_mode: 0 (any) or 1 (all)");
    TRY(row_table_covers(ix, ix->values));
    if (group) TRY(row_table_covers(ix, ix->groups));
    if (tags) TRY(row_table_covers(ix, ix->tags));
    const int cols = value_columns(ix);
    for (int64_t i = 0; i < nq; i++)
        ARGCHECK(range_bounded(between, i, cols),
                 "between: query " + std::to_string(i) + " bounds no column (an unrestricted query is "
                 "tk_index_knn_brute's or tk_index_query_batch's to answer)");
    if (group)
        for (int64_t i = 0; i < nq; i++) ARGCHECK(group[i] >= -1, "group: entries must be a group id >= 0 or -1");
    if (exclude)
        for (int64_t i = 0; i < nq; i++) ARGCHECK(exclude[i] >= -1 && exclude[i] < ix->N, "exclude: entries in [-1, N)");
    if (nq == 0) return TK_OK;
    TRY(flush_pending(ix));
    TRY(value_rows_ensure(ix));
    TRY(stored_bits_ensure(ix, "tk_index_knn_between"));
    TkBruteRestrict r{};
    r.n_rows = ix->N;
    r.tag_mode = tag_mode;
    if (allowed_mask) {
        std::vector<uint32_t> bits((size_t)(ix->N + 31) / 32, 0u);
        for (int64_t j = 0; j < ix->N; j++) bits[(size_t)(j >> 5)] |= (uint32_t)(allowed_mask[j] != 0) << (j & 31);
        TRY(vx_upload(ix->br_mask, bits.data(), bits.size(), r.allowed));
    }
    TRY(vx_upload(ix->br_exclude, exclude, (size_t)nq, r.exclude));
    TRY(vx_upload(ix->br_group, group, (size_t)nq, r.group));
    if (group) r.row_groups = ix->groups.by_row.as<int32_t>();
    TRY(vx_upload(ix->br_tags, tags, (size_t)nq, r.tags));
    if (tags) r.row_tags = ix->tags.by_row.as<uint64_t>();
    r.cols = cols;
    r.row_keys = ix->values.by_row.as<int64_t>();
    TRY(vx_upload(ix->br_ranges, between, (size_t)nq * 2 * cols, r.ranges));
    const size_t dsz = ix->data_dtype == TK_DATA_F64 ? 8 : 4;
    TRY(ix->br_q.ensure((size_t)nq * ix->d * 4));
    TRY(ix->br_out.ensure((size_t)nq * k * 8));
    if (out_dist) TRY(ix->br_dist.ensure((size_t)nq * k * dsz));
    HIPCHECK(hipMemcpy(ix->br_q.p, q, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice));
    TRY(range_spans(ix, r.ranges, nq));
    void *dist = out_dist ? ix->br_dist.p : nullptr;
    const float *X = ix->br_q.as<float>();
    int64_t *out = ix->br_out.as<int64_t>();
    if (ix->data_dtype == TK_DATA_F64) launch_range_exact<double, double>(ix, X, nq, k, r, out, dist);
    else if (ix->data_dtype == TK_DATA_F16) launch_range_exact<float, _Float16>(ix, X, nq, k, r, out, dist);
    else launch_range_exact<float, float>(ix, X, nq, k, r, out, dist);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out_ids, ix->br_out.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    if (out_dist) HIPCHECK(hipMemcpy(out_dist, dist, (size_t)nq * k * dsz, hipMemcpyDeviceToHost));
    return TK_OK;
}

extern "C" int tk_index_range_sizes(tk_index *ix, const int64_t *between, int64_t n, int64_t *out_len,
                                    int32_t *out_col)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: row values are not supported");
    ARGCHECK(n >= 0 && (n == 0 || (between && out_len && out_col)), "buffers");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    TRY(row_table_covers(ix, ix->values));
    if (n == 0) return TK_OK;
    TRY(flush_pending(ix));
    TRY(value_rows_ensure(ix));
    const int64_t *ranges_dev = nullptr;
    TRY(vx_upload(ix->br_ranges, between, (size_t)n * 2 * value_columns(ix), ranges_dev));
    TRY(range_spans(ix, ranges_dev, n));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    std::vector<int32_t> len((size_t)n);
    HIPCHECK(hipMemcpy(len.data(), ix->gx_len.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(out_col, ix->gx_col.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) out_len[i] = len[(size_t)i];
    return TK_OK;
}

extern "C" int tk_index_value_rows(tk_index *ix, int64_t *info4)
{
    IXLOCK(ix);
    ARGCHECK(ix && info4, "null index / buffer");
    const TkRowTable &t = ix->values;
    const bool have = t.span_state.current(t.set_gen) && t.n == ix->N && t.n > 0;
    info4[0] = have ? 1 : 0;
    info4[1] = have ? t.span_groups * ix->N * 4 : 0;
    info4[2] = t.span_state.builds;
    info4[3] = have ? t.span_groups : 0;
    return TK_OK;
}
