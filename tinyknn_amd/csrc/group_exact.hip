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
//   the kernel      one workgroup per query.  The span is walked in tiles of GX_TILE rows, a lane a row: rows that are
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

#define GX_THREADS 256
#define GX_TILE 256       // rows of the span per pass of the workgroup: a lane a row
#define GX_CAP 2048       // entries of the candidate buffer; k + GX_TILE <= GX_CAP for every k <= 1024

// the distance as an unsigned key that orders as the distance does (a NaN, which no finite data gives, sorts last)
template <typename T> struct GxKey;
template <> struct GxKey<float> {
    typedef uint32_t type;
    __device__ static type of(float v)
    {
        const uint32_t u = __float_as_uint(v);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    __device__ static float back(type u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
};
template <> struct GxKey<double> {
    typedef uint64_t type;
    __device__ static type of(double v)
    {
        const uint64_t u = (uint64_t)__double_as_longlong(v);
        return (u >> 63) ? ~u : (u | (1ull << 63));
    }
    __device__ static double back(type u)
    {
        return __longlong_as_double((long long)((u >> 63) ? (u & ~(1ull << 63)) : ~u));
    }
};

// LDS: kd[GX_CAP] distance keys | kid[GX_CAP] row ids | x[d] the query in T
static size_t gx_lds_bytes(int d, size_t key_bytes, size_t t_bytes)
{
    return (size_t)GX_CAP * (key_bytes + 4) + (size_t)d * t_bytes;
}

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
    typedef typename GxKey<T>::type K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    K *kd = (K *)smem;
    int32_t *kid = (int32_t *)(kd + GX_CAP);
    T *xs = (T *)(kid + GX_CAP);
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    for (int t = tid; t < d; t += GX_THREADS) xs[t] = (T)q[qi * d + t];
    if (tid == 0) s_count = 0;
    // the query's own attributes, once
    const int64_t q_ex = r.exclude ? r.exclude[qi] : -1;
    const uint64_t q_tags = r.tags ? r.tags[qi] : 0;
    int64_t q_lo[4] = {0, 0, 0, 0}, q_hi[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (c < r.cols) {
            q_lo[c] = r.ranges[(qi * r.cols + c) * 2];
            q_hi[c] = r.ranges[(qi * r.cols + c) * 2 + 1];
        }
    const int n = len[qi];
    const int32_t *span = span_rows + begin[qi];
    K tau = ~(K)0;          // the bound: the k-th distance key of the last cut
    int kept = 0;           // entries the buffer holds at most (an upper bound, the same in every lane)

    // Sort what the buffer holds by (distance, row id), keep the k best, tighten the bound.  Every lane arrives.
    auto cut = [&]() {
        __syncthreads();                        // every append so far is in LDS (and the first time: xs, s_count)
        const int nc = s_count < GX_CAP ? s_count : GX_CAP;
        int P = 1;
        while (P < nc) P <<= 1;
        for (int e = nc + tid; e < P; e += GX_THREADS) {
            kd[e] = ~(K)0;
            kid[e] = 0x7fffffff;
        }
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int e = tid; e < P / 2; e += GX_THREADS) {
                    const int lo = (e / stride) * 2 * stride + (e % stride), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const K a = kd[lo], b = kd[hi];
                    const int32_t ia = kid[lo], ib = kid[hi];
                    const bool gt = a > b || (a == b && ia > ib);
                    if (gt == up) {
                        kd[lo] = b; kd[hi] = a;
                        kid[lo] = ib; kid[hi] = ia;
                    }
                }
                __syncthreads();
            }
        kept = nc < k ? nc : k;
        if (nc >= k) tau = kd[k - 1];
        if (tid == 0) s_count = kept;
        __syncthreads();                        // the count is back before the next append, tau read before it
    };

    __syncthreads();                            // xs and the zero count, before the first append
    for (int t0 = 0; t0 < n; t0 += GX_TILE) {
        if (kept + GX_TILE > GX_CAP) cut();
        kept += GX_TILE;
        const int t = t0 + tid;
        if (t >= n) continue;
        const int32_t rid = span[t];
        bool ok = (stored[rid >> 5] >> (rid & 31)) & 1u;
        if (r.allowed) ok &= (r.allowed[rid >> 5] >> (rid & 31)) & 1u;
        ok &= (int64_t)rid != q_ex;
        if (!ok) continue;
        if (q_tags != 0) {
            const uint64_t rt = r.row_tags[rid];
            if (!(r.tag_mode ? (rt & q_tags) == q_tags : (rt & q_tags) != 0)) continue;
        }
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c < r.cols) {
                const int64_t key = r.row_keys[c * r.n_rows + rid];
                ok &= q_lo[c] <= key && key <= q_hi[c];
            }
        if (!ok) continue;
        const T dv = sqdist_row<T, TY>(rows + (int64_t)rid * d, xs, d);
        const K key = GxKey<T>::of(dv);
        if (key <= tau) {
            const int pos = atomicAdd(&s_count, 1);
            if (pos < GX_CAP) {                 // (always: kept bounds the count)
                kd[pos] = key;
                kid[pos] = rid;
            }
        }
    }
    cut();
    for (int e = tid; e < k; e += GX_THREADS) {
        out[qi * k + e] = e < kept ? (int64_t)kid[e] : -1;
        if (out_d) out_d[qi * k + e] = e < kept ? GxKey<T>::back(kd[e]) : (T)__builtin_huge_valf();
    }
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
static int stored_bits_ensure(tk_index *ix)
{
    if (ix->stored_state.current(ix->lists_gen)) return TK_OK;
    TRY(table_may_build(ix, "stored-row", "tk_index_knn_group"));
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
    TRY(stored_bits_ensure(ix));
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
