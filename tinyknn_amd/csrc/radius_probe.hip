// radius_probe.hip — every row within a radius of each query among the rows of its probed lists
// (IVF.radius_search(n_probes=), tk_index_radius_probe): FAISS's range_search on an IVF index.  The brute
// call (radius.hip, §3.19) multiplies every query with all N rows; here a query reads the lists its coarse stage names
// and nothing else, and is exact inside them.
//
// For query i with n_probes = P:
//   probes      the index's own coarse stage for P (coarse_top_chunks, api_build.hip: tk_index_top_centers' chunks with
//               the (m, kc) rows kept on the device), kc = min(P, n_lists)
//   lists       the distinct lists that row names; a -1 left by an unfilled coarse heap names the last list, as the
//               reference's negative index does; a list named at two ranks is walked at the first
//   candidates  the labels in [0, N) at positions < list_n of those lists; a label stored in several probed lists
//               (build(n_probes >= 2)) is a candidate at the earliest rank that holds a copy — decided from the twin
//               table (twins.hip: the lists of a stored row's other copies) against the probes row, before any vector
//               is read.  The table is the index's own, or — where the index keeps none because its labels are sparse,
//               as after IVF.remove has thinned it — one the first call of a layout makes for itself
//               (radius_probe_twins, api_index.hip).  Refused (TK_ERR_STATE) is only what no table describes: a label
//               stored more than 17 times, copies with different codes or in one list, repeating labels beyond int32,
//               and a table that does not fit the free memory
//   hits        candidates that pass the restriction (TkBruteRestrict by row id, span_exact.h's formulas) with
//               sqdist_row<T, TY>(row, query) <= radius[i]: the rescoring's distance, float32 on float32 and half
//               stores, float64 on float64 vectors (the radius widened from float32), inclusive
// Passes:
//   words    rp_words_kernel: per (query, rank) the 64-row words its list needs, ceil(list_n / 64); 0 at a rank whose
//            list an earlier rank names.  tk_scan_exclusive64 over them: where each (query, rank)'s words begin.
//   count    radius_probe_count_kernel<T, TY, RESTRICTED>: one workgroup of 256 lanes per (query, rank), the query in
//            LDS in T, the list walked in blocks of 64 rows a wave, a lane a row.  The hit predicate is ballotted per
//            wave; the 64-bit ballot IS the bitmap word of that (query, rank, block), written by one lane — every word
//            of the bitmap is written, none needs zeroing — and the same lane adds its popcount to count[q]: one
//            atomic per wave and block with hits.  No barrier in the loop; lanes past list_n never vote.
//   offsets  the caller's: counts to the host, their prefix sum in int64 (the CSR lims), checked against the limit
//   fill     radius_probe_fill_kernel<T, TY>: the same grid.  A wave reads its bitmap words and skips the zero ones
//            without touching a label; for set bits only it reads the label and computes sqdist_row again — the same
//            function on the same bytes, the same bits — and stores the key at keys[offset[q] + slot], slot from a
//            second, zeroed counter (one atomic per wave and block).  A store is guarded by slot < count[q]; were the
//            passes to disagree the error flag is raised and nothing is written outside the query's segment.
//            Why a bitmap and not a second gather of every candidate: the fill reads the vectors of the hits alone.
//   sort     float32: the key is GxKey<float> high, the row id low, 64 bits — radius.hip's segmented sort as it is
//            (tk_launch_radius_sort: no second instantiation of rocPRIM's kernels).  float64: (GxKey<double>, row id)
//            is 96 bits; the same 64-bit sort runs twice instead — first the distance keys alone, then every entry
//            takes the position of the first key equal to its own in its sorted segment (a binary search: equal
//            distances get equal ranks) and (rank, row id) is sorted.  Both sorts order distinct 64-bit keys, so the
//            result does not depend on the order the fill left.
//   decode   keys -> int64 ids and distances
#include "api_internal.h"
#include "sqdist_row.h"
#include "span_exact.h"

#define RP_THREADS 256

struct RpJob {
    const float *q;                 // (nq, d) prepared queries
    const void *rows;               // the vectors, TY
    const int64_t *probes;          // (nq, kc)
    const int64_t *ids, *ids_off, *list_n;
    const int32_t *twin_list;       // twins.hip, twin_w > 0
    const float *radius;            // (nq)
    const long long *words, *woff;  // (nq * kc): bitmap words of the (query, rank), and where they begin
    unsigned long long *bitmap;
    int *count;                     // (nq)
    // fill
    const int64_t *offset;          // (nq) the exclusive prefix sum of count
    int *slots, *err;
    unsigned long long *keys;
    int32_t *key_rows;              // float64 vectors: the row id beside its distance key
    int64_t n_lists, N;
    int d, kc, twin_w;
};

// the list a probe names: -1 (an unfilled coarse heap) is the last list; -1 for what names none
__device__ __forceinline__ int32_t rp_list(int64_t p, int64_t n_lists)
{
    if (p < 0) p += n_lists;
    return (p >= 0 && p < n_lists) ? (int32_t)p : -1;
}

__global__ __launch_bounds__(256) void rp_words_kernel(const int64_t *__restrict__ probes, int64_t n, int kc,
                                                       int64_t n_lists, const int64_t *__restrict__ list_n,
                                                       long long *__restrict__ words)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {               // (the scan's last entry: the total)
        words[i] = 0;
        return;
    }
    const int rank = (int)(i % kc);
    const int64_t *row = probes + (i - rank);
    const int32_t L = rp_list(row[rank], n_lists);
    bool walk = L >= 0;
    for (int t = 0; walk && t < rank; t++) walk = rp_list(row[t], n_lists) != L;
    words[i] = walk ? (list_n[L] + 63) / 64 : 0;
}

template <typename T, typename TY, bool RESTRICTED>
__global__ __launch_bounds__(RP_THREADS) void radius_probe_count_kernel(const RpJob j, const TkBruteRestrict r)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *xs = (T *)smem;
    int32_t *pl = (int32_t *)(xs + j.d);            // the lists of the earlier ranks (read where the index has twins)
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t b = blockIdx.x;
    const int nw = (int)j.words[b];
    if (nw == 0) return;                            // an empty list, or one an earlier rank walks
    const int64_t qi = b / j.kc;
    const int rank = (int)(b - qi * j.kc);
    for (int t = tid; t < j.d; t += RP_THREADS) xs[t] = (T)j.q[qi * j.d + t];
    if (j.twin_w > 0)
        for (int t = tid; t < rank; t += RP_THREADS) pl[t] = rp_list(j.probes[qi * j.kc + t], j.n_lists);
    const int32_t L = rp_list(j.probes[b], j.n_lists);
    const int64_t n = j.list_n[L], base = j.ids_off[L];
    const T rad = (T)j.radius[qi];
    // the query's own attributes, once
    const int32_t q_ex = (RESTRICTED && r.exclude) ? (int32_t)r.exclude[qi] : -1;
    const uint64_t q_tags = (RESTRICTED && r.tags) ? r.tags[qi] : 0;
    const int32_t q_group = (RESTRICTED && r.group) ? r.group[qi] : -1;
    int64_t q_lo[4] = {0, 0, 0, 0}, q_hi[4] = {0, 0, 0, 0};
    if (RESTRICTED) {
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c < r.cols) {
                q_lo[c] = r.ranges[(qi * r.cols + c) * 2];
                q_hi[c] = r.ranges[(qi * r.cols + c) * 2 + 1];
            }
    }
    const TY *rows = (const TY *)j.rows;
    unsigned long long *bm = j.bitmap + j.woff[b];
    __syncthreads();                                // xs and pl
    for (int blk = tid >> 6; blk < nw; blk += RP_THREADS / 64) {
        const int64_t pos = (int64_t)blk * 64 + lane;
        bool h = false;
        if (pos < n) {
            const int64_t flat = base + pos, id = j.ids[flat];
            bool ok = id >= 0 && id < j.N;
            if (ok && j.twin_w > 0) {               // a copy in a list of an earlier rank: counted there
                for (int u = 0; u < j.twin_w; u++) {
                    const int32_t l2 = j.twin_list[flat * j.twin_w + u];
                    if (l2 < 0) break;
                    for (int t = 0; t < rank; t++) ok &= pl[t] != l2;
                }
            }
            if (RESTRICTED && ok) {
                const int32_t rid = (int32_t)id;
                if (r.allowed) ok &= (r.allowed[rid >> 5] >> (rid & 31)) & 1u;
                ok &= rid != q_ex;
                if (ok && q_group >= 0) ok = r.row_groups[rid] == q_group;
                if (ok && q_tags != 0) {
                    const uint64_t rt = r.row_tags[rid];
                    ok = r.tag_mode ? (rt & q_tags) == q_tags : (rt & q_tags) != 0;
                }
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (ok && c < r.cols) {
                        const int64_t key = r.row_keys[c * r.n_rows + rid];
                        ok = q_lo[c] <= key && key <= q_hi[c];
                    }
            }
            if (ok) h = sqdist_row<T, TY>(rows + id * j.d, xs, j.d) <= rad;
        }
        const unsigned long long m = __ballot(h);
        if (lane == 0) {
            bm[blk] = m;
            if (m) atomicAdd(&j.count[qi], __popcll(m));
        }
    }
}

template <typename T, typename TY>
__global__ __launch_bounds__(RP_THREADS) void radius_probe_fill_kernel(const RpJob j)
{
    typedef typename GxKey<T>::type K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T *xs = (T *)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t b = blockIdx.x;
    const int nw = (int)j.words[b];
    if (nw == 0) return;
    const int64_t qi = b / j.kc;
    for (int t = tid; t < j.d; t += RP_THREADS) xs[t] = (T)j.q[qi * j.d + t];
    const int32_t L = rp_list(j.probes[b], j.n_lists);
    const int64_t base = j.ids_off[L], off = j.offset[qi];
    const uint32_t cnt = (uint32_t)j.count[qi];
    const TY *rows = (const TY *)j.rows;
    const unsigned long long *bm = j.bitmap + j.woff[b];
    __syncthreads();                                // xs
    for (int blk = tid >> 6; blk < nw; blk += RP_THREADS / 64) {
        const unsigned long long m = bm[blk];
        if (m == 0) continue;                       // (the same word in every lane of the wave)
        int first = 0;
        if (lane == 0) first = atomicAdd(&j.slots[qi], __popcll(m));
        first = __shfl(first, 0);
        if (!((m >> lane) & 1ull)) continue;
        const int64_t id = j.ids[base + (int64_t)blk * 64 + lane];
        const K key = GxKey<T>::of(sqdist_row<T, TY>(rows + id * j.d, xs, j.d));
        const uint32_t slot = (uint32_t)first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (slot < cnt) {
            if constexpr (sizeof(K) == 4) {
                j.keys[off + slot] = ((unsigned long long)key << 32) | (uint32_t)id;
            } else {
                j.keys[off + slot] = key;
                j.key_rows[off + slot] = (int32_t)id;
            }
        } else {
            atomicOr(j.err, 1);
        }
    }
}

// float64 vectors, the second sort's keys: entry i of segment s takes the position of the first key of the sorted
// segment that equals its own (equal distances: equal ranks), in front of its row id.  keys is overwritten in place.
__global__ __launch_bounds__(256) void rp_rank_kernel(unsigned long long *__restrict__ keys,
                                                      const int32_t *__restrict__ key_rows,
                                                      const unsigned long long *__restrict__ sorted,
                                                      const int64_t *__restrict__ lims, int64_t nq, int64_t total)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int64_t lo = 0, hi = nq;                        // lims[lo] <= i < lims[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (lims[mid] <= i) lo = mid; else hi = mid;
    }
    const unsigned long long k = keys[i];
    int64_t a = lims[lo], e = lims[lo + 1];
    while (a < e) {
        const int64_t mid = (a + e) >> 1;
        if (sorted[mid] < k) a = mid + 1; else e = mid;
    }
    keys[i] = ((unsigned long long)a << 32) | (uint32_t)key_rows[i];
}

// float64 vectors: ranked != NULL: (rank, row id) keys, sorted, the rank an index into dkeys (ids may alias ranked);
// NULL: entry i is (dkeys[i], key_rows[i]), as the fill left them
__global__ __launch_bounds__(256) void rp_decode64_kernel(const unsigned long long *ranked,
                                                          const int32_t *__restrict__ key_rows,
                                                          const unsigned long long *__restrict__ dkeys, int64_t n,
                                                          int64_t *ids, double *__restrict__ dist)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (ranked) {
        const unsigned long long k = ranked[i];
        ids[i] = (int64_t)(uint32_t)k;
        dist[i] = GxKey<double>::back(dkeys[k >> 32]);
    } else {
        ids[i] = key_rows[i];
        dist[i] = GxKey<double>::back(dkeys[i]);
    }
}

static size_t rp_lds(const RpJob &j, size_t t_bytes, bool fill)
{
    return (size_t)j.d * t_bytes + (fill || j.twin_w == 0 ? 0 : (size_t)j.kc * 4);
}

template <typename T, typename TY>
static void rp_launch(const RpJob &j, int64_t nq, const TkBruteRestrict *r, bool fill)
{
    const dim3 grid((unsigned)(nq * j.kc)), block(RP_THREADS);
    if (fill)
        hipLaunchKernelGGL((radius_probe_fill_kernel<T, TY>), grid, block, rp_lds(j, sizeof(T), true), 0, j);
    else if (r)
        hipLaunchKernelGGL((radius_probe_count_kernel<T, TY, true>), grid, block, rp_lds(j, sizeof(T), false), 0, j, *r);
    else
        hipLaunchKernelGGL((radius_probe_count_kernel<T, TY, false>), grid, block, rp_lds(j, sizeof(T), false), 0, j,
                           TkBruteRestrict{});
}

static void rp_pass(const tk_index *ix, const RpJob &j, int64_t nq, const TkBruteRestrict *r, bool fill)
{
    if (ix->data_dtype == TK_DATA_F64) rp_launch<double, double>(j, nq, r, fill);
    else if (ix->data_dtype == TK_DATA_F16) rp_launch<float, _Float16>(j, nq, r, fill);
    else rp_launch<float, float>(j, nq, r, fill);
}

static int rp_sort(tk_index *ix, const unsigned long long *in, unsigned long long *out, int64_t total, int64_t nq)
{
    size_t bytes = 0;
    if (tk_launch_radius_sort(nullptr, &bytes, in, out, total, nq, ix->rd_off.as<int64_t>(), nullptr))
        return fail(TK_ERR_HIP, "tk_launch_radius_sort: work memory query failed");
    TRY(ix->rd_tmp.ensure(bytes > 0 ? bytes : 1));
    if (tk_launch_radius_sort(ix->rd_tmp.p, &bytes, in, out, total, nq, ix->rd_off.as<int64_t>(), nullptr))
        return fail(TK_ERR_HIP, "tk_launch_radius_sort failed");
    return TK_OK;
}

// ---- C ABI ----

extern "C" int tk_index_radius_probe(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq,
                                     int n_probes, const float *radius, const uint8_t *allowed_mask,
                                     const int64_t *exclude, const int32_t *group, const uint64_t *tags, int tag_mode,
                                     const int64_t *between, int sorted, int count_only, int64_t max_results,
                                     int64_t *out_lims, int64_t *out_total)
{
    IXLOCK(ix);
    if (ix) ix->rd_total = ix->rp_total = -1;       // whatever this call does, the result of the last one is gone
    ARGCHECK(ix && ix->have_data && ix->have_lists && ix->have_pq && ix->have_centers,
             "set_pq, set_centers, set_lists and set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: radius_search is not supported");
    ARGCHECK(n_probes >= 1, "n_probes >= 1");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    ARGCHECK(ix->d <= 4096, "d <= 4096");
    ARGCHECK(nq >= 0 && out_lims && out_total && (nq == 0 || (q && q_pq && radius)), "buffers");
    ARGCHECK(count_only || (max_results >= 0 && max_results < (1ll << 31)), "0 <= max_results < 2^31");
    for (int64_t i = 0; i < nq; i++) ARGCHECK(radius[i] == radius[i], "radius: NaN");
    const int32_t *twin_list = nullptr;
    int twin_w = 0;
    TRY(radius_probe_twins(ix, &twin_list, &twin_w));
    TkBruteRestrict r;
    bool any;
    TRY(brute_restrict(ix, nq, allowed_mask, exclude, group, tags, tag_mode, between, r, any));
    out_lims[0] = 0;
    *out_total = 0;
    if (nq == 0) {
        if (!count_only) ix->rp_total = 0, ix->rp_f64 = ix->data_dtype == TK_DATA_F64;
        return TK_OK;
    }
    TRY(flush_pending(ix));
    const int kc = (int)(n_probes < ix->n_lists ? n_probes : ix->n_lists);
    const int64_t pairs = nq * kc;
    ARGCHECK(pairs < (1ll << 31), "nq * min(n_probes, n_lists) < 2^31");
    TRY(ix->rp_probes.ensure((size_t)pairs * 8));
    TRY(ix->rp_words.ensure((size_t)(pairs + 1) * 8));
    TRY(ix->rp_woff.ensure((size_t)(pairs + 1) * 8));
    TRY(ix->br_q.ensure((size_t)nq * ix->d * 4));
    TRY(ix->rd_radius.ensure((size_t)nq * 4));
    TRY(ix->rd_count.ensure((size_t)nq * 8 + 4));
    // the coarse stage, chunk by chunk; its probes stay on the device
    TRY(coarse_top_chunks(ix, q, q_pq, q_pq_is_f64, nq, n_probes, false,
                          [&](int64_t o, int64_t m, int kc_, const int64_t *probes, const float *) -> int {
                              if (kc_ != kc) return fail(TK_ERR_HIP, "radius_probe: the coarse stage's row width");
                              HIPCHECK(hipMemcpy(ix->rp_probes.as<int64_t>() + o * kc, probes, (size_t)m * kc * 8,
                                                 hipMemcpyDeviceToDevice));
                              return TK_OK;
                          }));
    HIPCHECK(hipMemcpy(ix->br_q.p, q, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ix->rd_radius.p, radius, (size_t)nq * 4, hipMemcpyHostToDevice));
    // bitmap words per (query, rank) and where they begin
    long long *words = ix->rp_words.as<long long>(), *woff = ix->rp_woff.as<long long>();
    hipLaunchKernelGGL(rp_words_kernel, dim3((unsigned)((pairs + 256) / 256)), dim3(256), 0, 0,
                       ix->rp_probes.as<int64_t>(), pairs, kc, ix->n_lists, ix->list_n.as<int64_t>(), words);
    size_t sbytes = 0;
    (void)tk_scan_exclusive64(nullptr, &sbytes, words, woff, pairs + 1, nullptr);
    TRY(ix->rp_scan.ensure(sbytes));
    if (tk_scan_exclusive64(ix->rp_scan.p, &sbytes, words, woff, pairs + 1, nullptr))
        return fail(TK_ERR_HIP, "tk_scan_exclusive64 failed");
    HIPCHECK(hipGetLastError());
    long long n_words = 0;
    HIPCHECK(hipMemcpy(&n_words, woff + pairs, 8, hipMemcpyDeviceToHost));
    if ((double)n_words * 8.0 > workspace_bytes()) {
        char b[200];
        snprintf(b, sizeof b, "radius_search(n_probes=): the candidate bitmap of %lld queries needs %lld bytes, more than "
                              "the workspace budget; ask fewer queries per call", (long long)nq, n_words * 8);
        return fail(TK_ERR_WORKSPACE, b);
    }
    TRY(ix->rp_bitmap.ensure((size_t)(n_words > 0 ? n_words : 1) * 8));
    int *count = ix->rd_count.as<int>(), *slots = count + nq, *err = slots + nq;
    HIPCHECK(hipMemsetAsync(count, 0, (size_t)nq * 8 + 4, nullptr));
    RpJob j{};
    j.q = ix->br_q.as<float>();
    j.rows = ix->data.p;
    j.probes = ix->rp_probes.as<int64_t>();
    j.ids = ix->ids.as<int64_t>();
    j.ids_off = ix->ids_off.as<int64_t>();
    j.list_n = ix->list_n.as<int64_t>();
    j.twin_list = twin_list;
    j.radius = ix->rd_radius.as<float>();
    j.words = words;
    j.woff = woff;
    j.bitmap = ix->rp_bitmap.as<unsigned long long>();
    j.count = count;
    j.slots = slots;
    j.err = err;
    j.n_lists = ix->n_lists;
    j.N = ix->N;
    j.d = ix->d;
    j.kc = kc;
    j.twin_w = twin_w;
    rp_pass(ix, j, nq, any ? &r : nullptr, false);
    HIPCHECK(hipGetLastError());
    std::vector<int> counts((size_t)nq);
    HIPCHECK(hipMemcpy(counts.data(), count, (size_t)nq * 4, hipMemcpyDeviceToHost));     // (synchronises)
    for (int64_t i = 0; i < nq; i++) out_lims[i + 1] = out_lims[i] + counts[(size_t)i];
    const int64_t total = *out_total = out_lims[nq];
    if (count_only) return TK_OK;
    if (total > max_results) {
        char b[160];
        snprintf(b, sizeof b, "radius_search: %lld rows lie within the radii, more than max_results = %lld",
                 (long long)total, (long long)max_results);
        return fail(TK_ERR_ARG, b);
    }
    const bool f64 = ix->data_dtype == TK_DATA_F64;
    if (total == 0) {
        ix->rp_total = 0, ix->rp_f64 = f64;
        return TK_OK;
    }
    TRY(ix->rd_off.ensure((size_t)(nq + 1) * 8));
    TRY(ix->rd_keys.ensure((size_t)total * 8));
    TRY(ix->rd_alt.ensure((size_t)total * 8));
    TRY(ix->rp_ids.ensure((size_t)total * 8));
    TRY(ix->rp_dist.ensure((size_t)total * (f64 ? 8 : 4)));
    if (f64) TRY(ix->rp_rows.ensure((size_t)total * 4));
    HIPCHECK(hipMemcpy(ix->rd_off.p, out_lims, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice));
    unsigned long long *keys = ix->rd_keys.as<unsigned long long>(), *alt = ix->rd_alt.as<unsigned long long>();
    j.offset = ix->rd_off.as<int64_t>();
    j.keys = keys;
    j.key_rows = ix->rp_rows.as<int32_t>();
    rp_pass(ix, j, nq, nullptr, true);
    HIPCHECK(hipGetLastError());
    int bad = 0;
    HIPCHECK(hipMemcpy(&bad, err, 4, hipMemcpyDeviceToHost));
    if (bad) return fail(TK_ERR_HIP, "radius_search: count and fill passes disagree");
    int64_t *ids = ix->rp_ids.as<int64_t>();
    const unsigned grid = (unsigned)((total + 255) / 256);
    if (!f64) {
        if (sorted) TRY(rp_sort(ix, keys, alt, total, nq));
        tk_launch_radius_decode(sorted ? alt : keys, total, ids, ix->rp_dist.as<float>(), nullptr);
    } else if (sorted) {
        TRY(rp_sort(ix, keys, alt, total, nq));                                 // the distance keys alone
        hipLaunchKernelGGL(rp_rank_kernel, dim3(grid), dim3(256), 0, 0, keys, j.key_rows, alt, j.offset, nq, total);
        TRY(rp_sort(ix, keys, (unsigned long long *)ids, total, nq));           // (rank, row id)
        hipLaunchKernelGGL(rp_decode64_kernel, dim3(grid), dim3(256), 0, 0, (const unsigned long long *)ids,
                           j.key_rows, alt, total, ids, ix->rp_dist.as<double>());
    } else {
        hipLaunchKernelGGL(rp_decode64_kernel, dim3(grid), dim3(256), 0, 0, (const unsigned long long *)nullptr,
                           j.key_rows, keys, total, ids, ix->rp_dist.as<double>());
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    ix->rp_total = total;
    ix->rp_f64 = f64;
    return TK_OK;
}

extern "C" int tk_index_radius_probe_fetch(tk_index *ix, int64_t *out_ids, void *out_dist)
{
    IXLOCK(ix);
    ARGCHECK(ix, "index");
    if (ix->rp_total < 0)
        return fail(TK_ERR_STATE, "tk_index_radius_probe_fetch: no result is held (tk_index_radius_probe first; a call "
                                  "that failed or only counted holds none, and a later radius call of either kind "
                                  "drops it)");
    if (ix->rp_total == 0) return TK_OK;
    ARGCHECK(out_ids, "buffers");
    HIPCHECK(hipMemcpy(out_ids, ix->rp_ids.p, (size_t)ix->rp_total * 8, hipMemcpyDeviceToHost));
    if (out_dist)
        HIPCHECK(hipMemcpy(out_dist, ix->rp_dist.p, (size_t)ix->rp_total * (ix->rp_f64 ? 8 : 4),
                           hipMemcpyDeviceToHost));
    return TK_OK;
}
