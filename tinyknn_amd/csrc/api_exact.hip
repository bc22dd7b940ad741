// api_exact.hip — the exact calls over all rows (knn_brute and its restricted and matrix forms, radius_brute) and what
// every exact call shares on the host: the restriction builder, the radius tail.
#include "api_internal.h"
#include "probe_job.h"

// ---------------------------------------------------------------------------
// exact k nearest vectors of IVF.data: the ground truth of recall (brute.hip)
// r (or NULL): the restriction, its arrays on the device.  retry: a candidate list that overflowed under the segment
// rule is not an error — the selection runs once more from the sampled tau with the segment length that cannot
// overflow, the largest multiple of 32 not above cap - k (a segment appends at most `seg` rows to at most k kept ones).
// matrix: the rows are half and the tiles run on the f16 matrix cores (brute_matrix.hip); the values are
// §3.22's dist_m and d may reach 4096.  false: float32 rows, d <= 128, numpy's part values.
// wide (not beside matrix): float32 rows through the slabbed tile kernel (brute_wide.hip): the same part
// values and d may reach 4096.
static int knn_brute(tk_index *ix, const float *q, int64_t nq, int k, const TkBruteRestrict *r, bool retry,
                     int64_t *out_ids, float *out_dist, bool matrix = false, bool wide = false)
{
    ARGCHECK(ix && ix->have_data, "set_data first");
    if (matrix) {           // (tk_index_knn_brute_matrix has made pm_check's refusals)
        ARGCHECK(ix->d <= 4096, "d <= 4096");
    } else {
        ARGCHECK(ix->data_dtype != TK_DATA_F64, "float32 vectors only");
        ARGCHECK(ix->data_dtype != TK_DATA_F16, "knn_brute is the ground truth on float32 vectors: this index stores "
                                                "them as half (store=\"float16\"); ask a float32 index");
        if (wide) ARGCHECK(ix->d <= 4096, "d <= 4096");
        else ARGCHECK(ix->d <= 128, "d <= 128");
    }
    ARGCHECK(nq >= 0 && q && out_ids, "buffers");
    ARGCHECK(k >= 1 && k <= 1024 && k <= ix->N, "1 <= k <= min(1024, N)");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    if (nq == 0) return TK_OK;
    TRY(flush_pending(ix));
    const int64_t ns = ix->N < 8192 ? ix->N : 8192;
    const int cap = 8192;
    TRY(ix->br_ynorm.ensure((size_t)ix->N * 4));
    TRY(ix->br_tau.ensure((size_t)nq * 4 * 2));              // tau, and its copy as the sample gave it
    TRY(ix->br_vals.ensure((size_t)nq * ns * 4));
    TRY(ix->br_cand.ensure((size_t)nq * cap * 8));
    TRY(ix->br_count.ensure((size_t)nq * 4 + 4));
    TRY(ix->br_out.ensure((size_t)nq * k * 8));
    TRY(ix->br_q.ensure((size_t)nq * ix->d * 4));
    TRY(ix->br_sample.ensure((size_t)ns * (ix->d + 1) * 4));
    if (out_dist) TRY(ix->br_dist.ensure((size_t)nq * k * 4));
    HIPCHECK(hipMemcpy(ix->br_q.p, q, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice));
    int *overflow = ix->br_count.as<int>() + nq;
    float *tau = ix->br_tau.as<float>(), *tau0 = tau + nq, *dist = out_dist ? ix->br_dist.as<float>() : nullptr;
    const float *X = ix->br_q.as<float>(), *Y = ix->data.as<float>();
    PmQueries pq{};
    if (matrix) TRY(pm_prepare(ix, nq, pq));
    const TkBruteMatrix planes{pq.xh, pq.xl, pq.xn, pq.xs, pq.dpad}, *mx = matrix ? &planes : nullptr;
    if (wide) {
        TRY(ix->bw_x2.ensure((size_t)nq * tk_brute_wide_dq(ix->d) * 4));
        TRY(ix->bw_xn.ensure((size_t)nq * 4));
        tk_launch_brute_wide_prepare(X, nq, ix->d, ix->bw_x2.as<float>(), ix->bw_xn.as<float>(), nullptr);
    }
    const TkBruteWide doubled{ix->bw_x2.as<float>(), ix->bw_xn.as<float>(), tk_brute_wide_dq(ix->d)},
        *wd = wide ? &doubled : nullptr;
    if (tk_launch_brute_tau(X, nq, ix->d, Y, ix->N, k, ix->br_ynorm.as<float>(), ix->br_vals.as<float>(), ns, tau,
                            ix->br_sample.as<float>(), r, nullptr, mx, wd))
        return fail(TK_ERR_HIP, "tk_launch_knn_brute: unsupported size / LDS attribute");
    if (retry) HIPCHECK(hipMemcpyAsync(tau0, tau, (size_t)nq * 4, hipMemcpyDeviceToDevice, nullptr));
    int64_t seg = tk_brute_segment(k, ns, cap);
    for (int attempt = 0;; attempt++) {
        if (tk_launch_brute_select(X, nq, ix->d, Y, ix->N, k, ix->br_ynorm.as<float>(), tau,
                                   ix->br_cand.as<unsigned long long>(), cap, ix->br_count.as<int>(), overflow,
                                   ix->br_out.as<int64_t>(), dist, seg, r, nullptr, mx, wd))
            return fail(TK_ERR_HIP, "tk_launch_knn_brute: unsupported size / LDS attribute");
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        int ov = 0;
        HIPCHECK(hipMemcpy(&ov, overflow, 4, hipMemcpyDeviceToHost));
        if (!ov) break;
        if (!retry || attempt == 1)
            return fail(TK_ERR_HIP, "knn_brute: candidate list overflow (one segment of rows holds more than 8192 rows within a query's running k-th distance: tied or stored together)");
        HIPCHECK(hipMemcpyAsync(tau, tau0, (size_t)nq * 4, hipMemcpyDeviceToDevice, nullptr));
        seg = (cap - k) / 32 * 32;
    }
    HIPCHECK(hipMemcpy(out_ids, ix->br_out.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    if (out_dist) HIPCHECK(hipMemcpy(out_dist, dist, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    return TK_OK;
}

extern "C" int tk_index_knn_brute(tk_index *ix, const float *q, int64_t nq, int k, int64_t *out_ids)
{
    IXLOCK(ix);
    return knn_brute(ix, q, nq, k, nullptr, false, out_ids, nullptr);
}

// ---- the restriction of an exact call from the caller's host arrays (api_internal.h: the phases) ----
int restrict_mode(const TkHostRestrict &h)
{
    ARGCHECK(h.tag_mode == 0 || h.tag_mode == 1, "tag_mode: 0 (any) or 1 (all)");
    return TK_OK;
}

int restrict_tables(const tk_index *ix, const TkHostRestrict &h)
{
    if (h.group) TRY(row_table_covers(ix, ix->groups));
    if (h.tags) TRY(row_table_covers(ix, ix->tags));
    if (h.between) TRY(row_table_covers(ix, ix->values));
    return TK_OK;
}

int restrict_ranges(const tk_index *ix, int64_t nq, const TkHostRestrict &h)
{
    if (h.exclude)
        for (int64_t i = 0; i < nq; i++)
            ARGCHECK(h.exclude[i] >= -1 && h.exclude[i] < ix->N, "exclude: entries in [-1, N)");
    return TK_OK;
}

int restrict_upload(tk_index *ix, int64_t nq, const TkHostRestrict &h, TkBruteRestrict &r, bool &any)
{
    r = TkBruteRestrict{};
    any = h.any();
    if (!any || nq == 0) return TK_OK;
    r.n_rows = ix->N;
    r.tag_mode = h.tag_mode;
    if (h.allowed_mask) {
        const std::vector<uint32_t> bits = pack_row_mask(h.allowed_mask, ix->N);
        TRY(host_upload(ix->br_mask, bits.data(), bits.size(), r.allowed));
    }
    TRY(host_upload(ix->br_exclude, h.exclude, (size_t)nq, r.exclude));
    TRY(host_upload(ix->br_group, h.group, (size_t)nq, r.group));
    TRY(host_upload(ix->br_tags, h.tags, (size_t)nq, r.tags));
    if (h.group) r.row_groups = ix->groups.by_row.as<int32_t>();
    if (h.tags) r.row_tags = ix->tags.by_row.as<uint64_t>();
    if (h.between) {
        r.cols = value_columns(ix);
        r.row_keys = ix->values.by_row.as<int64_t>();
        TRY(host_upload(ix->br_ranges, h.between, (size_t)nq * 2 * r.cols, r.ranges));
    }
    return TK_OK;
}

int brute_restrict(tk_index *ix, int64_t nq, const TkHostRestrict &h, TkBruteRestrict &r, bool &any)
{
    TRY(restrict_mode(h));
    TRY(restrict_tables(ix, h));
    TRY(restrict_ranges(ix, nq, h));
    return restrict_upload(ix, nq, h, r, any);
}

extern "C" int tk_index_knn_brute_ex(tk_index *ix, const float *q, int64_t nq, int k, const uint8_t *allowed_mask,
                                     const int64_t *exclude, const int32_t *group, const uint64_t *tags, int tag_mode,
                                     const int64_t *between, int64_t *out_ids, float *out_dist)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: knn_brute with restrictions is not supported");
    ARGCHECK(nq >= 0, "buffers");
    TkBruteRestrict r;
    bool any;
    TRY(brute_restrict(ix, nq, {allowed_mask, exclude, group, tags, tag_mode, between}, r, any));
    if (!any) return knn_brute(ix, q, nq, k, nullptr, true, out_ids, out_dist);
    if (nq == 0) return TK_OK;
    return knn_brute(ix, q, nq, k, &r, true, out_ids, out_dist);
}

// tk_index_knn_brute_ex on the f16 matrix cores for a half store, d <= 4096 (brute_matrix.hip)
extern "C" int tk_index_knn_brute_matrix(tk_index *ix, const float *q, int64_t nq, int k, const uint8_t *allowed_mask,
                                         const int64_t *exclude, const int32_t *group, const uint64_t *tags,
                                         int tag_mode, const int64_t *between, int64_t *out_ids, float *out_dist)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: knn_brute(matrix=True) is not supported");
    ARGCHECK(nq >= 0 && (nq == 0 || q), "buffers");
    TRY(pm_check(ix, q, nq));
    // (knn_brute's own, here in front of the restriction's uploads: nothing reaches the device for a refused call)
    ARGCHECK(ix->d <= 4096, "d <= 4096");
    ARGCHECK(k >= 1 && k <= 1024 && k <= ix->N, "1 <= k <= min(1024, N)");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    TkBruteRestrict r;
    bool any;
    TRY(brute_restrict(ix, nq, {allowed_mask, exclude, group, tags, tag_mode, between}, r, any));
    if (any && nq == 0) return TK_OK;
    return knn_brute(ix, q, nq, k, any ? &r : nullptr, true, out_ids, out_dist, true);
}

// tk_index_knn_brute_ex for a float32 store of any d <= 4096: the same part values from the slabbed tile kernel
// (brute_wide.hip)
extern "C" int tk_index_knn_brute_wide(tk_index *ix, const float *q, int64_t nq, int k, const uint8_t *allowed_mask,
                                       const int64_t *exclude, const int32_t *group, const uint64_t *tags,
                                       int tag_mode, const int64_t *between, int64_t *out_ids, float *out_dist)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: knn_brute(wide=True) is not supported");
    ARGCHECK(nq >= 0 && (nq == 0 || q), "buffers");
    // (knn_brute's own, here in front of the restriction's uploads: nothing reaches the device for a refused call)
    ARGCHECK(ix->data_dtype != TK_DATA_F64, "wide=True needs store=\"float32\": this index stores float64 vectors");
    ARGCHECK(ix->data_dtype != TK_DATA_F16, "wide=True needs store=\"float32\": this index stores its vectors as half "
                                            "(store=\"float16\"); its search over all rows is matrix=True");
    ARGCHECK(ix->d <= 4096, "d <= 4096");
    ARGCHECK(k >= 1 && k <= 1024 && k <= ix->N, "1 <= k <= min(1024, N)");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    TkBruteRestrict r;
    bool any;
    TRY(brute_restrict(ix, nq, {allowed_mask, exclude, group, tags, tag_mode, between}, r, any));
    if (any && nq == 0) return TK_OK;
    return knn_brute(ix, q, nq, k, any ? &r : nullptr, true, out_ids, out_dist, false, true);
}

// ---------------------------------------------------------------------------
// the tail of the two radius calls (api_internal.h)
int radius_lims(tk_index *ix, const int *count, int64_t nq, int count_only, int64_t max_results, int64_t *out_lims,
                int64_t *out_total, bool &fill)
{
    fill = false;
    std::vector<int> counts((size_t)nq);
    HIPCHECK(hipMemcpy(counts.data(), count, (size_t)nq * 4, hipMemcpyDeviceToHost));     // (synchronises)
    for (int64_t i = 0; i < nq; i++) out_lims[i + 1] = out_lims[i] + counts[(size_t)i];   // int64: nq x N may pass 2^31
    const int64_t total = *out_total = out_lims[nq];
    if (count_only) return TK_OK;
    if (total > max_results) {
        char b[160];
        snprintf(b, sizeof b, "radius_search: %lld rows lie within the radii, more than max_results = %lld",
                 (long long)total, (long long)max_results);
        return fail(TK_ERR_ARG, b);
    }
    if (total == 0) return TK_OK;
    TRY(ix->rd_off.ensure((size_t)(nq + 1) * 8));
    TRY(ix->rd_keys.ensure((size_t)total * 8));
    TRY(ix->rd_alt.ensure((size_t)total * 8));
    HIPCHECK(hipMemcpy(ix->rd_off.p, out_lims, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice));
    fill = true;
    return TK_OK;
}

int radius_passes_agree(const int *err)
{
    int bad = 0;
    HIPCHECK(hipMemcpy(&bad, err, 4, hipMemcpyDeviceToHost));
    if (bad) return fail(TK_ERR_HIP, "radius_search: count and fill passes disagree");
    return TK_OK;
}

int radius_sort(tk_index *ix, const unsigned long long *in, unsigned long long *out, int64_t total, int64_t nq)
{
    size_t bytes = 0;
    if (tk_launch_radius_sort(nullptr, &bytes, in, out, total, nq, ix->rd_off.as<int64_t>(), nullptr))
        return fail(TK_ERR_HIP, "tk_launch_radius_sort: work memory query failed");
    TRY(ix->rd_tmp.ensure(bytes > 0 ? bytes : 1));
    if (tk_launch_radius_sort(ix->rd_tmp.p, &bytes, in, out, total, nq, ix->rd_off.as<int64_t>(), nullptr))
        return fail(TK_ERR_HIP, "tk_launch_radius_sort failed");
    return TK_OK;
}

// ---------------------------------------------------------------------------
// every row within a radius of each query (radius.hip): count pass, offsets on the host, fill pass,
// segmented sort, decode; the decoded result stays in the index for tk_index_radius_fetch
extern "C" int tk_index_radius_brute(tk_index *ix, const float *q, int64_t nq, const float *radius,
                                     const uint8_t *allowed_mask, const int64_t *exclude, const int32_t *group,
                                     const uint64_t *tags, int tag_mode, const int64_t *between, int sorted,
                                     int count_only, int64_t max_results, int64_t *out_lims, int64_t *out_total)
{
    IXLOCK(ix);
    if (ix) ix->rd_total = ix->rp_total = -1;       // whatever this call does, the result of the last one is gone
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: radius_search is not supported");
    ARGCHECK(ix->data_dtype != TK_DATA_F64, "float32 vectors only");
    ARGCHECK(ix->data_dtype != TK_DATA_F16, "radius_search compares knn_brute's part values on float32 vectors: this "
                                            "index stores them as half (store=\"float16\"); ask a float32 index");
    ARGCHECK(ix->d <= 128, "d <= 128");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    ARGCHECK(nq >= 0 && out_lims && out_total && (nq == 0 || (q && radius)), "buffers");
    ARGCHECK(count_only || (max_results >= 0 && max_results < (1ll << 31)), "0 <= max_results < 2^31");
    for (int64_t i = 0; i < nq; i++) ARGCHECK(radius[i] == radius[i], "radius: NaN");
    TkBruteRestrict r;
    bool any;
    TRY(brute_restrict(ix, nq, {allowed_mask, exclude, group, tags, tag_mode, between}, r, any));
    out_lims[0] = 0;
    *out_total = 0;
    if (nq == 0) {
        if (!count_only) ix->rd_total = 0;
        return TK_OK;
    }
    TRY(flush_pending(ix));
    TRY(ix->br_ynorm.ensure((size_t)ix->N * 4));
    TRY(ix->br_q.ensure((size_t)nq * ix->d * 4));
    TRY(ix->rd_radius.ensure((size_t)nq * 4));
    TRY(ix->rd_count.ensure((size_t)nq * 8 + 4));
    HIPCHECK(hipMemcpy(ix->br_q.p, q, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ix->rd_radius.p, radius, (size_t)nq * 4, hipMemcpyHostToDevice));
    const float *X = ix->br_q.as<float>(), *Y = ix->data.as<float>(), *rad = ix->rd_radius.as<float>();
    float *yn = ix->br_ynorm.as<float>();
    int *count = ix->rd_count.as<int>(), *slots = count + nq, *err = slots + nq;
    const TkBruteRestrict *rp = any ? &r : nullptr;
    if (tk_launch_radius_count(X, nq, ix->d, Y, ix->N, yn, rad, count, rp, nullptr))
        return fail(TK_ERR_HIP, "tk_launch_radius_count: unsupported size / LDS attribute");
    HIPCHECK(hipGetLastError());
    bool fill;
    TRY(radius_lims(ix, count, nq, count_only, max_results, out_lims, out_total, fill));
    if (!fill) {
        if (!count_only) ix->rd_total = 0;
        return TK_OK;
    }
    const int64_t total = *out_total;
    TRY(ix->rd_dist.ensure((size_t)total * 4));
    unsigned long long *keys = ix->rd_keys.as<unsigned long long>(), *alt = ix->rd_alt.as<unsigned long long>();
    if (tk_launch_radius_fill(X, nq, ix->d, Y, ix->N, yn, rad, count, ix->rd_off.as<int64_t>(), slots, keys, err, rp,
                              nullptr))
        return fail(TK_ERR_HIP, "tk_launch_radius_fill: unsupported size / LDS attribute");
    HIPCHECK(hipGetLastError());
    TRY(radius_passes_agree(err));
    if (sorted) {
        TRY(radius_sort(ix, keys, alt, total, nq));
        std::swap(keys, alt);           // the sorted keys; the ids go where the unsorted ones were
    }
    tk_launch_radius_decode(keys, total, (int64_t *)alt, ix->rd_dist.as<float>(), nullptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    ix->rd_ids_alt = alt == ix->rd_alt.as<unsigned long long>();
    ix->rd_total = total;
    return TK_OK;
}

// ---------------------------------------------------------------------------
// tk_index_radius_brute through a 128 x 128 tile kernel with a stage, d <= 4096: on the f16 matrix cores for a half
// store (radius_matrix.hip) or, wide, on the f32 ones for a float32 store (radius_wide.hip).
// ONE pass counts and stages the first `cap` keys of every query; the counts cross to the host (the lims); the query
// tiles that hold a longer list are walked once more, every other query's keys are copied out of the stage; then
// radius_brute's tail.  stage_cap: 0 = the largest power of two with nq * cap * 8 <= RM_STAGE_BUDGET, within
// [1, RM_STAGE_MOST].  The two entry points have made the refusals in front of d <= 4096; the two forms differ in the
// queries' preparation, the rows' norms and the two launchers.
#define RM_STAGE_BUDGET ((int64_t)128 << 20)
#define RM_STAGE_MOST (1 << 14)
static int radius_brute_staged(tk_index *ix, bool wide, const float *q, int64_t nq, const float *radius,
                               const TkHostRestrict &h, int sorted, int count_only, int64_t max_results,
                               int64_t *out_lims, int64_t *out_total, int stage_cap)
{
    ARGCHECK(ix->d <= 4096, "d <= 4096");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    for (int64_t i = 0; i < nq; i++) ARGCHECK(radius[i] == radius[i], "radius: NaN");
    ARGCHECK(count_only || (max_results >= 0 && max_results < (1ll << 31)), "0 <= max_results < 2^31");
    ARGCHECK(stage_cap >= 0 && stage_cap <= (1 << 20) && (int64_t)stage_cap * nq * 8 <= ((int64_t)4 << 30),
             "stage_cap: 0, or a capacity in [1, 2^20] with nq * stage_cap * 8 <= 4 GiB");
    TkBruteRestrict r;
    bool any;
    TRY(brute_restrict(ix, nq, h, r, any));
    out_lims[0] = 0;
    *out_total = 0;
    if (nq == 0) {
        if (!count_only) ix->rd_total = 0;
        return TK_OK;
    }
    int cap = stage_cap;
    if (cap == 0)
        for (cap = 1; cap < RM_STAGE_MOST && (int64_t)2 * cap * nq * 8 <= RM_STAGE_BUDGET;) cap *= 2;
    const int64_t n_qt = (nq + 127) / 128;
    TRY(flush_pending(ix));
    TRY(ix->br_ynorm.ensure((size_t)(ix->N > 0 ? ix->N : 1) * 4));
    TRY(ix->br_q.ensure((size_t)nq * ix->d * 4));
    TRY(ix->rd_radius.ensure((size_t)nq * 4));
    TRY(ix->rd_count.ensure((size_t)nq * 8 + 4));
    if (!count_only) TRY(ix->rd_stage.ensure((size_t)nq * cap * 8));
    HIPCHECK(hipMemcpy(ix->br_q.p, q, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ix->rd_radius.p, radius, (size_t)nq * 4, hipMemcpyHostToDevice));
    PmQueries pq{};
    if (wide) {
        TRY(ix->bw_x2.ensure((size_t)nq * tk_brute_wide_dq(ix->d) * 4));
        TRY(ix->bw_xn.ensure((size_t)nq * 4));
        tk_launch_brute_wide_prepare(ix->br_q.as<float>(), nq, ix->d, ix->bw_x2.as<float>(), ix->bw_xn.as<float>(), nullptr);
    } else {
        TRY(pm_prepare(ix, nq, pq));
    }
    const TkBruteMatrix mx{pq.xh, pq.xl, pq.xn, pq.xs, pq.dpad};
    const TkBruteWide wd{ix->bw_x2.as<float>(), ix->bw_xn.as<float>(), tk_brute_wide_dq(ix->d)};
    const float *rad = ix->rd_radius.as<float>();
    float *yn = ix->br_ynorm.as<float>();
    int *count = ix->rd_count.as<int>(), *slots = count + nq, *err = slots + nq;
    unsigned long long *stage = count_only ? nullptr : ix->rd_stage.as<unsigned long long>();
    const TkBruteRestrict *rp = any ? &r : nullptr;
    if (wide) {
        if (tk_launch_radius_wide_count(wd, nq, ix->d, ix->data.as<float>(), ix->N, yn, rad, count, stage, cap, rp, nullptr))
            return fail(TK_ERR_HIP, "tk_launch_radius_wide_count: unsupported size");
    } else {
        if (ix->N > 0) tk_launch_brute_half_norms(ix->data.p, ix->N, ix->d, yn, nullptr);
        if (tk_launch_radius_matrix_count(mx, nq, ix->d, ix->data.p, ix->N, yn, rad, count, stage, cap, rp, nullptr))
            return fail(TK_ERR_HIP, "tk_launch_radius_matrix_count: unsupported size");
    }
    HIPCHECK(hipGetLastError());
    bool fill;
    TRY(radius_lims(ix, count, nq, count_only, max_results, out_lims, out_total, fill));
    if (!fill) {
        if (!count_only) ix->rd_total = 0;
        return TK_OK;
    }
    const int64_t total = *out_total;
    // the query tiles that hold a list longer than the stage: their list, and a flag per tile
    std::vector<int> tiles((size_t)(2 * n_qt), 0);
    int n_tiles = 0;
    for (int64_t t = 0; t < n_qt; t++) {
        bool over = false;
        for (int64_t i = t * 128; i < nq && i < (t + 1) * 128 && !over; i++) over = out_lims[i + 1] - out_lims[i] > cap;
        if (over) {
            tiles[(size_t)n_tiles++] = (int)t;
            tiles[(size_t)(n_qt + t)] = 1;
        }
    }
    const int *dev_tiles;
    TRY(host_upload(ix->rd_tiles, tiles.data(), tiles.size(), dev_tiles));
    TRY(ix->rd_dist.ensure((size_t)total * 4));
    unsigned long long *keys = ix->rd_keys.as<unsigned long long>(), *alt = ix->rd_alt.as<unsigned long long>();
    if (wide) {
        if (tk_launch_radius_wide_fill(wd, nq, ix->d, ix->data.as<float>(), ix->N, yn, rad, count, stage, cap, dev_tiles,
                                       n_tiles, dev_tiles + n_qt, ix->rd_off.as<int64_t>(), slots, keys, err, rp, nullptr))
            return fail(TK_ERR_HIP, "tk_launch_radius_wide_fill: unsupported size");
    } else if (tk_launch_radius_matrix_fill(mx, nq, ix->d, ix->data.p, ix->N, yn, rad, count, stage, cap, dev_tiles,
                                            n_tiles, dev_tiles + n_qt, ix->rd_off.as<int64_t>(), slots, keys, err, rp,
                                            nullptr)) {
        return fail(TK_ERR_HIP, "tk_launch_radius_matrix_fill: unsupported size");
    }
    HIPCHECK(hipGetLastError());
    TRY(radius_passes_agree(err));
    if (sorted) {
        TRY(radius_sort(ix, keys, alt, total, nq));
        std::swap(keys, alt);           // the sorted keys; the ids go where the unsorted ones were
    }
    tk_launch_radius_decode(keys, total, (int64_t *)alt, ix->rd_dist.as<float>(), nullptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    ix->rd_ids_alt = alt == ix->rd_alt.as<unsigned long long>();
    ix->rd_total = total;
    return TK_OK;
}

extern "C" int tk_index_radius_brute_matrix(tk_index *ix, const float *q, int64_t nq, const float *radius,
                                            const uint8_t *allowed_mask, const int64_t *exclude, const int32_t *group,
                                            const uint64_t *tags, int tag_mode, const int64_t *between, int sorted,
                                            int count_only, int64_t max_results, int64_t *out_lims, int64_t *out_total,
                                            int stage_cap)
{
    IXLOCK(ix);
    if (ix) ix->rd_total = ix->rp_total = -1;       // whatever this call does, the result of the last one is gone
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: radius_search(matrix=True) is not supported");
    ARGCHECK(nq >= 0 && out_lims && out_total && (nq == 0 || (q && radius)), "buffers");
    TRY(pm_check(ix, q, nq));
    return radius_brute_staged(ix, false, q, nq, radius, {allowed_mask, exclude, group, tags, tag_mode, between}, sorted,
                               count_only, max_results, out_lims, out_total, stage_cap);
}

// ... for a float32 store of any d <= 4096: part, knn_brute(wide=True)'s value (radius_wide.hip)
extern "C" int tk_index_radius_brute_wide(tk_index *ix, const float *q, int64_t nq, const float *radius,
                                          const uint8_t *allowed_mask, const int64_t *exclude, const int32_t *group,
                                          const uint64_t *tags, int tag_mode, const int64_t *between, int sorted,
                                          int count_only, int64_t max_results, int64_t *out_lims, int64_t *out_total,
                                          int stage_cap)
{
    IXLOCK(ix);
    if (ix) ix->rd_total = ix->rp_total = -1;       // whatever this call does, the result of the last one is gone
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: radius_search(wide=True) is not supported");
    ARGCHECK(nq >= 0 && out_lims && out_total && (nq == 0 || (q && radius)), "buffers");
    ARGCHECK(ix->data_dtype != TK_DATA_F64, "wide=True needs store=\"float32\": this index stores float64 vectors");
    ARGCHECK(ix->data_dtype != TK_DATA_F16, "wide=True needs store=\"float32\": this index stores its vectors as half "
                                            "(store=\"float16\"); its search over all rows is matrix=True");
    return radius_brute_staged(ix, true, q, nq, radius, {allowed_mask, exclude, group, tags, tag_mode, between}, sorted,
                               count_only, max_results, out_lims, out_total, stage_cap);
}

extern "C" int tk_index_radius_fetch(tk_index *ix, int64_t *out_ids, float *out_dist)
{
    IXLOCK(ix);
    ARGCHECK(ix, "index");
    if (ix->rd_total < 0)
        return fail(TK_ERR_STATE, "tk_index_radius_fetch: no result is held (tk_index_radius_brute first; a call that "
                                  "failed or only counted holds none)");
    if (ix->rd_total == 0) return TK_OK;
    ARGCHECK(out_ids, "buffers");
    HIPCHECK(hipMemcpy(out_ids, ix->rd_ids_alt ? ix->rd_alt.p : ix->rd_keys.p, (size_t)ix->rd_total * 8,
                       hipMemcpyDeviceToHost));
    if (out_dist) HIPCHECK(hipMemcpy(out_dist, ix->rd_dist.p, (size_t)ix->rd_total * 4, hipMemcpyDeviceToHost));
    return TK_OK;
}
