// api_build.hip — device-side build of an index, raw-query preparation, exact brute force and the batch
// form of _FastDistanceTable.top over one flat array (FlatTop).  (Split from api.hip in round 4.)
#include "api_internal.h"

// ---------------------------------------------------------------------------
// device-resident build (devbuild.hip): IVF.build for vectors that live in HBM
static int upload_rotation(tk_index *ix, const double *R, int d_pad)
{
    std::vector<double> rt((size_t)d_pad * ix->dq);
    for (int j = 0; j < ix->dq; j++)
        for (int t = 0; t < d_pad; t++) rt[(size_t)t * ix->dq + j] = R[(size_t)j * d_pad + t];
    TRY(ix->rot_t.ensure(rt.size() * 8));
    HIPCHECK(hipMemcpy(ix->rot_t.p, rt.data(), rt.size() * 8, hipMemcpyHostToDevice));
    ix->rot_d_pad = d_pad;
    return TK_OK;
}

extern "C" float *tk_index_alloc_data(tk_index *ix, int64_t N, int d)
{
    IXLOCK(ix);
    if (!ix || !ix->have_pq || N < 1 || d < 1) {
        fail(TK_ERR_ARG, "bad argument: tk_index_alloc_data (set_pq first, N >= 1, d >= 1)");
        return nullptr;
    }
    if (ix->data.ensure((size_t)N * d * 4) != TK_OK) return nullptr;
    ix->N = N;
    ix->d = d;
    ix->data_dtype = TK_DATA_F32;
    ix->have_data = ix->have_centers = ix->have_lists = false;   // until tk_index_build_dev
    return ix->data.as<float>();
}

static int synth_centres(DevBuf &buf, const float *centres, int n_centres, int d, const float **dev)
{
    *dev = nullptr;
    if (!centres || n_centres <= 0) return TK_OK;
    TRY(buf.ensure((size_t)n_centres * d * 4));
    HIPCHECK(hipMemcpy(buf.p, centres, (size_t)n_centres * d * 4, hipMemcpyHostToDevice));
    *dev = buf.as<float>();
    return TK_OK;
}

extern "C" int tk_index_synth_data(tk_index *ix, int64_t row0, int64_t n, uint64_t seed,
                                   const float *centres, int n_centres, float sigma)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->data.p && ix->N > 0, "tk_index_alloc_data first");
    ARGCHECK(ix->data_dtype == TK_DATA_F32, "float32 vectors (before tk_index_narrow_data)");
    ARGCHECK(row0 >= 0 && n >= 0 && row0 + n <= ix->N, "row range");
    const float *cd = nullptr;
    TRY(synth_centres(ix->stage, centres, n_centres, ix->d, &cd));
    tk_launch_synth_rows(ix->data.as<float>() + row0 * ix->d, row0, n, ix->d, seed, cd, n_centres, sigma, 0);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    return TK_OK;
}

// the same generator into host memory (queries, training samples)
extern "C" int tk_synth_rows(float *out, int64_t row0, int64_t n, int d, uint64_t seed,
                             const float *centres, int n_centres, float sigma)
{
    TRY(require_gpu());
    ARGCHECK(out && n >= 0 && d >= 1 && row0 >= 0, "buffers / sizes");
    DevBuf cb, xb;
    const float *cd = nullptr;
    int rc = synth_centres(cb, centres, n_centres, d, &cd);
    const int64_t slab = 1 << 20;
    for (int64_t o = 0; o < n && rc == TK_OK; o += slab) {
        const int64_t m = n - o < slab ? n - o : slab;
        if ((rc = xb.ensure((size_t)m * d * 4)) != TK_OK) break;
        tk_launch_synth_rows(xb.as<float>(), row0 + o, m, d, seed, cd, n_centres, sigma, 0);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(out + (size_t)o * d, xb.p, (size_t)m * d * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(TK_ERR_HIP, hipGetErrorString(e));
    }
    cb.release();
    xb.release();
    return rc;
}

// labels (m, M) of `m` float32 rows (m, d) on the device: pad1 / rotation (float64 FMA chain,
// as the device front end) into `rows`, then the nearest centroid per block
static int encode_rows_dev(tk_index *ix, const float *x, int64_t m, DevBuf &rows, uint8_t *labels)
{
    const bool rot = ix->rot_d_pad > 0;
    TRY(rows.ensure((size_t)m * ix->dq * (rot ? 8 : 4)));
    tk_launch_prepare_queries(x, m, ix->d, rot ? ix->rot_t.as<double>() : nullptr, ix->dq,
                              rot ? ix->rot_d_pad : ix->dq, rows.p, 0);
    if (tk_launch_encode_pq(ix->pq_centers.as<float>(), ix->dq, ix->dpb, rows.p, rot ? 1 : 0, m, labels, 0))
        return fail(TK_ERR_HIP, "encode_pq_kernel: LDS budget / attribute");
    HIPCHECK(hipGetLastError());
    return TK_OK;
}

// what tk_launch_assign reads: the search centres transposed (d, C) and their einsum norms
static int upload_search_centres(DevBuf &yt, DevBuf &yn, const float *search_centers, const float *ynorm2,
                                 int64_t C, int d)
{
    std::vector<float> ytv((size_t)C * d);
    for (int64_t j = 0; j < C; j++)
        for (int t = 0; t < d; t++) ytv[(size_t)t * C + j] = search_centers[(size_t)j * d + t];
    TRY(yt.ensure(ytv.size() * 4));
    TRY(yn.ensure((size_t)C * 4));
    HIPCHECK(hipMemcpy(yt.p, ytv.data(), ytv.size() * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(yn.p, ynorm2, (size_t)C * 4, hipMemcpyHostToDevice));
    return TK_OK;
}

// the n_probes nearest centres of m float32 rows on the device (ivf.py:85), normalised in place first
// (ivf.py:78-79) where `normalise`; slabs of 2^20 rows, as the build has always cut them
static void assign_rows_dev(float *X, int64_t m, int d, int normalise, const DevBuf &yt, const DevBuf &yn,
                            int64_t C, int kp, int64_t *nearest)
{
    const int64_t slab = 1 << 20;
    for (int64_t o = 0; o < m; o += slab) {
        const int64_t s = m - o < slab ? m - o : slab;
        if (normalise) tk_launch_normalise_rows(X + o * d, s, d, X + o * d, 0);
        tk_launch_assign(X + o * d, s, d, yt.p, yn.p, 0, (int)C, kp, nearest + o * kp, 0);
    }
}

// stable sort of T (list, row) pairs by list (L lists): with kp lists per row, the column blocks of
// the pair arrays keep column 0 before column 1 ... inside every list (utils.py:131-150)
static int sort_pairs_dev(DevBuf &keys, DevBuf &rows, DevBuf &keys2, DevBuf &rows2, DevBuf &tmp, int64_t T,
                          int64_t L)
{
    int bits = 1;
    while ((1ll << bits) < L) bits++;
    TRY(keys2.ensure((size_t)T * 4));
    TRY(rows2.ensure((size_t)T * 4));
    size_t tmp_bytes = 0;
    if (tk_sort_pairs(nullptr, &tmp_bytes, keys.as<int>(), keys2.as<int>(), rows.as<int>(), rows2.as<int>(), T, bits, 0))
        return fail(TK_ERR_HIP, "radix sort: size query failed");
    TRY(tmp.ensure(tmp_bytes > 0 ? tmp_bytes : 16));
    if (tk_sort_pairs(tmp.p, &tmp_bytes, keys.as<int>(), keys2.as<int>(), rows.as<int>(), rows2.as<int>(), T, bits, 0))
        return fail(TK_ERR_HIP, "radix sort failed");
    return TK_OK;
}

// PQ codes of the L active centres (ivf.py:92-96), packed into `codes` as one tiled list of
// ceil(L / 16) chunks; the code of the zero vector (list padding, fast_pq.py:165) is left at
// clab + ceil16(L) * M
static int encode_centres(tk_index *ix, const float *act, int64_t L, DevBuf &rot, DevBuf &crow, DevBuf &clab,
                          DevBuf &offs, DevBuf &codes, const uint8_t **zero_code)
{
    const int d = ix->d, M = ix->M, P = M / 2;
    const int64_t L16 = (L + 15) / 16 * 16, cc = L16 / 16;
    TRY(crow.ensure((size_t)(L16 + 16) * d * 4));
    TRY(clab.ensure((size_t)(L16 + 16) * M));
    HIPCHECK(hipMemset(crow.p, 0, (size_t)(L16 + 16) * d * 4));
    if (L > 0) HIPCHECK(hipMemcpy(crow.p, act, (size_t)L * d * 4, hipMemcpyHostToDevice));
    TRY(encode_rows_dev(ix, crow.as<float>(), L16 + 16, rot, clab.as<uint8_t>()));
    *zero_code = clab.as<uint8_t>() + (size_t)L16 * M;
    const size_t bytes = (size_t)tk_tiled_uint4s(cc, P) * 16;
    TRY(codes.ensure(bytes > 0 ? bytes : 16));
    HIPCHECK(hipMemset(codes.p, 0, bytes > 0 ? bytes : 16));
    const int64_t o[5] = {0, cc, 0, L, L};      // chunk offsets, id offsets, size of the one list
    TRY(offs.ensure(sizeof o));
    HIPCHECK(hipMemcpy(offs.p, o, sizeof o, hipMemcpyHostToDevice));
    tk_launch_pack_lists(clab.as<uint8_t>(), M, nullptr, offs.as<int64_t>() + 2, offs.as<int64_t>(),
                         offs.as<int64_t>() + 4, 1, *zero_code, codes.as<uint4>(), cc, 0);
    HIPCHECK(hipGetLastError());
    return TK_OK;
}

// the coarse stage's descriptors of L coded centres in center_chunks chunks
static int set_centre_slots(tk_index *ix, int64_t L, int64_t center_chunks)
{
    const int64_t cco[2] = {0, center_chunks};
    const int ci[3] = {0, (int)center_chunks, (int)L};
    const int64_t cl1[1] = {-1};
    TRY(ix->c_chunk_off.ensure(sizeof cco));
    TRY(ix->cslots_i.ensure(sizeof ci));
    TRY(ix->cslots_l.ensure(sizeof cl1));
    HIPCHECK(hipMemcpy(ix->c_chunk_off.p, cco, sizeof cco, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ix->cslots_i.p, ci, sizeof ci, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ix->cslots_l.p, cl1, sizeof cl1, hipMemcpyHostToDevice));
    ix->n_lists = L;
    ix->center_chunks = center_chunks;
    return TK_OK;
}

struct BufCleanup {
    std::vector<DevBuf *> v;
    ~BufCleanup() { for (DevBuf *b : v) b->release(); }
};

extern "C" int tk_index_build_dev(tk_index *ix, int normalise, const float *all_centers,
                                  const float *search_centers, const float *ynorm2, int64_t C,
                                  int n_probes, const double *R, int d_pad, int64_t *n_active_out)
{
    IXLOCK(ix);
    if (!search_centers) search_centers = all_centers;
    ARGCHECK(n_probes >= 1 && n_probes <= 9 && n_probes <= C, "n_probes must be 1 .. 9");
    const int kp = n_probes;
    ARGCHECK(ix && ix->have_pq && ix->data.p && ix->N > 0, "set_pq and tk_index_alloc_data first");
    ARGCHECK(ix->data_dtype == TK_DATA_F32, "the build reads float32 vectors (tk_index_narrow_data comes after it)");
    ARGCHECK(all_centers && ynorm2 && C >= 1 && C < (1ll << 31), "centres");
    ARGCHECK(ix->N * kp < (1ll << 31), "N * n_probes < 2^31");
    ARGCHECK(ix->d <= 384 && (!normalise || ix->d <= 128), "d <= 384 (128 with normalisation)");
    ARGCHECK(16 % ix->dpb == 0, "dims_per_block must divide 16 for the device encoder");
    ARGCHECK(R ? (d_pad >= ix->d && d_pad <= 16384) : ix->dq >= ix->d, "rotation / padding");
    TRY(flush_pending(ix));
    const int64_t N = ix->N;
    const int d = ix->d, M = ix->M;
    float *X = ix->data.as<float>();
    if (R) TRY(upload_rotation(ix, R, d_pad));
    else { ix->rot_t.release(); ix->rot_d_pad = 0; }
    const int64_t slab = 1 << 20;
    DevBuf yt, yn, near, keys, rows, keys2, rows2, count, remap, labels, rot, tmp, crow, clab;
    BufCleanup cl{{&yt, &yn, &near, &keys, &rows, &keys2, &rows2, &count, &remap, &labels, &rot, &tmp, &crow, &clab}};
    // ---- 1. data = X / |X| (ivf.py:78-79), nearest centre per row (ivf.py:85)
    TRY(upload_search_centres(yt, yn, search_centers, ynorm2, C, d));
    const int64_t T = N * kp;           // (list, row) pairs: every row sits in kp lists
    TRY(near.ensure((size_t)slab * kp * 8));
    TRY(keys.ensure((size_t)T * 4));
    TRY(rows.ensure((size_t)T * 4));
    TRY(count.ensure((size_t)C * kp * 4));
    HIPCHECK(hipMemset(count.p, 0, (size_t)C * kp * 4));
    for (int64_t o = 0; o < N; o += slab) {
        const int64_t m = N - o < slab ? N - o : slab;
        assign_rows_dev(X + o * d, m, d, normalise, yt, yn, C, kp, near.as<int64_t>());
        tk_launch_keys_count(near.as<int64_t>(), m, kp, o, N, keys.as<int>(), rows.as<int>(), count.as<int>(), 0);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipDeviceSynchronize());
    // ---- 2. active centres (ivf.py:91: all_centers[np.unique(nearest)]) and the CSR offsets
    std::vector<int> cntc((size_t)C * kp), rm((size_t)C, -1);
    HIPCHECK(hipMemcpy(cntc.data(), count.p, (size_t)C * kp * 4, hipMemcpyDeviceToHost));
    std::vector<float> act;
    std::vector<int64_t> sizes, cols;
    for (int64_t j = 0; j < C; j++) {
        int64_t c = 0;
        for (int t = 0; t < kp; t++) c += cntc[(size_t)j * kp + t];
        if (c > 0) {
            rm[(size_t)j] = (int)sizes.size();
            sizes.push_back(c);
            cols.insert(cols.end(), cntc.begin() + j * kp, cntc.begin() + (j + 1) * kp);
            act.insert(act.end(), all_centers + (size_t)j * d, all_centers + (size_t)(j + 1) * d);
        }
    }
    const int64_t L = (int64_t)sizes.size();
    {   // the reference groups the rows by RAW centre id into n_active lists and asserts
        // max(index) < n_active (utils.py:128, IVF.build -> group_data_by_indices): it only builds
        // when no empty centre precedes a used one.  Same contract here (the host build asserts too).
        int64_t last = -1;
        for (int64_t j = 0; j < C; j++)
            if (rm[(size_t)j] >= 0) last = j;
        ARGCHECK(last < L, "a centre that received no row precedes one that did: the reference's "
                           "group_data_by_indices asserts max(index) < n_active (utils.py:128)");
    }
    ListLayout lay;
    TRY(lay.set_sizes(sizes.data(), L));
    TRY(remap.ensure((size_t)C * 4));
    HIPCHECK(hipMemcpy(remap.p, rm.data(), (size_t)C * 4, hipMemcpyHostToDevice));
    tk_launch_remap_keys(keys.as<int>(), T, remap.as<int>(), 0);
    // ---- 3. rows grouped by list: stable sort of (list, row); with two lists per row the
    //         column-0 pairs precede the column-1 pairs of every list (utils.py:131-150)
    TRY(sort_pairs_dev(keys, rows, keys2, rows2, tmp, T, L));
    HIPCHECK(hipDeviceSynchronize());
    keys.release(); rows.release(); keys2.release(); tmp.release(); near.release();
    // ---- 4. PQ codes of every row (a row's code does not depend on its list)
    TRY(labels.ensure((size_t)N * M));
    for (int64_t o = 0; o < N; o += slab) {
        const int64_t m = N - o < slab ? N - o : slab;
        TRY(encode_rows_dev(ix, X + o * d, m, rot, labels.as<uint8_t>() + (size_t)o * M));
    }
    // ---- 5. the index: centres, their codes and the zero vector's code (list padding)
    const uint8_t *zero_code = nullptr;
    TRY(encode_centres(ix, act.data(), L, rot, crow, clab, ix->stage, ix->center_codes, &zero_code));
    TRY(ix->active_centers.ensure((size_t)L * d * 4));
    HIPCHECK(hipMemcpy(ix->active_centers.p, act.data(), (size_t)L * d * 4, hipMemcpyHostToDevice));
    TRY(set_centre_slots(ix, L, (L + 15) / 16));
    const int P = M / 2;
    // ---- 6. the index: lists
    TRY(lay.ids.ensure((size_t)T * 8));
    const size_t tiled_bytes = (size_t)tk_tiled_uint4s(lay.total_chunks, P) * 16;
    TRY(lay.codes.ensure(tiled_bytes));
    HIPCHECK(hipMemset(lay.codes.p, 0, tiled_bytes));
    tk_launch_pack_lists(labels.as<uint8_t>(), M, rows2.as<int>(), lay.ids_off.as<int64_t>(),
                         lay.list_chunk_off.as<int64_t>(), lay.list_n.as<int64_t>(), (int)L, zero_code,
                         lay.codes.as<uint4>(), lay.total_chunks, 0);
    tk_launch_widen_ids(rows2.as<int>(), T, lay.ids.as<int64_t>(), 0);
    HIPCHECK(hipGetLastError());
    if (kp > 1) {                   // the lane replay's duplicate test reads the labels as int32
        TRY(lay.ids32.ensure((size_t)T * 4));
        HIPCHECK(hipMemcpyAsync(lay.ids32.p, rows2.p, (size_t)T * 4, hipMemcpyDeviceToDevice, 0));
        lay.have_ids32 = true;
    }
    HIPCHECK(hipDeviceSynchronize());
    lay.ids_unique = kp == 1;       // one list per row: no label can repeat
    lay.max_label = N - 1;          // (labels are row numbers)
    lay.list_cols = cols;
    lay.kp = kp;
    ix->have_centers = ix->have_data = true;
    TRY(install_lists(ix, lay));
    if (n_active_out) *n_active_out = L;
    return TK_OK;
}

// float32 vectors in HBM -> halfs (tinyknn_hip.h): checked first, converted into a new buffer, swapped last
extern "C" int tk_index_narrow_data(tk_index *ix)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data && ix->data.p, "an index with its vectors");
    if (ix->data_dtype == TK_DATA_F16) return TK_OK;
    ARGCHECK(ix->data_dtype == TK_DATA_F32, "float64 vectors are rescored in float64: no half storage");
    ARGCHECK(!ix->data.borrowed, "a cloned shard borrows its vectors");
    ARGCHECK(!ix->data_lent, "shards cloned from this index borrow its vectors");
    TRY(flush_pending(ix));
    HIPCHECK(hipDeviceSynchronize());
    DevBuf flag, half;
    BufCleanup cl{{&flag, &half}};
    TRY(check_half_rows(ix->data.as<float>(), ix->N, ix->d, 0, flag));
    TRY(half.ensure((size_t)ix->N * ix->d * 2));
    tk_launch_narrow_rows(ix->data.as<float>(), ix->N, ix->d, half.p, 0);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    std::swap(ix->data, half);          // (the float32 buffer leaves with the cleanup)
    ix->data_dtype = TK_DATA_F16;
    return TK_OK;
}

extern "C" int tk_index_list_columns(tk_index *ix, int *kp, int64_t *counts)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_lists && kp, "an index with its lists");
    *kp = ix->list_kp;
    if (counts && ix->list_kp > 0)
        memcpy(counts, ix->list_cols.data(), ix->list_cols.size() * sizeof(int64_t));
    return TK_OK;
}

// What the stored labels say (all must lie in [0, N)): cnt = copies per row; out = {largest row stored, most copies
// of a row, fewest copies of a stored row, labels outside [0, N)}.  Synchronises the device.
static int row_copies(tk_index *ix, const int64_t *ids, int64_t T, DevBuf &cnt, DevBuf &out_d, int out[4])
{
    const int init[4] = {-1, 0, 0x7fffffff, 0};
    TRY(cnt.ensure((size_t)ix->N * 4));
    TRY(out_d.ensure(sizeof init));
    HIPCHECK(hipMemset(cnt.p, 0, (size_t)ix->N * 4));
    HIPCHECK(hipMemcpy(out_d.p, init, sizeof init, hipMemcpyHostToDevice));
    tk_launch_row_copies(ids, T, cnt.as<int>(), ix->N, out_d.as<int>(), 0);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(out, out_d.p, sizeof init, hipMemcpyDeviceToHost));
    return TK_OK;
}

// Every stored row sits in exactly kp lists.  Without removals that is total_ids == N * kp; after
// tk_index_remove_rows (or a host upload of lists saved after one) fewer entries remain, and every row still
// stored has its kp copies.
static int rows_sit_in(tk_index *ix, int kp, bool *ok)
{
    *ok = ix->total_ids == ix->N * kp;
    if (*ok || ix->total_ids > ix->N * kp || ix->total_ids % kp != 0) return TK_OK;
    DevBuf cnt, out_d;
    BufCleanup cl{{&cnt, &out_d}};
    int out[4];
    TRY(row_copies(ix, ix->ids.as<int64_t>(), ix->total_ids, cnt, out_d, out));
    *ok = out[3] == 0 && (ix->total_ids == 0 || (out[1] == kp && out[2] == kp));
    return TK_OK;
}

// list_columns against the list sizes: cw counts per list, none negative, adding up to the list
static int check_columns(const std::vector<int64_t> &cols0, const std::vector<int64_t> &size0, int64_t L, int cw)
{
    for (int64_t l = 0; l < L; l++) {
        int64_t s = 0;
        for (int t = 0; t < cw; t++) {
            ARGCHECK(cols0[(size_t)(l * cw + t)] >= 0, "list_columns: negative count");
            s += cols0[(size_t)(l * cw + t)];
        }
        ARGCHECK(s == size0[(size_t)l], "list_columns: a list's columns do not add up to its size");
    }
    return TK_OK;
}

// ---- what add and update do with their new rows, in the order they do it
// The nearest centres of the n rows Xn (device; given, or found as tk_index_build_dev finds them; the rows are
// normalised in place first where asked), their (centre, row) pairs in keys / prow and the members per
// (centre, column) in cntc
static int new_row_pairs(void *Xn, int64_t n, int d, int kp, const int64_t *nearest, int normalise,
                         const float *search_centers, const float *ynorm2, int64_t C, DevBuf &yt, DevBuf &yn,
                         DevBuf &near, DevBuf &keys, DevBuf &prow, DevBuf &count, std::vector<int> &cntc)
{
    const int64_t T = n * kp;
    TRY(near.ensure((size_t)T * 8));
    if (nearest) {
        HIPCHECK(hipMemcpy(near.p, nearest, (size_t)T * 8, hipMemcpyHostToDevice));
        if (normalise) tk_launch_normalise_rows((float *)Xn, n, d, (float *)Xn, 0);
    } else {
        TRY(upload_search_centres(yt, yn, search_centers, ynorm2, C, d));
        assign_rows_dev((float *)Xn, n, d, normalise, yt, yn, C, kp, near.as<int64_t>());
    }
    TRY(keys.ensure((size_t)T * 4));
    TRY(prow.ensure((size_t)T * 4));
    TRY(count.ensure((size_t)C * kp * 4));
    HIPCHECK(hipMemset(count.p, 0, (size_t)C * kp * 4));
    tk_launch_keys_count(near.as<int64_t>(), n, kp, 0, n, keys.as<int>(), prow.as<int>(), count.as<int>(), 0);
    HIPCHECK(hipGetLastError());
    cntc.resize((size_t)C * kp);
    HIPCHECK(hipMemcpy(cntc.data(), count.p, (size_t)C * kp * 4, hipMemcpyDeviceToHost));
    return TK_OK;
}

// The active centres stay a prefix 0 .. L1 - 1 (the build's contract, utils.py:128): L1 lists once the centres that
// received a row join the L0 old ones, or -1 where an unused centre would precede a used one
#define PREFIX_REFUSAL "a centre that received no row precedes one that did: the reference's " \
                       "group_data_by_indices asserts max(index) < n_active (utils.py:128)"
static int64_t active_prefix(const std::vector<int> &cntc, int64_t C, int kp, int64_t L0)
{
    int64_t L1 = 0, last = -1;
    for (int64_t j = 0; j < C; j++) {
        int64_t c = 0;
        for (int t = 0; t < kp; t++) c += cntc[(size_t)(j * kp + t)];
        if (j < L0 || c > 0) {
            L1++;
            last = j;
        }
    }
    return last < L1 ? L1 : -1;
}

// PQ labels (n, M) of the new rows in lab: given, or as the build encodes them
static int new_row_labels(tk_index *ix, const void *Xn, int64_t n, const uint8_t *labels, DevBuf &rot, DevBuf &lab)
{
    const int M = ix->M, d = ix->d;
    TRY(lab.ensure((size_t)n * M));
    if (labels) {
        HIPCHECK(hipMemcpy(lab.p, labels, (size_t)n * M, hipMemcpyHostToDevice));
        return TK_OK;
    }
    const int64_t slab = 1 << 20;
    for (int64_t o = 0; o < n; o += slab)
        TRY(encode_rows_dev(ix, (const float *)Xn + o * d, n - o < slab ? n - o : slab, rot,
                            lab.as<uint8_t>() + (size_t)o * M));
    return TK_OK;
}

// the zero vector's labels (the rows that pad a list) in zlab
static int zero_labels_dev(tk_index *ix, DevBuf &rot, DevBuf &zrow, DevBuf &zlab)
{
    TRY(zrow.ensure((size_t)16 * ix->d * 4));
    TRY(zlab.ensure((size_t)16 * ix->M));
    HIPCHECK(hipMemset(zrow.p, 0, (size_t)16 * ix->d * 4));
    return encode_rows_dev(ix, zrow.as<float>(), 16, rot, zlab.as<uint8_t>());
}

// L1 > L0 lists: the centres all_centers[:L1] in act1 and their codes in ccodes — the host's
// (pq.transform(active_centers)) retiled, or coded on the device
static int grown_centres(tk_index *ix, const float *all_centers, const uint64_t *center_codes, int64_t L1, DevBuf &rot,
                         DevBuf &crow, DevBuf &clab, DevBuf &coffs, DevBuf &act1, DevBuf &ccodes)
{
    const int d = ix->d, M = ix->M, P = M / 2;
    TRY(act1.ensure((size_t)L1 * d * 4));
    HIPCHECK(hipMemcpy(act1.p, all_centers, (size_t)L1 * d * 4, hipMemcpyHostToDevice));
    if (center_codes) {
        const int64_t cc = (L1 + 15) / 16;
        TRY(coffs.ensure((size_t)cc * M * 8));
        TRY(ccodes.ensure((size_t)tk_tiled_uint4s(cc, P) * 16));
        HIPCHECK(hipMemcpy(coffs.p, center_codes, (size_t)cc * M * 8, hipMemcpyHostToDevice));
        tk_launch_retile(coffs.as<uint4>(), ccodes.as<uint4>(), cc, P, 0);
        HIPCHECK(hipGetLastError());
        return TK_OK;
    }
    const uint8_t *zc = nullptr;
    return encode_centres(ix, all_centers, L1, rot, crow, clab, coffs, ccodes, &zc);
}

// The first half of a removal, which update shares: the n rows (device ids, checked in [0, N) by the caller) become
// a byte map, every stored entry is flagged keep / drop, the exclusive scan of the flags numbers the kept ones
// (keep, scan: T0 + 1 entries).  g = the scan at the (list, column) boundaries (cw per list, then the end): the kept
// entries in front of each.  ioff0 / cols0: the old id offsets and members per (list, boundary).
static int kept_entries(tk_index *ix, const int64_t *rows_d, int64_t n, const std::vector<int64_t> &ioff0,
                        const std::vector<int64_t> &cols0, int cw, DevBuf &dead, DevBuf &keep, DevBuf &scan,
                        DevBuf &tmp, DevBuf &bad, DevBuf &pos_d, DevBuf &gat, std::vector<int64_t> &g)
{
    const int64_t L = ix->n_lists, T0 = ix->total_ids, N = ix->N;
    TRY(dead.ensure((size_t)N));
    HIPCHECK(hipMemset(dead.p, 0, (size_t)N));
    TRY(bad.ensure(4));
    HIPCHECK(hipMemset(bad.p, 0, 4));
    TRY(keep.ensure((size_t)(T0 + 1) * 8));
    TRY(scan.ensure((size_t)(T0 + 1) * 8));
    tk_launch_mark_rows(rows_d, n, dead.as<uint8_t>(), 0);
    tk_launch_keep_flags(ix->ids.as<int64_t>(), T0, dead.as<uint8_t>(), N, keep.as<long long>(), bad.as<int>(), 0);
    HIPCHECK(hipGetLastError());
    size_t tmp_bytes = 0;
    if (tk_scan_exclusive64(nullptr, &tmp_bytes, nullptr, nullptr, T0 + 1, 0))
        return fail(TK_ERR_HIP, "scan: size query failed");
    TRY(tmp.ensure(tmp_bytes));
    if (tk_scan_exclusive64(tmp.p, &tmp_bytes, keep.as<long long>(), scan.as<long long>(), T0 + 1, 0))
        return fail(TK_ERR_HIP, "scan failed");
    // the scan at the (list, column) boundaries
    std::vector<int64_t> bpos((size_t)(L * cw + 1));
    g.resize(bpos.size());
    for (int64_t l = 0; l < L; l++) {
        int64_t o = ioff0[(size_t)l];
        for (int t = 0; t < cw; t++) {
            bpos[(size_t)(l * cw + t)] = o;
            o += cols0[(size_t)(l * cw + t)];
        }
    }
    bpos.back() = T0;
    TRY(pos_d.ensure(bpos.size() * 8));
    TRY(gat.ensure(bpos.size() * 8));
    HIPCHECK(hipMemcpy(pos_d.p, bpos.data(), bpos.size() * 8, hipMemcpyHostToDevice));
    tk_launch_gather_scan(scan.as<long long>(), pos_d.as<int64_t>(), (int64_t)bpos.size(), gat.as<int64_t>(), 0);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(g.data(), gat.p, g.size() * 8, hipMemcpyDeviceToHost));
    int bad_h = 0;
    HIPCHECK(hipMemcpy(&bad_h, bad.p, 4, hipMemcpyDeviceToHost));
    ARGCHECK(!bad_h, "the index holds labels outside [0, N): its rows cannot be named");
    return TK_OK;
}

// New rows merged into the built lists (tinyknn_hip.h).  Everything is validated and built in new buffers
// first; the index changes only at the end, where nothing can fail any more.
extern "C" int tk_index_add_rows(tk_index *ix, const void *rows, int rows_is_f64, int64_t n, int kp,
                                 const int64_t *nearest, const uint8_t *labels, const int64_t *list_columns,
                                 int normalise, const float *all_centers, const float *search_centers,
                                 const float *ynorm2, int64_t C, const uint64_t *center_codes,
                                 int64_t *n_active_out)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_pq && ix->have_centers && ix->have_lists && ix->have_data, "a complete index");
    ARGCHECK(!ix->sharded, "a list-sharded index takes no rows");
    ARGCHECK(n >= 0 && (n == 0 || rows), "rows");
    ARGCHECK(kp >= 1 && kp <= 9, "kp (lists per row) must be 1 .. 9");
    ARGCHECK(!rows_is_f64 == (ix->data_dtype != TK_DATA_F64),
             "float64 rows only for an index of float64 vectors (float32 rows for float32 and half vectors)");
    const bool half = ix->data_dtype == TK_DATA_F16;
    {
        bool sit = false;
        TRY(rows_sit_in(ix, kp, &sit));
        ARGCHECK(sit, "kp: every stored row sits in kp lists");
    }
    ARGCHECK(list_columns || ix->list_kp == kp,
             "list_columns: the index does not know its members per (list, column) (a host upload)");
    ARGCHECK(C >= ix->n_lists && C >= kp && C < (1ll << 31), "C: the number of centres");
    ARGCHECK((ix->N + n) * kp < (1ll << 31), "(N + n) * kp < 2^31");
    const int d = ix->d, M = ix->M, P = M / 2;
    if (!search_centers) search_centers = all_centers;
    ARGCHECK(nearest || (all_centers && ynorm2 && !rows_is_f64 && d <= 384 && (!normalise || d <= 128)),
             "device assignment: all_centers + ynorm2, float32 rows, d <= 384 (128 with normalisation)");
    ARGCHECK(!normalise || !rows_is_f64, "normalisation on the device: float32 rows");
    ARGCHECK(labels || !rows_is_f64, "device encoding: float32 rows (else pass labels)");
    ARGCHECK(16 % ix->dpb == 0, "dims_per_block must divide 16 for the device encoder");
    if (nearest)
        for (int64_t i = 0; i < n * kp; i++) ARGCHECK(nearest[i] >= 0 && nearest[i] < C, "nearest: a centre id");
    if (n_active_out) *n_active_out = ix->n_lists;
    if (n == 0) return TK_OK;
    TRY(settle_lists(ix));
    const int64_t L0 = ix->n_lists, N0 = ix->N, N1 = N0 + n;
    // ---- the old layout: list sizes and members per column
    std::vector<int64_t> size0((size_t)L0);
    HIPCHECK(hipMemcpy(size0.data(), ix->list_n.p, (size_t)L0 * 8, hipMemcpyDeviceToHost));
    std::vector<int64_t> cols0(list_columns ? list_columns : ix->list_cols.data(),
                               (list_columns ? list_columns : ix->list_cols.data()) + L0 * kp);
    TRY(check_columns(cols0, size0, L0, kp));
    const size_t esz = data_esz(ix->data_dtype);      // of a stored element; the rows come as float32 / float64
    DevBuf xstage, hflag, grown, yt, yn, near, keys, prow, keys2, rows2, count, lab, rot, tmp, zrow, zlab, crow, clab, coffs,
        act1, ccodes, noff_d, seg_d;
    BufCleanup cl{{&xstage, &hflag, &grown, &yt, &yn, &near, &keys, &prow, &keys2, &rows2, &count, &lab, &rot, &tmp, &zrow, &zlab,
                   &crow, &clab, &coffs, &act1, &ccodes, &noff_d, &seg_d}};
    ListLayout lay;
    // ---- 1. the rows behind the old ones (a larger buffer where they do not fit: the old one stays intact)
    void *base = ix->data.p;
    if ((size_t)N1 * d * esz > ix->data.cap) {
        TRY(grown.ensure((size_t)N1 * d * esz));
        HIPCHECK(hipMemcpy(grown.p, ix->data.p, (size_t)N0 * d * esz, hipMemcpyDeviceToDevice));
        base = grown.p;
    }
    // (half vectors: the rows are prepared as float32 in a buffer of their own and narrowed into the tail last)
    void *tail = (char *)base + (size_t)N0 * d * esz;
    void *Xn = tail;
    if (half) {
        TRY(xstage.ensure((size_t)n * d * 4));
        Xn = xstage.p;
    }
    HIPCHECK(hipMemcpy(Xn, rows, (size_t)n * d * (rows_is_f64 ? 8 : 4), hipMemcpyDefault));
    // ---- 2. nearest centres (given, or as tk_index_build_dev finds them), pairs per (centre, column)
    const int64_t T = n * kp;
    std::vector<int> cntc;
    TRY(new_row_pairs(Xn, n, d, kp, nearest, normalise, search_centers, ynorm2, C, yt, yn, near, keys, prow, count, cntc));
    // ---- 3. the active centres stay a prefix 0 .. L1 - 1 (the build's contract, utils.py:128)
    const int64_t L1 = active_prefix(cntc, C, kp, L0);
    ARGCHECK(L1 >= 0, PREFIX_REFUSAL);
    ARGCHECK(L1 == L0 || all_centers, "new lists: all_centers");
    // ---- 4. the new layout: list l's column block j = old_j ++ new_j
    std::vector<int64_t> size1((size_t)L1), noff((size_t)L1 + 1, 0), seg((size_t)L1 * kp * 2), cols1((size_t)L1 * kp);
    for (int64_t l = 0; l < L1; l++) {
        int64_t s = 0, sn = 0;
        for (int t = 0; t < kp; t++) {
            const int64_t o = l < L0 ? cols0[(size_t)(l * kp + t)] : 0, nn = cntc[(size_t)(l * kp + t)];
            seg[(size_t)(l * kp + t) * 2] = o;
            seg[(size_t)(l * kp + t) * 2 + 1] = nn;
            cols1[(size_t)(l * kp + t)] = o + nn;
            s += o + nn;
            sn += nn;
        }
        size1[(size_t)l] = s;
        noff[(size_t)l + 1] = noff[(size_t)l] + sn;
    }
    TRY(lay.set_sizes(size1.data(), L1));
    const int64_t chunks1 = lay.total_chunks, T1 = lay.total_ids;
    // ---- 5. new pairs grouped by list (centre ids are list ids: the active set is a prefix)
    TRY(sort_pairs_dev(keys, prow, keys2, rows2, tmp, T, L1));
    // ---- 6. codes of the new rows (given, or as the build encodes them), of the zero vector, of new centres
    TRY(new_row_labels(ix, Xn, n, labels, rot, lab));
    TRY(zero_labels_dev(ix, rot, zrow, zlab));
    if (L1 > L0) TRY(grown_centres(ix, all_centers, center_codes, L1, rot, crow, clab, coffs, act1, ccodes));
    if (half) {         // what the vectors will hold: every half finite, or nothing changes
        TRY(check_half_rows((const float *)Xn, n, d, N0, hflag));
        tk_launch_narrow_rows((const float *)Xn, n, d, tail, 0);
        HIPCHECK(hipGetLastError());
    }
    // ---- 7. the merged lists
    TRY(noff_d.ensure((size_t)(L1 + 1) * 8));
    TRY(seg_d.ensure(seg.size() * 8));
    HIPCHECK(hipMemcpy(noff_d.p, noff.data(), noff.size() * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(seg_d.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice));
    const size_t tiled_bytes = (size_t)tk_tiled_uint4s(chunks1, P) * 16;
    TRY(lay.codes.ensure(tiled_bytes));
    HIPCHECK(hipMemset(lay.codes.p, 0, tiled_bytes));
    TRY(lay.ids.ensure((size_t)T1 * 8));
    lay.have_ids32 = kp > 1;
    if (lay.have_ids32) TRY(lay.ids32.ensure((size_t)T1 * 4));
    tk_launch_merge_lists(ix->codes.as<uint4>(), ix->list_chunk_off.as<int64_t>(), ix->ids_off.as<int64_t>(),
                          ix->ids.as<int64_t>(), lab.as<uint8_t>(), M, rows2.as<int>(), noff_d.as<int64_t>(),
                          seg_d.as<int64_t>(), kp, lay.list_chunk_off.as<int64_t>(), lay.ids_off.as<int64_t>(),
                          lay.list_n.as<int64_t>(), (int)L1, zlab.as<uint8_t>(), N0, lay.codes.as<uint4>(),
                          lay.ids.as<int64_t>(), lay.have_ids32 ? lay.ids32.as<int32_t>() : nullptr, chunks1, 0);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    lay.ids_unique = kp == 1;
    lay.max_label = N1 - 1;
    lay.list_cols = cols1;
    lay.kp = kp;
    // ---- 8. the swap: the old buffers go with the cleanup and the layout
    if (grown.p) std::swap(ix->data, grown);
    if (L1 > L0) {
        std::swap(ix->active_centers, act1);
        std::swap(ix->center_codes, ccodes);
        TRY(set_centre_slots(ix, L1, (L1 + 15) / 16));     // (buffers of a few bytes that already exist)
    }
    ix->N = N1;
    TRY(install_lists(ix, lay));
    if (n_active_out) *n_active_out = L1;
    return TK_OK;
}

// Rows deleted from the built lists (tinyknn_hip.h).  Checks first, the new lists in new buffers, the swap last.
extern "C" int tk_index_remove_rows(tk_index *ix, const int64_t *rows, int64_t n, int kp,
                                    const int64_t *list_columns, int64_t *removed_out)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_pq && ix->have_centers && ix->have_lists && ix->have_data, "a complete index");
    ARGCHECK(!ix->sharded, "a list-sharded index removes no rows");
    ARGCHECK(n >= 0 && (n == 0 || rows), "rows");
    ARGCHECK(kp >= 1 && kp <= 9, "kp (lists per row) must be 1 .. 9");
    ARGCHECK(list_columns || ix->list_kp == 0 || ix->list_kp == kp,
             "kp: the index knows its members per (list, column) for another number of columns");
    ARGCHECK(ix->N < (1ll << 31) && ix->total_ids < (1ll << 31), "N and the stored entries < 2^31");
    ARGCHECK(16 % ix->dpb == 0, "dims_per_block must divide 16 for the device encoder");
    if (removed_out) *removed_out = 0;
    std::vector<int64_t> rv((size_t)n);
    if (n > 0) HIPCHECK(hipMemcpy(rv.data(), rows, (size_t)n * 8, hipMemcpyDefault));
    for (int64_t i = 0; i < n; i++) ARGCHECK(rv[(size_t)i] >= 0 && rv[(size_t)i] < ix->N, "rows: an id outside [0, N)");
    const int64_t L = ix->n_lists, T0 = ix->total_ids;
    // ---- the old layout: list sizes, offsets, members per column (where known)
    std::vector<int64_t> size0((size_t)L), ioff0((size_t)L + 1);
    HIPCHECK(hipMemcpy(size0.data(), ix->list_n.p, (size_t)L * 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(ioff0.data(), ix->ids_off.p, (size_t)(L + 1) * 8, hipMemcpyDeviceToHost));
    const int64_t *cols_src = list_columns ? list_columns : (ix->list_kp == kp ? ix->list_cols.data() : nullptr);
    const int cw = cols_src ? kp : 1;     // boundaries per list: its column blocks, or the list alone
    std::vector<int64_t> cols0(cols_src ? cols_src : size0.data(), (cols_src ? cols_src : size0.data()) + L * cw);
    TRY(check_columns(cols0, size0, L, cw));
    if (n == 0) return TK_OK;
    TRY(settle_lists(ix));
    DevBuf rows_d, dead, keep, scan, tmp, bad, pos_d, gat, src, rot, zrow, zlab, cnt, summ;
    BufCleanup cl{{&rows_d, &dead, &keep, &scan, &tmp, &bad, &pos_d, &gat, &src, &rot, &zrow, &zlab, &cnt, &summ}};
    ListLayout lay;
    // ---- 1. + 2. the dead rows, keep / drop per stored entry, its exclusive scan (new positions), the scan at the
    //              (list, column) boundaries: new sizes, offsets and columns
    TRY(rows_d.ensure((size_t)n * 8));
    HIPCHECK(hipMemcpy(rows_d.p, rv.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    std::vector<int64_t> g;
    TRY(kept_entries(ix, rows_d.as<int64_t>(), n, ioff0, cols0, cw, dead, keep, scan, tmp, bad, pos_d, gat, g));
    const int64_t T1 = g.back();
    if (T1 == T0) return TK_OK;     // nothing stored was named: the index stays exactly as it is
    std::vector<int64_t> size1((size_t)L), cols1((size_t)(L * cw));
    for (int64_t l = 0; l < L; l++) {
        for (int t = 0; t < cw; t++) cols1[(size_t)(l * cw + t)] = g[(size_t)(l * cw + t) + 1] - g[(size_t)(l * cw + t)];
        size1[(size_t)l] = g[(size_t)(l + 1) * cw] - g[(size_t)l * cw];
    }
    // ---- 3. the old position of every kept entry; the zero vector's code (list padding)
    TRY(src.ensure((size_t)(T1 > 0 ? T1 : 1) * 4));
    tk_launch_scatter_kept(keep.as<long long>(), scan.as<long long>(), T0, src.as<int>(), 0);
    HIPCHECK(hipGetLastError());
    TRY(zero_labels_dev(ix, rot, zrow, zlab));
    // ---- 4. the compacted lists (their small arrays are allocated while the kernels above run)
    TRY(lay.set_sizes(size1.data(), L));
    const int64_t chunks1 = lay.total_chunks;
    const size_t tiled_bytes = (size_t)tk_tiled_uint4s(chunks1, ix->M / 2) * 16;
    TRY(lay.codes.ensure(tiled_bytes > 0 ? tiled_bytes : 16));
    HIPCHECK(hipMemset(lay.codes.p, 0, tiled_bytes > 0 ? tiled_bytes : 16));
    TRY(lay.ids.ensure((size_t)(T1 > 0 ? T1 : 1) * 8));
    const bool want32 = ix->have_ids32 && T1 > 0;
    if (want32) TRY(lay.ids32.ensure((size_t)T1 * 4));
    tk_launch_compact_lists(ix->codes.as<uint4>(), ix->list_chunk_off.as<int64_t>(), ix->ids_off.as<int64_t>(),
                            ix->ids.as<int64_t>(), src.as<int>(), ix->M, lay.list_chunk_off.as<int64_t>(),
                            lay.ids_off.as<int64_t>(), lay.list_n.as<int64_t>(), (int)L, zlab.as<uint8_t>(),
                            lay.codes.as<uint4>(), lay.ids.as<int64_t>(), want32 ? lay.ids32.as<int32_t>() : nullptr,
                            chunks1, 0);
    HIPCHECK(hipGetLastError());
    // ---- 5. what tk_index_set_lists derives from the labels: distinct?  the largest?
    int cs[4];
    TRY(row_copies(ix, lay.ids.as<int64_t>(), T1, cnt, summ, cs));
    HIPCHECK(hipDeviceSynchronize());
    lay.ids_unique = cs[1] <= 1;
    lay.have_ids32 = want32 && !lay.ids_unique;
    // (the largest label as tk_index_set_lists finds it: the same twin table as an upload of these lists)
    lay.max_label = cs[0];
    if (cols_src) {
        lay.list_cols = cols1;
        lay.kp = kp;
    }
    // ---- 6. the swap: the old buffers go with the layout
    TRY(install_lists(ix, lay));
    if (removed_out) *removed_out = T0 - T1;
    return TK_OK;
}

// Stored rows replaced in place, ids kept (tinyknn_hip.h): tk_index_remove_rows of the ids and tk_index_add_rows of
// the rows in one pass over the code array, the new entries labelled ids[i] and their vectors written over rows
// ids[i].  The order matters, because this is the one list change that overwrites live vectors: (1) the checks;
// (2) settle_lists, so that batches in flight finish on the old lists AND the old vectors (as in add and remove it
// comes before the call's own device work, which then runs on an idle device); (3) the rows staged in a scratch
// buffer — never in the live store — and prepared, assigned, coded and (half store) checked there; (4) the new lists
// built completely in new buffers, what the labels say derived from them (row_copies, as the removal does), the
// device synchronised; (5) only then, behind the last point that can fail, the scatter into the store and the swap.
extern "C" int tk_index_update_rows(tk_index *ix, const int64_t *ids, int64_t n, const void *rows, int rows_is_f64,
                                    int kp, const int64_t *nearest, const uint8_t *labels,
                                    const int64_t *list_columns, int normalise, const float *all_centers,
                                    const float *search_centers, const float *ynorm2, int64_t C,
                                    const uint64_t *center_codes, int64_t *n_active_out, int64_t *removed_out)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_pq && ix->have_centers && ix->have_lists && ix->have_data, "a complete index");
    ARGCHECK(!ix->sharded, "a list-sharded index replaces no rows");
    ARGCHECK(n >= 0 && (n == 0 || (rows && ids)), "ids / rows");
    ARGCHECK(kp >= 1 && kp <= 9, "kp (lists per row) must be 1 .. 9");
    ARGCHECK(!rows_is_f64 == (ix->data_dtype != TK_DATA_F64),
             "float64 rows only for an index of float64 vectors (float32 rows for float32 and half vectors)");
    const bool half = ix->data_dtype == TK_DATA_F16;
    {
        bool sit = false;
        TRY(rows_sit_in(ix, kp, &sit));
        ARGCHECK(sit, "kp: every stored row sits in kp lists");
    }
    ARGCHECK(list_columns || ix->list_kp == kp,
             "list_columns: the index does not know its members per (list, column) (a host upload)");
    ARGCHECK(C >= ix->n_lists && C >= kp && C < (1ll << 31), "C: the number of centres");
    ARGCHECK(ix->N < (1ll << 31) && ix->total_ids < (1ll << 31) && ix->total_ids + n * kp < (1ll << 31),
             "N and the stored entries (+ n * kp) < 2^31");
    const int d = ix->d, M = ix->M, P = M / 2;
    if (!search_centers) search_centers = all_centers;
    ARGCHECK(nearest || (all_centers && ynorm2 && !rows_is_f64 && d <= 384 && (!normalise || d <= 128)),
             "device assignment: all_centers + ynorm2, float32 rows, d <= 384 (128 with normalisation)");
    ARGCHECK(!normalise || !rows_is_f64, "normalisation on the device: float32 rows");
    ARGCHECK(labels || !rows_is_f64, "device encoding: float32 rows (else pass labels)");
    ARGCHECK(16 % ix->dpb == 0, "dims_per_block must divide 16 for the device encoder");
    if (nearest)
        for (int64_t i = 0; i < n * kp; i++) ARGCHECK(nearest[i] >= 0 && nearest[i] < C, "nearest: a centre id");
    const int64_t L0 = ix->n_lists, T0 = ix->total_ids, N = ix->N;
    std::vector<int64_t> idv((size_t)n);
    if (n > 0) HIPCHECK(hipMemcpy(idv.data(), ids, (size_t)n * 8, hipMemcpyDefault));
    {
        std::vector<uint8_t> named((size_t)N, 0);
        for (int64_t i = 0; i < n; i++) {
            const int64_t r = idv[(size_t)i];
            ARGCHECK(r >= 0 && r < N, "ids: an id outside [0, N)");
            ARGCHECK(!named[(size_t)r], "ids: an id named twice");
            named[(size_t)r] = 1;
        }
    }
    if (n_active_out) *n_active_out = L0;
    if (removed_out) *removed_out = 0;
    if (n == 0) return TK_OK;
    TRY(settle_lists(ix));
    // ---- the old layout: list sizes, offsets, members per column
    std::vector<int64_t> size0((size_t)L0), ioff0((size_t)L0 + 1);
    HIPCHECK(hipMemcpy(size0.data(), ix->list_n.p, (size_t)L0 * 8, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(ioff0.data(), ix->ids_off.p, (size_t)(L0 + 1) * 8, hipMemcpyDeviceToHost));
    std::vector<int64_t> cols0(list_columns ? list_columns : ix->list_cols.data(),
                               (list_columns ? list_columns : ix->list_cols.data()) + L0 * kp);
    TRY(check_columns(cols0, size0, L0, kp));
    DevBuf xstage, hflag, ids_d, dead, keep, scan, stmp, bad, pos_d, gat, src, yt, yn, near, keys, prow, keys2, rows2, count,
        lab, rot, tmp, zrow, zlab, crow, clab, coffs, act1, ccodes, noff_d, seg_d, koff_d, cnt, summ;
    BufCleanup cl{{&xstage, &hflag, &ids_d, &dead, &keep, &scan, &stmp, &bad, &pos_d, &gat, &src, &yt, &yn, &near, &keys, &prow,
                   &keys2, &rows2, &count, &lab, &rot, &tmp, &zrow, &zlab, &crow, &clab, &coffs, &act1, &ccodes, &noff_d,
                   &seg_d, &koff_d, &cnt, &summ}};
    ListLayout lay;
    // ---- 1. the rows in a scratch buffer; nearest centres, pairs per (centre, column); what a half store will hold
    TRY(xstage.ensure((size_t)n * d * (rows_is_f64 ? 8 : 4)));
    void *Xn = xstage.p;
    HIPCHECK(hipMemcpy(Xn, rows, (size_t)n * d * (rows_is_f64 ? 8 : 4), hipMemcpyDefault));
    const int64_t T = n * kp;
    std::vector<int> cntc;
    TRY(new_row_pairs(Xn, n, d, kp, nearest, normalise, search_centers, ynorm2, C, yt, yn, near, keys, prow, count, cntc));
    const int64_t L1 = active_prefix(cntc, C, kp, L0);
    ARGCHECK(L1 >= 0, PREFIX_REFUSAL);
    ARGCHECK(L1 == L0 || all_centers, "new lists: all_centers");
    if (half) TRY(check_half_rows((const float *)Xn, n, d, 0, hflag));     // (names the row of `rows`, not an id)
    // ---- 2. the entries that stay: keep / drop per stored entry, the scan, the old position of every kept one
    TRY(ids_d.ensure((size_t)n * 8));
    HIPCHECK(hipMemcpy(ids_d.p, idv.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    std::vector<int64_t> g;
    TRY(kept_entries(ix, ids_d.as<int64_t>(), n, ioff0, cols0, kp, dead, keep, scan, stmp, bad, pos_d, gat, g));
    const int64_t Tk = g.back();
    TRY(src.ensure((size_t)(Tk > 0 ? Tk : 1) * 4));
    tk_launch_scatter_kept(keep.as<long long>(), scan.as<long long>(), T0, src.as<int>(), 0);
    HIPCHECK(hipGetLastError());
    // ---- 3. the new layout: list l's column block j = kept_j ++ new_j
    std::vector<int64_t> size1((size_t)L1), noff((size_t)L1 + 1, 0), koff((size_t)L1 + 1, Tk), seg((size_t)L1 * kp * 2),
        cols1((size_t)L1 * kp);
    for (int64_t l = 0; l < L1; l++) {
        int64_t s = 0, sn = 0;
        if (l < L0) koff[(size_t)l] = g[(size_t)(l * kp)];
        for (int t = 0; t < kp; t++) {
            const int64_t o = l < L0 ? g[(size_t)(l * kp + t) + 1] - g[(size_t)(l * kp + t)] : 0;
            const int64_t nn = cntc[(size_t)(l * kp + t)];
            seg[(size_t)(l * kp + t) * 2] = o;
            seg[(size_t)(l * kp + t) * 2 + 1] = nn;
            cols1[(size_t)(l * kp + t)] = o + nn;
            s += o + nn;
            sn += nn;
        }
        size1[(size_t)l] = s;
        noff[(size_t)l + 1] = noff[(size_t)l] + sn;
    }
    TRY(lay.set_sizes(size1.data(), L1));
    const int64_t chunks1 = lay.total_chunks, T1 = lay.total_ids;       // (T1 = Tk + n * kp > 0)
    // ---- 4. new pairs grouped by list; codes of the new rows, of the zero vector, of new centres
    TRY(sort_pairs_dev(keys, prow, keys2, rows2, tmp, T, L1));
    TRY(new_row_labels(ix, Xn, n, labels, rot, lab));
    TRY(zero_labels_dev(ix, rot, zrow, zlab));
    if (L1 > L0) TRY(grown_centres(ix, all_centers, center_codes, L1, rot, crow, clab, coffs, act1, ccodes));
    // ---- 5. the new lists: the old code array is read once, the new one written once
    TRY(noff_d.ensure(noff.size() * 8));
    TRY(koff_d.ensure(koff.size() * 8));
    TRY(seg_d.ensure(seg.size() * 8));
    HIPCHECK(hipMemcpy(noff_d.p, noff.data(), noff.size() * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(koff_d.p, koff.data(), koff.size() * 8, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(seg_d.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice));
    const size_t tiled_bytes = (size_t)tk_tiled_uint4s(chunks1, P) * 16;
    TRY(lay.codes.ensure(tiled_bytes));
    HIPCHECK(hipMemset(lay.codes.p, 0, tiled_bytes));
    TRY(lay.ids.ensure((size_t)T1 * 8));
    const bool want32 = kp > 1 || ix->have_ids32;
    if (want32) TRY(lay.ids32.ensure((size_t)T1 * 4));
    tk_launch_replace_lists(ix->codes.as<uint4>(), ix->list_chunk_off.as<int64_t>(), ix->ids_off.as<int64_t>(),
                            ix->ids.as<int64_t>(), (int)L0, src.as<int>(), koff_d.as<int64_t>(), lab.as<uint8_t>(), M,
                            rows2.as<int>(), ids_d.as<int64_t>(), noff_d.as<int64_t>(), seg_d.as<int64_t>(), kp,
                            lay.list_chunk_off.as<int64_t>(), lay.ids_off.as<int64_t>(), lay.list_n.as<int64_t>(), (int)L1,
                            zlab.as<uint8_t>(), lay.codes.as<uint4>(), lay.ids.as<int64_t>(),
                            want32 ? lay.ids32.as<int32_t>() : nullptr, chunks1, 0);
    HIPCHECK(hipGetLastError());
    // ---- 6. what tk_index_set_lists derives from the labels (as the removal): distinct?  the largest?
    int cs[4];
    TRY(row_copies(ix, lay.ids.as<int64_t>(), T1, cnt, summ, cs));
    HIPCHECK(hipDeviceSynchronize());
    lay.ids_unique = cs[1] <= 1;
    lay.have_ids32 = want32 && !lay.ids_unique;
    lay.max_label = cs[0];
    lay.list_cols = cols1;
    lay.kp = kp;
    // ---- 7. nothing fails from here on (a launch into buffers that exist; set_centre_slots: a few bytes that
    //         exist): the vectors over the old rows', the swap
    tk_launch_scatter_rows(Xn, n, d, ids_d.as<int64_t>(), ix->data.p, ix->data_dtype, 0);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());       // (ids_d and the scratch rows leave with this call)
    if (L1 > L0) {
        std::swap(ix->active_centers, act1);
        std::swap(ix->center_codes, ccodes);
        TRY(set_centre_slots(ix, L1, (L1 + 15) / 16));
    }
    TRY(install_lists(ix, lay));
    if (n_active_out) *n_active_out = L1;
    if (removed_out) *removed_out = T0 - Tk;
    return TK_OK;
}

// A complete unsharded index (tk_index_build_dev, or the host upload) becomes this rank's shard
// of a list-sharded index IN PLACE: the codes of the lists with owner[l] == rank are compacted
// into the rank's own array, everything else (centres, ids, vectors) stays replicated.
extern "C" int tk_index_shard_resident(tk_index *ix, const int32_t *owner, int rank, int world)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_lists && !ix->sharded, "a complete unsharded index");
    ARGCHECK(owner && world >= 1 && rank >= 0 && rank < world, "owner / rank / world");
    TRY(flush_pending(ix));
    HIPCHECK(hipDeviceSynchronize());
    const int64_t L = ix->n_lists;
    std::vector<int64_t> sizes((size_t)L), coff((size_t)L + 1, 0), loff((size_t)L + 1, 0);
    HIPCHECK(hipMemcpy(sizes.data(), ix->list_n.p, (size_t)L * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < L; i++) {
        ARGCHECK(owner[i] >= 0 && owner[i] < world, "owner out of range");
        const int64_t c = (sizes[(size_t)i] + 15) / 16;
        coff[(size_t)i + 1] = coff[(size_t)i] + c;
        loff[(size_t)i + 1] = loff[(size_t)i] + (owner[i] == rank ? c : 0);
    }
    const int P = ix->M / 2;
    TRY(ix->owner.ensure((size_t)L * 4));
    TRY(ix->local_chunk_off.ensure((size_t)(L + 1) * 8));
    HIPCHECK(hipMemcpy(ix->owner.p, owner, (size_t)L * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ix->local_chunk_off.p, loff.data(), (size_t)(L + 1) * 8, hipMemcpyHostToDevice));
    DevBuf mine;
    const size_t bytes = (size_t)tk_tiled_uint4s(loff[(size_t)L], P) * 16;
    TRY(mine.ensure(bytes > 0 ? bytes : 16));
    HIPCHECK(hipMemset(mine.p, 0, bytes > 0 ? bytes : 16));
    tk_launch_compact_tiled(ix->codes.as<uint4>(), mine.as<uint4>(), P, ix->list_chunk_off.as<int64_t>(),
                            ix->local_chunk_off.as<int64_t>(), (int)L, loff[(size_t)L], 0);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    ix->codes.release();
    ix->codes = mine;            // (DevBuf is a plain pointer + capacity)
    ix->sharded = true;
    ix->rank = rank;
    ix->world = world;
    return TK_OK;
}

// Another rank's shard of a complete unsharded index on the same device (tinyknn_hip.h): the clone borrows
// the replicated arrays and owns the compacted codes of its lists.
extern "C" tk_index *tk_index_clone_shard(tk_index *src, const int32_t *owner, int rank, int world)
{
    if (!src || !owner || world < 1 || rank < 0 || rank >= world || !src->have_lists || !src->have_data ||
        src->sharded) {
        (void)fail(TK_ERR_ARG, "bad argument: tk_index_clone_shard wants a complete unsharded index, an owner map and rank < world");
        return nullptr;
    }
    IXLOCK(src);
    if (flush_pending(src) != TK_OK || hipDeviceSynchronize() != hipSuccess) return nullptr;
    tk_index *ix = tk_index_create();
    if (!ix) return nullptr;
    ix->pq_centers.borrow(src->pq_centers);
    ix->dq = src->dq; ix->dpb = src->dpb; ix->M = src->M; ix->f_order = src->f_order; ix->order = src->order;
    ix->sqrt_nb = src->sqrt_nb;
    ix->active_centers.borrow(src->active_centers);
    ix->center_codes.borrow(src->center_codes);
    ix->n_lists = src->n_lists; ix->center_chunks = src->center_chunks; ix->d = src->d;
    ix->list_chunk_off.borrow(src->list_chunk_off);
    ix->list_n.borrow(src->list_n);
    ix->ids_off.borrow(src->ids_off);
    ix->ids.borrow(src->ids);
    ix->ids32.borrow(src->ids32);
    ix->have_ids32 = src->have_ids32;
    ix->labels24 = src->labels24;
    ix->twin_list.borrow(src->twin_list);
    ix->twin_off.borrow(src->twin_off);
    ix->twin_w = src->twin_w;
    ix->twin_unverified = src->twin_unverified;
    ix->twin_vouched = src->twin_vouched;
    ix->opt_replay_twin = src->opt_replay_twin;
    ix->total_chunks = src->total_chunks; ix->total_ids = src->total_ids;
    ix->max_list_chunks = src->max_list_chunks;
    ix->ids_unique = src->ids_unique;
    ix->cslots_i.borrow(src->cslots_i);
    ix->cslots_l.borrow(src->cslots_l);
    ix->c_chunk_off.borrow(src->c_chunk_off);
    ix->rot_t.borrow(src->rot_t);
    ix->rot_d_pad = src->rot_d_pad;
    ix->data.borrow(src->data);
    ix->N = src->N; ix->data_dtype = src->data_dtype;
    src->data_lent = true;
    ix->have_pq = ix->have_centers = ix->have_lists = ix->have_data = true;
    ix->plain_mode = src->plain_mode;
    // this rank's codes
    const int64_t L = ix->n_lists;
    std::vector<int64_t> sizes((size_t)L), loff((size_t)L + 1, 0);
    bool ok = hipMemcpy(sizes.data(), src->list_n.p, (size_t)L * 8, hipMemcpyDeviceToHost) == hipSuccess;
    for (int64_t i = 0; ok && i < L; i++) {
        ok = owner[i] >= 0 && owner[i] < world;
        loff[(size_t)i + 1] = loff[(size_t)i] + (owner[i] == rank ? (sizes[(size_t)i] + 15) / 16 : 0);
    }
    const int P = ix->M / 2;
    const size_t bytes = (size_t)tk_tiled_uint4s(loff[(size_t)L], P) * 16;
    ok = ok && ix->owner.ensure((size_t)L * 4) == TK_OK && ix->local_chunk_off.ensure((size_t)(L + 1) * 8) == TK_OK &&
         ix->codes.ensure(bytes > 0 ? bytes : 16) == TK_OK;
    ok = ok && hipMemcpy(ix->owner.p, owner, (size_t)L * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(ix->local_chunk_off.p, loff.data(), (size_t)(L + 1) * 8, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(ix->codes.p, 0, bytes > 0 ? bytes : 16) == hipSuccess;
    if (ok) {
        tk_launch_compact_tiled(src->codes.as<uint4>(), ix->codes.as<uint4>(), P, ix->list_chunk_off.as<int64_t>(),
                                ix->local_chunk_off.as<int64_t>(), (int)L, loff[(size_t)L], 0);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    if (!ok) {
        (void)fail(TK_ERR_HIP, "tk_index_clone_shard: owner out of range, or a HIP call failed");
        tk_index_destroy(ix);
        return nullptr;
    }
    ix->sharded = true;
    ix->rank = rank;
    ix->world = world;
    return ix;
}

// what a built index holds, back on the host in the reference's formats: list_sizes
// (n_lists,), codes (total chunks, M) uint64 Quick-ADC layout, ids (sum sizes,) — any NULL
extern "C" int tk_index_export_lists(tk_index *ix, int64_t *list_sizes, uint64_t *codes, int64_t *ids)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_lists && !ix->sharded, "an unsharded index with lists");
    if (list_sizes)
        HIPCHECK(hipMemcpy(list_sizes, ix->list_n.p, (size_t)ix->n_lists * 8, hipMemcpyDeviceToHost));
    if (ids && ix->total_ids > 0)
        HIPCHECK(hipMemcpy(ids, ix->ids.p, (size_t)ix->total_ids * 8, hipMemcpyDeviceToHost));
    if (codes && ix->total_chunks > 0) {
        const int P = ix->M / 2;
        const int64_t n4 = tk_tiled_uint4s(ix->total_chunks, P);
        std::vector<uint4> t((size_t)n4);
        HIPCHECK(hipMemcpy(t.data(), ix->codes.p, (size_t)n4 * 16, hipMemcpyDeviceToHost));
        uint4 *ref = (uint4 *)codes;
        for (int64_t c = 0; c < ix->total_chunks; c++)
            for (int p = 0; p < P; p++) ref[c * P + p] = t[(size_t)(((c >> 3) * P + p) * 8 + (c & 7))];
    }
    return TK_OK;
}

// active_centers (n_lists, d) float32, center_codes (ceil(n_lists/16), M) uint64 — any NULL
extern "C" int tk_index_export_centers(tk_index *ix, float *active_centers, uint64_t *center_codes)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_centers, "an index with centres");
    if (active_centers)
        HIPCHECK(hipMemcpy(active_centers, ix->active_centers.p, (size_t)ix->n_lists * ix->d * 4,
                           hipMemcpyDeviceToHost));
    if (center_codes) {
        const int P = ix->M / 2;
        const int64_t n4 = tk_tiled_uint4s(ix->center_chunks, P);
        std::vector<uint4> t((size_t)n4);
        HIPCHECK(hipMemcpy(t.data(), ix->center_codes.p, (size_t)n4 * 16, hipMemcpyDeviceToHost));
        uint4 *ref = (uint4 *)center_codes;
        for (int64_t c = 0; c < ix->center_chunks; c++)
            for (int p = 0; p < P; p++) ref[c * P + p] = t[(size_t)(((c >> 3) * P + p) * 8 + (c & 7))];
    }
    return TK_OK;
}

// rows of IVF.data by id (float32 vectors, or half vectors widened), e.g. the candidates a checker wants to rescore
extern "C" int tk_index_read_rows(tk_index *ix, const int64_t *rows, int64_t n, float *out)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data && ix->data_dtype != TK_DATA_F64, "an index with float32 or half vectors");
    ARGCHECK(n >= 0 && (n == 0 || (rows && out)), "buffers");
    for (int64_t i = 0; i < n; i++) ARGCHECK(rows[i] >= 0 && rows[i] < ix->N, "row id out of range");
    if (n == 0) return TK_OK;
    DevBuf r, o;
    int rc = r.ensure((size_t)n * 8);
    if (rc == TK_OK) rc = o.ensure((size_t)n * ix->d * 4);
    if (rc == TK_OK) {
        hipError_t e = hipMemcpy(r.p, rows, (size_t)n * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            tk_launch_gather_rows(ix->data.p, ix->data_dtype, ix->d, r.as<int64_t>(), n, o.as<float>(), 0);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(out, o.p, (size_t)n * ix->d * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(TK_ERR_HIP, hipGetErrorString(e));
    }
    r.release();
    o.release();
    return rc;
}

// ---------------------------------------------------------------------------
// device front end ("fast mode")
extern "C" int tk_index_set_rotation(tk_index *ix, const double *R, int d_pad)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_pq && ix->have_centers, "set_pq and set_centers first");
    if (!R) {
        ix->rot_t.release();
        ix->rot_d_pad = 0;
        return TK_OK;
    }
    ARGCHECK(d_pad >= ix->d && d_pad <= 16384, "d_pad");
    return upload_rotation(ix, R, d_pad);
}

extern "C" int tk_index_prepare_dev(tk_index *ix, const float *q_raw_dev, int64_t nq, int angular,
                                    float *qn_dev, void *q_pq_dev, void *stream)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_pq && ix->have_centers, "set_pq and set_centers first");
    ARGCHECK(nq >= 0 && q_raw_dev && qn_dev && q_pq_dev, "buffers");
    ARGCHECK(!angular || ix->d <= 128, "device normalisation needs d <= 128");
    ARGCHECK(ix->rot_d_pad > 0 || ix->dq >= ix->d, "unrotated PQ: dq >= d");
    hipStream_t st = (hipStream_t)stream;
    if (angular)
        tk_launch_normalise_rows(q_raw_dev, nq, ix->d, qn_dev, st);
    else if (qn_dev != q_raw_dev)
        HIPCHECK(hipMemcpyAsync(qn_dev, q_raw_dev, (size_t)nq * ix->d * 4, hipMemcpyDeviceToDevice, st));
    tk_launch_prepare_queries(qn_dev, nq, ix->d, ix->rot_d_pad ? ix->rot_t.as<double>() : nullptr,
                              ix->dq, ix->rot_d_pad ? ix->rot_d_pad : ix->dq, q_pq_dev, st);
    HIPCHECK(hipGetLastError());
    return TK_OK;
}

extern "C" int tk_index_query_batch_raw(tk_index *ix, const float *q_raw, int64_t nq, int angular,
                                        int k, int n_probes, int pass_1, int64_t *out_ids)
{
    IXLOCK(ix);
    Plan p;
    TRY(make_plan(ix, k, n_probes, pass_1, p));
    ARGCHECK(nq >= 0 && q_raw && out_ids, "buffers");
    if (nq == 0) return TK_OK;
    const int f64 = ix->rot_d_pad > 0;
    DevBuf raw, outbuf;
    TRY(raw.ensure((size_t)nq * ix->d * 4));
    TRY(ix->q.ensure((size_t)nq * ix->d * 4));
    TRY(ix->qpq.ensure((size_t)nq * ix->dq * (f64 ? 8 : 4)));
    TRY(outbuf.ensure((size_t)nq * k * 8));
    HIPCHECK(hipMemcpy(raw.p, q_raw, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice));
    int r = tk_index_prepare_dev(ix, raw.as<float>(), nq, angular, ix->q.as<float>(), ix->qpq.p, nullptr);
    if (r == TK_OK)
        r = tk_index_query_batch_dev(ix, ix->q.as<float>(), ix->qpq.p, f64, nq, k, n_probes, pass_1,
                                     outbuf.as<int64_t>(), nullptr);
    if (r == TK_OK) r = flush_pending(ix);
    if (r == TK_OK) {
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(out_ids, outbuf.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = fail(TK_ERR_HIP, hipGetErrorString(e));
    }
    raw.release();
    outbuf.release();
    return r;
}

// ---------------------------------------------------------------------------
// exact k nearest vectors of IVF.data: the ground truth of recall (brute.hip)
// r (or NULL): the restriction, its arrays on the device.  retry: a candidate list that overflowed under the segment
// rule is not an error — the selection runs once more from the sampled tau with the segment length that cannot
// overflow, the largest multiple of 32 not above cap - k (a segment appends at most `seg` rows to at most k kept ones).
static int knn_brute(tk_index *ix, const float *q, int64_t nq, int k, const TkBruteRestrict *r, bool retry,
                     int64_t *out_ids, float *out_dist)
{
    ARGCHECK(ix && ix->have_data, "set_data first");
    ARGCHECK(ix->data_dtype != TK_DATA_F64, "float32 vectors only");
    ARGCHECK(ix->data_dtype != TK_DATA_F16, "knn_brute is the ground truth on float32 vectors: this index stores "
                                            "them as half (store=\"float16\"); ask a float32 index");
    ARGCHECK(ix->d <= 128, "d <= 128");
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
    if (tk_launch_brute_tau(X, nq, ix->d, Y, ix->N, k, ix->br_ynorm.as<float>(), ix->br_vals.as<float>(), ns, tau,
                            ix->br_sample.as<float>(), r, nullptr))
        return fail(TK_ERR_HIP, "tk_launch_knn_brute: unsupported size / LDS attribute");
    if (retry) HIPCHECK(hipMemcpyAsync(tau0, tau, (size_t)nq * 4, hipMemcpyDeviceToDevice, nullptr));
    int64_t seg = tk_brute_segment(k, ns, cap);
    for (int attempt = 0;; attempt++) {
        if (tk_launch_brute_select(X, nq, ix->d, Y, ix->N, k, ix->br_ynorm.as<float>(), tau,
                                   ix->br_cand.as<unsigned long long>(), cap, ix->br_count.as<int>(), overflow,
                                   ix->br_out.as<int64_t>(), dist, seg, r, nullptr))
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

// A host array of a restricted call in its workspace buffer (NULL stays NULL)
template <typename T>
static int brute_upload(DevBuf &b, const T *host, size_t n, const T *&dev)
{
    dev = nullptr;
    if (!host) return TK_OK;
    TRY(b.ensure((n > 0 ? n : 1) * sizeof(T)));
    HIPCHECK(hipMemcpy(b.p, host, n * sizeof(T), hipMemcpyHostToDevice));
    dev = b.as<T>();
    return TK_OK;
}

// The restriction of a restricted exact call (tk_index_knn_brute_ex, tk_index_radius_brute, tk_index_radius_probe) from
// the caller's host arrays: the checks they make, the per-query arrays in the br_* workspace buffers, the by-row
// arrays of the index.
// any = false: nothing was given and r is empty.
int brute_restrict(tk_index *ix, int64_t nq, const uint8_t *allowed_mask, const int64_t *exclude,
                   const int32_t *group, const uint64_t *tags, int tag_mode, const int64_t *between,
                   TkBruteRestrict &r, bool &any)
{
    r = TkBruteRestrict{};
    ARGCHECK(tag_mode == 0 || tag_mode == 1, "tag_mode: 0 (any) or 1 (all)");
    // the by-row arrays only: no list-order table is made or read
    if (group) TRY(row_table_covers(ix, ix->groups));
    if (tags) TRY(row_table_covers(ix, ix->tags));
    if (between) TRY(row_table_covers(ix, ix->values));
    if (exclude)
        for (int64_t i = 0; i < nq; i++) ARGCHECK(exclude[i] >= -1 && exclude[i] < ix->N, "exclude: entries in [-1, N)");
    any = allowed_mask || exclude || group || tags || between;
    if (!any || nq == 0) return TK_OK;
    r.n_rows = ix->N;
    r.tag_mode = tag_mode;
    if (allowed_mask) {
        std::vector<uint32_t> bits((size_t)(ix->N + 31) / 32, 0u);
        for (int64_t j = 0; j < ix->N; j++)         // (no branch: a random mask would mispredict every other row)
            bits[(size_t)(j >> 5)] |= (uint32_t)(allowed_mask[j] != 0) << (j & 31);
        TRY(brute_upload(ix->br_mask, bits.data(), bits.size(), r.allowed));
    }
    TRY(brute_upload(ix->br_exclude, exclude, (size_t)nq, r.exclude));
    TRY(brute_upload(ix->br_group, group, (size_t)nq, r.group));
    TRY(brute_upload(ix->br_tags, tags, (size_t)nq, r.tags));
    if (group) r.row_groups = ix->groups.by_row.as<int32_t>();
    if (tags) r.row_tags = ix->tags.by_row.as<uint64_t>();
    if (between) {
        r.cols = value_columns(ix);
        r.row_keys = ix->values.by_row.as<int64_t>();
        TRY(brute_upload(ix->br_ranges, between, (size_t)nq * 2 * r.cols, r.ranges));
    }
    return TK_OK;
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
    TRY(brute_restrict(ix, nq, allowed_mask, exclude, group, tags, tag_mode, between, r, any));
    if (!any) return knn_brute(ix, q, nq, k, nullptr, true, out_ids, out_dist);
    if (nq == 0) return TK_OK;
    return knn_brute(ix, q, nq, k, &r, true, out_ids, out_dist);
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
    TRY(brute_restrict(ix, nq, allowed_mask, exclude, group, tags, tag_mode, between, r, any));
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
    if (total == 0) {
        ix->rd_total = 0;
        return TK_OK;
    }
    TRY(ix->rd_off.ensure((size_t)(nq + 1) * 8));
    TRY(ix->rd_keys.ensure((size_t)total * 8));
    TRY(ix->rd_alt.ensure((size_t)total * 8));
    TRY(ix->rd_dist.ensure((size_t)total * 4));
    HIPCHECK(hipMemcpy(ix->rd_off.p, out_lims, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice));
    unsigned long long *keys = ix->rd_keys.as<unsigned long long>(), *alt = ix->rd_alt.as<unsigned long long>();
    if (tk_launch_radius_fill(X, nq, ix->d, Y, ix->N, yn, rad, count, ix->rd_off.as<int64_t>(), slots, keys, err, rp,
                              nullptr))
        return fail(TK_ERR_HIP, "tk_launch_radius_fill: unsupported size / LDS attribute");
    HIPCHECK(hipGetLastError());
    int bad = 0;
    HIPCHECK(hipMemcpy(&bad, err, 4, hipMemcpyDeviceToHost));
    if (bad) return fail(TK_ERR_HIP, "radius_search: count and fill passes disagree");
    if (sorted) {
        size_t bytes = 0;
        if (tk_launch_radius_sort(nullptr, &bytes, keys, alt, total, nq, ix->rd_off.as<int64_t>(), nullptr))
            return fail(TK_ERR_HIP, "tk_launch_radius_sort: work memory query failed");
        TRY(ix->rd_tmp.ensure(bytes > 0 ? bytes : 1));
        if (tk_launch_radius_sort(ix->rd_tmp.p, &bytes, keys, alt, total, nq, ix->rd_off.as<int64_t>(), nullptr))
            return fail(TK_ERR_HIP, "tk_launch_radius_sort failed");
        std::swap(keys, alt);           // the sorted keys; the ids go where the unsorted ones were
    }
    tk_launch_radius_decode(keys, total, (int64_t *)alt, ix->rd_dist.as<float>(), nullptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    ix->rd_ids_alt = alt == ix->rd_alt.as<unsigned long long>();
    ix->rd_total = total;
    return TK_OK;
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

// _FastDistanceTable.top (fast_pq.py:284-312) for a BATCH of queries against the coded rows the
// index holds as its "centres" (tk_index_set_pq + tk_index_set_centers(rows, packed codes) are
// all it needs): per query a heap of rescore = min(2k + 10, n) PQ estimates over all rows, then
// the exact distances of those candidates, k best in ascending order — the coarse stage of
// IVF.query (ivf.py:131) is exactly this call, so the same three kernels run.  Host buffers;
// queries are processed in chunks whose distance rows fit one workspace.
// Rows far longer than the heap (n >= 2^16 rows): the scan runs on the matrix cores (plain_scan.hip)
// behind an exact HEAD — the first n/64 rows — after which the heap is full of real values and its
// bound far below the table's limit C; the lane replay checks exactly that per query (bound at the
// first plain block <= C) and fetches only the blocks whose minimum passes its bound (LAZY).  A chunk
// of queries in which any query fails the check is answered again by the exact kernel alone, and an
// index on which more than 1 % fail (rows without structure) stays on the exact kernel.
// out_dist (or NULL): the float32 exact squared distances beside the ids (+inf beside a -1 of the padding)
// The chunks of that call, their result left on the device: for every chunk of m queries from query o on, once its
// (m, kc) probes are in the workspace (and, where want_dist, their distances) and the device is idle, sink(o, m, kc,
// probes, dist) is called with device pointers that hold until it returns.  kc = min(k, n_lists).
int coarse_top_chunks(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq, int k,
                      bool want_dist, const TkProbeSink &sink)
{
    ARGCHECK(ix && ix->have_pq && ix->have_centers, "set_pq and set_centers first");
    ARGCHECK(nq >= 0 && k >= 1 && (nq == 0 || (q && q_pq)), "buffers / sizes");
    if (nq == 0) return TK_OK;
    TRY(flush_pending(ix));
    Plan p;
    const int64_t kc = k < ix->n_lists ? k : ix->n_lists;                        // fast_pq.py:263
    const int64_t rescore = 2 * kc + 10 < ix->n_lists ? 2 * kc + 10 : ix->n_lists;   // :264-265
    ARGCHECK(rescore * 12 + 16 <= 64 * 1024, "heap larger than 64 KiB of LDS");
    p.kc = (int)kc; p.rescore = (int)rescore; p.R = (int)rescore; p.S = 1;
    p.cap = 1; p.cap_min = 16;
    p.ccap_min = (ix->center_chunks + 15) / 16 * 16;
    int64_t chunk = (int64_t)(workspace_bytes() / ((double)ix->center_chunks * 17.0));
    chunk = chunk < 16 ? 16 : (chunk > MAX_SUB ? MAX_SUB : chunk);
    chunk = chunk < nq ? chunk : nq;
    Work &w = ix->works[0];
    const int M = ix->M;
    const size_t esz = q_pq_is_f64 ? 8 : 4;
    struct ScopedBuf : DevBuf {
        ~ScopedBuf() { release(); }
    } dbuf;             // (freed on every return)
    if (want_dist) TRY(dbuf.ensure((size_t)chunk * p.kc * 4));
    float *dist = want_dist ? dbuf.as<float>() : nullptr;
    const bool lanes = ix->heap_mode == 0 && tk_positions_fit(ix->center_chunks) && p.rescore <= TK_LANES_MAX_R;
    const bool lazy = lanes && ix->center_chunks >= 1024;
    const int hc = (int)(ix->center_chunks / 64 < 16 ? 16 : ix->center_chunks / 64);     // exact head, in chunks
    bool flat_plain = lanes && ix->plain_mode != 1 && plain_env_on() && tk_plain_fits(M) && ix->flat_plain_ok &&
                      ix->center_chunks >= 4096 && coarse_units(ix, chunk);
    TkPairSet pl;
    TRY(w.tables.ensure((size_t)chunk * M * 16));
    TRY(w.shift.ensure((size_t)chunk * 8));
    TRY(w.scale.ensure((size_t)chunk * 8));
    TRY(w.cdist.ensure((size_t)chunk * ix->center_chunks * 16));
    TRY(w.cmins.ensure((size_t)chunk * p.ccap_min));
    TRY(w.cheap_idx.ensure((size_t)chunk * p.rescore * 8));
    TRY(w.cheap_val.ensure((size_t)chunk * p.rescore * 4));
    TRY(w.probes.ensure((size_t)chunk * p.kc * 8));
    TRY(w.c_pair_off.ensure(8));
    TRY(w.c_unit_prefix.ensure(tk_unit_prefix_ints(1) * 4));
    TRY(w.c_pair_q.ensure(((size_t)chunk + 4) * 4));
    TRY(w.c_pair_f0.ensure(((size_t)chunk + 4) * 4));
    TRY(ix->q.ensure((size_t)chunk * ix->d * 4));
    TRY(ix->qpq.ensure((size_t)chunk * ix->dq * esz));
    if (flat_plain) {
        const int K = 64;
        const int64_t nsub = ((ix->center_chunks + 1) / 2 + K - 1) / K;
        TRY(w.qlim.ensure((size_t)chunk * 4));
        TRY(w.plain0.ensure((size_t)chunk * 4));
        TRY(w.repeat_flag.ensure((size_t)chunk));
        TRY(w.flag_list.ensure(((size_t)chunk + 1) * 4));
        TRY(w.p_pair_off.ensure(8));
        TRY(w.p_unit_prefix.ensure(tk_unit_prefix_ints(1) * 4));
        TRY(w.p_pair_q.ensure(((size_t)chunk + 4) * 4));
        TRY(w.p_pair_f0.ensure(((size_t)chunk + 4) * 4));
        TRY(w.p_unit_desc.ensure((size_t)((chunk + 31) / 32) * nsub * 16 + 64));
        if (!w.flag_host) {
            HIPCHECK(hipHostMalloc((void **)&w.flag_host, 64, hipHostMallocDefault));
            *w.flag_host = 0;
        }
        pl = TkPairSet{nullptr, nullptr, w.p_pair_off.as<int>(), w.p_unit_prefix.as<int>(), w.p_pair_q.as<int>(),
                       w.p_pair_f0.as<int>(), w.p_unit_desc.as<int>(), K};
        std::vector<int> h((size_t)chunk, hc);      // every query: plain sums from flat chunk hc on
        HIPCHECK(hipMemcpy(w.plain0.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
    // heap replay over the centre rows (fresh heap, positions as labels) + exact rescoring -> w.probes
    auto replay_rescore = [&](int64_t m, bool plain) -> int {
        if (!lanes) {
            Prof pf;
            return coarse_replay_probes(ix, w, ix->q.as<float>(), m, p, w.probes.as<int64_t>(), nullptr, pf, TkSecond(),
                                        nullptr, nullptr, dist);
        }
        TkLanesOpts o;
        o.lazy = lazy ? 1 : 0;
        if (plain) {
            o.skip = w.repeat_flag.as<unsigned char>();
            o.check = {w.plain0.as<int>(), w.qlim.as<int>()};
        }
        if (tk_launch_heap_replay_lanes(centre_replay_job(ix, w, m, p), o, nullptr))
            return fail(TK_ERR_HIP, "hipFuncSetAttribute(LDS size) failed");
        tk_launch_rescore(ix->q.as<float>(), 0, ix->d, ix->active_centers.p, 0, ix->n_lists,
                          w.cheap_idx.as<int64_t>(), p.rescore, m, p.kc, 0, w.probes.as<int64_t>(), nullptr, nullptr,
                          ix->opt_rescore_form, TkSecond(), TkSecond(), nullptr, dist);
        return TK_OK;
    };
    for (int64_t o = 0; o < nq; o += chunk) {
        const int64_t m = nq - o < chunk ? nq - o : chunk;
        HIPCHECK(hipMemcpy(ix->q.p, q + o * ix->d, (size_t)m * ix->d * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(ix->qpq.p, (const char *)q_pq + (size_t)o * ix->dq * esz, (size_t)m * ix->dq * esz,
                           hipMemcpyHostToDevice));
        Prof pf;
        bool exact = !flat_plain;
        if (flat_plain) {
            TRY(stage_tables(ix, w, ix->qpq.p, q_pq_is_f64, m, nullptr, pf, true));
            HIPCHECK(hipMemsetAsync(w.repeat_flag.p, 0, (size_t)m, nullptr));
            // plain sums of every row first; the exact kernel then overwrites the head chunks
            tk_launch_plain_identity(m, (int)ix->center_chunks, pl, nullptr);
            TkScanJob pj = coarse_job(ix, w, p);
            pj.unit_prefix = pl.unit_prefix; pj.pair_off = pl.pair_off; pj.pair_q = pl.pair_q; pj.pair_f0 = pl.pair_f0;
            pj.unit_desc4 = pl.unit_desc;
            if (tk_launch_scan_plain(pj, M, ix->order, plain_blocks(), nullptr))
                return fail(TK_ERR_HIP, "scan_plain_wave_kernel: LDS attribute / unsupported M");
            tk_launch_identity_pairs(m, hc, w.c_pair_off.as<int>(), w.c_unit_prefix.as<int>(),
                                     w.c_pair_q.as<int>(), w.c_pair_f0.as<int>(), nullptr);
            TkScanJob hj = coarse_job(ix, w, p), none;
            memset(&none, 0, sizeof none);
            hj.max_chunks = hc;
            tk_launch_scan_units2(hj, none, M, ix->order, 768, nullptr, nullptr, 0);
            TRY(replay_rescore(m, true));
            tk_launch_flagged_list(w.repeat_flag.as<unsigned char>(), m, w.flag_list.as<int>(), nullptr, w.flag_host);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipDeviceSynchronize());
            const int flagged = *w.flag_host;
            if (flagged > 0) exact = true;                       // (this chunk again, exactly)
            if ((double)flagged > 0.01 * (double)m) {            // rows without structure: not again on this index
                ix->flat_plain_ok = false;
                flat_plain = false;
            }
        }
        if (exact) {
            TRY(stage_tables(ix, w, ix->qpq.p, q_pq_is_f64, m, nullptr, pf));
            launch_coarse_scan(ix, w, m, p, nullptr);
            TRY(replay_rescore(m, false));
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipDeviceSynchronize());
        }
        TRY(sink(o, m, p.kc, w.probes.as<int64_t>(), dist));
    }
    return TK_OK;
}

static int top_centers(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq, int k,
                       int64_t *out_ids, float *out_dist)
{
    ARGCHECK(nq <= 0 || out_ids, "buffers / sizes");
    return coarse_top_chunks(ix, q, q_pq, q_pq_is_f64, nq, k, out_dist != nullptr,
                             [&](int64_t o, int64_t m, int kc, const int64_t *probes, const float *dist) -> int {
        if (kc == k) {
            HIPCHECK(hipMemcpy(out_ids + o * k, probes, (size_t)m * k * 8, hipMemcpyDeviceToHost));
            if (out_dist) HIPCHECK(hipMemcpy(out_dist + o * k, dist, (size_t)m * k * 4, hipMemcpyDeviceToHost));
        } else {    // fewer rows than k: rows of kc ids into rows of k, padded with -1 (+inf)
            std::vector<int64_t> tmp((size_t)m * kc);
            HIPCHECK(hipMemcpy(tmp.data(), probes, tmp.size() * 8, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < m; i++)
                for (int t = 0; t < k; t++)
                    out_ids[(o + i) * k + t] = t < kc ? tmp[(size_t)i * kc + t] : -1;
            if (out_dist) {
                std::vector<float> tmpd((size_t)m * kc);
                HIPCHECK(hipMemcpy(tmpd.data(), dist, tmpd.size() * 4, hipMemcpyDeviceToHost));
                for (int64_t i = 0; i < m; i++)
                    for (int t = 0; t < k; t++)
                        out_dist[(o + i) * k + t] = t < kc ? tmpd[(size_t)i * kc + t] : HUGE_VALF;
            }
        }
        return TK_OK;
    });
}

extern "C" int tk_index_top_centers(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64,
                                    int64_t nq, int k, int64_t *out_ids)
{
    IXLOCK(ix);
    return top_centers(ix, q, q_pq, q_pq_is_f64, nq, k, out_ids, nullptr);
}

extern "C" int tk_index_top_centers_dist(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64,
                                         int64_t nq, int k, int64_t *out_ids, float *out_dist)
{
    IXLOCK(ix);
    ARGCHECK(nq <= 0 || out_dist, "buffers / sizes");
    return top_centers(ix, q, q_pq, q_pq_is_f64, nq, k, out_ids, out_dist);
}
