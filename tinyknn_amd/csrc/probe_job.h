// probe_job.h — what the calls over the probed lists share: radius_probe.hip and knn_probe's two
// distance passes (probe_exact.hip: the exact pass, the tables, the selection and the host driver; probe_matrix.hip:
// the f16 matrix-core pass of matrix=True, §3.22; probe_f32.hip: the f32 matrix-core pass of wide=True, §3.27).
#pragma once
#include "api_internal.h"

// What a job over the probed lists of a call's queries reads, whichever call it is
struct ProbeJob {
    const float *q;                 // (nq, d) prepared queries of the whole call
    const void *rows;               // the vectors, TY
    const int64_t *probes;          // (nq, kc)
    const int64_t *ids, *ids_off, *list_n;
    const int32_t *twin_list;       // twins.hip, twin_w > 0
    int64_t n_lists, N;
    int d, kc, twin_w;
};

// the list a probe names: -1 (an unfilled coarse heap) is the last list; -1 for what names none
__device__ __forceinline__ int32_t probe_list(int64_t p, int64_t n_lists)
{
    if (p < 0) p += n_lists;
    return (p >= 0 && p < n_lists) ? (int32_t)p : -1;
}

// Per (query, rank) of the whole call what its list needs, in units of UNIT rows — 1: a distance key a row (knn_probe),
// 64: a bitmap word per 64 rows (radius_probe) — and 0 at a rank whose list an earlier rank names or that names none
template <int UNIT>
__global__ __launch_bounds__(256) void probe_len_kernel(const int64_t *__restrict__ probes, int64_t n, int kc,
                                                        int64_t n_lists, const int64_t *__restrict__ list_n,
                                                        long long *__restrict__ len)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {               // (the scan's last entry: the total)
        len[i] = 0;
        return;
    }
    const int rank = (int)(i % kc);
    const int64_t *row = probes + (i - rank);
    const int32_t L = probe_list(row[rank], n_lists);
    bool walk = L >= 0;
    for (int t = 0; walk && t < rank; t++) walk = probe_list(row[t], n_lists) != L;
    len[i] = walk ? (list_n[L] + (UNIT - 1)) / UNIT : 0;
}

// kc = min(n_probes, n_lists) and the refusal of a call with 2^31 (query, rank)s or more
static inline int probe_pairs(const tk_index *ix, int64_t nq, int n_probes, int &kc)
{
    kc = (int)(n_probes < ix->n_lists ? n_probes : ix->n_lists);
    ARGCHECK(nq * kc < (1ll << 31), "nq * min(n_probes, n_lists) < 2^31");
    return TK_OK;
}

// The prologue of a call over the probed lists, behind probe_pairs: the index's coarse stage for n_probes, chunk by
// chunk, its probes kept on the device (pl_probes); the queries in br_q; the lengths (probe_len_kernel<UNIT>, pl_len)
// and their exclusive prefix sum (pl_off), nq * kc + 1 entries each, still in flight when it returns; the fields of j
// every such job has.  call: named where the coarse stage's rows are not kc wide.
template <int UNIT>
static int probe_lengths(tk_index *ix, const char *call, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq,
                         int n_probes, int kc, const int32_t *twin_list, int twin_w, ProbeJob &j)
{
    const int64_t pairs = nq * kc;
    TRY(ix->pl_probes.ensure((size_t)pairs * 8));
    TRY(ix->pl_len.ensure((size_t)(pairs + 1) * 8));
    TRY(ix->pl_off.ensure((size_t)(pairs + 1) * 8));
    TRY(ix->br_q.ensure((size_t)nq * ix->d * 4));
    TRY(coarse_top_chunks(ix, q, q_pq, q_pq_is_f64, nq, n_probes, false,
                          [&](int64_t o, int64_t m, int kc_, const int64_t *probes, const float *) -> int {
                              if (kc_ != kc)
                                  return fail(TK_ERR_HIP, std::string(call) + ": the coarse stage's row width");
                              HIPCHECK(hipMemcpy(ix->pl_probes.as<int64_t>() + o * kc, probes, (size_t)m * kc * 8,
                                                 hipMemcpyDeviceToDevice));
                              return TK_OK;
                          }));
    HIPCHECK(hipMemcpy(ix->br_q.p, q, (size_t)nq * ix->d * 4, hipMemcpyHostToDevice));
    long long *len = ix->pl_len.as<long long>(), *off = ix->pl_off.as<long long>();
    hipLaunchKernelGGL(probe_len_kernel<UNIT>, dim3((unsigned)((pairs + 256) / 256)), dim3(256), 0, 0,
                       ix->pl_probes.as<int64_t>(), pairs, kc, ix->n_lists, ix->list_n.as<int64_t>(), len);
    size_t sbytes = 0;
    (void)tk_scan_exclusive64(nullptr, &sbytes, len, off, pairs + 1, nullptr);
    TRY(ix->pl_scan.ensure(sbytes > 0 ? sbytes : 1));
    if (tk_scan_exclusive64(ix->pl_scan.p, &sbytes, len, off, pairs + 1, nullptr))
        return fail(TK_ERR_HIP, "tk_scan_exclusive64 failed");
    HIPCHECK(hipGetLastError());
    j.q = ix->br_q.as<float>();
    j.rows = ix->data.p;
    j.probes = ix->pl_probes.as<int64_t>();
    j.ids = ix->ids.as<int64_t>();
    j.ids_off = ix->ids_off.as<int64_t>();
    j.list_n = ix->list_n.as<int64_t>();
    j.twin_list = twin_list;
    j.n_lists = ix->n_lists;
    j.N = ix->N;
    j.d = ix->d;
    j.kc = kc;
    j.twin_w = twin_w;
    return TK_OK;
}

#define PE_THREADS 256
#define PE_LDS_LIMIT (64 * 1024)
#define PE_QT_MAX 64

struct PeTile {
    int QT, RB;
    int xstride;            // elements of T between two queries in LDS
    int ystride;            // bytes between two staged rows in LDS
    size_t lds;
    int DS;                 // 0: probe_dist_kernel; else a slabbed kernel (wide, matrix, f32) and the elements of its slab
};

struct PeJob : ProbeJob {
    const long long *seglen, *segoff;   // (nq * kc + 1): keys of the (query, rank), and where they begin in the call
    long long seg_base;             // segoff of the chunk's first (query, rank): its key buffer begins there
    int64_t pair0, n_pairs;         // the chunk's (query, rank)s: [pair0, pair0 + n_pairs)
    int *count, *cursor, *list_off, *ntiles, *tile_off;    // (n_lists + 1) each
    int *pair_of;                   // the chunk's pairs by list: the (query, rank) index of each
    int4 *tiles;                    // (list, first pair, count, -)
    void *keys;                     // GxKey<T>::type per candidate position
    PeTile t;
};

// ---- probe_matrix.hip, used by probe_exact.hip's driver ----
// what pm_prepare leaves per query of the call: the two half planes of 2^e x, (nq, dpad) each, |x|^2 and 2^-e
struct PmQueries {
    const _Float16 *xh, *xl;
    const float *xn, *xs;
    int dpad;                       // d rounded up to 16
};
int pm_check(const tk_index *ix, const float *q, int64_t nq);           // the refusals of matrix=True; no device work
void pm_tile(PeTile &t);                                                // the matrix pass's tile
int pm_prepare(tk_index *ix, int64_t nq, PmQueries &mx);                // the queries in br_q -> mx (workspace of ix)
void pm_launch_dist(const PeJob &j, const PmQueries &mx, unsigned max_tiles);

// ---- probe_f32.hip, used by probe_exact.hip's driver ----
// the queries are tk_launch_brute_wide_prepare's: 2 x zero-extended and |x|^2 (TkBruteWide, kernels.h)
int pf_check(const tk_index *ix);                                       // the refusals of wide=True; no device work
void pf_tile(PeTile &t);                                                // the f32 matrix pass's tile
void pf_launch_dist(const PeJob &j, const TkBruteWide &wd, unsigned max_tiles);

// ---- probe_matrix.hip and brute_matrix.hip: how both stage a half row ----
// piece c (8 halfs) of a row of d halfs, zeros behind d, in loads of U: uint4 where d % 8 == 0, uint2 where d % 4 == 0
// (d = 100), else halfs — d is a multiple of the halfs of U, so a load is whole or not made
template <typename U>
__device__ __forceinline__ uint4 pm_row_piece(const _Float16 *row, int c, int d)
{
    constexpr int NU = 16 / (int)sizeof(U), E = (int)sizeof(U) / 2;
    union {
        uint4 v;
        U u[NU];
    } p;
    p.v = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NU; i++)
        if (c * 8 + i * E < d) p.u[i] = *(const U *)(row + c * 8 + i * E);
    return p.v;
}
