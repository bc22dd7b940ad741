// probe_job.h — what the two distance passes of knn_probe share (probe_exact.hip: the exact pass, the tables, the
// selection and the host driver; probe_matrix.hip: the f16 matrix-core pass of matrix=True).
#pragma once
#include "api_internal.h"

#define PE_THREADS 256
#define PE_LDS_LIMIT (64 * 1024)
#define PE_QT_MAX 64

struct PeTile {
    int QT, RB;
    int xstride;            // elements of T between two queries in LDS
    int ystride;            // bytes between two staged rows in LDS
    size_t lds;
    int DS;                 // 0: probe_dist_kernel; else probe_dist_wide_kernel and the elements of its slab
};

struct PeJob {
    const float *q;                 // (nq, d) prepared queries of the whole call
    const void *rows;               // the vectors, TY
    const int64_t *probes;          // (nq, kc)
    const int64_t *ids, *ids_off, *list_n;
    const int32_t *twin_list;       // twins.hip, twin_w > 0
    const long long *seglen, *segoff;   // (nq * kc + 1): keys of the (query, rank), and where they begin in the call
    long long seg_base;             // segoff of the chunk's first (query, rank): its key buffer begins there
    int64_t pair0, n_pairs;         // the chunk's (query, rank)s: [pair0, pair0 + n_pairs)
    int *count, *cursor, *list_off, *ntiles, *tile_off;    // (n_lists + 1) each
    int *pair_of;                   // the chunk's pairs by list: the (query, rank) index of each
    int4 *tiles;                    // (list, first pair, count, -)
    void *keys;                     // GxKey<T>::type per candidate position
    int64_t n_lists, N;
    int d, kc, twin_w;
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
