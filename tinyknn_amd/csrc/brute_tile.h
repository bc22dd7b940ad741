// brute_tile.h — the tile loop of the exact search over all rows as a device template: brute_tiles_kernel's loop
// (brute.hip) with what is done with a pair's part value as a parameter.  radius.hip builds its kernels on it;
// brute.hip keeps its own text of the same loop (built on this header knn_brute measured 2 – 4 % slower, radius.hip's
// header says where), so a change to the part arithmetic has to be made in both — tests/test_radius_gpu.py compares
// the two bit for bit on data that is not integer.
//
//   part[i][j] = (|x_i|^2 + |y_j|^2) - (2 x_i) . y_j          utils.py:84
// on the f32 matrix cores (v_mfma_f32_32x32x2_f32 = the f32 FMA chain over k ascending), norms in numpy's einsum
// order (np_order.h).  One workgroup = 4 waves = 128 query rows against 32 rows of Y at a time; the Y tile (32
// consecutive rows = one contiguous block of memory) is fetched once per workgroup into LDS in MFMA operand order,
// double-buffered.  LDS: A operands [4 waves][KT][64], B tiles [2][KT][64] floats (KT = ceil(d / 2)), and behind them
// (RESTRICTED) the attributes of the workgroup's 128 queries: tile_attr_bytes.  256 threads, d <= 128.
#pragma once
#include "kernels.h"
#include "np_order.h"

typedef float tk_f32x16 __attribute__((ext_vector_type(16)));

// The attributes of a workgroup's 128 queries, staged in LDS behind the tiles (RESTRICTED), only those of the
// restrictions given: ranges [128][2 cols] int64 (lo_0, hi_0, lo_1, ...), tags [128] uint64, exclude [128] int32
// (N < 2^31), group [128] int32 — 4 to 84 bytes a query.  At d = 100 the tiles take 76 800 bytes, so two workgroups
// share a CU's 160 KB as long as a query's attributes fit 40 bytes: every form but two or more value columns.
__host__ __device__ static inline size_t tile_attr_bytes(const TkBruteRestrict &r)
{
    return (size_t)128 * (16 * r.cols + (r.tags ? 8 : 0) + (r.exclude ? 4 : 0) + (r.group ? 4 : 0));
}

// The grid of one launch over `cols` columns: enough workgroups for the chip — blockIdx.y splits the rows of Y when
// there are few query tiles, at least 32 tiles per split
static inline dim3 brute_tile_grid(int64_t nq, int64_t cols)
{
    const unsigned qt = (unsigned)((nq + 127) / 128);
    int64_t sp = (1024 + qt - 1) / qt;
    const int64_t most = (cols + 1023) / 1024;
    sp = sp < 1 ? 1 : (sp > most ? most : sp);
    return dim3(qt, (unsigned)(sp < 1 ? 1 : sp));
}
static inline size_t brute_tile_lds(int d) { return (size_t)(4 + 2) * ((d + 1) / 2) * 64 * 4; }

// the query row behind accumulator register v of this lane, clamped to the last one (rows past nq repeat it and are
// never handed on)
__device__ __forceinline__ int64_t brute_tile_query(int v, int64_t nq)
{
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 + (v & 3) + 8 * (v >> 2) +
                        4 * ((threadIdx.x & 63) >> 5);
    return row < nq ? row : nq - 1;
}

// Every (query row, column) pair of the workgroup's 128 queries against rows [0, N) of Y (blockIdx.y's share of
// them), handed to
//   hit(v, row, j, part, live, passes)
// by all 64 lanes for every accumulator register v, whatever the lane's column and row are, so that the action may
// vote across the wave.  v: the register (the lane's v-th query row), row: the query, j: the row of Y, part: the value
// above; live: the pair exists — j < N, allowed, row < nq —, else part means nothing; passes(): does the lane's row
// pass the query's restriction (its attributes from LDS; RESTRICTED only).  The lane owns one column per tile: it
// loads that row's attributes once per tile (allowed bit, group, tags, up to 4 keys: 12 registers).
template <bool RESTRICTED, class Hit>
__device__ __forceinline__ void brute_tile_loop(
    const float *__restrict__ X, int64_t nq, int d, const float *__restrict__ Y,
    const float *__restrict__ ynorm2, int64_t all_cols, const TkBruteRestrict &r, Hit hit)
{
    const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    const int64_t my_row = r0 + col < nq ? r0 + col : nq - 1;
    const int KT = (d + 1) >> 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *a = (float *)smem + (size_t)(threadIdx.x >> 6) * KT * 64;     // A operands [t][lane]
    float *bt = (float *)smem + (size_t)4 * KT * 64;                      // B tiles [2][t][lane]
    int64_t *q_ranges = (int64_t *)((float *)smem + (size_t)6 * KT * 64);
    uint64_t *q_tags = (uint64_t *)(q_ranges + 128 * 2 * r.cols);
    int32_t *q_exclude = (int32_t *)(q_tags + (r.tags ? 128 : 0));
    int32_t *q_group = q_exclude + (r.exclude ? 128 : 0);
    if constexpr (RESTRICTED) {
        // (made visible by the barrier in front of the tile loop)
        if (threadIdx.x < 128) {
            const int t = threadIdx.x;
            int64_t row = (int64_t)blockIdx.x * 128 + t;
            row = row < nq ? row : nq - 1;
            if (r.exclude) q_exclude[t] = (int32_t)r.exclude[row];
            if (r.tags) q_tags[t] = r.tags[row];
            if (r.group) q_group[t] = r.group[row];
            for (int c = 0; c < 2 * r.cols; c++) q_ranges[t * 2 * r.cols + c] = r.ranges[row * 2 * r.cols + c];
        }
    }
    for (int t = 0; t < KT; t++) {
        const int kk = 2 * t + half;
        a[t * 64 + lane] = kk < d ? 2.0f * X[my_row * d + kk] : 0.0f;
    }
    float xn[16];
#pragma unroll
    for (int v = 0; v < 16; v++) {
        int64_t row = r0 + (v & 3) + 8 * (v >> 2) + 4 * half;
        row = row < nq ? row : nq - 1;
        xn[v] = einsum_selfdot<float>(X + row * d, d);
    }
    // blockIdx.y splits the rows of Y: few queries (a recall sample) would otherwise occupy a
    // handful of CUs; appends are atomic, so the split does not change the result
    const int64_t per_y = ((all_cols + gridDim.y - 1) / gridDim.y + 31) / 32 * 32;
    const int64_t c_begin = (int64_t)blockIdx.y * per_y;
    const int64_t ncols = c_begin + per_y < all_cols ? c_begin + per_y : all_cols;
    // B tile of rows [j0, j0+32): element (t, l) = Y[j0 + (l & 31)][2t + (l >> 5)].  The 32
    // rows are contiguous in memory: thread e reads float e of the block (coalesced) and
    // drops it at its operand position.
    const int tile_f = 32 * d;
    constexpr int PER = 32 * 128 / 256;        // floats per thread and tile at d <= 128
    float stage[PER];
    auto fetch = [&](int64_t j0) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int e = u * 256 + (int)threadIdx.x;
            // rows past the range read as zeros: element e belongs to row j0 + e / d, so it is
            // in range iff e < (ncols - j0) * d
            float val = 0.0f;
            if (e < tile_f && (int64_t)e < (ncols - j0) * d) val = Y[j0 * d + e];
            stage[u] = val;
        }
    };
    // operand position of this thread's tile elements (the same for every tile)
    int dst[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int e = u * 256 + (int)threadIdx.x;
        const int jj = e / d, kk = e - jj * d;
        dst[u] = e < tile_f ? (kk >> 1) * 64 + (kk & 1) * 32 + jj : -1;
    }
    auto commit = [&](int buf) {
#pragma unroll
        for (int u = 0; u < PER; u++)
            if (dst[u] >= 0) bt[(size_t)buf * KT * 64 + dst[u]] = stage[u];
    };
    if (d & 1)      // odd d: the k = d operands of the upper half-wave are zero in both buffers
        for (int e = threadIdx.x; e < 2 * 32; e += 256)
            bt[(size_t)(e >> 5) * KT * 64 + (KT - 1) * 64 + 32 + (e & 31)] = 0.0f;
    if (c_begin < ncols) {
        fetch(c_begin);
        commit(0);
    }
    __syncthreads();
    int buf = 0;
    for (int64_t j0 = c_begin; j0 < ncols; j0 += 32, buf ^= 1) {
        const bool more = j0 + 32 < ncols;
        if (more) fetch(j0 + 32);
        const int64_t j = j0 + col;
        // this lane's row of the index and what restricts it
        int64_t rid = 0, rkey[4] = {0, 0, 0, 0};
        uint64_t rtags = 0;
        int32_t rgroup = 0;
        bool row_ok = j < ncols;
        if constexpr (RESTRICTED) {
            if (row_ok) {
                rid = j;
                if (r.allowed) row_ok = (r.allowed[rid >> 5] >> (rid & 31)) & 1u;
                if (r.group) rgroup = r.row_groups[rid];
                if (r.tags) rtags = r.row_tags[rid];
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (c < r.cols) rkey[c] = r.row_keys[c * r.n_rows + rid];
            }
        }
        // does the lane's row pass the restriction of local query ql (its attributes from LDS)?
        auto passes = [&](int ql) {
            bool ok = true;
            if (r.exclude) ok = (int32_t)rid != q_exclude[ql];
            if (r.group) {
                const int32_t g = q_group[ql];
                ok &= g < 0 || rgroup == g;
            }
            if (r.tags) {
                const uint64_t t = q_tags[ql];
                ok &= t == 0 || (r.tag_mode ? (rtags & t) == t : (rtags & t) != 0);
            }
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (c < r.cols) {
                    const int64_t *b = q_ranges + (ql * r.cols + c) * 2;
                    ok &= b[0] <= rkey[c] && rkey[c] <= b[1];
                }
            return ok;
        };
        tk_f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; v++) acc[v] = 0.0f;
        const float *bb = bt + (size_t)buf * KT * 64;
#pragma unroll 4
        for (int t = 0; t < KT; t++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t * 64 + lane], bb[t * 64 + lane], acc, 0, 0, 0);
        const float yn = row_ok ? ynorm2[j] : 0.0f;
#pragma unroll
        for (int v = 0; v < 16; v++) {
            const int ql = (v & 3) + 8 * (v >> 2) + 4 * half;
            const int64_t row = r0 + ql;
            const float part = (xn[v] + yn) - acc[v];
            hit(v, row, j, part, row_ok && row < nq, [&]() { return passes((int)(threadIdx.x >> 6) * 32 + ql); });
        }
        if (more) commit(buf ^ 1);
        __syncthreads();
    }
}
