// brute_wide.hip — the exact search over ALL rows of a float32 store on the f32 matrix cores, any d <= 4096
// (knn_brute(wide=True), tk_index_knn_brute_wide).  The sampled tau, the norms of the rows, the segments,
// the overflow retry and the selection are brute.hip's; only the tile kernel and the queries' prep kernel live here.
// The value behind every key is brute.hip's part, bit for bit:
//   part = (|x|^2 + |y|^2) - acc
//   acc  = ONE float32 accumulator of v_mfma_f32_32x32x2_f32 per (query, row): k ascending from 0 over all of d, the A
//          operand 2 * x, starting at 0 — no split-K, no second accumulator; the FMA chain of brute.hip carried on
//          across the slabs
//   |.|^2 in numpy's einsum order (np_order.h): the rows' by row_norms_kernel, the queries' by the prep kernel
// so at d <= 128 the call returns the bytes of the default call.
//   work   a workgroup of 4 waves owns BW_QT = 128 queries (blockIdx.x, fastest: co-resident workgroups walk the same
//          rows and meet in L2) and walks its share of the rows (blockIdx.y, brute_tile_grid's rule) in blocks of
//          BW_RB = 128 contiguous rows.  Wave w owns the quadrant queries 64 (w & 1) .. + 63 x rows 64 (w >> 1) .. + 63:
//          four 32 x 32 accumulators, 64 registers.  Queries are the A operand, rows the B operand: a lane's column is
//          a row.  A k-pair is 4 independent MFMAs from 4 operand reads of 4 bytes (2 of the queries, 2 of the rows).
//   LDS    d is walked in slabs of BW_DS = 32 floats (16 k-pairs).  LDS holds one slab of the block's rows and one of
//          the tile's queries, row-major, BW_STRIDE = 33 floats apart: an odd number, so the 32 rows a half-wave reads
//          at one k lie in 32 different banks.  Slab tails and rows past the range are zeros: fma(0, 0, acc) = acc.
//          Behind them xn and tau of the tile's queries.  Static: 2 * 128 * 33 * 4 + 1 024 = 34 816 bytes; RESTRICTED
//          adds the queries' attributes, tile_attr_bytes' arrays at their largest and each at a fixed place, 10 240
//          bytes: 45 056.  Two workgroups a CU either way.  (BW_DS = 64 at an odd stride is 66 560 bytes of slabs: past
//          the 64 KiB a workgroup gets without asking.)
//          The next (block, slab) step's global loads sit in registers while this slab is multiplied (bm_walk's loop);
//          where d fits one slab the queries are staged once per workgroup.
//   end    brute_matrix.hip's: MODE 0 (the strided sample) writes part, or +inf where the pair fails its restriction,
//          to vals.  MODE 1 tests part <= tau first, then the restriction, and appends brute_select_kernel's key with
//          one atomicAdd on the query's counter.  A lane loads yn and the allowed bit of its two columns once per
//          block; a row's group, tags and keys are read where a pair within tau asks for them.
#include "kernels.h"
#include "np_order.h"
#include "brute_tile.h"

#define BW_THREADS 256
#define BW_QT 128
#define BW_RB 128
#define BW_DS 32                            // floats of a slab
#define BW_UR (BW_DS / 4)                   // 16-byte pieces of a slab of one row
#define BW_STRIDE (BW_DS + 1)               // floats between two staged rows
#define BW_NP (BW_RB * BW_UR / BW_THREADS)  // pieces a lane stages of the rows; of the queries as many
#define BW_ATTR (128 * (16 * 4 + 8 + 4 + 4))    // tile_attr_bytes at its largest: 4 value columns, tags, exclude, group
static_assert(BW_DS % 8 == 0 && BW_STRIDE % 2 == 1, "whole groups of 4 k-pairs; an odd stride in floats");
static_assert(BW_NP * BW_THREADS == BW_RB * BW_UR && BW_QT == BW_RB && BW_QT == 128, "whole pieces a lane; tile_attr_bytes' 128 queries");
static_assert((2 * BW_RB * BW_STRIDE + 2 * BW_QT) * 4 + BW_ATTR <= 64 * 1024, "static LDS");

template <bool RESTRICTED>
struct BwLds {
    float x[BW_QT * BW_STRIDE];                     // the tile's slab of 2 x
    float y[BW_RB * BW_STRIDE];                     // the block's slab of the rows
    float xn[BW_QT], tau[BW_QT];                    // what the epilogue reads of the tile's queries
    unsigned char attr[RESTRICTED ? BW_ATTR : 0];   // the queries' attributes (tile_attr_bytes)
};

struct BwJob {
    TkBruteWide wd;
    int64_t nq;
    int d;
    const float *Y;                 // rows [0, cols) of this launch
    const float *ynorm2;            // their norms
    int64_t cols;
    float *vals;                    // MODE 0: (nq, cols)
    const float *tau;               // MODE 1
    unsigned long long *cand;
    int cap;
    int *count;
    int64_t j_base, j_stride;       // column j is row j_base + j * j_stride of the index
    TkBruteRestrict r;
};

// The queries once per call: 2 x (exact) zero-extended to dq floats a row, a whole number of 16-byte pieces, and |x|^2
// in numpy's einsum order
__global__ void brute_wide_prepare_kernel(const float *__restrict__ X, int64_t nq, int d, int dq, float *__restrict__ x2,
                                          float *__restrict__ xn)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) xn[i] = einsum_selfdot<float>(X + i * d, d);
    if (i >= nq * dq) return;
    const int64_t q = i / dq;
    const int k = (int)(i - q * dq);
    x2[i] = k < d ? 2.0f * X[q * d + k] : 0.0f;
}

template <int MODE, bool RESTRICTED, typename U>
__device__ __forceinline__ void bw_walk(const BwJob &j, BwLds<RESTRICTED> &s)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = j.d, dq = j.wd.dq;
    const TkBruteRestrict &r = j.r;
    const int64_t q0 = (int64_t)blockIdx.x * BW_QT;
    const int NS = (d + BW_DS - 1) / BW_DS;                             // slabs
    // blockIdx.y's share of the columns, in whole blocks
    const int64_t per_y = ((j.cols + gridDim.y - 1) / gridDim.y + BW_RB - 1) / BW_RB * BW_RB;
    const int64_t c_begin = (int64_t)blockIdx.y * per_y;
    const int64_t ncols = c_begin + per_y < j.cols ? c_begin + per_y : j.cols;
    if (c_begin >= ncols) return;                                       // (the whole workgroup)
    const int64_t steps = (ncols - c_begin + BW_RB - 1) / BW_RB * NS;

    // what waits in LDS for the epilogue: xn and tau, and the attributes behind them (the arrays of tile_attr_bytes at
    // their largest, each at a fixed place: ranges [128][4 cols][2] int64, tags [128] uint64, exclude [128] int32,
    // group [128] int32).  Made visible by the barriers in front of the first slab
    int64_t *q_ranges = (int64_t *)s.attr;
    uint64_t *q_tags = (uint64_t *)(q_ranges + BW_QT * 8);
    int32_t *q_exclude = (int32_t *)(q_tags + BW_QT);
    int32_t *q_group = q_exclude + BW_QT;
    if (tid < BW_QT) {
        int64_t row = q0 + tid;
        row = row < j.nq ? row : j.nq - 1;
        s.xn[tid] = j.wd.xn[row];
        s.tau[tid] = MODE == 1 ? j.tau[row] : 0.0f;
        if constexpr (RESTRICTED) {
            if (r.exclude) q_exclude[tid] = (int32_t)r.exclude[row];
            if (r.tags) q_tags[tid] = r.tags[row];
            if (r.group) q_group[tid] = r.group[row];
            for (int c = 0; c < 2 * r.cols; c++) q_ranges[tid * 8 + c] = r.ranges[row * 2 * r.cols + c];
        }
    }

    // a lane's pieces: row (or query) tid / 8 + 32 p of the block, piece tid % 8 of the slab
    uint4 ry[BW_NP], rx[BW_NP];
    const int er = tid / BW_UR, ec = tid % BW_UR;
    const int qleft = (int)(j.nq - q0 < BW_QT ? j.nq - q0 : BW_QT);    // queries of the tile
    auto fetch_rows = [&](int64_t step) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
        const int64_t first = c_begin + b * BW_RB;
        const int left = (int)(ncols - first < BW_RB ? ncols - first : BW_RB);
        const float *yb = j.Y + (first + er) * d;
#pragma unroll
        for (int p = 0; p < BW_NP; p++)
            ry[p] = er + 32 * p < left ? bw_row_piece<U>(yb + (int64_t)(32 * p) * d, sl * BW_UR + ec, d)
                                       : make_uint4(0, 0, 0, 0);
    };
    auto fetch_queries = [&](int sl) {
        const int c = sl * BW_UR + ec;
        const float *xb = j.wd.x2 + (q0 + er) * dq + c * 4;
#pragma unroll
        for (int p = 0; p < BW_NP; p++)
            rx[p] = (er + 32 * p < qleft && c * 4 < dq) ? *(const uint4 *)(xb + (int64_t)(32 * p) * dq)
                                                        : make_uint4(0, 0, 0, 0);
    };
    auto put = [&](float *slab, int p, const uint4 &v) {
        float *at = slab + (er + 32 * p) * BW_STRIDE + ec * 4;
        at[0] = __uint_as_float(v.x);
        at[1] = __uint_as_float(v.y);
        at[2] = __uint_as_float(v.z);
        at[3] = __uint_as_float(v.w);
    };
    auto commit = [&](bool queries) {
#pragma unroll
        for (int p = 0; p < BW_NP; p++) put(s.y, p, ry[p]);
        if (queries) {
#pragma unroll
            for (int p = 0; p < BW_NP; p++) put(s.x, p, rx[p]);
        }
    };
    fetch_rows(0);
    fetch_queries(0);

    const int qh = wave & 1, rh = wave >> 1;        // the wave's quadrant
    // the lane's operands of k-pair t: k = 2 t + (lane >> 5) of query / row lane & 31 (and 32 further)
    const float *pa = s.x + (64 * qh + (lane & 31)) * BW_STRIDE + (lane >> 5);
    const float *pb = s.y + (64 * rh + (lane & 31)) * BW_STRIDE + (lane >> 5);
    tk_f32x16 acc[2][2];                            // [query half][row half]
    // the lane's two columns of the block: the row's norm and what restricts it
    float yn[2] = {0.0f, 0.0f};
    bool row_ok[2] = {false, false};
    int32_t rid[2] = {0, 0};                        // (N < 2^31)
    for (int64_t step = 0; step < steps; step++) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
        __syncthreads();                            // the last step's arithmetic is done with the slabs
        commit(NS > 1 || step == 0);
        __syncthreads();
        if (step + 1 < steps) {
            fetch_rows(step + 1);
            if (NS > 1) fetch_queries((int)((step + 1) % NS));
        }
        if (sl == 0) {
#pragma unroll
            for (int v = 0; v < 16; v++) acc[0][0][v] = acc[0][1][v] = acc[1][0][v] = acc[1][1][v] = 0.0f;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int64_t col = c_begin + b * BW_RB + 64 * rh + 32 * h + (lane & 31);
                row_ok[h] = col < ncols;
                yn[h] = row_ok[h] ? j.ynorm2[col] : 0.0f;
                if constexpr (RESTRICTED) {
                    if (row_ok[h]) {
                        const int64_t id = j.j_base + col * j.j_stride;
                        rid[h] = (int32_t)id;
                        if (r.allowed) row_ok[h] = (r.allowed[id >> 5] >> (id & 31)) & 1u;
                    }
                }
            }
        }
        // the slab's k-pairs in groups of 4 (the tail of the last group is zeros): 2 x . y into the four accumulators
        int nk = d - sl * BW_DS;
        nk = nk < BW_DS ? nk : BW_DS;
        const int ng = (nk + 7) / 8;
#pragma unroll 1
        for (int g = 0; g < ng; g++) {
#pragma unroll
            for (int t = 4 * g; t < 4 * g + 4; t++) {
                const float a0 = pa[2 * t], a1 = pa[32 * BW_STRIDE + 2 * t];
                const float b0 = pb[2 * t], b1 = pb[32 * BW_STRIDE + 2 * t];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if (sl != NS - 1) continue;
        // does the lane's column h pass the restriction of local query u?  The query's attributes come from LDS, the
        // row's group, tags and keys from memory: only the pairs within tau ask (MODE 0: the sample's)
        auto passes = [&](int u, int h) {
            const int64_t id = rid[h];
            bool ok = true;
            if (r.exclude) ok = rid[h] != q_exclude[u];
            if (r.group) {
                const int32_t g = q_group[u];
                ok &= g < 0 || r.row_groups[id] == g;
            }
            if (r.tags) {
                const uint64_t t = q_tags[u], rt = r.row_tags[id];
                ok &= t == 0 || (r.tag_mode ? (rt & t) == t : (rt & t) != 0);
            }
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (c < r.cols) {
                    const int64_t *bd = q_ranges + u * 8 + c * 2, key = r.row_keys[c * r.n_rows + id];
                    ok &= bd[0] <= key && key <= bd[1];
                }
            return ok;
        };
        const int64_t col0 = c_begin + b * BW_RB + 64 * rh + (lane & 31);
        // the lane's first query; accumulator register v of query half a adds the same ku = 32 a + 8 (v / 4) + v % 4 in
        // every lane: what a pair addresses is a base that is the same in every lane plus a 32-bit offset of the lane
        // (MODE 0: cols = ns <= 8192; MODE 1: 128 * cap entries), so no 64-bit address is kept per register
        int ul = 64 * qh + 4 * (lane >> 5);
        // (opaque to the optimiser, as in bm_walk: it would otherwise keep what every register's query addresses alive
        // across the whole walk)
        asm volatile("" : "+v"(ul));
        const unsigned vo = (unsigned)ul * (unsigned)j.cols + (unsigned)col0;
        const unsigned ko = (unsigned)ul * (unsigned)j.cap;
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int vg = 0; vg < 4; vg++) {
                // the four queries v & 3 of this group: one 16-byte read each of their xn and tau
                const int u0 = ul + 32 * a + 8 * vg;
                const float4 gxn = *(const float4 *)(s.xn + u0), gtau = *(const float4 *)(s.tau + u0);
                const float qxn[4] = {gxn.x, gxn.y, gxn.z, gxn.w}, qtau[4] = {gtau.x, gtau.y, gtau.z, gtau.w};
#pragma unroll
                for (int vi = 0; vi < 4; vi++) {
                    const int v = 4 * vg + vi, ku = 32 * a + 8 * vg + vi, u = ul + ku;
                    if (u >= qleft) continue;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const float part = (qxn[vi] + yn[h]) - acc[a][h][v];
                        if (MODE == 0) {
                            if (col0 + 32 * h >= ncols) continue;
                            float val = part;
                            if constexpr (RESTRICTED)
                                if (!row_ok[h] || !passes(u, h)) val = __builtin_inff();
                            (j.vals + (q0 + ku) * j.cols)[vo + 32 * h] = val;
                        } else if (row_ok[h] && part <= qtau[vi] && (!RESTRICTED || passes(u, h))) {
                            const int pos = atomicAdd(&(j.count + (q0 + ku))[(unsigned)ul], 1);
                            if (pos < j.cap) {
                                // brute_select_kernel's key: float bits made monotone, then the index
                                uint32_t k32 = __float_as_uint(part);
                                k32 = (k32 & 0x80000000u) ? ~k32 : (k32 | 0x80000000u);
                                (j.cand + (q0 + ku) * j.cap)[ko + (unsigned)pos] =
                                    ((unsigned long long)k32 << 32) | (uint32_t)(j.j_base + col0 + 32 * h);
                            }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);          // (the reads of the next group stay behind this one)
            }
    }
}

template <int MODE, bool RESTRICTED>
__global__ __launch_bounds__(BW_THREADS, 2) void brute_wide_tiles_kernel(const BwJob j)
{
    __shared__ __attribute__((aligned(16))) BwLds<RESTRICTED> s;
    if (j.d % 4 == 0) bw_walk<MODE, RESTRICTED, uint4>(j, s);
    else if (j.d % 2 == 0) bw_walk<MODE, RESTRICTED, uint2>(j, s);
    else bw_walk<MODE, RESTRICTED, float>(j, s);
}

// ---- what brute.hip's two halves and api_exact.hip call where the search is the wide one (wd != NULL) ----

// X (nq, d) -> x2 (nq, tk_brute_wide_dq(d)) and xn (nq)
void tk_launch_brute_wide_prepare(const float *X, int64_t nq, int d, float *x2, float *xn, hipStream_t s)
{
    const int dq = tk_brute_wide_dq(d);
    if (nq == 0) return;
    hipLaunchKernelGGL(brute_wide_prepare_kernel, dim3((unsigned)((nq * dq + 255) / 256)), dim3(256), 0, s, X, nq, d, dq,
                       x2, xn);
}

// One launch of the tile kernel over `cols` columns, as brute.hip's brute_tiles: mode 0 / 1, the grid by
// brute_tile_grid's rule, the restricted form where r is given
void tk_launch_brute_wide_tiles(int mode, const TkBruteWide &wd, int64_t nq, int d, const float *Y,
                                const float *ynorm2, int64_t cols, float *vals, const float *tau,
                                unsigned long long *cand, int cap, int *count, int64_t j_base, int64_t j_stride,
                                const TkBruteRestrict *r, hipStream_t s)
{
    const BwJob j{wd, nq, d, Y, ynorm2, cols, vals, tau, cand, cap, count, j_base, j_stride, r ? *r : TkBruteRestrict{}};
    const dim3 grid = brute_tile_grid(nq, cols);
    if (mode == 0 && r) hipLaunchKernelGGL((brute_wide_tiles_kernel<0, true>), grid, dim3(BW_THREADS), 0, s, j);
    else if (mode == 0) hipLaunchKernelGGL((brute_wide_tiles_kernel<0, false>), grid, dim3(BW_THREADS), 0, s, j);
    else if (r) hipLaunchKernelGGL((brute_wide_tiles_kernel<1, true>), grid, dim3(BW_THREADS), 0, s, j);
    else hipLaunchKernelGGL((brute_wide_tiles_kernel<1, false>), grid, dim3(BW_THREADS), 0, s, j);
}
