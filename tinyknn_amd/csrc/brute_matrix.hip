// brute_matrix.hip — the exact search over ALL rows of a half store on the f16 matrix cores, any d <= 4096
// (knn_brute(matrix=True), tk_index_knn_brute_matrix).  The sampled tau, the segments, the overflow retry
// and the selection are brute.hip's (brute_select_kernel); the queries are prepared by probe_matrix.hip (pm_prepare:
// the planes x_hi and x_lo of 2^e x, |x|^2, 2^-e); only the tile kernel and two small half kernels live here.  The value
// behind every key is §3.22's dist_m, bit for bit:
//   dist_m = max(0, (xn + yn) - 2 * (acc * 2^-e))
//   acc    = ONE float32 accumulator of v_mfma_f32_32x32x16_f16 per (query, row): K steps of 16 ascending over dpad,
//            in each step the x_hi product before the x_lo product — no split-K, no second accumulator
//   yn     = the float32 self-dot of float(y) in numpy's einsum order, once per call into ynorm2 (brute_half_norms_kernel)
// so knn_brute(matrix=True) and knn_probe(matrix=True) with every list probed return the same bytes.
//   work   a workgroup of 4 waves owns BM_QT = 128 queries (blockIdx.x, fastest: co-resident workgroups walk the same
//          rows and meet in L2) and walks its share of the rows (blockIdx.y, brute_tile_grid's rule) in blocks of
//          BM_RB = 128 — one contiguous piece of memory, no labels, no gather.  The rows are read ceil(nq / 128) times.
//          Wave w owns the quadrant queries 64 (w & 1) .. + 63 x rows 64 (w >> 1) .. + 63: four 32 x 32 accumulators,
//          64 registers.  Queries are the A operand, rows the B operand: a lane's column is a row.  A K step is 8 MFMAs
//          (hi, lo) x 2 query halves x 2 row halves from 6 operand reads of 16 bytes (4 of the planes, 2 of the rows);
//          the four hi products are issued before the four lo products, so no MFMA waits for the one before it.
//   LDS    d is walked in slabs of BM_DS = 64 halfs (4 K steps).  LDS holds one slab of the block's rows and of the
//          tile's two planes, BM_STRIDE = 144 bytes apart: 9 pieces of 16 bytes, an odd number (§3.21's bank rule).
//          The 16 bytes behind the x_hi slabs of queries 4g, 4g + 1 and 4g + 2 hold xn, 2^-e and tau of the queries
//          4g .. 4g + 3: the epilogue reads them with three 16-byte reads per four accumulator registers.  Static: 384 * 144 = 55 296 bytes; RESTRICTED adds the queries' attributes, tile_attr_bytes'
//          arrays at their largest and each at a fixed place, 10 240 bytes: 65 536, the 64 KiB a workgroup gets without asking.  Two workgroups a
//          CU either way.  DS = 112 as in §3.22 would take 92 160 bytes: one workgroup a CU.
//          The next (block, slab) step's global loads sit in registers while this slab is multiplied (pm_walk's
//          loop); where d fits one slab the planes are staged once per workgroup.
//   end    MODE 0 (the strided sample, copied contiguously by brute_half_sample_kernel) writes dist_m, or +inf where the
//          pair fails its restriction, to vals.  MODE 1 tests dist_m <= tau first, then the restriction, and appends
//          brute_select_kernel's key with one atomicAdd on the query's counter: a failing row takes no slot and never
//          tightens tau.  A lane loads yn and the allowed bit of its two columns once per block; a row's group, tags and
//          keys are read where a pair within tau asks for them.
#include "probe_job.h"
#include "np_order.h"
#include "brute_tile.h"

#define BM_THREADS 256
#define BM_QT 128
#define BM_RB 128
#define BM_DS 64                            // halfs of a slab
#define BM_UR (BM_DS / 8)                   // 16-byte pieces of a slab of one row
#define BM_STRIDE (BM_DS * 2 + 16)          // bytes between two staged rows: 9 pieces
#define BM_NP (BM_RB * BM_UR / BM_THREADS)  // pieces a lane stages of the rows; of the two planes twice as many
#define BM_ATTR (128 * (16 * 4 + 8 + 4 + 4))    // tile_attr_bytes at its largest: 4 value columns, tags, exclude, group
static_assert(BM_DS % 16 == 0 && (BM_STRIDE / 16) % 2 == 1, "whole K steps; an odd stride in pieces");
static_assert(BM_NP * BM_THREADS == BM_RB * BM_UR && BM_QT == BM_RB && BM_QT == 128, "whole pieces a lane; tile_attr_bytes' 128 queries");
static_assert(3 * BM_RB * BM_STRIDE + BM_ATTR <= 64 * 1024, "static LDS");

typedef _Float16 bm_half8 __attribute__((ext_vector_type(8)));
typedef float bm_float16 __attribute__((ext_vector_type(16)));

template <bool RESTRICTED>
struct BmLds {
    unsigned char xh[BM_QT * BM_STRIDE], xl[BM_QT * BM_STRIDE];     // the tile's slab of x_hi (+ xn, 2^-e, tau) and x_lo
    unsigned char yr[BM_RB * BM_STRIDE];                            // the block's slab of the rows
    unsigned char attr[RESTRICTED ? BM_ATTR : 0];                   // the queries' attributes (tile_attr_bytes)
};

struct BmJob {
    TkBruteMatrix mx;
    int64_t nq;
    int d;
    const _Float16 *Y;              // rows [0, cols) of this launch
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

// |float(y_j)|^2 in numpy's einsum order: probe_dist_matrix_kernel's yn
__global__ void brute_half_norms_kernel(const _Float16 *__restrict__ Y, int64_t n, int d, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const _Float16 *y = Y + i * d;
    out[i] = einsum_selfdot_fn<float>([&](int k) { return (float)y[k]; }, d);
}

// `ns` rows of Y at stride N / ns (row i * stride) -> a contiguous sample
__global__ void brute_half_sample_kernel(const _Float16 *__restrict__ Y, int d, int64_t ns, int64_t stride,
                                         _Float16 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns * d) return;
    const int64_t r = i / d;
    out[i] = Y[r * stride * d + (i - r * d)];
}

template <int MODE, bool RESTRICTED, typename U>
__device__ __forceinline__ void bm_walk(const BmJob &j, BmLds<RESTRICTED> &s)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = j.d, dpad = j.mx.dpad;
    const TkBruteRestrict &r = j.r;
    const int64_t q0 = (int64_t)blockIdx.x * BM_QT;
    const int up = dpad / 8;                                            // pieces of a whole plane row
    const int NS = (d + BM_DS - 1) / BM_DS;                             // slabs
    // blockIdx.y's share of the columns, in whole blocks
    const int64_t per_y = ((j.cols + gridDim.y - 1) / gridDim.y + BM_RB - 1) / BM_RB * BM_RB;
    const int64_t c_begin = (int64_t)blockIdx.y * per_y;
    const int64_t ncols = c_begin + per_y < j.cols ? c_begin + per_y : j.cols;
    if (c_begin >= ncols) return;                                       // (the whole workgroup)
    const int64_t steps = (ncols - c_begin + BM_RB - 1) / BM_RB * NS;

    // what waits in LDS for the epilogue: (xn, 2^-e, tau) behind each query's x_hi slab, the attributes behind the tiles
    // (the arrays of tile_attr_bytes at their largest, each at a fixed place: ranges [128][4 cols][2] int64, tags [128]
    // uint64, exclude [128] int32, group [128] int32 — every address is the lane's plus a constant)
    int64_t *q_ranges = (int64_t *)s.attr;
    uint64_t *q_tags = (uint64_t *)(q_ranges + BM_QT * 8);
    int32_t *q_exclude = (int32_t *)(q_tags + BM_QT);
    int32_t *q_group = q_exclude + BM_QT;
    if (tid < BM_QT) {
        int64_t row = q0 + tid;
        row = row < j.nq ? row : j.nq - 1;
        float *pad = (float *)(s.xh + (tid & ~3) * BM_STRIDE + BM_DS * 2) + (tid & 3);
        pad[0] = j.mx.xn[row];
        pad[BM_STRIDE / 4] = j.mx.xs[row];
        pad[2 * BM_STRIDE / 4] = MODE == 1 ? j.tau[row] : 0.0f;
        if constexpr (RESTRICTED) {
            if (r.exclude) q_exclude[tid] = (int32_t)r.exclude[row];
            if (r.tags) q_tags[tid] = r.tags[row];
            if (r.group) q_group[tid] = r.group[row];
            for (int c = 0; c < 2 * r.cols; c++) q_ranges[tid * 8 + c] = r.ranges[row * 2 * r.cols + c];
        }
    }

    // a lane's pieces: row (or query) tid / 8 + 32 p of the block, piece tid % 8 of the slab — one lane-varying base
    // each, the rest is the same in every lane
    uint4 ry[BM_NP], rx[2 * BM_NP];
    const int er = tid / BM_UR, ec = tid % BM_UR;
    const int qleft = (int)(j.nq - q0 < BM_QT ? j.nq - q0 : BM_QT);    // queries of the tile
    auto fetch_rows = [&](int64_t step) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
        const int64_t first = c_begin + b * BM_RB;
        const int left = (int)(ncols - first < BM_RB ? ncols - first : BM_RB);
        const _Float16 *yb = j.Y + (first + er) * d;
#pragma unroll
        for (int p = 0; p < BM_NP; p++)
            ry[p] = er + 32 * p < left ? pm_row_piece<U>(yb + (int64_t)(32 * p) * d, sl * BM_UR + ec, d)
                                       : make_uint4(0, 0, 0, 0);
    };
    auto fetch_queries = [&](int sl) {              // entries 0 .. BM_QT - 1: x_hi, then x_lo
        const int c = sl * BM_UR + ec;
        const int64_t at = (q0 + er) * dpad + c * 8;
#pragma unroll
        for (int p = 0; p < 2 * BM_NP; p++) {
            const _Float16 *plane = (const _Float16 *)(p < BM_NP ? j.mx.xh : j.mx.xl) + (int64_t)(32 * (p % BM_NP)) * dpad;
            rx[p] = (er + 32 * (p % BM_NP) < qleft && c < up) ? *(const uint4 *)(plane + at) : make_uint4(0, 0, 0, 0);
        }
    };
    auto commit = [&](bool queries) {
#pragma unroll
        for (int p = 0; p < BM_NP; p++) {
            const int e = tid + p * BM_THREADS;
            ((uint4 *)(s.yr + (e / BM_UR) * BM_STRIDE))[e % BM_UR] = ry[p];
        }
        if (queries) {
#pragma unroll
            for (int p = 0; p < 2 * BM_NP; p++) {
                const int e = tid + p * BM_THREADS, rr = e / BM_UR;
                ((uint4 *)((rr < BM_QT ? s.xh : s.xl) + (rr & (BM_QT - 1)) * BM_STRIDE))[e % BM_UR] = rx[p];
            }
        }
    };
    fetch_rows(0);
    fetch_queries(0);

    const int qh = wave & 1, rh = wave >> 1;        // the wave's quadrant
    const int koff = (lane >> 5) * 16;              // the lane's 8 halfs of a K step
    const unsigned char *pb = s.yr + (64 * rh + (lane & 31)) * BM_STRIDE + koff;
    const unsigned char *ph = s.xh + (64 * qh + (lane & 31)) * BM_STRIDE + koff;
    const unsigned char *pl = s.xl + (64 * qh + (lane & 31)) * BM_STRIDE + koff;
    bm_float16 acc[2][2];                           // [query half][row half]
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
                const int64_t col = c_begin + b * BM_RB + 64 * rh + 32 * h + (lane & 31);
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
        // the slab's K steps: (x_hi + x_lo) . y into the four accumulators, hi before lo in each
        int nk = (dpad - sl * BM_DS) / 16;
        nk = nk < BM_DS / 16 ? nk : BM_DS / 16;
#pragma unroll 1
        for (int ks = 0; ks < nk; ks++) {
            const bm_half8 b0 = *(const bm_half8 *)(pb + ks * 32), b1 = *(const bm_half8 *)(pb + 32 * BM_STRIDE + ks * 32);
            const bm_half8 h0 = *(const bm_half8 *)(ph + ks * 32), h1 = *(const bm_half8 *)(ph + 32 * BM_STRIDE + ks * 32);
            const bm_half8 l0 = *(const bm_half8 *)(pl + ks * 32), l1 = *(const bm_half8 *)(pl + 32 * BM_STRIDE + ks * 32);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h1, b1, acc[1][1], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l1, b1, acc[1][1], 0, 0, 0);
        }
        if (sl != NS - 1) continue;
        // does the lane's column h pass the restriction of local query u?  The query's attributes come from LDS, the
        // row's group, tags and keys from memory: only the pairs within tau ask (MODE 0: the sample's), and 26
        // registers for the attributes of two columns did not fit beside the accumulators at two workgroups a CU
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
        const int64_t col0 = c_begin + b * BM_RB + 64 * rh + (lane & 31);
        // the lane's first query; accumulator register v of query half a adds the same ku = 32 a + 8 (v / 4) + v % 4 in
        // every lane: what a pair addresses is a base that is the same in every lane plus a 32-bit offset of the lane
        // (MODE 0: cols = ns <= 8192; MODE 1: 128 * cap entries), so no 64-bit address is kept per register
        int ul = 64 * qh + 4 * (lane >> 5);
        // (opaque to the optimiser: it would otherwise keep what every register's query addresses — LDS offsets, the
        // u < qleft masks — alive across the whole walk, 60 registers and more, in scratch at two workgroups a CU)
        asm volatile("" : "+v"(ul));
        const unsigned vo = (unsigned)ul * (unsigned)j.cols + (unsigned)col0;
        const unsigned ko = (unsigned)ul * (unsigned)j.cap;
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int vg = 0; vg < 4; vg++) {
                // the four queries v & 3 of this group: one 16-byte read each of their xn, 2^-e and tau
                const int u0 = ul + 32 * a + 8 * vg;
                const unsigned char *pad = s.xh + u0 * BM_STRIDE + BM_DS * 2;
                const float4 gxn = *(const float4 *)pad, gxs = *(const float4 *)(pad + BM_STRIDE),
                             gtau = *(const float4 *)(pad + 2 * BM_STRIDE);
                const float qxn[4] = {gxn.x, gxn.y, gxn.z, gxn.w}, qxs[4] = {gxs.x, gxs.y, gxs.z, gxs.w},
                            qtau[4] = {gtau.x, gtau.y, gtau.z, gtau.w};
#pragma unroll
                for (int vi = 0; vi < 4; vi++) {
                    const int v = 4 * vg + vi, ku = 32 * a + 8 * vg + vi, u = ul + ku;
                    if (u >= qleft) continue;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const float dot = acc[a][h][v] * qxs[vi];
                        const float rr = (qxn[vi] + yn[h]) - 2.0f * dot;
                        const float dm = rr > 0.0f ? rr : 0.0f;
                        if (MODE == 0) {
                            if (col0 + 32 * h >= ncols) continue;
                            float val = dm;
                            if constexpr (RESTRICTED)
                                if (!row_ok[h] || !passes(u, h)) val = __builtin_inff();
                            (j.vals + (q0 + ku) * j.cols)[vo + 32 * h] = val;
                        } else if (row_ok[h] && dm <= qtau[vi] && (!RESTRICTED || passes(u, h))) {
                            const int pos = atomicAdd(&(j.count + (q0 + ku))[(unsigned)ul], 1);
                            if (pos < j.cap) {
                                // brute_select_kernel's key: float bits made monotone, then the index
                                uint32_t k32 = __float_as_uint(dm);
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
__global__ __launch_bounds__(BM_THREADS, 2) void brute_matrix_tiles_kernel(const BmJob j)
{
    __shared__ __attribute__((aligned(16))) BmLds<RESTRICTED> s;
    if (j.d % 8 == 0) bm_walk<MODE, RESTRICTED, uint4>(j, s);
    else if (j.d % 4 == 0) bm_walk<MODE, RESTRICTED, uint2>(j, s);
    else bm_walk<MODE, RESTRICTED, _Float16>(j, s);
}

// ---- what brute.hip's two halves call where the rows are half (mx != NULL) ----

void tk_launch_brute_half_norms(const void *Y, int64_t n, int d, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(brute_half_norms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const _Float16 *)Y, n,
                       d, out);
}

void tk_launch_brute_half_sample(const void *Y, int d, int64_t ns, int64_t stride, void *out, hipStream_t s)
{
    hipLaunchKernelGGL(brute_half_sample_kernel, dim3((unsigned)((ns * d + 255) / 256)), dim3(256), 0, s,
                       (const _Float16 *)Y, d, ns, stride, (_Float16 *)out);
}

// One launch of the tile kernel over `cols` columns, as brute.hip's brute_tiles: mode 0 / 1, the grid by
// brute_tile_grid's rule, the restricted form where r is given
void tk_launch_brute_matrix_tiles(int mode, const TkBruteMatrix &mx, int64_t nq, int d, const void *Y,
                                  const float *ynorm2, int64_t cols, float *vals, const float *tau,
                                  unsigned long long *cand, int cap, int *count, int64_t j_base, int64_t j_stride,
                                  const TkBruteRestrict *r, hipStream_t s)
{
    const BmJob j{mx, nq, d, (const _Float16 *)Y, ynorm2, cols, vals, tau, cand, cap, count, j_base, j_stride,
                  r ? *r : TkBruteRestrict{}};
    const dim3 grid = brute_tile_grid(nq, cols);
    if (mode == 0 && r) hipLaunchKernelGGL((brute_matrix_tiles_kernel<0, true>), grid, dim3(BM_THREADS), 0, s, j);
    else if (mode == 0) hipLaunchKernelGGL((brute_matrix_tiles_kernel<0, false>), grid, dim3(BM_THREADS), 0, s, j);
    else if (r) hipLaunchKernelGGL((brute_matrix_tiles_kernel<1, true>), grid, dim3(BM_THREADS), 0, s, j);
    else hipLaunchKernelGGL((brute_matrix_tiles_kernel<1, false>), grid, dim3(BM_THREADS), 0, s, j);
}
