// probe_matrix.hip — knn_probe's distance pass on the f16 matrix cores for half-stored vectors (IVF.knn_probe(matrix=True),
// tk_index_knn_probe_matrix).  Probes, segments, pairs, tiles, keys and the selection are probe_exact.hip's
// (§3.21), through its driver; only the distance behind each key differs.  For a prepared query x (float32) and a stored
// row y (half, read as exact reals):
//   dist_m = max(0, (xn + yn) - 2 * dot)   in float32
//   xn, yn = the float32 self-dots of x and of float(y) in numpy's einsum order (np_order.h, einsum_selfdot)
//   dot    = 2^-e * sum_t (x_hi,t + x_lo,t) * y_t, accumulated in float32 by v_mfma_f32_32x32x16_f16
//   x_hi   = half(2^e x),  x_lo = half(2^e x - float(x_hi))
// e puts the query's largest component into [2^14, 2^15) (0 for a zero query; at most 126): x_hi cannot overflow, a
// product of two halfs is exact in float32, scaling by 2^e is exact.  What is lost is float32 accumulation rounding and
// 2^-22 of the query; on data whose sums are exact in float32 nothing is, and the keys equal probe_dist_kernel's.
//   prepare   pm_prepare_kernel: a wave per query of the call.  The largest |x_t| (a wave reduction) gives e; the lanes
//             write the planes x_hi and x_lo, (nq, dpad) halfs each with dpad = d rounded up to 16 and zeros behind d;
//             lanes 0..3 walk the four accumulator chains of einsum_selfdot, lane 0 adds them and writes xn and 2^-e.
//   distance  probe_dist_matrix_kernel: a workgroup of 4 waves per tile of PM_QT = 64 queries.  The list is walked in
//             blocks of PM_RB = 128 rows and d in slabs of PM_DS = 112 halfs (7 K steps of 16).  LDS holds one slab of
//             the block's rows and of the tile's two query planes, PM_STRIDE = 240 bytes apart: 15 pieces of 16 bytes,
//             an odd number, so the 16-byte operand reads of lanes at consecutive rows start in different bank groups
//             (§3.21's rule).  The queries are the A operand (M = 32), the rows the B operand (N = 32): wave w owns rows
//             32w .. 32w + 31 of the block against the whole tile, one 16-float accumulator per 32 queries, two MFMAs a
//             K step (hi, lo) into each.  Lane l holds column l & 31 — one row's distances to the queries
//             8 (v / 4) + 4 (l / 32) + v % 4 — and stores them at the pair's segment + the row's position: lanes 0..31
//             write 32 consecutive keys of one segment.  The walk is one loop over (block, slab) steps as in
//             pe_wide_walk: the next step's global loads are in registers while this step's slab is multiplied.  Where
//             d fits one slab (d <= 112: the GloVe shape) the queries are staged once per tile.
//             yn: two lanes per row (row tid / 2: a row of the lane's own wave) read the staged slab and carry two of
//             einsum_selfdot's four chains each from slab to slab — whole groups of 16 in the order 3, 2, 1, 0, the
//             last partial group ascending over its zero-filled fours, which is the tail loop — and a shuffle hands the
//             sum to the lane that holds the row's column.  A slab is 7 whole groups, so a slab edge is a group edge.
// Why 64 queries a tile and not 32: a staged row meets twice the queries, so a list's rows are read half as often, at
// 16 more accumulator registers (181 VGPRs + 32 AGPRs, no scratch: two workgroups a CU, which LDS allows either way).
// LDS: static, 64 000 bytes (PmLds below), within the 64 KiB a workgroup gets without asking.
#include "probe_job.h"
#include "np_order.h"
#include "span_exact.h"

#define PM_THREADS 256
#define PM_QT 64
#define PM_RB 128
#define PM_DS 112                           // halfs of a slab
#define PM_UR (PM_DS / 8)                   // 16-byte pieces of a slab of one row
#define PM_STRIDE (PM_DS * 2 + 16)          // bytes between two staged rows: 15 pieces
#define PM_NP (PM_RB * PM_UR / PM_THREADS)  // pieces a lane stages of the rows, and of the two query planes
static_assert(PM_DS % 16 == 0 && (PM_STRIDE / 16) % 2 == 1, "whole K steps and einsum groups; an odd stride in pieces");
static_assert(PM_NP * PM_THREADS == PM_RB * PM_UR && 2 * PM_QT == PM_RB, "whole pieces a lane; the planes stage as the rows do");
static_assert(2 * PM_RB == PM_THREADS && PM_RB == 32 * (PM_THREADS / 64), "two lanes a row; 32 rows a wave");

typedef _Float16 pm_half8 __attribute__((ext_vector_type(8)));
typedef float pm_float16 __attribute__((ext_vector_type(16)));

struct PmLds {
    unsigned char xh[PM_QT * PM_STRIDE], xl[PM_QT * PM_STRIDE];     // the tile's slab of x_hi and x_lo
    unsigned char yr[PM_RB * PM_STRIDE];                            // the block's slab of the rows
    int32_t rid[2][PM_RB];          // the labels of this block and the next, -1: no row
    long long pseg[PM_QT];          // where each query's keys of this list begin
    int64_t qrow[PM_QT];            // each query's row of the planes
    float xn[PM_QT], xs[PM_QT];     // |x|^2 and 2^-e
};

__global__ __launch_bounds__(64) void pm_prepare_kernel(const float *__restrict__ q, const int d, const int dpad,
                                                        _Float16 *__restrict__ xh, _Float16 *__restrict__ xl,
                                                        float *__restrict__ xn, float *__restrict__ xs)
{
    const int lane = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const float *x = q + qi * d;
    float m = 0.0f;
    for (int c = lane; c < d; c += 64) m = fmaxf(m, fabsf(x[c]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    int e = 0;
    if (m > 0.0f) {
        int p;
        (void)frexpf(m, &p);        // m in [2^(p-1), 2^p)
        e = 15 - p < 126 ? 15 - p : 126;
    }
    for (int c = lane; c < dpad; c += 64) {
        const float v = c < d ? ldexpf(x[c], e) : 0.0f;
        const _Float16 hi = (_Float16)v;
        xh[qi * dpad + c] = hi;
        xl[qi * dpad + c] = (_Float16)(v - (float)hi);
    }
    // einsum_selfdot's accumulator `lane` of four
    float acc = 0.0f;
    if (lane < 4) {
        int i = 0;
        for (; d - i >= 16; i += 16)
#pragma unroll
            for (int g = 3; g >= 0; g--) acc = x[i + 4 * g + lane] * x[i + 4 * g + lane] + acc;
        for (; i < d; i += 4) {
            const float v = i + lane < d ? x[i + lane] : 0.0f;
            acc = v * v + acc;
        }
    }
    const float a1 = __shfl(acc, 1), a2 = __shfl(acc, 2), a3 = __shfl(acc, 3);
    if (lane == 0) {
        xn[qi] = (acc + a1) + (a2 + a3);
        xs[qi] = ldexpf(1.0f, -e);
    }
}

template <typename U>
__device__ __forceinline__ void pm_walk(const PeJob &j, const PmQueries &mx, PmLds &s, const int4 tile)
{
    typedef GxKey<float>::type K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = j.d, cnt = tile.z;
    const int64_t n = j.list_n[tile.x], base = j.ids_off[tile.x];
    const int up = mx.dpad / 8;                                         // pieces of a whole plane row
    const int NS = (d + PM_DS - 1) / PM_DS, G = d / 16;                 // slabs; whole einsum groups of a row
    const int64_t steps = (n + PM_RB - 1) / PM_RB * NS;
    const _Float16 *rows = (const _Float16 *)j.rows;
    K *keys = (K *)j.keys;
    const bool two = cnt > 32;                                          // (the same in every lane)
    uint4 ry[PM_NP], rx[PM_NP];
    auto label = [&](int64_t pos) -> int32_t {
        const int64_t id = pos < n ? j.ids[base + pos] : -1;
        return (id >= 0 && id < j.N) ? (int32_t)id : -1;
    };
    auto fetch_rows = [&](int64_t step) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
#pragma unroll
        for (int p = 0; p < PM_NP; p++) {
            const int e = tid + p * PM_THREADS, r = e / PM_UR, c = sl * PM_UR + e % PM_UR;
            const int32_t id = s.rid[b & 1][r];
            ry[p] = id >= 0 ? pm_row_piece<U>(rows + (int64_t)id * d, c, d) : make_uint4(0, 0, 0, 0);
        }
    };
    auto fetch_queries = [&](int sl) {              // entries 0 .. PM_QT - 1: x_hi, then x_lo
#pragma unroll
        for (int p = 0; p < PM_NP; p++) {
            const int e = tid + p * PM_THREADS, r = e / PM_UR, u = r & (PM_QT - 1), c = sl * PM_UR + e % PM_UR;
            const _Float16 *plane = r < PM_QT ? mx.xh : mx.xl;
            rx[p] = (u < cnt && c < up) ? ((const uint4 *)(plane + s.qrow[u] * mx.dpad))[c] : make_uint4(0, 0, 0, 0);
        }
    };
    auto commit = [&](bool queries) {
#pragma unroll
        for (int p = 0; p < PM_NP; p++) {
            const int e = tid + p * PM_THREADS, r = e / PM_UR, c = e % PM_UR;
            ((uint4 *)(s.yr + r * PM_STRIDE))[c] = ry[p];
            if (queries) ((uint4 *)((r < PM_QT ? s.xh : s.xl) + (r & (PM_QT - 1)) * PM_STRIDE))[c] = rx[p];
        }
    };

    for (int u = tid; u < cnt; u += PM_THREADS) {
        const int pr = j.pair_of[tile.y + u];
        const int64_t qi = pr / j.kc;
        s.pseg[u] = j.segoff[pr] - j.seg_base;
        s.qrow[u] = qi;
        s.xn[u] = mx.xn[qi];
        s.xs[u] = mx.xs[qi];
    }
    if (tid < PM_RB) s.rid[0][tid] = label(tid);
    __syncthreads();
    if (steps > 0) {
        fetch_rows(0);
        fetch_queries(0);
    }
    pm_float16 acc0, acc1;
    float yacc[2] = {0.0f, 0.0f};                   // the chains 2h and 2h + 1 of row tid / 2, h = tid & 1
    const int yrow = tid >> 1, yh = tid & 1;
    const int mrow = wave * 32 + (lane & 31);       // the lane's column: this row of the block
    const int koff = (lane >> 5) * 16;              // its 8 halfs of a K step
    for (int64_t step = 0; step < steps; step++) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
        const bool last = sl == NS - 1;
        int32_t next = -1;
        if (last && tid < PM_RB) next = label((b + 1) * PM_RB + tid);
        __syncthreads();                            // the last step's arithmetic is done with the slabs
        commit(NS > 1 || step == 0);
        if (last && tid < PM_RB) s.rid[(b + 1) & 1][tid] = next;       // (read again two blocks on, behind barriers)
        __syncthreads();
        if (step + 1 < steps) {
            fetch_rows(step + 1);
            if (NS > 1) fetch_queries((int)((step + 1) % NS));
        }
        if (sl == 0) {
#pragma unroll
            for (int v = 0; v < 16; v++) acc0[v] = acc1[v] = 0.0f;
            yacc[0] = yacc[1] = 0.0f;
        }
        // yn: the slab's groups of 16 of row yrow, the lane's two chains
        {
            const _Float16 *y = (const _Float16 *)(s.yr + yrow * PM_STRIDE) + 2 * yh;
#pragma unroll
            for (int g = 0; g < PM_DS / 16; g++) {
                const int gg = sl * (PM_DS / 16) + g;
                if (gg > G || (gg == G && d % 16 == 0)) break;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int m4 = gg < G ? 3 - t : t;      // whole groups 3, 2, 1, 0; the tail's fours ascending
                    const float v0 = (float)y[16 * g + 4 * m4], v1 = (float)y[16 * g + 4 * m4 + 1];
                    yacc[0] = v0 * v0 + yacc[0];
                    yacc[1] = v1 * v1 + yacc[1];
                }
            }
        }
        // the slab's K steps: (x_hi + x_lo) . y into the accumulators
        {
            int nk = (mx.dpad - sl * PM_DS) / 16;
            nk = nk < PM_DS / 16 ? nk : PM_DS / 16;
            const unsigned char *pb = s.yr + mrow * PM_STRIDE + koff;
            const unsigned char *ph = s.xh + (lane & 31) * PM_STRIDE + koff, *pl = s.xl + (lane & 31) * PM_STRIDE + koff;
            for (int ks = 0; ks < nk; ks++) {
                const pm_half8 bv = *(const pm_half8 *)(pb + ks * 32);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const pm_half8 *)(ph + ks * 32), bv, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const pm_half8 *)(pl + ks * 32), bv, acc0, 0, 0, 0);
                if (two) {
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const pm_half8 *)(ph + 32 * PM_STRIDE + ks * 32), bv,
                                                                  acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const pm_half8 *)(pl + 32 * PM_STRIDE + ks * 32), bv,
                                                                  acc1, 0, 0, 0);
                }
            }
        }
        if (!last) continue;
        const float ys = yacc[0] + yacc[1];                             // acc0 + acc1, or acc2 + acc3
        const float yn = __shfl(ys + __shfl_xor(ys, 1), 2 * (lane & 31));       // the row of the lane's column
        const int64_t pos = b * PM_RB + mrow;
        if (pos >= n) continue;
        const bool stored = s.rid[b & 1][mrow] >= 0;
#pragma unroll
        for (int v = 0; v < 16; v++) {
            const int u = 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int uu = u + 32 * h;
                if (uu >= cnt) continue;
                const float dot = (h ? acc1[v] : acc0[v]) * s.xs[uu];
                const float r = (s.xn[uu] + yn) - 2.0f * dot;
                keys[s.pseg[uu] + pos] = stored ? GxKey<float>::of(r > 0.0f ? r : 0.0f) : ~(K)0;
            }
        }
    }
}

__global__ __launch_bounds__(PM_THREADS) void probe_dist_matrix_kernel(const PeJob j, const PmQueries mx)
{
    __shared__ __attribute__((aligned(16))) PmLds s;
    if ((int)blockIdx.x >= j.tile_off[j.n_lists]) return;               // (the grid is an upper bound of the tiles)
    const int4 tile = j.tiles[blockIdx.x];
    if (j.d % 8 == 0) pm_walk<uint4>(j, mx, s, tile);
    else if (j.d % 4 == 0) pm_walk<uint2>(j, mx, s, tile);
    else pm_walk<_Float16>(j, mx, s, tile);
}

// ---- what probe_exact.hip's driver calls ----

int pm_check(const tk_index *ix, const float *q, int64_t nq)
{
    ARGCHECK(ix->data_dtype == TK_DATA_F16, "matrix=True needs store=\"float16\" (the rows are the f16 operands as stored)");
    const uint32_t *b = (const uint32_t *)q;
    const int64_t total = nq * ix->d;
    uint32_t bad = 0;
    for (int64_t i = 0; i < total; i++) bad |= ((b[i] & 0x7fffffffu) + 0x00800000u) & 0x80000000u;    // exponent all ones
    ARGCHECK(!bad, "matrix=True: a query holds a NaN or an infinity");
    return TK_OK;
}

void pm_tile(PeTile &t)
{
    t.QT = PM_QT;
    t.RB = PM_RB;
    t.xstride = t.ystride = PM_STRIDE;
    t.lds = sizeof(PmLds);
    t.DS = PM_DS;
}

int pm_prepare(tk_index *ix, int64_t nq, PmQueries &mx)
{
    const int dpad = (ix->d + 15) / 16 * 16;
    TRY(ix->pm_xh.ensure((size_t)nq * dpad * 2));
    TRY(ix->pm_xl.ensure((size_t)nq * dpad * 2));
    TRY(ix->pm_xn.ensure((size_t)nq * 8));
    mx.xh = ix->pm_xh.as<_Float16>();
    mx.xl = ix->pm_xl.as<_Float16>();
    mx.xn = ix->pm_xn.as<float>();
    mx.xs = mx.xn + nq;
    mx.dpad = dpad;
    hipLaunchKernelGGL(pm_prepare_kernel, dim3((unsigned)nq), dim3(64), 0, 0, ix->br_q.as<float>(), ix->d, dpad,
                       ix->pm_xh.as<_Float16>(), ix->pm_xl.as<_Float16>(), ix->pm_xn.as<float>(),
                       ix->pm_xn.as<float>() + nq);
    HIPCHECK(hipGetLastError());
    return TK_OK;
}

void pm_launch_dist(const PeJob &j, const PmQueries &mx, unsigned max_tiles)
{
    hipLaunchKernelGGL(probe_dist_matrix_kernel, dim3(max_tiles), dim3(PM_THREADS), 0, 0, j, mx);
}
