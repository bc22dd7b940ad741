// probe_f32.hip — knn_probe's distance pass on the f32 matrix cores for float32-stored vectors (IVF.knn_probe(wide=True),
// tk_index_knn_probe_wide).  Probes, segments, pairs, tiles, keys and the selection are probe_exact.hip's
// (§3.21), through its driver; only the value behind each key differs.  It is knn_brute(wide=True)'s part, bit for bit
// (brute_wide.hip, §3.25):
//   part = (xn + yn) - acc                 in float32, NOT clamped: rounding can make it slightly negative
//   acc  = ONE float32 accumulator of v_mfma_f32_32x32x2_f32 per (query, row): k ascending from 0 over all of d, the A
//          operand 2 * x, starting at 0 and carried across the slabs — no split-K, no second chain
//   xn, yn = the float32 self-dots of the query and of the row in numpy's einsum order (np_order.h, einsum_selfdot)
// so with every list probed the call returns knn_brute(wide=True)'s ids and bytes, and on data whose products and sums
// are exact in float32 those of the exact knn_probe.
//   queries   tk_launch_brute_wide_prepare (brute_wide.hip) on the call's queries: 2 x zero-extended to dq floats a row,
//             and xn.
//   distance  probe_dist_f32_kernel: a workgroup of 4 waves per tile of PF_QT = 64 queries.  The list is walked in blocks
//             of PF_RB = 128 rows and d in slabs of PF_DS floats.  LDS holds one slab of the block's rows and one of the
//             tile's queries, row-major, PF_STRIDE = PF_DS + 1 floats apart: an odd number, so the 32 rows (or queries)
//             a half-wave reads at one k lie in 32 different banks.  Slab tails, missing rows and missing queries are
//             zeros: fma(0, 0, acc) = acc.  The queries are the A operand (M = 32), the rows the B operand (N = 32):
//             wave w owns rows 32w .. 32w + 31 of the block against the whole tile, one 16-float accumulator per 32
//             queries — the second skipped where the tile has at most 32 — and a k-pair is 2 MFMAs from 3 operand reads
//             of 4 bytes.  Lane l holds column l & 31 — one row's values to the queries 8 (v / 4) + 4 (l / 32) + v % 4
//             — and stores them at the pair's segment + the row's position: lanes 0..31 write 32 consecutive keys of
//             one segment (probe_matrix.hip's pattern).  The walk is one loop over (block, slab) steps: the next step's
//             global loads are in registers while this step's slab is multiplied.  Where d fits one slab the queries
//             are staged once per tile.
//             yn: two lanes per row (row tid / 2: a row of the lane's own wave) read the staged slab and carry two of
//             einsum_selfdot's four chains each from slab to slab — whole groups of 16 in the order 3, 2, 1, 0, the
//             last partial group ascending over its zero-filled fours — and a shuffle hands the sum to the lane that
//             holds the row's column: row_norms_kernel's bytes without a pass over the rows no query probes.  A slab
//             is a whole number of groups, so a slab edge is a group edge.
// Why PF_DS = 64 and not 32: half the (block, slab) steps, so half the barriers and commits per multiplied k; §3.27 has
// both measured.  LDS: static, PfLds below: 192 * (PF_DS + 1) * 4 + 2 304 = 52 224 bytes, within the 64 KiB a workgroup
// gets without asking; two workgroups a CU (137 VGPRs, no scratch).
#include "probe_job.h"
#include "np_order.h"
#include "brute_tile.h"
#include "span_exact.h"

#define PF_THREADS 256
#define PF_QT 64
#define PF_RB 128
#define PF_DS 64                            // floats of a slab
#define PF_UR (PF_DS / 4)                   // 16-byte pieces of a slab of one row
#define PF_STRIDE (PF_DS + 1)               // floats between two staged rows
#define PF_NY (PF_RB * PF_UR / PF_THREADS)  // pieces a lane stages of the rows
#define PF_NX (PF_QT * PF_UR / PF_THREADS)  // and of the queries
static_assert(PF_DS % 16 == 0 && PF_STRIDE % 2 == 1, "whole einsum groups; an odd stride in floats");
static_assert(PF_NY * PF_THREADS == PF_RB * PF_UR && PF_NX * PF_THREADS == PF_QT * PF_UR, "whole pieces a lane");
static_assert(2 * PF_RB == PF_THREADS && PF_RB == 32 * (PF_THREADS / 64) && PF_QT == 64, "two lanes a row; 32 rows a wave; two accumulators");

struct PfLds {
    float x[PF_QT * PF_STRIDE];     // the tile's slab of 2 x
    float y[PF_RB * PF_STRIDE];     // the block's slab of the rows
    int32_t rid[2][PF_RB];          // the labels of this block and the next, -1: no row
    long long pseg[PF_QT];          // where each query's keys of this list begin
    int64_t qrow[PF_QT];            // each query's row of x2
    float xn[PF_QT];                // |x|^2
};
static_assert(sizeof(PfLds) <= 64 * 1024, "static LDS");

template <typename U>
__device__ __forceinline__ void pf_walk(const PeJob &j, const TkBruteWide &wd, PfLds &s, const int4 tile)
{
    typedef GxKey<float>::type K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = j.d, dq = wd.dq, cnt = tile.z;
    const int64_t n = j.list_n[tile.x], base = j.ids_off[tile.x];
    const int NS = (d + PF_DS - 1) / PF_DS, G = d / 16;                 // slabs; whole einsum groups of a row
    const int64_t steps = (n + PF_RB - 1) / PF_RB * NS;
    const float *rows = (const float *)j.rows;
    K *keys = (K *)j.keys;
    const bool two = cnt > 32;                                          // (the same in every lane)
    uint4 ry[PF_NY], rx[PF_NX];
    auto label = [&](int64_t pos) -> int32_t {
        const int64_t id = pos < n ? j.ids[base + pos] : -1;
        return (id >= 0 && id < j.N) ? (int32_t)id : -1;
    };
    // a lane's pieces: row (or query) tid / PF_UR + (256 / PF_UR) p, piece tid % PF_UR of the slab
    const int er = tid / PF_UR, ec = tid % PF_UR;
    auto fetch_rows = [&](int64_t step) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
#pragma unroll
        for (int p = 0; p < PF_NY; p++) {
            const int32_t id = s.rid[b & 1][er + p * (PF_THREADS / PF_UR)];
            ry[p] = id >= 0 ? bw_row_piece<U>(rows + (int64_t)id * d, sl * PF_UR + ec, d) : make_uint4(0, 0, 0, 0);
        }
    };
    auto fetch_queries = [&](int sl) {
        const int c = (sl * PF_UR + ec) * 4;
#pragma unroll
        for (int p = 0; p < PF_NX; p++) {
            const int u = er + p * (PF_THREADS / PF_UR);
            rx[p] = (u < cnt && c < dq) ? *(const uint4 *)(wd.x2 + s.qrow[u] * dq + c) : make_uint4(0, 0, 0, 0);
        }
    };
    auto put = [&](float *slab, int p, const uint4 &v) {
        float *at = slab + (er + p * (PF_THREADS / PF_UR)) * PF_STRIDE + ec * 4;
        at[0] = __uint_as_float(v.x);
        at[1] = __uint_as_float(v.y);
        at[2] = __uint_as_float(v.z);
        at[3] = __uint_as_float(v.w);
    };
    auto commit = [&](bool queries) {
#pragma unroll
        for (int p = 0; p < PF_NY; p++) put(s.y, p, ry[p]);
        if (queries) {
#pragma unroll
            for (int p = 0; p < PF_NX; p++) put(s.x, p, rx[p]);
        }
    };

    for (int u = tid; u < cnt; u += PF_THREADS) {
        const int pr = j.pair_of[tile.y + u];
        const int64_t qi = pr / j.kc;
        s.pseg[u] = j.segoff[pr] - j.seg_base;
        s.qrow[u] = qi;
        s.xn[u] = wd.xn[qi];
    }
    if (tid < PF_RB) s.rid[0][tid] = label(tid);
    __syncthreads();
    if (steps > 0) {
        fetch_rows(0);
        fetch_queries(0);
    }
    tk_f32x16 acc0, acc1;
    float yacc[2] = {0.0f, 0.0f};                   // the chains 2h and 2h + 1 of row tid / 2, h = tid & 1
    const int yrow = tid >> 1, yh = tid & 1;
    const int mrow = wave * 32 + (lane & 31);       // the lane's column: this row of the block
    // the lane's operands of k-pair t: k = 2 t + (lane >> 5) of query lane & 31 (and 32 further) and of row mrow
    const float *pa = s.x + (lane & 31) * PF_STRIDE + (lane >> 5);
    const float *pb = s.y + mrow * PF_STRIDE + (lane >> 5);
    for (int64_t step = 0; step < steps; step++) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
        const bool last = sl == NS - 1;
        int32_t next = -1;
        if (last && tid < PF_RB) next = label((b + 1) * PF_RB + tid);
        __syncthreads();                            // the last step's arithmetic is done with the slabs
        commit(NS > 1 || step == 0);
        if (last && tid < PF_RB) s.rid[(b + 1) & 1][tid] = next;       // (read again two blocks on, behind barriers)
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
            const float *y = s.y + yrow * PF_STRIDE + 2 * yh;
#pragma unroll
            for (int g = 0; g < PF_DS / 16; g++) {
                const int gg = sl * (PF_DS / 16) + g;
                if (gg > G || (gg == G && d % 16 == 0)) break;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int m4 = gg < G ? 3 - t : t;      // whole groups 3, 2, 1, 0; the tail's fours ascending
                    const float v0 = y[16 * g + 4 * m4], v1 = y[16 * g + 4 * m4 + 1];
                    yacc[0] = v0 * v0 + yacc[0];
                    yacc[1] = v1 * v1 + yacc[1];
                }
            }
        }
        // the slab's k-pairs in groups of 4 (the tail of the last group is zeros): 2 x . y into the accumulators
        {
            int nk = d - sl * PF_DS;
            nk = nk < PF_DS ? nk : PF_DS;
            const int ng = (nk + 7) / 8;
#pragma unroll 1
            for (int g = 0; g < ng; g++) {
#pragma unroll
                for (int t = 4 * g; t < 4 * g + 4; t++) {
                    const float bv = pb[2 * t];
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * t], bv, acc0, 0, 0, 0);
                    if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[32 * PF_STRIDE + 2 * t], bv, acc1, 0, 0, 0);
                }
            }
        }
        if (!last) continue;
        const float ys = yacc[0] + yacc[1];                             // acc0 + acc1, or acc2 + acc3
        const float yn = __shfl(ys + __shfl_xor(ys, 1), 2 * (lane & 31));       // the row of the lane's column
        const int64_t pos = b * PF_RB + mrow;
        if (pos >= n) continue;
        const bool stored = s.rid[b & 1][mrow] >= 0;
#pragma unroll
        for (int v = 0; v < 16; v++) {
            const int u = 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int uu = u + 32 * h;
                if (uu >= cnt) continue;
                const float part = (s.xn[uu] + yn) - (h ? acc1[v] : acc0[v]);
                keys[s.pseg[uu] + pos] = stored ? GxKey<float>::of(part) : ~(K)0;
            }
        }
    }
}

template <typename U>
__global__ __launch_bounds__(PF_THREADS, 2) void probe_dist_f32_kernel(const PeJob j, const TkBruteWide wd)
{
    __shared__ __attribute__((aligned(16))) PfLds s;
    if ((int)blockIdx.x >= j.tile_off[j.n_lists]) return;               // (the grid is an upper bound of the tiles)
    pf_walk<U>(j, wd, s, j.tiles[blockIdx.x]);
}

// ---- what probe_exact.hip's driver calls ----

int pf_check(const tk_index *ix)
{
    ARGCHECK(ix->data_dtype == TK_DATA_F32, "wide=True needs store=\"float32\" (the rows are the f32 operands as stored)");
    return TK_OK;
}

void pf_tile(PeTile &t)
{
    t.QT = PF_QT;
    t.RB = PF_RB;
    t.xstride = PF_STRIDE;
    t.ystride = PF_STRIDE * 4;
    t.lds = sizeof(PfLds);
    t.DS = PF_DS;
}

// one kernel per load width of a row: 16 bytes where d % 4 == 0, 8 where d % 2 == 0, else floats
void pf_launch_dist(const PeJob &j, const TkBruteWide &wd, unsigned max_tiles)
{
    if (j.d % 4 == 0) hipLaunchKernelGGL(probe_dist_f32_kernel<uint4>, dim3(max_tiles), dim3(PF_THREADS), 0, 0, j, wd);
    else if (j.d % 2 == 0) hipLaunchKernelGGL(probe_dist_f32_kernel<uint2>, dim3(max_tiles), dim3(PF_THREADS), 0, 0, j, wd);
    else hipLaunchKernelGGL(probe_dist_f32_kernel<float>, dim3(max_tiles), dim3(PF_THREADS), 0, 0, j, wd);
}
