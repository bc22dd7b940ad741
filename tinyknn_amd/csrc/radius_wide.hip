// radius_wide.hip — every row within a radius of each query over ALL rows of a float32 store on the f32 matrix cores,
// any d <= 4096 (radius_search(wide=True), tk_index_radius_brute_wide).  The queries are prepared by
// brute_wide.hip (tk_launch_brute_wide_prepare: 2 x zero-extended, |x|^2), the row norms are brute.hip's
// (row_norms_kernel, per call), the restriction builder and the tail (lims, segmented sort, decode, fetch) are
// radius.hip's, the unstage and the zero kernel radius_matrix.hip's; only the tile kernel lives here.  Row j is a hit of
// query i iff it passes the query's restriction and
//   part(i, j) <= radius[i]        float32, inclusive
// with part brute_wide.hip's value bit for bit: (xn + yn) - acc, ONE float32 accumulator of v_mfma_f32_32x32x2_f32 per
// pair, k ascending from 0 over all of d, the A operand 2 x, starting at 0; no split-K, no clamp (part may be negative).
//   walk   a copy of brute_wide.hip's bw_walk (that file stays as it is, its four instances and their resources pinned
//          by tests/test_knn_brute_wide_resources.py): 4 waves own 128 queries x blocks of 128 contiguous rows, a
//          64 x 64 quadrant a wave in four 32 x 32 accumulators, queries the A operand and rows the B operand, d in
//          slabs of 32 floats through LDS, row-major at an odd stride of 33 floats, the next step's global loads in
//          registers, brute_tile_grid's split of the rows over blockIdx.y.  Slab tails and rows past the range are
//          zeros: fma(0, 0, acc) = acc.  The fetches address with a base that is the same in every lane plus a 32-bit
//          offset of the lane (radius_matrix.hip's form).  xn and the RADIUS of the tile's queries wait behind the
//          slabs; the queries' attributes behind them when RESTRICTED.
//          Static LDS: 2 x 128 x 33 x 4 + 1 024 = 34 816 bytes, 45 056 restricted.
//   end    radius_matrix.hip's: the hit predicate is  in-tile query && live column && part <= radius, then the
//          restriction (a row's group, tags and keys are read where a pair is inside the radius).  It is ballotted per
//          accumulator register and row half: the low and the high 32 lanes hold two different queries against 32 rows
//          each, so one lane per half adds the half's popcount to the query's counter and every hit lane takes base +
//          popcount(hits below it) — one atomic per (wave, register, row half, query) with hits.  No lane skips a ballot.
//   PASS 0 count: the atomic goes to count[q], nothing is stored (radius_count(wide=True)).
//   PASS 1 count and stage: the base the atomic on count[q] returns is already a slot; a hit whose slot < cap writes
//          its key (brute_select_kernel's: monotone float bits high, row id low) to stage[q * cap + slot].
//   PASS 2 refill: the same walk, blockIdx.x mapped through the compacted list of the query tiles that hold a query
//          with count > cap.  Every query of such a tile is refilled from a zeroed slots[q] into keys[offset[q] + slot],
//          each store guarded by slot < count[q], the error flag raised otherwise.  Not launched when no tile overflowed.
// No store lands outside its segment: the stage write is guarded by slot < cap, the refill write by slot < count[q].
#include "kernels.h"
#include "brute_tile.h"

#define RW_THREADS 256
#define RW_QT 128
#define RW_RB 128
#define RW_DS 32                            // floats of a slab
#define RW_UR (RW_DS / 4)                   // 16-byte pieces of a slab of one row
#define RW_STRIDE (RW_DS + 1)               // floats between two staged rows
#define RW_NP (RW_RB * RW_UR / RW_THREADS)  // pieces a lane stages of the rows; of the queries as many
#define RW_ATTR (128 * (16 * 4 + 8 + 4 + 4))    // tile_attr_bytes at its largest: 4 value columns, tags, exclude, group
static_assert(RW_DS % 8 == 0 && RW_STRIDE % 2 == 1, "whole groups of 4 k-pairs; an odd stride in floats");
static_assert(RW_NP * RW_THREADS == RW_RB * RW_UR && RW_QT == RW_RB && RW_QT == 128, "whole pieces a lane; tile_attr_bytes' 128 queries");
static_assert((2 * RW_RB * RW_STRIDE + 2 * RW_QT) * 4 + RW_ATTR <= 64 * 1024, "static LDS");

template <bool RESTRICTED>
struct RwLds {
    float x[RW_QT * RW_STRIDE];                     // the tile's slab of 2 x
    float y[RW_RB * RW_STRIDE];                     // the block's slab of the rows
    float xn[RW_QT], rad[RW_QT];                    // what the epilogue reads of the tile's queries
    unsigned char attr[RESTRICTED ? RW_ATTR : 0];   // the queries' attributes (tile_attr_bytes)
};

struct RwJob {
    TkBruteWide wd;
    int64_t nq;
    int d;
    const float *Y;                 // rows [0, cols)
    const float *ynorm2;            // their norms
    int64_t cols;
    const float *radius;            // (nq)
    int *count;                     // (nq): PASS 0 / 1 add to it, PASS 2 reads it
    unsigned long long *stage;      // PASS 1: (nq, cap)
    int cap;
    const int *tiles;               // PASS 2: the query tile of blockIdx.x
    const int64_t *offset;          // PASS 2: (nq) where each query's keys begin
    int *slots;                     // PASS 2: (nq), zeroed
    unsigned long long *keys;       // PASS 2
    int *err;                       // PASS 2
    TkBruteRestrict r;
};

// piece c (4 floats) of a row of d floats, zeros behind d, in loads of U: uint4 where d % 4 == 0, uint2 where d % 2 == 0,
// else floats — d is a multiple of the floats of U, so a load is whole or not made (bw_row_piece's forms)
template <typename U>
__device__ __forceinline__ uint4 rw_row_piece(const float *row, int c, int d)
{
    constexpr int NU = 16 / (int)sizeof(U), E = (int)sizeof(U) / 4;
    union {
        uint4 v;
        U u[NU];
    } p;
    p.v = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NU; i++)
        if (c * 4 + i * E < d) p.u[i] = *(const U *)(row + c * 4 + i * E);
    return p.v;
}

template <int PASS, bool RESTRICTED, typename U>
__device__ __forceinline__ void rw_walk(const RwJob &j, RwLds<RESTRICTED> &s)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = j.d, dq = j.wd.dq;
    const TkBruteRestrict &r = j.r;
    const int64_t q0 = (int64_t)(PASS == 2 ? j.tiles[blockIdx.x] : (int)blockIdx.x) * RW_QT;
    const int NS = (d + RW_DS - 1) / RW_DS;                             // slabs
    // blockIdx.y's share of the columns, in whole blocks
    const int64_t per_y = ((j.cols + gridDim.y - 1) / gridDim.y + RW_RB - 1) / RW_RB * RW_RB;
    const int64_t c_begin = (int64_t)blockIdx.y * per_y;
    const int64_t ncols = c_begin + per_y < j.cols ? c_begin + per_y : j.cols;
    if (c_begin >= ncols) return;                                       // (the whole workgroup)
    const int64_t steps = (ncols - c_begin + RW_RB - 1) / RW_RB * NS;

    // what waits in LDS for the epilogue: xn and the radius, and the attributes behind them (the arrays of
    // tile_attr_bytes at their largest, each at a fixed place).  Made visible by the barriers in front of the first slab
    int64_t *q_ranges = (int64_t *)s.attr;
    uint64_t *q_tags = (uint64_t *)(q_ranges + RW_QT * 8);
    int32_t *q_exclude = (int32_t *)(q_tags + RW_QT);
    int32_t *q_group = q_exclude + RW_QT;
    if (tid < RW_QT) {
        int64_t row = q0 + tid;
        row = row < j.nq ? row : j.nq - 1;
        s.xn[tid] = j.wd.xn[row];
        s.rad[tid] = j.radius[row];
        if constexpr (RESTRICTED) {
            if (r.exclude) q_exclude[tid] = (int32_t)r.exclude[row];
            if (r.tags) q_tags[tid] = r.tags[row];
            if (r.group) q_group[tid] = r.group[row];
            for (int c = 0; c < 2 * r.cols; c++) q_ranges[tid * 8 + c] = r.ranges[row * 2 * r.cols + c];
        }
    }

    // a lane's pieces: row (or query) tid / 8 + 32 p of the block, piece tid % 8 of the slab
    uint4 ry[RW_NP], rx[RW_NP];
    const int er = tid / RW_UR, ec = tid % RW_UR;
    const int qleft = (int)(j.nq - q0 < RW_QT ? j.nq - q0 : RW_QT);    // queries of the tile
    auto fetch_rows = [&](int64_t step) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
        const int64_t first = c_begin + b * RW_RB;
        const int left = (int)(ncols - first < RW_RB ? ncols - first : RW_RB);
        // (a base that is the same in every lane plus a 32-bit offset of the lane: 128 rows of d <= 4096 floats)
        const float *yb = j.Y + first * d;
#pragma unroll
        for (int p = 0; p < RW_NP; p++) {
            unsigned at = (unsigned)(er + 32 * p) * (unsigned)d;
            asm volatile("" : "+v"(at));            // (one 32-bit offset: no 64-bit part of it is kept from step to step)
            ry[p] = er + 32 * p < left ? rw_row_piece<U>(yb + at, sl * RW_UR + ec, d) : make_uint4(0, 0, 0, 0);
        }
    };
    auto fetch_queries = [&](int sl) {
        const int c = sl * RW_UR + ec;
        const float *xb = j.wd.x2 + q0 * dq;
#pragma unroll
        for (int p = 0; p < RW_NP; p++) {
            unsigned at = (unsigned)(er + 32 * p) * (unsigned)dq + (unsigned)c * 4u;
            asm volatile("" : "+v"(at));            // (one 32-bit offset: no 64-bit part of it is kept from step to step)
            rx[p] = (er + 32 * p < qleft && c * 4 < dq) ? *(const uint4 *)(xb + at) : make_uint4(0, 0, 0, 0);
        }
    };
    auto put = [&](float *slab, int p, const uint4 &v) {
        float *at = slab + (er + 32 * p) * RW_STRIDE + ec * 4;
        at[0] = __uint_as_float(v.x);
        at[1] = __uint_as_float(v.y);
        at[2] = __uint_as_float(v.z);
        at[3] = __uint_as_float(v.w);
    };
    auto commit = [&](bool queries) {
#pragma unroll
        for (int p = 0; p < RW_NP; p++) put(s.y, p, ry[p]);
        if (queries) {
#pragma unroll
            for (int p = 0; p < RW_NP; p++) put(s.x, p, rx[p]);
        }
    };
    fetch_rows(0);
    fetch_queries(0);

    const int qh = wave & 1, rh = wave >> 1;        // the wave's quadrant
    const int half = lane >> 5, lc = lane & 31;     // the lane's half of a register (its query), its column
    // the lane's operands of k-pair t: k = 2 t + half of query / row lc (and 32 further)
    const float *pa = s.x + (64 * qh + lc) * RW_STRIDE + half;
    const float *pb = s.y + (64 * rh + lc) * RW_STRIDE + half;
    tk_f32x16 acc[2][2];                            // [query half][row half]
    // the lane's two columns of the block: the row's norm and what restricts it
    float yn[2] = {0.0f, 0.0f};
    bool row_ok[2] = {false, false};
    int32_t rid0 = 0;                               // the row of column 0; column 1 is 32 further (N < 2^31)
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
                const int64_t col = c_begin + b * RW_RB + 64 * rh + 32 * h + lc;
                row_ok[h] = col < ncols;
                yn[h] = row_ok[h] ? j.ynorm2[col] : 0.0f;
                if (h == 0) rid0 = (int32_t)col;
                if constexpr (RESTRICTED)
                    if (row_ok[h] && r.allowed) row_ok[h] = (r.allowed[col >> 5] >> (col & 31)) & 1u;
            }
        }
        // the slab's k-pairs in groups of 4 (the tail of the last group is zeros): 2 x . y into the four accumulators
        int nk = d - sl * RW_DS;
        nk = nk < RW_DS ? nk : RW_DS;
        const int ng = (nk + 7) / 8;
#pragma unroll 1
        for (int g = 0; g < ng; g++) {
#pragma unroll
            for (int t = 4 * g; t < 4 * g + 4; t++) {
                const float a0 = pa[2 * t], a1 = pa[32 * RW_STRIDE + 2 * t];
                const float b0 = pb[2 * t], b1 = pb[32 * RW_STRIDE + 2 * t];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if (sl != NS - 1) continue;
        // does the lane's column h pass the restriction of local query u?  The query's attributes come from LDS, the
        // row's group, tags and keys from memory: only the pairs inside the radius ask
        auto passes = [&](int u, int h) {
            int32_t id = rid0 + 32 * h;
            // (opaque: the 32 registers of a column ask for the same row, and what one pair loaded of it would otherwise
            // be kept for the others — two columns' attributes do not fit beside the accumulators)
            asm volatile("" : "+v"(id));
            bool ok = true;
            if (r.exclude) ok = id != q_exclude[u];
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
                    const int64_t *bd = q_ranges + u * 8 + c * 2, key = r.row_keys[c * r.n_rows + (int64_t)id];
                    ok &= bd[0] <= key && key <= bd[1];
                }
            return ok;
        };
        // the lane's first query; accumulator register v of query half a adds the same ku = 32 a + 8 (v / 4) + v % 4 in
        // every lane: what a pair addresses is a base that is the same in every lane plus a 32-bit offset of the lane
        // (128 * cap stage entries: cap <= 2^20), so no 64-bit address is kept per register
        int ul = 64 * qh + 4 * half;
        // (opaque to the optimiser, as in bw_walk: it would otherwise keep what every register's query addresses alive
        // across the whole walk)
        asm volatile("" : "+v"(ul));
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int vg = 0; vg < 4; vg++) {
                // the four queries v & 3 of this group: one 16-byte read each of their xn and radius
                const int u0 = ul + 32 * a + 8 * vg;
                const float4 gxn = *(const float4 *)(s.xn + u0), grad = *(const float4 *)(s.rad + u0);
                const float qxn[4] = {gxn.x, gxn.y, gxn.z, gxn.w}, qrad[4] = {grad.x, grad.y, grad.z, grad.w};
#pragma unroll
                for (int vi = 0; vi < 4; vi++) {
                    const int v = 4 * vg + vi, ku = 32 * a + 8 * vg + vi, u = ul + ku;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const float part = (qxn[vi] + yn[h]) - acc[a][h][v];
                        bool hit = u < qleft && row_ok[h] && part <= qrad[vi];
                        // (every lane of the wave votes; what follows is the same branch in every lane)
                        if (__ballot(hit) == 0) continue;
                        if constexpr (RESTRICTED)
                            if (hit) hit = passes(u, h);
                        const unsigned long long m = __ballot(hit);
                        if (RESTRICTED && m == 0) continue;
                        // the hits of the two queries of this register, and the first hit lane of each (any lane where
                        // there is none: it is no hit lane and adds nothing)
                        const uint32_t m0 = (uint32_t)m, m1 = (uint32_t)(m >> 32), mh = half ? m1 : m0;
                        const int lead0 = m0 ? __ffs(m0) - 1 : 0, lead1 = 32 + (m1 ? __ffs(m1) - 1 : 0);
                        const bool leads = hit && (lane == lead0 || lane == lead1);
                        int *ctr = (PASS == 2 ? j.slots : j.count) + q0;
                        if constexpr (PASS == 0) {
                            if (leads) atomicAdd(&ctr[(unsigned)u], __popc(mh));
                        } else {
                            int base = 0;
                            if (leads) base = atomicAdd(&ctr[(unsigned)u], __popc(mh));
                            const int base0 = __builtin_amdgcn_readlane(base, lead0), base1 = __builtin_amdgcn_readlane(base, lead1);
                            base = half ? base1 : base0;
                            if (hit) {
                                const uint32_t slot = (uint32_t)base + (half ? __builtin_amdgcn_mbcnt_hi(mh, 0u)
                                                                                : __builtin_amdgcn_mbcnt_lo(mh, 0u));
                                // brute_select_kernel's key: float bits made monotone, then the row
                                uint32_t k32 = __float_as_uint(part);
                                k32 = (k32 & 0x80000000u) ? ~k32 : (k32 | 0x80000000u);
                                const unsigned long long key = ((unsigned long long)k32 << 32) | (uint32_t)(rid0 + 32 * h);
                                if constexpr (PASS == 1) {
                                    if (slot < (uint32_t)j.cap) (j.stage + q0 * j.cap)[(unsigned)u * (unsigned)j.cap + slot] = key;
                                } else {
                                    if (slot < (uint32_t)(j.count + q0)[(unsigned)u])
                                        j.keys[(j.offset + q0)[(unsigned)u] + slot] = key;
                                    else
                                        atomicOr(j.err, 1);
                                }
                            }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);          // (the reads of the next group stay behind this one)
            }
    }
}

template <int PASS, bool RESTRICTED>
__global__ __launch_bounds__(RW_THREADS, 2) void radius_wide_tiles_kernel(const RwJob j)
{
    __shared__ __attribute__((aligned(16))) RwLds<RESTRICTED> s;
    if (j.d % 4 == 0) rw_walk<PASS, RESTRICTED, uint4>(j, s);
    else if (j.d % 2 == 0) rw_walk<PASS, RESTRICTED, uint2>(j, s);
    else rw_walk<PASS, RESTRICTED, float>(j, s);
}

template <int PASS>
static void rw_tiles(const RwJob &j, dim3 grid, bool restricted, hipStream_t s)
{
    if (restricted) hipLaunchKernelGGL((radius_wide_tiles_kernel<PASS, true>), grid, dim3(RW_THREADS), 0, s, j);
    else hipLaunchKernelGGL((radius_wide_tiles_kernel<PASS, false>), grid, dim3(RW_THREADS), 0, s, j);
}

// |y_j|^2 in numpy's einsum order: brute.hip's kernel, launched from here as radius.hip launches it
__global__ void row_norms_kernel(const float *__restrict__ Y, int64_t n, int d, float *__restrict__ out);

// The first pass over Y (N, d) float32, N < 2^31, d <= 4096: ynorm2 (N) takes the norms of Y (per call: add() and
// update() are seen), count (nq) is zeroed and takes every query's number of hits; stage == NULL: PASS 0, nothing else
// is written; else PASS 1 and stage (nq, cap) takes the first cap keys of every query.  wd:
// tk_launch_brute_wide_prepare's copy of the nq queries.
int tk_launch_radius_wide_count(const TkBruteWide &wd, int64_t nq, int d, const float *Y, int64_t N, float *ynorm2,
                                const float *radius, int *count, unsigned long long *stage, int cap,
                                const TkBruteRestrict *r, hipStream_t s)
{
    if (nq <= 0) return 0;
    if (d > 4096 || N >= (1ll << 31) || (stage && (cap < 1 || cap > (1 << 20)))) return -1;
    tk_launch_radius_zero(count, nq, s);
    if (N <= 0) return 0;
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, Y, N, d, ynorm2);
    const RwJob j{wd, nq, d, Y, ynorm2, N, radius, count, stage, stage ? cap : 0, nullptr, nullptr,
                  nullptr, nullptr, nullptr, r ? *r : TkBruteRestrict{}};
    const dim3 grid = brute_tile_grid(nq, N);
    if (stage) rw_tiles<1>(j, grid, r != nullptr, s);
    else rw_tiles<0>(j, grid, r != nullptr, s);
    return 0;
}

// Behind the first pass and the offsets: tiles (n_tiles) the query tiles to refill, ascending, refilled (ceil(nq / 128))
// 1 for each of them, both on the device.  PASS 2 over those tiles (slots (nq) and err (1) are zeroed here), then the
// unstage of every other query.  err != 0 afterwards: the passes disagreed (no store was made outside a segment).
int tk_launch_radius_wide_fill(const TkBruteWide &wd, int64_t nq, int d, const float *Y, int64_t N,
                               const float *ynorm2, const float *radius, const int *count,
                               const unsigned long long *stage, int cap, const int *tiles, int n_tiles,
                               const int *refilled, const int64_t *offset, int *slots, unsigned long long *keys,
                               int *err, const TkBruteRestrict *r, hipStream_t s)
{
    if (nq <= 0 || N <= 0) return 0;
    if (d > 4096 || N >= (1ll << 31) || cap < 1 || cap > (1 << 20)) return -1;
    tk_launch_radius_zero(err, 1, s);
    if (n_tiles > 0) {
        tk_launch_radius_zero(slots, nq, s);
        const RwJob j{wd, nq, d, Y, ynorm2, N, radius, (int *)count, nullptr, 0, tiles, offset,
                      slots, keys, err, r ? *r : TkBruteRestrict{}};
        const dim3 grid(n_tiles, brute_tile_grid((int64_t)n_tiles * RW_QT, N).y);
        rw_tiles<2>(j, grid, r != nullptr, s);
    }
    tk_launch_radius_unstage(stage, cap, count, offset, refilled, nq, keys, s);
    return 0;
}
