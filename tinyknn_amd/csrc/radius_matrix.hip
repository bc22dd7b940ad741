// radius_matrix.hip — every row within a radius of each query over ALL rows of a half store, on the f16 matrix cores,
// any d <= 4096 (radius_search(matrix=True), tk_index_radius_brute_matrix).  The queries are prepared by
// probe_matrix.hip (pm_prepare), the row norms are brute_matrix.hip's (brute_half_norms_kernel), the restriction builder
// and the tail (lims, segmented sort, decode, fetch) are radius.hip's; the tile kernel and the unstage kernel live
// here.  Row j is a hit of query i iff it passes the query's restriction and
//   dist_m(i, j) <= radius[i]        float32, inclusive
// with dist_m §3.22 / §3.23's value bit for bit: max(0, (xn + yn) - 2 (acc 2^-e)), ONE float32 accumulator of
// v_mfma_f32_32x32x16_f16 per pair, K steps of 16 ascending over dpad, x_hi before x_lo in each step.
//   walk   a copy of brute_matrix.hip's bm_walk (that file stays as it is, its four instances and their resources
//          pinned by tests/test_knn_brute_matrix_resources.py): 4 waves own 128 queries x blocks of 128 contiguous
//          rows, a 64 x 64 quadrant a wave in four 32 x 32 accumulators, queries the A operand and rows the B operand,
//          d in slabs of 64 halfs through LDS at a 144-byte stride, the next step's global loads in registers,
//          brute_tile_grid's split of the rows over blockIdx.y.  xn, 2^-e and the RADIUS of four queries sit in the 16
//          bytes behind their x_hi slabs; the queries' attributes behind the tiles when RESTRICTED.
//          Static LDS: 55 296 bytes, 65 536 restricted.
//   end    the hit predicate is  in-tile query && live column && dm <= radius, then the restriction (a row's group,
//          tags and keys are read where a pair is inside the radius).  It is ballotted per accumulator register and row
//          half: the low and the high 32 lanes hold two different queries against 32 rows each, so one lane per half
//          adds the half's popcount to the query's counter and every hit lane takes base + popcount(hits below it) —
//          one atomic per (wave, register, row half, query) with hits.  A query beyond the tile's last or a column
//          beyond the end makes the predicate false; no lane skips a ballot.
//   PASS 0 count: the atomic goes to count[q], nothing is stored (radius_count(matrix=True)).
//   PASS 1 count and stage: the base the atomic on count[q] returns is already a slot; a hit whose slot < cap writes
//          its key (brute_select_kernel's: monotone float bits high, row id low) to stage[q * cap + slot].  After this
//          ONE pass every query with count <= cap has its whole list staged.
//   PASS 2 refill: the same walk, blockIdx.x mapped through the compacted list of the query tiles that hold a query
//          with count > cap (built on the host from the counts it fetches for the lims anyway).  Every query of such a
//          tile is refilled from a zeroed slots[q] into keys[offset[q] + slot], each store guarded by slot < count[q],
//          the error flag raised otherwise.  Not launched when no tile overflowed.
//   unstage radius_unstage_kernel: a wave per query of the tiles NOT refilled copies stage[q * cap .. + count[q]] to
//          keys[offset[q] ..], two keys (16 bytes) a lane where source and destination are aligned alike.
// No store lands outside its segment: the stage write is guarded by slot < cap, the refill write by slot < count[q].
#include "probe_job.h"
#include "brute_tile.h"

#define RM_THREADS 256
#define RM_QT 128
#define RM_RB 128
#define RM_DS 64                            // halfs of a slab
#define RM_UR (RM_DS / 8)                   // 16-byte pieces of a slab of one row
#define RM_STRIDE (RM_DS * 2 + 16)          // bytes between two staged rows: 9 pieces
#define RM_NP (RM_RB * RM_UR / RM_THREADS)  // pieces a lane stages of the rows; of the two planes twice as many
#define RM_ATTR (128 * (16 * 4 + 8 + 4 + 4))    // tile_attr_bytes at its largest: 4 value columns, tags, exclude, group
static_assert(RM_DS % 16 == 0 && (RM_STRIDE / 16) % 2 == 1, "whole K steps; an odd stride in pieces");
static_assert(RM_NP * RM_THREADS == RM_RB * RM_UR && RM_QT == RM_RB && RM_QT == 128, "whole pieces a lane; tile_attr_bytes' 128 queries");
static_assert(3 * RM_RB * RM_STRIDE + RM_ATTR <= 64 * 1024, "static LDS");

typedef _Float16 rm_half8 __attribute__((ext_vector_type(8)));
typedef float rm_float16 __attribute__((ext_vector_type(16)));

template <bool RESTRICTED>
struct RmLds {
    unsigned char xh[RM_QT * RM_STRIDE], xl[RM_QT * RM_STRIDE];     // the tile's slab of x_hi (+ xn, 2^-e, radius) and x_lo
    unsigned char yr[RM_RB * RM_STRIDE];                            // the block's slab of the rows
    unsigned char attr[RESTRICTED ? RM_ATTR : 0];                   // the queries' attributes (tile_attr_bytes)
};

struct RmJob {
    TkBruteMatrix mx;
    int64_t nq;
    int d;
    const _Float16 *Y;              // rows [0, cols)
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

template <int PASS, bool RESTRICTED, typename U>
__device__ __forceinline__ void rm_walk(const RmJob &j, RmLds<RESTRICTED> &s)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = j.d, dpad = j.mx.dpad;
    const TkBruteRestrict &r = j.r;
    const int64_t q0 = (int64_t)(PASS == 2 ? j.tiles[blockIdx.x] : (int)blockIdx.x) * RM_QT;
    const int up = dpad / 8;                                            // pieces of a whole plane row
    const int NS = (d + RM_DS - 1) / RM_DS;                             // slabs
    // blockIdx.y's share of the columns, in whole blocks
    const int64_t per_y = ((j.cols + gridDim.y - 1) / gridDim.y + RM_RB - 1) / RM_RB * RM_RB;
    const int64_t c_begin = (int64_t)blockIdx.y * per_y;
    const int64_t ncols = c_begin + per_y < j.cols ? c_begin + per_y : j.cols;
    if (c_begin >= ncols) return;                                       // (the whole workgroup)
    const int64_t steps = (ncols - c_begin + RM_RB - 1) / RM_RB * NS;

    // what waits in LDS for the epilogue: (xn, 2^-e, radius) behind each query's x_hi slab, the attributes behind the
    // tiles (the arrays of tile_attr_bytes at their largest, each at a fixed place)
    int64_t *q_ranges = (int64_t *)s.attr;
    uint64_t *q_tags = (uint64_t *)(q_ranges + RM_QT * 8);
    int32_t *q_exclude = (int32_t *)(q_tags + RM_QT);
    int32_t *q_group = q_exclude + RM_QT;
    if (tid < RM_QT) {
        int64_t row = q0 + tid;
        row = row < j.nq ? row : j.nq - 1;
        float *pad = (float *)(s.xh + (tid & ~3) * RM_STRIDE + RM_DS * 2) + (tid & 3);
        pad[0] = j.mx.xn[row];
        pad[RM_STRIDE / 4] = j.mx.xs[row];
        pad[2 * RM_STRIDE / 4] = j.radius[row];
        if constexpr (RESTRICTED) {
            if (r.exclude) q_exclude[tid] = (int32_t)r.exclude[row];
            if (r.tags) q_tags[tid] = r.tags[row];
            if (r.group) q_group[tid] = r.group[row];
            for (int c = 0; c < 2 * r.cols; c++) q_ranges[tid * 8 + c] = r.ranges[row * 2 * r.cols + c];
        }
    }

    // a lane's pieces: row (or query) tid / 8 + 32 p of the block, piece tid % 8 of the slab
    uint4 ry[RM_NP], rx[2 * RM_NP];
    const int er = tid / RM_UR, ec = tid % RM_UR;
    const int qleft = (int)(j.nq - q0 < RM_QT ? j.nq - q0 : RM_QT);    // queries of the tile
    auto fetch_rows = [&](int64_t step) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
        const int64_t first = c_begin + b * RM_RB;
        const int left = (int)(ncols - first < RM_RB ? ncols - first : RM_RB);
        // (a base that is the same in every lane plus a 32-bit offset of the lane: 128 rows of d <= 4096 halfs)
        const _Float16 *yb = j.Y + first * d;
#pragma unroll
        for (int p = 0; p < RM_NP; p++) {
            unsigned at = (unsigned)(er + 32 * p) * (unsigned)d;
            asm volatile("" : "+v"(at));            // (one 32-bit offset: no 64-bit part of it is kept from step to step)
            ry[p] = er + 32 * p < left ? pm_row_piece<U>(yb + at, sl * RM_UR + ec, d) : make_uint4(0, 0, 0, 0);
        }
    };
    auto fetch_queries = [&](int sl) {              // entries 0 .. RM_QT - 1: x_hi, then x_lo
        const int c = sl * RM_UR + ec;
#pragma unroll
        for (int p = 0; p < 2 * RM_NP; p++) {
            const _Float16 *plane = (const _Float16 *)(p < RM_NP ? j.mx.xh : j.mx.xl) + q0 * dpad;
            unsigned at = (unsigned)(er + 32 * (p % RM_NP)) * (unsigned)dpad + (unsigned)c * 8u;
            asm volatile("" : "+v"(at));            // (one 32-bit offset: no 64-bit part of it is kept from step to step)
            rx[p] = (er + 32 * (p % RM_NP) < qleft && c < up) ? *(const uint4 *)(plane + at) : make_uint4(0, 0, 0, 0);
        }
    };
    auto commit = [&](bool queries) {
#pragma unroll
        for (int p = 0; p < RM_NP; p++) {
            const int e = tid + p * RM_THREADS;
            ((uint4 *)(s.yr + (e / RM_UR) * RM_STRIDE))[e % RM_UR] = ry[p];
        }
        if (queries) {
#pragma unroll
            for (int p = 0; p < 2 * RM_NP; p++) {
                const int e = tid + p * RM_THREADS, rr = e / RM_UR;
                ((uint4 *)((rr < RM_QT ? s.xh : s.xl) + (rr & (RM_QT - 1)) * RM_STRIDE))[e % RM_UR] = rx[p];
            }
        }
    };
    fetch_rows(0);
    fetch_queries(0);

    const int qh = wave & 1, rh = wave >> 1;        // the wave's quadrant
    const int half = lane >> 5, lc = lane & 31;     // the lane's half of a register (its query), its column
    const int koff = half * 16;                     // the lane's 8 halfs of a K step
    const unsigned char *pb = s.yr + (64 * rh + lc) * RM_STRIDE + koff;
    const unsigned char *ph = s.xh + (64 * qh + lc) * RM_STRIDE + koff;
    const unsigned char *pl = s.xl + (64 * qh + lc) * RM_STRIDE + koff;
    rm_float16 acc[2][2];                           // [query half][row half]
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
                const int64_t col = c_begin + b * RM_RB + 64 * rh + 32 * h + lc;
                row_ok[h] = col < ncols;
                yn[h] = row_ok[h] ? j.ynorm2[col] : 0.0f;
                if (h == 0) rid0 = (int32_t)col;
                if constexpr (RESTRICTED)
                    if (row_ok[h] && r.allowed) row_ok[h] = (r.allowed[col >> 5] >> (col & 31)) & 1u;
            }
        }
        // the slab's K steps: (x_hi + x_lo) . y into the four accumulators, hi before lo in each
        int nk = (dpad - sl * RM_DS) / 16;
        nk = nk < RM_DS / 16 ? nk : RM_DS / 16;
#pragma unroll 1
        for (int ks = 0; ks < nk; ks++) {
            const rm_half8 b0 = *(const rm_half8 *)(pb + ks * 32), b1 = *(const rm_half8 *)(pb + 32 * RM_STRIDE + ks * 32);
            const rm_half8 h0 = *(const rm_half8 *)(ph + ks * 32), h1 = *(const rm_half8 *)(ph + 32 * RM_STRIDE + ks * 32);
            const rm_half8 l0 = *(const rm_half8 *)(pl + ks * 32), l1 = *(const rm_half8 *)(pl + 32 * RM_STRIDE + ks * 32);
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
        // (opaque to the optimiser, as in bm_walk: it would otherwise keep what every register's query addresses alive
        // across the whole walk)
        asm volatile("" : "+v"(ul));
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int vg = 0; vg < 4; vg++) {
                // the four queries v & 3 of this group: one 16-byte read each of their xn, 2^-e and radius
                const int u0 = ul + 32 * a + 8 * vg;
                const unsigned char *pad = s.xh + u0 * RM_STRIDE + RM_DS * 2;
                const float4 gxn = *(const float4 *)pad, gxs = *(const float4 *)(pad + RM_STRIDE),
                             grad = *(const float4 *)(pad + 2 * RM_STRIDE);
                const float qxn[4] = {gxn.x, gxn.y, gxn.z, gxn.w}, qxs[4] = {gxs.x, gxs.y, gxs.z, gxs.w},
                            qrad[4] = {grad.x, grad.y, grad.z, grad.w};
#pragma unroll
                for (int vi = 0; vi < 4; vi++) {
                    const int v = 4 * vg + vi, ku = 32 * a + 8 * vg + vi, u = ul + ku;
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const float dot = acc[a][h][v] * qxs[vi];
                        const float rr = (qxn[vi] + yn[h]) - 2.0f * dot;
                        const float dm = rr > 0.0f ? rr : 0.0f;
                        bool hit = u < qleft && row_ok[h] && dm <= qrad[vi];
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
                                uint32_t k32 = __float_as_uint(dm);
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
__global__ __launch_bounds__(RM_THREADS, 2) void radius_matrix_tiles_kernel(const RmJob j)
{
    __shared__ __attribute__((aligned(16))) RmLds<RESTRICTED> s;
    if (j.d % 8 == 0) rm_walk<PASS, RESTRICTED, uint4>(j, s);
    else if (j.d % 4 == 0) rm_walk<PASS, RESTRICTED, uint2>(j, s);
    else rm_walk<PASS, RESTRICTED, _Float16>(j, s);
}

// A wave per query: stage[q * cap .. + count[q]] -> keys[offset[q] ..] for the queries of the tiles that were not
// refilled (refilled[q / 128] == 0; theirs all hold count <= cap).  Source and destination are 8-byte aligned; where
// both are odd one key is copied first, where both are then even two keys (16 bytes) a lane, else key by key.
__global__ __launch_bounds__(256) void radius_unstage_kernel(const unsigned long long *__restrict__ stage, int cap,
                                                             const int *__restrict__ count,
                                                             const int64_t *__restrict__ offset,
                                                             const int *__restrict__ refilled, int64_t nq,
                                                             unsigned long long *__restrict__ keys)
{
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq || refilled[q / RM_QT]) return;
    const int n = count[q] < cap ? count[q] : cap;      // (count <= cap in a tile that was not refilled)
    const int64_t src0 = q * cap, dst0 = offset[q];
    const unsigned long long *src = stage + src0;
    unsigned long long *dst = keys + dst0;
    if (((src0 ^ dst0) & 1) == 0) {
        const int head = (int)(src0 & 1) < n ? (int)(src0 & 1) : n;
        if (lane < head) dst[0] = src[0];
        const int pairs = (n - head) / 2;
        const ulonglong2 *s2 = (const ulonglong2 *)(src + head);
        ulonglong2 *d2 = (ulonglong2 *)(dst + head);
        for (int i = lane; i < pairs; i += 64) d2[i] = s2[i];
        if (lane == 0 && head + 2 * pairs < n) dst[n - 1] = src[n - 1];
    } else {
        for (int i = lane; i < n; i += 64) dst[i] = src[i];
    }
}

// a small kernel instead of a memset node: the counters of one call
__global__ void radius_matrix_zero_kernel(int *__restrict__ p, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

void tk_launch_radius_zero(int *p, int64_t n, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(radius_matrix_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n);
}

void tk_launch_radius_unstage(const unsigned long long *stage, int cap, const int *count, const int64_t *offset,
                              const int *refilled, int64_t nq, unsigned long long *keys, hipStream_t s)
{
    hipLaunchKernelGGL(radius_unstage_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, stage, cap, count, offset,
                       refilled, nq, keys);
}

template <int PASS>
static void rm_tiles(const RmJob &j, dim3 grid, bool restricted, hipStream_t s)
{
    if (restricted) hipLaunchKernelGGL((radius_matrix_tiles_kernel<PASS, true>), grid, dim3(RM_THREADS), 0, s, j);
    else hipLaunchKernelGGL((radius_matrix_tiles_kernel<PASS, false>), grid, dim3(RM_THREADS), 0, s, j);
}

// The first pass over Y (N, d) half, N < 2^31, d <= 4096: count (nq) is zeroed and takes every query's number of hits;
// stage == NULL: PASS 0, nothing else is written; else PASS 1 and stage (nq, cap) takes the first cap keys of every
// query.  mx: pm_prepare's planes of the nq queries; ynorm2 (N): brute_half_norms_kernel's.
int tk_launch_radius_matrix_count(const TkBruteMatrix &mx, int64_t nq, int d, const void *Y, int64_t N,
                                  const float *ynorm2, const float *radius, int *count, unsigned long long *stage,
                                  int cap, const TkBruteRestrict *r, hipStream_t s)
{
    if (nq <= 0) return 0;
    if (d > 4096 || N >= (1ll << 31) || (stage && (cap < 1 || cap > (1 << 20)))) return -1;
    tk_launch_radius_zero(count, nq, s);
    if (N <= 0) return 0;
    const RmJob j{mx, nq, d, (const _Float16 *)Y, ynorm2, N, radius, count, stage, stage ? cap : 0, nullptr, nullptr,
                  nullptr, nullptr, nullptr, r ? *r : TkBruteRestrict{}};
    const dim3 grid = brute_tile_grid(nq, N);
    if (stage) rm_tiles<1>(j, grid, r != nullptr, s);
    else rm_tiles<0>(j, grid, r != nullptr, s);
    return 0;
}

// Behind the first pass and the offsets: tiles (n_tiles) the query tiles to refill, ascending, refilled (ceil(nq / 128))
// 1 for each of them, both on the device.  PASS 2 over those tiles (slots (nq) and err (1) are zeroed here), then the
// unstage of every other query.  err != 0 afterwards: the passes disagreed (no store was made outside a segment).
int tk_launch_radius_matrix_fill(const TkBruteMatrix &mx, int64_t nq, int d, const void *Y, int64_t N,
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
        const RmJob j{mx, nq, d, (const _Float16 *)Y, ynorm2, N, radius, (int *)count, nullptr, 0, tiles, offset,
                      slots, keys, err, r ? *r : TkBruteRestrict{}};
        const dim3 grid(n_tiles, brute_tile_grid((int64_t)n_tiles * RM_QT, N).y);
        rm_tiles<2>(j, grid, r != nullptr, s);
    }
    tk_launch_radius_unstage(stage, cap, count, offset, refilled, nq, keys, s);
    return 0;
}
