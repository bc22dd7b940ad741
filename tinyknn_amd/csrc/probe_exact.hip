// probe_exact.hip — the exact k nearest rows among the rows of the lists each query probes (IVF.knn_probe,
// tk_index_knn_probe): FAISS's IVF-Flat search.  Probes, candidates, restrictions and distance are
// radius_probe.hip's (§3.20) word for word; the answer is the first k candidates ascending by (distance, row id), so it
// equals the first k entries of every list of radius_search(+inf, n_probes=P), ids and distance bits alike.
//
// radius_probe.hip is query-major: a workgroup per (query, rank), a lane per row, every lane fetching its own row — a
// list probed by 92 queries of a batch is read 92 times.  Here the distances are made LIST-major and selected
// QUERY-major:
//   segments  probe_len_kernel<1> (probe_job.h: the prologue radius_probe shares): per (query, rank) of the whole call
//             the keys its list needs — list_n, 0 at a rank whose list an earlier rank names or that names none.  tk_scan_exclusive64: where each (query, rank)'s segment of
//             distance keys begins.  The offsets cross to the host once: the call is cut into chunks of whole queries
//             whose key buffers fit the budget (workspace_bytes(); TK_OPT_PROBE_BUDGET for tests).
//   pairs     per chunk: pe_count_kernel counts the pairs (a (query, rank) with keys) per list with atomics,
//             tk_scan_exclusive gives every list's first pair and first tile, pe_fill_kernel writes the pairs through a
//             cursor (their order inside a list is whatever the atomics gave; nothing below depends on it),
//             pe_table_kernel cuts every list's pairs into tiles of at most QT: (list, first pair, count).
//   distance  probe_dist_kernel<T, TY>: a workgroup per tile.  The tile's queries go to LDS once, in T.  The list is
//             walked in blocks of RB rows: the labels of the block, then the rows themselves — 16-byte loads that run
//             contiguously across the lanes along a row (d * sizeof(TY) a multiple of 16; else element loads, equally
//             contiguous) — into LDS rows of an odd number of 16-byte pieces.  Then a lane takes one row of the block
//             and 4 of the tile's queries (sqdist_row4, sqdist_row.h: the row's pieces read once, four accumulator
//             sets, per query the rescoring's operations in the rescoring's order) and stores four keys, each at its
//             pair's segment + the row's position in the list: coalesced across the lanes.  A position whose label is
//             outside [0, N) gets the all-ones key; its row is never read.
//   select    probe_select_kernel<T>: a workgroup per query streams the key segments of its ranks beside the labels.  A
//             position is a candidate when its key is not all-ones, no copy of its label sits in a list of an earlier
//             rank (the twin table, radius_probe_count_kernel's rule) and it passes the restriction (by row id).
//             Candidates at or under the bound go to span_exact.h's candidate buffer (GX_CAP entries in LDS), cut to
//             the k best by (key, id) in front of a block that could overflow it.  No vector is read.
// LDS of the distance pass: QT * xstride * sizeof(T) + RB * (ystride + 4) + QT * 8 bytes <= 64 KiB, the most a workgroup
// gets without asking: xstride = d rounded up to a 16-byte multiple, ystride = the row's bytes rounded up to an ODD
// number of 16-byte pieces (lanes at consecutive rows read 16-byte pieces: with an odd stride in pieces any 8 — and any
// 16 — consecutive rows start in different 16-byte bank groups).  pe_tile picks RB (64 down to 8) as the largest for
// which 4 queries fit, QT as the most queries that fit beside it (a multiple of 4, at most 64), and doubles RB up to
// 256 while a full tile leaves room.  Assumed, not measured: that a CU's 160 KiB hold two or three such workgroups
// whose staging and arithmetic overlap; nothing is double-buffered inside one.
// Where not even 4 queries and 8 whole rows fit (d from 1 365 on float32 vectors, 2 041 on half, 683 on float64; up to
// 4 096) the distance pass is probe_dist_wide_kernel below: the same tiles, keys and places, d walked in slabs.
// The driver at the end of this file also serves the two matrix-core passes, which replace the distance kernel and
// nothing else: probe_matrix.hip (matrix=True, half rows, §3.22) and probe_f32.hip (wide=True, float32 rows, §3.27).
#include "probe_job.h"
#include "sqdist_row.h"
#include "span_exact.h"

__global__ __launch_bounds__(256) void pe_clear_kernel(int *__restrict__ a, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = 0;
}

__global__ __launch_bounds__(256) void pe_count_kernel(const PeJob j)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= j.n_pairs) return;
    const int64_t p = j.pair0 + i;
    if (j.seglen[p] > 0) atomicAdd(&j.count[probe_list(j.probes[p], j.n_lists)], 1);
}

__global__ __launch_bounds__(256) void pe_ntiles_kernel(const PeJob j)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l > j.n_lists) return;
    j.ntiles[l] = l < j.n_lists ? (j.count[l] + j.t.QT - 1) / j.t.QT : 0;      // (count[n_lists] stays 0: the totals)
}

__global__ __launch_bounds__(256) void pe_fill_kernel(const PeJob j)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= j.n_pairs) return;
    const int64_t p = j.pair0 + i;
    if (j.seglen[p] <= 0) return;
    const int32_t L = probe_list(j.probes[p], j.n_lists);
    const int slot = atomicAdd(&j.cursor[L], 1);
    if (slot < j.count[L]) j.pair_of[j.list_off[L] + slot] = (int)p;           // (always: the count pass saw the same)
}

__global__ __launch_bounds__(256) void pe_table_kernel(const PeJob j)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= j.n_lists) return;
    const int n = j.count[l], first = j.list_off[l], t0 = j.tile_off[l];
    for (int t = 0; t * j.t.QT < n; t++) {
        const int left = n - t * j.t.QT;
        j.tiles[t0 + t] = make_int4((int)l, first + t * j.t.QT, left < j.t.QT ? left : j.t.QT, 0);
    }
}

template <typename T, typename TY>
__global__ __launch_bounds__(PE_THREADS) void probe_dist_kernel(const PeJob j)
{
    typedef typename GxKey<T>::type K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int QT = j.t.QT, RB = j.t.RB, xstride = j.t.xstride, ystride = j.t.ystride, d = j.d;
    T *xq = (T *)smem;                                                  // QT queries, xstride apart
    unsigned char *yr = smem + (size_t)QT * xstride * sizeof(T);        // RB rows, ystride bytes apart
    int32_t *rid = (int32_t *)(yr + (size_t)RB * ystride);              // the block's labels, -1: no row
    long long *pseg = (long long *)(rid + RB);                          // where each query's keys of this list begin
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= j.tile_off[j.n_lists]) return;               // (the grid is an upper bound of the tiles)
    const int4 tile = j.tiles[blockIdx.x];
    const int32_t L = tile.x;
    const int first = tile.y, cnt = tile.z;
    for (int e = tid; e < cnt * xstride; e += PE_THREADS) {
        const int u = e / xstride, c = e - u * xstride;
        const int64_t qi = j.pair_of[first + u] / j.kc;
        xq[e] = c < d ? (T)j.q[qi * d + c] : (T)0;
    }
    for (int u = tid; u < cnt; u += PE_THREADS) pseg[u] = j.segoff[j.pair_of[first + u]] - j.seg_base;
    const int64_t n = j.list_n[L], base = j.ids_off[L];
    const TY *rows = (const TY *)j.rows;
    K *keys = (K *)j.keys;
    const int QG = (cnt + 3) >> 2;
    const bool quads = ((size_t)d * sizeof(TY)) % 16 == 0;
    const int nqd = (int)((size_t)d * sizeof(TY) / 16);
    for (int64_t r0 = 0; r0 < n; r0 += RB) {
        __syncthreads();                            // the last block's arithmetic is done with yr and rid
        for (int e = tid; e < RB; e += PE_THREADS) {
            const int64_t id = r0 + e < n ? j.ids[base + r0 + e] : -1;
            rid[e] = (id >= 0 && id < j.N) ? (int32_t)id : -1;
        }
        __syncthreads();
        if (quads) {
            for (int e = tid; e < RB * nqd; e += PE_THREADS) {
                const int rr = e / nqd, c = e - rr * nqd;
                const int32_t id = rid[rr];
                if (id >= 0) ((uint4 *)(yr + (size_t)rr * ystride))[c] = ((const uint4 *)(rows + (int64_t)id * d))[c];
            }
        } else {
            for (int e = tid; e < RB * d; e += PE_THREADS) {
                const int rr = e / d, c = e - rr * d;
                const int32_t id = rid[rr];
                if (id >= 0) ((TY *)(yr + (size_t)rr * ystride))[c] = rows[(int64_t)id * d + c];
            }
        }
        __syncthreads();                            // (the first time also: xq and pseg)
        for (int item = tid; item < RB * QG; item += PE_THREADS) {
            const int rr = item & (RB - 1), qg = item / RB;
            const int64_t pos = r0 + rr;
            if (pos >= n) continue;
            const int u0 = qg * 4;
            T dv[4];
            const bool stored = rid[rr] >= 0;
            if (stored) {
                const T *x[4];
#pragma unroll
                for (int u = 0; u < 4; u++) x[u] = xq + (size_t)(u0 + u < cnt ? u0 + u : u0) * xstride;
                sqdist_row4<T, TY>((const TY *)(yr + (size_t)rr * ystride), x, d, dv);
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (u0 + u < cnt) keys[pseg[u0 + u] + pos] = stored ? GxKey<T>::of(dv[u]) : ~(K)0;
        }
    }
}

// ---- the wide distance kernel: d walked in slabs (d beyond what probe_dist_kernel's LDS holds) ----
// A tile is PEW_QT queries, a block PEW_RB rows, a slab DS = 32 * L elements (128 floats, 64 doubles: a multiple of
// sqdist_row's group of 4 * L, so a slab edge falls between two iterations of its main loop).  LDS holds one slab of
// the queries (T) and one slab of the rows (TY, DS * sizeof(TY) + 16 bytes apart: an odd number of 16-byte pieces), the
// labels of two blocks and per query its row of q and its key segment — static, the compiler reports it.  The walk is
// one loop over (block, slab) steps: the next step's global loads go into registers (fetch) while this step's slab is
// summed, and are written to LDS (commit) between the two barriers of the next step.  A lane owns one row of the block
// and the PEW_NI query quads  wave, wave + 4, ...  for the whole walk over d: PEW_NI * 4 * L accumulators in registers
// from slab to slab, the row's pieces read once a group for all its quads, the queries' pieces LDS broadcasts.
#define PEW_QT 32
#define PEW_RB 64
#define PEW_NI (PEW_RB * PEW_QT / 4 / PE_THREADS)
static_assert(PEW_RB == 64 && PEW_NI * 4 * PE_THREADS == PEW_RB * PEW_QT, "a wave is one block of rows; whole items a lane");

template <typename T> struct PeWide {
    static constexpr int L = 16 / (int)sizeof(T);
    static constexpr int DS = 32 * L;
};

template <typename T, typename TY>
struct PeWideLds {
    static constexpr int DS = PeWide<T>::DS, YS = DS * (int)sizeof(TY) + 16;
    T xq[PEW_QT * DS];
    unsigned char yr[PEW_RB * YS];
    int32_t rid[2][PEW_RB];         // the labels of this block and the next, -1: no row
    long long pseg[PEW_QT];         // where each query's keys of this list begin
    int64_t qrow[PEW_QT];           // each query's row of q
};

// QUADS: d * sizeof(TY) is a multiple of 16, rows are staged in 16-byte pieces; else element by element
template <typename T, typename TY, bool QUADS>
__device__ __forceinline__ void pe_wide_walk(const PeJob &j, PeWideLds<T, TY> &s, const int4 tile)
{
    typedef typename GxKey<T>::type K;
    typedef typename std::conditional<QUADS, uint4, TY>::type U;        // what a lane fetches of the rows
    constexpr int L = PeWide<T>::L, DS = PeWide<T>::DS, YS = PeWideLds<T, TY>::YS;
    constexpr int UR = DS * (int)sizeof(TY) / (int)sizeof(U);           // units of a row's slab
    constexpr int NU = PEW_RB * UR / PE_THREADS, NX = PEW_QT * DS / PE_THREADS;
    const int tid = threadIdx.x, d = j.d, cnt = tile.z;
    const int64_t n = j.list_n[tile.x], base = j.ids_off[tile.x];
    const int ud = QUADS ? (int)((size_t)d * sizeof(TY) / 16) : d;      // units of a whole row
    const int NS = (d + DS - 1) / DS, G = d / (4 * L);                  // slabs; whole groups of a row
    const int64_t steps = (n + PEW_RB - 1) / PEW_RB * NS;
    const TY *rows = (const TY *)j.rows;
    K *keys = (K *)j.keys;
    const int rr = tid & (PEW_RB - 1);                                  // the lane's row of every block
    bool on[PEW_NI];
    const T *x[PEW_NI][4];
#pragma unroll
    for (int it = 0; it < PEW_NI; it++) {
        const int u0 = (tid / PEW_RB + it * (PE_THREADS / PEW_RB)) * 4;
        on[it] = u0 < cnt;
#pragma unroll
        for (int u = 0; u < 4; u++) x[it][u] = s.xq + (u0 + u < cnt ? u0 + u : 0) * DS;
    }
    U ry[NU];
    float rx[NX];
    auto label = [&](int64_t pos) -> int32_t {
        const int64_t id = pos < n ? j.ids[base + pos] : -1;
        return (id >= 0 && id < j.N) ? (int32_t)id : -1;
    };
    auto fetch = [&](int64_t step) {                // the step's slab of the block's rows and of the tile's queries
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
#pragma unroll
        for (int p = 0; p < NU; p++) {
            const int e = tid + p * PE_THREADS, r = e / UR, c = sl * UR + e % UR;
            const int32_t id = s.rid[b & 1][r];
            U v = U();
            if (id >= 0 && c < ud) v = ((const U *)(rows + (int64_t)id * d))[c];
            ry[p] = v;
        }
#pragma unroll
        for (int p = 0; p < NX; p++) {
            const int e = tid + p * PE_THREADS, u = e / DS, c = sl * DS + e % DS;
            rx[p] = (u < cnt && c < d) ? j.q[s.qrow[u] * d + c] : 0.0f;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int p = 0; p < NU; p++) {
            const int e = tid + p * PE_THREADS;
            ((U *)(s.yr + (size_t)(e / UR) * YS))[e % UR] = ry[p];
        }
#pragma unroll
        for (int p = 0; p < NX; p++) s.xq[tid + p * PE_THREADS] = (T)rx[p];
    };

    for (int u = tid; u < cnt; u += PE_THREADS) {
        const int pr = j.pair_of[tile.y + u];
        s.pseg[u] = j.segoff[pr] - j.seg_base;
        s.qrow[u] = pr / j.kc;
    }
    if (tid < PEW_RB) s.rid[0][tid] = label(tid);
    __syncthreads();
    if (steps > 0) fetch(0);
    T acc[PEW_NI][4][L];
    bool stored = false;
    for (int64_t step = 0; step < steps; step++) {
        const int64_t b = step / NS;
        const int sl = (int)(step - b * NS);
        const bool last = sl == NS - 1;
        int32_t next = -1;
        if (last && tid < PEW_RB) next = label((b + 1) * PEW_RB + tid);
        __syncthreads();                            // the last step's arithmetic is done with xq and yr
        commit();
        if (last && tid < PEW_RB) s.rid[(b + 1) & 1][tid] = next;      // (read again two blocks on, behind barriers)
        __syncthreads();
        if (step + 1 < steps) fetch(step + 1);
        const int64_t pos = b * PEW_RB + rr;
        if (sl == 0) {
            stored = pos < n && s.rid[b & 1][rr] >= 0;
            sq4_init<T, PEW_NI>(acc);
        }
        const TY *y = (const TY *)(s.yr + (size_t)rr * YS);
        int ng = G - sl * (DS / (4 * L));
        ng = ng < 0 ? 0 : ng < DS / (4 * L) ? ng : DS / (4 * L);
        if (stored) sq4_groups<T, TY, PEW_NI>(y, x, on, ng, acc);
        if (!last) continue;
        T dv[PEW_NI][4];
        if (stored) {
            sq4_tail<T, TY, PEW_NI>(y, x, on, ng * 4 * L, d - G * 4 * L, acc);
            sq4_finish<T, PEW_NI>(acc, dv);
        }
        if (pos < n)
#pragma unroll
            for (int it = 0; it < PEW_NI; it++) {
                const int u0 = (tid / PEW_RB + it * (PE_THREADS / PEW_RB)) * 4;
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (u0 + u < cnt) keys[s.pseg[u0 + u] + pos] = stored ? GxKey<T>::of(dv[it][u]) : ~(K)0;
            }
    }
}

template <typename T, typename TY>
__global__ __launch_bounds__(PE_THREADS) void probe_dist_wide_kernel(const PeJob j)
{
    __shared__ __attribute__((aligned(16))) PeWideLds<T, TY> s;
    if ((int)blockIdx.x >= j.tile_off[j.n_lists]) return;               // (the grid is an upper bound of the tiles)
    const int4 tile = j.tiles[blockIdx.x];
    if (((size_t)j.d * sizeof(TY)) % 16 == 0) pe_wide_walk<T, TY, true>(j, s, tile);
    else pe_wide_walk<T, TY, false>(j, s, tile);
}

// LDS: kd[GX_CAP] distance keys | kid[GX_CAP] row ids | pl[kc] the lists of the query's ranks
static size_t pe_select_lds(int kc, size_t key_bytes) { return (size_t)GX_CAP * (key_bytes + 4) + (size_t)kc * 4; }

template <typename T>
__global__ __launch_bounds__(GX_THREADS) void probe_select_kernel(const PeJob j, const TkBruteRestrict r,
                                                                  const int64_t q0, const int k,
                                                                  int64_t *__restrict__ out, T *__restrict__ out_d)
{
    typedef typename GxKey<T>::type K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    K *kd = (K *)smem;
    int32_t *kid = (int32_t *)(kd + GX_CAP);
    int32_t *pl = kid + GX_CAP;
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int64_t qi = q0 + blockIdx.x;
    for (int t = tid; t < j.kc; t += GX_THREADS) pl[t] = probe_list(j.probes[qi * j.kc + t], j.n_lists);
    if (tid == 0) s_count = 0;
    // the query's own attributes, once
    const int32_t q_ex = r.exclude ? (int32_t)r.exclude[qi] : -1;
    const uint64_t q_tags = r.tags ? r.tags[qi] : 0;
    const int32_t q_group = r.group ? r.group[qi] : -1;
    int64_t q_lo[4] = {0, 0, 0, 0}, q_hi[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (c < r.cols) {
            q_lo[c] = r.ranges[(qi * r.cols + c) * 2];
            q_hi[c] = r.ranges[(qi * r.cols + c) * 2 + 1];
        }
    K tau = ~(K)0;          // the bound: the k-th distance key of the last cut
    int kept = 0;           // entries the buffer holds at most (an upper bound, the same in every lane)

    // span_exact.h's cut: sort what the buffer holds by (distance, row id), keep the k best, tighten the bound
    auto cut = [&]() {
        __syncthreads();
        const int nc = s_count < GX_CAP ? s_count : GX_CAP;
        int P = 1;
        while (P < nc) P <<= 1;
        for (int e = nc + tid; e < P; e += GX_THREADS) {
            kd[e] = ~(K)0;
            kid[e] = 0x7fffffff;
        }
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int e = tid; e < P / 2; e += GX_THREADS) {
                    const int lo = (e / stride) * 2 * stride + (e % stride), hi = lo + stride;
                    const bool up = (lo & size) == 0;
                    const K a = kd[lo], b = kd[hi];
                    const int32_t ia = kid[lo], ib = kid[hi];
                    const bool gt = a > b || (a == b && ia > ib);
                    if (gt == up) {
                        kd[lo] = b; kd[hi] = a;
                        kid[lo] = ib; kid[hi] = ia;
                    }
                }
                __syncthreads();
            }
        kept = nc < k ? nc : k;
        if (nc >= k) tau = kd[k - 1];
        if (tid == 0) s_count = kept;
        __syncthreads();
    };

    __syncthreads();                                // pl and the zero count
    const K *keys = (const K *)j.keys;
    for (int rank = 0; rank < j.kc; rank++) {
        const int64_t p = qi * j.kc + rank;
        const int64_t len = j.seglen[p];
        if (len <= 0) continue;                     // (the same in every lane)
        const int64_t base = j.ids_off[pl[rank]];
        const K *seg = keys + (j.segoff[p] - j.seg_base);
        for (int64_t t0 = 0; t0 < len; t0 += GX_TILE) {
            if (kept + GX_TILE > GX_CAP) cut();
            kept += GX_TILE;
            const int64_t pos = t0 + tid;
            if (pos >= len) continue;
            const K key = seg[pos];
            if (key == ~(K)0 || key > tau) continue;
            const int64_t flat = base + pos;
            const int32_t rid = (int32_t)j.ids[flat];
            bool ok = true;
            for (int u = 0; u < j.twin_w; u++) {    // a copy in a list of an earlier rank: a candidate there
                const int32_t l2 = j.twin_list[flat * j.twin_w + u];
                if (l2 < 0) break;
                for (int t = 0; t < rank; t++) ok &= pl[t] != l2;
            }
            if (r.allowed) ok &= (r.allowed[rid >> 5] >> (rid & 31)) & 1u;
            ok &= rid != q_ex;
            if (ok && q_group >= 0) ok = r.row_groups[rid] == q_group;
            if (ok && q_tags != 0) {
                const uint64_t rt = r.row_tags[rid];
                ok = r.tag_mode ? (rt & q_tags) == q_tags : (rt & q_tags) != 0;
            }
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (ok && c < r.cols) {
                    const int64_t v = r.row_keys[c * r.n_rows + rid];
                    ok = q_lo[c] <= v && v <= q_hi[c];
                }
            if (!ok) continue;
            const int at = atomicAdd(&s_count, 1);
            if (at < GX_CAP) {                      // (always: kept bounds the count)
                kd[at] = key;
                kid[at] = rid;
            }
        }
    }
    cut();
    for (int e = tid; e < k; e += GX_THREADS) {
        out[qi * k + e] = e < kept ? (int64_t)kid[e] : -1;
        out_d[qi * k + e] = e < kept ? GxKey<T>::back(kd[e]) : (T)__builtin_huge_valf();
    }
}

// ---- launch ----

static size_t pe_lds(const PeTile &t, int QT, int RB, size_t tb)
{
    return (size_t)QT * t.xstride * tb + (size_t)RB * (t.ystride + 4) + (size_t)QT * 8;
}

// QT, RB and the strides for the index's d and store; false: not even 4 queries and 8 rows fit
static bool pe_tile_for(int d, size_t tb, size_t yb, PeTile &t)
{
    const int L = (int)(16 / tb);
    t.xstride = (d + L - 1) / L * L;
    t.ystride = (int)((((size_t)d * yb + 15) / 16) | 1) * 16;
    t.QT = 0;
    for (t.RB = 64; t.RB >= 8; t.RB >>= 1) {
        const long long room = (long long)PE_LDS_LIMIT - (long long)t.RB * (t.ystride + 4);
        const long long fit = room > 0 ? room / (long long)((size_t)t.xstride * tb + 8) : 0;
        t.QT = (int)(fit < PE_QT_MAX ? fit / 4 * 4 : PE_QT_MAX);
        if (t.QT >= 4) break;
    }
    if (t.QT < 4) return false;
    while (t.QT == PE_QT_MAX && t.RB < 256 && pe_lds(t, t.QT, t.RB * 2, tb) <= PE_LDS_LIMIT) t.RB *= 2;
    t.lds = pe_lds(t, t.QT, t.RB, tb);
    return true;
}

// the tile of the call: probe_dist_kernel's where the whole rows fit its LDS (and TK_OPT_PROBE_WIDE does not ask
// otherwise), else the wide kernel's fixed one
static int pe_tile(const tk_index *ix, PeTile &t)
{
    ARGCHECK(ix->d <= 4096, "d <= 4096");
    const bool f64 = ix->data_dtype == TK_DATA_F64;
    const size_t tb = f64 ? 8 : 4, yb = data_esz(ix->data_dtype);
    t.DS = 0;
    if (!ix->opt_probe_wide && pe_tile_for(ix->d, tb, yb, t)) return TK_OK;
    t.QT = PEW_QT;
    t.RB = PEW_RB;
    t.DS = f64 ? PeWide<double>::DS : PeWide<float>::DS;
    t.xstride = t.DS;
    t.ystride = t.DS * (int)yb + 16;
    t.lds = f64 ? sizeof(PeWideLds<double, double>)
                : yb == 2 ? sizeof(PeWideLds<float, _Float16>) : sizeof(PeWideLds<float, float>);
    return TK_OK;
}

// mx / wd: the queries of the f16 / f32 matrix pass where the call takes one (pe_knn_probe), else NULL
template <typename T, typename TY>
static void pe_launch(const PeJob &j, const PmQueries *mx, const TkBruteWide *wd, unsigned max_tiles,
                      const TkBruteRestrict &r, int64_t q0, int64_t m, int k, int64_t *out, void *out_d)
{
    typedef typename GxKey<T>::type K;
    if (mx) pm_launch_dist(j, *mx, max_tiles);      // (float keys on half rows)
    else if (wd) pf_launch_dist(j, *wd, max_tiles); // (float keys on float rows)
    else if (j.t.DS) hipLaunchKernelGGL((probe_dist_wide_kernel<T, TY>), dim3(max_tiles), dim3(PE_THREADS), 0, 0, j);
    else hipLaunchKernelGGL((probe_dist_kernel<T, TY>), dim3(max_tiles), dim3(PE_THREADS), j.t.lds, 0, j);
    hipLaunchKernelGGL((probe_select_kernel<T>), dim3((unsigned)m), dim3(GX_THREADS), pe_select_lds(j.kc, sizeof(K)), 0,
                       j, r, q0, k, out, (T *)out_d);
}

static int pe_scan(tk_index *ix, const int *in, int *out, int64_t n)
{
    size_t bytes = 0;
    (void)tk_scan_exclusive(nullptr, &bytes, in, out, n, nullptr);
    TRY(ix->pl_scan.ensure(bytes > 0 ? bytes : 1));
    if (tk_scan_exclusive(ix->pl_scan.p, &bytes, in, out, n, nullptr))
        return fail(TK_ERR_HIP, "tk_scan_exclusive failed");
    return TK_OK;
}

// ---- C ABI ----

extern "C" int tk_index_knn_probe_tile(tk_index *ix, int *qt, int *rb)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data && qt && rb, "set_data first");
    PeTile t;
    TRY(pe_tile(ix, t));
    *qt = t.QT;
    *rb = t.RB;
    return TK_OK;
}

// the distance pass of a call: the exact one, probe_matrix.hip's (matrix=True) or probe_f32.hip's (wide=True)
enum PePass { PE_EXACT, PE_F16_MATRIX, PE_F32_MATRIX };

// the body of tk_index_knn_probe, tk_index_knn_probe_matrix and tk_index_knn_probe_wide
static int pe_knn_probe(tk_index *ix, PePass pass, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq, int k,
                        int n_probes, const TkHostRestrict &h, int64_t *out_ids, void *out_dist)
{
    IXLOCK(ix);
    ARGCHECK(ix && ix->have_data && ix->have_lists && ix->have_pq && ix->have_centers,
             "set_pq, set_centers, set_lists and set_data first");
    ARGCHECK(!ix->sharded, "list-sharded index: knn_probe is not supported");
    ARGCHECK(k >= 1 && k <= 1024, "1 <= k <= 1024");
    ARGCHECK(n_probes >= 1, "n_probes >= 1");
    ARGCHECK(ix->N < (1ll << 31), "N < 2^31");
    PeTile tile;
    TRY(pe_tile(ix, tile));
    ARGCHECK(nq >= 0 && (nq == 0 || (q && q_pq && out_ids)), "buffers");
    if (pass == PE_F16_MATRIX) {
        TRY(pm_check(ix, q, nq));
        pm_tile(tile);
    } else if (pass == PE_F32_MATRIX) {
        TRY(pf_check(ix));
        pf_tile(tile);
    }
    const int32_t *twin_list = nullptr;
    int twin_w = 0;
    TRY(radius_probe_twins(ix, &twin_list, &twin_w));
    TkBruteRestrict r;
    bool any;
    TRY(brute_restrict(ix, nq, h, r, any));
    if (nq == 0) return TK_OK;
    TRY(flush_pending(ix));
    const bool f64 = ix->data_dtype == TK_DATA_F64;
    const size_t ksz = f64 ? 8 : 4;
    int kc;
    TRY(probe_pairs(ix, nq, n_probes, kc));
    const int64_t pairs = nq * kc;
    ARGCHECK(pe_select_lds(kc, ksz) <= 64 * 1024, "n_probes: the probed lists of a query do not fit 64 KiB of LDS");
    TRY(ix->pe_lists.ensure((size_t)(ix->n_lists + 1) * 5 * 4));
    TRY(ix->pe_out.ensure((size_t)nq * k * (8 + ksz)));
    PeJob j{};
    // the coarse stage; the keys of every (query, rank) and where they begin
    TRY(probe_lengths<1>(ix, "knn_probe", q, q_pq, q_pq_is_f64, nq, n_probes, kc, twin_list, twin_w, j));
    PmQueries mx{};
    if (pass == PE_F16_MATRIX) TRY(pm_prepare(ix, nq, mx));
    const int dq = tk_brute_wide_dq(ix->d);
    if (pass == PE_F32_MATRIX) {
        TRY(ix->bw_x2.ensure((size_t)nq * dq * 4));
        TRY(ix->bw_xn.ensure((size_t)nq * 4));
        tk_launch_brute_wide_prepare(ix->br_q.as<float>(), nq, ix->d, ix->bw_x2.as<float>(), ix->bw_xn.as<float>(), nullptr);
    }
    const TkBruteWide wd{ix->bw_x2.as<float>(), ix->bw_xn.as<float>(), dq};
    const long long *segoff = ix->pl_off.as<long long>();
    std::vector<long long> off((size_t)pairs + 1);
    HIPCHECK(hipMemcpy(off.data(), segoff, (size_t)(pairs + 1) * 8, hipMemcpyDeviceToHost));      // (synchronises)
    // chunks of whole queries whose keys fit the budget
    const double budget = ix->opt_probe_budget > 0 ? (double)ix->opt_probe_budget : workspace_bytes();
    for (int64_t i = 0; i < nq; i++) {
        const long long need = (off[(size_t)((i + 1) * kc)] - off[(size_t)(i * kc)]) * (long long)ksz;
        if ((double)need > budget) {
            char b[240];
            snprintf(b, sizeof b, "knn_probe: the distance keys of query %lld alone need %lld bytes, more than the "
                                  "workspace budget of %.0f bytes; ask fewer probes", (long long)i, need, budget);
            return fail(TK_ERR_WORKSPACE, b);
        }
    }
    j.seglen = ix->pl_len.as<long long>();
    j.segoff = segoff;
    const int64_t nl1 = ix->n_lists + 1;
    j.count = ix->pe_lists.as<int>();
    j.cursor = j.count + nl1;
    j.list_off = j.cursor + nl1;
    j.ntiles = j.list_off + nl1;
    j.tile_off = j.ntiles + nl1;
    j.t = tile;
    int64_t *out = ix->pe_out.as<int64_t>();
    void *out_d = (void *)(out + nq * k);
    const unsigned lgrid = (unsigned)((nl1 + 255) / 256);
    for (int64_t o = 0; o < nq;) {
        int64_t e = o + 1;
        while (e < nq && (double)((off[(size_t)((e + 1) * kc)] - off[(size_t)(o * kc)]) * (long long)ksz) <= budget) e++;
        const int64_t m = e - o;
        j.pair0 = o * kc;
        j.n_pairs = m * kc;
        j.seg_base = off[(size_t)j.pair0];
        const long long n_keys = off[(size_t)(e * kc)] - j.seg_base;
        const int64_t max_tiles = j.n_pairs / tile.QT + (j.n_pairs < ix->n_lists ? j.n_pairs : ix->n_lists);
        TRY(ix->pe_keys.ensure((size_t)(n_keys > 0 ? n_keys : 1) * ksz));
        TRY(ix->pe_pairs.ensure((size_t)j.n_pairs * 4));
        TRY(ix->pe_tiles.ensure((size_t)(max_tiles > 0 ? max_tiles : 1) * 16));
        j.keys = ix->pe_keys.p;
        j.pair_of = ix->pe_pairs.as<int>();
        j.tiles = ix->pe_tiles.as<int4>();
        const unsigned pgrid = (unsigned)((j.n_pairs + 255) / 256);
        hipLaunchKernelGGL(pe_clear_kernel, dim3((unsigned)((2 * nl1 + 255) / 256)), dim3(256), 0, 0, j.count, 2 * nl1);
        hipLaunchKernelGGL(pe_count_kernel, dim3(pgrid), dim3(256), 0, 0, j);
        hipLaunchKernelGGL(pe_ntiles_kernel, dim3(lgrid), dim3(256), 0, 0, j);
        TRY(pe_scan(ix, j.count, j.list_off, nl1));
        TRY(pe_scan(ix, j.ntiles, j.tile_off, nl1));
        hipLaunchKernelGGL(pe_fill_kernel, dim3(pgrid), dim3(256), 0, 0, j);
        hipLaunchKernelGGL(pe_table_kernel, dim3(lgrid), dim3(256), 0, 0, j);
        if (f64) pe_launch<double, double>(j, nullptr, nullptr, (unsigned)max_tiles, r, o, m, k, out, out_d);
        else if (ix->data_dtype == TK_DATA_F16)
            pe_launch<float, _Float16>(j, pass == PE_F16_MATRIX ? &mx : nullptr, nullptr, (unsigned)max_tiles, r, o, m, k,
                                       out, out_d);
        else
            pe_launch<float, float>(j, nullptr, pass == PE_F32_MATRIX ? &wd : nullptr, (unsigned)max_tiles, r, o, m, k, out,
                                    out_d);
        HIPCHECK(hipGetLastError());
        o = e;
    }
    HIPCHECK(hipMemcpy(out_ids, out, (size_t)nq * k * 8, hipMemcpyDeviceToHost));                 // (synchronises)
    if (out_dist) HIPCHECK(hipMemcpy(out_dist, out_d, (size_t)nq * k * ksz, hipMemcpyDeviceToHost));
    return TK_OK;
}

extern "C" int tk_index_knn_probe(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq, int k,
                                  int n_probes, const uint8_t *allowed_mask, const int64_t *exclude,
                                  const int32_t *group, const uint64_t *tags, int tag_mode, const int64_t *between,
                                  int64_t *out_ids, void *out_dist)
{
    return pe_knn_probe(ix, PE_EXACT, q, q_pq, q_pq_is_f64, nq, k, n_probes,
                        {allowed_mask, exclude, group, tags, tag_mode, between}, out_ids, out_dist);
}

extern "C" int tk_index_knn_probe_matrix(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq,
                                         int k, int n_probes, const uint8_t *allowed_mask, const int64_t *exclude,
                                         const int32_t *group, const uint64_t *tags, int tag_mode,
                                         const int64_t *between, int64_t *out_ids, void *out_dist)
{
    return pe_knn_probe(ix, PE_F16_MATRIX, q, q_pq, q_pq_is_f64, nq, k, n_probes,
                        {allowed_mask, exclude, group, tags, tag_mode, between}, out_ids, out_dist);
}

extern "C" int tk_index_knn_probe_wide(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq, int k,
                                       int n_probes, const uint8_t *allowed_mask, const int64_t *exclude,
                                       const int32_t *group, const uint64_t *tags, int tag_mode, const int64_t *between,
                                       int64_t *out_ids, void *out_dist)
{
    return pe_knn_probe(ix, PE_F32_MATRIX, q, q_pq, q_pq_is_f64, nq, k, n_probes,
                        {allowed_mask, exclude, group, tags, tag_mode, between}, out_ids, out_dist);
}
