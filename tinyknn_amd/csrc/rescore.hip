// rescore.hip — exact second pass on gfx950.
//
// Replaces knn_brute1 + bottom_k (utils.py:89-92, 22-25) as used by
// _FastDistanceTable.top (fast_pq.py:307-312, coarse stage) and IVF.query
// (ivf.py:154-163, final stage), and turns the coarse result into the per-slot
// scan descriptors of the list scan.
//
// Distances restate numpy's einsum("ij,ij->i") rounding (SSE3 baseline: 16-byte
// vectors = 4 float32 or 2 float64 lanes, un-fused multiply-add, 4-vector groups
// folded 3,2,1,0, zero-filled tail vector, pairwise horizontal add); float32 when
// both the vectors and the query are float32, float64 otherwise (numpy's
// promotion of `Y - x`); built with -ffp-contract=off.  One lane owns one
// candidate row and carries the lane-accumulators.  The k best are returned in ascending distance (ties:
// lower candidate position first) — the order numpy's argpartition yields on the
// fixture host for these sizes; a rank-by-counting pass in LDS does the ordering.
#include <stdlib.h>
#include <string.h>

#include <type_traits>
#include "kernels.h"
#include "sqdist_row.h"

// A wave-uniform value of the capped epilogue made HERE and kept in VECTOR registers (no instruction is emitted).  The
// capped kernels carry four more arguments than the distance forms, which use 97 of the 102 scalar registers: left to
// itself the compiler keeps every argument a per-query pointer is made of alive through the sums and, in the staged
// kernels, parks 4 scalars in vector lanes.  The epilogue uses these values per lane anyway (store addresses, a
// gather's base, a compare).
#define HELD(x) asm volatile("" : "+v"(x))

// LDS: cand[R] (int64) | dist[R] (T) | x[d] (T)
// DIST: also write the distance of every id written to out_d (second call of a pair: out_d_b; either may be NULL),
// +inf beside a -1; where the heap holds <= k ids (no rescoring) their rows are read for it.  The ids-only kernels
// below are this body with DIST = false, unchanged.
// CAP (per_group=, cap_select.h): every candidate goes to its rank in LDS behind x[] — id | distance | group, the
// group read by the row id the vector is fetched by — and cap_select writes the row; where the heap holds <= k ids the
// rank is the position.  LDS: ... | x[d] | up to 8 bytes of padding | CapRanked<T>(R)
template <typename T, typename TY, typename TX, bool DIST, bool CAP = false>
__device__ __forceinline__ void rescore_body(unsigned char *smem, const TX *__restrict__ q, int d,
                                             const TY *__restrict__ rows, int64_t n_rows,
                                             const int64_t *__restrict__ cand, int R, int k, int strip,
                                             int64_t *__restrict__ out, int *__restrict__ out_count,
                                             const TX *__restrict__ q_b, int64_t q_na, int64_t *__restrict__ out_b,
                                             int64_t out_na, T *__restrict__ out_d, T *__restrict__ out_d_b,
                                             const TkCap &cap = TkCap())
{
    int64_t *cs = (int64_t *)smem;
    T *ds = (T *)(smem + (size_t)R * 8);
    T *xs = ds + R;
    const CapRanked<T> by(CAP ? smem + (((size_t)R * 8 + ((size_t)R + d) * sizeof(T) + 7) & ~(size_t)7) : nullptr, R);
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const int64_t *c = cand + qi * R;
    unsigned capm = 0;
    const int32_t *groups = CAP ? cap.groups : nullptr;     // (the epilogue's scalars: read here, kept in vector registers)
    if (CAP) capm = cap_of(cap, qi);

    const TX *qrow = (q_b && qi >= q_na) ? q_b + (qi - q_na) * d : q + qi * d;   // second call of a pair
    for (int t = tid; t < d; t += blockDim.x) xs[t] = (T)qrow[t];
    // ordered compaction of the candidate ids (ivf.py:154-155 drops -1)
    if (tid < 64) {
        int base = 0;
        for (int t0 = 0; t0 < R; t0 += 64) {
            int t = t0 + tid;
            int64_t id = t < R ? c[t] : -1;
            bool keep = t < R && (!strip || id != -1);
            uint64_t m = __builtin_amdgcn_ballot_w64(keep);
            int before = __builtin_popcountll(m & ((1ull << tid) - 1ull));
            if (keep) cs[base + before] = id;
            base += __builtin_popcountll(m);
        }
        if (tid == 0) s_count = base;
    }
    __syncthreads();
    const int nc = s_count;
    const bool second = out_b && qi >= out_na;
    int64_t *o = second ? out_b + (qi - out_na) * k : out + qi * k;
    T *od = nullptr;
    if (DIST) od = second ? (out_d_b ? out_d_b + (qi - out_na) * k : nullptr) : (out_d ? out_d + qi * k : nullptr);
    int *oc = nullptr;
    if (CAP) {      // the query's own pointers, made here: the arguments they come from need not outlive the sums
        oc = out_count ? out_count + qi : nullptr;
        HELD(o);
        HELD(od);
        HELD(oc);
        HELD(groups);
        HELD(capm);
    }
    if (CAP && nc <= k) {       // heap order: rank = position
        for (int t = tid; t < nc; t += blockDim.x) {
            int64_t id = cs[t];
            by.id[t] = id;
            if (id < 0) id += n_rows;
            by.group[t] = groups[id];
            if (od) by.dist[t] = sqdist_row<T, TY>(rows + id * (int64_t)d, xs, d);
        }
        cap_select(by, nc, k, capm, o, od, oc);
        return;
    }
    if (nc <= k) {  // ivf.py:158-159 / fast_pq.py:307-308: heap order, no rescoring
        for (int t = tid; t < k; t += blockDim.x) o[t] = t < nc ? cs[t] : -1;
        if (tid == 0 && out_count) out_count[qi] = nc;
        if (DIST && od)
            for (int t = tid; t < k; t += blockDim.x) {
                T dv = (T)__builtin_huge_valf();
                if (t < nc) {
                    int64_t id = cs[t];
                    if (id < 0) id += n_rows;
                    dv = sqdist_row<T, TY>(rows + id * (int64_t)d, xs, d);
                }
                od[t] = dv;
            }
        return;
    }
    for (int t = tid; t < nc; t += blockDim.x) {
        int64_t id = cs[t];
        if (id < 0) id += n_rows;  // numpy fancy indexing with a negative index
        if (strip & 0x100) id = 0;            // timing experiment (wrong results): one row for every lane
        else if (strip & 0x200) id = blockIdx.x * 128 + t;    // ... consecutive rows
        ds[t] = sqdist_row<T, TY>(rows + id * (int64_t)d, xs, d);
    }
    __syncthreads();
    for (int t = tid; t < nc; t += blockDim.x) {
        const T dv = ds[t];
        int rank = 0;
        for (int u = 0; u < nc; u++) {
            const T du = ds[u];
            rank += (du < dv) || (du == dv && u < t);
        }
        if (CAP) {
            int64_t id = cs[t];
            by.id[rank] = id;
            by.dist[rank] = dv;
            by.group[rank] = groups[id < 0 ? id + n_rows : id];
        } else if (rank < k) {
            o[rank] = cs[t];
            if (DIST && od) od[rank] = dv;
        }
    }
    if (CAP) {
        cap_select(by, nc, k, capm, o, od, oc);
        return;
    }
    if (tid == 0 && out_count) out_count[qi] = k;
}

template <typename T, typename TY, typename TX>
__global__ __launch_bounds__(128) void rescore_kernel(const TX *__restrict__ q, int d,
                                                      const TY *__restrict__ rows,
                                                      int64_t n_rows,
                                                      const int64_t *__restrict__ cand, int R,
                                                      int k, int strip, int64_t *__restrict__ out,
                                                      int *__restrict__ out_count, const TX *__restrict__ q_b,
                                                      int64_t q_na, int64_t *__restrict__ out_b, int64_t out_na)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rescore_body<T, TY, TX, false>(smem, q, d, rows, n_rows, cand, R, k, strip, out, out_count, q_b, q_na, out_b,
                                   out_na, nullptr, nullptr);
}

template <typename T, typename TY, typename TX>
__global__ __launch_bounds__(128) void rescore_dist_kernel(const TX *__restrict__ q, int d,
                                                           const TY *__restrict__ rows, int64_t n_rows,
                                                           const int64_t *__restrict__ cand, int R, int k, int strip,
                                                           int64_t *__restrict__ out, int *__restrict__ out_count,
                                                           const TX *__restrict__ q_b, int64_t q_na,
                                                           int64_t *__restrict__ out_b, int64_t out_na,
                                                           T *__restrict__ out_d, T *__restrict__ out_d_b)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rescore_body<T, TY, TX, true>(smem, q, d, rows, n_rows, cand, R, k, strip, out, out_count, q_b, q_na, out_b,
                                  out_na, out_d, out_d_b);
}

// A staged row travels and rests as pieces of four elements: 16 bytes of float32, 8 bytes of IEEE half (GloVe's
// 200-byte half rows have no whole number of 16-byte pieces).
// (the compiler's own vector types: they can sit behind an LDS-qualified pointer on the host pass too)
typedef float float2_t __attribute__((ext_vector_type(2)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef unsigned uint2_t __attribute__((ext_vector_type(2)));
template <typename TY> struct RowPiece;
template <> struct RowPiece<float> { typedef float4_t type; };
template <> struct RowPiece<_Float16> { typedef uint2_t type; };

// The half of a piece that one lane of a pair sums: elements 2s, 2s + 1 — 8 bytes of a float32 piece, 4 of a half one.
template <typename P> struct HalfPiece;
template <> struct HalfPiece<float4_t> { typedef float2_t type; };
template <> struct HalfPiece<uint2_t> { typedef unsigned type; };

__device__ __forceinline__ float2_t widen2(const float2_t p) { return p; }

__device__ __forceinline__ float2_t widen2(const unsigned p)    // float(half): exact
{
    typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
    const half2_t h = __builtin_bit_cast(half2_t, p);
    return float2_t{(float)h.x, (float)h.y};
}

// sqdist_row<float, float> (after float(y) for half rows) for a row held in LDS as pieces, summed by TWO lanes: the
// four lane-accumulators of sqdist_row never meet before the last line, so lane s of the pair carries acc[2s] and
// acc[2s + 1] as one 2-vector (yp, xp: the row and the query from element 2s on, so piece j is yp[2j] / xp[2j]) and
// returns their sum, acc[2s] + acc[2s + 1]; the caller adds the partner's.  Per accumulator the operations and their
// order are sqdist_row's (un-fused subtract, multiply, add; groups of four pieces folded 3,2,1,0; whole pieces in the
// tail), here two at a time (v_pk_add_f32 / v_pk_mul_f32, which round as the scalar forms do; -ffp-contract=off).
template <typename H>
__device__ __forceinline__ float sqdist_row_lds(const H *__restrict__ yp, const float2_t *xp, int d4)
{
    float2_t acc = {0.f, 0.f};
    int j = 0;
    for (; d4 - j >= 4; j += 4) {
        float2_t df[4];
#pragma unroll
        for (int t = 0; t < 4; t++) df[t] = widen2(yp[2 * (j + t)]) - xp[2 * (j + t)];
        const float2_t ab3 = df[3] * df[3] + acc;
        const float2_t ab2 = df[2] * df[2] + ab3;
        const float2_t ab1 = df[1] * df[1] + ab2;
        acc = df[0] * df[0] + ab1;
    }
    for (; j < d4; j++) {            // d % 4 == 0: whole vectors only
        const float2_t df = widen2(yp[2 * j]) - xp[2 * j];
        acc = df * df + acc;
    }
    return acc.x + acc.y;
}

// LDS addresses as numbers, and back: what a ds instruction takes, so that a clamp is one v_min on it.
#define LDS_AT(p) ((unsigned)(size_t)(__attribute__((address_space(3))) const void *)(p))
#define LDS_PTR(T, a) ((__attribute__((address_space(3))) T *)(size_t)(a))
// The first address of an unrolled run, hidden from the optimiser (no instruction is emitted): seeing through it, it
// carries each of the run's sixteen addresses round the enclosing loop in a register of its own, for the loads and
// again for the stores, and at 134 VGPRs no longer keeps sixteen loads in flight.
#define OPAQUE(x) asm("" : "+v"(x))

// the value of the neighbouring lane (lane ^ 1): one DPP move, no LDS
__device__ __forceinline__ float from_pair_lane(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
}

// Strict-count ranks of a lane's NV values dv[] among ds[0 .. nc4) (nc rounded up to 4 with +inf): per value and
// element one compare and one add.  cnt[j] = #{u : ds[u] < dv[j]} is the final rank of dv[j] when every pair of the nc
// distances is strictly ordered — and then the counts of all nc values add up to nc (nc - 1) / 2; a pair that is not
// (equal, +0 / -0, a NaN) adds 0 where an ordered one adds 1, so the sum falls short exactly when there is one.
template <int NV>
__device__ __forceinline__ void strict_counts(const float *ds, int nc4, const float *dv, int *cnt)
{
#pragma unroll
    for (int j = 0; j < NV; j++) cnt[j] = 0;
    for (int u = 0; u < nc4; u += 4) {
        const float4_t du = *(const float4_t *)(ds + u);
#pragma unroll
        for (int j = 0; j < NV; j++) {
            cnt[j] += du.x < dv[j];
            cnt[j] += du.y < dv[j];
            cnt[j] += du.z < dv[j];
            cnt[j] += du.w < dv[j];
        }
    }
}

// make_slots_kernel's work for ONE query by the wave that ranked its probed lists (S <= 64): lane s
// holds the id of slot s.  Same outputs, same atomics.
__device__ __forceinline__ void slots_epilogue(const TkSlotsOut &so, int64_t qi, int S, int lane, int64_t cl)
{
    const bool act = lane < S;
    bool wr = false;
    if (act && cl < 0) { cl += so.n_lists; wr = true; }
    const bool wrapped = __builtin_amdgcn_ballot_w64(wr) != 0;
    int64_t c0 = 0, rows = 0, loff = 0;
    int len = 0, n = 0;
    if (act) {
        c0 = so.list_chunk_off[cl];
        len = (int)(so.list_chunk_off[cl + 1] - c0);
        const int64_t ln = so.list_n[cl];
        n = (int)ln;
        rows = ln;
        loff = so.ids_off[cl];
    }
    int acc = len;              // inclusive scans over the slots
    int64_t racc = rows;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ua = __shfl_up(acc, o, 64);
        const int64_t ur = __shfl_up(racc, o, 64);
        if (lane >= o) { acc += ua; racc += ur; }
    }
    if (lane == 0) so.slot_prefix[qi * (S + 1)] = 0;
    if (act) {
        so.slot_prefix[qi * (S + 1) + lane + 1] = acc;
        so.slot_chunk0[qi * S + lane] = c0;
        so.slot_n[qi * S + lane] = n;
        so.slot_label_off[qi * S + lane] = loff;
    }
    // leading slots that stay exact: until the lists scanned so far hold R rows
    const uint64_t full = __builtin_amdgcn_ballot_w64(act && racc >= (int64_t)so.R);
    int e = full ? __builtin_ctzll(full) + 1 : S;
    const bool plain_ok = so.slot_exact && !wrapped && so.qlim[qi] != TK_PLAIN_NEVER;
    const int e_walk = e;
    if (!plain_ok) e = S;
    bool head = false;
    if (so.slot_exact) {
        const int E = (so.R + 15) >> 4;
        const int first_len = __shfl(acc, 0, 64);
        head = plain_ok && e_walk == 1 && first_len > E;
        const int at_e = e > 0 ? __shfl(acc, e - 1, 64) : 0;
        if (lane == 0) {
            so.slot_exact[qi] = head ? 0 : e;
            so.plain0[qi] = head ? E : at_e;
        }
    }
    if (so.pair_count && act && !(so.owner && so.owner[cl] != so.me)) {
        if (head && lane == 0) {
            atomicAdd(&so.pair_count3[cl], 1);
            atomicAdd(&so.pair_count2[cl], 1);
        } else {
            atomicAdd(lane < e ? &so.pair_count[cl] : &so.pair_count2[cl], 1);
        }
    }
    if (lane == 0 && so.repeat_flag) so.repeat_flag[qi] = wrapped;
}

// rescore_body for float32 sums (float32 queries; rows TY = float, or _Float16: the result is what the float32
// rows float(half(x)) give) with d % 4 == 0, rows staged through LDS: in the kernel above a lane walks its own
// row, so every load instruction of a wave touches 64 different lines — 2775 line visits per query at R = 111,
// d = 100 — and that address traffic is what it costs the scan kernels it runs beside
// (profiles/r02_scan_grid.md).  Here the wave reads TILE candidate rows as one stream of pieces (RowPiece),
// consecutive lanes = consecutive pieces of a row (4 lines per 400-byte row), drops them into a tile, and two
// lanes per row then run the identical summation (sqdist_row: numpy's order, two of its four accumulators each)
// from LDS.  A half tile stays in half (half the float32 tile's LDS) and is widened where it is summed.
// The row stride of the tile is an ODD number of pieces, which makes the half-piece reads of the sum conflict-free
// (worked out where they are issued).  A candidate's row is resolved ONCE, by the compaction, into a byte offset
// kept beside its id; the ranking is one walk over the distances with the strict comparison, checked by the sum
// of the counts, and falls back to the walk that breaks ties by position (strict_counts).
// LDS: cand[R] (int64) | row offset[R] (int64) | dist[R] | x[d] | tile[TILE + 1 spare][stride] | have_slots: the
// k results (int64)
// DIST as rescore_body (the short-heap branch reads its rows with sqdist_row: the same summation as sqdist_row_lds)
// CAP as rescore_body: both rankings and the short-heap branch leave every candidate at its rank in CapRanked<float>(R),
// which lies where the fused form keeps its k results (a capped launch writes no descriptors), and cap_select writes.
template <typename TY, int TILE, bool DIST, bool CAP = false>
__device__ __forceinline__ void rescore_staged_body(unsigned char *smem, const float *__restrict__ q, int d,
                                                    const TY *__restrict__ rows, int64_t n_rows,
                                                    const int64_t *__restrict__ cand, int R, int k, int strip,
                                                    int64_t *__restrict__ out, int *__restrict__ out_count,
                                                    int stride, const float *__restrict__ q_b, int64_t q_na,
                                                    int64_t *__restrict__ out_b, int64_t out_na,
                                                    const TkSlotsOut *__restrict__ so_dev, float *__restrict__ out_d,
                                                    float *__restrict__ out_d_b, const TkCap &cap = TkCap())
{
    typedef typename RowPiece<TY>::type P;
    typedef typename HalfPiece<P>::type H;
    const bool have_slots = so_dev != nullptr;
    int64_t *cs = (int64_t *)smem;
    int64_t *ro = cs + R;                                // a kept candidate's row, in bytes from `rows`
    float *ds = (float *)(smem + (size_t)R * 16);
    float *xs = ds + ((R + 3) & ~3);
    P *tile = (P *)(xs + ((d + 3) & ~3));                // 16-byte aligned
    constexpr int PER16 = 16 / (int)sizeof(P);
    // behind the tile rounded up to 16 bytes: have_slots, the k results in order; CAP, the candidates by rank
    unsigned char *const behind = (unsigned char *)(tile + (((TILE + 1) * stride + PER16 - 1) & ~(PER16 - 1)));
    const CapRanked<float> by(behind, R);
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const int64_t *c = cand + qi * R;
    unsigned capm = 0;
    const int32_t *groups = CAP ? cap.groups : nullptr;     // (the epilogue's scalars: read here, kept in vector registers)
    if (CAP) capm = cap_of(cap, qi);
    const float *qrow = (q_b && qi >= q_na) ? q_b + (qi - q_na) * d : q + qi * d;   // second call of a pair
    for (int t = tid; t < d; t += 64) xs[t] = qrow[t];
    // ordered compaction of the candidate ids (ivf.py:154-155 drops -1)
    int nc = 0;
    for (int t0 = 0; t0 < R; t0 += 64) {
        const int t = t0 + tid;
        const int64_t id = t < R ? c[t] : -1;
        const bool keep = t < R && (!strip || id != -1);
        const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
        const int before = __builtin_popcountll(m & ((1ull << tid) - 1ull));
        if (keep) {
            cs[nc + before] = id;
            // numpy fancy indexing with a negative index, resolved once per candidate
            ro[nc + before] = (id < 0 ? id + n_rows : id) * (int64_t)d * (int64_t)sizeof(TY);
        }
        nc += __builtin_popcountll(m);
    }
    // the ranking reads ds[] four at a time: +inf behind the last distance is below no value
    if (tid < ((-nc) & 3)) ds[nc + tid] = __builtin_huge_valf();
    __syncthreads();
    const bool second = out_b && qi >= out_na;
    int64_t *o = second ? out_b + (qi - out_na) * k : out + qi * k;
    float *od = nullptr;
    if (DIST) od = second ? (out_d_b ? out_d_b + (qi - out_na) * k : nullptr) : (out_d ? out_d + qi * k : nullptr);
    int *oc = nullptr;
    if (CAP) {      // the query's own pointers, made here: the arguments they come from need not outlive the sums
        oc = out_count ? out_count + qi : nullptr;
        HELD(o);
        HELD(od);
        HELD(oc);
        HELD(groups);
        HELD(capm);
    }
    if (CAP && nc <= k) {       // heap order: rank = position
        for (int t = tid; t < nc; t += 64) {
            int64_t id = cs[t];
            by.id[t] = id;
            if (id < 0) id += n_rows;
            by.group[t] = groups[id];
            if (od) by.dist[t] = sqdist_row<float, TY>(rows + id * (int64_t)d, xs, d);
        }
        cap_select(by, nc, k, capm, o, od, oc);
        return;
    }
    if (nc <= k) {  // ivf.py:158-159 / fast_pq.py:307-308: heap order, no rescoring
        for (int t = tid; t < k; t += 64) o[t] = t < nc ? cs[t] : -1;
        if (tid == 0 && out_count) out_count[qi] = nc;
        if (DIST && od)
            for (int t = tid; t < k; t += 64) {
                float dv = __builtin_huge_valf();
                if (t < nc) {
                    int64_t id = cs[t];
                    if (id < 0) id += n_rows;
                    dv = sqdist_row<float, TY>(rows + id * (int64_t)d, xs, d);
                }
                od[t] = dv;
            }
        if (have_slots) slots_epilogue(*so_dev, qi, k, tid, tid < nc ? cs[tid < k ? tid : 0] : -1);
        return;
    }
    const int d4 = d >> 2;                   // pieces per row
    // lanes_per_row = the power of two >= d4 (16, 32 or 64): a load instruction covers
    // 64 / lanes_per_row whole rows, lane (rr, pc) fetches piece pc of its row
    const int lpr_log = d4 <= 16 ? 4 : (d4 <= 32 ? 5 : 6);
    const int rr = tid >> lpr_log, pc = tid & ((1 << lpr_log) - 1), rpi = 64 >> lpr_log;
    // A lane's LDS addresses are plain numbers (LDS_AT: base included), each one add of a wave-uniform multiple of
    // the step and one min: the row position comes resolved from ro[], so a load costs one LDS read and one 64-bit
    // add onto the lane's base (piece pc of row 0).
    const char *const lane_base = (const char *)rows + (size_t)pc * sizeof(P);
    const unsigned ro_step = rpi * 8, st_step = rpi * stride * (unsigned)sizeof(P);
    const int half = tid & 1, prow = tid >> 1;           // the sum: lanes 2p, 2p + 1 share row p of 32
    const float2_t *const xp = (const float2_t *)xs + half;
    for (int t0 = 0; t0 < nc; t0 += TILE) {
        const int nt = nc - t0 < TILE ? nc - t0 : TILE;
        if (pc < d4)
            for (int r0 = rr; r0 < nt; r0 += 16 * rpi) {
                // sixteen loads in flight per lane before the first LDS store waits for one; rows past the tile
                // re-read its last row
                P v[16];
                unsigned ro_at = LDS_AT(ro + t0 + r0), st_at = LDS_AT(tile + r0 * stride + pc);
                const unsigned ro_last = LDS_AT(ro + t0 + nt - 1), st_spare = LDS_AT(tile + nt * stride + pc);
                OPAQUE(ro_at);
                OPAQUE(st_at);
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const unsigned a = ro_at + u * ro_step;
                    v[u] = *(const P *)(lane_base + *LDS_PTR(const int64_t, a < ro_last ? a : ro_last));
                }
                // unconditional stores (rows past the tile land in row nt, which is summed by nobody and exists:
                // the tile has TILE + 1 rows): a branch here lets the compiler sink each load next to its store,
                // one exposed latency apiece
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const unsigned a = st_at + u * st_step;
                    *LDS_PTR(P, a < st_spare ? a : st_spare) = v[u];
                }
            }
        __syncthreads();
        // two lanes per row, all 64 at work on a 32-row tile (a 64-row tile goes in two halves).  Banks: lane
        // (p, s) reads 8 bytes (float32 rows) at dword 4 * (p * stride + j) + 2s — ds_read_b64 serves lanes 0-31
        // and 32-63 apart, 16 rows each, p * stride distinct mod 16 for an odd stride, so the 32 lanes cover the
        // 64 banks once; 4 bytes (half rows) at dword 2 * (p * stride + j) + s, p * stride distinct mod 32 over the
        // 32 rows: 64 lanes, 64 banks.  The query's 2 addresses per read are broadcasts.  No conflicts either way.
        for (int rb = 0; rb < nt; rb += 32) {
            const int r = rb + prow;            // (rows nt .. TILE - 1 hold stale pieces: summed, not kept)
            const float mine = sqdist_row_lds((const H *)(tile + r * stride) + half, xp, d4);
            const float sum = mine + from_pair_lane(mine);      // (acc[0] + acc[1]) + (acc[2] + acc[3])
            if (half == 0 && r < nt) ds[t0 + r] = sum;
        }
        __syncthreads();
    }
    int64_t *ps = (int64_t *)behind;
    // rank by counting: a lane keeps its values (t = tid, tid + 64, ...: at most four, R <= 256) in registers and
    // walks ds[] once with the strict comparison alone; beyond nc it holds -inf, which nothing is below
    float dv[4];
    int cnt[4];
#pragma unroll
    for (int j = 0; j < 4; j++) dv[j] = tid + 64 * j < nc ? ds[tid + 64 * j] : -__builtin_huge_valf();
    const int nc4 = (nc + 3) & ~3;
    if (nc <= 64) { strict_counts<1>(ds, nc4, dv, cnt); cnt[1] = cnt[2] = cnt[3] = 0; }
    else if (nc <= 128) { strict_counts<2>(ds, nc4, dv, cnt); cnt[2] = cnt[3] = 0; }
    else strict_counts<4>(ds, nc4, dv, cnt);
    int total = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) total += __shfl_xor(total, m, 64);
    if (total == nc * (nc - 1) / 2) {       // every pair strictly ordered: the counts are the ranks
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int t = tid + 64 * j;
            if (CAP) {
                if (t < nc) {
                    const int64_t id = cs[t];
                    by.id[cnt[j]] = id;
                    by.dist[cnt[j]] = dv[j];
                    by.group[cnt[j]] = groups[id < 0 ? id + n_rows : id];
                }
            } else if (t < nc && cnt[j] < k) {
                o[cnt[j]] = cs[t];
                if (DIST && od) od[cnt[j]] = dv[j];
                if (have_slots) ps[cnt[j]] = cs[t];
            }
        }
    } else {                                // equal distances (or a NaN): ties go to the lower position
        for (int t = tid; t < nc; t += 64) {
            const float dvt = ds[t];
            int rank = 0;
            for (int u = 0; u < nc; u++) {
                const float du = ds[u];
                rank += (du < dvt) || (du == dvt && u < t);
            }
            if (CAP) {
                const int64_t id = cs[t];
                by.id[rank] = id;
                by.dist[rank] = dvt;
                by.group[rank] = groups[id < 0 ? id + n_rows : id];
            } else if (rank < k) {
                o[rank] = cs[t];
                if (DIST && od) od[rank] = dvt;
                if (have_slots) ps[rank] = cs[t];
            }
        }
    }
    if (CAP) {
        cap_select(by, nc, k, capm, o, od, oc);
        return;
    }
    if (tid == 0 && out_count) out_count[qi] = k;
    if (have_slots) {
        __syncthreads();
        slots_epilogue(*so_dev, qi, k, tid, tid < k ? ps[tid] : -1);
    }
}

// The kernels of the body, under the names the resource tests pin and profiles/ records.  (The distance forms on
// half rows carry "distances" in their names: the resource test of the float32 / float64 ones counts the names that
// hold "dist_kernel".  They take no descriptors: the coarse stage, which writes them, asks for no distances.)
template <int TILE>
__global__ __launch_bounds__(64) void rescore_staged_kernel(const float *__restrict__ q, int d,
                                                            const float *__restrict__ rows,
                                                            int64_t n_rows,
                                                            const int64_t *__restrict__ cand, int R,
                                                            int k, int strip, int64_t *__restrict__ out,
                                                            int *__restrict__ out_count, int stride4,
                                                            const float *__restrict__ q_b, int64_t q_na,
                                                            int64_t *__restrict__ out_b, int64_t out_na,
                                                            const TkSlotsOut *__restrict__ so_dev)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rescore_staged_body<float, TILE, false>(smem, q, d, rows, n_rows, cand, R, k, strip, out, out_count, stride4, q_b,
                                            q_na, out_b, out_na, so_dev, nullptr, nullptr);
}

template <int TILE>
__global__ __launch_bounds__(64) void rescore_staged_dist_kernel(const float *__restrict__ q, int d,
                                                                 const float *__restrict__ rows, int64_t n_rows,
                                                                 const int64_t *__restrict__ cand, int R, int k,
                                                                 int strip, int64_t *__restrict__ out,
                                                                 int *__restrict__ out_count, int stride4,
                                                                 const float *__restrict__ q_b, int64_t q_na,
                                                                 int64_t *__restrict__ out_b, int64_t out_na,
                                                                 float *__restrict__ out_d, float *__restrict__ out_d_b)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rescore_staged_body<float, TILE, true>(smem, q, d, rows, n_rows, cand, R, k, strip, out, out_count, stride4, q_b,
                                           q_na, out_b, out_na, nullptr, out_d, out_d_b);
}

template <int TILE>
__global__ __launch_bounds__(64) void rescore_staged_half_kernel(const float *__restrict__ q, int d,
                                                                 const _Float16 *__restrict__ rows, int64_t n_rows,
                                                                 const int64_t *__restrict__ cand, int R, int k,
                                                                 int strip, int64_t *__restrict__ out,
                                                                 int *__restrict__ out_count, int stride8,
                                                                 const float *__restrict__ q_b, int64_t q_na,
                                                                 int64_t *__restrict__ out_b, int64_t out_na,
                                                                 const TkSlotsOut *__restrict__ so_dev)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rescore_staged_body<_Float16, TILE, false>(smem, q, d, rows, n_rows, cand, R, k, strip, out, out_count, stride8,
                                               q_b, q_na, out_b, out_na, so_dev, nullptr, nullptr);
}

template <int TILE>
__global__ __launch_bounds__(64) void rescore_staged_half_distances_kernel(const float *__restrict__ q, int d,
                                                                      const _Float16 *__restrict__ rows,
                                                                      int64_t n_rows, const int64_t *__restrict__ cand,
                                                                      int R, int k, int strip,
                                                                      int64_t *__restrict__ out,
                                                                      int *__restrict__ out_count, int stride8,
                                                                      const float *__restrict__ q_b, int64_t q_na,
                                                                      int64_t *__restrict__ out_b, int64_t out_na,
                                                                      float *__restrict__ out_d,
                                                                      float *__restrict__ out_d_b)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rescore_staged_body<_Float16, TILE, true>(smem, q, d, rows, n_rows, cand, R, k, strip, out, out_count, stride8,
                                              q_b, q_na, out_b, out_na, nullptr, out_d, out_d_b);
}

// the lane-per-row kernel's distance-writing form on half rows: rescore_body<float, _Float16, float, true>, as
// rescore_dist_kernel<float, _Float16, float> would be
__global__ __launch_bounds__(128) void rescore_half_distances_kernel(const float *__restrict__ q, int d,
                                                                     const _Float16 *__restrict__ rows, int64_t n_rows,
                                                                     const int64_t *__restrict__ cand, int R, int k,
                                                                     int strip, int64_t *__restrict__ out,
                                                                     int *__restrict__ out_count,
                                                                     const float *__restrict__ q_b, int64_t q_na,
                                                                     int64_t *__restrict__ out_b, int64_t out_na,
                                                                     float *__restrict__ out_d,
                                                                     float *__restrict__ out_d_b)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rescore_body<float, _Float16, float, true>(smem, q, d, rows, n_rows, cand, R, k, strip, out, out_count, q_b, q_na,
                                               out_b, out_na, out_d, out_d_b);
}

// The capped forms (per_group=): the two bodies with CAP, one kernel per form, the distance pointers NULL for ids alone.
// (Names of their own: the resource tests find the kernels above by substrings of theirs, the half ones by the row
// type in the mangled name — so the row type is named here by its code, ROWS = TK_DATA_F32 / _F64 / _F16 as
// tk_launch_rescore's rows_dtype, and the rows come in untyped.)
template <int ROWS> struct RowsOf;
template <> struct RowsOf<0> { typedef float type; };
template <> struct RowsOf<1> { typedef double type; };
template <> struct RowsOf<2> { typedef _Float16 type; };
template <typename TY> constexpr int rows_code()
{
    return std::is_same<TY, _Float16>::value ? 2 : (std::is_same<TY, double>::value ? 1 : 0);
}

template <typename T, int ROWS, typename TX>
__global__ __launch_bounds__(128) void capped_rows_kernel(const TX *__restrict__ q, int d, const void *__restrict__ rows,
                                                          int64_t n_rows, const int64_t *__restrict__ cand, int R, int k,
                                                          int strip, int64_t *__restrict__ out,
                                                          int *__restrict__ out_count, const TX *__restrict__ q_b,
                                                          int64_t q_na, int64_t *__restrict__ out_b, int64_t out_na,
                                                          T *__restrict__ out_d, T *__restrict__ out_d_b, const TkCap cap)
{
    typedef typename RowsOf<ROWS>::type TY;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rescore_body<T, TY, TX, true, true>(smem, q, d, (const TY *)rows, n_rows, cand, R, k, strip, out, out_count, q_b,
                                        q_na, out_b, out_na, out_d, out_d_b, cap);
}

template <int ROWS, int TILE>
__global__ __launch_bounds__(64) void capped_tile_kernel(const float *__restrict__ q, int d, const void *__restrict__ rows,
                                                         int64_t n_rows, const int64_t *__restrict__ cand, int R, int k,
                                                         int strip, int64_t *__restrict__ out,
                                                         int *__restrict__ out_count, int stride,
                                                         const float *__restrict__ q_b, int64_t q_na,
                                                         int64_t *__restrict__ out_b, int64_t out_na,
                                                         float *__restrict__ out_d, float *__restrict__ out_d_b,
                                                         const TkCap cap)
{
    typedef typename RowsOf<ROWS>::type TY;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    rescore_staged_body<TY, TILE, true, true>(smem, q, d, (const TY *)rows, n_rows, cand, R, k, strip, out, out_count,
                                              stride, q_b, q_na, out_b, out_na, nullptr, out_d, out_d_b, cap);
}

// ---- host side -------------------------------------------------------------------------------------------------
// One call as tk_launch_rescore received it; a launcher casts the pointers to the types it was chosen for.
struct RescoreCall {
    const void *q, *rows;
    int d, R, k, strip;
    int64_t n_rows, nq;
    const int64_t *cand;
    int64_t *out;
    int *out_count;
    hipStream_t s;
    TkSecond q2, out2;
    void *dist, *dist_b;    // want_d: where the distances go (either may be null)
    bool want_d;
    const TkCap *cap;       // per_group=: the capped kernels (or NULL)
};

// the kernels by row type
template <int TILE> static auto staged_ids_kernel(const float *) { return rescore_staged_kernel<TILE>; }
template <int TILE> static auto staged_ids_kernel(const _Float16 *) { return rescore_staged_half_kernel<TILE>; }
template <int TILE> static auto staged_dist_kernel(const float *) { return rescore_staged_dist_kernel<TILE>; }
template <int TILE> static auto staged_dist_kernel(const _Float16 *) { return rescore_staged_half_distances_kernel<TILE>; }

template <typename T, typename TY, typename TX> static auto rows_dist_kernel()
{
    if constexpr (std::is_same<TY, _Float16>::value) return rescore_half_distances_kernel;
    else return rescore_dist_kernel<T, TY, TX>;
}

// every lane walks its own row: sums in T, rows TY, queries TX
template <typename T, typename TY, typename TX>
static void launch_rows(const RescoreCall &c)
{
    // one wave is enough for the coarse stage's 2 * n_probes + 10 candidates: the second wave of
    // a 128-thread workgroup only waited at the barriers and took a wave slot beside the scan
    const dim3 grid((unsigned)c.nq), block(c.R <= 64 ? 64 : 128);
    const size_t lds = (size_t)c.R * 8 + ((size_t)c.R + c.d) * sizeof(T) + 16;
    const TX *q = (const TX *)c.q, *q_b = (const TX *)c.q2.b;
    const TY *rows = (const TY *)c.rows;
    if (c.cap)      // (the candidates by rank behind x[], 8-byte aligned)
        hipLaunchKernelGGL((capped_rows_kernel<T, rows_code<TY>(), TX>), grid, block,
                           ((lds - 16 + 7) & ~(size_t)7) + cap_lds_bytes(c.R, sizeof(T)), c.s, q, c.d, c.rows, c.n_rows, c.cand, c.R, c.k, c.strip, c.out, c.out_count, q_b, c.q2.n_a,
                           (int64_t *)c.out2.b, c.out2.n_a, (T *)c.dist, (T *)c.dist_b, *c.cap);
    else if (c.want_d)
        hipLaunchKernelGGL((rows_dist_kernel<T, TY, TX>()), grid, block, lds, c.s, q, c.d, rows, c.n_rows, c.cand, c.R,
                           c.k, c.strip, c.out, c.out_count, q_b, c.q2.n_a, (int64_t *)c.out2.b, c.out2.n_a,
                           (T *)c.dist, (T *)c.dist_b);
    else
        hipLaunchKernelGGL((rescore_kernel<T, TY, TX>), grid, block, lds, c.s, q, c.d, rows, c.n_rows, c.cand, c.R,
                           c.k, c.strip, c.out, c.out_count, q_b, c.q2.n_a, (int64_t *)c.out2.b, c.out2.n_a);
}

template <typename TY, int TILE>
static void launch_staged_tile(const RescoreCall &c, size_t lds, int stride, const TkSlotsOut *so)
{
    const dim3 grid((unsigned)c.nq), block(64);
    const float *q = (const float *)c.q, *q_b = (const float *)c.q2.b;
    const TY *rows = (const TY *)c.rows;
    if (c.cap)
        hipLaunchKernelGGL((capped_tile_kernel<rows_code<TY>(), TILE>), grid, block, lds, c.s, q, c.d, c.rows, c.n_rows, c.cand, c.R,
                           c.k, c.strip, c.out, c.out_count, stride, q_b, c.q2.n_a, (int64_t *)c.out2.b, c.out2.n_a,
                           (float *)c.dist, (float *)c.dist_b, *c.cap);
    else if (c.want_d)
        hipLaunchKernelGGL(staged_dist_kernel<TILE>(rows), grid, block, lds, c.s, q, c.d, rows, c.n_rows, c.cand, c.R,
                           c.k, c.strip, c.out, c.out_count, stride, q_b, c.q2.n_a, (int64_t *)c.out2.b, c.out2.n_a,
                           (float *)c.dist, (float *)c.dist_b);
    else
        hipLaunchKernelGGL(staged_ids_kernel<TILE>(rows), grid, block, lds, c.s, q, c.d, rows, c.n_rows, c.cand, c.R,
                           c.k, c.strip, c.out, c.out_count, stride, q_b, c.q2.n_a, (int64_t *)c.out2.b, c.out2.n_a,
                           so);
}

// float32 sums on rows TY (float32 queries): returns 1 when the descriptors were written too, else 0.
// Rows staged through LDS in tiles of 32 (form 2, DEFAULT) / 64 (form 1) rows, or every lane
// walking its own row (form 0); tk_index_set_option(TK_OPT_RESCORE_FORM).  Round 2
// (profiles/r02_scan_grid.md): the 32-row form was the fastest alone (0.118 ms per 10 000
// queries against 0.135) but lost in the pipeline — its workgroups (15-29 KB of LDS) were
// placed late next to the exact scan's persistent grid: 0.68-0.70 ms per batch against 0.656.
// Round 3, next to the plain kernel (two 58 KB workgroups per CU leave 44 KB): 0.495 ms per
// batch against 0.543 (profiles/r03/ab_pipeline_knobs.txt) — the 64 lines a wave touches per
// load in mode 0 were costing the scans beside it more than its own time.
template <typename TY>
static int launch_float_sums(const RescoreCall &c, int form, const TkSlotsOut *slots)
{
    const int staged = form < 0 || form > 2 ? 2 : form;
    // (heaps beyond 256 entries: a 64-lane workgroup walks 16+ tiles one after the other — n_probes 50,
    //  R = 511: 3.18 M queries/s staged against 3.85 M with the 128-lane lane-per-row kernel)
    if (staged && c.d % 4 == 0 && c.d <= 256 && c.R <= 256) {
        const int stride = (c.d / 4) | 1;                       // odd number of pieces
        const int tile_rows = staged == 2 ? 32 : 64;
        const bool fuse = slots != nullptr && c.k <= 64;        // (slots: a DEVICE copy of the structure)
        const size_t tile_bytes = (size_t)(tile_rows + 1) * stride * sizeof(typename RowPiece<TY>::type);
        // ids and resolved row offsets (8 bytes each per candidate) | distances | query | tile | fused: the k results;
        // capped: the candidates by rank
        const size_t lds = (size_t)c.R * 16 +
                           (size_t)(((c.R + 3) & ~3) + ((c.d + 3) & ~3)) * 4 + ((tile_bytes + 15) & ~(size_t)15) +
                           (fuse ? (size_t)c.k * 8 : 0) + (c.cap ? cap_lds_bytes(c.R, 4) : 0);
        if (lds <= 64 * 1024) {
            if (tile_rows == 32) launch_staged_tile<TY, 32>(c, lds, stride, fuse ? slots : nullptr);
            else launch_staged_tile<TY, 64>(c, lds, stride, fuse ? slots : nullptr);
            return fuse ? 1 : 0;
        }
    }
    launch_rows<float, TY, float>(c);
    return 0;
}

// rows_dtype: TK_DATA_F32 / TK_DATA_F64 / TK_DATA_F16 (the coarse stage and tk_bottom_k pass 0 / 1)
int tk_launch_rescore(const void *q, int q_is_f64, int d, const void *rows, int rows_dtype,
                      int64_t n_rows, const int64_t *cand, int R, int64_t nq, int k, int strip,
                      int64_t *out, int *out_count, hipStream_t s, int form, TkSecond q2, TkSecond out2,
                      const TkSlotsOut *slots, void *dist, TkSecond dist2, const TkCap *cap)
{
    if (nq == 0 || k == 0) return 0;
    const bool want_d = dist != nullptr || dist2.b != nullptr;
    if (want_d || cap) slots = nullptr;         // (the descriptors' caller asks for no distances and no cap)
    void *dist_b = out2.b ? const_cast<void *>(dist2.b) : nullptr;     // (rows of the second call: out2.n_a on)
    const RescoreCall c = {q, rows, d, R, k, strip, n_rows, nq, cand, out, out_count, s, q2, out2, dist, dist_b, want_d,
                           cap};
    if (rows_dtype == 2)                        // half vectors: float32 queries only (the index's final stage)
        return q_is_f64 ? -1 : launch_float_sums<_Float16>(c, form, slots);
    const int rows_is_f64 = rows_dtype == 1;
    if (!q_is_f64 && !rows_is_f64) return launch_float_sums<float>(c, form, slots);
    // numpy promotes `Y - x` to float64
    if (rows_is_f64 && q_is_f64) launch_rows<double, double, double>(c);
    else if (rows_is_f64) launch_rows<double, double, float>(c);
    else launch_rows<double, float, double>(c);
    return 0;
}

// ---------------------------------------------------------------------------
// probes (nq, S) -> scan descriptors.  A negative list id (an unfilled coarse heap
// slot, fast_pq.py:307-312 does not filter them) addresses from the end, as the
// reference's Python list indexing does (ivf.py:141).
__global__ void make_slots_kernel(const int64_t *__restrict__ probes, int S, int64_t nq,
                                  int64_t n_lists, const int64_t *__restrict__ list_chunk_off,
                                  const int64_t *__restrict__ list_n,
                                  const int64_t *__restrict__ ids_off, int *__restrict__ slot_prefix,
                                  int64_t *__restrict__ slot_chunk0, int *__restrict__ slot_n,
                                  int64_t *__restrict__ slot_label_off,
                                  unsigned char *__restrict__ repeat_flag,
                                  int *__restrict__ pair_count, const int *__restrict__ owner,
                                  int me, const int *__restrict__ qlim, int R,
                                  int *__restrict__ slot_exact, int *__restrict__ pair_count2,
                                  int *__restrict__ plain0, int *__restrict__ pair_count3)
{
    int64_t qi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    int acc = 0;
    bool wrapped = false;  // a wrapped id may name a list that is probed twice
    slot_prefix[qi * (S + 1)] = 0;
    // leading slots that stay exact: until the lists scanned so far hold 2R rows (the heap is then
    // full of real values and its bound far below the table's limit; the replay checks)
    int e = S;
    int64_t rows = 0;
    for (int s = 0; s < S; s++) {
        int64_t cl = probes[qi * S + s];
        if (cl < 0) { cl += n_lists; wrapped = true; }
        int64_t c0 = list_chunk_off[cl];
        acc += (int)(list_chunk_off[cl + 1] - c0);
        slot_prefix[qi * (S + 1) + s + 1] = acc;
        slot_chunk0[qi * S + s] = c0;
        slot_n[qi * S + s] = (int)list_n[cl];
        slot_label_off[qi * S + s] = ids_off[cl];
        rows += list_n[cl];
        if (e == S && rows >= (int64_t)R) e = s + 1;        // (R here: the rows the exact kernel keeps)
    }
    const bool plain_ok = slot_exact && !wrapped && qlim[qi] != TK_PLAIN_NEVER;
    const int e_walk = e;
    if (!plain_ok) e = S;
    bool head = false;
    if (slot_exact) {
        // head mode: the first list alone holds 2R rows and is longer than the head
        const int E = (R + 15) >> 4;
        head = plain_ok && e_walk == 1 && slot_prefix[qi * (S + 1) + 1] > E;
        slot_exact[qi] = head ? 0 : e;
        plain0[qi] = head ? E : slot_prefix[qi * (S + 1) + e];
    }
    if (pair_count)
        for (int s = 0; s < S; s++) {
            int64_t cl = probes[qi * S + s];
            if (cl < 0) cl += n_lists;
            // pairs per list, for the list-major scan (sharded index: of the lists I own)
            if (owner && owner[cl] != me) continue;
            if (head && s == 0) {
                atomicAdd(&pair_count3[cl], 1);
                atomicAdd(&pair_count2[cl], 1);
            } else {
                atomicAdd(s < e ? &pair_count[cl] : &pair_count2[cl], 1);
            }
        }
    if (repeat_flag) repeat_flag[qi] = wrapped;
}

// The same with one WAVE per query, lane s = slot s (S <= 64): the thread-per-query form walks its S slots one
// dependent load after the other — 76 us for the 80 000 queries x 10 slots of a list-sharded batch at W = 8,
// every rank doing all of it; here the slots of a query are loaded at once and scanned by shuffles.
__global__ __launch_bounds__(256) void make_slots_wave_kernel(const int64_t *__restrict__ probes, int S, int64_t nq,
                                                              const TkSlotsOut so)
{
    const int lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;       // (whole waves leave: the ballots below see full waves only)
    slots_epilogue(so, qi, S, lane, lane < S ? probes[qi * S + lane] : -1);
}

void tk_launch_make_slots(const int64_t *probes, const int *probe_count, int kc, int64_t nq,
                          int64_t n_lists, const int64_t *list_chunk_off, const int64_t *list_n,
                          const int64_t *ids_off, int *slot_prefix, int64_t *slot_chunk0,
                          int *slot_n, int64_t *slot_label_off, unsigned char *repeat_flag,
                          int *pair_count, const int *owner, int me, hipStream_t s,
                          const int *qlim, int R, int *slot_exact, int *pair_count2, int *plain0,
                          int *pair_count3)
{
    (void)probe_count;
    if (nq == 0) return;
    if (!qlim || !pair_count2 || !plain0 || !pair_count3) slot_exact = nullptr;
    if (kc <= 64 && nq >= 4096) {
        TkSlotsOut so;
        so.n_lists = n_lists; so.list_chunk_off = list_chunk_off; so.list_n = list_n; so.ids_off = ids_off;
        so.slot_prefix = slot_prefix; so.slot_chunk0 = slot_chunk0; so.slot_n = slot_n; so.slot_label_off = slot_label_off;
        so.repeat_flag = repeat_flag; so.pair_count = pair_count; so.owner = owner; so.me = me; so.qlim = qlim; so.R = R;
        so.slot_exact = slot_exact; so.pair_count2 = pair_count2; so.plain0 = plain0; so.pair_count3 = pair_count3;
        hipLaunchKernelGGL(make_slots_wave_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, probes, kc, nq, so);
        return;
    }
    hipLaunchKernelGGL(make_slots_kernel, dim3((unsigned)((nq + 127) / 128)), dim3(128), 0, s,
                       probes, kc, nq, n_lists, list_chunk_off, list_n, ids_off, slot_prefix,
                       slot_chunk0, slot_n, slot_label_off, repeat_flag, pair_count, owner, me,
                       qlim, R, slot_exact, pair_count2, plain0, pair_count3);
}
