// span_exact.h — the walk that the exact searches over a span of row ids share: group_exact.hip (a query's group,
// DESIGN §3.17) and value_exact.hip (a query's value range, §3.18).  One workgroup per query.  The span — `n` row ids,
// in any order — is walked in tiles of GX_TILE rows, a lane a row: rows that are not stored or fail a restriction
// (allowed bit, exclude, group where the form tests it, tags any / all, ranges — by row id, the formulas of brute.hip's
// restricted form; the query's own attributes sit in scalar registers) are dropped, the others get sqdist_row<T, TY>
// (sqdist_row.h: the rescoring's distance, numpy's einsum order bit for bit) and, where that is not above the query's
// bound, a slot in a candidate buffer in LDS: GX_CAP entries of (distance key, row id).  In front of a tile that could
// overflow the buffer it is cut back: sorted by (distance, row id) — a bitonic sort over the entries it holds — cut to
// its k best, the bound tightened to the k-th distance.  "Could": the count the decision uses is an upper bound kept in
// a register (entries after the last cut + GX_TILE per tile since), so the tile loop has no barrier and the waves of a
// workgroup stream through their rows independently.  The last cut is the result: ascending by (distance, row id),
// -1 / +inf behind fewer than k survivors — the same whatever order the span lists its rows in.
#pragma once
#include "kernels.h"
#include "sqdist_row.h"

#define GX_THREADS 256
#define GX_TILE 256       // rows of the span per pass of the workgroup: a lane a row
#define GX_CAP 2048       // entries of the candidate buffer; k + GX_TILE <= GX_CAP for every k <= 1024

// the distance as an unsigned key that orders as the distance does (a NaN, which no finite data gives, sorts last)
template <typename T> struct GxKey;
template <> struct GxKey<float> {
    typedef uint32_t type;
    __device__ static type of(float v)
    {
        const uint32_t u = __float_as_uint(v);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    __device__ static float back(type u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
};
template <> struct GxKey<double> {
    typedef uint64_t type;
    __device__ static type of(double v)
    {
        const uint64_t u = (uint64_t)__double_as_longlong(v);
        return (u >> 63) ? ~u : (u | (1ull << 63));
    }
    __device__ static double back(type u)
    {
        return __longlong_as_double((long long)((u >> 63) ? (u & ~(1ull << 63)) : ~u));
    }
};

// LDS: kd[GX_CAP] distance keys | kid[GX_CAP] row ids | x[d] the query in T
static inline size_t gx_lds_bytes(int d, size_t key_bytes, size_t t_bytes)
{
    return (size_t)GX_CAP * (key_bytes + 4) + (size_t)d * t_bytes;
}

// The body of a kernel of GX_THREADS lanes, gx_lds_bytes of dynamic LDS, block qi = query qi.
// span / n: the query's row ids.  stored: the N-bit map of stored rows.  r: the restriction's device arrays
// (TkBruteRestrict); GROUPS: r.group / r.row_groups are tested (group[qi] < 0: any group) — false where the span IS the
// group and the two fields are not read.
template <typename T, typename TY, bool GROUPS>
__device__ __forceinline__ void span_exact_body(const float *__restrict__ q, int d, const TY *__restrict__ rows,
                                                const int32_t *__restrict__ span, const int n,
                                                const uint32_t *__restrict__ stored, const TkBruteRestrict &r, int k,
                                                int64_t *__restrict__ out, T *__restrict__ out_d)
{
    typedef typename GxKey<T>::type K;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    K *kd = (K *)smem;
    int32_t *kid = (int32_t *)(kd + GX_CAP);
    T *xs = (T *)(kid + GX_CAP);
    __shared__ int s_count;
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    for (int t = tid; t < d; t += GX_THREADS) xs[t] = (T)q[qi * d + t];
    if (tid == 0) s_count = 0;
    // the query's own attributes, once
    const int32_t q_ex = r.exclude ? (int32_t)r.exclude[qi] : -1;      // (entries lie in [-1, N), N < 2^31)
    const uint64_t q_tags = r.tags ? r.tags[qi] : 0;
    const int32_t q_group = (GROUPS && r.group) ? r.group[qi] : -1;
    int64_t q_lo[4] = {0, 0, 0, 0}, q_hi[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; c++)
        if (c < r.cols) {
            q_lo[c] = r.ranges[(qi * r.cols + c) * 2];
            q_hi[c] = r.ranges[(qi * r.cols + c) * 2 + 1];
        }
    K tau = ~(K)0;          // the bound: the k-th distance key of the last cut
    int kept = 0;           // entries the buffer holds at most (an upper bound, the same in every lane)

    // Sort what the buffer holds by (distance, row id), keep the k best, tighten the bound.  Every lane arrives.
    auto cut = [&]() {
        __syncthreads();                        // every append so far is in LDS (and the first time: xs, s_count)
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
        __syncthreads();                        // the count is back before the next append, tau read before it
    };

    __syncthreads();                            // xs and the zero count, before the first append
    for (int t0 = 0; t0 < n; t0 += GX_TILE) {
        if (kept + GX_TILE > GX_CAP) cut();
        kept += GX_TILE;
        const int t = t0 + tid;
        if (t >= n) continue;
        const int32_t rid = span[t];
        bool ok = (stored[rid >> 5] >> (rid & 31)) & 1u;
        if (r.allowed) ok &= (r.allowed[rid >> 5] >> (rid & 31)) & 1u;
        ok &= rid != q_ex;
        if (!ok) continue;
        if (GROUPS && q_group >= 0 && r.row_groups[rid] != q_group) continue;
        if (q_tags != 0) {
            const uint64_t rt = r.row_tags[rid];
            if (!(r.tag_mode ? (rt & q_tags) == q_tags : (rt & q_tags) != 0)) continue;
        }
        // (The GROUPS form also holds the query's group and the groups' base in scalar registers and has none to spare
        // for the four plane bases — its float64 form spilled six: it walks the planes by a pointer of the lane.)
        const int64_t *kc = r.row_keys + rid;
#pragma unroll
        for (int c = 0; c < 4; c++)
            if (c < r.cols) {
                const int64_t key = GROUPS ? *kc : r.row_keys[c * r.n_rows + rid];
                if (GROUPS) kc += r.n_rows;
                ok &= q_lo[c] <= key && key <= q_hi[c];
            }
        if (!ok) continue;
        const T dv = sqdist_row<T, TY>(rows + (int64_t)rid * d, xs, d);
        const K key = GxKey<T>::of(dv);
        if (key <= tau) {
            const int pos = atomicAdd(&s_count, 1);
            if (pos < GX_CAP) {                 // (always: kept bounds the count)
                kd[pos] = key;
                kid[pos] = rid;
            }
        }
    }
    cut();
    for (int e = tid; e < k; e += GX_THREADS) {
        out[qi * k + e] = e < kept ? (int64_t)kid[e] : -1;
        if (out_d) out_d[qi * k + e] = e < kept ? GxKey<T>::back(kd[e]) : (T)__builtin_huge_valf();
    }
}
