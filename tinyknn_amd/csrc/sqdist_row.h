// sqdist_row.h — the squared distance of one stored row to a query in numpy's einsum order: the one text that the
// rescoring (rescore.hip) and the exact search inside a group (group_exact.hip) rank by, so their distances are the
// same bits and mix freely.  Built with -ffp-contract=off.
#pragma once

// (tried: nontemporal loads of the candidate rows, so that they would not evict the scan
// kernels' code and table lines from L2 — 2.5x slower alone, 0.135 -> 0.332 ms per 10 000
// queries, and the scan beside it 0.61 -> 0.79 ms: a lane fetches its row in 25 pieces of 16 B
// and an uncached piece is a memory transaction of its own.  -DTK_NT=1 rebuilds that.)
#ifndef TK_NT
#define TK_NT 0
#endif

// (tried: the 16-byte pieces of three groups requested before the first is used — 3 dependent
// trips to memory per 100-float row instead of 7, 77 VGPRs instead of 44: 0.138 -> 0.150 ms alone
// and the batch 0.650 -> 0.693 ms; the kernel's cost to its neighbours is the NUMBER of
// line visits, and bunching them makes it worse.  `#pragma unroll 4` alone changes nothing: the
// compiler keeps each group's loads behind the previous group's arithmetic.)
// squared distance of row y to the query xs in numpy's einsum order, computed in T
// (float when both operands are float32, else double as numpy promotes): L = 16 /
// sizeof(T) lane-accumulators, groups of 4 vectors folded 3,2,1,0, zero tail.
template <typename T, typename TY>
__device__ __forceinline__ T sqdist_row(const TY *__restrict__ y, const T *xs, int d)
{
    constexpr int L = 16 / (int)sizeof(T);
    T acc[L];
#pragma unroll
    for (int l = 0; l < L; l++) acc[l] = 0;
    int i = 0;
    for (; d - i >= 4 * L; i += 4 * L) {
        T df[4 * L];
#pragma unroll
        for (int t = 0; t < 4 * L; t++) df[t] = (T)(TK_NT ? __builtin_nontemporal_load(y + i + t) : y[i + t]) - xs[i + t];
#pragma unroll
        for (int l = 0; l < L; l++) {
            T ab3 = df[3 * L + l] * df[3 * L + l] + acc[l];
            T ab2 = df[2 * L + l] * df[2 * L + l] + ab3;
            T ab1 = df[L + l] * df[L + l] + ab2;
            acc[l] = df[l] * df[l] + ab1;
        }
    }
    for (; i < d; i += L) {
#pragma unroll
        for (int l = 0; l < L; l++) {
            T df = (i + l < d) ? ((T)y[i + l] - xs[i + l]) : (T)0;
            acc[l] = df * df + acc[l];
        }
    }
    if (L == 4) return (acc[0] + acc[1]) + (acc[2 % L] + acc[3 % L]);
    return acc[0] + acc[1 % L];
}

// The 4-query form (probe_exact.hip): one row against four queries in one walk over d.  y is a row staged in LDS, x[0..3]
// four queries in LDS, all 16-byte aligned; every 16-byte piece of the row is read once (sq4_load: one 16-byte read a
// piece) and feeds four sets of the lane-accumulators above.  Per query the operations and their order are
// sqdist_row's exactly — the difference, the square, the folds 3, 2, 1, 0, the zero tail, the final pairing — so out[u]
// has the bits of sqdist_row(y, x[u], d).
template <typename T, typename E, int CNT>
__device__ __forceinline__ void sq4_load(const E *p, T *dst)
{
    constexpr int N = 16 / (int)sizeof(E);
    typedef E vec __attribute__((ext_vector_type(N)));
#pragma unroll
    for (int c = 0; c < CNT / N; c++) {
        const vec v = ((const vec *)p)[c];
#pragma unroll
        for (int t = 0; t < N; t++) dst[c * N + t] = (T)v[t];
    }
}

template <typename T, typename TY>
__device__ __forceinline__ void sqdist_row4(const TY *__restrict__ y, const T *const x[4], int d, T out[4])
{
    constexpr int L = 16 / (int)sizeof(T);
    T acc[4][L];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int l = 0; l < L; l++) acc[u][l] = 0;
    int i = 0;
    for (; d - i >= 4 * L; i += 4 * L) {
        T yv[4 * L];
        sq4_load<T, TY, 4 * L>(y + i, yv);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            T df[4 * L];
            sq4_load<T, T, 4 * L>(x[u] + i, df);
#pragma unroll
            for (int t = 0; t < 4 * L; t++) df[t] = yv[t] - df[t];
#pragma unroll
            for (int l = 0; l < L; l++) {
                T ab3 = df[3 * L + l] * df[3 * L + l] + acc[u][l];
                T ab2 = df[2 * L + l] * df[2 * L + l] + ab3;
                T ab1 = df[L + l] * df[L + l] + ab2;
                acc[u][l] = df[l] * df[l] + ab1;
            }
        }
    }
    for (; i < d; i += L) {
#pragma unroll
        for (int l = 0; l < L; l++) {
            const bool in = i + l < d;
            const T yv = in ? (T)y[i + l] : (T)0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                T df = in ? (yv - x[u][i + l]) : (T)0;
                acc[u][l] = df * df + acc[u][l];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
        out[u] = (L == 4) ? (acc[u][0] + acc[u][1]) + (acc[u][2 % L] + acc[u][3 % L]) : acc[u][0] + acc[u][1 % L];
}

// The 4-query form cut into pieces along d (probe_exact.hip's wide kernel): the accumulator sets of NI items — one row
// against NI quads of queries — live in the caller's registers while d is walked in slabs whose length is a multiple of
// 4 * L, so every slab edge falls between two iterations of the main loop above.  sq4_init, then per slab sq4_groups
// over the slab's whole groups (y and x[it][u] point at the slab's first element), in the last slab sq4_tail, then
// sq4_finish: per query sqdist_row4's operations in sqdist_row4's order, the same bits.  An item whose on[it] is false
// is left alone; the row's pieces are read once a group for all NI items.
template <typename T, int NI>
__device__ __forceinline__ void sq4_init(T (&acc)[NI][4][16 / sizeof(T)])
{
#pragma unroll
    for (int it = 0; it < NI; it++)
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int l = 0; l < 16 / (int)sizeof(T); l++) acc[it][u][l] = 0;
}

template <typename T, typename TY, int NI>
__device__ __forceinline__ void sq4_groups(const TY *__restrict__ y, const T *const (&x)[NI][4], const bool (&on)[NI],
                                           int n, T (&acc)[NI][4][16 / sizeof(T)])
{
    constexpr int L = 16 / (int)sizeof(T);
    for (int g = 0; g < n; g++) {
        const int i = g * 4 * L;
        T yv[4 * L];
        sq4_load<T, TY, 4 * L>(y + i, yv);
#pragma unroll
        for (int it = 0; it < NI; it++) {
            if (!on[it]) continue;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                T df[4 * L];
                sq4_load<T, T, 4 * L>(x[it][u] + i, df);
#pragma unroll
                for (int t = 0; t < 4 * L; t++) df[t] = yv[t] - df[t];
#pragma unroll
                for (int l = 0; l < L; l++) {
                    T ab3 = df[3 * L + l] * df[3 * L + l] + acc[it][u][l];
                    T ab2 = df[2 * L + l] * df[2 * L + l] + ab3;
                    T ab1 = df[L + l] * df[L + l] + ab2;
                    acc[it][u][l] = df[l] * df[l] + ab1;
                }
            }
        }
    }
}

// the zero-padded tail: the elements [i, i + rem) of the slab, rem < 4 * L, in steps of L
template <typename T, typename TY, int NI>
__device__ __forceinline__ void sq4_tail(const TY *__restrict__ y, const T *const (&x)[NI][4], const bool (&on)[NI],
                                         int i, int rem, T (&acc)[NI][4][16 / sizeof(T)])
{
    constexpr int L = 16 / (int)sizeof(T);
    for (const int end = i + rem; i < end; i += L) {
#pragma unroll
        for (int l = 0; l < L; l++) {
            const bool in = i + l < end;
            const T yv = in ? (T)y[i + l] : (T)0;
#pragma unroll
            for (int it = 0; it < NI; it++) {
                if (!on[it]) continue;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    T df = in ? (yv - x[it][u][i + l]) : (T)0;
                    acc[it][u][l] = df * df + acc[it][u][l];
                }
            }
        }
    }
}

template <typename T, int NI>
__device__ __forceinline__ void sq4_finish(const T (&acc)[NI][4][16 / sizeof(T)], T (&out)[NI][4])
{
    constexpr int L = 16 / (int)sizeof(T);
#pragma unroll
    for (int it = 0; it < NI; it++)
#pragma unroll
        for (int u = 0; u < 4; u++)
            out[it][u] = (L == 4) ? (acc[it][u][0] + acc[it][u][1]) + (acc[it][u][2 % L] + acc[it][u][3 % L])
                                  : acc[it][u][0] + acc[it][u][1 % L];
}
