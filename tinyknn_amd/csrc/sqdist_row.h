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
