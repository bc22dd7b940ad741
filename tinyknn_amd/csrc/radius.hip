// radius.hip — every row within a radius of each query, exactly (IVF.radius_search): the other
// standard question of a vector index beside "the k nearest" — FAISS's range_search, scikit-learn's radius_neighbors.
//
// A row j is a hit of query i iff it passes the query's restriction (TkBruteRestrict, as knn_brute's) and
//   part[i][j] <= radius[i]        float32, inclusive
// with part the value brute.hip ranks by, so for every k the ids of knn_brute_dist(k) are the first k entries of the
// list at radius = part[k - 1].  The tile loop and the part expression are brute_tile.h's: a copy of the loop of
// brute_tiles_kernel with the per-pair action as a parameter.  brute.hip itself keeps its own text — built on the
// header its four forms took the same registers or fewer, but knn_brute measured 2 – 4 % slower than the parent
// (profiles/r24/bench_parent_vs_change.txt), so it stays byte for byte — and tests/test_radius_gpu.py holds the two
// to the same bits.  A list has no fixed capacity, so the append of brute.hip's pass B becomes
//   count   radius_tiles_kernel<false>: hits per query -> count[q] (int32; N < 2^31)
//   offsets the caller's: the counts to the host, their exclusive prefix sum in int64 (the CSR `lims`), checked against
//           the caller's limit, and back to the device
//   fill    radius_tiles_kernel<true>: the same pass again; hit -> keys[offset[q] + slot], slot from a second, zeroed
//           counter per query.  The key is brute.hip's: float bits made monotone in the high word, the row id in the
//           low word, so u64 order is (part, id) order.  A store is guarded by slot < count[q]: a fill can never write
//           outside its query's segment; were the two passes to disagree, the error flag is raised instead.
//   sort    rocprim::segmented_radix_sort_keys over all 64 bits, the offsets as segment bounds: lists of any length
//           (brute_select_kernel's LDS sort ends at 8 192 entries).  Skipped for an unsorted result.
//   decode  keys -> int64 ids and float32 part values (the monotone map inverted)
// Atomics are aggregated per wave (HIP guide, guideline 12): an accumulator register v holds one query row per 32-lane
// half against 32 columns, so the hit predicate is ballotted per v, one lane per half adds the half's popcount and
// every hit lane takes base + popcount(hits below it) — one atomic per (wave, tile, query row) with hits instead of one
// per hit.  A wide radius makes every lane a hit on the same address; this is what keeps that case from serialising.
// Clamped query rows (row >= nq) and columns past the end never vote.
// Grid and LDS layout are pass B's: 128 queries per workgroup, blockIdx.y splitting the rows of Y when queries are few.
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "brute_tile.h"

template <bool FILL, bool RESTRICTED>
__global__ __launch_bounds__(256) void radius_tiles_kernel(
    const float *__restrict__ X, int64_t nq, int d, const float *__restrict__ Y,
    const float *__restrict__ ynorm2, int64_t N, const float *__restrict__ radius, int *__restrict__ count,
    const int64_t *__restrict__ offset, int *__restrict__ slots, unsigned long long *__restrict__ keys,
    int *__restrict__ err, TkBruteRestrict r)
{
    const int col = threadIdx.x & 31, half = (threadIdx.x & 63) >> 5;
    float rq[16];
#pragma unroll
    for (int v = 0; v < 16; v++) rq[v] = radius[brute_tile_query(v, nq)];
    brute_tile_loop<RESTRICTED>(
        X, nq, d, Y, ynorm2, N, r,
        [&](int v, int64_t row, int64_t j, float part, bool live, auto passes) {
            bool h = live && part <= rq[v];
            if constexpr (RESTRICTED)
                if (h) h = passes();
            const unsigned long long m = __ballot(h);
            const uint32_t mh = half ? (uint32_t)(m >> 32) : (uint32_t)m;      // the hits of this half's query row
            const int leader = mh ? __ffs(mh) - 1 : 0;
            if constexpr (!FILL) {
                if (h && col == leader) atomicAdd(&count[row], __popc(mh));
            } else {
                int base = 0;
                if (h && col == leader) base = atomicAdd(&slots[row], __popc(mh));
                base = __shfl(base, half * 32 + leader);
                if (h) {
                    const uint32_t slot = (uint32_t)(base + __popc(mh & ((1u << col) - 1u)));
                    if (slot < (uint32_t)count[row]) {
                        uint32_t u = __float_as_uint(part);
                        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                        keys[offset[row] + slot] = ((unsigned long long)u << 32) | (uint32_t)j;
                    } else {
                        atomicOr(err, 1);
                    }
                }
            }
        });
}

// keys -> row ids and part values
__global__ void radius_decode_kernel(const unsigned long long *__restrict__ keys, int64_t n, int64_t *__restrict__ ids,
                                     float *__restrict__ dist)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const uint32_t u = (uint32_t)(k >> 32);
    ids[i] = (int64_t)(uint32_t)k;
    dist[i] = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

static int radius_attrs()
{
    static bool attr_set = false;
    if (!attr_set) {
        const void *fns[] = {(const void *)radius_tiles_kernel<false, false>, (const void *)radius_tiles_kernel<true, false>,
                             (const void *)radius_tiles_kernel<false, true>, (const void *)radius_tiles_kernel<true, true>};
        for (const void *f : fns)
            if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
                return -1;
        attr_set = true;
    }
    return 0;
}

template <bool FILL>
static int radius_tiles(const float *X, int64_t nq, int d, const float *Y, int64_t N, const float *ynorm2,
                        const float *radius, int *count, const int64_t *offset, int *slots, unsigned long long *keys,
                        int *err, const TkBruteRestrict *r, hipStream_t s)
{
    if (nq <= 0 || N <= 0) return 0;
    if (d > 128 || N >= (1ll << 31) || radius_attrs()) return -1;
    const dim3 grid = brute_tile_grid(nq, N);
    if (r)
        hipLaunchKernelGGL((radius_tiles_kernel<FILL, true>), grid, dim3(256), brute_tile_lds(d) + tile_attr_bytes(*r),
                           s, X, nq, d, Y, ynorm2, N, radius, count, offset, slots, keys, err, *r);
    else
        hipLaunchKernelGGL((radius_tiles_kernel<FILL, false>), grid, dim3(256), brute_tile_lds(d), s, X, nq, d, Y,
                           ynorm2, N, radius, count, offset, slots, keys, err, TkBruteRestrict{});
    return 0;
}

// |y_j|^2 in numpy's einsum order: brute.hip's kernel, launched from here as knn_brute launches it
__global__ void row_norms_kernel(const float *__restrict__ Y, int64_t n, int d, float *__restrict__ out);

// X (nq, d), Y (N, d), radius (nq) float32 on the device, d <= 128, N < 2^31.  ynorm2 (N) is the caller's and takes
// the norms of Y (row_norms_kernel, per call as in knn_brute: add() and update() are seen); count (nq) int32 is
// zeroed here and takes every query's number of hits.
int tk_launch_radius_count(const float *X, int64_t nq, int d, const float *Y, int64_t N, float *ynorm2,
                           const float *radius, int *count, const TkBruteRestrict *r, hipStream_t s)
{
    if (nq <= 0) return 0;
    if (N > 0)
        hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, Y, N, d, ynorm2);
    (void)hipMemsetAsync(count, 0, (size_t)nq * 4, s);
    return radius_tiles<false>(X, nq, d, Y, N, ynorm2, radius, count, nullptr, nullptr, nullptr, nullptr, r, s);
}

// The second pass: count as the first left it, offset (nq) int64 its exclusive prefix sum, keys (sum of count) u64;
// slots (nq) int32 and err (1) int32 are zeroed here.  err != 0 afterwards: the passes disagreed (no store was made
// outside a query's segment).
int tk_launch_radius_fill(const float *X, int64_t nq, int d, const float *Y, int64_t N, const float *ynorm2,
                          const float *radius, int *count, const int64_t *offset, int *slots,
                          unsigned long long *keys, int *err, const TkBruteRestrict *r, hipStream_t s)
{
    if (nq <= 0) return 0;
    (void)hipMemsetAsync(slots, 0, (size_t)nq * 4, s);
    (void)hipMemsetAsync(err, 0, 4, s);
    return radius_tiles<true>(X, nq, d, Y, N, ynorm2, radius, count, offset, slots, keys, err, r, s);
}

// Every list ascending by (part, id): keys_in -> keys_out, total < 2^32 keys in nq segments bounded by offsets (nq + 1).
// tmp == NULL: only *tmp_bytes is set (the work memory the sort asks for).
int tk_launch_radius_sort(void *tmp, size_t *tmp_bytes, const unsigned long long *keys_in, unsigned long long *keys_out,
                          int64_t total, int64_t nq, const int64_t *offsets, hipStream_t s)
{
    if (total >= (1ll << 32) || nq >= (1ll << 32)) return -1;
    size_t bytes = tmp ? *tmp_bytes : 0;
    const hipError_t e = rocprim::segmented_radix_sort_keys(tmp, bytes, keys_in, keys_out, (unsigned)total,
                                                            (unsigned)nq, offsets, offsets + 1, 0, 64, s);
    if (!tmp) *tmp_bytes = bytes;
    return e == hipSuccess ? 0 : -1;
}

void tk_launch_radius_decode(const unsigned long long *keys, int64_t n, int64_t *ids, float *dist, hipStream_t s)
{
    if (n > 0)
        hipLaunchKernelGGL(radius_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, n, ids, dist);
}
