// brute.hip — exact k nearest rows, the ground truth of every recall figure
// (knn_brute, utils.py:66-86, as the reference's benches use it: examples/bench.py:85);
// the one dense contraction around the path.
//
//   part[i][j] = (|x_i|^2 + |y_j|^2) - (2 x_i) . y_j          utils.py:84
// on the f32 matrix cores: v_mfma_f32_32x32x2_f32 is bit-for-bit the f32 FMA chain over k
// ascending (MI355X guide, "FP32-input MFMA"), i.e. what OpenBLAS returns for (2X) @ Y.T, and
// the norms use numpy's einsum order (np_order.h) — the part values are numpy's.
// Selection of the k smallest without data-dependent loops:
//   pass A  part values of `ns` rows of Y taken at a constant stride over the whole matrix
//           (not its first rows: cluster-ordered data would give a useless bound) -> (nq, ns)
//   sort    per query: k-th smallest of them = tau_q           (bitonic sort in LDS)
//   pass B  the rows of Y in segments of `seg` rows: every (part, j) with part <= tau_q is
//           appended to the query's candidate list (atomic counter, capacity `cap`); after
//           each segment the list is sorted, cut to its k best and tau_q tightened to the k-th
//           of them, so a segment adds about k * seg / max(ns, rows seen) entries whatever N is
//   result  the k best after the last segment, by (part, j) ascending.  Ties: lower j first.
// Segment length (brute_segment).  tau_q is the k-th smallest of ns sampled rows, so of
// `seg` rows about k * seg / ns lie within it.  That count is an order statistic's: its
// relative spread is 1 / sqrt(k), and rows that are not in random order (a query's cluster
// stored together) raise a segment's share further.  seg is therefore the largest power of two
// with k * seg / ns <= cap / 4, a factor 4 below the capacity, and never more than 2^20:
//   seg = min(2^20, 2^floor(log2(cap * ns / (4 k))))
// With ns = cap = 8192 that is 2^20 for k <= 16, 2^17 for k = 100 and 2^14 for k = 1024.
// A list that overflows all the same is reported (`overflow`) and the call fails; it is never
// cut silently.  That remains for more than `cap` rows of one segment within tau_q: exact ties
// (duplicated rows), or a query whose near rows are stored together so that one segment holds
// more than 4 times its share of them.
// Restricted (tk_index_knn_brute_ex): the k nearest among the rows that pass a query's restriction
// (TkBruteRestrict).  The predicate enters pass A (a failing (query, sample row) pair counts as +inf, so tau is the k-th
// smallest over the passing sample rows and +inf below k of them) and pass B (tested before the append: a failing row
// takes no slot and never tightens tau).  There an overflow is not an error: the caller repeats pass B once from the
// sampled tau with seg = the largest multiple of 32 not above cap - k, and a segment that appends at most seg rows to
// at most k kept ones cannot overflow.
// One workgroup = 4 waves = 128 query rows against 32 rows of Y at a time; the Y tile (32
// consecutive rows = one contiguous block of memory) is fetched once per workgroup into LDS
// in MFMA operand order, double-buffered.
#include "kernels.h"
#include "np_order.h"

typedef float tk_f32x16 __attribute__((ext_vector_type(16)));

// |y_j|^2 in numpy's einsum order
__global__ void row_norms_kernel(const float *__restrict__ Y, int64_t n, int d, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = einsum_selfdot<float>(Y + i * d, d);
}

// The attributes of a workgroup's 128 queries, staged in LDS behind the tiles (RESTRICTED), only those of the
// restrictions given: ranges [128][2 cols] int64 (lo_0, hi_0, lo_1, ...), tags [128] uint64, exclude [128] int32
// (N < 2^31), group [128] int32 — 4 to 84 bytes a query.  At d = 100 the tiles take 76 800 bytes, so two workgroups
// share a CU's 160 KB as long as a query's attributes fit 40 bytes: every form but two or more value columns.
__host__ __device__ static inline size_t brute_attr_bytes(const TkBruteRestrict &r)
{
    return (size_t)128 * (16 * r.cols + (r.tags ? 8 : 0) + (r.exclude ? 4 : 0) + (r.group ? 4 : 0));
}

// MODE 0: write part values of rows [0, ns) of Y to vals (nq, ns).
// MODE 1: append (part, j) with part <= tau[row] to cand (nq, cap) / count (nq,).
// RESTRICTED: column j of Y is row j_base + j * j_stride of the index (MODE 0: the strided sample), and a (query,
// row) pair counts only where the row passes the query's restriction r: MODE 0 writes +inf for the others, MODE 1
// tests the pair before the append, so a failing row neither takes a slot of the list nor tightens tau.  A lane owns
// one column per tile: it loads that row's attributes once per tile (allowed bit, group, tags, up to 4 keys: 12
// registers); the queries' attributes wait in LDS and are read only for the pairs within tau.
template <int MODE, bool RESTRICTED>
__global__ __launch_bounds__(256) void brute_tiles_kernel(
    const float *__restrict__ X, int64_t nq, int d, const float *__restrict__ Y,
    const float *__restrict__ ynorm2, int64_t N, float *__restrict__ vals, int64_t ns,
    const float *__restrict__ tau, unsigned long long *__restrict__ cand, int cap,
    int *__restrict__ count, int64_t j_base, int64_t j_stride, TkBruteRestrict r)
{
    const int lane = threadIdx.x & 63, half = lane >> 5, col = lane & 31;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    const int64_t my_row = r0 + col < nq ? r0 + col : nq - 1;
    const int KT = (d + 1) >> 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *a = (float *)smem + (size_t)(threadIdx.x >> 6) * KT * 64;     // A operands [t][lane]
    float *bt = (float *)smem + (size_t)4 * KT * 64;                      // B tiles [2][t][lane]
    int64_t *q_ranges = (int64_t *)((float *)smem + (size_t)6 * KT * 64);
    uint64_t *q_tags = (uint64_t *)(q_ranges + 128 * 2 * r.cols);
    int32_t *q_exclude = (int32_t *)(q_tags + (r.tags ? 128 : 0));
    int32_t *q_group = q_exclude + (r.exclude ? 128 : 0);
    if constexpr (RESTRICTED) {
        // (made visible by the barrier in front of the tile loop)
        if (threadIdx.x < 128) {
            const int t = threadIdx.x;
            int64_t row = (int64_t)blockIdx.x * 128 + t;
            row = row < nq ? row : nq - 1;
            if (r.exclude) q_exclude[t] = (int32_t)r.exclude[row];
            if (r.tags) q_tags[t] = r.tags[row];
            if (r.group) q_group[t] = r.group[row];
            for (int c = 0; c < 2 * r.cols; c++) q_ranges[t * 2 * r.cols + c] = r.ranges[row * 2 * r.cols + c];
        }
    }
    for (int t = 0; t < KT; t++) {
        const int kk = 2 * t + half;
        a[t * 64 + lane] = kk < d ? 2.0f * X[my_row * d + kk] : 0.0f;
    }
    float xn[16], tq[16];
#pragma unroll
    for (int v = 0; v < 16; v++) {
        int64_t row = r0 + (v & 3) + 8 * (v >> 2) + 4 * half;
        row = row < nq ? row : nq - 1;
        xn[v] = einsum_selfdot<float>(X + row * d, d);
        tq[v] = MODE == 1 ? tau[row] : 0.0f;
    }
    // blockIdx.y splits the rows of Y: few queries (a recall sample) would otherwise occupy a
    // handful of CUs; appends are atomic, so the split does not change the result
    const int64_t all_cols = MODE == 0 ? ns : N;
    const int64_t per_y = ((all_cols + gridDim.y - 1) / gridDim.y + 31) / 32 * 32;
    const int64_t c_begin = (int64_t)blockIdx.y * per_y;
    const int64_t ncols = c_begin + per_y < all_cols ? c_begin + per_y : all_cols;
    // B tile of rows [j0, j0+32): element (t, l) = Y[j0 + (l & 31)][2t + (l >> 5)].  The 32
    // rows are contiguous in memory: thread e reads float e of the block (coalesced) and
    // drops it at its operand position.
    const int tile_f = 32 * d;
    constexpr int PER = 32 * 128 / 256;        // floats per thread and tile at d <= 128
    float stage[PER];
    auto fetch = [&](int64_t j0) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int e = u * 256 + (int)threadIdx.x;
            // rows past the range read as zeros: element e belongs to row j0 + e / d, so it is
            // in range iff e < (ncols - j0) * d
            float val = 0.0f;
            if (e < tile_f && (int64_t)e < (ncols - j0) * d) val = Y[j0 * d + e];
            stage[u] = val;
        }
    };
    // operand position of this thread's tile elements (the same for every tile)
    int dst[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int e = u * 256 + (int)threadIdx.x;
        const int jj = e / d, kk = e - jj * d;
        dst[u] = e < tile_f ? (kk >> 1) * 64 + (kk & 1) * 32 + jj : -1;
    }
    auto commit = [&](int buf) {
#pragma unroll
        for (int u = 0; u < PER; u++)
            if (dst[u] >= 0) bt[(size_t)buf * KT * 64 + dst[u]] = stage[u];
    };
    if (d & 1)      // odd d: the k = d operands of the upper half-wave are zero in both buffers
        for (int e = threadIdx.x; e < 2 * 32; e += 256)
            bt[(size_t)(e >> 5) * KT * 64 + (KT - 1) * 64 + 32 + (e & 31)] = 0.0f;
    if (c_begin < ncols) {
        fetch(c_begin);
        commit(0);
    }
    __syncthreads();
    int buf = 0;
    for (int64_t j0 = c_begin; j0 < ncols; j0 += 32, buf ^= 1) {
        const bool more = j0 + 32 < ncols;
        if (more) fetch(j0 + 32);
        const int64_t j = j0 + col;
        // this lane's row of the index and what restricts it
        int64_t rid = 0, rkey[4] = {0, 0, 0, 0};
        uint64_t rtags = 0;
        int32_t rgroup = 0;
        bool row_ok = j < ncols;
        if constexpr (RESTRICTED) {
            if (row_ok) {
                rid = j_base + j * j_stride;
                if (r.allowed) row_ok = (r.allowed[rid >> 5] >> (rid & 31)) & 1u;
                if (r.group) rgroup = r.row_groups[rid];
                if (r.tags) rtags = r.row_tags[rid];
#pragma unroll
                for (int c = 0; c < 4; c++)
                    if (c < r.cols) rkey[c] = r.row_keys[c * r.n_rows + rid];
            }
        }
        // does the lane's row pass the restriction of local query ql (its attributes from LDS)?
        auto passes = [&](int ql) {
            bool ok = true;
            if (r.exclude) ok = (int32_t)rid != q_exclude[ql];
            if (r.group) {
                const int32_t g = q_group[ql];
                ok &= g < 0 || rgroup == g;
            }
            if (r.tags) {
                const uint64_t t = q_tags[ql];
                ok &= t == 0 || (r.tag_mode ? (rtags & t) == t : (rtags & t) != 0);
            }
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (c < r.cols) {
                    const int64_t *b = q_ranges + (ql * r.cols + c) * 2;
                    ok &= b[0] <= rkey[c] && rkey[c] <= b[1];
                }
            return ok;
        };
        tk_f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; v++) acc[v] = 0.0f;
        const float *bb = bt + (size_t)buf * KT * 64;
#pragma unroll 4
        for (int t = 0; t < KT; t++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t * 64 + lane], bb[t * 64 + lane], acc, 0, 0, 0);
        // (MODE 0 writes every column of the sample: +inf where the row is not allowed)
        if (MODE == 0 ? j < ncols : row_ok) {
            const float yn = ynorm2[j];
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int ql = (v & 3) + 8 * (v >> 2) + 4 * half;
                const int64_t row = r0 + ql;
                const float part = (xn[v] + yn) - acc[v];
                if (row < nq) {
                    if (MODE == 0) {
                        float val = part;
                        if constexpr (RESTRICTED)
                            if (!row_ok || !passes((int)(threadIdx.x >> 6) * 32 + ql)) val = __builtin_inff();
                        vals[row * ns + j] = val;
                    } else if (part <= tq[v] && (!RESTRICTED || passes((int)(threadIdx.x >> 6) * 32 + ql))) {
                        const int pos = atomicAdd(&count[row], 1);
                        if (pos < cap) {
                            // order-preserving key: float bits made monotone, then the index
                            uint32_t u = __float_as_uint(part);
                            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                            cand[row * (int64_t)cap + pos] = ((unsigned long long)u << 32) | (uint32_t)(j_base + j);
                        }
                    }
                }
            }
        }
        if (more) commit(buf ^ 1);
        __syncthreads();
    }
}

// Bitonic sort of up to TK_BR_SORT 64-bit keys per query in LDS (one workgroup per query).
// MODE 0: keys = part values of the sample (index ignored) -> tau[q] = k-th smallest.
// MODE 1: keys = candidates (part, j) -> out[q][0..k) = j of the k smallest; the k smallest
//         stay at the head of the query's list (count = min(k, n)) and tau[q] becomes the
//         k-th part value once k candidates exist: the next segment of rows appends to that.
//         out_dist (or NULL): the part value beside each j, +inf beside -1.
#define TK_BR_SORT 8192
template <int MODE>
__global__ __launch_bounds__(1024) void brute_select_kernel(
    const float *__restrict__ vals, int64_t ns, unsigned long long *__restrict__ cand, int cap,
    int *__restrict__ count, int k, float *__restrict__ tau, int64_t *__restrict__ out,
    int *__restrict__ overflow, float *__restrict__ out_dist)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *key = (unsigned long long *)smem;
    const int64_t q = blockIdx.x;
    int n = MODE == 0 ? (int)ns : count[q];
    if (MODE == 1 && n > cap) {
        if (threadIdx.x == 0) atomicOr(overflow, 1);
        n = cap;
    }
    int P = 1;
    while (P < n) P <<= 1;
    for (int e = threadIdx.x; e < P; e += 1024) {
        unsigned long long kk = ~0ull;
        if (e < n) {
            if (MODE == 0) {
                uint32_t u = __float_as_uint(vals[q * ns + e]);
                u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                kk = ((unsigned long long)u << 32) | (uint32_t)e;
            } else {
                kk = cand[q * (int64_t)cap + e];
            }
        }
        key[e] = kk;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = threadIdx.x; e < P / 2; e += 1024) {
                const int lo = (e / stride) * 2 * stride + (e % stride), hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const unsigned long long x = key[lo], y = key[hi];
                if ((x > y) == up) { key[lo] = y; key[hi] = x; }
            }
            __syncthreads();
        }
    if (MODE == 0) {
        if (threadIdx.x == 0) {
            const uint32_t u = (uint32_t)(key[k - 1 < n ? k - 1 : n - 1] >> 32);
            tau[q] = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
        }
    } else {
        for (int e = threadIdx.x; e < k; e += 1024) {
            out[q * k + e] = e < n ? (int64_t)(uint32_t)key[e] : -1;
            if (e < n) cand[q * (int64_t)cap + e] = key[e];
            if (out_dist) {
                const uint32_t u = (uint32_t)(key[e] >> 32);
                out_dist[q * k + e] = e < n ? __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u) : __builtin_inff();
            }
        }
        if (threadIdx.x == 0) {
            count[q] = n < k ? n : k;
            if (n >= k) {
                const uint32_t u = (uint32_t)(key[k - 1] >> 32);
                tau[q] = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
            }
        }
    }
}

// `ns` rows of Y at stride N / ns (row i * stride) -> a contiguous sample
__global__ void sample_rows_kernel(const float *__restrict__ Y, int d, int64_t ns, int64_t stride,
                                   float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns * d) return;
    const int64_t r = i / d;
    out[i] = Y[r * stride * d + (i - r * d)];
}

// rows per segment of pass B: the largest power of two with k * seg / ns <= cap / 4, at most 2^20
int64_t tk_brute_segment(int k, int64_t ns, int cap)
{
    const int64_t most = (int64_t)cap * ns / (4 * (int64_t)k);
    int64_t seg = 32;
    while (seg < (1 << 20) && 2 * seg <= most) seg <<= 1;
    return seg;
}

static int brute_attrs()
{
    static bool attr_set = false;
    if (!attr_set) {
        const void *fns[] = {(const void *)brute_tiles_kernel<0, false>, (const void *)brute_tiles_kernel<1, false>,
                             (const void *)brute_tiles_kernel<0, true>, (const void *)brute_tiles_kernel<1, true>,
                             (const void *)brute_select_kernel<0>, (const void *)brute_select_kernel<1>};
        for (const void *f : fns)
            if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
                return -1;
        attr_set = true;
    }
    return 0;
}

// One launch of the tile kernel over `cols` columns: enough workgroups for the chip (the rows of Y are split when
// there are few query tiles), the restricted form with its queries' attributes behind the tiles in LDS
template <int MODE>
static void brute_tiles(const float *X, int64_t nq, int d, const float *Y, const float *ynorm2, int64_t cols,
                        float *vals, const float *tau, unsigned long long *cand, int cap, int *count, int64_t j_base,
                        int64_t j_stride, const TkBruteRestrict *r, hipStream_t s)
{
    const int KT = (d + 1) / 2;
    const size_t tile_lds = (size_t)(4 + 2) * KT * 64 * 4;
    const unsigned qt = (unsigned)((nq + 127) / 128);
    int64_t sp = (1024 + qt - 1) / qt;
    const int64_t most = (cols + 1023) / 1024;          // at least 32 tiles per split
    sp = sp < 1 ? 1 : (sp > most ? most : sp);
    const dim3 grid(qt, (unsigned)(sp < 1 ? 1 : sp));
    if (r)
        hipLaunchKernelGGL((brute_tiles_kernel<MODE, true>), grid, dim3(256), tile_lds + brute_attr_bytes(*r), s, X,
                           nq, d, Y, ynorm2, cols, vals, cols, tau, cand, cap, count, j_base, j_stride, *r);
    else
        hipLaunchKernelGGL((brute_tiles_kernel<MODE, false>), grid, dim3(256), tile_lds, s, X, nq, d, Y, ynorm2, cols,
                           vals, cols, tau, cand, cap, count, j_base, j_stride, TkBruteRestrict{});
}

// X (nq, d), Y (N, d) float32 on the device, d <= 128, N < 2^31; ynorm2 (N), vals (nq * ns), tau (nq), sample
// (ns * (d + 1)) floats are the caller's.  ns <= TK_BR_SORT, k <= ns <= N.
int tk_launch_brute_tau(const float *X, int64_t nq, int d, const float *Y, int64_t N, int k, float *ynorm2,
                        float *vals, int64_t ns, float *tau, float *sample, const TkBruteRestrict *r, hipStream_t s)
{
    if (nq == 0) return 0;
    if (d > 128 || ns > TK_BR_SORT || k > ns || ns > N || brute_attrs()) return -1;
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, Y, N, d, ynorm2);
    // tau from a strided sample of the whole matrix (its rows are rows of Y: tau >= the true
    // k-th smallest part, bit for bit the same arithmetic)
    float *snorm = sample + (size_t)ns * d;
    hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)((ns * d + 255) / 256)), dim3(256), 0, s, Y, d, ns,
                       N / ns, sample);
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s, sample, ns, d, snorm);
    brute_tiles<0>(X, nq, d, sample, snorm, ns, vals, nullptr, nullptr, 0, nullptr, 0, N / ns, r, s);
    hipLaunchKernelGGL(brute_select_kernel<0>, dim3((unsigned)nq), dim3(1024), (size_t)TK_BR_SORT * 8, s,
                       vals, ns, nullptr, 0, nullptr, k, tau, nullptr, nullptr, nullptr);
    return 0;
}

// cand (nq * cap) u64, count (nq) int, overflow (1) int are the caller's; out (nq, k) int64.
// cap <= TK_BR_SORT, 2k <= cap, seg a multiple of 32.
int tk_launch_brute_select(const float *X, int64_t nq, int d, const float *Y, int64_t N, int k, const float *ynorm2,
                           float *tau, unsigned long long *cand, int cap, int *count, int *overflow, int64_t *out,
                           float *out_dist, int64_t seg, const TkBruteRestrict *r, hipStream_t s)
{
    if (nq == 0) return 0;
    if (d > 128 || cap > TK_BR_SORT || 2 * k > cap || seg < 32 || seg % 32 || brute_attrs()) return -1;
    (void)hipMemsetAsync(count, 0, (size_t)nq * 4, s);
    (void)hipMemsetAsync(overflow, 0, 4, s);
    for (int64_t s0 = 0; s0 < N; s0 += seg) {
        const int64_t m = N - s0 < seg ? N - s0 : seg;
        brute_tiles<1>(X, nq, d, Y + s0 * d, ynorm2 + s0, m, nullptr, tau, cand, cap, count, s0, 1, r, s);
        hipLaunchKernelGGL(brute_select_kernel<1>, dim3((unsigned)nq), dim3(1024), (size_t)TK_BR_SORT * 8, s,
                           nullptr, 0, cand, cap, count, k, tau, out, overflow, out_dist);
    }
    return 0;
}

// Both halves, unrestricted, with the segment rule above.  Work buffers as the halves take them.
// ns <= TK_BR_SORT, cap <= TK_BR_SORT, k <= ns <= N, 2k <= cap.
int tk_launch_knn_brute(const float *X, int64_t nq, int d, const float *Y, int64_t N, int k,
                        float *ynorm2, float *vals, int64_t ns, float *tau,
                        unsigned long long *cand, int cap, int *count, int *overflow, int64_t *out,
                        float *sample, hipStream_t s)
{
    if (tk_launch_brute_tau(X, nq, d, Y, N, k, ynorm2, vals, ns, tau, sample, nullptr, s)) return -1;
    return tk_launch_brute_select(X, nq, d, Y, N, k, ynorm2, tau, cand, cap, count, overflow, out, nullptr,
                                  tk_brute_segment(k, ns, cap), nullptr, s);
}
