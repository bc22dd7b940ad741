// devbuild.hip — IVF.build for vectors that already live in HBM, and the seeded generator
// of the synthetic 100M x 128 configuration ("per-GPU generation on device
// (seeded per shard), codes produced by the build's encoder"; 8f.1).
//
// What IVF.build does (ivf.py:77-102, build n_probes = 1) without the vectors ever visiting
// the host: nearest centre per row (assign kernels of build.hip), nearest centroid per block
// (encode_pq_kernel), rows grouped by list (stable radix sort of (list, row): a list holds its
// rows in ascending row order, where numpy's unstable argsort leaves the order unspecified),
// 16-row chunks packed into the Quick-ADC byte layout (_transform.py:4-77) directly in the
// tiled order the scan kernels read.  api.hip drives these kernels (tk_index_build_dev).
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>      // radix_sort_pairs of the offline build only (ROCm's own primitives library)

#include "kernels.h"

// ---------------------------------------------------------------------------
// counter-based generator: every value is a pure function of (seed, row, column pair), so a
// data set does not depend on how its rows are split over calls, slabs or ranks
__device__ __forceinline__ uint64_t tk_mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// X[i] = centres[c(row)] + sigma * N(0, 1), c(row) uniform in [0, n_centres) (no centres: the
// noise alone).  One thread per (row, pair of columns): Box-Muller gives two normals.
__global__ void synth_rows_kernel(float *__restrict__ X, int64_t row0, int64_t n, int d, uint64_t seed,
                                  const float *__restrict__ centres, int n_centres, float sigma)
{
    const int hp = (d + 1) >> 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * hp) return;
    const int64_t r = i / hp;
    const int pr = (int)(i - r * hp);
    const uint64_t row = (uint64_t)(row0 + r);
    const uint64_t u = tk_mix64(seed ^ tk_mix64(row * 0x100000001B3ull + (uint64_t)pr));
    const float u1 = ((float)(uint32_t)(u >> 32) + 1.0f) * 2.3283064365386963e-10f;   // (0, 1]
    const float u2 = (float)(uint32_t)u * 2.3283064365386963e-10f;                    // [0, 1)
    const float rad = sqrtf(-2.0f * logf(u1));
    float z0 = rad * cosf(6.283185307179586f * u2), z1 = rad * sinf(6.283185307179586f * u2);
    float b0 = 0.f, b1 = 0.f;
    const int c0 = 2 * pr, c1 = 2 * pr + 1;
    if (centres) {
        const int64_t c = (int64_t)(tk_mix64(seed * 31 + row) % (uint64_t)n_centres);
        b0 = centres[c * d + c0];
        if (c1 < d) b1 = centres[c * d + c1];
    }
    X[r * d + c0] = b0 + sigma * z0;
    if (c1 < d) X[r * d + c1] = b1 + sigma * z1;
}

void tk_launch_synth_rows(float *X, int64_t row0, int64_t n, int d, uint64_t seed, const float *centres,
                          int n_centres, float sigma, hipStream_t s)
{
    // slabs: a launch addresses at most 2^32 - 1 threads (grid x block)
    const int hp = (d + 1) / 2;
    const int64_t slab = (int64_t)1 << 22;
    for (int64_t o = 0; o < n; o += slab) {
        const int64_t m = n - o < slab ? n - o : slab;
        hipLaunchKernelGGL(synth_rows_kernel, dim3((unsigned)((m * hp + 255) / 256)), dim3(256), 0, s,
                           X + o * d, row0 + o, m, d, seed, centres, n_centres, sigma);
    }
}

// ---------------------------------------------------------------------------
// nearest (n, kp) int64 of a slab -> sort keys / values + the per-(centre, column) histogram
// count[centre * kp + j].  Column j of the rows goes to block j of the pair arrays (block stride N):
// group_data_by_indices (utils.py:131-150) appends a list's column-0 members first, then its
// column-1 members, and a stable sort of the pairs by list keeps exactly that order.
__global__ void keys_count_kernel(const int64_t *__restrict__ nearest, int64_t n, int kp, int64_t row0,
                                  int64_t N, int *__restrict__ keys, int *__restrict__ rows,
                                  int *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * kp) return;
    const int64_t r = i / kp;
    const int j = (int)(i - r * kp);
    const int k = (int)nearest[i];
    keys[(int64_t)j * N + row0 + r] = k;
    rows[(int64_t)j * N + row0 + r] = (int)(row0 + r);
    atomicAdd(&count[(int64_t)k * kp + j], 1);
}

void tk_launch_keys_count(const int64_t *nearest, int64_t n, int kp, int64_t row0, int64_t N, int *keys,
                          int *rows, int *count, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(keys_count_kernel, dim3((unsigned)((n * kp + 255) / 256)), dim3(256), 0, s, nearest, n,
                       kp, row0, N, keys, rows, count);
}

// centre id -> active-list id (ivf.py:91: active_centers = all_centers[np.unique(nearest)])
__global__ void remap_keys_kernel(int *__restrict__ keys, int64_t n, const int *__restrict__ remap)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = remap[keys[i]];
}

void tk_launch_remap_keys(int *keys, int64_t n, const int *remap, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(remap_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, n, remap);
}

// stable sort of (list, row) pairs by list; tmp == NULL: size query.  Offline build only (tk_index_build_dev).
int tk_sort_pairs(void *tmp, size_t *tmp_bytes, const int *keys_in, int *keys_out, const int *vals_in,
                  int *vals_out, int64_t n, int bits, hipStream_t s)
{
    size_t bytes = *tmp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u,
                                             (unsigned)bits, s);
    *tmp_bytes = bytes;
    return e == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------
// Exclusive prefix sum in ONE launch (the per-batch sums of a list-sharded rank: segment positions, pair offsets).
// Single pass with decoupled look-back: workgroups take tiles in ticket order (so every predecessor of a tile is
// already running: the waits below always end), a tile publishes its AGGREGATE as soon as it is reduced and its
// inclusive PREFIX once it knows what lies in front; a tile finds that by walking back 64 tiles at a time with
// wave 0 — the first tile with a prefix ends the walk, the aggregates on the way are added.  State of a tile =
// one 64-bit word (flag in the top two bits, value below: a single relaxed atomic publishes both).
//   tmp layout: [0] ticket (unsigned), [8 ...) one uint64 per tile; zeroed by a memset in front of the kernel.
#define TK_SCAN_THREADS 256
#define TK_SCAN_ITEMS 8
#define TK_SCAN_TILE (TK_SCAN_THREADS * TK_SCAN_ITEMS)
#define TK_SCAN_AGG (1ull << 62)
#define TK_SCAN_PFX (2ull << 62)
#define TK_SCAN_VAL ((1ull << 62) - 1ull)

template <typename T>
__global__ __launch_bounds__(TK_SCAN_THREADS) void scan_exclusive_kernel(const T *__restrict__ in, T *__restrict__ out,
                                                                         int64_t n, unsigned *ticket,
                                                                         unsigned long long *state)
{
    __shared__ unsigned tile_s;
    __shared__ long long wave_sum[TK_SCAN_THREADS / 64];
    __shared__ long long excl_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) tile_s = atomicAdd(ticket, 1u);
    __syncthreads();
    const int64_t tile = tile_s;
    const int64_t base = tile * TK_SCAN_TILE + (int64_t)tid * TK_SCAN_ITEMS;
    long long v[TK_SCAN_ITEMS];
    long long mine = 0;
#pragma unroll
    for (int i = 0; i < TK_SCAN_ITEMS; i++) {
        v[i] = base + i < n ? (long long)in[base + i] : 0;
        mine += v[i];
    }
    // inclusive scan of the threads' sums inside the wave
    long long inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    long long wave_off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < TK_SCAN_THREADS / 64; w++) {
        wave_off += w < wave ? wave_sum[w] : 0;
        total += wave_sum[w];
    }
    if (wave == 0) {
        long long excl = 0;
        if (tile == 0) {
            if (lane == 0) __hip_atomic_store(&state[0], TK_SCAN_PFX | ((unsigned long long)total & TK_SCAN_VAL),
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(&state[tile], TK_SCAN_AGG | ((unsigned long long)total & TK_SCAN_VAL),
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int64_t j = tile - 1;; j -= 64) {
                const int64_t idx = j - lane;
                unsigned long long st = TK_SCAN_PFX;                    // (in front of tile 0: a prefix of zero)
                if (idx >= 0) {
                    do {
                        st = __hip_atomic_load(&state[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } while ((st >> 62) == 0);
                }
                const unsigned long long has_pfx = __ballot((st >> 62) == 2);
                const int first = has_pfx ? __builtin_ctzll(has_pfx) : 64;
                // sign-extend the 62-bit value (sums of non-negative counts here, but keep the arithmetic exact)
                long long val = (long long)((st & TK_SCAN_VAL) << 2) >> 2;
                val = lane <= first ? val : 0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) val += __shfl_xor(val, o, 64);
                excl += val;
                if (has_pfx) break;
            }
            if (lane == 0) __hip_atomic_store(&state[tile],
                                              TK_SCAN_PFX | ((unsigned long long)(excl + total) & TK_SCAN_VAL),
                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) excl_s = excl;
    }
    __syncthreads();
    long long run = excl_s + wave_off + (inc - mine);
#pragma unroll
    for (int i = 0; i < TK_SCAN_ITEMS; i++) {
        if (base + i < n) out[base + i] = (T)run;
        run += v[i];
    }
}

static size_t scan_tmp_bytes(int64_t n)
{
    const int64_t tiles = (n + TK_SCAN_TILE - 1) / TK_SCAN_TILE;
    return 8 + (size_t)(tiles > 0 ? tiles : 1) * 8;
}

template <typename T>
static int scan_exclusive_impl(void *tmp, size_t *tmp_bytes, const T *in, T *out, int64_t n, hipStream_t s)
{
    const size_t need = scan_tmp_bytes(n);
    if (!tmp) {
        *tmp_bytes = need;
        return 0;
    }
    if (*tmp_bytes < need) return -1;
    if (n <= 0) return 0;
    if (hipMemsetAsync(tmp, 0, need, s) != hipSuccess) return -1;
    const int64_t tiles = (n + TK_SCAN_TILE - 1) / TK_SCAN_TILE;
    hipLaunchKernelGGL(scan_exclusive_kernel<T>, dim3((unsigned)tiles), dim3(TK_SCAN_THREADS), 0, s, in, out, n,
                       (unsigned *)tmp, (unsigned long long *)((char *)tmp + 8));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// exclusive prefix sum of n ints; tmp == NULL: size query.  in == out is allowed (a thread reads its items before
// any thread of the grid writes them: tiles do not overlap).
int tk_scan_exclusive(void *tmp, size_t *tmp_bytes, const int *in, int *out, int64_t n, hipStream_t s)
{
    return scan_exclusive_impl<int>(tmp, tmp_bytes, in, out, n, s);
}

int tk_scan_exclusive64(void *tmp, size_t *tmp_bytes, const long long *in, long long *out, int64_t n,
                        hipStream_t s)
{
    return scan_exclusive_impl<long long>(tmp, tmp_bytes, in, out, n, s);
}

__global__ void widen_ids_kernel(const int *__restrict__ rows, int64_t n, int64_t *__restrict__ ids)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = rows[i];
}

void tk_launch_widen_ids(const int *rows, int64_t n, int64_t *ids, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(widen_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, n, ids);
}

// ---------------------------------------------------------------------------
// labels (rows, M) uint8 -> tiled Quick-ADC chunks of all lists.  One thread per (global chunk
// c, block pair p): byte r of its 16-byte group = code[row_r][2p] | code[row_r][2p+1] << 4,
// row_r = the r-th row of the chunk in list order (rows_sorted; NULL: rows are already in list
// order); rows past the list's end carry the zero vector's code (pad2 + transform,
// fast_pq.py:165).
__global__ void pack_lists_kernel(const uint8_t *__restrict__ labels, int M,
                                  const int *__restrict__ rows_sorted,
                                  const int64_t *__restrict__ ids_off,
                                  const int64_t *__restrict__ chunk_off,
                                  const int64_t *__restrict__ list_n, int n_lists,
                                  const uint8_t *__restrict__ zero_code, uint4 *__restrict__ tiled,
                                  int64_t total_chunks)
{
    const int P = M >> 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_chunks * P) return;
    const int64_t c = i / P;
    const int p = (int)(i - c * P);
    int lo = 0, hi = n_lists;   // chunk_off[lo] <= c < chunk_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t j = c - chunk_off[lo];
    const int64_t base = ids_off[lo] + 16 * j;
    const int64_t left = list_n[lo] - 16 * j;
    const uint32_t zb = (uint32_t)zero_code[2 * p] | ((uint32_t)zero_code[2 * p + 1] << 4);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 16; r++) {
        uint32_t b = zb;
        if (r < left) {
            const int64_t row = rows_sorted ? (int64_t)rows_sorted[base + r] : base + r;
            const uint8_t *lab = labels + row * M + 2 * p;
            b = (uint32_t)lab[0] | ((uint32_t)lab[1] << 4);
        }
        w[r >> 2] |= b << (8 * (r & 3));
    }
    tiled[((c >> 3) * P + p) * 8 + (c & 7)] = make_uint4(w[0], w[1], w[2], w[3]);
}

void tk_launch_pack_lists(const uint8_t *labels, int M, const int *rows_sorted, const int64_t *ids_off,
                          const int64_t *chunk_off, const int64_t *list_n, int n_lists,
                          const uint8_t *zero_code, uint4 *tiled, int64_t total_chunks, hipStream_t s)
{
    const int64_t items = total_chunks * (M / 2);
    if (items <= 0) return;
    hipLaunchKernelGGL(pack_lists_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, labels, M,
                       rows_sorted, ids_off, chunk_off, list_n, n_lists, zero_code, tiled, total_chunks);
}

// New rows merged into built lists (tk_index_add_rows): list l's column-j block becomes old_j ++ new_j.
// seg[(l * kp + j) * 2 + {0, 1}] = (old, new) members of that block; the old ones sit at list positions
// sum_{j' < j} old_j' of the old layout (old_chunk_off / old_ids_off; lists past the old ones have none),
// the new ones at sorted-pair positions new_off[l] + sum_{j' < j} new_j' (rows_sorted: new row numbers,
// grouped by list, column blocks in order, rows ascending — tk_sort_pairs' output).  One thread per
// (output chunk, block pair), as pack_lists_kernel: output row r of the chunk finds its segment and
// copies the packed byte of its old position, or packs labels_new[row][2p .. 2p + 1]; nothing old is
// decoded or re-encoded.  The p == 0 thread of a chunk also writes the chunk's ids (old labels, or
// n_old + new row) and their int32 copy (ids32 may be NULL).
__global__ void merge_lists_kernel(const uint4 *__restrict__ old_tiled, const int64_t *__restrict__ old_chunk_off,
                                   const int64_t *__restrict__ old_ids_off, const int64_t *__restrict__ old_ids,
                                   const uint8_t *__restrict__ labels_new, int M, const int *__restrict__ rows_sorted,
                                   const int64_t *__restrict__ new_off, const int64_t *__restrict__ seg, int kp,
                                   const int64_t *__restrict__ chunk_off, const int64_t *__restrict__ ids_off,
                                   const int64_t *__restrict__ list_n, int n_lists, const uint8_t *__restrict__ zero_code,
                                   int64_t n_old, uint4 *__restrict__ tiled, int64_t *__restrict__ ids,
                                   int32_t *__restrict__ ids32, int64_t total_chunks)
{
    const int P = M >> 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_chunks * P) return;
    const int64_t c = i / P;
    const int p = (int)(i - c * P);
    int lo = 0, hi = n_lists;   // chunk_off[lo] <= c < chunk_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t pos0 = 16 * (c - chunk_off[lo]);
    const int64_t n_l = list_n[lo];
    const int64_t *sg = seg + (int64_t)lo * kp * 2;
    const uint32_t zb = (uint32_t)zero_code[2 * p] | ((uint32_t)zero_code[2 * p + 1] << 4);
    uint32_t w[4] = {0, 0, 0, 0};
    int64_t cur_oc = -1;                  // the old chunk held in `cur` (consecutive rows mostly share one)
    uint4 cur = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        uint32_t b = zb;
        const int64_t pos = pos0 + r;
        if (pos < n_l) {
            int64_t q = pos, obase = 0, nbase = new_off[lo];
            int64_t old_pos = -1, new_at = -1;
            for (int t = 0; t < kp; t++) {
                const int64_t o = sg[2 * t], nn = sg[2 * t + 1];
                if (q < o) { old_pos = obase + q; break; }
                q -= o;
                if (q < nn) { new_at = nbase + q; break; }
                q -= nn;
                obase += o;
                nbase += nn;
            }
            int64_t label = -1;
            if (old_pos >= 0) {
                const int64_t oc = old_chunk_off[lo] + (old_pos >> 4);
                if (oc != cur_oc) {
                    cur = old_tiled[((oc >> 3) * P + p) * 8 + (oc & 7)];
                    cur_oc = oc;
                }
                const int rr = (int)(old_pos & 15);
                const uint32_t word = rr < 4 ? cur.x : (rr < 8 ? cur.y : (rr < 12 ? cur.z : cur.w));
                b = (word >> (8 * (rr & 3))) & 0xffu;
                if (p == 0) label = old_ids[old_ids_off[lo] + old_pos];
            } else if (new_at >= 0) {
                const int64_t row = rows_sorted[new_at];
                const uint8_t *lab = labels_new + row * M + 2 * p;
                b = (uint32_t)lab[0] | ((uint32_t)lab[1] << 4);
                if (p == 0) label = n_old + row;
            }
            if (p == 0) {
                ids[ids_off[lo] + pos] = label;
                if (ids32) ids32[ids_off[lo] + pos] = (int32_t)label;
            }
        }
        w[r >> 2] |= b << (8 * (r & 3));
    }
    tiled[((c >> 3) * P + p) * 8 + (c & 7)] = make_uint4(w[0], w[1], w[2], w[3]);
}

void tk_launch_merge_lists(const uint4 *old_tiled, const int64_t *old_chunk_off, const int64_t *old_ids_off,
                           const int64_t *old_ids, const uint8_t *labels_new, int M, const int *rows_sorted,
                           const int64_t *new_off, const int64_t *seg, int kp, const int64_t *chunk_off,
                           const int64_t *ids_off, const int64_t *list_n, int n_lists, const uint8_t *zero_code,
                           int64_t n_old, uint4 *tiled, int64_t *ids, int32_t *ids32, int64_t total_chunks,
                           hipStream_t s)
{
    const int64_t items = total_chunks * (M / 2);
    if (items <= 0) return;
    hipLaunchKernelGGL(merge_lists_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, old_tiled,
                       old_chunk_off, old_ids_off, old_ids, labels_new, M, rows_sorted, new_off, seg, kp, chunk_off,
                       ids_off, list_n, n_lists, zero_code, n_old, tiled, ids, ids32, total_chunks);
}

// ---------------------------------------------------------------------------
// Rows removed from built lists (tk_index_remove_rows).  The rows (checked in [0, N) on the host) become a byte
// map over the row ids; every stored entry is flagged keep / drop; the exclusive scan of the flags gives a kept
// entry its new position (lists and entries keep their order), src[] maps it back; compact_lists_kernel writes the
// new tiled array.  Nothing is decoded or re-encoded.
__global__ void mark_rows_kernel(const int64_t *__restrict__ rows, int64_t n, uint8_t *__restrict__ dead)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dead[rows[i]] = 1;     // (duplicates write the same byte)
}

// keep[i] = 1 for a stored entry whose row stays, 0 for one removed; keep[T] = 0, so that the exclusive scan's
// element T is the number kept.  A label outside [0, N) sets *bad (no row id can name it).
__global__ void keep_flags_kernel(const int64_t *__restrict__ ids, int64_t T, const uint8_t *__restrict__ dead,
                                  int64_t N, long long *__restrict__ keep, int *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > T) return;
    long long k = 0;
    if (i < T) {
        const int64_t id = ids[i];
        if (id >= 0 && id < N) k = dead[id] ? 0 : 1;
        else { k = 1; *bad = 1; }
    }
    keep[i] = k;
}

void tk_launch_mark_rows(const int64_t *rows, int64_t n, uint8_t *dead, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(mark_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, n, dead);
}

void tk_launch_keep_flags(const int64_t *ids, int64_t T, const uint8_t *dead, int64_t N, long long *keep, int *bad,
                          hipStream_t s)
{
    hipLaunchKernelGGL(keep_flags_kernel, dim3((unsigned)((T + 1 + 255) / 256)), dim3(256), 0, s, ids, T, dead, N,
                       keep, bad);
}

// src[scan[i]] = i for every kept entry: the old position of every new one
__global__ void scatter_kept_kernel(const long long *__restrict__ keep, const long long *__restrict__ scan, int64_t T,
                                    int *__restrict__ src)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T && keep[i]) src[scan[i]] = (int)i;
}

// out[j] = scan[pos[j]]: the new positions of the (list, column) boundaries
__global__ void gather_scan_kernel(const long long *__restrict__ scan, const int64_t *__restrict__ pos, int64_t m,
                                   int64_t *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) out[j] = scan[pos[j]];
}

void tk_launch_scatter_kept(const long long *keep, const long long *scan, int64_t T, int *src, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(scatter_kept_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, keep, scan, T, src);
}

void tk_launch_gather_scan(const long long *scan, const int64_t *pos, int64_t m, int64_t *out, hipStream_t s)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(gather_scan_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, scan, pos, m, out);
}

// The compacted lists: one thread per (output chunk, block pair), as merge_lists_kernel.  Output row r of the chunk
// (list position pos, global position g) copies the packed byte of its old position src[g] (in the same list: the
// scan keeps list boundaries); rows past the list's end take the zero vector's code.  The p == 0 thread of a chunk
// also writes the chunk's ids and their int32 copy (ids32 may be NULL).
__global__ void compact_lists_kernel(const uint4 *__restrict__ old_tiled, const int64_t *__restrict__ old_chunk_off,
                                     const int64_t *__restrict__ old_ids_off, const int64_t *__restrict__ old_ids,
                                     const int *__restrict__ src, int M, const int64_t *__restrict__ chunk_off,
                                     const int64_t *__restrict__ ids_off, const int64_t *__restrict__ list_n,
                                     int n_lists, const uint8_t *__restrict__ zero_code, uint4 *__restrict__ tiled,
                                     int64_t *__restrict__ ids, int32_t *__restrict__ ids32, int64_t total_chunks)
{
    const int P = M >> 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_chunks * P) return;
    const int64_t c = i / P;
    const int p = (int)(i - c * P);
    int lo = 0, hi = n_lists;   // chunk_off[lo] <= c < chunk_off[lo + 1] (empty lists are stepped over)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t pos0 = 16 * (c - chunk_off[lo]);
    const int64_t n_l = list_n[lo], g0 = ids_off[lo], og0 = old_ids_off[lo], oc0 = old_chunk_off[lo];
    const uint32_t zb = (uint32_t)zero_code[2 * p] | ((uint32_t)zero_code[2 * p + 1] << 4);
    uint32_t w[4] = {0, 0, 0, 0};
    int64_t cur_oc = -1;                  // the old chunk held in `cur` (consecutive rows mostly share one)
    uint4 cur = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        uint32_t b = zb;
        const int64_t pos = pos0 + r;
        if (pos < n_l) {
            const int64_t og = src[g0 + pos];
            const int64_t old_pos = og - og0;
            const int64_t oc = oc0 + (old_pos >> 4);
            if (oc != cur_oc) {
                cur = old_tiled[((oc >> 3) * P + p) * 8 + (oc & 7)];
                cur_oc = oc;
            }
            const int rr = (int)(old_pos & 15);
            const uint32_t word = rr < 4 ? cur.x : (rr < 8 ? cur.y : (rr < 12 ? cur.z : cur.w));
            b = (word >> (8 * (rr & 3))) & 0xffu;
            if (p == 0) {
                const int64_t label = old_ids[og];
                ids[g0 + pos] = label;
                if (ids32) ids32[g0 + pos] = (int32_t)label;
            }
        }
        w[r >> 2] |= b << (8 * (r & 3));
    }
    tiled[((c >> 3) * P + p) * 8 + (c & 7)] = make_uint4(w[0], w[1], w[2], w[3]);
}

void tk_launch_compact_lists(const uint4 *old_tiled, const int64_t *old_chunk_off, const int64_t *old_ids_off,
                             const int64_t *old_ids, const int *src, int M, const int64_t *chunk_off,
                             const int64_t *ids_off, const int64_t *list_n, int n_lists, const uint8_t *zero_code,
                             uint4 *tiled, int64_t *ids, int32_t *ids32, int64_t total_chunks, hipStream_t s)
{
    const int64_t items = total_chunks * (M / 2);
    if (items <= 0) return;
    hipLaunchKernelGGL(compact_lists_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, old_tiled,
                       old_chunk_off, old_ids_off, old_ids, src, M, chunk_off, ids_off, list_n, n_lists, zero_code,
                       tiled, ids, ids32, total_chunks);
}

// Stored rows replaced in built lists (tk_index_update_rows): the removal's compaction and the addition's merge in
// one pass.  List l's column-j block becomes (old_j minus the replaced rows, old order kept) ++ new_j.
// seg[(l * kp + j) * 2 + {0, 1}] = (kept, new) members of that block.  The kept ones are numbered as the removal
// numbers them — kept entry kept_off[l] + sum_{j' < j} kept_j' + q of the compacted order, whose old global position
// is src[] (scatter_kept's output; in the same list: the scan keeps list boundaries) — the new ones sit at
// sorted-pair positions new_off[l] + sum_{j' < j} new_j' (rows_sorted, as merge_lists_kernel reads it).  One thread
// per (output chunk, block pair): a kept member copies the packed byte and the label of its old position, a new
// member packs labels_new[row][2p .. 2p + 1] and takes the label new_ids[row]; nothing old is decoded or re-encoded,
// padding rows take the zero vector's code.  Removed entries leave gaps between the old positions of consecutive
// kept members: the old chunk held in `cur` is named by cur_oc and fetched again only when the position leaves it, so
// a chunk is read once per thread however many of its rows went (as in compact_lists_kernel).  Lists past the old
// ones (l >= n_old_lists) have no kept member and read nothing old.  The p == 0 thread writes ids and ids32.
__global__ void replace_lists_kernel(const uint4 *__restrict__ old_tiled, const int64_t *__restrict__ old_chunk_off,
                                     const int64_t *__restrict__ old_ids_off, const int64_t *__restrict__ old_ids,
                                     int n_old_lists, const int *__restrict__ src, const int64_t *__restrict__ kept_off,
                                     const uint8_t *__restrict__ labels_new, int M, const int *__restrict__ rows_sorted,
                                     const int64_t *__restrict__ new_ids, const int64_t *__restrict__ new_off,
                                     const int64_t *__restrict__ seg, int kp, const int64_t *__restrict__ chunk_off,
                                     const int64_t *__restrict__ ids_off, const int64_t *__restrict__ list_n,
                                     int n_lists, const uint8_t *__restrict__ zero_code, uint4 *__restrict__ tiled,
                                     int64_t *__restrict__ ids, int32_t *__restrict__ ids32, int64_t total_chunks)
{
    const int P = M >> 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total_chunks * P) return;
    const int64_t c = i / P;
    const int p = (int)(i - c * P);
    int lo = 0, hi = n_lists;   // chunk_off[lo] <= c < chunk_off[lo + 1] (empty lists are stepped over)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_off[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t pos0 = 16 * (c - chunk_off[lo]);
    const int64_t n_l = list_n[lo], g0 = ids_off[lo];
    const bool had = lo < n_old_lists;
    const int64_t og0 = had ? old_ids_off[lo] : 0, oc0 = had ? old_chunk_off[lo] : 0, k0 = had ? kept_off[lo] : 0;
    const int64_t *sg = seg + (int64_t)lo * kp * 2;
    const uint32_t zb = (uint32_t)zero_code[2 * p] | ((uint32_t)zero_code[2 * p + 1] << 4);
    uint32_t w[4] = {0, 0, 0, 0};
    int64_t cur_oc = -1;                  // the old chunk held in `cur` (kept neighbours mostly share one, gaps or not)
    uint4 cur = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        uint32_t b = zb;
        const int64_t pos = pos0 + r;
        if (pos < n_l) {
            int64_t q = pos, kbase = k0, nbase = new_off[lo];
            int64_t kept_at = -1, new_at = -1;
            for (int t = 0; t < kp; t++) {
                const int64_t o = sg[2 * t], nn = sg[2 * t + 1];
                if (q < o) { kept_at = kbase + q; break; }
                q -= o;
                if (q < nn) { new_at = nbase + q; break; }
                q -= nn;
                kbase += o;
                nbase += nn;
            }
            int64_t label = -1;
            if (kept_at >= 0 && had) {
                const int64_t og = src[kept_at];
                const int64_t old_pos = og - og0;
                const int64_t oc = oc0 + (old_pos >> 4);
                if (oc != cur_oc) {
                    cur = old_tiled[((oc >> 3) * P + p) * 8 + (oc & 7)];
                    cur_oc = oc;
                }
                const int rr = (int)(old_pos & 15);
                const uint32_t word = rr < 4 ? cur.x : (rr < 8 ? cur.y : (rr < 12 ? cur.z : cur.w));
                b = (word >> (8 * (rr & 3))) & 0xffu;
                if (p == 0) label = old_ids[og];
            } else if (new_at >= 0) {
                const int64_t row = rows_sorted[new_at];
                const uint8_t *lab = labels_new + row * M + 2 * p;
                b = (uint32_t)lab[0] | ((uint32_t)lab[1] << 4);
                if (p == 0) label = new_ids[row];
            }
            if (p == 0) {
                ids[g0 + pos] = label;
                if (ids32) ids32[g0 + pos] = (int32_t)label;
            }
        }
        w[r >> 2] |= b << (8 * (r & 3));
    }
    tiled[((c >> 3) * P + p) * 8 + (c & 7)] = make_uint4(w[0], w[1], w[2], w[3]);
}

void tk_launch_replace_lists(const uint4 *old_tiled, const int64_t *old_chunk_off, const int64_t *old_ids_off,
                             const int64_t *old_ids, int n_old_lists, const int *src, const int64_t *kept_off,
                             const uint8_t *labels_new, int M, const int *rows_sorted, const int64_t *new_ids,
                             const int64_t *new_off, const int64_t *seg, int kp, const int64_t *chunk_off,
                             const int64_t *ids_off, const int64_t *list_n, int n_lists, const uint8_t *zero_code,
                             uint4 *tiled, int64_t *ids, int32_t *ids32, int64_t total_chunks, hipStream_t s)
{
    const int64_t items = total_chunks * (M / 2);
    if (items <= 0) return;
    hipLaunchKernelGGL(replace_lists_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, old_tiled,
                       old_chunk_off, old_ids_off, old_ids, n_old_lists, src, kept_off, labels_new, M, rows_sorted,
                       new_ids, new_off, seg, kp, chunk_off, ids_off, list_n, n_lists, zero_code, tiled, ids, ids32,
                       total_chunks);
}

// The replaced rows' vectors: staged row i (prepared, row-major (n, d)) goes to row new_ids[i] of the store.  One
// thread per element, consecutive threads along d (a wave writes one row's consecutive elements, or the ends of two);
// the ids are distinct (checked by the caller), so no two staged rows meet.  TX -> TY: float -> float and
// double -> double copy; float -> _Float16 is narrow_rows_kernel's conversion (round-to-nearest-even, subnormals kept).
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void scatter_rows_kernel(const TX *__restrict__ X, int64_t n, int d,
                                                           const int64_t *__restrict__ new_ids, TY *__restrict__ data)
{
    const int64_t total = n * d, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / d;
        data[new_ids[r] * d + (i - r * d)] = (TY)X[i];
    }
}

void tk_launch_scatter_rows(const void *X, int64_t n, int d, const int64_t *new_ids, void *data, int data_dtype,
                            hipStream_t s)
{
    if (n <= 0) return;
    const int64_t total = n * d;
    const dim3 grid((unsigned)(total / 256 + 1 < 8192 ? total / 256 + 1 : 8192)), block(256);
    if (data_dtype == 2)
        hipLaunchKernelGGL((scatter_rows_kernel<float, _Float16>), grid, block, 0, s, (const float *)X, n, d, new_ids,
                           (_Float16 *)data);
    else if (data_dtype == 1)
        hipLaunchKernelGGL((scatter_rows_kernel<double, double>), grid, block, 0, s, (const double *)X, n, d, new_ids,
                           (double *)data);
    else
        hipLaunchKernelGGL((scatter_rows_kernel<float, float>), grid, block, 0, s, (const float *)X, n, d, new_ids,
                           (float *)data);
}

// Copies per row of the stored labels: cnt[row] += 1 per entry (cnt: N ints, zeroed); a label outside [0, N) is
// counted in *outside instead.
__global__ void row_copies_kernel(const int64_t *__restrict__ ids, int64_t T, int64_t N, int *__restrict__ cnt,
                                  int *__restrict__ outside)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const int64_t id = ids[i];
    if (id >= 0 && id < N) atomicAdd(&cnt[id], 1);
    else atomicAdd(outside, 1);
}

// out[0] = the largest row with a copy (-1: none), out[1] = the most copies of a row, out[2] = the fewest copies of
// a stored row (out[0 .. 2]: {-1, 0, INT_MAX} on entry).  One atomic per wave.
__global__ void copies_summary_kernel(const int *__restrict__ cnt, int64_t N, int *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = i < N ? cnt[i] : 0;
    int hi_row = c > 0 ? (int)i : -1, most = c, fewest = c > 0 ? c : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        hi_row = max(hi_row, __shfl_xor(hi_row, o, 64));
        most = max(most, __shfl_xor(most, o, 64));
        fewest = min(fewest, __shfl_xor(fewest, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (hi_row >= 0) atomicMax(&out[0], hi_row);
        if (most > 0) atomicMax(&out[1], most);
        if (fewest != 0x7fffffff) atomicMin(&out[2], fewest);
    }
}

void tk_launch_row_copies(const int64_t *ids, int64_t T, int *cnt, int64_t N, int *out, hipStream_t s)
{
    if (T > 0)
        hipLaunchKernelGGL(row_copies_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, ids, T, N, cnt,
                           out + 3);
    if (N > 0)
        hipLaunchKernelGGL(copies_summary_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, cnt, N, out);
}

// rows of an (N, d) matrix gathered by id as float32 (rescoring vectors for the checker, stored rows as queries):
// float32 vectors, vectors stored as IEEE half, widened (exact), or float64 vectors rounded to nearest even
template <typename TY>
__global__ void gather_rows_kernel(const TY *__restrict__ X, int d, const int64_t *__restrict__ rows, int64_t n,
                                   float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * d) return;
    const int64_t r = i / d;
    out[i] = (float)X[rows[r] * d + (i - r * d)];
}

void tk_launch_gather_rows(const void *X, int data_dtype, int d, const int64_t *rows, int64_t n, float *out,
                           hipStream_t s)
{
    // slabs of fewer than 2^31 elements: the block count of a launch is cast to 32 bits and must fit them
    const int64_t slab = (((int64_t)1 << 31) - 256) / d;
    for (int64_t o = 0; o < n; o += slab) {
        const int64_t m = n - o < slab ? n - o : slab;
        const dim3 grid((unsigned)((m * d + 255) / 256)), block(256);
        const int64_t *r = rows + o;
        float *to = out + o * d;
        if (data_dtype == 2)
            hipLaunchKernelGGL(gather_rows_kernel<_Float16>, grid, block, 0, s, (const _Float16 *)X, d, r, m, to);
        else if (data_dtype == 1)       // (double -> float: round to nearest even, numpy's astype)
            hipLaunchKernelGGL(gather_rows_kernel<double>, grid, block, 0, s, (const double *)X, d, r, m, to);
        else
            hipLaunchKernelGGL(gather_rows_kernel<float>, grid, block, 0, s, (const float *)X, d, r, m, to);
    }
}

// Half storage of float32 rows.  The check pass: *first_bad (set to INT64_MAX by the caller) = the first row
// holding a value whose half is not finite — |x| >= 65520 rounds to infinity under round-to-nearest-even
// (65504 is the largest half, 65520 the tie above it, which goes to the even side: infinity), and so do inf
// and NaN fail `|x| < 65520`.
__global__ __launch_bounds__(256) void check_half_kernel(const float *__restrict__ X, int64_t n, int d,
                                                         unsigned long long *__restrict__ first_bad)
{
    const int64_t total = n * d, stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long bad = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride)
        if (!(__builtin_fabsf(X[i]) < 65520.0f)) {
            const unsigned long long r = (unsigned long long)(i / d);
            if (r < bad) bad = r;
        }
    if (bad != ~0ull) atomicMin(first_bad, bad);
}

void tk_launch_check_half(const float *X, int64_t n, int d, unsigned long long *first_bad, hipStream_t s)
{
    if (n <= 0) return;
    const int64_t total = n * d;
    const unsigned blocks = (unsigned)(total / 256 + 1 < 4096 ? total / 256 + 1 : 4096);
    hipLaunchKernelGGL(check_half_kernel, dim3(blocks), dim3(256), 0, s, X, n, d, first_bad);
}

// The conversion: round-to-nearest-even, subnormal halves kept (the hardware's v_cvt_f16_f32 in its default
// mode: what numpy's astype(float16) gives for every value that passed the check).
__global__ __launch_bounds__(256) void narrow_rows_kernel(const float *__restrict__ X, int64_t total,
                                                          _Float16 *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) out[i] = (_Float16)X[i];
}

void tk_launch_narrow_rows(const float *X, int64_t n, int d, void *out, hipStream_t s)
{
    if (n <= 0) return;
    const int64_t total = n * d;
    const unsigned blocks = (unsigned)(total / 256 + 1 < 8192 ? total / 256 + 1 : 8192);
    hipLaunchKernelGGL(narrow_rows_kernel, dim3(blocks), dim3(256), 0, s, X, total, (_Float16 *)out);
}

// chunks of the lists a rank owns, copied from the whole index's tiled code array into the
// rank's own (compact) tiled array: local chunk cl of list l = global chunk coff[l] + cl - loff[l]
__global__ void compact_tiled_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int P,
                                     const int64_t *__restrict__ global_off,
                                     const int64_t *__restrict__ local_off, int n_lists,
                                     int64_t local_chunks)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= local_chunks * P) return;
    const int64_t cl = i / P;
    const int p = (int)(i - cl * P);
    int lo = 0, hi = n_lists;   // local_off[lo] <= cl < local_off[hi]; empty (foreign) lists are skipped
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (local_off[mid] <= cl) lo = mid; else hi = mid;
    }
    const int64_t cg = global_off[lo] + (cl - local_off[lo]);
    dst[((cl >> 3) * P + p) * 8 + (cl & 7)] = src[((cg >> 3) * P + p) * 8 + (cg & 7)];
}

void tk_launch_compact_tiled(const uint4 *src, uint4 *dst, int P, const int64_t *global_off,
                             const int64_t *local_off, int n_lists, int64_t local_chunks, hipStream_t s)
{
    const int64_t items = local_chunks * P;
    if (items <= 0) return;
    hipLaunchKernelGGL(compact_tiled_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, src, dst,
                       P, global_off, local_off, n_lists, local_chunks);
}

// ---------------------------------------------------------------------------
// measurement plumbing: a kernel that only READS `n` uint4 (every byte once, 16 B per lane and
// load, a wave 1 KiB contiguous — the access pattern of the flat scan), for the streaming-read
// ceiling bench.py prints beside the HBM-scale scan leg
__global__ __launch_bounds__(256) void read_only_kernel(const uint4 *__restrict__ src, int64_t n,
                                                        uint32_t *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint32_t acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint4 v = src[i];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x12345678u) out[0] = acc;      // never true for the test pattern: keeps the loads
}

void tk_launch_read_only(const void *src, int64_t n_uint4, uint32_t *out, hipStream_t s)
{
    hipLaunchKernelGGL(read_only_kernel, dim3(65536), dim3(256), 0, s, (const uint4 *)src, n_uint4, out);
}

// ... and one that reads `n_gather` ROWS of `row16` 16-byte pieces each, chosen at random among n_rows (a hash
// of the gather index), the way the rescoring kernel reads its candidates: consecutive lanes = consecutive
// pieces of a row, a wave's load instruction covers 64 / lanes_per_row whole rows, 16 loads in flight per lane.
// The ceiling of `roofline.rescore` (MI355X_MICROARCH.md quotes 5.5-5.6 TB/s for 1 152-byte rows; GloVe's are 400).
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4 *__restrict__ src, int64_t n_rows, int row16,
                                                          int lpr_log, int64_t n_gather, uint32_t *__restrict__ out)
{
    const int lpr = 1 << lpr_log;
    const int64_t lane_rows = ((int64_t)gridDim.x * blockDim.x) >> lpr_log;       // rows in flight per load round
    const int64_t g0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> lpr_log;
    const int pc = threadIdx.x & (lpr - 1);
    uint32_t acc = 0;
    for (int64_t g = g0; g < n_gather; g += 16 * lane_rows) {
        uint4 v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const uint64_t gi = (uint64_t)(g + u * lane_rows);
            uint64_t h = gi * 0x9E3779B97F4A7C15ull;
            h ^= h >> 29;
            h *= 0xBF58476D1CE4E5B9ull;
            h ^= h >> 32;
            const int64_t row = (int64_t)(h % (uint64_t)n_rows);
            v[u] = (pc < row16 && gi < (uint64_t)n_gather) ? src[row * row16 + pc] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 16; u++) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    }
    if (acc == 0x12345678u) out[0] = acc;
}

void tk_launch_gather_rows(const void *src, int64_t n_rows, int row_bytes, int64_t n_gather, uint32_t *out, hipStream_t s)
{
    const int row16 = row_bytes / 16;
    const int lpr_log = row16 <= 16 ? 4 : (row16 <= 32 ? 5 : 6);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(8192), dim3(256), 0, s, (const uint4 *)src, n_rows, row16, lpr_log,
                       n_gather, out);
}
