/*
 * tinyknn_hip.h — C ABI of libtinyknn_hip.so, the MI355X (gfx950) implementation
 * of the ONE hot path of thomasahle/tinyknn: the Quick-ADC 4-bit PQ code scan, the
 * bounded order-dependent top-R heap, the per-query distance table and the exact
 * rescoring that sit behind FastPQ / _FastDistanceTable / IVF.query.
 *
 * Every entry point names the reference interface it replaces (file:line relative
 * to the reference repository).  Plain pointers and sizes only; no torch types.
 * Conventions
 *   - return value: 0 = ok, <0 = error; tk_last_error() gives the text
 *     (the reference kernels are void/nogil and cannot fail; its Python layer
 *     raises AssertionError — the Python binding maps error codes to that).
 *   - pointers are HOST pointers unless the parameter name ends in _dev;
 *     buffers are caller-owned, written in place, nothing is retained
 *     (same ownership rule as the Cython memoryview arguments).
 *   - `order`: accumulation order of the saturating int8 sum.
 *     TK_ORDER_SSE = _fast_pq.pyx:209-236 (one accumulator),
 *     TK_ORDER_AVX = _fast_pq_256.pyx:126-156 (two accumulators, merged last);
 *     the reference's public API uses AVX (fast_pq.py:21-24).
 *   - `stream`: a hipStream_t passed as void* (NULL = the default stream).  Device
 *     entry points only enqueue work; host-pointer entry points synchronise.
 * There is no CPU fallback: without a usable GPU every compute call fails.
 */
#ifndef TINYKNN_HIP_H
#define TINYKNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TK_ORDER_SSE 0
#define TK_ORDER_AVX 1

#define TK_OK 0
#define TK_ERR_ARG (-1)     /* bad argument (shape/size contract violated)   */
#define TK_ERR_HIP (-2)     /* HIP runtime error                              */
#define TK_ERR_STATE (-3)   /* index not fully populated for this call        */
#define TK_ERR_WORKSPACE (-4) /* the call's device work memory would exceed the workspace budget: ask fewer queries */

/* ---- library -------------------------------------------------------------- */
const char *tk_last_error(void);
int tk_version(void);
/* number of visible GPUs; 0 when there is none (compute calls then fail) */
int tk_device_count(void);
int tk_set_device(int device);

/* ---- drop-in kernels on host buffers -------------------------------------- */

/* estimate_pq_sse(data, tables, out, signd)  _fast_pq.pyx:101-111
 * estimate_pq_avx(...)                       _fast_pq_256.pyx:52-62
 * data: uint64 (chunks, M) Quick-ADC layout (_transform.py:4-77); tables: uint64
 * (2M,) (_transform.py:114-138); out: uint64 (>= 2*chunks,), 16 int8/uint8 per chunk. */
int tk_estimate_pq(const uint64_t *data, int64_t chunks, int M, const uint64_t *tables,
                   uint64_t *out, int signd, int order);

/* Batched form of the same call: nq tables (nq, 2M) against one code array,
 * out (nq, 2*chunks).  What examples/example.py:60-66 does in a Python loop. */
int tk_estimate_pq_batch(const uint64_t *data, int64_t chunks, int M,
                         const uint64_t *tables, int64_t nq, uint64_t *out, int signd,
                         int order);

/* query_pq_sse(data, n, tables, indices, vals, signd, labels=None)  _fast_pq.pyx:114-206
 * query_pq_avx(...)                                                 _fast_pq_256.pyx:65-123
 * indices int64 (R,), vals int32 (R,) are read AND written (one heap is threaded
 * through several calls, ivf.py:137-150).  labels: int64 (>= n,) or NULL. */
int tk_query_pq(const uint64_t *data, int64_t chunks, int M, int64_t n,
                const uint64_t *tables, int64_t *indices, int32_t *vals, int R, int signd,
                const int64_t *labels, int order);

/* init_heap(indices, vals, signd)   _fast_pq.pyx:240-252 */
int tk_init_heap(int64_t *indices, int32_t *vals, int R, int signd);
/* insert(indices, vals, i, v)       _fast_pq.pyx:274-307 */
int tk_heap_insert(int64_t *indices, int32_t *vals, int R, int64_t i, int32_t v);
/* insert_is(indices, vals, i, v)    _fast_pq.pyx:256-271 */
int tk_heap_insert_is(int64_t *indices, int32_t *vals, int R, int64_t i, int32_t v);

/* FastPQ.distance_table / udistance_table   fast_pq.py:186-222 / :224-252
 * centers: float32 (16, dq) row-major; f_order != 0 when the caller's array was
 * F-ordered (dims_per_block == 1 leaves such a view, fast_pq.py:99-101; numpy then
 * sums the mean in that order).  q: (nq, dq) padded (and rotated) queries, float32
 * (q_is_f64 == 0) or float64.  aux0/aux1: signed: sqrt_n_blocks, unused;
 * unsigned: log(n_blocks), sqrt(n_blocks).  Outputs: tables uint8 (nq, M, 16) (the
 * transform_tables byte image), shift (nq,) in q's dtype, scale float64 (nq,).
 * dims_per_block 1 .. 32, at most 512 blocks, in both query types (as tk_index_set_pq).
 * The unsigned table sums a block's squares as numpy's `.sum(axis=-1)` does: one pairwise
 * leaf — sequential below 8 elements, 8 accumulators and a tail from 8 on. */
int tk_build_tables(const float *centers, int dq, int dpb, int f_order, const void *q,
                    int q_is_f64, int64_t nq, double aux0, double aux1, int signd,
                    uint8_t *tables, void *shift, double *scale);

/* knn_brute1(x, Y, k)  utils.py:89-92 (+ bottom_k :22-25): squared distances of
 * the n rows of Y (n, d) to x (d,), each float32 or float64 (flags; float64
 * arithmetic if either is, as numpy promotes `Y - x`), positions of the k smallest
 * in ascending order (ties: lower position first).  k >= n returns arange(n).
 * out_pos: int64 (min(k, n),).  Returns the count written, or <0. */
int64_t tk_knn_brute1(const void *x, int x_is_f64, const void *Y, int y_is_f64, int64_t n, int d,
                      int64_t k, int64_t *out_pos);

/* ---- device-resident code array ---------------------------------------------
 * A TransformedData (fast_pq.py:30,184) kept in HBM so that repeated
 * estimate_distances / top calls on the same data (examples/example.py:60-66 runs
 * 1000 of them) do not re-send the codes over PCIe. */
/* (a tk_codes handle carries the scratch of the calls made on it: one caller at a time per
 * handle; the host-buffer entry points above share one mutex-guarded scratch) */
typedef struct tk_codes tk_codes;
tk_codes *tk_codes_upload(const uint64_t *data, int64_t chunks, int M);
void tk_codes_free(tk_codes *c);
/* estimate_pq_* against the resident array: nq tables (nq, 2M) -> out (nq, 2*chunks) */
int tk_codes_estimate(tk_codes *c, const uint64_t *tables, int64_t nq, uint64_t *out, int signd,
                      int order);
/* same with device-resident tables (nq, M, 16) uint8 / out (nq, chunks*16) bytes, enqueued
 * on `stream`; four queries share each pass over the codes when nq >= 4 */
int tk_codes_estimate_dev(tk_codes *c, const void *tables_dev, int64_t nq, void *out_dev,
                          int signd, int order, void *stream);
/* query_pq_* against the resident array (indices / vals / labels are host buffers) */
int tk_codes_query(tk_codes *c, int64_t n, const uint64_t *tables, int64_t *indices,
                   int32_t *vals, int R, int signd, const int64_t *labels, int order);

/* ---- offline build path: the step before the hot path -------------
 * Both restate numpy's rounding (einsum order; OpenBLAS GEMM = FMA chain over k for the
 * shapes involved; argpartition's dumb_select) and reproduce the compiled reference's codes
 * and list memberships on the golden fixtures.
 *
 * tk_encode_pq: the per-block nearest-centroid search of FastPQ.transform
 * (fast_pq.py:174-181: knn_brute(col, code, 1) for every block).  data: (n, dq) rows after
 * the reference's padding (utils.py pad2) and, for a rotated PQ, after `data @ R.T` (a BLAS
 * GEMM that stays on the host; then float64).  labels: (n, M) uint8, to be packed by
 * transform_data (_transform.py:4-77). */
int tk_encode_pq(const float *centers, int dq, int dpb, const void *data, int data_is_f64,
                 int64_t n, uint8_t *labels);
/* tk_assign_lists: knn_brute(X, Y, k, metric) of IVF.build (ivf.py:85, utils.py:66-86) for
 * k <= 2 and d <= 384.  X: (n, d) float32 rows — whole 100-row chunks only (n % 100 rows at
 * the end of a data set are a differently shaped GEMM in numpy: the caller keeps numpy for
 * them); normalise != 0: X is divided by its row norms first (angular metric,
 * utils.py:73-74; d <= 128).  Y: (L, d) centres AFTER the caller's numpy normalisation,
 * float32 or float64, ynorm2 = np.einsum("ij,ij->i", Y, Y) in Y's dtype.
 * nearest: (n, k) int64 in numpy's argpartition order. */
int tk_assign_lists(const float *X, int64_t n, int d, int normalise, const void *Y, int y_is_f64,
                    const void *ynorm2, int64_t L, int k, int64_t *nearest);

/* ---- device-resident IVF index --------------------------------------------
 * Holds what the reference's IVF object holds after fit+build (ivf.py:14-17,
 * 77-102) in HBM, re-tiled for coalesced scans, and answers batches of queries
 * with the kernel pipeline that replaces IVF.query (ivf.py:106-163). */
typedef struct tk_index tk_index;

tk_index *tk_index_create(void);
void tk_index_destroy(tk_index *ix);

/* FastPQ state: centers (16, dq) float32, dims_per_block, sqrt_n_blocks
 * (fast_pq.py:99-102); f_order as in tk_build_tables; order = TK_ORDER_*.
 * dims_per_block 1 .. 32; an even number of blocks, at most 512 (float32 and float64 q_pq). */
int tk_index_set_pq(tk_index *ix, const float *centers, int dq, int dpb, int f_order,
                    double sqrt_n_blocks, int order);
/* active_centers (n_lists, d) float32 and their packed codes
 * pq_transformed_centers.packed (center_chunks, M)   ivf.py:91-96 */
int tk_index_set_centers(tk_index *ix, const float *active_centers, int64_t n_lists, int d,
                         const uint64_t *center_codes, int64_t center_chunks);
/* pq_transformed_points / ids (ivf.py:100-102) flattened list-major:
 * list_sizes (n_lists,) true rows; codes (sum ceil(size/16), M) packed chunks;
 * ids (sum size,) labels. */
int tk_index_set_lists(tk_index *ix, const int64_t *list_sizes, const uint64_t *codes,
                       const int64_t *ids);
/* IVF.data: the (normalised) vectors used for rescoring.  dtype: TK_DATA_F32 (0) or TK_DATA_F64 (1) as the
 * caller's X was (ivf.py:77-79 keeps X's dtype), or TK_DATA_F16 (2): `data` points at N * d IEEE halfs (the
 * caller rounded its float32 vectors: round-to-nearest-even, subnormals kept, every half finite) and the index
 * stores 2 bytes per element.  A half index answers, bit for bit, what the float32 index holding float(half(x))
 * answers: the final rescoring widens each stored value and sums in float32 (distances are float32); lists,
 * codes, probes and heaps do not read the vectors.
 * tk_index_narrow_data: the float32 vectors an index already holds in HBM (tk_index_alloc_data +
 *   tk_index_build_dev, or a float32 upload) become halfs, in a new buffer (the float32 one is freed: 1.5 x the
 *   float32 size for the length of the call).  A check pass runs first: a value whose half is not finite
 *   (|x| >= 65520, inf, NaN) is TK_ERR_ARG naming the first such row, and the index stays as it was.  A half
 *   index: TK_OK, nothing done.  Refused (TK_ERR_ARG): float64 vectors; a cloned shard (its vectors are
 *   borrowed) and an index that shards were cloned from (they are lent).  Batches in flight finish first.
 * tk_index_store: the dtype code of the index's vectors (TK_DATA_*), or -1 with no vectors set. */
#define TK_DATA_F32 0
#define TK_DATA_F64 1
#define TK_DATA_F16 2
int tk_index_set_data(tk_index *ix, const void *data, int dtype, int64_t N, int d);
int tk_index_narrow_data(tk_index *ix);
int tk_index_store(tk_index *ix);

/* _FastDistanceTable.top(transformed_data, data, k) (fast_pq.py:284-312) for a batch of queries
 * against the rows the index holds as its centres — tk_index_set_pq + tk_index_set_centers(rows,
 * packed codes) is all this call needs: per query a heap of rescore = min(2k + 10, n) PQ
 * estimates over ALL rows, then the exact float32 distances of those candidates (knn_brute1,
 * utils.py:89-92), the k best in ascending order.  (The coarse stage of IVF.query, ivf.py:131,
 * is this call on the coded centres.)  q: (nq, d) float32 rows as distance_table takes them,
 * q_pq: their padded / rotated form; out_ids: (nq, k) int64, -1 beyond n. */
int tk_index_top_centers(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq,
                         int k, int64_t *out_ids);
/* The same, and out_dist: (nq, k) float32, the exact squared distance beside each id (knn_brute1's
 * values, the ones the ids are ranked by; +inf beside a -1). */
int tk_index_top_centers_dist(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq,
                              int k, int64_t *out_ids, float *out_dist);

/* Largest batch the workspace is currently sized for grows on demand; this call
 * pre-sizes it (so that tk_index_query_batch_dev never allocates, e.g. under
 * stream capture). */
int tk_index_reserve(tk_index *ix, int64_t nq, int k, int n_probes, int pass_1);

/* IVF.query for a batch  ivf.py:106-163.
 * q: (nq, d) float32 queries AFTER the metric's normalisation (ivf.py:125-127 is
 * done by the host binding with numpy, as the reference does);
 * q_pq: (nq, dq) padded (rotated) queries for the table build, float32 or float64.
 * pass_1 <= 0 selects (n_probes+1)*k+1 (ivf.py:135-136).
 * out_ids: int64 (nq, k), rows padded with -1 when fewer than k ids exist.
 * Optional debug outputs (NULL to skip): out_probes int64 (nq, min(n_probes,n_lists)),
 * out_heap_idx int64 (nq, pass_1), out_heap_val int32 (nq, pass_1). */
int tk_index_query_batch(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64,
                         int64_t nq, int k, int n_probes, int pass_1, int64_t *out_ids,
                         int64_t *out_probes, int64_t *out_heap_idx, int32_t *out_heap_val);

/* Same with device-resident inputs/outputs, enqueued on `stream`, no sync.  Large
 * batches are processed in sub-batches whose distance buffers stay under 16 GB (TINYKNN_WORKSPACE_GB):
 * EQUAL parts of at most tk_index_max_sub_batch queries, each through the pipeline by itself (calls that fit one
 * workspace are what pairs up under tk_index_set_coalesce).
 * An index handle serves one caller at a time: its entry points take a per-handle lock, so
 * calls from several threads are serialised (the reference's kernels are nogil and re-entrant
 * on distinct buffers; use one handle per thread for concurrency). */
int tk_index_query_batch_dev(tk_index *ix, const float *q_dev, const void *q_pq_dev,
                             int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                             int64_t *out_ids_dev, void *stream);

/* Batches in flight.  depth = 1 (default): tk_index_query_batch_dev enqueues the whole
 * pipeline on the caller's stream.  depth > 1: ALL code scans and the table builds run on
 * the caller's stream, in order — call c launches ONE kernel there that carries the list
 * scan of call c-2 and the coarse scan of call c as one pool of work — the coarse heap
 * replays + descriptors of all batches on one internal stream, and the heap replay (157
 * waves per 10 000 queries) + rescoring of a batch on one of `depth` more, handed over by
 * events and overlapping the scans of the later batches.  depth = 2 keeps the total at the
 * four hardware queues HIP maps streams onto (more streams share queues and serialise).
 * tk_index_join enqueues the list scans still owed and their replays.  The caller must not
 * reuse the input/output buffers of a call before tk_index_join(ix, stream), which also
 * makes `stream` wait for every batch in flight.  Stream capture (hipGraph) of a batch
 * needs depth = 1: the pipelined mode hands work to streams outside the capture. */
int tk_index_set_pipeline(tk_index *ix, int depth);
int tk_index_join(tk_index *ix, void *stream);
/* n = 2 (pipelined mode only): two consecutive tk_index_query_batch_dev[_ex] calls with the same
 * k / n_probes / pass_1 / stream run through the pipeline as ONE batch of nq_a + nq_b queries.
 * The kernels that leave most of the chip idle (two heap replays of 157 dependent waves per
 * 10 000 queries, the small kernels of the coarse stage) take as long for 20 000 queries as for
 * 10 000.  The first call is held and returns; the second joins it and enqueues the pair.  Nothing is
 * copied: the kernels read each call's queries from, and write its ids to, the call's own buffers
 * (which stay the library's until tk_index_join, as above); each call's completion event is recorded
 * behind the pair's last kernel.  Results are those of separate calls
 * (the same kernels over the same rows).  A held call is launched alone by tk_index_join /
 * tk_index_quiesce / any tk_index_set_*, or when the next call cannot join it.
 * A HELD call has enqueued NOTHING yet: its completion event (tk_index_query_batch_dev_ex) is not
 * recorded and its pinned copy not ordered until its partner arrives or tk_index_join runs — wait on
 * such an event only after one of the two (tk_index_pending() > 0 says calls are still owed;
 * hipEventSynchronize on a never-recorded event returns at once).  n = 1 (default):
 * every call its own batch.  ivf.py:106-163 answers one query per call; the batch forms here and
 * everything about their scheduling are this library's. */
int tk_index_set_coalesce(tk_index *ix, int n);
/* what tk_index_set_coalesce was last given (1 or 2); the pipeline depth is info8[5] of tk_index_info */
int tk_index_coalesce(tk_index *ix);
/* hipGraph of the pipelined mode: tk_index_quiesce (device-synchronising; forgets the completion
 * events of earlier calls), then capture on a non-NULL stream any number of
 * tk_index_query_batch_dev calls followed by tk_index_join on that stream.  The internal streams
 * fork from the capturing stream through the events the calls record on it and are all joined
 * again by tk_index_join, so the capture is one self-contained graph: replaying it runs the
 * captured batches at the pipelined rate (workspaces, events and streams must exist beforehand:
 * run the same calls once uncaptured, tk_index_set_profiling off).
 * The capture state is the CALL's, not the index's: an entry point is "inside a capture" iff the stream it is given
 * is being captured (tk_index_query_batch_dev and its _ex forms, tk_index_join); it then queries no event, and
 * refuses to make a restriction's table.  Entry points that take no stream (tk_index_query_batch, tk_index_knn_group,
 * tk_index_knn_between, tk_index_set_*, ...) are never inside a capture: they may follow a capture at once, with no
 * tk_index_quiesce in between, and make the tables they need.  A call still owed (held for its partner, or pending
 * in the pipeline) keeps the state of the stream IT was issued on: whoever enqueues its remaining stages — the next
 * call, tk_index_join, a tk_index_set_* that flushes — does so as inside that capture.  A capture is complete only
 * after tk_index_join on the capturing stream. */
int tk_index_quiesce(tk_index *ix);

/* Heap replay strategy.  0 = automatic: when the replay can skip `insert`'s
 * duplicate-label scan without changing the result (fresh heaps and pairwise
 * distinct labels, i.e. IVF.build(n_probes=1)) each LANE replays one query (64
 * queries per wave, heap columns in LDS; pass_1 <= 574), or, for larger heaps, a
 * wave replays one query on packed 32-bit entries; otherwise the general kernel
 * (int64 labels + duplicate scan, one query per wave) runs.  1 = always the
 * general kernel.  2 = the packed wave kernel instead of the lane kernel.  3 = the
 * wave-per-query register heap (heaps of <= 513 entries; automatic for small batches,
 * TK_OPT_PAIR_NQ) for every batch size.  All are
 * bit-exact replays of _fast_pq_256.pyx:73-123; the switch exists for A/B timing
 * and for the parity tests. */
int tk_index_set_heap_mode(tk_index *ix, int mode);

/* Probed-list scan strategy.  0 = automatic: list-major (each chunk scored for
 * four queries per pass, pairs grouped by list on the device) when a batch has at
 * least 8 (query, probe) pairs per list, else query-major (one query per wave).
 * 1 = always query-major, 2 = always list-major.  Identical outputs. */
int tk_index_set_scan_mode(tk_index *ix, int mode);

/* Probed lists behind the first ones as PLAIN integer sums on the int8 matrix cores
 * (v_mfma_i32_32x32x32_i8: one-hot(code) x table), clamped to int8.  For a query whose table
 * bounds the negative mass of each of the reference's saturating chains by 128, clamp(plain sum)
 * equals the value compute_block_dists_avx (_fast_pq_256.pyx:126-156) returns wherever that value
 * is below C = 127 - (negative mass) and is >= C elsewhere; the replay inserts only rows below
 * its bound, which never rises (_fast_pq_256.pyx:73-123), so once the bound is <= C the replay
 * over the plain sums IS the replay over the reference's values.  The first probed lists of a
 * query (until they hold 2 * pass_1 rows) stay on the exact kernel; the lane replay checks the
 * condition per query and the queries that fail it are scanned again exactly and replayed again:
 * results are identical to mode 1 in every case (tests/test_plain_scan_gpu.py).
 * 0 = automatic (list-major batches, signed tables, <= 52 blocks, lane replay): a flagged query
 * costs two scans and two replays, so the path first proves itself on ONE probe batch (the batches
 * behind it stay exact until its flagged count has come back — read from a page-locked word, never
 * waited for), is used while at most 1 % of a batch's queries are flagged, and otherwise pauses
 * for 256..4096 batches before the next probe (data without structure: 42 % flagged on iid
 * vectors); 1 = off; 2 = always (no pausing: tests, A/B).  Every mode returns identical results.
 * Environment TINYKNN_PLAIN_SCAN=0 switches it off process-wide. */
int tk_index_set_plain_scan(tk_index *ix, int mode);
/* Accounting of the plain path for the last batch enqueued (synchronises): out8 = plain units
 * (tiles of 32 pairs), plain pairs, exact pair records, head pair records, queries flagged for the
 * re-scan, sum over the plain units of the list's chunk pairs, state of mode 0 (0 probe next,
 * 1 waiting for the probe's count, 2 on, 3 paused), batches left of the pause. */
int tk_index_plain_stats(tk_index *ix, int64_t *out8);
/* Which heap replay the last batch enqueued took for its probed lists (read-only, nothing is waited for; with
 * batches in flight: the last one whose replay has been launched).  out4 = the form (below; -1 before the first
 * batch), 1 where the lane replay ran lazy (TK_OPT_REPLAY_LAZY), 1 where the register heap ran on value8 << 24 |
 * label24 entries (TK_OPT_LABELS24), the twin table width the TWIN form used (0 for every other form).  Results
 * never depend on the form; the tests of one form assert that their batch took it.
 * It is the form the dispatch CHOSE: the launcher of the lane replay would still drop a twin table that came without
 * its arrays or with uniform slots (no list replay passes either).  A call that the library splits into sub-batches
 * reports its last sub-batch alone: a short tail may have taken TK_REPLAY_PAIR where the others did not. */
#define TK_REPLAY_PAIR 0            /* register heap, one query per wave (small batches, heap mode 3) */
#define TK_REPLAY_LANES 1           /* lane per query, distinct labels */
#define TK_REPLAY_PACKED_DISTINCT 2 /* packed wave kernel, distinct labels */
#define TK_REPLAY_LANES_TWIN 3      /* lane per query, labels that repeat: duplicate test from the twin table */
#define TK_REPLAY_LANES_DEDUPE 4    /* lane per query, labels that repeat: duplicate test on a hash set of the labels */
#define TK_REPLAY_PACKED 5          /* packed wave kernel, duplicate test for every query */
#define TK_REPLAY_GENERAL 6         /* general wave kernel (heap mode 1, rows too long for position entries) */
int tk_index_last_replay(tk_index *ix, int64_t *out4);
/* The two buckets (0..63, never equal) in which the lane replay's hash set may keep `label`: four labels per
 * bucket, four more in a stash, and a lane whose label finds all of them taken falls back to a scan of its heap's
 * labels.  The kernel's own function (no device needed): what a test draws colliding labels from. */
int tk_label_buckets(uint32_t label, int *b1, int *b2);
/* Per-index options (no process-wide state: the reference's entry points carry none either,
 * _fast_pq.pyx:101-307 are nogil and re-entrant).  Results never depend on an option; they exist for
 * A/B measurements and for the tests.
 *   TK_OPT_SCAN_FORM     table rows of the exact list-major kernel: 0 = per-lane global loads (DEFAULT;
 *                        fastest, profiles/r02_scan_forms.md), 1 / 2 = staged per block in LDS (a launch
 *                        that carries the exact heads of a plain batch always runs form 0: only that
 *                        form knows row limits)
 *   TK_OPT_RESCORE_FORM  candidate rows of the rescoring: 2 = staged through LDS in tiles of 32 rows
 *                        (DEFAULT), 1 = tiles of 64, 0 = every lane walks its own row (always for float64
 *                        operands and d % 4 != 0)
 *   TK_OPT_PLAIN_LIMIT   a cap on every query's table limit C (plain_scan.hip's lemma; INT_MAX = none):
 *                        -128 sends EVERY query of a plain batch through the exact re-scan + second
 *                        replay (tests/test_plain_scan_gpu.py) */
#define TK_OPT_SCAN_FORM 1
#define TK_OPT_RESCORE_FORM 2
#define TK_OPT_PLAIN_LIMIT 3
/*   TK_OPT_REPLAY_LAZY   the lane replay of the probed lists: 1 = nothing is staged, a lane reads its row's block
 *                        minima and fetches a block only where its minimum passes the bound (as FlatTop's
 *                        replay); 0 = every block staged through LDS; -1 = by the index (DEFAULT: lazy where a
 *                        query's probed lists hold more than 8 heap sizes of blocks — 100M x 128: 6 250 blocks
 *                        against a heap of 111).  Identical results. */
#define TK_OPT_REPLAY_LAZY 4
/*   TK_OPT_REPLAY_COUNT  1: the lane replays of the probed lists count their insert rounds (measurement plumbing
 *                        for bench.py's roofline.replay; read and zeroed by tk_index_replay_stats); 0 (DEFAULT): off */
#define TK_OPT_REPLAY_COUNT 5
/*   TK_OPT_REPLAY_TWIN   labels that repeat (IVF.build(n_probes >= 2), ivf.py:53): 1 (DEFAULT) = the lane replay
 *                        decides `insert`'s duplicate test (_fast_pq.pyx:284-287) from the positions of a row's
 *                        other copies (twins.hip's table, heap.hip TWIN form: 64 queries per wave, position
 *                        entries, no set of labels); 0 = the hash set of the labels in the heap (32 queries per
 *                        wave).  Identical results. */
#define TK_OPT_REPLAY_TWIN 6
/*   TK_OPT_TWIN_VOUCH    the TWIN form rests on two facts about the lists: the copies of a label lie in different lists
 *                        and carry the same code — true of IVF.build's lists (ivf.py:77-102: a list's codes are the codes
 *                        of data[ids]).  tk_index_set_lists and tk_index_build_dev hold every list's codes and CHECK
 *                        them on the device (an index that fails keeps the label-based test); a rank that was handed
 *                        only its own lists' codes (tk_index_set_lists_shard) cannot, and uses the table only behind
 *                        1 = "the caller has checked" (tinyknn_amd.DeviceIndex does, on the host).  0 (DEFAULT). */
#define TK_OPT_TWIN_VOUCH 7
/*   TK_OPT_PAIR_NQ       batches of up to this many queries (DEFAULT 8192 one batch at a time, at most 4096 per launch — a pair
 *                        of calls of 2048 — in pipelined mode; 0 = never; environment TINYKNN_PAIR_NQ sets the default of new indexes) replay their heaps
 *                        one query per WAVE with the heap in registers, two / four / eight nodes per lane (heaps of <= 129 /
 *                        257 / 513 entries: IVF.query's 111 and its coarse top's 30 at the reference's bench settings,
 *                        examples/bench.py:118-137): one query per call is ~760 dependent inserts, 0.47 of 0.54 ms in the
 *                        lane kernel, 0.12 of 0.19 ms here.  Same heap arrays. */
#define TK_OPT_PAIR_NQ 8
/*   TK_OPT_LABELS24      the register heap's duplicate test (labels that repeat, IVF.build(n_probes >= 2); a probe list
 *                        that names a list twice): 1 (DEFAULT) = on entries value8 << 24 | label24 — one register per
 *                        slot, as with positions — where every label of the index is below 0xffffff (16.7 M rows);
 *                        0 = always on (value, label64) entries, three registers per slot (what larger indexes get). */
#define TK_OPT_LABELS24 9
int tk_index_set_option(tk_index *ix, int option, int value);
/* The table behind TK_OPT_REPLAY_TWIN (diagnostics, tests): *rows = stored rows (the length of the concatenated
 * ids), *w = other copies listed per row (0: no table — labels distinct, not int32, or one label stored more
 * than 17 times); list_out / off_out (rows x w int32 each, or NULL): list and offset inside that list of a
 * row's u-th other copy, -1 where a label has fewer copies.  What the reference finds by scanning the heap's
 * labels in `insert` (_fast_pq.pyx:284-287) follows from these positions (heap.hip, TWIN form). */
int tk_index_twin_table(tk_index *ix, int64_t *rows, int *w, int32_t *list_out, int32_t *off_out);

/* Stage timing.  on = n > 0: every n-th (sub-)batch records HIP events on its streams
 * around the stages (no synchronisation in the query call; 1 = every batch).
 * tk_index_last_profile synchronises that stream and returns the mean
 * milliseconds per stage over the batches recorded since the last read
 * [tables, coarse_scan, coarse_heap, coarse_rescore+slots, scan, heap, rescore, plain kernel alone
 * (HIP events in front of and behind scan_plain_wave_kernel on the stream it is launched on; 0 when
 * no recorded batch ran it)], their count, and the algorithmic bytes the list-scan kernel streamed for the
 * most recent batch (code bytes + table + heap per query; with depth > 1 the
 * timed launch also carries the next batch's coarse scan, whose bytes are included). */
int tk_index_set_profiling(tk_index *ix, int on);
int tk_index_last_profile(tk_index *ix, float *ms8, double *scan_bytes, int *batches);

/* measurement plumbing (bench.py): GB/s of a kernel that only reads `bytes` of HBM, every byte
 * once with the flat scan's access pattern — the streaming-read ceiling of the box */
/* out4 = insert rounds summed over the replay waves, the most rounds one wave ran, waves, and — summed over the
 * waves — the refills of the per-lane rings (the form without a duplicate test) or the 16-block segments walked
 * (the others), since TK_OPT_REPLAY_COUNT was set / the last call (synchronises, zeroes) */
int tk_index_replay_stats(tk_index *ix, int64_t *out4);
int tk_measure_read_bandwidth(int64_t bytes, int reps, double *gbps);
/* ... and of a kernel that gathers n_gather random rows of row_bytes (16 .. 1024, a multiple of 16) out of
 * table_bytes of HBM with the rescoring kernel's access pattern (knn_brute1's `data[indices]`, utils.py:89-92):
 * the ceiling bench.py's roofline.rescore is quoted against. */
int tk_measure_gather_bandwidth(int64_t table_bytes, int row_bytes, int64_t n_gather, int reps, double *gbps);
/* The library's own exclusive prefix sum (one launch, decoupled look-back: devbuild.hip) on host arrays — the
 * per-batch sums of a list-sharded rank go through it on the device; this entry exists so that a test can check it
 * against numpy at any length.  is64: int64 elements, else int32.  in_host == out_host is allowed. */
int tk_scan_exclusive_host(const void *in_host, void *out_host, int64_t n, int is64);

/* ---- device-resident build ----------------------------------------
 * IVF.build(X, n_probes = 1 or 2) (ivf.py:77-102) for float32 vectors that are produced IN HBM
 * and never visit the host — how the 100M x 128 configuration is assembled ("per-GPU
 * generation on device (seeded per shard), codes produced by the build's encoder").
 * tk_index_alloc_data: after tk_index_set_pq; the index allocates its (N, d) float32
 *   rescoring vectors and returns the device pointer for the caller to fill (NULL on error).
 * tk_index_synth_data: fills rows [row0, row0 + n) with centres[c(row)] + sigma * N(0, 1)
 *   from a counter-based generator — a pure function of (seed, row, column), independent of
 *   how the rows are split over calls or ranks; centres: host (n_centres, d) float32 or NULL
 *   (noise only).  tk_synth_rows: the same generator into a host buffer (queries, samples).
 * tk_index_build_dev: normalise != 0 divides every row by its norm first (ivf.py:78-79);
 *   the n_probes <= 2 nearest of the C centres per row (knn_brute(data, all_centers, n_probes),
 *   ivf.py:85; with 2 every row sits in two lists, column-0 members of a list before its column-1
 *   members as group_data_by_indices appends them, and the replay runs its duplicate test):
 *   search_centers (C, d) float32 = all_centers after knn_brute's own normalisation for the
 *   angular metric (utils.py:75; NULL: all_centers themselves), ynorm2 its einsum norms),
 *   active centres = the rows of all_centers that own a vector, in id order (ivf.py:91), PQ codes of
 *   every row and of the active centres (R (dq, d_pad) float64 = FastPQ.R or NULL; the
 *   rotation is the float64 FMA chain of the device front end, not numpy's DGEMM), rows
 *   grouped by list in ASCENDING ROW ORDER (numpy's unstable argsort leaves the order inside
 *   a list unspecified, utils.py:131), packed into the Quick-ADC layout.  The index is then
 *   complete (centres, lists, data).  n_active_out: number of lists.
 * tk_index_export_lists / _centers / tk_index_read_rows: what a built index holds, back on
 *   the host in the reference's formats (list_sizes (n_lists,), packed codes (sum
 *   ceil(size/16), M) uint64, ids (sum size,); active centres and their packed codes; rows of
 *   IVF.data by id; float32 vectors, or half vectors widened) — any output may be NULL. */
float *tk_index_alloc_data(tk_index *ix, int64_t N, int d);
int tk_index_synth_data(tk_index *ix, int64_t row0, int64_t n, uint64_t seed, const float *centres,
                        int n_centres, float sigma);
int tk_synth_rows(float *out, int64_t row0, int64_t n, int d, uint64_t seed, const float *centres,
                  int n_centres, float sigma);
int tk_index_build_dev(tk_index *ix, int normalise, const float *all_centers,
                       const float *search_centers, const float *ynorm2, int64_t C, int n_probes,
                       const double *R, int d_pad, int64_t *n_active_out);
int tk_index_export_lists(tk_index *ix, int64_t *list_sizes, uint64_t *codes, int64_t *ids);
int tk_index_export_centers(tk_index *ix, float *active_centers, uint64_t *center_codes);
int tk_index_read_rows(tk_index *ix, const int64_t *rows, int64_t n, float *out);

/* ---- rows added to a built index, in place (IVF.add) ----------------------------------------
 * tk_index_add_rows appends n rows with ids N .. N + n - 1 and leaves the index exactly as the
 * index's own build over (old rows, new rows) would: a row's code and lists do not depend on the
 * other rows.  Every list keeps its old members at their old positions inside their column
 * block: with kp lists per row (the build's n_probes) list l's column-j block becomes
 * old_j ++ new_j, new_j = the new rows whose nearest[:, j] is l in ASCENDING row order (for
 * kp >= 2 new column-0 members land in the middle of a list, before the old column-1 members,
 * where group_data_by_indices puts them).  An index made by tk_index_build_dev over N + n rows
 * is byte-identical; against a host build (numpy's unstable argsort) the order inside a kp = 1
 * list is unspecified, as there.  Padding rows carry the zero vector's code.
 *   rows: (n, d) float32, or float64 (rows_is_f64) where the index's vectors are float64; host
 *     or device memory.  normalise != 0: divided by their norm on the device first (float32).
 *     An index of half vectors (TK_DATA_F16) takes float32 rows: they are normalised, assigned and coded
 *     from their float32 values in a staging buffer (lists and codes are the float32 index's), checked
 *     (a value whose half is not finite: TK_ERR_ARG naming the row, nothing changed) and only then
 *     appended to the stored vectors rounded to half.
 *   nearest (n, kp) int64 centre ids, or NULL: found on the device as tk_index_build_dev finds
 *     them (all_centers / search_centers / ynorm2 / C as there).
 *   labels (n, M) uint8 PQ labels, or NULL: encoded on the device as tk_index_build_dev does.
 *   list_columns (n_lists, kp) int64 members per (list, column) of the old lists, or NULL where the
 *     index knows them (tk_index_build_dev, an earlier add: tk_index_list_columns).
 *   C: centres; new rows may activate centres n_lists .. only so that the active ones stay a prefix
 *     (the build's contract, utils.py:128; else TK_ERR_ARG).  New lists are appended, their centres
 *     (rows of all_centers) coded by center_codes ((ceil(L'/16), M) uint64 packed, host) or, NULL,
 *     on the device.  n_active_out: number of lists afterwards.
 * Batches in flight are completed first; allowed sets made before fail afterwards (a new layout).
 * A refused or failed call leaves the index as it was.  A list-sharded index is refused.
 * tk_index_list_columns: *kp = columns known (0: none, a host upload), counts (n_lists, kp). */
int tk_index_add_rows(tk_index *ix, const void *rows, int rows_is_f64, int64_t n, int kp,
                      const int64_t *nearest, const uint8_t *labels, const int64_t *list_columns,
                      int normalise, const float *all_centers, const float *search_centers,
                      const float *ynorm2, int64_t C, const uint64_t *center_codes, int64_t *n_active_out);
int tk_index_list_columns(tk_index *ix, int *kp, int64_t *counts);

/* ---- rows removed from a built index, in place (IVF.remove) ----------------------------------
 * tk_index_remove_rows deletes every stored copy of the n rows named by `rows` (int64 row ids in
 * [0, N), host or device memory; duplicates allowed; ids in range but no longer stored are ignored,
 * so a second call changes nothing).  Ids stay stable: N and the vectors are untouched (a removed
 * row's vector stays as dead weight) and a later tk_index_add_rows still appends ids N ..  Every
 * list keeps its surviving members in their old order: with kp lists per row list l's column-j
 * block becomes old_j minus the removed rows.  A list that empties stays, with its centre.  The
 * index afterwards is byte-identical to tk_index_set_lists of the filtered lists (sizes, offsets,
 * codes with the zero vector's code in the padding rows, ids, their int32 copy, twin table).
 *   kp, list_columns (n_lists, kp) int64 members per (list, column), or NULL where the index knows
 *     them (tk_index_build_dev, tk_index_add_rows, an earlier removal: tk_index_list_columns); given
 *     ones are checked against the list sizes.  Neither: the lists are compacted all the same and
 *     their columns stay unknown.
 *   removed_out: stored entries removed (a row stored in kp lists counts kp times), or NULL.
 * Batches in flight are completed first; allowed sets made before fail afterwards (a new layout)
 * unless nothing stored was named.  An id outside [0, N) is refused (TK_ERR_ARG), as is a
 * list-sharded index; a refused or failed call leaves the index as it was.
 * tk_index_add_rows after a removal: every row still stored must sit in exactly kp lists (checked
 * on the device where fewer than N * kp entries remain). */
int tk_index_remove_rows(tk_index *ix, const int64_t *rows, int64_t n, int kp,
                         const int64_t *list_columns, int64_t *removed_out);

/* ---- stored rows replaced in a built index, in place, ids kept (IVF.update) -------------------
 * tk_index_update_rows gives the n rows named by `ids` (int64 row ids in [0, N), pairwise
 * distinct; host or device memory) the new vectors `rows` (n, d).  The index afterwards is the
 * one that tk_index_remove_rows(ids) followed by tk_index_add_rows(rows) gives on the same index,
 * with two differences: the added row N + i carries the label ids[i] in every list, and its
 * prepared vector sits in row ids[i] of the stored vectors, not behind the old rows.  N and the
 * size of the vector store do not change.  With kp lists per row list l's column-j block becomes
 * (old_j minus the rows in ids, old order kept) ++ (the rows i whose nearest[:, j] is l,
 * ASCENDING i, labelled ids[i]).  A row in ids that was removed earlier is stored again (the hole
 * is refilled); a row whose nearest list does not change moves to the end of its column block; a
 * list that empties stays, with its centre; rows that activate centres n_lists .. append lists
 * under the prefix rule of tk_index_add_rows.  The index is byte-identical to tk_index_set_lists
 * of those lists (sizes, offsets, codes with the zero vector's code in the padding rows, ids,
 * their int32 copy, twin table) over the vectors with their rows replaced.
 *   rows, nearest, labels, list_columns, normalise, all_centers, search_centers, ynorm2, C,
 *     center_codes, n_active_out: as in tk_index_add_rows — the rows are prepared exactly as there
 *     (normalisation, assignment, PQ labels; a half store takes float32 rows, assigns and codes
 *     them from their float32 values and stores them rounded as tk_index_narrow_data rounds).
 *   removed_out: stored entries of the old versions that went (kp per row that was stored), or NULL.
 * The lists are rewritten in ONE pass: the old code array is read once and the new one written
 * once (nothing old is decoded or re-encoded), the vectors are scattered once.
 * Order inside the call: batches in flight are completed first, on the old lists AND the old
 * vectors; the rows are staged and prepared in a scratch buffer, never in the live store; the new
 * lists are built completely in new buffers; only behind the last point that can fail are the
 * vectors overwritten and the lists swapped.  So a refused or failed call leaves the lists and
 * the vectors as they were.  Refused (TK_ERR_ARG): an id outside [0, N) or named twice; a row
 * whose half is not finite on a half store (naming the row of `rows`); what tk_index_add_rows
 * and tk_index_remove_rows refuse (a list-sharded index, kp against the stored copies, unknown
 * list_columns, the prefix rule).  Allowed sets made before fail afterwards (a new layout); the
 * row-position table of exclude= and the group table follow the new layout on their next use.
 * n == 0 changes nothing. */
int tk_index_update_rows(tk_index *ix, const int64_t *ids, int64_t n, const void *rows, int rows_is_f64,
                         int kp, const int64_t *nearest, const uint8_t *labels, const int64_t *list_columns,
                         int normalise, const float *all_centers, const float *search_centers,
                         const float *ynorm2, int64_t C, const uint64_t *center_codes,
                         int64_t *n_active_out, int64_t *removed_out);

/* ---- device front end, "fast mode"  -----------------------------------
 * What IVF.query does on the host before the table build (ivf.py:125-128,
 * fast_pq.py:200-204): float32 normalisation for the angular metric, zero padding to dq,
 * rotation by R.  NOT bit-identical to the host path, which is the default everywhere:
 * numpy normalises with a BLAS dot and rotates with a BLAS GEMV whose summation orders are
 * not restated.  Here the norm is numpy's pairwise float32 sum (bit for bit
 * x / np.linalg.norm(x, axis=1)) and the rotation a float64 FMA chain over ascending t.
 * Measured against the host's: a normalised element is at most 4 float32 ulp
 * away (74 % identical, 22 % one ulp); a rotated one differs by at most 7.5 * 2^-53 * sum_t
 * |x_t R_jt| — a few float64 ulp of an ordinary output (median 2), thousands where the sum
 * cancels to a small value.  The ids differ only where that flips a quantised table entry or
 * a rescoring tie.
 * tk_index_set_rotation: R (dq, d_pad) float64 row-major = FastPQ.R, or NULL (no rotation).
 * tk_index_prepare_dev: q_raw_dev (nq, d) float32 -> qn_dev (nq, d) float32 (normalised if
 * `angular`, else a copy; may alias q_raw_dev) and q_pq_dev (nq, dq) float64 when a rotation
 * is set, float32 otherwise — the two inputs of tk_index_query_batch_dev. */
int tk_index_set_rotation(tk_index *ix, const double *R, int d_pad);
int tk_index_prepare_dev(tk_index *ix, const float *q_raw_dev, int64_t nq, int angular,
                         float *qn_dev, void *q_pq_dev, void *stream);
/* raw float32 queries on the host -> ids on the host through the fast front end (H2D,
 * prepare, pipeline, D2H; synchronous) */
int tk_index_query_batch_raw(tk_index *ix, const float *q_raw, int64_t nq, int angular, int k,
                             int n_probes, int pass_1, int64_t *out_ids);

/* ---- exact host front end + streaming sessions (front.hip) ------------------------------
 * The host side of IVF.query (ivf.py:125-128, fast_pq.py:200-204): float32 normalisation
 * by np.linalg.norm = sqrtf(cblas_sdot(x, x)), pad1, and the float64 rotation
 * q @ R.T = cblas_dgemv(ColMajor, Trans, d_pad, dq, 1, R, d_pad, x, 1, 0, y, 1).  The
 * summation orders of those two calls belong to the BLAS build numpy links and are not
 * restated: tk_host_blas_bind resolves both symbols from THAT library (path of the shared
 * object numpy loaded; ILP64 "64_"-suffixed and "scipy_"-prefixed names are tried first),
 * and tk_prepare_queries_host calls them row by row from a thread pool — the reference's
 * arithmetic, bit for bit, without the Python loop.  No restated CPU arithmetic: without a
 * bound BLAS the call fails (TK_ERR_STATE).
 * tk_host_threads(n): pool size (n <= 0: keep / create the default = min(cores, 32), env
 * TINYKNN_HOST_THREADS); returns the size in use.
 * tk_prepare_queries_host: q_raw (nq, d) float32 -> qn (nq, d) float32 (normalised when
 * `angular`; may alias q_raw: the reference normalises in place) and, with R (dq, d_pad)
 * float64 row-major = FastPQ.R, q_pq (nq, dq) float64 = pad1(qn) @ R.T.  Without R the
 * table-build query is pad1(qn) (zeros appended), which needs no arithmetic. */
int tk_host_blas_bind(const char *blas_shared_object_path);
int tk_host_blas_bound(void);
int tk_host_threads(int n);
int tk_prepare_queries_host(const float *q_raw, int64_t nq, int d, int angular, float *qn,
                            const double *R, int dq, int d_pad, double *q_pq);

/* tk_index_query_batch_dev with a completion hook: behind the batch's last kernel the ids
 * are copied into out_ids_pinned (page-locked host memory, or NULL) and done_event (a
 * hipEvent_t, or NULL) is recorded.  With tk_index_set_pipeline(depth > 1) that happens up
 * to three calls later (or at tk_index_join); tk_index_pending = number of calls whose last
 * stage is not enqueued yet.  nq must fit one sub-batch (tk_index_max_sub_batch).
 * With tk_index_set_coalesce(ix, 2) the first call of a pair is only held: done_event is valid
 * (recorded) only once the partner call has been made or tk_index_join has run.
 * The internal front / replay streams of the pipelined mode belong to the PROCESS (one set per
 * device, shared by every index).  While a hipGraph capture of one index is open (between
 * tk_index_quiesce and the end of the capture) no other index of the process may be used: its work
 * would be pulled into, or invalidate, the foreign capture. */
int tk_index_query_batch_dev_ex(tk_index *ix, const float *q_dev, const void *q_pq_dev,
                                int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                                int64_t *out_ids_dev, int64_t *out_ids_pinned, void *done_event,
                                void *stream);
int64_t tk_index_max_sub_batch(tk_index *ix, int k, int n_probes, int pass_1);

/* Allowed sets: IVF.query restricted to a subset of the rows (one tenant, one category, "not deleted").
 * A query with allowed set A returns what IVF.query (ivf.py:106-163) returns when `insert` in query_pq
 * (_fast_pq_256.pyx:114-118, _fast_pq.pyx:197-201) runs only for labels in A; everything else is the
 * reference's: coarse stage and probe order, pass_1, the stale bound per 16-row block, the -1 removal and
 * the `len(indices) <= k` early return (ivf.py:152-156), knn_brute1 over the surviving candidates
 * (ivf.py:157-163).  Results are bit for bit those of that guarded reference.
 * tk_allow_create: mask = N bytes over row ids 0..N-1 (nonzero = allowed), uploaded once and turned on the
 * device into 16 bits per stored chunk in list-position order, from the index's device-resident labels (so
 * indexes built in HBM work too).  A set belongs to the layout of the lists it was made for: after the lists
 * are set again a query with it fails (TK_ERR_STATE).  Not for list-sharded indexes.
 * tk_allow_count: allowed stored rows (a label stored in two lists counts twice), < 0 on error.
 * tk_allow_destroy: enqueues the index's calls still owed, waits for the device, frees the set.  Destroy
 * every set of an index before the index. */
typedef struct tk_allow tk_allow;
int tk_allow_create(tk_index *ix, const uint8_t *mask, int64_t n, tk_allow **out);
int64_t tk_allow_count(const tk_allow *a);
int tk_allow_destroy(tk_allow *a);
/* tk_index_query_batch / tk_index_query_batch_dev_ex with an allowed set (NULL: the unrestricted call).
 * A set that allows every stored row takes the unrestricted path.  With tk_index_set_coalesce(ix, 2) only
 * calls with the same set (or none) pair up.  The automatic plain-scan state (tk_index_set_plain_scan 0)
 * is the unrestricted traffic's: restricted calls take the exact scan in that mode and leave the state
 * as it is; mode 2 runs them on the plain path too. */
int tk_index_query_batch_allow(tk_index *ix, const tk_allow *allow, const float *q, const void *q_pq,
                               int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                               int64_t *out_ids, int64_t *out_probes, int64_t *out_heap_idx,
                               int32_t *out_heap_val);
int tk_index_query_batch_dev_allow(tk_index *ix, const tk_allow *allow, const float *q_dev,
                                   const void *q_pq_dev, int q_pq_is_f64, int64_t nq, int k, int n_probes,
                                   int pass_1, int64_t *out_ids_dev, int64_t *out_ids_pinned,
                                   void *done_event, void *stream);
/* Ids and their distances.  out_dist[i, j] is the exact squared Euclidean distance between stored row
 * out_ids[i, j] of tk_index_set_data's vectors and query row q[i], summed as knn_brute1 does (utils.py:89-92:
 * einsum("ij,ij->i", diff, diff) of diff = data[id] - q) — the value the rescoring ranks by.  Element type:
 * float32, or float64 after tk_index_set_data(..., TK_DATA_F64) (numpy's promotion of `Y - x`); +inf
 * beside every -1.  The ids are those of the ids-only call, bit for bit.  Where a query had more than k
 * candidates its row is in rescored order (distances non-decreasing); where it had k or fewer the ids keep
 * heap order (ivf.py:158-159) and each still gets its distance, so such a row need not be sorted.
 * allow: an allowed set, or NULL for every row.  tk_index_query_batch_dist: host buffers, as
 * tk_index_query_batch without the debug outputs.  tk_index_query_batch_dev_dist: device buffers, as
 * tk_index_query_batch_dev_ex without the pinned copy — sub-batches, the pipelined mode and pairs of calls
 * (a pair may join a call that wants distances with one that does not: each writes only its own buffers);
 * out_dist_dev belongs to the library, as out_ids_dev does, until done_event or tk_index_join. */
int tk_index_query_batch_dist(tk_index *ix, const tk_allow *allow, const float *q, const void *q_pq,
                              int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                              int64_t *out_ids, void *out_dist);
int tk_index_query_batch_dev_dist(tk_index *ix, const tk_allow *allow, const float *q_dev,
                                  const void *q_pq_dev, int q_pq_is_f64, int64_t nq, int k, int n_probes,
                                  int pass_1, int64_t *out_ids_dev, void *out_dist_dev, void *done_event,
                                  void *stream);
/* One excluded row per query, and stored rows as queries (k-NN graphs, de-duplication, "more like this row").
 * exclude[i] = e: query i returns what IVF.query (ivf.py:106-163) returns when `insert` in query_pq runs only
 * for labels != e — the allowed set "every row but e", with everything else the reference's as for allowed sets
 * above; bit for bit that guarded reference.  e = -1: nothing excluded for that query.  On the device every stored
 * copy of e in a probed list takes the heap's empty value in the query's distance row, where the allowed set's
 * pass runs (behind the list scans and every exact re-scan, in front of every replay; never on the coarse stage).
 * The copies are found in a row-position table: 4 (N + 2) + 4 T bytes for N rows and T stored entries (plus
 * the allocator's eighth of slack: 0.8 GB at 100M rows stored once, 1.2 GB stored twice), made from the
 * device-resident labels by the first call that passes an exclude array, once per layout of the lists (again after
 * tk_index_set_lists, _add_rows, _remove_rows; that call synchronises the device, so make it outside a stream
 * capture), freed with the index.  Calls without an array never make it.  T and N must be below 2^31.
 * tk_index_query_batch_ex2 / _dev_ex2: tk_index_query_batch / _dev_ex with everything at once; allow, exclude,
 * out_dist and the debug outputs may each be NULL.  The host call checks exclude (an entry outside [-1, N):
 * TK_ERR_ARG, nothing run) and passes an array of only -1 on as none.  The device call does not read exclude_dev
 * on the host: an entry outside [0, N) there excludes nothing.  exclude_dev (int64, nq entries) belongs to the
 * library until done_event or tk_index_join, like the other buffers.  Not for list-sharded indexes.
 * Sub-batches, the pipelined mode and pairs of calls as the _dist call; ANY two calls that could pair without an
 * exclude array still pair with one, on either side (each half reads its own array or none).  An excluding call
 * takes the scan an unrestricted call takes (the automatic plain-scan state counts its verdicts).
 * tk_index_gather_queries_dev: qn_dev[i] = float32(data[rows_dev[i]]) — a copy of float32 vectors, half
 * vectors widened, float64 vectors rounded to nearest even — NOT normalised again, and q_pq_dev as
 * tk_index_prepare_dev makes it from qn_dev (padded; rotated with the device's float64 FMA chain where a rotation
 * is set: float64 iff rotated).  rows_dev: int64 entries in [0, N), the caller's promise.  Enqueued on `stream`.
 * tk_index_gather_queries: the same with host buffers (rows checked), for inspection and tests.
 * tk_index_query_rows: rows on the host in (checked: outside [0, N) is TK_ERR_ARG), gather + _ex2 in library
 * buffers; exclude_self != 0: exclude = rows.  A row that was removed is still a vector: nothing is masked for it.
 * tk_index_row_table: info4 = {table exists for the current lists, its bytes, times one was made, its entries}. */
int tk_index_query_batch_ex2(tk_index *ix, const tk_allow *allow, const int64_t *exclude, const float *q,
                             const void *q_pq, int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                             int64_t *out_ids, void *out_dist, int64_t *out_probes, int64_t *out_heap_idx,
                             int32_t *out_heap_val);
int tk_index_query_batch_dev_ex2(tk_index *ix, const tk_allow *allow, const int64_t *exclude_dev,
                                 const float *q_dev, const void *q_pq_dev, int q_pq_is_f64, int64_t nq, int k,
                                 int n_probes, int pass_1, int64_t *out_ids_dev, void *out_dist_dev,
                                 void *done_event, void *stream);
int tk_index_gather_queries_dev(tk_index *ix, const int64_t *rows_dev, int64_t nq, float *qn_dev,
                                void *q_pq_dev, void *stream);
int tk_index_gather_queries(tk_index *ix, const int64_t *rows, int64_t nq, float *qn, void *q_pq);
int tk_index_query_rows(tk_index *ix, const tk_allow *allow, const int64_t *rows, int64_t nq, int exclude_self,
                        int k, int n_probes, int pass_1, int64_t *out_ids, void *out_dist, int64_t *out_probes,
                        int64_t *out_heap_idx, int32_t *out_heap_val);
int tk_index_row_table(tk_index *ix, int64_t *info4);
/* Every query of a batch restricted to its own group of rows (one tenant, language or category per row).
 * groups[r] in [0, 2^31 - 1) is row r's group.  A query with group g >= 0 returns what IVF.query (ivf.py:106-163)
 * returns when `insert` in query_pq runs only for labels with groups[label] == g — the allowed set "groups == g",
 * for that query alone, with everything else the reference's as for allowed sets above; bit for bit that guarded
 * reference.  g = -1: the query is unrestricted.  A g that no row carries: the query returns no id (a row of -1).
 * With an allowed set and / or an exclude array as well, `insert` runs only for labels that pass all of them.
 * tk_index_set_groups: n == N ids on the host (outside [0, 2^31 - 1): TK_ERR_ARG), uploaded once and kept until
 * they are replaced, cleared (NULL, 0) or the index is destroyed; completes the batches in flight first.
 * tk_index_groups: the number of rows the groups cover, 0 for none.
 * On the device the rows of other groups in a probed list take the heap's empty value in the query's distance row,
 * where the allowed set's pass runs (behind the list scans and every exact re-scan, in front of every replay; never
 * on the coarse stage).  Their groups are read from a table in list-position order, 64 bytes per stored chunk of 16
 * rows beside the 4 N bytes by row id (0.4 GB each at 100M rows stored once, plus the allocator's eighth of slack),
 * made from the device-resident labels by the first call that passes a group array, once per layout of the lists
 * (again after tk_index_set_lists, _add_rows, _remove_rows and after tk_index_set_groups; that call synchronises
 * the device, so make it outside a stream capture), freed with the index.  Calls without an array never make it
 * and launch nothing more than before.
 * tk_index_query_batch_ex3 / _dev_ex3: _ex2 with one more pointer, group / group_dev (int32, nq entries), which may
 * be NULL.  The host call checks group (an entry < -1: TK_ERR_ARG, nothing run) and passes an array of only -1 on as
 * none.  The device call does not read group_dev on the host: an entry < 0 there leaves its query unrestricted.
 * group_dev belongs to the library until done_event or tk_index_join, like the other buffers.
 * Refused, nothing run: a group array while no groups are set, or while they cover fewer rows than the index has
 * (after tk_index_add_rows: TK_ERR_STATE, set them again); a list-sharded index (TK_ERR_ARG).
 * Sub-batches and the pipelined mode as the _ex2 calls.  A call with a group array is a restricted call: in the
 * automatic plain-scan mode it takes the exact scan and leaves the automatic state alone, as a call with an allowed
 * set; two calls pair (tk_index_set_coalesce) only where both pass a group array or neither does.
 * tk_index_group_table: info4 = {table exists for the current lists, its bytes, times one was made, the bytes of
 * the groups by row id}. */
int tk_index_set_groups(tk_index *ix, const int32_t *groups, int64_t n);
int64_t tk_index_groups(tk_index *ix);
int tk_index_query_batch_ex3(tk_index *ix, const tk_allow *allow, const int64_t *exclude, const int32_t *group,
                             const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq, int k, int n_probes,
                             int pass_1, int64_t *out_ids, void *out_dist, int64_t *out_probes,
                             int64_t *out_heap_idx, int32_t *out_heap_val);
int tk_index_query_batch_dev_ex3(tk_index *ix, const tk_allow *allow, const int64_t *exclude_dev,
                                 const int32_t *group_dev, const float *q_dev, const void *q_pq_dev, int q_pq_is_f64,
                                 int64_t nq, int k, int n_probes, int pass_1, int64_t *out_ids_dev,
                                 void *out_dist_dev, void *done_event, void *stream);
int tk_index_group_table(tk_index *ix, int64_t *info4);
/* Every query of a batch restricted to the rows that carry its tags (several categories or ACL principals per row).
 * tags[r] is row r's 64-bit mask: bit t set = the row carries tag t, 64 tags per index, 0 = a row without tags.  A
 * query carries a mask m, the call one mode: tag_mode 0 ("any") — a row passes iff (tags[r] & m) != 0; tag_mode 1
 * ("all") — iff (tags[r] & m) == m; another mode: TK_ERR_ARG.  A query with m != 0 returns what IVF.query
 * (ivf.py:106-163) returns when `insert` in query_pq runs only for labels that pass — that allowed set, for that
 * query alone, with everything else the reference's as for allowed sets above; bit for bit that guarded reference.
 * m == 0: the query is unrestricted in both modes.  No row passes: the query returns no id (a row of -1).  With an
 * allowed set, an exclude array and / or a group array as well, `insert` runs only for labels that pass all of them.
 * tk_index_set_tags: n == N masks on the host, uploaded once and kept until they are replaced, cleared (NULL, 0) or
 * the index is destroyed; completes the batches in flight first.
 * tk_index_tags: the number of rows the tags cover, 0 for none.
 * On the device the probed rows that do not pass take the heap's empty value in the query's distance row, where the
 * group pass runs (behind the list scans and every exact re-scan, in front of every replay; never on the coarse
 * stage).  Their tags are read from a table in list-position order, 128 bytes per stored chunk of 16 rows beside the
 * 8 N bytes by row id (0.8 GB each at 100M rows stored once, plus the allocator's eighth of slack), made from the
 * device-resident labels by the first call that passes a tag array, once per layout of the lists (again after
 * tk_index_set_lists, _add_rows, _remove_rows, _update_rows and after tk_index_set_tags; that call synchronises the
 * device, so make it outside a stream capture), freed with the index.  Calls without an array never make it and
 * launch nothing more than before.
 * tk_index_query_batch_ex4 / _dev_ex4: _ex3 with one more pointer, tags / tags_dev (uint64, nq entries), which may be
 * NULL, and tag_mode.  The host call passes an array of only zeros on as none.  The device call does not read
 * tags_dev on the host: an entry of 0 there leaves its query unrestricted.  tags_dev belongs to the library until
 * done_event or tk_index_join, like the other buffers.  _ex3 is this call without a tag array.
 * Refused, nothing run: a tag array while no tags are set, or while they cover fewer rows than the index has (after
 * tk_index_add_rows: TK_ERR_STATE, set them again); a list-sharded index (TK_ERR_ARG).
 * Sub-batches and the pipelined mode as the _ex3 calls.  A call with a tag array is a restricted call: in the
 * automatic plain-scan mode it takes the exact scan and leaves the automatic state alone; two calls pair
 * (tk_index_set_coalesce) only where both pass a tag array with the same mode or neither passes one.
 * tk_index_tag_table: info4 = {table exists for the current lists, its bytes, times one was made, the bytes of the
 * tags by row id}. */
int tk_index_set_tags(tk_index *ix, const uint64_t *tags, int64_t n);
int64_t tk_index_tags(tk_index *ix);
int tk_index_query_batch_ex4(tk_index *ix, const tk_allow *allow, const int64_t *exclude, const int32_t *group,
                             const uint64_t *tags, int tag_mode, const float *q, const void *q_pq, int q_pq_is_f64,
                             int64_t nq, int k, int n_probes, int pass_1, int64_t *out_ids, void *out_dist,
                             int64_t *out_probes, int64_t *out_heap_idx, int32_t *out_heap_val);
int tk_index_query_batch_dev_ex4(tk_index *ix, const tk_allow *allow, const int64_t *exclude_dev,
                                 const int32_t *group_dev, const uint64_t *tags_dev, int tag_mode, const float *q_dev,
                                 const void *q_pq_dev, int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                                 int64_t *out_ids_dev, void *out_dist_dev, void *done_event, void *stream);
int tk_index_tag_table(tk_index *ix, int64_t *info4);
/* Every query of a batch restricted to the rows whose values lie in its ranges ("newer than t", "price between a and
 * b").  Rows carry `cols` numeric columns, 1 <= cols <= 4, as int64 KEYS; a query carries one inclusive interval
 * [lo_c, hi_c] of keys per column, and a row passes iff lo_c <= key[row, c] <= hi_c for every column c.  The library
 * compares int64 only: a caller maps its values and bounds to keys with a strictly monotone function (integers: the
 * value itself; floats, widened to float64, -0.0 folded into +0.0, no NaN: the bits b where b >= 0, else
 * b ^ 0x7FFFFFFFFFFFFFFF — tinyknn_amd.ivf.value_keys).  An unbounded end is INT64_MIN (lo) / INT64_MAX (hi): the
 * comparison is simply true.  A query with a bounded column returns what IVF.query (ivf.py:106-163) returns when
 * `insert` in query_pq runs only for labels that pass — that allowed set, for that query alone, with everything else
 * the reference's as for allowed sets above; bit for bit that guarded reference.  Every bound unbounded: the query is
 * unrestricted.  lo > hi, or no row passes: the query returns no id (a row of -1).  With an allowed set, an exclude
 * array, a group array and / or a tag array as well, `insert` runs only for labels that pass all of them.
 * tk_index_set_values: keys column-major, (cols, n) with n == N, on the host, uploaded once and kept until they are
 * replaced, cleared (NULL, 0, 0) or the index is destroyed; completes the batches in flight first.  cols outside
 * 1..4: TK_ERR_ARG.
 * tk_index_values: the number of rows the values cover, 0 for none.  tk_index_value_columns: their columns, 0 for none.
 * On the device the probed rows that do not pass take the heap's empty value in the query's distance row, behind the
 * tag pass (behind the list scans and every exact re-scan, in front of every replay; never on the coarse stage).
 * Their keys are read from a table in list-position order, column-major: 128 bytes per stored chunk of 16 rows and
 * column beside the 8 cols N bytes by row id (0.8 GB each per column at 100M rows stored once, plus the allocator's
 * eighth of slack; padding rows hold INT64_MIN), made from the device-resident labels by the first call that passes a
 * range array, once per layout of the lists (again after tk_index_set_lists, _add_rows, _remove_rows, _update_rows and
 * after tk_index_set_values; that call synchronises the device, so make it outside a stream capture), freed with the
 * index.  The pass reads only the columns a query bounds.  Calls without an array never make the table and launch
 * nothing more than before.
 * tk_index_query_batch_ex5 / _dev_ex5: _ex4 with one more pointer, between / between_dev (int64, nq x cols x 2 keys:
 * query-major, then column, then lo, hi), which may be NULL.  The host call passes an array of only unbounded entries
 * on as none (that call takes the unrestricted path).  The device call does not read between_dev on the host: a query
 * whose entries are all unbounded there is unrestricted.  between_dev belongs to the library until done_event or
 * tk_index_join, like the other buffers.  _ex4 is this call without a range array.
 * Refused, nothing run: a range array while no values are set, or while they cover fewer rows than the index has
 * (after tk_index_add_rows: TK_ERR_STATE, set them again); a list-sharded index (TK_ERR_ARG).
 * Sub-batches and the pipelined mode as the _ex4 calls.  A call with a range array is a restricted call: in the
 * automatic plain-scan mode it takes the exact scan and leaves the automatic state alone; two calls pair
 * (tk_index_set_coalesce) only where both pass a range array or neither passes one.
 * tk_index_value_table: info4 = {table exists for the current lists, its bytes, times one was made, the bytes of the
 * keys by row id}. */
int tk_index_set_values(tk_index *ix, const int64_t *keys, int64_t n, int cols);
int64_t tk_index_values(tk_index *ix);
int tk_index_value_columns(tk_index *ix);
int tk_index_query_batch_ex5(tk_index *ix, const tk_allow *allow, const int64_t *exclude, const int32_t *group,
                             const uint64_t *tags, int tag_mode, const int64_t *between, const float *q,
                             const void *q_pq, int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                             int64_t *out_ids, void *out_dist, int64_t *out_probes, int64_t *out_heap_idx,
                             int32_t *out_heap_val);
int tk_index_query_batch_dev_ex5(tk_index *ix, const tk_allow *allow, const int64_t *exclude_dev,
                                 const int32_t *group_dev, const uint64_t *tags_dev, int tag_mode,
                                 const int64_t *between_dev, const float *q_dev, const void *q_pq_dev, int q_pq_is_f64,
                                 int64_t nq, int k, int n_probes, int pass_1, int64_t *out_ids_dev, void *out_dist_dev,
                                 void *done_event, void *stream);
int tk_index_value_table(tk_index *ix, int64_t *info4);
/* At most m rows of any one group among a query's answers ("the 10 nearest DOCUMENTS, not chunks": field collapsing,
 * result diversification).  Groups are the ones tk_index_set_groups stores.  Everything up to the query's candidates is
 * unchanged — probes, scans, restrictions, the heap of R = pass_1 or (n_probes + 1) k + 1 entries — so this extends the
 * last lines of IVF.query, ivf.py:154-163: let c[0 .. nc) be the heap's ids with the -1 entries dropped, in heap order
 * (ivf.py:154-155).  Where nc > k they are ranked by ascending exact squared distance, ties to the lower position in c
 * (what bottom_k returns, ivf.py:160-163); where nc <= k by position (ivf.py:158-159).  That order is walked and a
 * candidate is kept while fewer than m of its group have been kept, until k are kept — equivalently, a candidate is
 * kept iff fewer than m candidates of its group rank before it.  The kept ids are returned in rank order, the row
 * padded with -1 (distances: +inf), every returned id with its exact distance where distances are asked for.  A
 * candidate's group is groups[id], a negative id meaning id + N as where its vector is fetched.
 * per_group / per_group_dev: int32, nq entries, m per query; 0: no cap for that query (it returns what the call without
 * the array returns).  The pool is the heap: with a small m a query can run out of groups before it has k ids — a
 * larger pass_1 or n_probes widens it; nothing is widened here.
 * tk_index_query_batch_ex6 / _dev_ex6: _ex5 with one more pointer, which may be NULL.  The host call checks per_group
 * (an entry < 0: TK_ERR_ARG, nothing run) and passes an array of only zeros on as none.  The device call does not read
 * per_group_dev on the host: an entry <= 0 there leaves its query uncapped.  per_group_dev belongs to the library
 * until done_event or tk_index_join, like the other buffers.  _ex5 is this call without a cap array.
 * Refused, nothing run: a cap array while no groups are set, or while they cover fewer rows than the index has
 * (TK_ERR_STATE, as for a group array); a list-sharded index; a heap whose ranking does not fit the rescoring's 64 KiB
 * of LDS beside the heap (R * 28 + 4 d + 32 bytes, float64 vectors R * 36 + 8 d + 32: TK_ERR_ARG).
 * On the device the final rescoring alone changes: its capped kernels keep every candidate (id, distance, group — one
 * 4-byte read per candidate from the groups by row id) at its rank in LDS and select from there.  The first capped
 * call of a layout makes the group table as a call with a group array does (it synchronises the device).  A cap is not
 * a restriction of the scans: a call with a cap alone takes the scan an unrestricted call takes.  Sub-batches and the
 * pipelined mode as the _ex5 calls; two calls pair (tk_index_set_coalesce) only where both pass a cap array or neither
 * does, and a call's answers do not depend on pipeline depth, pairing or sub-batching. */
int tk_index_query_batch_ex6(tk_index *ix, const tk_allow *allow, const int64_t *exclude, const int32_t *group,
                             const uint64_t *tags, int tag_mode, const int64_t *between, const int32_t *per_group,
                             const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq, int k, int n_probes,
                             int pass_1, int64_t *out_ids, void *out_dist, int64_t *out_probes, int64_t *out_heap_idx,
                             int32_t *out_heap_val);
int tk_index_query_batch_dev_ex6(tk_index *ix, const tk_allow *allow, const int64_t *exclude_dev,
                                 const int32_t *group_dev, const uint64_t *tags_dev, int tag_mode,
                                 const int64_t *between_dev, const int32_t *per_group_dev, const float *q_dev,
                                 const void *q_pq_dev, int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                                 int64_t *out_ids_dev, void *out_dist_dev, void *done_event, void *stream);
/* hipStream_t on which to copy a batch's inputs in (pipelined mode: the index's front stream,
 * where the batch's first kernel runs; NULL: use the stream the batch is enqueued on) */
void *tk_index_input_stream(tk_index *ix);
int tk_index_pending(tk_index *ix);
/* info8 = {d, dq, M, n_lists, rotation d_pad (0: none), pipeline depth, N, total chunks} */
int tk_index_info(tk_index *ix, int64_t *info8);

/* Streaming session: IVF.query for a stream of batches, raw float32 queries on the host in,
 * ids on the host out (ivf.py:106-163 per row).  submit = exact host preparation on the
 * pool (above) into page-locked staging, H2D on a copy stream, the device pipeline on a
 * compute stream, D2H of the ids behind the last kernel; it returns a ticket at once, so
 * that the preparation and the copies of a batch overlap the kernels of the batches before
 * it.  out_ids (nq, k) is written by tk_stream_wait(ticket) / tk_stream_drain (or by a later
 * submit that reuses the slot: n_slots batches may be outstanding) and must stay valid
 * until then.  R / d_pad as in tk_prepare_queries_host (NULL: unrotated PQ).
 * tk_stream_submit_prepared: the same from already prepared rows (qn, q_pq as
 * tk_index_query_batch takes them).  A session owns its index while batches are
 * outstanding; one thread at a time. */
typedef struct tk_stream tk_stream;
tk_stream *tk_stream_create(tk_index *ix, int64_t max_nq, int k, int n_probes, int pass_1,
                            int angular, const double *R, int d_pad, int n_slots);
int64_t tk_stream_submit(tk_stream *s, const float *q_raw, int64_t nq, int64_t *out_ids);
int64_t tk_stream_submit_prepared(tk_stream *s, const float *qn, const void *q_pq, int64_t nq,
                                  int64_t *out_ids);
/* n_probes / pass_1 of the submits that follow (drains the session first; its staging buffers
 * are kept, so that a sweep over n_probes does not re-allocate page-locked memory) */
int tk_stream_set_probes(tk_stream *s, int n_probes, int pass_1);
int tk_stream_wait(tk_stream *s, int64_t ticket);
int tk_stream_drain(tk_stream *s);
double tk_stream_prepare_seconds(tk_stream *s);
void tk_stream_destroy(tk_stream *s);

/* ---- exact k nearest vectors: the ground truth of recall --------------
 * knn_brute(q, IVF.data, k, "euclidean") (utils.py:66-86, as examples/bench.py:85 uses it) on
 * the f32 matrix cores: part = (|q|^2 + |y|^2) - (2q).y with numpy's einsum norms and the
 * GEMM as the f32 FMA chain (v_mfma_f32_32x32x2_f32) — numpy's part values bit for bit — and
 * the k smallest in ascending (part, row) order (numpy's argpartition leaves the order of
 * the first k, and the choice among exact ties at the k-th value, unspecified).
 * q: (nq, d) float32 host, already normalised for the angular metric like IVF.data;
 * out_ids: (nq, k) int64 host.  float32 vectors, d <= 128, 1 <= k <= min(1024, N), N < 2^31.
 * The rows are scanned in segments whose length follows from k (2^20 rows for k <= 16, 2^17 for
 * k = 100, 2^14 for k = 1024; the rule is in brute.hip), each adding to a list of 8192 candidates
 * per query.  Refused (TK_ERR_HIP, "candidate list overflow", no ids written): a query for which
 * one segment holds more than 8192 rows within its running k-th distance, i.e. rows tied at
 * that distance (thousands of duplicates) or near rows stored together so densely that one
 * segment holds more than 4 times its share of them.  A list is never cut silently. */
int tk_index_knn_brute(tk_index *ix, const float *q, int64_t nq, int k, int64_t *out_ids);
/* The same under the restrictions of the query calls: the k rows with the smallest (part, row) among the rows j in
 * [0, N) that pass every condition given (host arrays, NULL: not given):
 *   allowed_mask (N,) uint8 by ROW ID (not an allowed set, which is laid out by list position): allowed_mask[j] != 0
 *   exclude (nq,)   j != exclude[i]; -1 excludes nothing
 *   group (nq,)     group[i] < 0, or the row's group (tk_index_set_groups) == group[i]
 *   tags (nq,)      tags[i] == 0, or with the row's mask m (tk_index_set_tags) tag_mode 0: (m & tags[i]) != 0,
 *                   1: (m & tags[i]) == tags[i]
 *   between (nq, C, 2)  lo <= key <= hi on each of the C columns of tk_index_set_values (int64 keys, both inclusive)
 * Fewer than k passing rows: the row of out_ids ends in -1.  out_dist (or NULL): (nq, k) float32, the `part` value
 * beside each id (numpy's knn_brute value, which rounding can make slightly negative — not the knn_brute1 distance
 * the query calls' _dist entry points return), +inf beside -1.
 * The predicate is applied inside the tile kernel before a row is appended, and the first tau is taken over the
 * sample rows that pass (+inf below k of them).  A candidate list that overflows under the segment rule is not an
 * error here: the selection is repeated once with segments of the largest multiple of 32 not above 8192 - k rows,
 * which cannot overflow.  TK_ERR_STATE with the query calls' texts where group / tags / between is given and the
 * index has no such values for all N rows; only the arrays by row id are read — no list-order table is made.
 * Not for a list-sharded index; float32 vectors, d, k and N as above. */
int tk_index_knn_brute_ex(tk_index *ix, const float *q, int64_t nq, int k, const uint8_t *allowed_mask,
                          const int64_t *exclude, const int32_t *group, const uint64_t *tags, int tag_mode,
                          const int64_t *between, int64_t *out_ids, float *out_dist);
/* Every row within a radius of each query, exactly (radius.hip): row j is a hit of query i iff it passes
 * the query's restrictions — allowed_mask / exclude / group / tags, tag_mode / between exactly as
 * tk_index_knn_brute_ex takes them, host arrays, NULL: not given — and part(i, j) <= radius[i], compared in float32,
 * inclusive; part is the value that call reports in out_dist, bit for bit (the two share the tile loop), so for every
 * k its ids are the first k entries of this call's list at radius = its k-th part value.  q: (nq, d) prepared
 * queries; radius: (nq) float32, +inf (every passing row) and negative values (normally no row) allowed, NaN refused.
 * The result is CSR: out_lims (nq + 1) int64 with out_lims[0] = 0, query i's hits at [out_lims[i], out_lims[i + 1]),
 * *out_total = out_lims[nq].  Both are written before the total is compared with max_results (< 2^31): a total
 * above it is TK_ERR_ARG with the total in the text, and no result is held — a list is never cut.  count_only: the
 * count pass alone (max_results is not looked at, nothing is held; nq x N may exceed 2^31, the sums are int64).
 * Otherwise the decoded result stays on the device, in buffers of the index, until the next call of this function on
 * the index or its destruction; tk_index_radius_fetch copies it out: out_ids (total) int64 and out_dist (total, or
 * NULL) float32 part values.  sorted != 0: every list ascending by (part, id) — knn_brute's order, the same bytes
 * from run to run; 0: the order inside a list is unspecified (the sort is skipped).  tk_index_radius_fetch with no
 * result held: TK_ERR_STATE.  Two passes over all N rows on the f32 matrix cores plus a segmented radix sort; the
 * counts cross to the host between the passes (one synchronisation).  The vectors of removed rows stay in HBM, as for
 * tk_index_knn_brute: allowed_mask with the surviving rows is the truth after a removal.
 * Float32 vectors, d <= 128, N < 2^31; not for a list-sharded index; TK_ERR_STATE with the query calls' texts where
 * group / tags / between is given and the index has no such values for all N rows.  Synchronous. */
int tk_index_radius_brute(tk_index *ix, const float *q, int64_t nq, const float *radius, const uint8_t *allowed_mask,
                          const int64_t *exclude, const int32_t *group, const uint64_t *tags, int tag_mode,
                          const int64_t *between, int sorted, int count_only, int64_t max_results, int64_t *out_lims,
                          int64_t *out_total);
int tk_index_radius_fetch(tk_index *ix, int64_t *out_ids, float *out_dist);
/* Every row within a radius of each query among the rows of the lists the query probes (radius_probe.hip, DESIGN
 * 3.20): FAISS's range_search on an IVF index.  For query i with n_probes = P >= 1:
 *   probes      the index's own coarse stage for P — the row tk_index_top_centers(k = P) gives and the query calls
 *               probe; it depends on P alone (kc = min(P, n_lists), coarse rescore 2 kc + 10), on no k.  q: (nq, d)
 *               prepared queries, q_pq: (nq, dq) float32, or float64 where q_pq_is_f64, as the query calls take them.
 *   lists       the distinct lists that row names; a -1 left by an unfilled coarse heap names the last list, as the
 *               reference's negative index does; a list named twice is walked once.
 *   candidates  the labels in [0, N) stored in those lists at positions < list_n.  Rows that tk_index_remove_rows took
 *               out are therefore never candidates (tk_index_radius_brute needs allowed_mask for that).  A row stored
 *               in several probed lists is a candidate once.
 *   hits        candidate j is a hit iff it passes the query's restrictions — allowed_mask / exclude / group / tags,
 *               tag_mode / between exactly as tk_index_radius_brute takes them — and dist(i, j) <= radius[i],
 *               inclusive: dist is the rescoring's squared distance (sqdist_row.h), float32 on float32 and half
 *               stores, float64 on float64 vectors (compared with (double)radius[i]) — the values the query calls
 *               return as distances and tk_index_knn_group returns, bit for bit.  It is NOT tk_index_radius_brute's
 *               `part`: the two round differently and agree exactly on integer data.
 * radius, out_lims, *out_total, max_results, count_only, sorted: as tk_index_radius_brute's; sorted lists ascend by
 * (dist, id), the same bytes from run to run; max_results is compared with the final total (every row once).  The
 * decoded result is held on the device until the next radius call of either kind on the index (tk_index_radius_brute
 * drops it too, and this call drops that one's) or its destruction; tk_index_radius_probe_fetch copies it out:
 * out_ids (total) int64, out_dist (total, or NULL) float32 — float64 on float64 vectors.  With nothing held:
 * TK_ERR_STATE.
 * The count pass leaves one bit per candidate, the fill pass reads it: sum over the query's distinct probed lists of
 * ceil(list_n / 64) 64-bit words.  A call whose bitmap would exceed the workspace budget (16 GB, TINYKNN_WORKSPACE_GB)
 * is TK_ERR_WORKSPACE before either pass runs: ask fewer queries per call.  The coarse stage synchronises per chunk of
 * queries, as tk_index_top_centers does; after it the word total and the counts cross to the host.
 * Every vector store, d <= 4096, N < 2^31, nq * min(P, n_lists) < 2^31.  Refused before any device work: a
 * list-sharded index, n_probes < 1, a NaN radius (TK_ERR_ARG); group / tags / between without their row values for
 * all N rows, and an index whose labels repeat and for which no twin table can be made — a row stored in two probed
 * lists could not be listed once (TK_ERR_STATE): a label stored more than 17 times, copies of a label with different
 * codes or in one list, repeating labels beyond int32, no free memory for the table.  An index that keeps no table only
 * because its labels are sparse (tk_index_twin_table: width 0 after tk_index_remove_rows thinned it) gets one made by
 * the first such call of a layout, kept until the lists change.  Synchronous, under the index lock, after the calls
 * still owed. */
int tk_index_radius_probe(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq, int n_probes,
                          const float *radius, const uint8_t *allowed_mask, const int64_t *exclude,
                          const int32_t *group, const uint64_t *tags, int tag_mode, const int64_t *between, int sorted,
                          int count_only, int64_t max_results, int64_t *out_lims, int64_t *out_total);
int tk_index_radius_probe_fetch(tk_index *ix, int64_t *out_ids, void *out_dist);
/* The exact k nearest rows inside each query's own group (group_exact.hip): what the restricted call
 * above answers for group[i] >= 0 among the rows that are STORED, at a cost that follows the size of the group instead
 * of N — a query reads the rows of its group and no other.  Ranked by the rescoring's distance (numpy's einsum order
 * bit for bit, the value the query calls' _dist entry points return), so ids and distances mix freely with theirs:
 * the k smallest (distance, row id) among the rows j with
 *   group (nq,)     REQUIRED: the row's group (tk_index_set_groups) == group[i]; every entry >= 0, else TK_ERR_ARG and
 *                   nothing is run.  An id no row carries: a row of -1.
 *   stored          some list holds label j: rows taken out by tk_index_remove_rows never come back (their vectors
 *                   stay in HBM), so the call answers what the index would answer
 *   allowed_mask / exclude / tags, tag_mode / between   as above (host arrays, NULL: not given)
 * Fewer than k such rows: the row of out_ids ends in -1.  out_dist (or NULL): (nq, k) squared distances beside the
 * ids, float32 — float64 on an index of float64 vectors, as numpy promotes — and +inf beside -1.  All three vector
 * stores (float32, half, float64); 1 <= k <= min(1024, N); N < 2^31.
 * One workgroup per query walks the group's rows, so a group of any size is answered — the whole index in one group
 * included — but a large one slowly: tk_index_knn_brute_ex(group) is the call there.
 * Two tables are made by the first call that needs them (each synchronises the device: not inside a stream capture):
 * the row ids gathered by group id (a radix sort on the device; 4 N + 8 G + 4 bytes for G distinct groups, about 20 N
 * bytes of work memory while it is made), made again after tk_index_set_groups and by nothing else; and an N-bit map of
 * the stored rows, made again after the lists changed.  Calls that do not ask for them never make them.
 * TK_ERR_STATE with the query calls' texts where the groups (or, given tags / between, the tags / values) do not
 * cover all N rows.  Synchronous; not for a list-sharded index.
 * tk_index_group_sizes: out[i] = the number of rows that carry group[i] (host arrays of n entries), 0 for an id no
 * row carries — counted over all N rows, the removed ones too.  It makes the first table where it is missing.
 * tk_index_group_rows: info4 = {that table exists for the current groups, its bytes, times one was made, distinct
 * group ids}. */
int tk_index_knn_group(tk_index *ix, const float *q, int64_t nq, int k, const int32_t *group,
                       const uint8_t *allowed_mask, const int64_t *exclude, const uint64_t *tags, int tag_mode,
                       const int64_t *between, int64_t *out_ids, void *out_dist);
int tk_index_group_sizes(tk_index *ix, const int32_t *group, int64_t n, int64_t *out);
int tk_index_group_rows(tk_index *ix, int64_t *info4);
/* The exact k nearest rows inside each query's value range (value_exact.hip): what tk_index_knn_brute_ex
 * answers under `between` among the rows that are STORED, at a cost that follows the number of rows ONE column of the
 * range admits instead of N.  A range over one column is a contiguous span of the rows sorted by that column; query i
 * walks the shortest such span among the columns it bounds (ties: the lowest column) and tests every condition given
 * on each row of it, by row id — the formulas of the restricted call above.  Ranked as tk_index_knn_group ranks: the k
 * smallest (rescoring distance, row id), the same bits as that call's and the query calls' distances.
 *   between (nq, C, 2)  REQUIRED: inclusive int64 keys (lo, hi) per value column, INT64_MIN / INT64_MAX for an end that
 *                   is not bounded.  A query that bounds no column: TK_ERR_ARG and nothing is run (an unrestricted
 *                   query is tk_index_knn_brute's or tk_index_query_batch's to answer).  lo > hi: a row of -1.
 *   allowed_mask / exclude / group (-1: any) / tags, tag_mode   as above (host arrays, NULL: not given)
 * Outputs, stores, k, N, d as tk_index_knn_group.  One workgroup per query walks the span, so a wide range is
 * answered slowly: tk_index_knn_brute_ex(between) is the call there.
 * Two tables are made by the first call that needs them (each synchronises the device: not inside a stream capture):
 * per value column the row ids ascending by (key, row id) — a radix sort on the device over all 64 key bits; 4 N bytes
 * per column stay, about 24 N bytes of work memory while it is made — made again after tk_index_set_values and by
 * nothing else; and tk_index_knn_group's N-bit map of the stored rows.  Calls that do not ask for them never make them.
 * TK_ERR_STATE with the query calls' texts where the values (or, given group / tags, the groups / tags) do not cover
 * all N rows.  Synchronous; not for a list-sharded index.
 * tk_index_range_sizes: for n queries' ranges (host, (n, C, 2)) out_len[i] = the length of the span query i would
 * walk and out_col[i] its column: (N, -1) for a query that bounds no column, 0 for an empty interval.  Counted over all
 * N rows, the removed ones too — what the walk costs, and an upper bound on the rows that pass.  It makes the first
 * table where it is missing.
 * tk_index_value_rows: info4 = {that table exists for the current values, its bytes, times one was made, columns}. */
int tk_index_knn_between(tk_index *ix, const float *q, int64_t nq, int k, const int64_t *between,
                         const uint8_t *allowed_mask, const int64_t *exclude, const int32_t *group,
                         const uint64_t *tags, int tag_mode, int64_t *out_ids, void *out_dist);
int tk_index_range_sizes(tk_index *ix, const int64_t *between, int64_t n, int64_t *out_len, int32_t *out_col);
int tk_index_value_rows(tk_index *ix, int64_t *info4);

/* ---- list-sharded index over `world` ranks, one process per GPU --------
 * The inverted lists (ivf.py:100-102) are partitioned by cluster id: owner[l] is the rank
 * that stores list l's packed codes.  PQ, coarse centres, ids and the rescoring vectors are
 * replicated (set_pq / set_centers / set_data as usual), so every rank derives the same
 * probe order without communication.  tk_index_set_lists_shard replaces tk_index_set_lists:
 * list_sizes and ids describe ALL lists, codes_owned only the lists with owner[l] == rank,
 * concatenated in list order.
 *
 * The reference chains all probed lists of a query through ONE order-dependent heap
 * (ivf.py:137-150), so partial top-k's do not merge; the exchange carries the int8 distance
 * bytes to the query's home rank (query i lives on rank i / ceil(nq/world)), which replays
 * the heap exactly as the unsharded index does.  One batch =
 *   tk_index_shard_coarse_dev  distance tables for all nq queries, then the coarse stage
 *                              (dtable.top(centers), ivf.py:131) of this rank's HOME queries
 *                              only; probes_home_dev: int64 (ceil(nq/world), min(n_probes,
 *                              n_lists)), rows past nq = 0;
 *   all-gather of the probes   -> probes_all (world * ceil(nq/world), ...) = the probe lists
 *                              of all queries in query order (RCCL, by the caller);
 *   tk_index_shard_scan_dev    the owned (query, list) segments scored straight into
 *                              `send_dev`: `world` regions of `capacity` uint4 (16 distances
 *                              each), region h = my segments of rank h's queries, in (query,
 *                              probe slot) order; *flag_dev |= 1 if a region overflowed
 *                              (repeat the batch with a larger capacity).  probes_all_dev ==
 *                              NULL: the replicated form — this call builds the tables and
 *                              runs the coarse stage for ALL queries itself (no coarse call,
 *                              no probe all-gather; 1/3 of a batch's work is then not
 *                              divided by `world`);
 *   all-to-all(send -> recv)   equal splits of capacity*16 bytes (RCCL, by the caller);
 *   tk_index_shard_finish_dev  received segments -> distance rows of the home queries,
 *                              heap replay, rescoring; out_ids_home_dev: int64
 *                              (ceil(nq/world), k), rows past nq and missing ids = -1; flag_dev:
 *                              the batch's flag word (may be NULL behind tk_index_shard_scan_dev /
 *                              the two-phase scan; required behind tk_index_shard_scan_plain_dev,
 *                              which may raise bit 4 in it, see there);
 *   all-gather of the id rows  (by the caller).
 * All calls enqueue on `stream` and use workspace `slot` (< pipeline depth), so that
 * several batches can be in flight on different streams.  nq <= 131072 per batch. */
int tk_index_set_lists_shard(tk_index *ix, const int64_t *list_sizes, const int32_t *owner,
                             int rank, int world, const uint64_t *codes_owned,
                             const int64_t *ids);
/* a complete unsharded index (host upload or tk_index_build_dev) -> this rank's shard, in place:
 * the codes of the lists with owner[l] == rank are compacted on the device, the rest is dropped */
int tk_index_shard_resident(tk_index *ix, const int32_t *owner, int rank, int world);
int tk_index_shard_coarse_dev(tk_index *ix, int slot, const float *q_dev, const void *q_pq_dev,
                              int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                              int64_t *probes_home_dev, void *stream);
int tk_index_shard_scan_dev(tk_index *ix, int slot, const float *q_dev, const void *q_pq_dev,
                            int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                            const int64_t *probes_all_dev, int64_t capacity, void *send_dev,
                            int *flag_dev, void *stream);
int tk_index_shard_finish_dev(tk_index *ix, int slot, const float *q_dev, int64_t nq, int k,
                              int n_probes, int pass_1, int64_t capacity, const void *recv_dev,
                              int64_t *out_ids_home_dev, int *flag_dev, void *stream);
/* tk_index_shard_scan_dev in the form the unsharded pipeline scans (ivf.py:137-150 through
 * _fast_pq_256.pyx:73-156): of every owned segment only the rows a query scans first — the head of
 * its first probed list, two heap sizes — go through the exact kernel, everything else is scored as
 * plain sums on the int8 matrix cores, and the REPLAY at the query's home rank checks the condition
 * under which those are the reference's values (its bound at the first plain block <= the limit C of
 * the query's table; tk_index_set_plain_scan).  One kernel chain, no extra collective.  A home query
 * that fails the check raises bit 4 of *flag_dev in tk_index_shard_finish_dev (the codes to scan it
 * again exactly are on other ranks): the flag word travels with the ids, every rank sees it, and
 * the batch is repeated behind tk_index_shard_scan_head_dev (below).  Arguments as
 * tk_index_shard_scan_dev + bound_dev (NULL here); falls back to tk_index_shard_scan_dev by itself
 * where the form does not apply (tk_index_shard_plain says 0, heaps beyond the lane replay, world *
 * capacity shorter than the longest list, labels that repeat WITHOUT a twin table).  Labels that repeat
 * (IVF.build(n_probes >= 2)) take this form through the lane replay's TWIN test where the index holds
 * the twin table (tk_index_twin_table: width > 0) and its premises are verified — on a rank that was
 * handed only its own lists' codes (tk_index_set_lists_shard) the device cannot check them: the host
 * wrapper checks over all lists and vouches (tk_index_set_option TK_OPT_TWIN_VOUCH).
 *
 * The same with ONE byte per query exchanged first — for data on which the optimistic form fails (one
 * query in 20 000 of the 100M x 128 index; a sharded batch holds 120 000):
 *   tk_index_shard_scan_head_dev   tables / probe lists / segment positions as tk_index_shard_scan_dev;
 *                                  the HEAD of every first probed list this rank owns — its first
 *                                  ceil(2 R / 16) chunks, R the heap size; ceil(4 R / 16) where labels
 *                                  repeat — scored exactly into send_dev; bound_dev[nq] = the bound
 *                                  after it (order key, as tk_index_shard_bound_dev; 255 elsewhere).
 *                                  Where the one-phase form does not apply (see above) this call IS
 *                                  tk_index_shard_scan_dev, bound_dev is 255 for every query and the
 *                                  plain call behind it does nothing;
 *   all-reduce(MIN, uint8)         by the caller;
 *   tk_index_shard_scan_plain_dev(bound_dev)
 *                                  the one-phase scan, with every query whose bound is above its table's
 *                                  limit kept on the exact kernel: the check at home cannot fail.  (The
 *                                  call writes "never" over those queries' limits in the slot: a scan
 *                                  form run behind it on the same slot needs the batch's tables and
 *                                  limits anew — tk_index_shard_coarse_dev, or a replicated scan call.)
 * Against tk_index_shard_scan_first_dev / _rest_dev, phase 1 scores ~14 chunks per query instead of a
 * whole list, and replays as many. */
int tk_index_shard_scan_plain_dev(tk_index *ix, int slot, const float *q_dev, const void *q_pq_dev,
                                  int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                                  const int64_t *probes_all_dev, int64_t capacity, void *send_dev,
                                  int *flag_dev, const uint8_t *bound_dev, void *stream);
int tk_index_shard_scan_head_dev(tk_index *ix, int slot, const float *q_dev, const void *q_pq_dev,
                                 int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                                 const int64_t *probes_all_dev, int64_t capacity, void *send_dev,
                                 int *flag_dev, uint8_t *bound_dev, void *stream);
/* The library's process-wide internal streams (one set per device): role 0 = the front stream (high
 * priority: table builds, coarse stages), role 1 = replay stream i (0 <= i < 8).  For hosts that run a
 * stage pipeline of their own over the list-sharded entry points — which only enqueue on the stream
 * they are given — without creating streams that would share HIP's four hardware queues with these.
 * NULL on error.  Never destroy them. */
void *tk_shared_stream(int role, int i);
/* Another rank's shard of a complete UNSHARDED index on the same device: a new handle that borrows
 * the source's replicated arrays (PQ, centres, list tables, ids, vectors — the source must outlive
 * it and must not be re-populated meanwhile) and owns only the codes of the lists with
 * owner[l] == rank, compacted on the device.  The source stays usable and unsharded.  This is how
 * several ranks of a list partition are played on ONE GPU (tests, bench.py's one-rank share of a
 * W = 8 partition): a 100M x 128 index holds its 51 GB of vectors once, not once per rank. */
tk_index *tk_index_clone_shard(tk_index *src, const int32_t *owner, int rank, int world);

/* Longest (source -> home) stream of the slot's last tk_index_shard_scan_dev in uint4, fitted or
 * not, among the streams THIS rank sends or receives: max-reduce it over the ranks and size `capacity` by it (the regions of the dense exchange
 * travel whole).  Synchronises with the device. */
int tk_index_shard_usage(tk_index *ix, int slot, int64_t *max_stream_uint4);

/* Filtered exchange — the same batch with a fraction of the bytes on
 * the links.  Every insert of a 16-code block is below the bound captured at the block's start
 * (_fast_pq_256.pyx:73,111-123), so the bound never increases from block to block: a distance
 * that is not below B1, the bound after the query's FIRST probed list, can never enter the
 * heap.  After tk_index_shard_scan_dev (whose buffer then stays on the rank: `scan_dev`):
 *   tk_index_shard_bound_dev   bound_dev[nq] bytes: B1 (order key = distance byte ^ 0x80) of
 *                              the queries whose first probed list this rank owns — replayed
 *                              from the fresh heap over that list — and 255 elsewhere
 *                              (computed from the heap's VALUES alone, which is exact as long
 *                              as the ids inside one list are distinct: a row joins a list
 *                              once, ivf.py:85-102, utils.py:131-150);
 *   all-reduce(MIN, uint8)     -> B1 of every query on every rank (by the caller);
 *   tk_index_shard_filter_dev  the blocks that travel — all of a query's first list, of the
 *                              later lists those whose minimum is below B1 — as records of 5
 *                              int32 {row * cap + block (in the home rank's distance rows), 16
 *                              distance bytes}, grouped by home rank in records_dev (room for
 *                              world * capacity records); counts_dev: 3 * world int32,
 *                              [0, world) = records per home rank, [2 world, 3 world) = all
 *                              blocks this rank scored per home rank (what the dense exchange
 *                              carries), the middle third is scratch;
 *   all-to-all of the counts, then of the records with those splits (by the caller);
 *   tk_index_shard_finish_filtered_dev
 *                              home rows filled with the largest value — a block that did not
 *                              travel then behaves like the real one: no byte of it is below
 *                              any bound — received blocks dropped in, replay, rescoring as
 *                              tk_index_shard_finish_dev; *flag_dev |= 2 on a record that does
 *                              not belong to this rank's rows (never written).
 * Same slot, nq, k, n_probes, pass_1 and capacity as the scan call; the probe lists handed to
 * it must still be alive.  Results are identical to the dense exchange. */
int tk_index_shard_bound_dev(tk_index *ix, int slot, int64_t nq, int k, int n_probes, int pass_1,
                             int64_t capacity, const void *scan_dev, uint8_t *bound_dev,
                             void *stream);
/* ... and WITHOUT a host synchronisation (region_records >= 1; 0 = the compact form above, flag_dev / acc_dev
 * may then be NULL): the records of home rank h go to records_dev[h * region_records, ...) (room for world *
 * region_records records of 5 int32), so the all-to-all of the records has equal splits and can be enqueued
 * before any count is known; the counts (counts_dev[0, world)) travel in their own equal-split all-to-all and
 * are read by the home rank ON THE DEVICE: tk_index_shard_finish_filtered_dev with counts_recv_dev[world] takes
 * the received regions (region s from source rank s; n_records is then ignored), with counts_recv_dev == NULL
 * n_records compact records.  A home rank's records beyond region_records are dropped and *flag_dev |= 1 — the
 * batch's overflow flag, handled like a `capacity` overflow (region_records = capacity can never overflow;
 * callers trim it to what the batches need, multi_gpu.py).  Wire bytes: world * region_records * 20 per rank
 * instead of the exact 20 * records.  acc_dev (or NULL): int64[3] kept by the caller across batches, updated
 * atomically — [0] largest per-home count seen (what the regions must hold), [1] += records, [2] += blocks
 * scored.  (Until round 6 the two forms were four entry points: ..._filter_regions_dev / ..._finish_regions_dev.) */
int tk_index_shard_filter_dev(tk_index *ix, int slot, int64_t nq, int k, int n_probes, int pass_1,
                              int64_t capacity, const void *scan_dev, const uint8_t *bound_dev,
                              int32_t *counts_dev, int32_t *records_dev, int64_t region_records,
                              int *flag_dev, int64_t *acc_dev, void *stream);
int tk_index_shard_finish_filtered_dev(tk_index *ix, int slot, const float *q_dev, int64_t nq,
                                       int k, int n_probes, int pass_1, const int32_t *records_dev,
                                       int64_t n_records, const int32_t *counts_recv_dev,
                                       int64_t region_records, int64_t *out_ids_home_dev, int *flag_dev,
                                       void *stream);
/* The sharded scan in two phases, the second on the int8 matrix cores (tk_index_set_plain_scan's
 * kernel).  The plain sums are the reference's values for a query from the point where its heap's
 * bound is at most the limit C of its table, and B1 — the bound after the query's FIRST probed list
 * (ivf.py:137-152 over that list alone) — is known to every rank before the rest is scanned:
 *   tk_index_shard_scan_first_dev  as tk_index_shard_scan_dev up to the segment positions; the
 *                                  FIRST slots this rank owns scored exactly into send_dev;
 *                                  bound_dev[nq] = B1 (order key, as tk_index_shard_bound_dev) of
 *                                  the queries whose first list this rank owns, 255 elsewhere;
 *   all-reduce(MIN, uint8)         by the caller;
 *   tk_index_shard_scan_rest_dev   the slots behind the first: queries with B1 <= C on the plain
 *                                  kernel, the others on the exact one — as are the queries whose
 *                                  probe list wrapped (a -1 of the coarse heap names the last list)
 *                                  and, where world * capacity is shorter than the longest list,
 *                                  all of them (the plain kernel scores a segment that overflowed
 *                                  its region to the buffer's tail).  The plain kernel's bytes are
 *                                  clamp(plain sum of the signed table, -128, 127), padding rows of
 *                                  a list's last chunk included; both kernels write the 16-byte
 *                                  blocks of this rank's own segments and nothing else unless a
 *                                  region overflowed.  No query is scanned twice,
 *                                  nothing is repaired afterwards; tk_index_shard_finish_dev / the
 *                                  filtered exchange (with this bound: no tk_index_shard_bound_dev)
 *                                  follow as after tk_index_shard_scan_dev and return the same ids.
 * tk_index_shard_plain: 1 if the two-phase form applies to (k, n_probes, pass_1) — M <= 52,
 * n_probes >= 2, distinct labels or labels that repeat under a (verified or vouched) twin table, or
 * tk_index_set_plain_scan(ix, 2); not switched off; replicated
 * state only, so every rank answers alike — else 0 (use tk_index_shard_scan_dev), < 0 on error. */
int tk_index_shard_plain(tk_index *ix, int k, int n_probes, int pass_1);
int tk_index_shard_scan_first_dev(tk_index *ix, int slot, const float *q_dev, const void *q_pq_dev,
                                  int q_pq_is_f64, int64_t nq, int k, int n_probes, int pass_1,
                                  const int64_t *probes_all_dev, int64_t capacity, void *send_dev,
                                  int *flag_dev, uint8_t *bound_dev, void *stream);
int tk_index_shard_scan_rest_dev(tk_index *ix, int slot, int64_t nq, int k, int n_probes, int pass_1,
                                 int64_t capacity, void *send_dev, const uint8_t *bound_dev,
                                 void *stream);
/* Books of the slot's last tk_index_shard_scan_rest_dev (synchronises): out4 = pairs this rank
 * scored on the plain kernel, tiles of 32 of them, exact pair records of the slots behind the
 * first, queries (of all nq) whose bound let them go the plain way. */
int tk_index_shard_plain_stats(tk_index *ix, int slot, int64_t *out4);

#ifdef __cplusplus
}
#endif
#endif
