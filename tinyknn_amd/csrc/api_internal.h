// api_internal.h — what the translation units of the C ABI share (api.hip: host-pointer entry points and
// resident code arrays; api_index.hip: the resident index and its pipeline; api_shard.hip: the list-sharded
// entry points; api_build.hip: device build, raw queries, brute force, FlatTop).  Not part of the ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/tinyknn_hip.h"
#include "kernels.h"

int tk_fail(int code, const std::string &msg);      // sets tk_last_error() of this thread, returns code
static inline int fail(int code, const std::string &msg) { return tk_fail(code, msg); }

#define HIPCHECK(x)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) {                                                              \
            char b_[512];                                                                    \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_),      \
                     __FILE__, __LINE__);                                                    \
            return fail(TK_ERR_HIP, b_);                                                     \
        }                                                                                    \
    } while (0)

#define ARGCHECK(cond, msg)                                                                  \
    do {                                                                                     \
        if (!(cond)) return fail(TK_ERR_ARG, std::string("bad argument: ") + msg);           \
    } while (0)

int tk_require_gpu();     // TK_OK, or the "no HIP device: no CPU fallback" error
static inline int require_gpu() { return tk_require_gpu(); }

// growable device buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool borrowed = false;      // memory of another index (tk_index_clone_shard): never freed or grown here
    void borrow(const DevBuf &o)
    {
        release();
        p = o.p;
        cap = o.cap;
        borrowed = p != nullptr;
    }
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return TK_OK;
        if (borrowed) return fail(TK_ERR_ARG, "bad argument: a borrowed array of a cloned shard cannot grow");
        if (p) HIPCHECK(hipFree(p));
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        HIPCHECK(hipMalloc(&p, want));
        cap = want;
        return TK_OK;
    }
    void release()
    {
        if (p && !borrowed) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        borrowed = false;
    }
    template <typename T>
    T *as() const { return (T *)p; }
};

#define TRY(x)                         \
    do {                               \
        int r_ = (x);                  \
        if (r_ != TK_OK) return r_;    \
    } while (0)

#define TK_DBG_SYNC(tag)                                                                       \
    do {                                                                                       \
        static const int on_ = getenv("TINYKNN_DEBUG_SYNC") ? 1 : 0;                           \
        if (on_) {                                                                             \
            fprintf(stderr, "[dbg] %s ...", tag);                                              \
            fflush(stderr);                                                                    \
            hipError_t e_ = hipDeviceSynchronize();                                            \
            fprintf(stderr, " %s\n", hipGetErrorString(e_));                                   \
            fflush(stderr);                                                                    \
        }                                                                                      \
    } while (0)

// what a list-sharded scan call left in its slot (api_shard.hip; every scan entry point sets it)
enum class ShardState {
    None,           // no scan yet, or the last one stopped on an error
    Exact,         // exact rows in the send buffer
    OnePhase,       // tk_index_shard_scan_plain_dev's rows: the home replay checks the lemma
    HeadOwed,       // tk_index_shard_scan_head_dev ran: _scan_plain_dev(bound_dev) is owed
    RestOwed,       // tk_index_shard_scan_first_dev ran: _scan_rest_dev is owed
};

// buffers of ONE batch in flight
struct Work {
    DevBuf tables, shift, scale, cdist, cheap_idx, cheap_val, probes, slot_prefix, slot_chunk0,
        slot_n, slot_loff, dist, heap_idx, heap_val, repeat_flag, cmins, mins, u_count, u_cursor,
        u_pair_off, u_unit_prefix, u_pair_q, u_pair_f0, c_pair_off, c_unit_prefix, c_pair_q,
        c_pair_f0, spos, rpos, smins, pair_cnt, pair_off, scan_tmp, tally, usage, pos_lens, pos_off,
        qlim, slot_exact, p_count, p_cursor, p_pair_off, p_unit_prefix, p_pair_q, p_pair_f0, flag_list, p_unit_desc,
        plain0, h_count, h_cursor, h_pair_off, h_unit_prefix, h_pair_q, h_pair_f0,   // plain_scan.hip
        plain_q,                                                                       // two-phase sharded scan
        slots_desc;        // pool of TkSlotsOut for the coarse rescoring's epilogue (device copies)
    // The descriptors the fused epilogue reads are IMMUTABLE once written: a small pool per workspace,
    // entry i = slots_pinned[i] (page-locked host memory that outlives every call: the source of the
    // upload, also when that upload is recorded as a node of a hipGraph) and slots_desc[i] (device).
    // A batch looks its descriptor up by content; a new one takes the next free entry; a full pool
    // sends the batch to the unfused make_slots launch.  Nothing a captured graph refers to changes.
    TkSlotsOut *slots_pinned = nullptr;
    int slots_n = 0;
    unsigned slots_need_upload = 0;     // bit i: entry i was only uploaded inside a capture so far
    // list-sharded batch: what tk_index_shard_scan_dev left for the filtered exchange
    const int64_t *shard_probes = nullptr;
    int64_t shard_nq = 0, shard_capacity = 0;
    ShardState shard_state = ShardState::None;     // what the slot's last list-sharded scan call left
    // pipelined mode (depth > 1): hand-offs between the caller's stream and a latency stream
    hipEvent_t tables_done = nullptr, coarse_scanned = nullptr, front_done = nullptr,
               scanned = nullptr, done = nullptr;
    bool busy = false;                                 // `done` has been recorded
    uint64_t td_seq = 0, fd_seq = 0;                   // order in which tables_done / front_done were last recorded
    // plain_scan.hip: how many queries of the workspace's last plain batch were flagged — a
    // page-locked word the device writes and an event behind it, polled (never waited for) when a
    // later call looks at the workspace
    int *flag_host = nullptr;
    hipEvent_t plain_ev = nullptr;
    bool plain_pending = false;
    bool last_plain = false;    // the last batch that used this workspace went the plain way
    int64_t plain_nq = 0;
    void release()
    {
        if (flag_host) (void)hipHostFree(flag_host);
        flag_host = nullptr;
        if (plain_ev) (void)hipEventDestroy(plain_ev);
        plain_ev = nullptr;
        plain_pending = false;
        if (slots_pinned) (void)hipHostFree(slots_pinned);
        slots_pinned = nullptr;
        slots_n = 0;
        slots_need_upload = 0;
        DevBuf *b[] = {&tables, &shift, &scale, &cdist, &cheap_idx, &cheap_val, &probes,
                       &slot_prefix, &slot_chunk0, &slot_n, &slot_loff, &dist, &heap_idx, &heap_val,
                       &repeat_flag, &cmins, &mins, &u_count, &u_cursor, &u_pair_off, &u_unit_prefix,
                       &u_pair_q, &u_pair_f0, &c_pair_off, &c_unit_prefix, &c_pair_q, &c_pair_f0,
                       &spos, &rpos, &smins, &pair_cnt, &pair_off, &scan_tmp, &tally, &usage, &pos_lens, &pos_off,
                       &qlim, &slot_exact, &p_count, &p_cursor, &p_pair_off, &p_unit_prefix, &p_pair_q, &p_pair_f0, &flag_list, &p_unit_desc,
                       &plain0, &h_count, &h_cursor, &h_pair_off, &h_unit_prefix, &h_pair_q, &h_pair_f0,
                       &plain_q, &slots_desc};
        for (DevBuf *x : b) x->release();
        hipEvent_t *evs[] = {&tables_done, &coarse_scanned, &front_done, &scanned, &done};
        for (hipEvent_t *e : evs) {
            if (*e) (void)hipEventDestroy(*e);
            *e = nullptr;
        }
        busy = false;
    }
};

// a table made for ONE layout of the lists: whether it exists, the lists_gen it was made for, how often one was made
struct TkTableState {
    bool ok = false;
    uint64_t gen = 0;
    int64_t builds = 0;
    bool current(uint64_t lists_gen) const { return ok && gen == lists_gen; }
    void made(uint64_t lists_gen) { ok = true, gen = lists_gen, builds++; }
};

// One value per row that queries are restricted by (row_table.hip): by row id as the caller set them (n of them, 0:
// none), and in list-position order, 16 per stored chunk — made by the first call that names an array of the kind.
// noun / called / unit: what the kind's error texts name ("group" / "grouped" / "id").  esz: bytes per row — fixed by the
// kind, or (values: 8 per column, column-major) by row_table_set.
struct TkRowTable {
    size_t esz;
    const char *noun, *called, *unit;
    DevBuf by_row, table;
    int64_t n = 0;
    TkTableState state;
    // The groups alone (group_exact.hip): every row id gathered by group id — span_rows[N] int32, a group's rows one
    // contiguous span, ascending; span_gid[G] the sorted distinct ids; span_off[G + 1] where each span begins.  Made by
    // the first call that needs it, for ONE upload of the values: set_gen counts them (row_table_set), not the lists.
    // The values (value_exact.hip) keep one thing of the kind, with the same lifetime: span_rows[C][N] int32, column c's
    // plane the row ids ascending by (key of column c, row id) — a range over one column is a contiguous span of it.
    // span_gid / span_off stay empty there; span_groups is the number of columns the planes were made for.
    DevBuf span_rows, span_gid, span_off;
    int64_t span_groups = 0;
    uint64_t set_gen = 0;
    TkTableState span_state;
};

#define IXLOCK(ix_)                                               \
    std::unique_lock<std::recursive_mutex> ixlock_;               \
    if (ix_) ixlock_ = std::unique_lock<std::recursive_mutex>((ix_)->mu)

struct Pending;

struct tk_index {
    // one caller at a time: every entry point takes this lock (the reference's kernels are
    // nogil and re-entrant on distinct buffers; calls on one handle from several threads are
    // serialised here instead of corrupting the pipeline state)
    std::recursive_mutex mu;
    // FastPQ
    DevBuf pq_centers;
    int dq = 0, dpb = 0, M = 0, f_order = 0, order = TK_ORDER_AVX;
    double sqrt_nb = 0;
    // coarse
    DevBuf active_centers, center_codes;
    int64_t n_lists = 0, center_chunks = 0;
    int d = 0;
    // lists
    DevBuf list_chunk_off, list_n, ids_off, ids, codes, ids32;
    bool have_ids32 = false;   // every label fits int32: the lane kernel can run the duplicate test
    bool labels24 = false;     // every label is in [0, 0xffffff): the register heap's duplicate test on one register per slot
    int opt_labels24 = 1;      // TK_OPT_LABELS24: 0 = (value, label64) entries even where the labels would fit (tests)
    // repeating labels: where the other copies of every stored row are (twins.hip); twin_w = copies - 1, 0 = no table
    DevBuf twin_list, twin_off;
    int twin_w = 0;
    // tk_index_radius_probe's table where the index keeps none (radius_probe_twins, api_index.hip): made by the first
    // such call of a layout whose labels repeat, dropped with the layout; label_bound: the layout's largest label + 1
    DevBuf rp_twin_list, rp_twin_off;
    int rp_twin_w = 0;
    int64_t label_bound = 0;
    // the table rests on two facts the index build checks where it holds every list's codes (twins.hip: copies of a
    // label lie in different lists and carry the same code); a rank that was handed only its own lists' codes
    // (tk_index_set_lists_shard) cannot, and uses the table only if the caller vouches (TK_OPT_TWIN_VOUCH)
    bool twin_unverified = false, twin_vouched = false;
    int opt_replay_twin = 1;   // TK_OPT_REPLAY_TWIN: 1 = the lane replay decides `insert`'s duplicate test from the twin table
    int64_t total_chunks = 0, total_ids = 0;
    int max_list_chunks = 0;
    uint64_t lists_gen = 0;    // counts the times the lists were (re-)set: an allowed set is valid for one layout
    // where every row is stored (rows.hip): made by the first call that names an exclude array, for ONE layout
    DevBuf row_pos_off, row_pos;
    TkTableState row_pos_state;
    // which rows are stored (group_exact.hip): bit r of an N-bit map = some list holds label r; made from the labels
    // by the first tk_index_knn_group call, for ONE layout
    DevBuf stored_bits;
    TkTableState stored_state;
    // a group id per row (groups.hip) and a 64-bit tag mask per row (tags.hip): by row id as tk_index_set_groups /
    // tk_index_set_tags uploaded them, and in list-position order — made by the first call that names a group / tag
    // array, for ONE layout, as the table above
    TkRowTable groups{4, "group", "grouped", "id"}, tags{8, "tag", "tagged", "mask"};
    // 1 to 4 int64 keys per row (between.hip), column-major in both orders: esz = 8 x columns, set by tk_index_set_values
    TkRowTable values{8, "value", "valued", "key"};
    // members per (list, column of nearest): list l holds its column-0 members first, then column 1's, ...
    // (group_data_by_indices); known after tk_index_build_dev / tk_index_add_rows (list_kp = columns), not
    // after a host upload (list_kp = 0: tk_index_add_rows takes them from the caller)
    std::vector<int64_t> list_cols;
    int list_kp = 0;
    bool ids_unique = false;   // no label occurs twice => the lane-per-query replay is exact
    int heap_mode = 0;         // 0 auto (pair for small batches, lanes, else packed wave), 1 general wave, 2 packed wave, 3 pair
    int opt_pair_nq = 8192;    // TK_OPT_PAIR_NQ: batches up to this many queries take the wave-per-query register heap
    bool have_pq = false, have_centers = false, have_lists = false, have_data = false;
    // list-sharded index: this rank stores the codes of the lists it owns;
    // list_chunk_off stays the GLOBAL layout (every rank derives the same distance rows),
    // local_chunk_off addresses this rank's code storage (lists of other ranks: empty)
    DevBuf owner, local_chunk_off;
    DevBuf rot_t;            // fast mode: R transposed (d_pad, dq) float64, or empty
    DevBuf br_ynorm, br_vals, br_tau, br_cand, br_count, br_out, br_q, br_sample;   // tk_index_knn_brute
    DevBuf br_dist, br_mask, br_exclude, br_group, br_tags, br_ranges;              // ... and what _ex adds
    // tk_index_radius_brute: radii, counts (nq) + slots (nq) + error flag, offsets (nq + 1), the keys as filled, the
    // other half of the sort (keys in one, ids in the other), the part values, the sort's work memory.  rd_total >= 0:
    // a result is held for tk_index_radius_fetch, its ids in rd_alt (rd_ids_alt) or rd_keys
    DevBuf rd_radius, rd_count, rd_off, rd_keys, rd_alt, rd_dist, rd_tmp;
    int64_t rd_total = -1;
    bool rd_ids_alt = false;
    // tk_index_radius_probe (radius_probe.hip): the call's probes (nq, kc) int64, bitmap words per (query, rank) int32
    // and their exclusive prefix sum int64 (+ the scan's work memory), the hit bitmap; float64 vectors: the row ids
    // beside the distance keys; the decoded ids and distances.  rp_total >= 0: a result is held for
    // tk_index_radius_probe_fetch (rp_f64: its distances are float64).  The radii, counters, offsets, keys and the
    // sort's buffers are the rd_* ones above: one radius result of either kind is held at a time.
    DevBuf rp_probes, rp_words, rp_woff, rp_scan, rp_bitmap, rp_rows, rp_ids, rp_dist;
    int64_t rp_total = -1;
    bool rp_f64 = false;
    DevBuf gx_begin, gx_len;                                                        // tk_index_knn_group: a query's span
    DevBuf gx_col;                                                                  // tk_index_knn_between: ... and its column
    int rot_d_pad = 0;
    int rank = 0, world = 1;
    bool sharded = false;
    // vectors
    DevBuf data;
    int64_t N = 0;
    int data_dtype = 0;        // TK_DATA_F32 / TK_DATA_F64 / TK_DATA_F16
    bool data_lent = false;    // shards were cloned from this index: they borrow its arrays
    // index-static descriptors of the coarse stage, staging buffers of the host API
    DevBuf cslots_i, cslots_l, c_chunk_off, q, qpq, stage;
    int scan_mode = 0;         // 0 auto, 1 query-major kernel, 2 list-major (units) kernel
    // tk_index_set_option
    int opt_scan_form = 0;             // exact list-major kernel: 0 per-lane table-row loads, 1 / 2 rows staged in LDS
    int opt_rescore_form = 2;          // rescoring: 2 / 1 rows staged through LDS in tiles of 32 / 64, 0 lane per row
    int opt_plain_limit = 0x7fffffff;  // a cap on every query's table limit (tests: provokes the re-scan path)
    DevBuf replay_counters;            // TK_OPT_REPLAY_COUNT: 4 x uint64 the list replays add to (tk_index_replay_stats)
    bool opt_replay_count = false;
    int opt_replay_lazy = -1;          // lane replay of the lists: 1 lazy (blocks fetched where their minimum passes), 0 staged, -1 auto
    bool flat_plain_ok = true;         // tk_index_top_centers: the plain path has not failed on this index
    int plain_state = 0;       // PLAIN_PROBE .. PLAIN_OFF (see plain_poll)
    int plain_skip = 0;        // OFF: batches left before the next probe
    int plain_backoff = 256;   // OFF: length of the next pause (doubled by a failed probe, up to 4096)
    int plain_wait = 0;        // WAIT: batches seen while no verdict is pending (a probe that was abandoned)
    bool capturing = false;    // the entry point now running was given a stream that is being captured into a hipGraph
                               // (api_index.hip: CaptureScope; false between calls): no event queries, no table builds
    int plain_mode = 0;        // 0 auto: probed lists behind the first ones as plain sums on the matrix
                               // cores where the lemma of plain_scan.hip allows AND few queries need the
                               // re-scan (plain_poll); 1: exact kernel only; 2: plain always
    bool host_out_kernel = false;   // a batch's pinned host copy of the ids is written by a kernel
    // per-batch workspaces: `depth` batches may be in flight (tk_index_set_pipeline),
    // each on its own internal stream
    std::vector<Work> works;
    int depth = 1;
    uint64_t calls = 0;
    std::vector<hipStream_t> lat_streams;    // `depth` of them (pipelined mode)
    hipEvent_t ev_in = nullptr;              // caller's stream -> a batch's stream
    std::deque<std::unique_ptr<Pending>> pending;   // batches whose list scan is still to be enqueued (up to 3 between calls)
    uint64_t ev_seq = 0;                     // counts the records of tables_done / front_done (pipeline_step's merged wait)
    int coalesce = 1;                        // 2: two consecutive calls run as ONE batch (tk_index_set_coalesce)
    std::unique_ptr<Pending> held;           // ... the first of such a pair, waiting for the second
    hipStream_t front_stream = nullptr;      // coarse replays + descriptors of all batches, in order
    // profiling: one set of 8 events per recorded batch, read back on demand
    int profiling = 0;
    uint64_t prof_seen = 0;
    std::vector<hipEvent_t> evs;   // 8 per set
    std::vector<hipStream_t> ev_streams;
    std::vector<char> ev_plain;    // the set's batch ran the plain kernel (events 8, 9 recorded)
    size_t ev_used = 0;            // sets recorded since the last read
    int last_S = 0, last_R = 0, last_work = 0;
    int64_t last_nq = 0;
    int64_t last_replay[4] = {-1, 0, 0, 0};    // tk_index_last_replay: form, lazy, label24 entries, twin width (stage_back)
};

// the value columns an index has (0: none), and the int64 keys of one column's plane of the value table (between.hip)
static inline int value_columns(const tk_index *ix) { return ix->values.n > 0 ? (int)(ix->values.esz / 8) : 0; }
static inline int64_t value_plane(const tk_index *ix) { return (ix->total_chunks > 0 ? ix->total_chunks : 1) * 16; }

// an allowed set (allow.hip): 16 bits per stored chunk in list-position order, for ONE layout of the lists
struct tk_allow {
    tk_index *ix = nullptr;
    DevBuf bits;
    int64_t count = 0;         // allowed stored rows (a label stored twice counts twice)
    int64_t stored = 0;        // stored rows of the layout
    uint64_t lists_gen = 0;    // tk_index::lists_gen when it was made
};
// A finished layout of the inverted lists on its way into an index (install_lists): the device arrays in the index's
// formats and what the host knows about them.  What it still holds when it goes — the index's old arrays after
// install_lists, its own after a call that failed before — is released with it.
static const int64_t NO_LABEL_BOUND = 1ll << 62;    // max_label of a layout with a negative label: no compact label form applies
struct ListLayout {
    DevBuf codes, ids, list_chunk_off, ids_off, list_n;
    DevBuf ids32;               // the labels as int32 where have_ids32 (they repeat, and all fit)
    bool have_ids32 = false;
    int64_t total_chunks = 0, total_ids = 0, max_list_chunks = 0;
    int64_t max_label = -1;     // the largest label (-1: no stored entry)
    bool ids_unique = false;    // no label occurs twice
    std::vector<int64_t> list_cols;     // members per (list, column), kp columns; empty: unknown
    int kp = 0;
    // a rank's upload of the lists it owns (tk_index_set_lists_shard): every list's owner, this rank's chunk offsets
    bool sharded = false;
    int rank = 0, world = 1;
    DevBuf owner, local_chunk_off;
    // the CSR arrays of L lists of these sizes (16 rows to a chunk) and the totals they give
    int set_sizes(const int64_t *sizes, int64_t L)
    {
        std::vector<int64_t> coff((size_t)L + 1, 0), ioff((size_t)L + 1, 0);
        for (int64_t i = 0; i < L; i++) {
            const int64_t c = (sizes[i] + 15) / 16;
            coff[(size_t)i + 1] = coff[(size_t)i] + c;
            ioff[(size_t)i + 1] = ioff[(size_t)i] + sizes[i];
            if (c > max_list_chunks) max_list_chunks = c;
        }
        ARGCHECK(max_list_chunks < (1ll << 26), "list too long");
        total_chunks = coff[(size_t)L];
        total_ids = ioff[(size_t)L];
        TRY(list_chunk_off.ensure((size_t)(L + 1) * 8));
        TRY(ids_off.ensure((size_t)(L + 1) * 8));
        TRY(list_n.ensure((size_t)(L > 0 ? L : 1) * 8));
        HIPCHECK(hipMemcpy(list_chunk_off.p, coff.data(), (size_t)(L + 1) * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(ids_off.p, ioff.data(), (size_t)(L + 1) * 8, hipMemcpyHostToDevice));
        if (L > 0) HIPCHECK(hipMemcpy(list_n.p, sizes, (size_t)L * 8, hipMemcpyHostToDevice));
        return TK_OK;
    }
    ListLayout() = default;
    ListLayout(const ListLayout &) = delete;
    ~ListLayout()
    {
        for (DevBuf *b : {&codes, &ids, &list_chunk_off, &ids_off, &list_n, &ids32, &owner, &local_chunk_off}) b->release();
    }
};
// the set a batch applies: NULL where the set allows every stored row (no kernel at all)
const tk_allow *allow_effective(const tk_allow *a);

// What ONE call restricts its answers by, any of it absent: an allowed set (allow.hip), and per query (device arrays,
// or NULL) a row the query may not return (rows.hip), a group it is restricted to (groups.hip), a tag mask it is
// restricted by (tags.hip) in the call's tag_mode (0: a row passes with any of the mask's tags, 1: with all of them),
// its ranges (between.hip): 2 x cols int64 keys per query, (lo, hi) per column; cols: the index's when the call came.
struct TkCallRestrict {
    const tk_allow *allow = nullptr;
    const int64_t *exclude = nullptr;
    const int32_t *group = nullptr;
    const uint64_t *tags = nullptr;
    int tag_mode = 0;
    const int64_t *between = nullptr;
    int cols = 0;
    // Not a restriction of what the scans see but a shape of what comes back: at most per_group[q] rows of any group
    // among query q's answers, 0 for no cap (cap_select.h; int32 per query).  It reads the groups by row id only.
    const int32_t *per_group = nullptr;
    // the call's rows from row o on
    TkCallRestrict at(int64_t o) const
    {
        return {allow, exclude ? exclude + o : nullptr, group ? group + o : nullptr, tags ? tags + o : nullptr, tag_mode,
                between ? between + o * 2 * cols : nullptr, cols, per_group ? per_group + o : nullptr};
    }
    // Join rule: two calls run as one batch (coalesce_call) with the same allowed set, both grouped or neither (the
    // two kinds take different scans: exact_scan), both tagged in one mode or neither (one mode per launch), both ranged or neither,
    // both capped or neither (the two kinds take different rescoring kernels).
    bool joins(const TkCallRestrict &o) const
    {
        return allow == o.allow && !group == !o.group && !tags == !o.tags && (!tags || tag_mode == o.tag_mode) &&
               !between == !o.between && !per_group == !o.per_group;
    }
    // Table rule: what the passes read exists before the call's first launch (each made once per layout of the lists,
    // synchronising the device; TK_ERR_STATE where the index has no groups / tags / values for every row).  Defined below.
    int ensure_tables(tk_index *ix, int64_t nq) const;
};

// What a BATCH is restricted by: the one call's, or (a pair, joins()) the first call's with the second call's arrays
// behind them — a TkSecond with b == NULL: the second call's rows are unrestricted in that kind.
struct TkRestrict {
    const tk_allow *allow = nullptr;
    int tag_mode = 0;
    const int64_t *exclude = nullptr;
    const int32_t *group = nullptr;
    const uint64_t *tags = nullptr;
    const int64_t *between = nullptr;
    const int32_t *per_group = nullptr;
    TkSecond exclude2, group2, tags2, between2, per_group2;
    TkRestrict() = default;
    // a: the first call; b (or NULL: one call): the second, whose rows start at batch row n_a
    TkRestrict(const TkCallRestrict &a, const TkCallRestrict *b = nullptr, int64_t n_a = 0)
        : allow(a.allow), tag_mode(a.tag_mode), exclude(a.exclude), group(a.group), tags(a.tags),
          between(a.between), per_group(a.per_group)
    {
        if (b) exclude2 = {b->exclude, n_a}, group2 = {b->group, n_a}, tags2 = {b->tags, n_a}, between2 = {b->between, n_a};
        if (b) per_group2 = {b->per_group, n_a};
    }
    // the final rescoring caps its answers per group; no pass, and the scan an uncapped batch takes (not in any())
    bool capped() const { return per_group || per_group2.b; }
    bool excludes() const { return exclude || exclude2.b; }
    bool grouped() const { return group || group2.b; }
    bool tagged() const { return tags || tags2.b; }
    bool ranged() const { return between || between2.b; }
    // Anything set: the batch launches at least one restricting pass
    bool any() const { return allow || excludes() || grouped() || tagged() || ranged(); }
    // Exact-scan rule: a batch with an allowed set, a group, tag or range array takes the exact scan in the automatic
    // plain-scan mode (plain_for); an excluded row masks a byte or two and does not.
    bool exact_scan() const { return allow || grouped() || tagged() || ranged(); }
};
struct Plan {
    int kc, rescore, R, S;
    int64_t cap;       // uint4 per query in the distance buffer
    int64_t cap_min;   // bytes per query in the block-minimum buffer (multiple of 16)
    int64_t ccap_min;  // same for the coarse stage
};

#define TK_SLOTS_POOL 16
int reserve_slots_pool(Work &w);      // api_index.hip: the pool above exists (not inside a capture)

static const int64_t MAX_SUB = 32768;  // gridDim.y limit of the scan kernels is 65535
// a sharded batch only runs the list-major kernels (no gridDim.y); what bounds it is int32 unit
// counts and the 16 GB of distance rows per rank, both checked in shard_args
static const int64_t MAX_SHARD_BATCH = 131072;

// stage timers of one batch (tk_index_set_profiling)
#define TK_PROF_EVENTS 10     // per recorded batch: 8 stage marks + 2 around the plain kernel alone
struct Prof {
    const std::vector<hipEvent_t> *evs = nullptr;   // the index's event pool (it may grow)
    size_t base = 0;
    int evi = 0;
    int set = -1;
    bool plain_marked = false;
    int mark(hipStream_t st)
    {
        if (evs) HIPCHECK(hipEventRecord((*evs)[base + (size_t)evi++], st));
        return TK_OK;
    }
    int mark_plain(int which, hipStream_t st)       // 0: in front of the plain kernel, 1: behind it
    {
        if (evs) {
            HIPCHECK(hipEventRecord((*evs)[base + 8 + (size_t)which], st));
            plain_marked = true;
        }
        return TK_OK;
    }
};

// the distance tables a batch's scans read: the workspace's, or the gathered rows of a list-sharded batch
inline const uint4 *tables_of(const Work &w) { return w.tables.as<uint4>(); }

// ---- api_index.hip, used by the other files
static inline size_t data_esz(int dtype) { return dtype == TK_DATA_F64 ? 8 : (dtype == TK_DATA_F16 ? 2 : 4); }
// TK_OK, or TK_ERR_ARG naming row0 + the first of n float32 rows (device) with a value whose half is not finite
int check_half_rows(const float *X, int64_t n, int d, int64_t row0, DevBuf &flag);
int flush_pending(tk_index *ix);
// nothing in flight, the device idle, the automatic plain-scan state back to its first probe: the lists may change
int settle_lists(tk_index *ix);
// THE place where an index takes a new set of lists.  The arrays are swapped in (the old ones leave with `lay`), every
// field derived from the layout is set, allowed sets made for the old layout stop working (lists_gen), the twin table
// (twins.hip; none where the labels are distinct, too sparse, or one label has more than 16 copies) is made again.
// Nothing fails once the swap has begun — a twin table that cannot be made is no table — so a caller that did its
// checks and allocations first changes the index entirely or not at all.
int install_lists(tk_index *ix, ListLayout &lay);
// tk_index_radius_probe's twin table (api_index.hip): the index's own, or one made for the call where the labels repeat
// and the index keeps none; *w = 0: the labels are distinct.  Refused (TK_ERR_STATE): a label stored more than 17 times,
// copies with different codes or in one list, labels beyond int32, no memory to spare
int radius_probe_twins(tk_index *ix, const int32_t **list, int *w);
bool twin_replay(const tk_index *ix, const struct Plan &p);
int make_plan(const tk_index *ix, int k, int n_probes, int pass_1, Plan &p);
bool plain_env_on();
int plain_k(const tk_index *ix, int64_t nq, const Plan &p);
size_t plain_desc_bytes(const tk_index *ix, int64_t nq, const Plan &p);
double workspace_bytes();
bool coarse_units(const tk_index *ix, int64_t nq);
// row0: the tables (and limits) of rows [row0, row0 + nq) of the workspace; qpq_dev points at row row0's query
int stage_tables(tk_index *ix, Work &w, const void *qpq_dev, int qpq_f64, int64_t nq, hipStream_t st, Prof &pf,
                 bool plain = false, TkSecond qpq2 = TkSecond(), int64_t row0 = 0);
TkScanJob coarse_job(const tk_index *ix, const Work &w, const Plan &p);
int plain_blocks();
int shard_plain_blocks();
void launch_coarse_scan(tk_index *ix, Work &w, int64_t nq, const Plan &p, hipStream_t st,
                        const uint4 *tables = nullptr);
// ---- api_build.hip, used by radius_probe.hip
// The index's coarse stage for k probes (tk_index_top_centers' chunks), its result left on the device: see there.
typedef std::function<int(int64_t o, int64_t m, int kc, const int64_t *probes_dev, const float *dist_dev)> TkProbeSink;
int coarse_top_chunks(tk_index *ix, const float *q, const void *q_pq, int q_pq_is_f64, int64_t nq, int k,
                      bool want_dist, const TkProbeSink &sink);
// the restriction of a restricted exact call from the caller's host arrays (see there); any = false: none given
int brute_restrict(tk_index *ix, int64_t nq, const uint8_t *allowed_mask, const int64_t *exclude,
                   const int32_t *group, const uint64_t *tags, int tag_mode, const int64_t *between,
                   TkBruteRestrict &r, bool &any);
// the replay over the coded centres of queries [0, nq) (one slot every query shares, positions as labels)
TkReplayJob centre_replay_job(const tk_index *ix, Work &w, int64_t nq, const Plan &p);
// dist (or NULL): the probes' exact float32 distances beside probes_out (FlatTop; the IVF coarse stage asks for none)
int coarse_replay_probes(tk_index *ix, Work &w, const float *q_dev, int64_t nq, const Plan &p,
                         int64_t *probes_out, hipStream_t st, Prof &pf, TkSecond q2 = TkSecond(),
                         const TkSlotsOut *slots = nullptr, int *slots_written = nullptr, float *dist = nullptr);
void coarse_slots(tk_index *ix, Work &w, const int64_t *probes, int64_t nq, const Plan &p,
                  int *pair_count, const int *owner, int me, hipStream_t st, bool plain = false);
int stage_coarse_rest(tk_index *ix, Work &w, const float *q_dev, int64_t nq, const Plan &p,
                      int *pair_count, const int *owner, int me, hipStream_t st, Prof &pf,
                      bool plain = false, TkSecond q2 = TkSecond());
// plain_flag (list-sharded home rank): queries the plain path's lemma does not cover raise bit 4 of
// *plain_flag instead of being scanned again (the codes are on other ranks: the batch is repeated)
// dist_dev / dist2 (or NULL): the rescoring's distances beside out_dev / out2 (tk_launch_rescore's dist / dist2)
int stage_back(tk_index *ix, Work &w, const float *q_dev, int64_t q0, int64_t nq, int k,
               const Plan &p, int64_t *out_dev, hipStream_t st, Prof &pf, bool plain = false,
               TkSecond q2 = TkSecond(), TkSecond out2 = TkSecond(), int *plain_flag = nullptr,
               const TkRestrict &r = TkRestrict(), void *dist_dev = nullptr, TkSecond dist2 = TkSecond());
// a table of the index's current lists may be made now: there are lists, and no stream capture is under way
int table_may_build(const tk_index *ix, const char *table, const char *call);
// rows.hip: the row-position table of the index's current lists exists (made now if not: synchronises the device)
int row_pos_ensure(tk_index *ix);
// row_table.hip — set: calls still owed run first, then the values are uploaded (n == N of them; `check`, if any, has
// the last word on them; esz, if not 0, is the kind's bytes per row from now on) or (n == 0) dropped.  ensure: values for every row the index has (else TK_ERR_STATE) and the
// table of its current lists, made now if not by `launch` (synchronises the device).  info: tk_index_*_table's info4.
int row_table_set(tk_index *ix, TkRowTable &t, const void *vals, int64_t n,
                  int (*check)(const void *vals, int64_t n) = nullptr, size_t esz = 0);
int row_table_ensure(tk_index *ix, TkRowTable &t, void (*launch)(const tk_index *ix));
int row_table_covers(const tk_index *ix, const TkRowTable &t);    // TK_ERR_STATE unless by_row covers all N rows
int row_table_info(const tk_index *ix, const TkRowTable &t, int64_t *info4);
int group_table_ensure(tk_index *ix);       // groups.hip
int group_rows_ensure(tk_index *ix);        // group_rows.hip: the rows by group of the groups the index has now
int value_rows_ensure(tk_index *ix);        // value_rows.hip: the rows in value order, per column, of the values it has now
// group_exact.hip: the N-bit map of stored rows of the current lists (made now if not: synchronises the device);
// call: the entry point that asks, named in the error where the map cannot be made
int stored_bits_ensure(tk_index *ix, const char *call);
int tag_table_ensure(tk_index *ix);         // tags.hip
int value_table_ensure(tk_index *ix);       // between.hip
inline int TkCallRestrict::ensure_tables(tk_index *ix, int64_t nq) const
{
    if (exclude && nq > 0) TRY(row_pos_ensure(ix));
    if ((group || per_group) && nq > 0) TRY(group_table_ensure(ix));
    if (tags && nq > 0) TRY(tag_table_ensure(ix));
    if (between && nq > 0) TRY(value_table_ensure(ix));
    return TK_OK;
}
int head_chunks(const tk_index *ix, const Plan &p);    // chunks of a first probed list the exact kernel keeps (head mode)
// the workspace's three pair sets: whole lists exact / plain tiles / heads
TkPairSet exact_pairs(const Work &w);
TkPairSet plain_pairs(const tk_index *ix, const Work &w, int64_t nq, const Plan &p);
TkPairSet head_pairs(const Work &w);
// the list scans' jobs over those sets, into the workspace's distance rows
TkScanJob list_job(const tk_index *ix, const Work &w, const Plan &p);
TkScanJob plain_job(const tk_index *ix, const Work &w, const Plan &p);
TkScanJob head_job(const tk_index *ix, const Work &w, const Plan &p);
