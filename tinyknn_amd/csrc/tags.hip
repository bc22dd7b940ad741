// tags.hip — every query of a batch restricted to the rows that carry its tags
// (tk_index_set_tags / tk_index_query_batch[_dev]_ex4).
//
// What tags mean: rows carry a 64-bit mask, tags[r], bit t set = row r carries tag t; a mask of 0 is a
// row without tags.  A query carries a mask m, the call one mode: "any" — a row passes iff (tags[r] & m) != 0; "all" —
// iff (tags[r] & m) == m.  A query with m != 0 returns what the reference's IVF.query (ivf.py:106-163) returns when
// `insert` in query_pq runs only for labels that pass — the allowed set of §3.8, for that query alone, and so the
// allow pass's move: every probed row that does not pass gets the heap's empty value in the distance bytes, behind the
// list scans and every re-scan, in front of every replay that reads dist / mins.  m == 0: the query is unrestricted
// in both modes (the truth of the formula in "all", the convention "no filter was given" in "any").  Every stored copy
// of a label has the label's tags, so the copies are all in or all out (twin lemma); a masked byte is the empty value
// in both scans (plain-scan lemma).
//
// The tag table in list-position order: 16 uint64 per stored chunk, indexed like the group table (entry 16 c + r = the
// tags of row r of global chunk c; 0, which passes no restricted query in either mode since m != 0 there, for the rows
// that pad a list's last chunk and for labels outside [0, N)).  128 bytes per stored chunk: 0.8 GB for 100M rows
// stored once, beside the 8 N bytes of the tags by row id.  Made from the device-resident labels by the first call
// that names a tag array, for one layout of the lists (lists_gen), as the group table.
#include "api_internal.h"
#include "chunk_mask.h"

// One workgroup per list, threads striding over the list's rows padded to whole chunks (group_table_kernel's geometry).
__global__ __launch_bounds__(256) void tag_table_kernel(const int64_t *__restrict__ list_chunk_off,
                                                        const int64_t *__restrict__ list_n,
                                                        const int64_t *__restrict__ ids_off,
                                                        const int64_t *__restrict__ ids,
                                                        const uint64_t *__restrict__ row_tags, int64_t N,
                                                        uint64_t *__restrict__ table)
{
    const int64_t l = blockIdx.x;
    const int64_t c0 = list_chunk_off[l];
    const int64_t rows = (list_chunk_off[l + 1] - c0) * 16;     // padded to whole chunks
    const int64_t n = list_n[l];
    const int64_t io = ids_off[l];
    for (int64_t r = threadIdx.x; r < rows; r += blockDim.x) {
        uint64_t t = 0;
        if (r < n) {
            const int64_t lab = ids[io + r];
            if (lab >= 0 && lab < N) t = row_tags[lab];
        }
        table[c0 * 16 + r] = t;
    }
}

// group_pass_kernel's geometry: one workgroup per query, the slot prefix in LDS, a binary search to the slot,
// slot_chunk0 to the global chunk.  The 16-bit keep mask is made from the chunk's 16 tag masks (eight 16-byte loads)
// with 64-bit compares, ALL: (t & m) == m, else (t & m) != 0.  m_a: the masks of rows [0, n_a) of the batch, m_b: of
// the rows behind them (a pair of calls, both of one mode); NULL, or an entry of 0: the query is unrestricted and its
// workgroup returns before it touches anything.  q0, only: as group_pass_kernel.
template <bool SIGNED, bool ALL>
__global__ __launch_bounds__(256) void tag_pass_kernel(uint4 *__restrict__ dist, int64_t cap,
                                                       uint8_t *__restrict__ mins, int64_t cap_min,
                                                       const int *__restrict__ slot_prefix,
                                                       const int64_t *__restrict__ slot_chunk0, int S,
                                                       const ulonglong2 *__restrict__ table,
                                                       const uint64_t *__restrict__ m_a,
                                                       const uint64_t *__restrict__ m_b, int64_t n_a, int64_t q0,
                                                       const int *__restrict__ only)
{
    extern __shared__ int pre[];        // S + 1
    int64_t q = blockIdx.x;
    if (only) {
        if ((int)blockIdx.x >= only[0]) return;
        q = only[1 + blockIdx.x];
    }
    const int64_t row = q0 + q;
    const uint64_t *ma = row < n_a ? m_a : m_b;
    if (!ma) return;
    const uint64_t m = ma[row < n_a ? row : row - n_a];
    if (m == 0) return;
    for (int s = threadIdx.x; s <= S; s += blockDim.x) pre[s] = slot_prefix[q * (S + 1) + s];
    __syncthreads();
    const int total = pre[S];
    for (int f = threadIdx.x; f < total; f += blockDim.x) {
        int lo = 0, hi = S;     // largest lo with pre[lo] <= f (pre is non-decreasing, pre[0] = 0)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (pre[mid] <= f) lo = mid; else hi = mid;
        }
        const ulonglong2 *t = table + (slot_chunk0[q * S + lo] + (f - pre[lo])) * 8;
        uint32_t b = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const ulonglong2 v = t[j];
            const uint64_t x = (uint64_t)v.x & m, y = (uint64_t)v.y & m;
            const uint32_t px = ALL ? x == m : x != 0, py = ALL ? y == m : y != 0;
            b |= (px | (py << 1)) << (2 * j);
        }
        tk_mask_chunk<SIGNED>(dist + q * cap + f, mins + q * cap_min + f, b);
    }
}

void tk_launch_tag_pass(uint4 *dist, int64_t cap, uint8_t *mins, int64_t cap_min, int64_t nq,
                        const int *slot_prefix, const int64_t *slot_chunk0, int S, const uint64_t *table,
                        const uint64_t *m_a, TkSecond m_b, int all, int64_t q0, int signd, const int *only,
                        hipStream_t s)
{
    if (nq <= 0 || (!m_a && !m_b.b)) return;
    const int64_t n_a = m_b.n_a > 0 ? m_b.n_a : INT64_MAX;     // (no second call: every row is m_a's)
    const size_t lds = (size_t)(S + 1) * 4;
#define TK_TAG_PASS(SG, AL)                                                                                          \
    hipLaunchKernelGGL((tag_pass_kernel<SG, AL>), dim3((unsigned)nq), dim3(256), lds, s, dist, cap, mins, cap_min,  \
                       slot_prefix, slot_chunk0, S, (const ulonglong2 *)table, m_a, (const uint64_t *)m_b.b, n_a,   \
                       q0, only)
    if (signd) {
        if (all) TK_TAG_PASS(true, true); else TK_TAG_PASS(true, false);
    } else {
        if (all) TK_TAG_PASS(false, true); else TK_TAG_PASS(false, false);
    }
#undef TK_TAG_PASS
}

// What a call that names a tag array needs: tags for every row the index has now, and the table for the index's
// current lists — made on the first such call, and again after the lists changed.  Synchronises the device (once per
// layout).
int tag_table_ensure(tk_index *ix)
{
    if (ix->tags_n == 0) return fail(TK_ERR_STATE, "a tag array was passed but the index has no tags: tk_index_set_tags first");
    if (ix->tags_n != ix->N)
        return fail(TK_ERR_STATE, "the tags cover " + std::to_string(ix->tags_n) + " rows, the index has " +
                                      std::to_string(ix->N) + " now: set them again (tk_index_set_tags)");
    if (ix->tag_table_ok && ix->tag_table_gen == ix->lists_gen) return TK_OK;
    ARGCHECK(ix->have_lists && ix->have_data, "index has no lists / data yet");
    ARGCHECK(!ix->capturing, "the tag table cannot be made inside a stream capture: make one tagged call before "
                             "the capture");
    ix->tag_table_ok = false;
    TRY(ix->tag_table.ensure((size_t)(ix->total_chunks > 0 ? ix->total_chunks : 1) * 128));
    if (ix->n_lists > 0)
        hipLaunchKernelGGL(tag_table_kernel, dim3((unsigned)ix->n_lists), dim3(256), 0, 0,
                           ix->list_chunk_off.as<int64_t>(), ix->list_n.as<int64_t>(), ix->ids_off.as<int64_t>(),
                           ix->ids.as<int64_t>(), ix->row_tags.as<uint64_t>(), ix->N, ix->tag_table.as<uint64_t>());
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    ix->tag_table_ok = true;
    ix->tag_table_gen = ix->lists_gen;
    ix->tag_table_builds++;
    return TK_OK;
}

// ---- C ABI ----

extern "C" int tk_index_set_tags(tk_index *ix, const uint64_t *tags, int64_t n)
{
    IXLOCK(ix);
    ARGCHECK(ix, "null index");
    ARGCHECK(n >= 0 && (n == 0 || tags), "tags: n masks, or NULL and 0");
    ARGCHECK(!ix->sharded, "list-sharded index: row tags are not supported");
    if (n > 0) ARGCHECK(ix->have_data && n == ix->N, "tags: one mask per row of the index (n == N)");
    TRY(flush_pending(ix));                 // calls still owed that read the old tags are enqueued ...
    HIPCHECK(hipDeviceSynchronize());       // ... and have run
    ix->tag_table_ok = false;
    ix->tags_n = 0;
    if (n == 0) {
        ix->row_tags.release();
        ix->tag_table.release();
        return TK_OK;
    }
    TRY(ix->row_tags.ensure((size_t)n * 8));
    HIPCHECK(hipMemcpy(ix->row_tags.p, tags, (size_t)n * 8, hipMemcpyHostToDevice));
    ix->tags_n = n;
    return TK_OK;
}

extern "C" int64_t tk_index_tags(tk_index *ix)
{
    IXLOCK(ix);
    if (!ix) return fail(TK_ERR_ARG, "bad argument: null index");
    return ix->tags_n;
}

extern "C" int tk_index_tag_table(tk_index *ix, int64_t *info4)
{
    IXLOCK(ix);
    ARGCHECK(ix && info4, "null index / buffer");
    const bool have = ix->tag_table_ok && ix->tag_table_gen == ix->lists_gen;
    info4[0] = have ? 1 : 0;
    info4[1] = have ? (ix->total_chunks > 0 ? ix->total_chunks : 1) * 128 : 0;
    info4[2] = ix->tag_table_builds;
    info4[3] = ix->tags_n * 8;
    return TK_OK;
}
