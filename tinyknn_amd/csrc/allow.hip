// allow.hip — an allowed set of row ids for IVF.query (tk_allow_create / tk_index_query_batch[_dev]_allow).
//
// What a set means: a query returns what the reference's IVF.query (ivf.py:106-163) returns when
// `insert` in query_pq (_fast_pq_256.pyx:114-118, _fast_pq.pyx:197-201) runs only for labels in the set.  Nothing
// else changes: coarse stage and probe order, pass_1, the stale bound per 16-row block, the -1 removal and the
// `len(indices) <= k` early return, knn_brute1 over the surviving candidates.
//
// How (the equivalence tests/test_allowed_cpu.py checks): guarding `insert` with `label in A` gives the same heap,
// bit for bit, as giving every disallowed row the heap's empty value (127 signed, 255 unsigned) — at the start of
// every block top_bound == vals[0]; a block either refreshes the bound to vals[0] or inserts nothing, so a refresh
// after only disallowed passing rows changes nothing; within a block both forms compare against the same bound; and
// the empty value is below no bound, like a saturated row of the reference.  That is what pad_fix_kernel (heap.hip)
// already does to the rows that pad a list's last chunk: the allow pass does it to every probed chunk, after the
// list scans and before any replay reads dist / mins.
//
// The set is a bitmap in list-position order: 16 bits per stored chunk, indexed like list_chunk_off (bit r of chunk
// c = row r of the chunk; the rows that pad a list's last chunk get 0).
#include "api_internal.h"
#include "chunk_mask.h"

// One workgroup per list.  Each wave takes 64 consecutive rows of the list (4 chunks): lane j tests row j's label,
// the wave's ballot holds the 4 chunks' 16-bit masks, lanes 0/16/32/48 write them.  Coalesced reads of the labels.
__global__ __launch_bounds__(256) void allow_bits_kernel(const int64_t *__restrict__ list_chunk_off,
                                                         const int64_t *__restrict__ list_n,
                                                         const int64_t *__restrict__ ids_off,
                                                         const int64_t *__restrict__ ids,
                                                         const uint8_t *__restrict__ mask, int64_t N,
                                                         uint16_t *__restrict__ bits,
                                                         unsigned long long *__restrict__ count)
{
    const int64_t l = blockIdx.x;
    const int64_t c0 = list_chunk_off[l];
    const int64_t rows = (list_chunk_off[l + 1] - c0) * 16;     // padded to whole chunks
    const int64_t n = list_n[l];
    const int64_t io = ids_off[l];
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)threadIdx.x - lane; base < rows; base += blockDim.x) {
        const int64_t r = base + lane;
        bool ok = false;
        if (r < n) {
            const int64_t lab = ids[io + r];
            ok = lab >= 0 && lab < N && mask[lab] != 0;
        }
        const unsigned long long b = __ballot(ok);
        if ((lane & 15) == 0 && r < rows) bits[c0 + (r >> 4)] = (uint16_t)(b >> lane);
        if (lane == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
    }
}

// One workgroup per query over the query's probed chunks (tk_mask_probed, chunk_mask.h), a chunk's keep mask its 16
// bits of the set: a chunk whose bits are all set is not touched; one with none set is written without being read;
// else its disallowed bytes take the empty value and its minimum byte is recomputed.  only (or NULL): [count, q_0,
// q_1, ...] — just these queries (tk_pass_query).
template <bool SIGNED>
__global__ __launch_bounds__(256) void allow_pass_kernel(uint4 *__restrict__ dist, int64_t cap,
                                                         uint8_t *__restrict__ mins, int64_t cap_min,
                                                         const int *__restrict__ slot_prefix,
                                                         const int64_t *__restrict__ slot_chunk0, int S,
                                                         const uint16_t *__restrict__ bits,
                                                         const int *__restrict__ only)
{
    int64_t q;
    if (!tk_pass_query(blockIdx.x, only, q)) return;
    tk_mask_probed<SIGNED>(dist, cap, mins, cap_min, slot_prefix, slot_chunk0, S, q,
                           [=](int64_t c) -> uint32_t { return bits[c]; });
}

void tk_launch_allow_pass(uint4 *dist, int64_t cap, uint8_t *mins, int64_t cap_min, int64_t nq,
                          const int *slot_prefix, const int64_t *slot_chunk0, int S, const uint16_t *bits,
                          int signd, const int *only, hipStream_t s)
{
    if (nq <= 0) return;
    const size_t lds = (size_t)(S + 1) * 4;
    const auto kernel = signd ? allow_pass_kernel<true> : allow_pass_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nq), dim3(256), lds, s, dist, cap, mins, cap_min, slot_prefix, slot_chunk0,
                       S, bits, only);
}

const tk_allow *allow_effective(const tk_allow *a)
{
    return a && a->count < a->stored ? a : nullptr;
}

// ---- C ABI ----

extern "C" int tk_allow_create(tk_index *ix, const uint8_t *mask, int64_t n, tk_allow **out)
{
    IXLOCK(ix);
    ARGCHECK(ix && mask && out, "null index / mask / output");
    *out = nullptr;
    ARGCHECK(ix->have_lists && ix->have_data, "index has no lists / data yet");
    ARGCHECK(!ix->sharded, "list-sharded index: allowed sets are not supported");
    ARGCHECK(n == ix->N, "mask length must equal the index's row count N");
    TRY(require_gpu());
    tk_allow *a = new tk_allow;
    a->ix = ix;
    a->lists_gen = ix->lists_gen;
    a->stored = ix->total_ids;
    DevBuf m, cnt;
    int r = TK_OK;
    auto run = [&]() -> int {
        TRY(m.ensure((size_t)(n > 0 ? n : 1)));
        TRY(cnt.ensure(8));
        TRY(a->bits.ensure((size_t)(ix->total_chunks > 0 ? ix->total_chunks : 1) * 2));
        HIPCHECK(hipMemcpy(m.p, mask, (size_t)n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(cnt.p, 0, 8));
        if (ix->n_lists > 0)
            hipLaunchKernelGGL(allow_bits_kernel, dim3((unsigned)ix->n_lists), dim3(256), 0, 0,
                               ix->list_chunk_off.as<int64_t>(), ix->list_n.as<int64_t>(), ix->ids_off.as<int64_t>(),
                               ix->ids.as<int64_t>(), m.as<uint8_t>(), n, a->bits.as<uint16_t>(),
                               cnt.as<unsigned long long>());
        HIPCHECK(hipGetLastError());
        unsigned long long c = 0;
        HIPCHECK(hipMemcpy(&c, cnt.p, 8, hipMemcpyDeviceToHost));
        a->count = (int64_t)c;
        return TK_OK;
    };
    r = run();
    m.release();
    cnt.release();
    if (r != TK_OK) {
        a->bits.release();
        delete a;
        return r;
    }
    *out = a;
    return TK_OK;
}

extern "C" int64_t tk_allow_count(const tk_allow *a)
{
    if (!a) return fail(TK_ERR_ARG, "bad argument: null allowed set");
    return a->count;
}

extern "C" int tk_allow_destroy(tk_allow *a)
{
    if (!a) return TK_OK;
    int r = TK_OK;
    {
        IXLOCK(a->ix);
        r = flush_pending(a->ix);           // calls still owed that read the set are enqueued ...
        const hipError_t e = hipDeviceSynchronize();      // ... and have run
        if (r == TK_OK && e != hipSuccess) r = fail(TK_ERR_HIP, hipGetErrorString(e));
        a->bits.release();
    }
    delete a;
    return r;
}
