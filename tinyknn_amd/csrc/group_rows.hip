// group_rows.hip — every row id gathered by group id, on the device (TkRowTable::span_*; what group_exact.hip walks).
// span_rows[N] int32: the rows of one group one contiguous span, ascending; span_gid[G]: the sorted distinct group ids;
// span_off[G + 1]: where the spans begin.  Group ids are sparse in [0, 2^31 - 1), so this is a sort by key: rocPRIM's
// radix sort over (group, row) pairs — 31 key bits, stable — its run-length encoding of the sorted keys, and
// tk_scan_exclusive over the run lengths.  The library's kernels are instantiated in this file alone.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

#include "api_internal.h"

__global__ __launch_bounds__(256) void iota_rows_kernel(int32_t *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
}

// The rows by group for the groups the index has now: made on the first call, and again after tk_index_set_groups.
// Work memory (freed before it returns): the sorted keys, the row ids going in, the run-length encoding's outputs at
// their worst-case size and the library's own — about 20 N bytes beside the 4 N + 8 G that stay.
int group_rows_ensure(tk_index *ix)
{
    TkRowTable &t = ix->groups;
    TRY(row_table_covers(ix, t));
    if (t.span_state.current(t.set_gen)) return TK_OK;
    TRY(table_may_build(ix, "rows-by-group", "tk_index_knn_group"));
    ARGCHECK(ix->N < 0x7ffffff0ll, "rows by group: N < 2^31");
    t.span_state.ok = false;
    const int64_t N = ix->N;
    DevBuf keys, iota, uniq, counts, runs, tmp;
    auto run = [&]() -> int {
        const unsigned grid = (unsigned)((N + 255) / 256);
        TRY(keys.ensure((size_t)N * 4));
        TRY(iota.ensure((size_t)N * 4));
        TRY(uniq.ensure((size_t)N * 4));
        TRY(counts.ensure((size_t)(N + 1) * 4));
        TRY(runs.ensure(4));
        TRY(t.span_rows.ensure((size_t)N * 4));
        hipLaunchKernelGGL(iota_rows_kernel, dim3(grid), dim3(256), 0, 0, iota.as<int32_t>(), N);
        // ids lie in [0, 2^31 - 1): 31 key bits.  The sort is stable, so a group's rows stay ascending.
        size_t bytes = 0;
        const uint32_t *kin = t.by_row.as<uint32_t>();
        HIPCHECK(rocprim::radix_sort_pairs(nullptr, bytes, kin, keys.as<uint32_t>(), iota.as<int32_t>(),
                                           t.span_rows.as<int32_t>(), (size_t)N, 0u, 31u, (hipStream_t) nullptr));
        TRY(tmp.ensure(bytes > 0 ? bytes : 1));
        HIPCHECK(rocprim::radix_sort_pairs(tmp.p, bytes, kin, keys.as<uint32_t>(), iota.as<int32_t>(),
                                           t.span_rows.as<int32_t>(), (size_t)N, 0u, 31u, (hipStream_t) nullptr));
        HIPCHECK(hipMemset(counts.p, 0, (size_t)(N + 1) * 4));
        size_t rle = 0;
        HIPCHECK(rocprim::run_length_encode(nullptr, rle, keys.as<uint32_t>(), (unsigned)N, uniq.as<uint32_t>(),
                                            counts.as<int>(), runs.as<int>(), (hipStream_t) nullptr));
        TRY(tmp.ensure(rle > 0 ? rle : 1));
        HIPCHECK(rocprim::run_length_encode(tmp.p, rle, keys.as<uint32_t>(), (unsigned)N, uniq.as<uint32_t>(),
                                            counts.as<int>(), runs.as<int>(), (hipStream_t) nullptr));
        int G = 0;
        HIPCHECK(hipMemcpy(&G, runs.p, 4, hipMemcpyDeviceToHost));
        if (G < 1 || G > N) return fail(TK_ERR_HIP, "rows by group: the run-length encoding gave no group count");
        TRY(t.span_gid.ensure((size_t)G * 4));
        TRY(t.span_off.ensure((size_t)(G + 1) * 4));
        HIPCHECK(hipMemcpy(t.span_gid.p, uniq.p, (size_t)G * 4, hipMemcpyDeviceToDevice));
        size_t scan = 0;
        if (tk_scan_exclusive(nullptr, &scan, nullptr, nullptr, G + 1, 0)) return fail(TK_ERR_HIP, "scan size query");
        TRY(tmp.ensure(scan > 0 ? scan : 1));
        // (counts[G] is the zero of the memset: entry G of the scan is N)
        if (tk_scan_exclusive(tmp.p, &scan, counts.as<int>(), t.span_off.as<int>(), G + 1, 0))
            return fail(TK_ERR_HIP, "scan");
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        t.span_groups = G;
        return TK_OK;
    };
    const int rc = run();
    for (DevBuf *b : {&keys, &iota, &uniq, &counts, &runs, &tmp}) b->release();
    if (rc != TK_OK) return rc;
    t.span_state.made(t.set_gen);
    return TK_OK;
}
