// value_rows.hip — the rows in value order, on the device (TkRowTable::span_rows of the values; what value_exact.hip
// walks).  For every value column c a plane of N int32: the row ids ascending by (key of column c, row
// id), so the rows whose key lies in [lo, hi] are one contiguous span of the plane.  rocPRIM's radix sort over (key,
// row) pairs — the int64 keys by row id as tk_index_set_values uploaded them, all 64 bits, signed, stable — of which
// only the row ids are kept: 4 N bytes per column; the span lookup reads a key through its row id.  The library's
// kernels are instantiated in this file alone (its onesweep kernel uses scratch; no kernel of ours does).
#include <rocprim/device/device_radix_sort.hpp>

#include "api_internal.h"

__global__ __launch_bounds__(256) void value_iota_kernel(int32_t *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
}

// The rows in value order for the values the index has now, every column at once: made on the first call that needs
// them, and again after tk_index_set_values; they follow the values, not the lists.  Work memory (freed before it
// returns): the sorted keys of one column, the row ids going in and the library's own — about 24 N bytes beside the
// 4 N per column that stay.
int value_rows_ensure(tk_index *ix)
{
    TkRowTable &t = ix->values;
    TRY(row_table_covers(ix, t));
    if (t.span_state.current(t.set_gen)) return TK_OK;
    TRY(table_may_build(ix, "rows-by-value", "tk_index_knn_between"));
    ARGCHECK(ix->N < 0x7ffffff0ll, "rows by value: N < 2^31");
    t.span_state.ok = false;
    const int64_t N = ix->N;
    const int C = value_columns(ix);
    DevBuf keys, iota, tmp;
    auto run = [&]() -> int {
        TRY(keys.ensure((size_t)N * 8));
        TRY(iota.ensure((size_t)N * 4));
        TRY(t.span_rows.ensure((size_t)C * (size_t)N * 4));
        hipLaunchKernelGGL(value_iota_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, iota.as<int32_t>(), N);
        for (int c = 0; c < C; c++) {
            const int64_t *kin = t.by_row.as<int64_t>() + (size_t)c * (size_t)N;
            int32_t *out = t.span_rows.as<int32_t>() + (size_t)c * (size_t)N;
            size_t bytes = 0;
            HIPCHECK(rocprim::radix_sort_pairs(nullptr, bytes, kin, keys.as<int64_t>(), iota.as<int32_t>(), out,
                                               (size_t)N, 0u, 64u, (hipStream_t) nullptr));
            TRY(tmp.ensure(bytes > 0 ? bytes : 1));
            HIPCHECK(rocprim::radix_sort_pairs(tmp.p, bytes, kin, keys.as<int64_t>(), iota.as<int32_t>(), out,
                                               (size_t)N, 0u, 64u, (hipStream_t) nullptr));
        }
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipDeviceSynchronize());
        t.span_groups = C;
        return TK_OK;
    };
    const int rc = run();
    for (DevBuf *b : {&keys, &iota, &tmp}) b->release();
    if (rc != TK_OK) return rc;
    t.span_state.made(t.set_gen);
    return TK_OK;
}
