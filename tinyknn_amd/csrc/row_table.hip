// row_table.hip — the host side that the per-row tables share (TkRowTable, api_internal.h: the groups of groups.hip, the
// tags of tags.hip, the values of between.hip; their kernels stay in those files).  The error texts name the kind by the nouns it carries.
#include "api_internal.h"

int table_may_build(const tk_index *ix, const char *table, const char *call)
{
    ARGCHECK(ix->have_lists && ix->have_data, "index has no lists / data yet");
    ARGCHECK(!ix->capturing, std::string("the ") + table + " table cannot be made inside a stream capture: make one " +
                                 call + " call before the capture");
    return TK_OK;
}

int row_table_set(tk_index *ix, TkRowTable &t, const void *vals, int64_t n, int (*check)(const void *vals, int64_t n),
                  size_t esz)
{
    const std::string nouns = std::string(t.noun) + "s", unit = t.unit;
    ARGCHECK(n >= 0 && (n == 0 || vals), nouns + ": n " + unit + "s, or NULL and 0");
    ARGCHECK(!ix->sharded, "list-sharded index: row " + nouns + " are not supported");
    if (n > 0) {
        ARGCHECK(ix->have_data && n == ix->N, nouns + ": one " + unit + " per row of the index (n == N)");
        if (check) TRY(check(vals, n));
    }
    TRY(flush_pending(ix));                 // calls still owed that read the old values are enqueued ...
    HIPCHECK(hipDeviceSynchronize());       // ... and have run
    t.state.ok = false;
    t.span_state.ok = false;                // (the rows by group follow the values, not the lists)
    t.set_gen++;
    t.n = 0;
    if (n == 0) {
        for (DevBuf *b : {&t.by_row, &t.table, &t.span_rows, &t.span_gid, &t.span_off}) b->release();
        return TK_OK;
    }
    if (esz) t.esz = esz;                   // (a kind whose element size is fixed when it is set: between.hip)
    TRY(t.by_row.ensure((size_t)n * t.esz));
    HIPCHECK(hipMemcpy(t.by_row.p, vals, (size_t)n * t.esz, hipMemcpyHostToDevice));
    t.n = n;
    return TK_OK;
}

// What every call that names an array of the kind needs: the kind's values by row id, for all N rows
int row_table_covers(const tk_index *ix, const TkRowTable &t)
{
    if (t.n == 0 || t.n != ix->N) {
        const std::string noun = t.noun, nouns = noun + "s";
        if (t.n == 0)
            return fail(TK_ERR_STATE, "a " + noun + " array was passed but the index has no " + nouns +
                                          ": tk_index_set_" + nouns + " first");
        return fail(TK_ERR_STATE, "the " + nouns + " cover " + std::to_string(t.n) + " rows, the index has " +
                                      std::to_string(ix->N) + " now: set them again (tk_index_set_" + nouns + ")");
    }
    return TK_OK;
}

// Made on the first call that names an array of the kind, and again after the lists changed: once per layout.
int row_table_ensure(tk_index *ix, TkRowTable &t, void (*launch)(const tk_index *ix))
{
    TRY(row_table_covers(ix, t));
    if (t.state.current(ix->lists_gen)) return TK_OK;
    TRY(table_may_build(ix, t.noun, t.called));
    t.state.ok = false;
    TRY(t.table.ensure((size_t)(ix->total_chunks > 0 ? ix->total_chunks : 1) * 16 * t.esz));
    if (ix->n_lists > 0) launch(ix);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    t.state.made(ix->lists_gen);
    return TK_OK;
}

int row_table_info(const tk_index *ix, const TkRowTable &t, int64_t *info4)
{
    const bool have = t.state.current(ix->lists_gen);
    info4[0] = have ? 1 : 0;
    info4[1] = have ? (ix->total_chunks > 0 ? ix->total_chunks : 1) * 16 * (int64_t)t.esz : 0;
    info4[2] = t.state.builds;
    info4[3] = t.n * (int64_t)t.esz;
    return TK_OK;
}
