"""Chains of IVF.add / remove / update on the GPU, on the awkward indexes of tests/list_chain_shapes.py: the four kernels
that rewrite a built index in place (devbuild.hip: merge_lists_kernel, compact_lists_kernel, replace_lists_kernel,
scatter_rows_kernel, with keep_flags, scatter_kept, gather_scan and row_copies) on one-list indexes, lists of 0, 1 and
15-17 rows, a code array of one partial 8-chunk tile, M from 4 to 68, empty column blocks, float64 and half stores —
and from the layout the change before left: emptied lists refilled, removed rows stored again, added rows replaced and
removed, every row removed and rows added into the empty index, every later list's chunk offset shifted.
tests/test_list_chain_cpu.py shows that the default seeds hold these categories and holds the model (ListsModel)
against the host path first.

After EVERY step the device index is compared with the model and with a fresh upload of the model's lists and vectors
(byte for byte: sizes, codes with their padding rows, ids, centres, twin table, vectors — the empty index included,
which an upload accepts), and answers one batch as the guarded reference does over the model (ids, probes, heap
arrays; distances bit for bit against the upload).  In the middle and at the end of the chain every execution mode,
stored rows as queries, an allowed set and (seeds with groups) a grouped batch run too.  The row-position table and
the group table are compared there and not after every step: both are made lazily, by the first query_rows / group=
call of a layout, so a step without such a call has no table to compare; and the library shows their size only
(row_table(), group_table(): bytes, entries), their contents are witnessed by the answers of those calls.

Leg A: a host-built index with a device copy — assignment and codes come from the host, the kernels only move them.
Leg B: an index built in HBM (build_resident) — the device prepares, assigns and encodes the new rows itself.  What it
chose is read back off its lists and must reproduce them through the model; the vectors it stored are held against
the rows passed in, prepared on the host; the assignment against float64 distances and the labels against the
oracle's encoder, both from those host-prepared rows where the store is half."""
import contextlib
import os
import signal
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import list_chain_shapes as lc  # noqa: E402
from allowed_reference import guarded_batch  # noqa: E402
from groups_reference import grouped_batch  # noqa: E402
from rows_reference import excluded_batch  # noqa: E402
from store_reference import oracle_index, rounded  # noqa: E402
from test_build_path import _labels_same_up_to_exact_ties  # noqa: E402
from test_remove_gpu import _twins  # noqa: E402
from test_update_gpu import _ref_ivf  # noqa: E402
from update_reference import assignment_of_added  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("probes", "heap_idx", "heap_val")
MODES = ((0, 0), (1, 1), (2, 2), (0, 2), (3, 0))      # (heap_mode, scan_mode) as tests/test_fuzz_gpu.py
# A seed's budget on the Python side: the slowest default seeds take 2-3 s on an MI355X (profiles/r15/), the fresh
# uploads and the reference's Python replay included.  The alarm ends a seed whose Python side runs away (a reference
# loop that does not end, a chain that grows); it cannot interrupt a call blocked inside the library.
LIMIT = 30.0
SEEDS = list(lc.seeds())
RESIDENT_SEEDS = lc.resident_seeds(SEEDS)


@contextlib.contextmanager
def time_limit(seconds, what):
    def over(signum, frame):
        raise TimeoutError(f"{what}: more than {seconds:.0f} s")
    old = signal.signal(signal.SIGALRM, over)
    signal.setitimer(signal.ITIMER_REAL, seconds)
    try:
        yield
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)
        signal.signal(signal.SIGALRM, old)


def _same(got, gd, want, wd, msg):
    np.testing.assert_array_equal(got, want, err_msg=str(msg))
    for key in KEYS:
        np.testing.assert_array_equal(gd[key], wd[key], err_msg=f"{key} {msg}")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _lists_of(dev):
    """(ids per list, labels per list, padding labels per list) as the device holds them"""
    from tinyknn_amd._transform import unpack
    sizes, codes, ids = dev.export_lists()
    coff = np.concatenate([[0], np.cumsum((sizes + 15) // 16)])
    ioff = np.concatenate([[0], np.cumsum(sizes)])
    ids_l, lab_l, pad_l = [], [], []
    for i in range(len(sizes)):
        lab = unpack(codes[coff[i]:coff[i + 1]]) if sizes[i] else np.zeros((0, dev.M), np.uint8)
        ids_l.append(ids[ioff[i]:ioff[i + 1]].copy())
        lab_l.append(lab[:sizes[i]].copy())
        pad_l.append(lab[sizes[i]:].copy())
    return ids_l, lab_l, pad_l


def _assert_model(dev, m, msg, rows=True, cols_known=True):
    """the device's lists, columns, sizes, N and vectors are the model's — read directly, no upload between
    (cols_known=False: a host upload that no change has touched yet does not know its members per column)"""
    assert dev.N == m.N and dev.n_lists == m.L, msg
    np.testing.assert_array_equal(dev.list_sizes, m.sizes, err_msg=f"list_sizes {msg}")
    if cols_known:
        np.testing.assert_array_equal(dev.list_columns(), m.cols, err_msg=f"list_columns {msg}")
    else:
        assert dev.list_columns() is None, msg
    ids_l, lab_l, pad_l = _lists_of(dev)
    for l in range(m.L):
        np.testing.assert_array_equal(ids_l[l], m.ids[l], err_msg=f"ids of list {l} {msg}")
        np.testing.assert_array_equal(lab_l[l], m.labels[l], err_msg=f"codes of list {l} {msg}")
        assert len(pad_l[l]) == (-len(m.ids[l])) % 16 and (pad_l[l] == m.zero).all(), f"padding rows of list {l} {msg}"
    if rows and m.data.dtype == np.float32:     # (read_rows reads float32 and half stores)
        assert _bits(dev.read_rows(np.arange(m.N)), np.asarray(m.stored(), np.float32)), f"vectors {msg}"


def _assert_upload(dev, up, msg):
    """byte-identical to the fresh upload: lists, centres, twin table"""
    for name, x, y in zip(("sizes", "codes", "ids"), dev.export_lists(), up.export_lists()):
        assert _bits(x, y), f"export_lists: {name} {msg}"
    for name, x, y in zip(("centres", "centre codes"), dev.export_centers(), up.export_centers()):
        assert _bits(x, y), f"export_centers: {name} {msg}"
    assert dev.twin_table_width() == up.twin_table_width(), f"twin_table_width {msg}"
    np.testing.assert_array_equal(_twins(dev), _twins(up), err_msg=f"twin table {msg}")
    if dev.store != "float64":
        assert _bits(dev.read_rows(np.arange(dev.N)), up.read_rows(np.arange(up.N))), f"vectors against the upload {msg}"


def _restore(dev):
    dev.set_heap_mode(0)
    dev.set_scan_mode(0)
    dev.set_pipeline(1)


def _check(oracle, c, qn, qp, ref_of, dev, m, rng, msg, deep, fresh_rows, cols_known=True):
    """Everything asserted after a step.  c: the shape (k, n_probes); qn, qp: the prepared queries; ref_of(m) -> the
    IVF a fresh upload and the oracle take (the model's lists and vectors); deep: the mode sweep, stored rows as
    queries, an allowed set, groups; fresh_rows: ids the step just stored (for the stored-row queries)."""
    from tinyknn_amd.ivf import DeviceIndex
    k, p = c["k"], c["n_probes"]
    _assert_model(dev, m, msg, cols_known=cols_known)
    ref = ref_of(m)
    ox = oracle_index(oracle, ref, np.asarray(m.stored()))
    want, wd = guarded_batch(oracle, ox, qn, k, p, debug=True)
    got, gd = dev.query_batch(qn, qp, k, p, debug=True)
    _same(got, gd, want, wd, msg)
    empty = m.sizes.sum() == 0
    if empty:
        assert (got == -1).all() and (want == -1).all(), msg
        assert dev.twin_table_width() == 0 or _twins(dev).size == 0, msg
    up = DeviceIndex(ref)           # (with no stored row too: tk_index_set_lists takes sizes that are all 0)
    try:
        _assert_upload(dev, up, msg)
        ia, da = dev.query_batch(qn, qp, k, p, return_distances=True)
        ib, db = up.query_batch(qn, qp, k, p, return_distances=True)
        np.testing.assert_array_equal(ia, want, err_msg=msg)
        np.testing.assert_array_equal(ib, want, err_msg=f"the upload {msg}")
        assert _bits(da, db), f"distances {msg}"
        if not deep:
            return
        try:
            for heap_mode, scan_mode in MODES:
                dev.set_heap_mode(heap_mode)
                dev.set_scan_mode(scan_mode)
                got, gd = dev.query_batch(qn, qp, k, p, debug=True)
                _same(got, gd, want, wd, f"heap_mode={heap_mode} scan_mode={scan_mode} {msg}")
            dev.set_heap_mode(0)
            dev.set_scan_mode(0)
            dev.set_pipeline(2)
            for _ in range(2):
                np.testing.assert_array_equal(dev.query_batch(qn, qp, k, p), want, err_msg=f"pipelined {msg}")
        finally:
            _restore(dev)
        # an allowed set over the current N
        mask = rng.rand(m.N) < 0.5
        got, gd = dev.query_batch(qn, qp, k, p, debug=True, allowed=mask)
        w2, wd2 = guarded_batch(oracle, ox, qn, k, p, allowed=mask, debug=True)
        _same(got, gd, w2, wd2, f"allowed {msg}")
        if empty:
            return
        # stored rows as queries: rows the step just stored among them
        stored = m.stored_ids()
        fresh = np.intersect1d(np.asarray(fresh_rows, np.int64), stored)
        rows = np.concatenate([fresh[:8], rng.choice(stored, 16 - min(8, len(fresh)))]).astype(np.int64)
        rq, rp = dev.gather_queries(rows)
        if m.data.dtype == np.float32:
            assert _bits(rq, np.asarray(m.stored(), np.float32)[rows]), f"gather_queries {msg}"
        w3, wd3 = excluded_batch(oracle, ox, rq, rows, k, p, q_pq=rp if dev.rotated() else None, debug=True)
        got, gd = dev.query_rows(rows, k, p, debug=True)
        _same(got, gd, w3, wd3, f"query_rows {msg}")
        assert not (got == rows[:, None]).any(), f"a row returned itself {msg}"
        np.testing.assert_array_equal(up.query_rows(rows, k, p), w3, err_msg=f"query_rows of the upload {msg}")
        ta, tb = dev.row_table(), up.row_table()
        assert ta["built"] and tb["built"] and (ta["bytes"], ta["entries"]) == (tb["bytes"], tb["entries"]), (ta, tb, msg)
        if m.groups is not None:
            assert dev.groups_set() == m.N, msg
            up.set_groups(m.groups)
            group = rng.randint(-1, 5, size=len(qn)).astype(np.int32)
            group[0] = rng.randint(0, 5)        # (a group array of only -1 restricts nothing: no table is made)
            w4, wd4 = grouped_batch(oracle, ox, qn, group, m.groups, k, p, debug=True)
            got, gd = dev.query_batch(qn, qp, k, p, debug=True, group=group)
            _same(got, gd, w4, wd4, f"group {msg}")
            np.testing.assert_array_equal(up.query_batch(qn, qp, k, p, group=group), w4, err_msg=f"group, upload {msg}")
            ga, gb = dev.group_table(), up.group_table()
            assert ga["built"] and gb["built"], (ga, gb, msg)
            assert (ga["bytes"], ga["row_bytes"]) == (gb["bytes"], gb["row_bytes"]), (ga, gb, msg)
    finally:
        up.close()


def _deep_steps(n):
    """the two steps with the full set of checks: the middle of the chain and its end"""
    return {n // 2 - 1 if n >= 2 else 0, n - 1}


# ---- leg A ----

def _host_chain(oracle, seed):
    case = lc.case(seed)
    if case.skipped:
        pytest.skip(case.skipped)
    ivf, m = case.fresh_ivf(), case.model()
    built_L = m.L
    rng = np.random.RandomState(lc.STREAM + 400000 + seed)
    c, qn, qp = case.shape, case.qn, case.qp

    def ref_of(m):
        return _ref_ivf(ivf, (m.ids, m.labels), m.data, m.zero, L1=m.L if m.L > built_L else None)

    dev = ivf.device_index()        # BEFORE the chain: every change below runs on the device
    try:
        _check(oracle, c, qn, qp, ref_of, dev, m, rng, f"{case} before the chain", False, (), cols_known=False)
        deep = _deep_steps(len(case.ops))
        touched = False         # has a change rewritten the lists yet?  (a removal that names nothing stored does not)
        for i, op in enumerate(case.ops):
            msg = f"{case} after step {i} of {[(o['kind'], o['sel']) for o in case.ops]}"
            assert lc.apply_to_ivf(ivf, op) is ivf
            assert ivf.device_index() is dev, msg
            stored = m.sizes.sum()
            m.apply(op)
            touched |= op["kind"] != "remove" or m.sizes.sum() != stored
            lc.assert_host_lists(ivf, m, msg)       # the host mirror, read back off the device
            if op["kind"] == "update" and m.data.dtype == np.float32:
                assert _bits(dev.read_rows(op["ids"]), np.asarray(m.stored(), np.float32)[op["ids"]]), f"new rows {msg}"
            fresh = () if op["kind"] == "remove" else (op["ids"] if op["kind"] == "update"
                                                        else np.arange(m.N - len(op["X"]), m.N))
            _check(oracle, c, qn, qp, ref_of, dev, m, rng, msg, i in deep, fresh, cols_known=touched)
    finally:
        dev.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_chain_on_a_host_built_index(oracle, seed):
    with time_limit(LIMIT, f"host-built seed {seed}"):
        _host_chain(oracle, seed)


# ---- leg B ----

def _assignment_of(dev, op, N0):
    """(nearest (n, kp), labels (n, M)) the device gave the rows of `op`, read off its lists: a new row sits in list
    nearest[i, j]'s column-j block, once per column, and carries labels[i] there."""
    ids_l, lab_l, _ = _lists_of(dev)
    cols = dev.list_columns()
    if op["kind"] == "add":
        return assignment_of_added((ids_l, lab_l, cols), N0, len(op["X"]))
    ids = op["ids"]
    kp = cols.shape[1]
    at = np.full(int(ids.max()) + 1, -1, np.int64)
    at[ids] = np.arange(len(ids))
    nearest = np.full((len(ids), kp), -1, np.int64)
    labels = np.zeros((len(ids), dev.M), np.uint8)
    for l in range(len(ids_l)):
        a = ids_l[l]
        col_of = np.repeat(np.arange(kp), cols[l])
        sel = np.flatnonzero((a < len(at)) & (at[np.minimum(a, len(at) - 1)] >= 0))
        assert (nearest[at[a[sel]], col_of[sel]] == -1).all(), "a replaced row sits twice in one column"
        nearest[at[a[sel]], col_of[sel]] = l
        labels[at[a[sel]]] = lab_l[l][sel]
    assert (nearest >= 0).all(), "a replaced row is missing from a column"
    return nearest, labels


EPS = 2.0 ** -24        # the unit roundoff of float32


def _norm_err(d):
    """The relative error of a float32 row normalised in float32, whatever the order of the sum: d products and d - 1
    additions for the squared norm (at most d eps relative, all terms positive), half of that through the root, one
    rounding each for root and quotient, and room for a reciprocal root of a few ulp in place of the pair."""
    return (d / 2 + 8) * EPS


def _host_prepared(res, X):
    """the rows as add / update prepare them, on the host: float32, normalised in float32 for angular"""
    x = np.ascontiguousarray(X, dtype=np.float32)
    if res.metric == "angular":
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return x


def _assert_stored_rows(res, half, X, read, msg):
    """The vectors the device stored for the rows X it was given, against X prepared on the host.  Euclidean rows are
    stored as they are: bit for bit (a half store: float16 of them, round to nearest even).  Angular rows are
    normalised on the device: two float32 normalisations of one row differ by at most 2 _norm_err(d) |x|; a half
    store adds half a unit of the half's last place, 2^-11 |x|, or 2^-25 below the normal halfs."""
    prep = _host_prepared(res, X)
    if res.metric != "angular":
        assert _bits(read, rounded(prep) if half else prep), f"stored rows differ from the rows passed in {msg}"
        return
    tol = 2 * _norm_err(prep.shape[1]) * np.abs(prep)
    if half:
        tol = tol + 2.0 ** -11 * np.abs(prep) * (1 + 2 * _norm_err(prep.shape[1])) + 2.0 ** -25
    worst = np.abs(read.astype(np.float64) - prep.astype(np.float64)) - tol
    assert (worst <= 0).all(), f"stored rows differ from the normalised rows passed in by {worst.max()} past the bound {msg}"


def _assert_assignment(ivf, rows, nearest, msg, rows_err=0.0):
    """The kp centres the device chose are the kp nearest in float64, in order, up to what float32 arithmetic can
    tell apart: |x - y|^2 is formed there from |x|^2 + |y|^2 - 2 x.y, d + 2 roundings of terms bounded by
    |x|^2 + |y|^2, so two centres whose float64 distances differ by less than B = 4 (d + 2) 2^-24 (|x|^2 + max |y|^2)
    are a tie.  rows: the prepared rows the device searched with (float32), or (rows_err > 0) rows within the relative
    error rows_err of them: a distance then moves by at most 2 |x - y| rows_err |x| <= rows_err (3 |x|^2 + |y|^2),
    and two by twice that."""
    X = np.asarray(rows, np.float64)
    Y = np.asarray(ivf.all_centers, np.float32)
    if ivf.metric == "angular":
        Y = Y / np.linalg.norm(Y, axis=1, keepdims=True)
    Y = Y.astype(np.float64)
    d2 = ((X[:, None, :] - Y[None]) ** 2).sum(axis=2)
    scale = (X ** 2).sum(axis=1) + (Y ** 2).sum(axis=1).max()
    B = 4 * (X.shape[1] + 2) * EPS * scale + 2 * rows_err * 3 * scale
    chosen = np.take_along_axis(d2, nearest, axis=1)
    assert (np.diff(chosen, axis=1) >= -B[:, None]).all(), f"the chosen centres are out of order {msg}"
    rest = d2.copy()
    np.put_along_axis(rest, nearest, np.inf, axis=1)
    assert (chosen[:, -1] <= rest.min(axis=1) + B).all(), f"a nearer centre was passed over {msg}"
    assert all(len(set(r)) == len(r) for r in nearest.tolist()), f"a centre chosen twice {msg}"


def _assert_labels(oracle, ivf, rows, labels, msg, rows_err=0.0):
    """The device's PQ labels against the oracle's encoder over the same prepared rows, padded and rotated as
    FastPQ.transform does; at most 1e-5 of them + 2 may differ at all.
    Unrotated codes from the very rows the device coded (rows_err = 0): as tests/test_build_gpu.py holds the build —
    a differing label must be an EXACT tie of the minimum in numpy's own float32 `part`.
    Otherwise exact float32 ties are not the right rule, and a bound takes their place: a differing label's centroid
    must be within tol of the nearest in float64.  A rotated PQ is coded from float64 values which the device makes
    with its own chain of FMAs where numpy calls DGEMM (IVF.build_resident's docstring): each rotated coordinate
    within (dq + 2) 2^-53 |x| of the other, so a block distance within 2^-40 (|x|^2 + max |c|^2).  Rows only known
    within rows_err (a half store of normalised rows): a block moves by at most rows_err |x| and its distance to a
    centroid by 2 |x_b - c| rows_err |x| <= 2 rows_err (|x|^2 + max |c|^2); unrotated, the float32 sums of the search
    add 8 * 2^-24 * (|x_b|^2 + max |c|^2)."""
    pq = ivf.pq
    dpb = pq.dims_per_block
    X = np.asarray(rows, np.float32)
    pad = (-X.shape[1]) % (4 * dpb)
    Xp = np.concatenate([X, np.zeros((len(X), pad), X.dtype)], axis=1)
    if pq.R is not None:
        Xp = Xp @ pq.R.T
    Xp = np.ascontiguousarray(Xp)
    want = oracle.encode_pq(pq.centers, dpb, Xp)
    if pq.R is None and rows_err == 0.0:
        _labels_same_up_to_exact_ties(pq.centers, dpb, Xp, labels, want)
        return
    bad = np.argwhere(want != labels)
    assert len(bad) <= 1e-5 * want.size + 2, f"{len(bad)} labels differ {msg}"
    x2 = (np.asarray(X, np.float64) ** 2).sum(axis=1)
    for i, b in bad:
        xb = np.asarray(Xp[i, b * dpb:(b + 1) * dpb], np.float64)
        cb = np.asarray(pq.centers[:, b * dpb:(b + 1) * dpb], np.float64)
        part = ((xb[None] - cb) ** 2).sum(axis=1)
        c2 = (cb ** 2).sum(axis=1).max()
        tol = 2 * 2 * rows_err * (x2[i] + c2)
        tol += 2.0 ** -40 * (x2[i] + c2) if pq.R is not None else 8 * EPS * ((xb ** 2).sum() + c2)
        assert part[labels[i, b]] <= part.min() + tol, f"row {i} block {b}: not a nearest centroid {msg}"


def _resident_index(case, seed):
    """An index built in HBM over the generator's own rows for this seed's shape, centres and codebook fitted on
    exactly those rows (tinyknn_amd.ivf.synth_rows gives the host the rows the device generates), so that every
    centre has rows of its own."""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import synth_rows
    c = lc.resident_shape(seed)
    cent = np.ascontiguousarray(case.cent, dtype=np.float32)
    gen = lc.STREAM + seed
    X0 = synth_rows(c["n"], c["d"], gen, cent, 0.5)
    res = IVF(c["metric"], c["n_clusters"], FastPQ(2) if c["rotate"] else FastPQ(2, rotate_dim=None))
    state = np.random.get_state()
    np.random.seed(lc.STREAM + 600000 + seed)
    try:
        res.fit(X0)
    finally:
        np.random.set_state(state)
    try:
        res.build_resident(c["n"], c["d"], gen, cent, 0.5, n_probes=c["build_probes"],
                           store="float16" if c["store"] == "float16" else None)
    except AssertionError as e:     # (k-means can still leave a centre without a row of its own: the reference's refusal)
        assert "utils.py:128" in str(e), e
        pytest.skip("the device build rejects this shape exactly as the reference does")
    return res, c


def _resident_chain(oracle, seed):
    case = lc.case(seed)
    if case.skipped:
        pytest.skip(case.skipped)
    res, c = _resident_index(case, seed)
    half = c["store"] == "float16"
    dev = res.device_index()
    if dev.n_lists != c["n_clusters"]:
        dev.close()
        pytest.skip("inactive centres: the reference's grouping asserts on them")
    rng = np.random.RandomState(lc.STREAM + 500000 + seed)
    qn, qp = res._prepare(case.qs.copy())
    qn, qp = np.ascontiguousarray(qn), np.ascontiguousarray(qp)
    ids_l, lab_l, _ = _lists_of(dev)
    # (the vectors as the store gives them back: a half store's are rounded already)
    m = lc.ListsModel(ids_l, lab_l, dev.list_columns(), dev.read_rows(np.arange(dev.N)),
                      lc.zero_labels_of(res.pq, c["d"], np.float32))
    built_L = m.L

    def ref_of(m):
        ref = _ref_ivf(res, (m.ids, m.labels), m.data, m.zero, L1=m.L if m.L > built_L else None)
        ref.store = "float16" if half else None
        return ref

    try:
        _check(oracle, c, qn, qp, ref_of, dev, m, rng, f"resident {case} before the chain", False, ())
        n_ops = c["n_ops"]
        plan = [None] * n_ops
        if c["steered"]:
            plan.insert(0, "edges")
        if c["empty_then_add"]:
            at = int(rng.randint(1 if c["steered"] else 0, len(plan) - 1))
            plan[at:at + 2] = ["remove", "add"]
        deep = _deep_steps(len(plan))
        done = []
        for i, force in enumerate(plan):
            if force == "edges":
                op = dict(kind="remove", sel="edges", ids=lc.edge_removal(m, rng), X=None, groups=None)
            else:
                op = lc.draw_op(case, m, rng, {}, force=force, prepare=False)
            if op["X"] is not None:
                op["X"] = np.ascontiguousarray(op["X"], dtype=np.float32)
            done.append((op["kind"], op["sel"]))
            msg = f"resident {case} after step {i} of {done}"
            N0 = m.N
            assert lc.apply_to_ivf(res, op) is res
            if op["kind"] == "remove":
                m.remove(op["ids"])
                fresh = ()
            else:
                near, lab = _assignment_of(dev, op, N0)
                fresh = op["ids"] if op["kind"] == "update" else np.arange(N0, N0 + len(op["X"]))
                new = dev.read_rows(fresh)
                _assert_stored_rows(res, half, op["X"], new, msg)
                if op["kind"] == "add":
                    m.add(new, near, lab)
                else:
                    m.update(op["ids"], new, near, lab)
                # What the device searched and coded: float32 rows.  A float32 store holds exactly those (read back);
                # a half store holds their halfs, so the host's preparation of the rows passed in stands for them:
                # exact for euclidean, within two float32 normalisations for angular.
                if half:
                    err = 2 * _norm_err(c["d"]) if res.metric == "angular" else 0.0
                    _assert_assignment(res, _host_prepared(res, op["X"]), near, msg, rows_err=err)
                    _assert_labels(oracle, res, _host_prepared(res, op["X"]), lab, msg, rows_err=err)
                else:
                    _assert_assignment(res, new, near, msg)
                    _assert_labels(oracle, res, new, lab, msg)
            np.testing.assert_array_equal(res.list_columns, m.cols, err_msg=msg)
            np.testing.assert_array_equal(res.list_sizes, m.sizes, err_msg=msg)
            _check(oracle, c, qn, qp, ref_of, dev, m, rng, msg, i in deep, fresh)
    finally:
        dev.close()


@pytest.mark.parametrize("seed", RESIDENT_SEEDS)
def test_chain_on_a_resident_index(oracle, seed):
    with time_limit(LIMIT, f"resident seed {seed}"):
        _resident_chain(oracle, seed)
