"""The exact search inside a query's value range (tk_index_knn_between) against its reference
(tests/between_exact_reference.py): ids and distance bits equal on every case, range_sizes equal to the span model.
Every store and width, span lengths at the edges of k, of the tile and of the candidate buffer, span ends on every
awkward key, one to four columns, ties, every restriction, the lists changing under it, and IVF.query_batch(between=,
exact_below=)."""
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from between_exact_reference import knn_between_reference, span_model, value_order  # noqa: E402
from between_exact_shapes import (DUP_ROWS, K, MAX, MIN, columns, dups, edges, everything, extremes, floats,  # noqa: E402
                                  narrow_dtypes, ties, wide_and_narrow)
from brute_restricted_reference import passes  # noqa: E402
from conftest import golden  # noqa: E402
from group_exact_reference import append_model, einsum_distances, reference_data, same_bits  # noqa: E402
from test_group_exact_gpu import _index  # noqa: E402

pytestmark = pytest.mark.gpu


def _cut(between, rows):
    return tuple(None if b is None else np.asarray(b)[rows] for b in between)


def _check(oracle, got, qn, data, k, between, values, stored=None, einsum=True, **restrictions):
    """a (ids, dist) answer against the reference: ids, distance bits, dtype; numpy's einsum within 1 ulp"""
    ids, dist = got
    want_ids, want_dist = knn_between_reference(oracle, qn, data, k, between, values, stored=stored, **restrictions)
    assert ids.dtype == np.int64 and ids.shape == (len(qn), k)
    np.testing.assert_array_equal(ids, want_ids)
    assert dist.dtype == want_dist.dtype and same_bits(dist, want_dist)
    assert np.isposinf(dist[ids < 0]).all()
    if einsum and (ids >= 0).any():
        live = ids >= 0
        np.testing.assert_array_max_ulp(dist[live], einsum_distances(qn, data, ids)[live], maxulp=1)
    return ids, dist


def _sizes(dev, f):
    """range_sizes against the span model -> (len, col)"""
    length, col = dev.range_sizes(f["between"], f["nq"])
    want_len, want_col = span_model(f["values"], f["between"], f["nq"])
    assert length.dtype == np.int64 and col.dtype == np.int32
    np.testing.assert_array_equal(length, want_len, err_msg=f["name"])
    np.testing.assert_array_equal(col, want_col, err_msg=f["name"])
    return length, col


def _run_fixture(oracle, f, ks=(K,), d=12):
    """An index over random rows with the fixture's values: range_sizes is the model's, and the queries that bound a
    column are answered as the reference answers them.  -> (dev, Y, X, the bounded queries, ids at the last k)"""
    rng = np.random.RandomState(zlib.crc32(f["name"].encode()) % 2**31)
    values, between, nq = f["values"], f["between"], f["nq"]
    n = len(values)
    Y = rng.randn(n, d).astype(np.float32)
    X = rng.randn(nq, d).astype(np.float32)
    dev = _index(Y)
    dev.set_values(values)
    length, col = _sizes(dev, f)
    rows = np.flatnonzero(col >= 0)
    ids = None
    for k in ks:
        got = dev.knn_between(X[rows], k, _cut(between, rows), return_distances=True)
        ids, _ = _check(oracle, got, X[rows], Y, k, _cut(between, rows), values)
        # the span bounds what passes; with one column (nothing removed, no other restriction) it is what passes
        found = (ids >= 0).sum(axis=1)
        assert (found <= np.minimum(k, length[rows])).all(), f["name"]
        if np.ndim(values) == 1:
            np.testing.assert_array_equal(found, np.minimum(k, length[rows]), err_msg=f["name"])
    info = dev.value_rows()
    cols = 1 if np.ndim(values) == 1 else np.shape(values)[1]
    assert info == dict(built=True, bytes=4 * n * cols, builds=1, columns=cols), info
    return dev, Y, X, rows, ids


# ---- 1. stores and widths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", [None, "float16"])
@pytest.mark.parametrize("d", [1, 20, 100, 127, 128])
def test_stores_and_widths(oracle, store, d):
    rng = np.random.RandomState(2000 + d)
    n = 3000
    Y = rng.randn(n, d).astype(np.float32)
    dev = _index(Y, store)
    values = rng.randint(0, 10**9, size=n).astype(np.int64)      # a timestamp
    dev.set_values(values)
    ref = reference_data(Y, store)
    assert dev.value_rows() == dict(built=False, bytes=0, builds=0, columns=0)
    for nq, k in ((0, K), (1, K), (4, 1), (4, K), (4, 100), (4, 1024), (1000, K)):
        X = rng.randn(nq, d).astype(np.float32)
        lo = rng.randint(0, 10**9, size=nq).astype(np.int64)
        hi = lo + (10**9 * rng.choice([0.002, 0.01, 0.1, 0.5], size=nq)).astype(np.int64)
        if nq:
            X[0] = Y[5]                                 # a query on a row, inside its window
            lo[0], hi[0] = values[5] - 10**7, values[5] + 10**7
        if nq == 4:
            lo[1], hi[1] = 0, 10**9                     # every row
        _check(oracle, dev.knn_between(X, k, (lo, hi), return_distances=True), X, ref, k, (lo, hi), values)
        np.testing.assert_array_equal(dev.knn_between(X, k, (lo, hi)),
                                      knn_between_reference(oracle, X, ref, k, (lo, hi), values)[0])
        if nq:
            _sizes(dev, dict(name="timestamps", values=values, between=(lo, hi), nq=nq))
    assert dev.value_rows() == dict(built=True, bytes=4 * n, builds=1, columns=1)


def test_float64_vectors_on_the_fixture(oracle):
    from store_reference import fixture_ivf
    g = golden("g6_ivf_eu20f64.npz")
    ivf = fixture_ivf(g)
    data, qn = g["data"], np.ascontiguousarray(g["qn"], dtype=np.float32)
    assert data.dtype == np.float64
    n = len(data)
    dev = ivf.device_index()
    rng = np.random.RandomState(64)
    values = np.stack([rng.randn(n), rng.randint(0, 50, size=n)], axis=1)          # float64 columns
    dev.set_values(values)
    stored = np.zeros(n, dtype=bool)
    stored[np.concatenate([np.asarray(i) for i in ivf.ids])] = True
    for k in (1, K, 100, min(1024, n)):
        q = qn[:40] if k > 100 else qn
        lo = np.stack([rng.randn(len(q)) - 1, rng.randint(0, 40, size=len(q)).astype(np.float64)], axis=1)
        hi = lo + np.stack([rng.rand(len(q)) * 3, rng.randint(0, 30, size=len(q)).astype(np.float64)], axis=1)
        lo[::3, 0], hi[::3, 0] = -np.inf, np.inf            # column 1 alone
        lo[1::3, 1], hi[1::3, 1] = -np.inf, np.inf          # column 0 alone
        _, dist = _check(oracle, dev.knn_between(q, k, (lo, hi), return_distances=True), q, data, k, (lo, hi),
                         values, stored=stored)
        assert dist.dtype == np.float64
        _sizes(dev, dict(name="f64", values=values, between=(lo, hi), nq=len(q)))


# ---- 2. span lengths at the edges -------------------------------------------------------------------------------------
def test_span_lengths_at_the_edges(oracle):
    from tinyknn_amd import _lib
    assert (_lib.GROUP_EXACT_TILE, _lib.GROUP_EXACT_CAP) == (256, 2048)
    f, lengths = edges()
    rng = np.random.RandomState(8)
    values, between = f["values"], f["between"]
    Y = rng.randn(len(values), 20).astype(np.float32)
    X = rng.randn(f["nq"], 20).astype(np.float32)
    dev = _index(Y)
    dev.set_values(values)
    length, col = _sizes(dev, f)
    np.testing.assert_array_equal(length, lengths)
    assert (col == 0).all()
    for k in (1, K, 100):
        ids, dist = _check(oracle, dev.knn_between(X, k, between, return_distances=True), X, Y, k, between, values)
        np.testing.assert_array_equal((ids >= 0).sum(axis=1), np.minimum(k, lengths))
        assert np.isposinf(dist[lengths == 0]).all()
    # many queries in one window
    many = rng.randn(300, 20).astype(np.float32)
    window = (np.full(300, between[0][5]), np.full(300, between[1][5]))
    _check(oracle, dev.knn_between(many, K, window, return_distances=True), many, Y, K, window, values)


def test_every_row_in_one_window_and_the_buffer_is_cut_back(oracle):
    """N = 6000 rows in ONE window, and query 0 sees them in descending distance along the walk — which is in value
    order, not by row id: every row is within the bound when its lane looks, so the buffer of 2048 fills and is cut at
    least twice in front of tiles (the model of the appends, fed the distances in value order, says so)."""
    from tinyknn_amd import _lib
    tile, cap = _lib.GROUP_EXACT_TILE, _lib.GROUP_EXACT_CAP
    f = everything()
    values, between = f["values"], f["between"]
    rng = np.random.RandomState(10)
    n, d = len(values), 8
    order = value_order(values)
    assert not np.array_equal(order, np.arange(n))
    Y = rng.randn(n, d).astype(np.float32)
    Y[order, 0] = 10.0 + (n - np.arange(n)) * 0.25      # the first coordinate falls along the walk
    X = rng.randn(f["nq"], d).astype(np.float32)
    X[0] = 0
    X[0, 0] = -100.0
    dev = _index(Y)
    dev.set_values(values)
    length, col = _sizes(dev, f)
    assert (length == n).all() and (col == 0).all()
    for k in (K, 1024):
        dv = oracle.sqdist_gather(X[0], Y, order)
        assert (np.diff(dv) < 0).all()
        cuts, most = append_model(dv, k, tile, cap)
        assert cuts >= 2 and most <= cap, (cuts, most)
        assert append_model(oracle.sqdist_gather(X[1], Y, order), k, tile, cap)[1] <= cap
        ids, _ = _check(oracle, dev.knn_between(X, k, between, return_distances=True), X, Y, k, between, values)
        np.testing.assert_array_equal(ids[0], order[::-1][:k])


# ---- 3. span ends -----------------------------------------------------------------------------------------------------
def test_ends_on_keys_many_rows_carry(oracle):
    fs = dups()
    dev, Y, X, rows, _ = _run_fixture(oracle, fs[0], ks=(K, 400))
    length, _ = dev.range_sizes(fs[0]["between"], fs[0]["nq"])
    v = fs[0]["values"]
    assert length[0] == DUP_ROWS                                 # lo == hi on the key of 300 rows
    assert length[1] == np.sum((v >= 50) & (v <= 60)) and length[2] == np.sum((v >= 40) & (v <= 50))
    assert length[5] == length[1] - DUP_ROWS and length[6] == length[2] - DUP_ROWS      # upper against lower bound
    assert list(length[7:9]) == [0, 0] and list(length[11:13]) == [0, 0] and length[13] == len(v)
    for f in fs[1:]:
        _run_fixture(oracle, f)


def test_int64_extremes_as_values_and_bounds(oracle):
    f = extremes()
    dev, _, _, rows, _ = _run_fixture(oracle, f, ks=(K, 30))
    length, col = dev.range_sizes(f["between"], f["nq"])
    assert list(length[:5]) == [20, 20, 25, 25, 5] and (length[7], col[7]) == (len(f["values"]), -1)
    assert length[9] == 0 and 7 not in rows


@pytest.mark.parametrize("which", [0, 1])
def test_float_columns(oracle, which):
    f = floats()[which]
    dev, _, _, rows, _ = _run_fixture(oracle, f, ks=(K, 200))
    if which == 0:
        length, col = dev.range_sizes(f["between"], f["nq"])
        v = f["values"][:, 0]
        assert length[0] == length[1] == np.sum(v == 0) and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
        assert length[3] == np.sum(np.isneginf(v)) > 0 and length[4] == np.sum(np.isposinf(v)) > 0
        assert (col[7], col[8], length[9]) == (-1, 1, 0)


@pytest.mark.parametrize("which", [0, 1])
def test_float16_and_uint64_columns(oracle, which):
    _run_fixture(oracle, narrow_dtypes()[which])


# ---- 4. columns -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_one_to_four_columns(oracle, C):
    f = columns(C)
    dev, _, _, rows, _ = _run_fixture(oracle, f)
    _, col = dev.range_sizes(f["between"], f["nq"])
    assert col[-1] == -1 and len(rows) == f["nq"] - 1
    assert len(set(col[:-1])) == C                              # queries of one batch walk different columns


def test_the_narrow_column_is_walked_whichever_it_is(oracle):
    answers = []
    for narrow in (0, 1):
        f = wide_and_narrow(narrow)
        rng = np.random.RandomState(92)                 # the same vectors and queries for both
        Y = rng.randn(len(f["values"]), 12).astype(np.float32)
        X = rng.randn(f["nq"], 12).astype(np.float32)
        dev = _index(Y)
        dev.set_values(f["values"])
        assert (_sizes(dev, f)[1] == narrow).all()
        answers.append(_check(oracle, dev.knn_between(X, K, f["between"], return_distances=True), X, Y, K, f["between"],
                              f["values"]))
    np.testing.assert_array_equal(answers[0][0], answers[1][0])
    assert same_bits(answers[0][1], answers[1][1]) and (answers[0][0] >= 0).any()


def test_ties_in_length_go_to_the_lowest_column(oracle):
    f = ties()
    dev, _, _, _, _ = _run_fixture(oracle, f)
    length, col = dev.range_sizes(f["between"], f["nq"])
    assert (col == 1).all() and (length > 0).all()


# ---- 5. ties in distance ----------------------------------------------------------------------------------------------
def test_ties_in_distance(oracle):
    rng = np.random.RandomState(30)
    n, d = 4000, 16
    Y = rng.randn(n, d).astype(np.float32)
    values = rng.permutation(n).astype(np.int64)
    same = np.sort(rng.choice(n, size=300, replace=False))      # 300 identical rows, anywhere in the value order
    Y[same] = Y[same[0]]
    order = value_order(values)
    at = np.flatnonzero(np.isin(order, same))
    assert at.min() < 500 and at.max() > 3500 and not np.array_equal(order[at], same)
    # a window of 600 rows whose span positions 255 and 256 — across the tile border — are twins
    b = 1000
    span = order[b:b + 600]
    free = [p for p in (255, 256) if span[p] not in same]
    assert len(free) == 2
    Y[span[256]] = Y[span[255]]
    X = np.stack([Y[same[0]], Y[span[255]]])
    between = (np.array([0, b], dtype=np.int64), np.array([n, b + 599], dtype=np.int64))
    dev = _index(Y)
    dev.set_values(values)
    np.testing.assert_array_equal(dev.range_sizes(between)[0], [n, 600])
    ids, dist = _check(oracle, dev.knn_between(X, K, between, return_distances=True), X, Y, K, between, values)
    np.testing.assert_array_equal(ids[0], same[:K])             # the lowest ids, wherever the walk met them
    assert (dist[0] == 0).all()
    np.testing.assert_array_equal(ids[1][:2], np.sort(span[255:257]))
    assert (dist[1][:2] == 0).all()


# ---- 6. restrictions --------------------------------------------------------------------------------------------------
_BASE = {}
TWIN_FAILS, TWIN_A, TWIN_B = 100, 200, 300      # three identical rows inside query 0's window: query 0 lies on them


def _base():
    if not _BASE:
        rng = np.random.RandomState(40)
        n, d, nq = 4000, 16, 67
        Y = rng.randn(n, d).astype(np.float32)
        Y[TWIN_A] = Y[TWIN_B] = Y[TWIN_FAILS]
        values = rng.randint(0, 10000, size=(n, 2)).astype(np.int64)
        values[[TWIN_FAILS, TWIN_A, TWIN_B], 0] = 5000
        X = rng.randn(nq, d).astype(np.float32)
        X[0] = Y[TWIN_FAILS]
        own = rng.choice(np.arange(400, n), size=nq, replace=False)
        X[1::2] = Y[own[1::2]]                          # every other query lies on a row inside its window
        lo = np.stack([values[own, 0] - rng.randint(0, 1500, size=nq), np.full(nq, MIN)], axis=1)
        hi = np.stack([values[own, 0] + rng.randint(0, 1500, size=nq), np.full(nq, MAX)], axis=1)
        lo[3::8, 1], hi[3::8, 1] = 1000, 9000           # some bound the second column too
        values[own[3::8], 1] = 5000
        lo[0], hi[0] = (4000, MIN), (6000, MAX)
        groups = rng.randint(0, 4, size=n).astype(np.int32)
        groups[[TWIN_FAILS, TWIN_A, TWIN_B]] = 2
        row_tags = np.array([sum(1 << int(b) for b in rng.choice(8, size=rng.randint(1, 4), replace=False))
                             for _ in range(n)], dtype=np.uint64)
        row_tags[TWIN_FAILS], row_tags[TWIN_A], row_tags[TWIN_B] = 0b0001, 0b0110, 0b0110
        dev = _index(Y)
        dev.set_values(values)
        dev.set_groups(groups)
        dev.set_tags(row_tags)
        _BASE.update(Y=Y, X=X, n=n, nq=nq, values=values, between=(lo, hi), own=own, groups=groups, row_tags=row_tags,
                     dev=dev)
    return _BASE


def _twins_answer(ids):
    assert TWIN_FAILS not in ids[0]
    np.testing.assert_array_equal(ids[0][:2], [TWIN_A, TWIN_B])


def test_nothing_but_the_ranges(oracle):
    b = _base()
    ids, _ = _check(oracle, b["dev"].knn_between(b["X"], K, b["between"], return_distances=True), b["X"], b["Y"], K,
                    b["between"], b["values"])
    np.testing.assert_array_equal(ids[0][:3], [TWIN_FAILS, TWIN_A, TWIN_B])
    assert (ids[1::2, 0] == b["own"][1::2]).all()


@pytest.mark.parametrize("as_ids", [False, True])
def test_allowed_alone(oracle, as_ids):
    b = _base()
    mask = np.random.RandomState(41).rand(b["n"]) < 0.3
    mask[TWIN_FAILS], mask[TWIN_A], mask[TWIN_B] = False, True, True
    got = b["dev"].knn_between(b["X"], K, b["between"], allowed=np.flatnonzero(mask) if as_ids else mask,
                               return_distances=True)
    _twins_answer(_check(oracle, got, b["X"], b["Y"], K, b["between"], b["values"], allowed=mask)[0])


def test_exclude_alone(oracle):
    b = _base()
    exclude = b["own"].copy()
    exclude[0] = TWIN_FAILS
    exclude[5::7] = -1
    got = b["dev"].knn_between(b["X"], K, b["between"], exclude=exclude, return_distances=True)
    ids, _ = _check(oracle, got, b["X"], b["Y"], K, b["between"], b["values"], exclude=exclude)
    _twins_answer(ids)
    assert ids[5][0] == b["own"][5] and ids[1][0] != b["own"][1]            # (kept where -1, gone where named)


def test_group_alone_with_unrestricted_entries(oracle):
    b = _base()
    rng = np.random.RandomState(42)
    group = rng.randint(-1, 5, size=b["nq"]).astype(np.int32)  # (-1: any group; 4: an id no row carries)
    group[0] = 2
    groups = b["groups"].copy()
    groups[TWIN_FAILS] = 1                                      # (the base's device groups are set again below)
    b["dev"].set_groups(groups)
    try:
        got = b["dev"].knn_between(b["X"], K, b["between"], group=group, return_distances=True)
        ids, _ = _check(oracle, got, b["X"], b["Y"], K, b["between"], b["values"], group=group, groups=groups)
    finally:
        b["dev"].set_groups(b["groups"])
    _twins_answer(ids)
    assert (group == -1).any() and (ids[group == 4] == -1).all() and (ids[group == -1] >= 0).any()
    assert b["dev"].group_rows()["builds"] == 0                 # the rows by group are knn_group's, not made here


@pytest.mark.parametrize("mode", ["any", "all"])
def test_tags_alone(oracle, mode):
    b = _base()
    rng = np.random.RandomState(43)
    tags = np.array([sum(1 << int(t) for t in rng.choice(8, size=rng.randint(1, 3), replace=False))
                     for _ in range(b["nq"])], dtype=np.uint64)
    tags[3::9] = 0
    tags[0] = 0b0110
    got = b["dev"].knn_between(b["X"], K, b["between"], tags=tags, tags_mode=mode, return_distances=True)
    _twins_answer(_check(oracle, got, b["X"], b["Y"], K, b["between"], b["values"], tags=tags, tags_mode=mode,
                         row_tags=b["row_tags"])[0])


def test_the_other_column_fails_the_nearer_twin(oracle):
    b = _base()
    values = b["values"].copy()
    values[[TWIN_FAILS, TWIN_A, TWIN_B], 1] = [9500, 5000, 5000]
    lo, hi = b["between"][0].copy(), b["between"][1].copy()
    lo[0], hi[0] = (4000, 1000), (6000, 9000)       # the span is column 0's or 1's; the other is tested per row
    b["dev"].set_values(values)
    try:
        got = b["dev"].knn_between(b["X"], K, (lo, hi), return_distances=True)
        ids, _ = _check(oracle, got, b["X"], b["Y"], K, (lo, hi), values)
    finally:
        b["dev"].set_values(b["values"])
    _twins_answer(ids)


def test_all_together_and_too_few_passing_rows(oracle):
    b = _base()
    rng = np.random.RandomState(45)
    n, nq = b["n"], b["nq"]
    mask = rng.rand(n) < 0.7
    mask[[TWIN_FAILS, TWIN_A, TWIN_B]] = True
    exclude = b["own"].copy()
    exclude[0] = TWIN_FAILS                             # query 0: the twin it lies on is the one excluded
    group = rng.randint(-1, 4, size=nq).astype(np.int32)
    group[0] = 2
    tags = rng.randint(0, 256, size=nq).astype(np.uint64)
    tags[0] = 0
    tags[2::5] = 0xf0 | (1 << 40)                       # "all" of five tags: few rows, or none
    r = dict(allowed=mask, exclude=exclude, group=group, groups=b["groups"], tags=tags, tags_mode="all",
             row_tags=b["row_tags"])
    counts = np.array([passes(i, n, between=b["between"], values=b["values"], **r).sum() for i in range(nq)])
    assert (counts >= K).any() and ((counts < K) & (counts > 0)).any() and (counts == 0).any(), counts
    kw = dict(allowed=mask, exclude=exclude, group=group, tags=tags, tags_mode="all")
    ids, _ = _check(oracle, b["dev"].knn_between(b["X"], K, b["between"], return_distances=True, **kw), b["X"], b["Y"],
                    K, b["between"], b["values"], **r)
    _twins_answer(ids)
    np.testing.assert_array_equal((ids >= 0).sum(axis=1), np.minimum(counts, K))
    np.testing.assert_array_equal(b["dev"].knn_between(b["X"], K, b["between"], **kw), ids)


def test_state_errors_and_refusals():
    from tinyknn_amd import _lib
    from tinyknn_amd._lib import TinyKnnHipError
    from tinyknn_amd.ivf import AllowSet
    rng = np.random.RandomState(80)
    Y = rng.randn(2000, 16).astype(np.float32)
    X = rng.randn(5, 16).astype(np.float32)
    dev = _index(Y)
    with pytest.raises(TinyKnnHipError, match="no values"):
        dev.knn_between(X, K, (0, 1))
    with pytest.raises(TinyKnnHipError, match="no values"):
        dev.range_sizes((0, 1))
    dev.set_values(np.arange(2000, dtype=np.int64))
    with pytest.raises(TinyKnnHipError, match="no groups"):
        dev.knn_between(X, K, (0, 100), group=1)
    with pytest.raises(TinyKnnHipError, match="no tags"):
        dev.knn_between(X, K, (0, 100), tags=1)
    with pytest.raises(ValueError, match="query 2 bounds no column"):
        dev.knn_between(X, K, (np.array([0, 0, MIN, 0, 0]), np.array([9, 9, MAX, 9, 9])))
    # ... which the library refuses by itself too
    keys = np.array([[[0, 9]], [[MIN, MAX]]], dtype=np.int64)
    out = np.zeros((2, K), dtype=np.int64)
    rc = _lib.lib().tk_index_knn_between(dev._h, _lib.ptr(X[:2].copy(), _lib._f32p), 2, K, keys.ctypes.data, None, None,
                                         None, None, 0, _lib.ptr(out, _lib._i64p), None)
    assert rc == -1 and "query 1 bounds no column" in _lib.lib().tk_last_error().decode()
    with pytest.raises(AssertionError):
        dev.knn_between(X, 0, (0, 100))
    with pytest.raises(AssertionError):
        dev.knn_between(X, 1025, (0, 100))
    with pytest.raises(TypeError, match="AllowSet"):
        dev.knn_between(X, K, (0, 100), allowed=object.__new__(AllowSet))
    assert dev.value_rows()["builds"] == 0              # nothing was made by the refused calls
    dev.world = 2                                       # (what a list-sharded index looks like to the Python layer)
    try:
        with pytest.raises(RuntimeError, match="list-sharded"):
            dev.knn_between(X, K, (0, 100))
    finally:
        dev.world = 1
    ids = dev.knn_between(X, K, (0, 100))
    assert (ids >= 0).all() and (ids <= 100).all() and dev.value_rows()["builds"] == 1
    np.testing.assert_array_equal(dev.range_sizes((np.array([0, 5, MIN]), np.array([100, 4, MAX]))),
                                  (np.array([101, 0, 2000]), np.array([0, 0, -1])))


# ---- 7. list changes --------------------------------------------------------------------------------------------------
def test_after_remove_add_and_update(oracle):
    from test_remove_gpu import SEED, SIGMA, _fitted, _host_index
    from tinyknn_amd.ivf import synth_rows
    d, n0 = 100, 3000
    ivf = _host_index("euclidean", d, 1, N=n0)
    dev = ivf.device_index()
    cent = _fitted("euclidean", d)[2]
    qs = synth_rows(48, d, SEED + 1, cent, SIGMA)
    qn, qp = ivf._prepare(qs.copy())
    rng = np.random.RandomState(4)
    values = rng.randint(0, 3000, size=n0).astype(np.int64)
    values[rng.choice(n0, size=15, replace=False)] = 7
    lo = rng.randint(0, 2500, size=len(qn)).astype(np.int64)
    hi = lo + rng.randint(50, 500, size=len(qn))
    lo[:4], hi[:4] = 7, 7                               # four queries in the window of one value
    between = (lo, hi)
    ivf.set_values(values)
    # calls that do not ask for the rows by value never make them
    dev.query_batch(qn, qp, K, 5)
    dev.query_batch(qn, qp, K, 5, between=between)
    dev.knn_brute(qn, K, between=between)
    assert dev.value_rows() == dict(built=False, bytes=0, builds=0, columns=0)

    def check(stored):
        got = dev.knn_between(qn, K, between, return_distances=True)
        return _check(oracle, got, qn, np.asarray(ivf.data), K, between, np.asarray(ivf.values), stored=stored)[0]
    stored = np.ones(n0, dtype=bool)
    before = check(stored)
    assert dev.value_rows()["builds"] == 1 and (before[:4, 0] >= 0).all()
    # remove: the nearest row of every query, and every row of value 7
    dead = np.unique(np.concatenate([before[:, 0], np.flatnonzero(values == 7)]))
    ivf.remove(dead)
    stored[dead] = False
    gone = check(stored)
    assert not np.isin(gone, dead).any() and (gone[:4] == -1).all()
    assert dev.value_rows()["builds"] == 1              # the rows by value follow the values, not the lists
    np.testing.assert_array_equal(dev.range_sizes((7, 7))[0], [np.sum(values == 7)])       # (removed rows are counted)
    # add(values=): the new rows are found, the table is made once more
    new = synth_rows(400, d, SEED, cent, SIGMA, row0=n0)
    ivf.add(new, values=np.where(np.arange(400) < 40, 7, rng.randint(0, 3000, size=400)))
    stored = np.concatenate([stored, np.ones(400, dtype=bool)])
    assert not dev.value_rows()["built"]
    added = check(stored)
    assert dev.value_rows()["builds"] == 2 and (added >= n0).any() and (added[:4] >= n0).all()
    assert dev.value_rows()["bytes"] == 4 * (n0 + 400)
    # update(values=): the new vectors are ranked under the new values, removed rows come back
    rows = np.concatenate([np.arange(n0 + 40, n0 + 43), dead[:5]])
    X = np.repeat(qn[:1], len(rows), axis=0) + 1e-3 * rng.randn(len(rows), d).astype(np.float32)
    ivf.update(rows, X, values=np.full(len(rows), 7))
    stored[rows] = True
    moved = check(stored)
    assert dev.value_rows()["builds"] == 3 and np.isin(moved[0][:len(rows)], rows).all()


# ---- 8. exact_below ---------------------------------------------------------------------------------------------------
def test_exact_below_routes_narrow_ranges(oracle):
    from test_remove_gpu import SEED, SIGMA, _fitted, _host_index
    from tinyknn_amd.ivf import synth_rows
    d, n0 = 100, 4000
    ivf = _host_index("euclidean", d, 1, N=n0)
    qs = synth_rows(120, d, SEED + 1, _fitted("euclidean", d)[2], SIGMA)
    rng = np.random.RandomState(5)
    values = rng.permutation(n0).astype(np.int64)               # distinct: a window's length is its width
    ivf.set_values(values)
    nq = len(qs)
    width = np.where(rng.rand(nq) < 0.5, 12, 930)
    lo = rng.randint(0, n0 - 930, size=nq).astype(np.int64)
    hi = lo + width - 1
    lo[::10], hi[::10] = MIN, MAX                               # queries that bound nothing
    between = (lo, hi)
    T = 100
    bounded = lo != MIN
    routed = bounded & (width < T)
    assert routed.any() and (~routed & bounded).any() and (~bounded).any()
    qn, _ = ivf._prepare(qs.copy())
    for want_dist in (False, True):
        plain = ivf.query_batch(qs, K, 2, between=between, return_distances=want_dist)
        got = ivf.query_batch(qs, K, 2, between=between, exact_below=T, return_distances=want_dist)
        exact = ivf.knn_between(qs[routed], K, _cut(between, routed), return_distances=want_dist)
        if want_dist:
            np.testing.assert_array_equal(got[0][routed], exact[0])
            np.testing.assert_array_equal(got[0][~routed], plain[0][~routed])
            assert got[1].dtype == plain[1].dtype == exact[1].dtype == np.float32
            assert same_bits(got[1][routed], exact[1]) and same_bits(got[1][~routed], plain[1][~routed])
            _check(oracle, exact, qn[routed], np.asarray(ivf.data), K, _cut(between, routed), values)
            got, plain = got[0], plain[0]
        else:
            np.testing.assert_array_equal(got[routed], exact)
            np.testing.assert_array_equal(got[~routed], plain[~routed])
        # the point of the feature: two probed lists hold fewer than k rows of a 12-row window, the routed call finds
        # every one the window has
        assert (plain[routed] == -1).any() and (got[routed] >= 0).all()
    length, col = ivf.device_index().range_sizes(between)
    np.testing.assert_array_equal(length, np.where(bounded, width, n0))
    np.testing.assert_array_equal(col, np.where(bounded, 0, -1))
    np.testing.assert_array_equal(ivf.query_batch(qs, K, 2, between=between, exact_below=0),
                                  ivf.query_batch(qs, K, 2, between=between))
    everything_routed = ivf.query_batch(qs, K, 2, between=between, exact_below=n0 + 1)
    np.testing.assert_array_equal(everything_routed[bounded], ivf.knn_between(qs[bounded], K, _cut(between, bounded)))
    np.testing.assert_array_equal(everything_routed[~bounded], ivf.query_batch(qs, K, 2, between=between)[~bounded])
