"""The exact search inside a query's own group (tk_index_knn_group) against its reference
(tests/group_exact_reference.py): ids and distance bits equal on every case, numpy's einsum within 1 ulp.  Every
store and width, group sizes at the edges of k, of the tile and of the candidate buffer, ties, every restriction, the
lists changing under it, and IVF.query_batch(exact_below=)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from brute_restricted_reference import passes  # noqa: E402
from conftest import golden  # noqa: E402
from group_exact_reference import (append_model, einsum_distances, knn_group_reference, reference_data,  # noqa: E402
                                   same_bits)

pytestmark = pytest.mark.gpu

K = 10
FAR = 2**31 - 2             # the largest group id there is


def _index(data, store=None):
    """a DeviceIndex that only needs its vectors: one list holding every row (as tests/test_brute_gpu.py makes it)"""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import TransformedData
    from tinyknn_amd._transform import transform_data
    n, d = data.shape
    dq = d + (-d) % 8
    ivf = IVF("euclidean", 1, FastPQ(2))
    ivf.pq.centers = np.zeros((16, dq), np.float32)
    ivf.pq.sqrt_n_blocks = float(np.sqrt(dq // 2))
    ivf.active_centers = np.zeros((1, d), np.float32)
    ivf.pq_transformed_centers = TransformedData(1, transform_data(np.zeros((16, dq // 2), np.uint8)))
    pad = (-n) % 16
    ivf.pq_transformed_points = [TransformedData(n, transform_data(np.zeros((n + pad, dq // 2), np.uint8)))]
    ivf.ids = [np.arange(n, dtype=np.int64)]
    ivf.data = data
    ivf.store = store
    return ivf.device_index()


def _check(oracle, got, qn, data, k, group, groups, stored=None, einsum=True, **restrictions):
    """a (ids, dist) answer against the reference: ids, distance bits, dtype; numpy's einsum within 1 ulp"""
    ids, dist = got
    want_ids, want_dist = knn_group_reference(oracle, qn, data, k, group, groups, stored=stored, **restrictions)
    assert ids.dtype == np.int64 and ids.shape == (len(qn), k)
    np.testing.assert_array_equal(ids, want_ids)
    assert dist.dtype == want_dist.dtype and same_bits(dist, want_dist)
    assert np.isposinf(dist[ids < 0]).all()
    if einsum and (ids >= 0).any():
        live = ids >= 0
        np.testing.assert_array_max_ulp(dist[live], einsum_distances(qn, data, ids)[live], maxulp=1)
    return ids, dist


# ---- 1. stores and widths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", [None, "float16"])
@pytest.mark.parametrize("d", [1, 20, 100, 127, 128])
def test_stores_and_widths(oracle, store, d):
    rng = np.random.RandomState(1000 + d)
    n = 3000
    Y = rng.randn(n, d).astype(np.float32)
    dev = _index(Y, store)
    groups = rng.choice(np.array([0, 3, 70000, FAR], dtype=np.int64), size=n).astype(np.int32)
    dev.set_groups(groups)
    ref = reference_data(Y, store)
    assert dev.group_rows() == dict(built=False, bytes=0, builds=0, groups=0)
    for nq, k in ((0, K), (1, K), (4, 1), (4, K), (4, 100), (4, 1024), (1000, K)):
        X = rng.randn(nq, d).astype(np.float32)
        if nq:
            X[0] = Y[5]                                 # a query on a row
        group = groups[rng.randint(0, n, size=nq)]
        _check(oracle, dev.knn_group(X, k, group, return_distances=True), X, ref, k, group, groups)
        np.testing.assert_array_equal(dev.knn_group(X, k, group), knn_group_reference(oracle, X, ref, k, group, groups)[0])
    info = dev.group_rows()
    assert info["built"] and info["builds"] == 1 and info["groups"] == 4 and info["bytes"] == 4 * n + 4 * 4 + 4 * 5
    np.testing.assert_array_equal(dev.group_sizes([0, 3, 70000, FAR, 1, 2**31 - 1 - 2]),
                                  [np.sum(groups == g) for g in (0, 3, 70000, FAR)] + [0, 0])


def test_float64_vectors_on_the_fixture(oracle):
    from store_reference import fixture_ivf
    g = golden("g6_ivf_eu20f64.npz")
    ivf = fixture_ivf(g)
    data, qn = g["data"], np.ascontiguousarray(g["qn"], dtype=np.float32)
    assert data.dtype == np.float64
    n = len(data)
    dev = ivf.device_index()
    rng = np.random.RandomState(64)
    groups = rng.randint(0, 6, size=n).astype(np.int32)
    dev.set_groups(groups)
    stored = np.zeros(n, dtype=bool)
    stored[np.concatenate([np.asarray(i) for i in ivf.ids])] = True
    for k in (1, K, 100, min(1024, n)):
        q = qn[:40] if k > 100 else qn
        group = rng.randint(0, 6, size=len(q)).astype(np.int32)
        _, dist = _check(oracle, dev.knn_group(q, k, group, return_distances=True), q, data, k, group, groups,
                         stored=stored)
        assert dist.dtype == np.float64


# ---- 2. group sizes at the edges --------------------------------------------------------------------------------------
_EDGES = {}
SIZES = {11: 1, 12: K - 1, 13: K, 14: K + 1, 15: 255, 16: 256, 17: 257, 18: 300, FAR: 2049, 1000003: 2047}


def _edges():
    """N = 8000, d = 20: groups of the sizes above (ids sparse up to 2^31 - 2), the rest in group 0; group 18 is 300
    identical rows; group 17's rows at span positions 255 and 256 — across the tile border — are twins"""
    if not _EDGES:
        from tinyknn_amd import _lib
        assert (_lib.GROUP_EXACT_TILE, _lib.GROUP_EXACT_CAP) == (256, 2048)
        rng = np.random.RandomState(7)
        n, d = 8000, 20
        Y = rng.randn(n, d).astype(np.float32)
        groups = np.zeros(n, dtype=np.int32)
        free = rng.permutation(n)
        at = 0
        for g, size in SIZES.items():
            groups[free[at:at + size]] = g
            at += size
        Y[groups == 18] = Y[np.flatnonzero(groups == 18)[0]]
        span17 = np.flatnonzero(groups == 17)
        Y[span17[256]] = Y[span17[255]]
        dev = _index(Y)
        dev.set_groups(groups)
        _EDGES.update(Y=Y, groups=groups, dev=dev, span17=span17)
    return _EDGES


def test_group_sizes_at_the_edges(oracle):
    e = _edges()
    Y, groups, dev = e["Y"], e["groups"], e["dev"]
    rng = np.random.RandomState(8)
    ids_of = list(SIZES) + [0, 999]                     # 999: an id no row carries
    group = np.array(ids_of * 3, dtype=np.int32)        # queries of one batch in different groups, three in each
    X = rng.randn(len(group), Y.shape[1]).astype(np.float32)
    np.testing.assert_array_equal(dev.group_sizes(np.array(ids_of)), list(SIZES.values()) + [8000 - sum(SIZES.values()), 0])
    for k in (1, K, 100):
        ids, dist = _check(oracle, dev.knn_group(X, k, group, return_distances=True), X, Y, k, group, groups)
        for i, g in enumerate(group):
            assert (ids[i] >= 0).sum() == min(k, int(np.sum(groups == g)))
        assert (ids[group == 999] == -1).all() and np.isposinf(dist[group == 999]).all()


def test_many_queries_in_one_group(oracle):
    e = _edges()
    rng = np.random.RandomState(9)
    X = rng.randn(300, e["Y"].shape[1]).astype(np.float32)
    group = np.full(len(X), 17, dtype=np.int32)
    _check(oracle, e["dev"].knn_group(X, K, group, return_distances=True), X, e["Y"], K, group, e["groups"])


def test_ties(oracle):
    e = _edges()
    Y, groups, dev, span17 = e["Y"], e["groups"], e["dev"], e["span17"]
    rows18 = np.flatnonzero(groups == 18)
    X = np.stack([Y[rows18[0]], Y[span17[255]]])
    group = np.array([18, 17], dtype=np.int32)
    ids, dist = _check(oracle, dev.knn_group(X, K, group, return_distances=True), X, Y, K, group, groups)
    np.testing.assert_array_equal(ids[0], rows18[:K])           # 300 identical rows: the lowest ids
    assert (dist[0] == 0).all()
    np.testing.assert_array_equal(ids[1][:2], span17[255:257])  # the twins across the tile border, the lower first
    assert (dist[1][:2] == 0).all()


def test_one_group_holds_every_row_and_the_buffer_is_cut_back(oracle):
    """N = 6000 rows in ONE group, and query 0 sees them in descending distance: every row is within the bound when its
    lane looks, so the buffer of 2048 fills and is cut at least twice in front of tiles (the model of the appends says
    so); the other queries are random."""
    from tinyknn_amd import _lib
    tile, cap = _lib.GROUP_EXACT_TILE, _lib.GROUP_EXACT_CAP
    rng = np.random.RandomState(10)
    n, d = 6000, 8
    Y = rng.randn(n, d).astype(np.float32)
    Y[:, 0] = 10.0 + (n - np.arange(n)) * 0.25          # the first coordinate falls with the row id
    X = rng.randn(6, d).astype(np.float32)
    X[0] = 0
    X[0, 0] = -100.0
    groups = np.full(n, 424242, dtype=np.int32)
    dev = _index(Y)
    dev.set_groups(groups)
    group = groups[:len(X)].copy()
    for k in (K, 1024):
        dv = oracle.sqdist_gather(X[0], Y, np.arange(n))
        cuts, most = append_model(dv, k, tile, cap)
        assert cuts >= 2 and most <= cap, (cuts, most)
        assert append_model(oracle.sqdist_gather(X[1], Y, np.arange(n)), k, tile, cap)[1] <= cap
        ids, _ = _check(oracle, dev.knn_group(X, k, group, return_distances=True), X, Y, k, group, groups)
        np.testing.assert_array_equal(ids[0], np.arange(n - 1, n - 1 - k, -1))
    assert dev.group_rows()["groups"] == 1 and dev.group_sizes(424242)[0] == n


# ---- 3. restrictions --------------------------------------------------------------------------------------------------
_BASE = {}
TWIN_FAILS, TWIN_A, TWIN_B = 100, 200, 300      # three identical rows of group 2: query 0 lies on them; the lowest must fail


def _base():
    if not _BASE:
        rng = np.random.RandomState(20)
        n, d, nq = 4000, 16, 67
        Y = rng.randn(n, d).astype(np.float32)
        Y[TWIN_A] = Y[TWIN_B] = Y[TWIN_FAILS]
        groups = rng.randint(0, 4, size=n).astype(np.int32)
        groups[[TWIN_FAILS, TWIN_A, TWIN_B]] = 2
        X = rng.randn(nq, d).astype(np.float32)
        X[0] = Y[TWIN_FAILS]
        own = rng.choice(np.arange(400, n), size=nq, replace=False)
        X[1::2] = Y[own[1::2]]                          # every other query lies on a row ...
        group = rng.randint(0, 4, size=nq).astype(np.int32)
        group[1::2] = groups[own[1::2]]                 # ... of its own group
        group[0] = 2
        row_tags = np.array([sum(1 << int(b) for b in rng.choice(8, size=rng.randint(1, 4), replace=False))
                             for _ in range(n)], dtype=np.uint64)
        row_tags[TWIN_FAILS], row_tags[TWIN_A], row_tags[TWIN_B] = 0b0001, 0b0110, 0b0110
        dev = _index(Y)
        dev.set_groups(groups)
        dev.set_tags(row_tags)
        _BASE.update(Y=Y, X=X, n=n, nq=nq, groups=groups, group=group, own=own, row_tags=row_tags, dev=dev)
    return _BASE


def _twins_answer(ids):
    assert TWIN_FAILS not in ids[0]
    np.testing.assert_array_equal(ids[0][:2], [TWIN_A, TWIN_B])


def _values_and_ranges(kind, rng, n, nq):
    if kind == "i1":
        values = rng.randint(-1000, 1000, size=n).astype(np.int64)
        values[TWIN_FAILS], values[TWIN_A], values[TWIN_B] = 999, 5, 5
        lo = rng.randint(-1000, 400, size=nq).astype(np.int64)
        hi = lo + rng.randint(100, 900, size=nq)
        lo[4::10] = np.iinfo(np.int64).min
        hi[6::10] = np.iinfo(np.int64).max
        lo[8::10], hi[8::10] = 10, -10                  # lo > hi: nothing passes
        lo[0], hi[0] = 0, 10
        return values, (lo, hi)
    values = rng.randint(-100, 100, size=(n, 4)).astype(np.float32) / 4
    values[TWIN_FAILS], values[TWIN_A], values[TWIN_B] = 24.75, 1.5, 1.5
    lo = (rng.randint(-100, 0, size=(nq, 4)) / 4).astype(np.float32)
    hi = lo + (rng.randint(60, 200, size=(nq, 4)) / 4).astype(np.float32)
    lo[4::10, 1] = -np.inf
    hi[6::10, 2] = np.inf
    lo[8::10, 3], hi[8::10, 3] = 2.0, 1.0
    lo[0], hi[0] = 0.0, 2.0
    return values, (lo, hi)


@pytest.mark.parametrize("as_ids", [False, True])
def test_allowed_alone(oracle, as_ids):
    b = _base()
    mask = np.random.RandomState(21).rand(b["n"]) < 0.3
    mask[TWIN_FAILS], mask[TWIN_A], mask[TWIN_B] = False, True, True
    got = b["dev"].knn_group(b["X"], K, b["group"], allowed=np.flatnonzero(mask) if as_ids else mask,
                             return_distances=True)
    _twins_answer(_check(oracle, got, b["X"], b["Y"], K, b["group"], b["groups"], allowed=mask)[0])


def test_exclude_alone(oracle):
    b = _base()
    exclude = b["own"].copy()
    exclude[0] = TWIN_FAILS
    exclude[5::7] = -1
    got = b["dev"].knn_group(b["X"], K, b["group"], exclude=exclude, return_distances=True)
    ids, _ = _check(oracle, got, b["X"], b["Y"], K, b["group"], b["groups"], exclude=exclude)
    _twins_answer(ids)
    assert ids[5][0] == b["own"][5] and ids[1][0] != b["own"][1]            # (kept where -1, gone where named)


@pytest.mark.parametrize("mode", ["any", "all"])
def test_tags_alone(oracle, mode):
    b = _base()
    rng = np.random.RandomState(23)
    tags = np.array([sum(1 << int(t) for t in rng.choice(8, size=rng.randint(1, 3), replace=False))
                     for _ in range(b["nq"])], dtype=np.uint64)
    tags[3::9] = 0
    tags[0] = 0b0110
    got = b["dev"].knn_group(b["X"], K, b["group"], tags=tags, tags_mode=mode, return_distances=True)
    _twins_answer(_check(oracle, got, b["X"], b["Y"], K, b["group"], b["groups"], tags=tags, tags_mode=mode,
                         row_tags=b["row_tags"])[0])


@pytest.mark.parametrize("kind", ["i1", "f4"])
def test_between_alone(oracle, kind):
    b = _base()
    values, between = _values_and_ranges(kind, np.random.RandomState(24), b["n"], b["nq"])
    b["dev"].set_values(values)
    got = b["dev"].knn_group(b["X"], K, b["group"], between=between, return_distances=True)
    ids, _ = _check(oracle, got, b["X"], b["Y"], K, b["group"], b["groups"], between=between, values=values)
    _twins_answer(ids)
    assert (ids[8] == -1).all()


def test_all_together_and_too_few_passing_rows(oracle):
    b = _base()
    rng = np.random.RandomState(25)
    n, nq = b["n"], b["nq"]
    values, (lo, hi) = _values_and_ranges("f4", rng, n, nq)
    lo, hi = lo - 10, hi + 10
    lo[8::10, 3], hi[8::10, 3] = 2.0, 1.0
    b["dev"].set_values(values)
    mask = rng.rand(n) < 0.7
    mask[[TWIN_FAILS, TWIN_A, TWIN_B]] = True
    exclude = b["own"].copy()
    exclude[0] = TWIN_FAILS                             # query 0: the twin it lies on is the one excluded
    tags = rng.randint(0, 256, size=nq).astype(np.uint64)
    tags[0] = 0
    tags[2::5] = 0xf0 | (1 << 40)                       # "all" of five tags: few rows, or none
    r = dict(allowed=mask, exclude=exclude, tags=tags, tags_mode="all", row_tags=b["row_tags"], between=(lo, hi),
             values=values)
    counts = np.array([(passes(i, n, **r) & (b["groups"] == b["group"][i])).sum() for i in range(nq)])
    assert (counts >= K).any() and ((counts < K) & (counts > 0)).any() and (counts == 0).any(), counts
    got = b["dev"].knn_group(b["X"], K, b["group"], allowed=mask, exclude=exclude, tags=tags, tags_mode="all",
                             between=(lo, hi), return_distances=True)
    ids, _ = _check(oracle, got, b["X"], b["Y"], K, b["group"], b["groups"], **r)
    _twins_answer(ids)
    np.testing.assert_array_equal((ids >= 0).sum(axis=1), np.minimum(counts, K))
    np.testing.assert_array_equal(b["dev"].knn_group(b["X"], K, b["group"], allowed=mask, exclude=exclude, tags=tags,
                                                     tags_mode="all", between=(lo, hi)), ids)


def test_state_errors_and_refusals():
    from tinyknn_amd._lib import TinyKnnHipError
    from tinyknn_amd.ivf import AllowSet
    rng = np.random.RandomState(80)
    Y = rng.randn(2000, 16).astype(np.float32)
    X = rng.randn(5, 16).astype(np.float32)
    dev = _index(Y)
    with pytest.raises(TinyKnnHipError, match="no groups"):
        dev.knn_group(X, K, 1)
    with pytest.raises(TinyKnnHipError, match="no groups"):
        dev.group_sizes([1])
    dev.set_groups(np.zeros(len(Y), dtype=np.int32))
    with pytest.raises(TinyKnnHipError, match="no tags"):
        dev.knn_group(X, K, 0, tags=1)
    with pytest.raises(TinyKnnHipError, match="no values"):
        dev.knn_group(X, K, 0, between=(0, 1))
    with pytest.raises(AssertionError, match=">= 0"):
        dev.knn_group(X, K, [0, 0, -1, 0, 0])
    with pytest.raises(AssertionError):
        dev.knn_group(X, 0, 0)
    with pytest.raises(AssertionError):
        dev.knn_group(X, 1025, 0)
    with pytest.raises(TypeError, match="AllowSet"):
        dev.knn_group(X, K, 0, allowed=object.__new__(AllowSet))
    assert dev.group_rows()["builds"] == 0              # nothing was made by the refused calls
    dev.world = 2                                       # (what a list-sharded index looks like to the Python layer)
    try:
        with pytest.raises(RuntimeError, match="list-sharded"):
            dev.knn_group(X, K, 0)
    finally:
        dev.world = 1
    ids = dev.knn_group(X, K, 0)
    assert (ids >= 0).all() and dev.group_rows()["builds"] == 1


# ---- 4. list changes --------------------------------------------------------------------------------------------------
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
    groups = rng.randint(0, 30, size=n0).astype(np.int32)
    group = rng.randint(0, 30, size=len(qn)).astype(np.int32)
    group[:4] = 7
    ivf.set_groups(groups)
    # calls without the feature never make the tables
    dev.query_batch(qn, qp, K, 5, group=group)
    dev.knn_brute(qn, K, group=group)
    assert dev.group_rows() == dict(built=False, bytes=0, builds=0, groups=0)

    def check(stored):
        got = dev.knn_group(qn, K, group, return_distances=True)
        return _check(oracle, got, qn, np.asarray(ivf.data), K, group, np.asarray(ivf.groups), stored=stored)[0]
    stored = np.ones(n0, dtype=bool)
    before = check(stored)
    assert dev.group_rows()["builds"] == 1
    # remove: the nearest row of every query, and the whole of group 7
    dead = np.unique(np.concatenate([before[:, 0], np.flatnonzero(groups == 7)]))
    ivf.remove(dead)
    stored[dead] = False
    gone = check(stored)
    assert not np.isin(gone, dead).any() and (gone[:4] == -1).all()
    assert dev.group_rows()["builds"] == 1              # the rows by group follow the groups, not the lists
    np.testing.assert_array_equal(dev.group_sizes([7]), [np.sum(groups == 7)])     # (removed rows are counted)
    # add(groups=): the new rows are found, the table is made once more
    new = synth_rows(400, d, SEED, cent, SIGMA, row0=n0)
    ivf.add(new, groups=np.where(np.arange(400) < 40, 7, rng.randint(0, 30, size=400)))
    stored = np.concatenate([stored, np.ones(400, dtype=bool)])
    assert not dev.group_rows()["built"]
    added = check(stored)
    assert dev.group_rows()["builds"] == 2 and (added >= n0).any() and (added[:4] >= n0).all()
    # update: the new vectors are ranked (rows of group 7 moved onto query 0), removed rows come back
    new7 = np.flatnonzero(np.asarray(ivf.groups) == 7)
    rows = np.concatenate([new7[new7 >= n0][:3], dead[:5]])
    X = np.repeat(qn[:1], len(rows), axis=0) + 1e-3 * rng.randn(len(rows), d).astype(np.float32)
    ivf.update(rows, X)
    stored[rows] = True
    moved = check(stored)
    assert np.isin(moved[0][:3], rows).all()


# ---- 5. exact_below ---------------------------------------------------------------------------------------------------
def test_exact_below_routes_small_groups(oracle):
    from test_remove_gpu import SEED, SIGMA, _fitted, _host_index
    from tinyknn_amd.ivf import synth_rows
    d, n0 = 100, 4000
    ivf = _host_index("euclidean", d, 1, N=n0)
    dev = ivf.device_index()
    qs = synth_rows(120, d, SEED + 1, _fitted("euclidean", d)[2], SIGMA)
    rng = np.random.RandomState(5)
    # groups 0 .. 99 of about 12 rows (1200 rows), groups 1000 .. 1002 of about 930
    groups = np.where(np.arange(n0) < 1200, rng.randint(0, 100, size=n0), 1000 + rng.randint(0, 3, size=n0)).astype(np.int32)
    groups = groups[rng.permutation(n0)]
    ivf.set_groups(groups)
    group = np.where(rng.rand(len(qs)) < 0.5, rng.randint(0, 100, size=len(qs)), 1000 + rng.randint(0, 3, size=len(qs)))
    group[::10] = -1
    group = group.astype(np.int32)
    sizes = np.array([np.sum(groups == g) for g in group])
    T = 100
    routed = (group >= 0) & (sizes < T)
    assert routed.any() and (~routed & (group >= 0)).any() and (group == -1).any()
    qn, _ = ivf._prepare(qs.copy())
    for want_dist in (False, True):
        plain = ivf.query_batch(qs, K, 2, group=group, return_distances=want_dist)
        exact = ivf.knn_group(qs[routed], K, group[routed], return_distances=want_dist)
        got = ivf.query_batch(qs, K, 2, group=group, exact_below=T, return_distances=want_dist)
        if want_dist:
            np.testing.assert_array_equal(got[0][routed], exact[0])
            np.testing.assert_array_equal(got[0][~routed], plain[0][~routed])
            assert got[1].dtype == plain[1].dtype == exact[1].dtype == np.float32
            assert same_bits(got[1][routed], exact[1]) and same_bits(got[1][~routed], plain[1][~routed])
            _check(oracle, exact, qn[routed], np.asarray(ivf.data), K, group[routed], groups)
            got, plain = got[0], plain[0]
        else:
            np.testing.assert_array_equal(got[routed], exact)
            np.testing.assert_array_equal(got[~routed], plain[~routed])
        # the point of the feature: two probed lists hold fewer than k rows of a small group, the routed call finds
        # every one the group has
        full = routed & (sizes >= K)
        assert full.any() and (plain[full] == -1).any() and (got[full] >= 0).all()
    np.testing.assert_array_equal(ivf.query_batch(qs, K, 2, group=group, exact_below=0),
                                  ivf.query_batch(qs, K, 2, group=group))
    everything = ivf.query_batch(qs, K, 2, group=group, exact_below=n0 + 1)
    np.testing.assert_array_equal(everything[group >= 0], ivf.knn_group(qs[group >= 0], K, group[group >= 0]))
    np.testing.assert_array_equal(everything[group < 0], ivf.query_batch(qs, K, 2, group=group)[group < 0])
