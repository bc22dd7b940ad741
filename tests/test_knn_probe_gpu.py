"""The exact k nearest rows of the probed lists (tk_index_knn_probe) against the reference the tree has
for the radius call over the same lists (tests/radius_probe_reference.py at radius +inf), every list cut to its first k
and padded with -1 / +inf: ids equal, distances the same dtype and bytes."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import golden  # noqa: E402
from radius_probe_reference import oracle_probes, passes, radius_probe_csr  # noqa: E402
from store_reference import fixture_ivf, oracle_index, rounded  # noqa: E402

pytestmark = pytest.mark.gpu


def _cut(csr, k):
    """the reference's lists cut to their first k: (ids (nq, k) int64, dist (nq, k)), -1 / +inf behind short ones"""
    lims, ids, dist = csr
    W = np.full((len(lims) - 1, k), -1, dtype=np.int64)
    D = np.full((len(lims) - 1, k), np.inf, dtype=dist.dtype)
    for i, (a, b) in enumerate(zip(lims[:-1], lims[1:])):
        m = min(k, b - a)
        W[i, :m], D[i, :m] = ids[a:a + m], dist[a:a + m]
    return W, D


def _same(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    assert got[0].dtype == np.int64 and got[1].dtype == want[1].dtype and got[1].tobytes() == want[1].tobytes(), what


@functools.lru_cache(maxsize=None)
def _fixture(tag, store=None):
    from oracle import oracle
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = fixture_ivf(g, store=store)
    data = rounded(g["data"]) if store == "float16" else g["data"]
    return ivf, ivf.device_index(), oracle_index(oracle, ivf, data), np.ascontiguousarray(g["qn"]), \
        np.ascontiguousarray(g["qpq"]), data


# ---- 1. the golden fixtures -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,store", [("eu20", None), ("an100", None), ("an100b2", None), ("eu128", None),
                                       ("eu20f64", None), ("eu20", "float16"), ("an100b2", "float16")])
def test_fixtures(oracle, tag, store):
    ivf, dev, ox, qn, qpq, data = _fixture(tag, store)
    for P in (1, 2, 10, ox.n_lists + 3):
        everything = radius_probe_csr(oracle, ox, qn, data, np.inf, P)
        for k in (1, 10, 50):
            _same(dev.knn_probe(qn, qpq, k, P, return_distances=True), _cut(everything, k), f"{tag} P={P} k={k}")
        np.testing.assert_array_equal(dev.knn_probe(qn, qpq, 10, P), _cut(everything, 10)[0])


# ---- 2. tile edges ----------------------------------------------------------------------------------------------------
TILES = {1: (64, 256), 20: (64, 256), 100: (64, 64), 127: (60, 64), 128: (60, 64), 300: (20, 32)}   # d: (QT, RB), §3.21


@functools.lru_cache(maxsize=None)
def _edges(d):
    """A euclidean index with centres set by hand, far apart: lists of 0, 1, RB - 1, RB, RB + 1 and 2 049 rows around
    their centres and one of 300 copies of its centre (list 0: one row, removed again)"""
    from oracle import oracle
    from tinyknn_amd import IVF, FastPQ
    oracle.build()
    RB = TILES[d][1]
    lengths = [0, 1, RB - 1, RB, RB + 1, 2049, 300]
    rng = np.random.RandomState(700 + d)
    L = len(lengths)
    cent = np.zeros((L, d), dtype=np.float32)
    if d >= L:
        cent[np.arange(L), np.arange(L)] = 8.0
    else:
        cent[:, 0] = 8.0 * np.arange(L)
    member = np.repeat(np.arange(L), [max(n, 1) for n in lengths])
    X = (cent[member] + 0.5 * rng.randn(len(member), d).astype(np.float32)).astype(np.float32)
    X[member == L - 1] = cent[L - 1]
    perm = rng.permutation(len(X))
    X, member = np.ascontiguousarray(X[perm]), member[perm]
    ivf = IVF("euclidean", L, FastPQ(2))
    ivf.all_centers = cent
    state = np.random.get_state()
    np.random.seed(77)
    try:
        ivf.pq.fit(X)
        ivf.build(X, n_probes=1, device=False)
    finally:
        np.random.set_state(state)
    ivf.remove(np.flatnonzero(member == 0))
    assert [len(ivf.ids[l]) for l in range(L)] == lengths
    return ivf, oracle_index(oracle, ivf, ivf.data), cent, lengths


@pytest.mark.parametrize("d", sorted(TILES))
def test_tile_edges(oracle, d):
    ivf, ox, cent, lengths = _edges(d)
    dev = ivf.device_index()
    QT, RB = TILES[d]
    assert dev.knn_probe_tile() == (QT, RB)
    rng = np.random.RandomState(d)
    L = len(lengths)

    def ask(at, P, ks, what):
        qn, qpq = ivf._prepare((cent[at] + 0.25 * rng.randn(len(at), d).astype(np.float32)).astype(np.float32))
        probes = oracle_probes(ox, qn, P)
        assert len(at) == 0 or (probes[:, 0] == at).all()
        everything = radius_probe_csr(oracle, ox, qn, ivf.data, np.inf, P, probes=probes)
        for k in ks:
            got = dev.knn_probe(qn, qpq, k, P, return_distances=True)
            assert got[0].shape == got[1].shape == (len(at), k)
            _same(got, _cut(everything, k), f"d={d} {what} k={k}")
        return everything

    # a query at every centre: every list length once (k = 64 and 1 024 are above the short lists' rows)
    got = ask(np.arange(L), 1, (1, 64, 1024), "own list")
    np.testing.assert_array_equal(np.diff(got[0]), lengths)
    ask(np.arange(L), 3, (64,), "three lists")
    # the 300 identical rows: ties rank by id
    ids, dist = dev.knn_probe(*ivf._prepare(cent[L - 1:].copy()), 300, 2, return_distances=True)
    assert (np.diff(ids[0]) > 0).all() and (dist == 0).all()
    # 1 ... QT + 1 queries on the longest list: the group of 4 queries a lane takes and the tile, both sides
    for n in (1, 3, 4, 5, QT, QT + 1):
        ask(np.full(n, 5), 1, (64,), f"{n} queries on one list")
    ask(np.zeros(0, dtype=np.int64), 2, (5,), "nq=0")


# ---- 3. restrictions --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restricted_case():
    ivf, dev, ox, qn, qpq, data = _fixture("eu20")
    rng = np.random.RandomState(31)
    N, nq = len(data), len(qn)
    b = dict(groups=rng.randint(0, 4, size=N).astype(np.int32), row_tags=rng.randint(1, 256, size=N).astype(np.uint64),
             values=rng.randint(0, 100, size=N).astype(np.int64))
    dev.set_groups(b["groups"])
    dev.set_tags(b["row_tags"])
    dev.set_values(b["values"])
    lo = rng.randint(0, 50, size=nq).astype(np.int64)
    few = np.zeros(N, dtype=bool)
    few[rng.choice(N, 40, replace=False)] = True                       # fewer than k = 10 of them in any 5 lists
    kinds = dict(allowed=dict(allowed=rng.rand(N) < 0.4), exclude=dict(exclude=rng.randint(-1, N, size=nq)),
                 group=dict(group=rng.randint(-1, 4, size=nq).astype(np.int32)),
                 tags_any=dict(tags=rng.randint(0, 16, size=nq).astype(np.uint64), tags_mode="any"),
                 tags_all=dict(tags=rng.randint(0, 16, size=nq).astype(np.uint64), tags_mode="all"),
                 between=dict(between=(lo, lo + 45)), few=dict(allowed=few))
    kinds["all"] = dict(kinds["allowed"], **kinds["exclude"], **kinds["group"], **kinds["tags_any"], **kinds["between"])
    return b, kinds


@pytest.mark.parametrize("kind", ["allowed", "exclude", "group", "tags_any", "tags_all", "between", "all", "few"])
def test_restrictions(oracle, kind):
    ivf, dev, ox, qn, qpq, data = _fixture("eu20")
    b, kinds = _restricted_case()
    kw = dict(kinds[kind])
    ref_kw = dict(kw, **{name: b[name] for name, by in (("groups", "group"), ("row_tags", "tags"), ("values", "between"))
                         if by in kw})
    P, k = 5, 10
    probes = oracle_probes(ox, qn, P)
    if kind == "exclude":                               # every query's own nearest candidate
        kw["exclude"] = ref_kw["exclude"] = _cut(radius_probe_csr(oracle, ox, qn, data, np.inf, P, probes=probes), 1)[0][:, 0]
    oks = [passes(i, len(data), **ref_kw) for i in range(len(qn))]
    want = _cut(radius_probe_csr(oracle, ox, qn, data, np.inf, P, oks=oks, probes=probes), k)
    free = _cut(radius_probe_csr(oracle, ox, qn, data, np.inf, P, probes=probes), k)
    assert (want[0] != free[0]).any() and ((want[0][:, -1] == -1).any() if kind == "few" else (want[0] >= 0).any())
    _same(dev.knn_probe(qn, qpq, k, P, return_distances=True, **kw), want, kind)


# ---- 4. a call cut into query chunks ----------------------------------------------------------------------------------
def test_a_cut_call_is_the_whole_call_and_a_query_over_the_budget_is_refused(oracle):
    from tinyknn_amd import _lib
    ivf, dev, ox, qn, qpq, data = _fixture("eu128")
    P, k = 3, 25
    probes = oracle_probes(ox, qn, P)
    want = _cut(radius_probe_csr(oracle, ox, qn, data, np.inf, P, probes=probes), k)
    _same(dev.knn_probe(qn, qpq, k, P, return_distances=True), want, "uncut")
    need = [4 * sum(int(ox.list_n[l]) for l in set((p % ox.n_lists).tolist())) for p in probes]     # key bytes a query
    try:
        dev.set_option(_lib.OPT_PROBE_BUDGET, max(need))        # every query fits alone, few fit together
        assert sum(need) > 3 * max(need)
        _same(dev.knn_probe(qn, qpq, k, P, return_distances=True), want, "cut")
        dev.set_option(_lib.OPT_PROBE_BUDGET, max(need) - 4)
        with pytest.raises(_lib.TinyKnnHipError, match=f"query {int(np.argmax(need))} alone need {max(need)} bytes"):
            dev.knn_probe(qn, qpq, k, P)
    finally:
        dev.set_option(_lib.OPT_PROBE_BUDGET, 0)
    _same(dev.knn_probe(qn, qpq, k, P, return_distances=True), want, "afterwards")


# ---- 5. the lists change ----------------------------------------------------------------------------------------------
def test_after_remove_add_and_update(oracle):
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(41)
    n, d, L = 1200, 20, 8
    cent = rng.randn(L, d) * 3
    X = (cent[rng.randint(L, size=n)] + 0.5 * rng.randn(n, d)).astype(np.float32)
    Q = (cent[rng.randint(L, size=40)] + 0.5 * rng.randn(40, d)).astype(np.float32)
    ivf = IVF("euclidean", L, FastPQ(2))
    state = np.random.get_state()
    np.random.seed(4)
    try:
        ivf.fit(X).build(X, n_probes=2, device=False)
    finally:
        np.random.set_state(state)
    qn, qpq = ivf._prepare(Q.copy())
    dev = ivf.device_index()

    def check(what):
        ox = oracle_index(oracle, ivf, ivf.data)          # (the IVF's host copies of the lists follow every change)
        got = dev.knn_probe(qn, qpq, 40, 3, return_distances=True)
        _same(got, _cut(radius_probe_csr(oracle, ox, qn, ivf.data, np.inf, 3), 40), what)
        return got[0]

    gone = np.unique(check("built"))[1::3]                  # a third of the rows that were answers
    ivf.remove(gone)
    assert not np.isin(check("removed"), gone).any()
    ivf.add((cent[rng.randint(L, size=150)] + 0.5 * rng.randn(150, d)).astype(np.float32))
    grown = check("added")
    assert (grown >= n).any()
    moved = np.setdiff1d(np.unique(grown[grown >= 0]), gone)[:60]
    ivf.update(moved, (cent[rng.randint(L, size=len(moved))] + 0.5 * rng.randn(len(moved), d)).astype(np.float32))
    check("updated")


# ---- 6. agreement with the radius call --------------------------------------------------------------------------------
def test_the_first_k_of_the_radius_call_are_the_answer():
    ivf, dev, ox, qn, qpq, data = _fixture("an100b2")
    qs = golden("g6_ivf_an100b2.npz")["qs"]
    for P, k in ((2, 10), (10, 50)):
        csr = ivf.radius_search(qs, np.inf, n_probes=P)
        _same(ivf.knn_probe(qs, k, P, return_distances=True), _cut(csr, k), f"P={P}")
        _same(dev.knn_probe(qn, qpq, k, P, return_distances=True), _cut(dev.radius_probe(qn, qpq, np.inf, P), k), f"P={P}")
