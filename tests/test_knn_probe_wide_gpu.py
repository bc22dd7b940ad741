"""knn_probe's wide distance kernel (probe_dist_wide_kernel, DESIGN §3.21: d walked in slabs, d <= 4096) against the
reference of the radius call over the same lists (tests/radius_probe_reference.py at radius +inf) cut to k and padded
with -1 / +inf: ids equal, distances the same dtype and bytes.  At the widths the whole-row kernel refuses the kernel is
chosen by width; at the slab edges it is forced with TK_OPT_PROBE_WIDE on rows of a few KB."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from radius_probe_reference import oracle_probes, passes, radius_probe_csr  # noqa: E402
from store_reference import oracle_index, rounded  # noqa: E402
from test_knn_probe_gpu import _cut, _fixture, _restricted_case, _same  # noqa: E402
from tinyknn_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
QT, RB = _lib.PROBE_WIDE_TILE
LENGTHS = [0, 1, RB - 1, RB, RB + 1, 2 * RB + 3, 300]


def _index(d, store):
    """test_knn_probe_gpu._edges for a vector store, lists of LENGTHS rows, the last one copies of its centre; FastPQ(2)
    fitted behind a rotation to at most 64 dims that costs O(d) to draw (fit() draws a d x d matrix)"""
    from oracle import oracle
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import dpad
    from tinyknn_amd.utils import pad2
    oracle.build()
    rng = np.random.RandomState(900 + d)
    L = len(LENGTHS)
    cent = np.zeros((L, d), dtype=np.float32)
    if d >= L:
        cent[np.arange(L), np.arange(L)] = 8.0
    else:
        cent[:, 0] = 8.0 * np.arange(L)
    member = np.repeat(np.arange(L), [max(n, 1) for n in LENGTHS])
    X = (cent[member] + 0.5 * rng.randn(len(member), d).astype(np.float32)).astype(np.float32)
    X[member == L - 1] = cent[L - 1]
    perm = rng.permutation(len(X))
    X, member = np.ascontiguousarray(X[perm]), member[perm]
    X = rounded(X) if store == "float16" else X.astype(np.float64) if store == "float64" else X
    ivf = IVF("euclidean", L, FastPQ(2))
    ivf.all_centers = cent
    P = pad2(X, 16, dpad * 2)
    ivf.pq.R = np.ascontiguousarray(np.linalg.qr(rng.randn(P.shape[1], 64))[0].T)
    state = np.random.get_state()
    np.random.seed(77)
    try:
        ivf.pq.centers = np.array(ivf.pq._fit_code(P @ ivf.pq.R.T), dtype=np.float32).transpose(1, 0, 2).reshape(16, -1)
        ivf.pq.sqrt_n_blocks = np.sqrt(ivf.pq.centers.shape[1] // 2)
        ivf.build(X, n_probes=1, device=False)
    finally:
        np.random.set_state(state)
    ivf.remove(np.flatnonzero(member == 0))
    assert [len(ivf.ids[l]) for l in range(L)] == LENGTHS
    ivf.store = "float16" if store == "float16" else None
    dev = ivf.device_index()
    assert dev.store == store
    return ivf, dev, oracle_index(oracle, ivf, ivf.data), cent


def _lists_and_queries(oracle, d, store, wide, tile=(QT, RB)):
    ivf, dev, ox, cent = _index(d, store)
    dev.set_option(_lib.OPT_PROBE_WIDE, wide)
    assert dev.knn_probe_tile() == tile
    rng = np.random.RandomState(d)
    L = len(LENGTHS)

    def ask(at, P, ks, what):
        qn, qpq = ivf._prepare((cent[at] + 0.25 * rng.randn(len(at), d).astype(np.float32)).astype(np.float32))
        probes = oracle_probes(ox, qn, P)
        assert (probes[:, 0] == at).all()
        everything = radius_probe_csr(oracle, ox, qn, ivf.data, np.inf, P, probes=probes)
        for k in ks:
            _same(dev.knn_probe(qn, qpq, k, P, return_distances=True), _cut(everything, k), f"{store} d={d} {what} k={k}")
        return everything

    np.testing.assert_array_equal(np.diff(ask(np.arange(L), 1, (1, 64), "own list")[0]), LENGTHS)
    ask(np.arange(L), 3, (1, 64), "three lists")
    # the 300 identical rows rank by id; then 1 ... QT + 1 queries on the longest list of distinct rows and of all rows
    ids, dist = dev.knn_probe(*ivf._prepare(cent[L - 1:].copy()), 300, 2, return_distances=True)
    assert (np.diff(ids[0]) > 0).all() and (dist == 0).all()
    for n in (1, 3, 4, 5, QT, QT + 1):
        for l in (L - 2, L - 1):
            ask(np.full(n, l), 1, (64,), f"{n} queries on list {l}")


# The first width the whole-row kernel refuses is 1 365 on float32 vectors, 2 041 on half, 683 on float64 (element loads
# and a tail, each); 1 351 and 681, once documented as refused, fit it with its smallest tile and keep it.
@pytest.mark.parametrize("store,d", [("float32", 1351), ("float32", 1365), ("float32", 1536), ("float32", 4096),
                                     ("float16", 2041), ("float16", 3072), ("float16", 4096), ("float64", 681),
                                     ("float64", 683), ("float64", 4096)])
def test_real_widths_the_kernel_chosen_by_width(oracle, store, d):
    _lists_and_queries(oracle, d, store, 0, (4, 8) if d in (1351, 681) else (QT, RB))


@pytest.mark.parametrize("store,d", [(s, d) for s, L4 in (("float32", 16), ("float16", 16), ("float64", 8))   # L4 = 4 * L
                                     for DS in (_lib.PROBE_WIDE_DS[s],)
                                     for d in (1, L4 - 1, L4, L4 + 1, DS - 1, DS, DS + 1, 2 * DS + 5)])
def test_slab_edges_forced_wide(oracle, store, d):
    _lists_and_queries(oracle, d, store, 1)


@pytest.mark.parametrize("tag", ["eu20", "an100b2"])
def test_forced_on_the_fixtures_is_the_unforced_call(tag):
    ivf, dev, ox, qn, qpq, data = _fixture(tag)
    want = dev.knn_probe(qn, qpq, 50, 10, return_distances=True)
    narrow = dev.knn_probe_tile()
    try:
        dev.set_option(_lib.OPT_PROBE_WIDE, 1)
        assert dev.knn_probe_tile() == (QT, RB) != narrow
        _same(dev.knn_probe(qn, qpq, 50, 10, return_distances=True), want, tag)
    finally:
        dev.set_option(_lib.OPT_PROBE_WIDE, 0)
    assert dev.knn_probe_tile() == narrow


def test_all_restrictions_forced_wide(oracle):
    ivf, dev, ox, qn, qpq, data = _fixture("eu20")
    b, kinds = _restricted_case()
    oks = [passes(i, len(data), **kinds["all"], **b) for i in range(len(qn))]
    want = _cut(radius_probe_csr(oracle, ox, qn, data, np.inf, 5, oks=oks), 10)
    try:
        dev.set_option(_lib.OPT_PROBE_WIDE, 1)
        _same(dev.knn_probe(qn, qpq, 10, 5, return_distances=True, **kinds["all"]), want)
    finally:
        dev.set_option(_lib.OPT_PROBE_WIDE, 0)


def test_a_cut_wide_call_is_the_whole_call(oracle):
    ivf, dev, ox, cent = _index(1365, "float32")
    assert dev.knn_probe_tile() == (QT, RB)
    qn, qpq = ivf._prepare(np.repeat(cent, 3, axis=0) + np.float32(0.125))
    want = _cut(radius_probe_csr(oracle, ox, qn, ivf.data, np.inf, 3), 25)
    _same(dev.knn_probe(qn, qpq, 25, 3, return_distances=True), want, "uncut")
    dev.set_option(_lib.OPT_PROBE_BUDGET, 4 * sum(sorted(LENGTHS)[-3:]))      # a query's three longest lists, no more
    _same(dev.knn_probe(qn, qpq, 25, 3, return_distances=True), want, "cut")


def test_d_4097_is_refused_and_the_index_stays_usable():
    ivf, dev, ox, cent = _index(4097, "float32")
    qn, qpq = ivf._prepare(cent.copy())
    for call in (lambda: dev.knn_probe(qn, qpq, 3, 2), dev.knn_probe_tile):
        with pytest.raises(AssertionError, match="d <= 4096"):
            call()
    assert dev.query_batch(qn, qpq, 3, 2).shape == (len(cent), 3)
