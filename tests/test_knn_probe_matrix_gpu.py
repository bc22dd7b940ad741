"""knn_probe(matrix=True): the distances of knn_probe on the f16 matrix cores for half-stored vectors (probe_matrix.hip,
DESIGN §3.22).  Where every product and sum is exact in float32 the call must equal the exact call, ids and distance
bytes; elsewhere every distance lies within B of the float64 distance and the answer is the right set up to B.

Subnormal rows: rows m * 2^-24, |m| <= 1023, must give the exact call's bytes unless the instruction flushes them.  With
an integer query neither call is exact (3 - m * 2^-24 needs 26 bits; at d = 100 sum m^2 passes 2^24), so the case is
drawn where the premise "every product and sum is exact" holds: queries in {-1, 0, 1} * 2^-24 and, at d = 100, 15
nonzero coordinates a row — sum (x - y)^2 <= 15 * 1024^2 + 85 <= 2^24.  The rows stay half subnormals with |m| <= 1023."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from radius_probe_reference import candidates, oracle_probes  # noqa: E402
from store_reference import oracle_index, rounded  # noqa: E402
from test_knn_probe_gpu import _same  # noqa: E402
from tinyknn_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
QT, RB = _lib.PROBE_MATRIX_TILE
DS = _lib.PROBE_MATRIX_DS
LENGTHS = [0, 1, 31, 32, 33, RB - 1, RB, RB + 1, 2 * RB + 1]


def _ivf(X, cent, metric="euclidean", n_probes=1):
    """A half-store IVF over X with the centres set by hand; FastPQ(2) fitted behind a rotation to at most 64 dims that
    costs O(d) to draw (test_knn_probe_wide_gpu._index)"""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import dpad
    from tinyknn_amd.utils import pad2
    rng = np.random.RandomState(5)
    ivf = IVF(metric, len(cent), FastPQ(2))
    cent = cent / np.linalg.norm(cent, axis=1, keepdims=True) if metric == "angular" else cent
    ivf.all_centers = np.ascontiguousarray(cent, dtype=np.float32)
    P = pad2(X, 16, dpad * 2)
    ivf.pq.R = np.ascontiguousarray(np.linalg.qr(rng.randn(P.shape[1], 64))[0].T)
    state = np.random.get_state()
    np.random.seed(77)
    try:
        ivf.pq.centers = np.array(ivf.pq._fit_code(P @ ivf.pq.R.T), dtype=np.float32).transpose(1, 0, 2).reshape(16, -1)
        ivf.pq.sqrt_n_blocks = np.sqrt(ivf.pq.centers.shape[1] // 2)
        ivf.build(X, n_probes=n_probes, device=False, store="float16")
    finally:
        np.random.set_state(state)
    return ivf


@functools.lru_cache(maxsize=None)
def _integers(d, n_probes=1):
    """rows with integer coordinates in [-3, 3]; coordinate 0 (and 1) names the list, so the lists have LENGTHS rows
    (d = 1 has seven values: without the lists of 32 and RB rows)"""
    rng = np.random.RandomState(100 + d)
    lengths = LENGTHS if d > 1 else [n for n in LENGTHS if n not in (32, RB)]
    L = len(lengths)
    cent = np.zeros((L, d), dtype=np.float32)
    cent[:, 0] = np.arange(L) % 7 - 3
    if d > 1:
        cent[:, 1] = 3 * (np.arange(L) // 7)
    member = np.repeat(np.arange(L), [max(n, 1) for n in lengths])
    X = rng.randint(-3, 4, size=(len(member), d)).astype(np.float32)
    X[:, :2] = cent[member][:, :2]
    perm = rng.permutation(len(X))
    X, member = np.ascontiguousarray(X[perm]), member[perm]
    ivf = _ivf(X, cent, n_probes=n_probes)
    if n_probes == 1:
        ivf.remove(np.flatnonzero(member == 0))
        assert [len(ivf.ids[l]) for l in range(L)] == lengths
    return ivf, ivf.device_index(), rng.randint(-3, 4, size=(QT + 1, d)).astype(np.float32)


def _both(ivf, dev, Q, k, P, **kw):
    qn, qpq = ivf._prepare(Q.copy())
    want = dev.knn_probe(qn, qpq, k, P, return_distances=True, **kw)
    _same(dev.knn_probe(qn, qpq, k, P, return_distances=True, matrix=True, **kw), want, f"k={k} P={P}")
    return want


# every query probes every list: each list length meets each tile size
@pytest.mark.parametrize("d,nq", [(d, QT + 1) for d in (1, 7, 8, 15, 16, 17, 100, DS - 1, DS, DS + 1, 2 * DS + 1, 4096)]
                         + [(17, n) for n in (1, 31, 32, 33, QT)])
def test_integer_data_is_the_exact_call(d, nq):
    ivf, dev, Q = _integers(d)
    for k in (1, 10, 300):
        ids, dist = _both(ivf, dev, Q[:nq], k, len(ivf.ids))
    assert ids.shape == (nq, 300) and (ids >= 0).all()


def test_integer_twins_restrictions_a_cut_call_and_changed_lists():
    ivf, dev, Q = _integers(100, n_probes=2)
    assert dev.twin_table_width() == 1
    _both(ivf, dev, Q, 10, 3)
    N = len(ivf.data)
    rng = np.random.RandomState(3)
    dev.set_groups(rng.randint(0, 4, size=N).astype(np.int32))
    dev.set_tags(rng.randint(1, 256, size=N).astype(np.uint64))
    dev.set_values(rng.randint(0, 100, size=N).astype(np.int64))
    _both(ivf, dev, Q, 10, 3, allowed=rng.rand(N) < 0.5, exclude=rng.randint(-1, N, size=len(Q)),
          group=rng.randint(-1, 4, size=len(Q)).astype(np.int32), tags=rng.randint(0, 16, size=len(Q)).astype(np.uint64),
          between=(np.zeros(len(Q), np.int64), np.full(len(Q), 60, np.int64)))
    ivf, dev, Q = _integers(17)
    want = _both(ivf, dev, Q, 10, 4)
    try:
        dev.set_option(_lib.OPT_PROBE_BUDGET, 4 * sum(sorted(LENGTHS)[-4:]))     # a query's four longest lists, no more
        _same(_both(ivf, dev, Q, 10, 4), want, "cut")
    finally:
        dev.set_option(_lib.OPT_PROBE_BUDGET, 0)
    ivf, dev, Q = _integers.__wrapped__(15)                 # (its own copy: the lists change)
    rng = np.random.RandomState(4)
    live = np.sort(np.concatenate([np.asarray(l, dtype=np.int64) for l in ivf.ids]))
    ivf.remove(live[0:300:3])
    ivf.add(rng.randint(-3, 4, size=(150, 15)).astype(np.float32))
    ivf.update(live[1:200:3], rng.randint(-3, 4, size=(67, 15)).astype(np.float32))
    _both(ivf, dev, Q, 40, len(ivf.ids))


@pytest.mark.parametrize("d", [16, 100])
def test_subnormal_rows_are_not_flushed(d):
    rng = np.random.RandomState(d)
    M = rng.randint(-1023, 1024, size=(700, d))
    if d > 16:
        M[np.argsort(rng.rand(*M.shape), axis=1) >= 15] = 0
    X = (M * 2.0 ** -24).astype(np.float32)
    ivf = _ivf(X, X[:5])
    ids, dist = _both(ivf, ivf.device_index(), (rng.randint(-1, 2, size=(QT + 1, d)) * 2.0 ** -24).astype(np.float32), 10, 5)
    assert (ids >= 0).all() and (dist > 0).any()


@pytest.mark.parametrize("metric,d", [(m, d) for m in ("angular", "euclidean") for d in (16, 17, 100, 1536)]
                         + [("split", 16)])
def test_the_bound_and_the_set(oracle, metric, d):
    """|dist_m - D| <= B = (2d + 8) 2^-24 (|x|^2 + |y|^2 + 2S) + 2^-21 S against float64; with tau the k-th dist_m every
    candidate with D < tau - B is returned and every returned row has D <= tau + B; ascending by (dist_m, id)"""
    rng = np.random.RandomState(d)
    n, nq, k, P = 1200, 40, 10, 3
    if metric == "split":                                   # queries that need more than 11 bits: x_lo matters
        X = rng.randint(-3, 4, size=(n, d)).astype(np.float32)
        Q = (rng.randint(-3, 4, size=(nq, d)) + rng.randint(-3, 4, size=(nq, d)) * 2.0 ** -11).astype(np.float32)
    else:
        scale = 1.0 if metric == "angular" else 30.0
        X, Q = (scale * rng.randn(n, d)).astype(np.float32), (scale * rng.randn(nq, d)).astype(np.float32)
    ivf = _ivf(X, X[:6], "euclidean" if metric == "split" else metric)
    dev = ivf.device_index()
    qn, qpq = ivf._prepare(Q.copy())
    stored = rounded(ivf.data)
    ids, dm = dev.knn_probe(qn, qpq, k, P, return_distances=True, matrix=True)
    ox = oracle_index(oracle, ivf, stored)
    probes = oracle_probes(ox, qn, P)
    worst = 0.0
    for i in range(nq):
        cand = candidates(ox, probes[i], len(stored))
        x, Y = qn[i].astype(np.float64), stored[cand].astype(np.float64)
        D, S = ((x - Y) ** 2).sum(axis=1), (np.abs(x) * np.abs(Y)).sum(axis=1)
        B = (2 * d + 8) * 2.0 ** -24 * ((x ** 2).sum() + (Y ** 2).sum(axis=1) + 2 * S) + 2.0 ** -21 * S
        live = ids[i] >= 0
        assert live.sum() == min(k, len(cand)) and np.isin(ids[i][live], cand).all()
        at = np.searchsorted(cand, ids[i][live])
        err = np.abs(dm[i][live].astype(np.float64) - D[at])
        worst = max(worst, float((err / B[at]).max()))
        assert (err <= B[at]).all(), (i, err / B[at])
        tau = float(dm[i][k - 1])                           # (+inf where fewer than k candidates: all are returned)
        assert np.isin(cand[D < tau - B], ids[i]).all() and (D[at] <= tau + B[at]).all(), i
        order = np.lexsort((ids[i][live], dm[i][live]))
        assert (order == np.arange(live.sum())).all(), i
    print(f"{metric} d={d}: largest |dist_m - D| / B = {worst:.4f}")


@pytest.mark.parametrize("case", ["float32", "float64", "nan", "inf"])
def test_refusals_leave_the_index_usable(case):
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(9)
    X = rng.randn(600, 20).astype(np.float32)
    if case in ("nan", "inf"):
        ivf = _ivf(X, X[:4])
    else:
        ivf = IVF("euclidean", 4, FastPQ(2))
        ivf.fit(X).build(X.astype(case), n_probes=1, device=False)
    dev = ivf.device_index()
    qn, qpq = ivf._prepare(X[:8].copy())
    bad = qn.copy()
    if case in ("nan", "inf"):
        bad[3, 7] = np.nan if case == "nan" else -np.inf
    with pytest.raises(AssertionError, match='needs store="float16"' if case.startswith("float") else "NaN or an infinity"):
        dev.knn_probe(bad, qpq, 5, 2, matrix=True)
    assert (dev.knn_probe(qn, qpq, 5, 2) >= 0).all()
