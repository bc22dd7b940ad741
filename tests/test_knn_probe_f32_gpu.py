"""knn_probe(wide=True): the distances of knn_probe on the f32 matrix cores for float32-stored vectors (probe_f32.hip,
DESIGN §3.27).  The value behind each key is knn_brute(wide=True)'s part: with every list probed the call must return
that call's ids and bytes; where every product and sum is exact in float32 (integers in [-3, 3]: 2 * 9 * 4096 < 2^24)
it must equal the exact knn_probe, ids and distance bytes; elsewhere every value lies within
B = (d + 4) 2^-23 (|x|^2 + |y|^2 + 2 sum |x_k| |y_k|) of the float64 distance (derived in test_knn_brute_wide_gpu.py for
this chain) and the answer is the right set up to B.

Largest |part - D| / B seen (test_the_bound_and_the_set, MI355X): 0.0077 at d = 129, 0.0045 at d = 300, 0.0012 at
d = 1 536."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from radius_probe_reference import candidates, oracle_probes  # noqa: E402
from store_reference import oracle_index  # noqa: E402
from test_knn_brute_wide_gpu import _ivf  # noqa: E402
from test_knn_probe_gpu import _same  # noqa: E402
from test_knn_probe_matrix_gpu import _ivf as _ivf_half  # noqa: E402
from tinyknn_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
QT, RB = _lib.PROBE_F32_TILE
DS = _lib.PROBE_F32_DS
LENGTHS = [0, 1, 31, 32, 33, RB - 1, RB, RB + 1, 2 * RB + 1]


@functools.lru_cache(maxsize=None)
def _integers(d, n_probes=1):
    """test_knn_probe_matrix_gpu._integers on a float32 store: rows with integer coordinates in [-3, 3]; coordinate 0
    (and 1) names the list, so the lists have LENGTHS rows (d = 1 has seven values: without the lists of 32 and RB rows)"""
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
    ivf = _ivf(X, cent)
    if n_probes == 1:
        ivf.remove(np.flatnonzero(member == 0))
        assert [len(ivf.ids[l]) for l in range(L)] == lengths
    else:
        ivf.build(X, n_probes=n_probes, device=False)       # (again: every row in its n_probes nearest lists)
    return ivf, ivf.device_index(), rng.randint(-3, 4, size=(QT + 1, d)).astype(np.float32)


def _both(ivf, dev, Q, k, P, **kw):
    qn, qpq = ivf._prepare(Q.copy())
    want = dev.knn_probe(qn, qpq, k, P, return_distances=True, **kw)
    _same(dev.knn_probe(qn, qpq, k, P, return_distances=True, wide=True, **kw), want, f"k={k} P={P}")
    return want


# every query probes every list: each list length meets each tile size
@pytest.mark.parametrize("d,nq", [(d, QT + 1) for d in (1, 2, 3, 7, DS - 1, DS, DS + 1, 2 * DS + 1, 128, 129, 300, 4096)]
                         + [(129, n) for n in (1, 31, 32, 33, QT)])
def test_integer_data_is_the_exact_call(d, nq):
    ivf, dev, Q = _integers(d)
    for k in (1, 10, 300):
        ids, dist = _both(ivf, dev, Q[:nq], k, len(ivf.ids))
    assert ids.shape == (nq, 300) and (ids >= 0).all()


def _randn(metric, d):
    rng = np.random.RandomState(d)
    scale = 1.0 if metric == "angular" else 30.0
    X, Q = (scale * rng.randn(1200, d)).astype(np.float32), (scale * rng.randn(QT + 3, d)).astype(np.float32)
    ivf = _ivf(X, X[:6], metric)
    return ivf, ivf.device_index(), ivf._prepare(Q.copy())


@pytest.mark.parametrize("metric,d", [(m, d) for m in ("angular", "euclidean") for d in (17, 100, 129, 300)])
def test_every_list_probed_is_knn_brute_wide(metric, d):
    """the chain order, the carry across slabs on rounded values, and the norms summed inside the kernel"""
    ivf, dev, (qn, qpq) = _randn(metric, d)
    _same(dev.knn_probe(qn, qpq, 10, 6, return_distances=True, wide=True), dev.knn_brute_dist(qn, 10, wide=True))


@pytest.mark.parametrize("metric,d", [(m, d) for m in ("angular", "euclidean") for d in (129, 300, 1536)])
def test_the_bound_and_the_set(oracle, metric, d):
    """|part - D| <= B against float64; the returned ids are candidates of the oracle's probes, ascending by (part, id);
    with tau the k-th part every candidate with D < tau - B is returned"""
    k, P = 10, 3
    ivf, dev, (qn, qpq) = _randn(metric, d)
    ids, part = dev.knn_probe(qn, qpq, k, P, return_distances=True, wide=True)
    ox = oracle_index(oracle, ivf, ivf.data)
    probes = oracle_probes(ox, qn, P)
    worst = 0.0
    for i in range(len(qn)):
        cand = candidates(ox, probes[i], len(ivf.data))
        x, Y = qn[i].astype(np.float64), ivf.data[cand].astype(np.float64)
        D = ((x - Y) ** 2).sum(axis=1)
        B = (d + 4) * 2.0 ** -23 * ((x ** 2).sum() + (Y ** 2).sum(axis=1) + 2 * (np.abs(x) * np.abs(Y)).sum(axis=1))
        live = ids[i] >= 0
        assert live.sum() == min(k, len(cand)) and np.isin(ids[i][live], cand).all()
        at = np.searchsorted(cand, ids[i][live])
        err = np.abs(part[i][live].astype(np.float64) - D[at])
        worst = max(worst, float((err / B[at]).max()))
        assert (err <= B[at]).all(), (i, err / B[at])
        tau = float(part[i][k - 1])                         # (+inf where fewer than k candidates: all are returned)
        assert np.isin(cand[D < tau - B], ids[i]).all(), i
        order = np.lexsort((ids[i][live], part[i][live]))
        assert (order == np.arange(live.sum())).all(), i
    print(f"{metric} d={d}: largest |part - D| / B = {worst:.4f}")


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


@pytest.mark.parametrize("case", ["float16", "float64", "both"])
def test_refusals_leave_the_index_usable(case):
    rng = np.random.RandomState(9)
    X = rng.randn(600, 20).astype(np.float32)
    ivf = _ivf_half(X, X[:4]) if case == "float16" else _ivf(X, X[:4], store="float64" if case == "float64" else "float32")
    dev = ivf.device_index()
    qn, qpq = ivf._prepare(X[:8].copy())
    with pytest.raises(ValueError if case == "both" else AssertionError, match="not both" if case == "both" else 'store="float32"'):
        dev.knn_probe(qn, qpq, 5, 2, wide=True, matrix=case == "both")
    assert (dev.knn_probe(qn, qpq, 5, 2) >= 0).all()
