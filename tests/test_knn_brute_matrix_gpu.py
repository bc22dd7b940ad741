"""knn_brute(matrix=True): the exact search over all rows of a half store on the f16 matrix cores (brute_matrix.hip,
DESIGN §3.23).  On integer data every product and sum is exact in float32, so ids and distance bytes are numpy's; on
other data the call returns knn_probe(matrix=True)'s bytes with every list probed, within §3.22's B of float64.

Largest |dist_m - D| / B seen (test_one_dist_m, MI355X): 0.038 at d = 17, 0.009 at d = 100, 0.0015 at d = 1 536.
k = 300 is cut to N where the index has fewer rows (k <= N is the call's own condition)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from brute_reference import CAP, int_part, k_best, segment_rows, within_tau_per_segment  # noqa: E402
from brute_restricted_reference import passes, restricted_dist, restricted_k_best  # noqa: E402
from store_reference import rounded  # noqa: E402
from test_knn_probe_gpu import _same  # noqa: E402
from test_knn_probe_matrix_gpu import _ivf  # noqa: E402
from tinyknn_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
QT, RB = _lib.BRUTE_MATRIX_TILE
DS = _lib.BRUTE_MATRIX_DS


@functools.lru_cache(maxsize=None)
def _integers(d, n, nq=QT + 1, lim=3):
    """a half-store index over n rows with integer coordinates in [-lim, lim], its device copy, nq such queries and
    the exact int64 distances of every (query, row)"""
    rng = np.random.RandomState(1000 * d + n)
    X = rng.randint(-lim, lim + 1, size=(n, d)).astype(np.float32)
    ivf = _ivf(X, rng.randn(4, d))
    Q = rng.randint(-lim, lim + 1, size=(nq, d)).astype(np.float32)
    return ivf, ivf.device_index(), Q, int_part(Q, rounded(ivf.data))


def _check(dev, Q, D, k, oks=None, **kw):
    ids, dist = dev.knn_brute_dist(Q, k, matrix=True, **kw)
    for i in range(len(Q)):
        ok = np.ones(D.shape[1], dtype=bool) if oks is None else oks[i]
        want = restricted_k_best(D[i], ok, k)
        np.testing.assert_array_equal(ids[i], want, err_msg=f"query {i} k={k}")
        assert dist[i].tobytes() == restricted_dist(D[i], want).tobytes(), (i, k)
    return ids


@pytest.mark.parametrize("d,n,nq", [(d, 700, QT + 1) for d in (1, 7, 8, 15, 16, 17, 100, DS - 1, DS, DS + 1, 2 * DS + 1, 4096)]
                         + [(17, n, QT + 1) for n in (300, RB - 1, RB, RB + 1, 2 * RB + 1)]
                         + [(17, 700, nq) for nq in (1, 31, 32, 33, 63, 64, 65, QT - 1, QT)])
def test_integer_data_is_numpys(d, n, nq):
    ivf, dev, Q, D = _integers(d, n)
    for k in (1, 10, 300 if n >= 300 else n):
        _check(dev, Q[:nq], D[:nq], k)
        np.testing.assert_array_equal(dev.knn_brute(Q[:nq], k, matrix=True), [k_best(D[i], k) for i in range(nq)])


N_R = 2 * 8192          # the sample is every second row


@functools.lru_cache(maxsize=None)
def _restricted():
    ivf, dev, Q, D = _integers(100, N_R)
    rng = np.random.RandomState(3)
    nq = len(Q)
    rows = dict(groups=rng.randint(0, 4, size=N_R).astype(np.int32), row_tags=rng.randint(1, 256, size=N_R).astype(np.uint64),
                values=rng.randint(0, 100, size=N_R).astype(np.int64))
    rows["groups"][:5] = 4                                          # a group of 5 rows: fewer than k pass
    dev.set_groups(rows["groups"])
    dev.set_tags(rows["row_tags"])
    dev.set_values(rows["values"])
    group = rng.randint(-1, 4, size=nq).astype(np.int32)
    group[::7] = 4
    kw = dict(allowed=rng.rand(N_R) < 0.5, exclude=rng.randint(-1, N_R, size=nq), group=group,
              tags=rng.randint(0, 16, size=nq).astype(np.uint64),
              between=(np.zeros(nq, np.int64), np.full(nq, 60, np.int64)),
              unsampled=np.arange(N_R) % 2 == 1)                    # no sample row passes: tau = +inf
    return dev, Q, D, rows, kw


@pytest.mark.parametrize("which", ["all", "allowed", "exclude", "group", "tags", "between", "unsampled"])
def test_restrictions(which):
    dev, Q, D, rows, kw = _restricted()
    names = ["allowed", "exclude", "group", "tags", "between"] if which == "all" else [which]
    kw = {("allowed" if n == "unsampled" else n): kw[n] for n in names}
    oks = [passes(i, N_R, **kw, **rows) for i in range(len(Q))]
    ids = _check(dev, Q, D, 10, oks, **kw)
    assert (ids[:, -1] == -1).any() == (which in ("all", "group"))


@pytest.mark.parametrize("metric,d", [(m, d) for m in ("angular", "euclidean") for d in (17, 100, 1536)])
def test_one_dist_m(metric, d):
    """the bytes of knn_probe(matrix=True) with every list probed, each within B = (2d + 8) 2^-24 (|x|^2 + |y|^2 + 2S)
    + 2^-21 S of the float64 distance"""
    rng = np.random.RandomState(d)
    scale = 1.0 if metric == "angular" else 30.0
    X, Q = (scale * rng.randn(1200, d)).astype(np.float32), (scale * rng.randn(40, d)).astype(np.float32)
    ivf = _ivf(X, X[:6], metric)
    dev = ivf.device_index()
    qn, qpq = ivf._prepare(Q.copy())
    ids, dm = dev.knn_brute_dist(qn, 10, matrix=True)
    _same((ids, dm), dev.knn_probe(qn, qpq, 10, len(ivf.ids), return_distances=True, matrix=True), f"{metric} d={d}")
    x, Y = qn.astype(np.float64)[:, None, :], rounded(ivf.data).astype(np.float64)[ids]
    Dt, S = ((x - Y) ** 2).sum(axis=2), (np.abs(x) * np.abs(Y)).sum(axis=2)
    B = (2 * d + 8) * 2.0 ** -24 * ((x ** 2).sum(axis=2) + (Y ** 2).sum(axis=2) + 2 * S) + 2.0 ** -21 * S
    err = np.abs(dm.astype(np.float64) - Dt)
    print(f"{metric} d={d}: largest |dist_m - D| / B = {(err / B).max():.4f}")
    assert (err <= B).all(), (err / B).max()


@pytest.mark.parametrize("nq", [3, 130])
def test_several_segments(nq):
    n, k = 300_000, 100
    ivf, dev, Q, D = _integers(8, n, 130, 100)
    assert segment_rows(k, n) == 2 ** 17 and n % 2 ** 17 and -(-n // 2 ** 17) == 3
    for i in range(nq):
        assert max(within_tau_per_segment(D[i], k)) + k <= CAP, i
    _check(dev, Q[:nq], D[:nq], k)


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
        dev.knn_brute(bad, 5, matrix=True)
    assert (dev.knn_probe(qn, qpq, 5, 2) >= 0).all()
    if case in ("nan", "inf"):
        assert (dev.knn_brute(qn, 5, matrix=True) >= 0).all()
        with pytest.raises(AssertionError, match="half"):
            dev.knn_brute(qn, 5)
