"""knn_brute(wide=True): the exact search over all rows of a float32 store of any d <= 4096 (brute_wide.hip, DESIGN
§3.25).  On integer data every product and sum is exact in float32 (2 * 9 * 4096 < 2^24), so ids and distance bytes are
numpy's; at d <= 128 the call returns the bytes of the default call; trailing zero columns change nothing; elsewhere
every value lies within B = (d + 4) 2^-23 (|x|^2 + |y|^2 + 2S), S = sum |x_k| |y_k|, of the float64 distance: to first
order the chain, the two norms and the two final operations give (d + 2) 2^-24 of that sum, and twice that covers the
higher-order terms at d 2^-24 <= 2^-12.

Largest |part - D| / B seen (test_within_the_bound_of_float64, MI355X): 0.011 at d = 129, 0.0048 at d = 300, 0.0015 at
d = 1 536.
k = 300 is cut to N where the index has fewer rows (k <= N is the call's own condition)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from brute_reference import CAP, int_part, k_best, segment_rows, within_tau_per_segment  # noqa: E402
from brute_restricted_reference import passes, restricted_dist, restricted_k_best  # noqa: E402
from test_knn_probe_matrix_gpu import _ivf as _ivf_half  # noqa: E402
from tinyknn_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
QT, RB = _lib.BRUTE_WIDE_TILE
DS = _lib.BRUTE_WIDE_DS


def _ivf(X, cent, metric="euclidean", store="float32"):
    """test_knn_probe_matrix_gpu._ivf for a float32 (or float64) store: the centres set by hand, FastPQ(2) fitted behind
    a rotation to at most 64 dims that costs O(d) to draw"""
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
        ivf.build(X.astype(store), n_probes=1, device=False)
    finally:
        np.random.set_state(state)
    return ivf


@functools.lru_cache(maxsize=None)
def _integers(d, n, nq=QT + 1, lim=3):
    """test_knn_brute_matrix_gpu._integers on a float32 store: n rows with integer coordinates in [-lim, lim], the
    device copy, nq such queries and the exact int64 distances of every (query, row)"""
    rng = np.random.RandomState(1000 * d + n)
    X = rng.randint(-lim, lim + 1, size=(n, d)).astype(np.float32)
    ivf = _ivf(X, rng.randn(4, d))
    Q = rng.randint(-lim, lim + 1, size=(nq, d)).astype(np.float32)
    return ivf.device_index(), Q, int_part(Q, ivf.data)


def _check(dev, Q, D, k, oks=None, **kw):
    ids, dist = dev.knn_brute_dist(Q, k, wide=True, **kw)
    for i in range(len(Q)):
        ok = np.ones(D.shape[1], dtype=bool) if oks is None else oks[i]
        want = restricted_k_best(D[i], ok, k)
        np.testing.assert_array_equal(ids[i], want, err_msg=f"query {i} k={k}")
        assert dist[i].tobytes() == restricted_dist(D[i], want).tobytes(), (i, k)
    return ids


@pytest.mark.parametrize("d,n,nq", [(d, 700, QT + 1) for d in (1, 2, 3, 7, DS - 1, DS, DS + 1, 2 * DS + 1, 128, 129, 300, 4096)]
                         + [(129, n, QT + 1) for n in (300, RB - 1, RB, RB + 1, 2 * RB + 1)]
                         + [(129, 700, nq) for nq in (1, 31, 32, 33, 63, 64, 65, QT - 1, QT)])
def test_integer_data_is_numpys(d, n, nq):
    dev, Q, D = _integers(d, n)
    for k in (1, 10, 300 if n >= 300 else n):
        _check(dev, Q[:nq], D[:nq], k)
        np.testing.assert_array_equal(dev.knn_brute(Q[:nq], k, wide=True), [k_best(D[i], k) for i in range(nq)])


def _randn(metric, d, zero_from=None):
    rng = np.random.RandomState(d)
    scale = 1.0 if metric == "angular" else 30.0
    X, Q = (scale * rng.randn(1200, d)).astype(np.float32), (scale * rng.randn(QT + 3, d)).astype(np.float32)
    if zero_from is not None:
        X[:, zero_from:] = Q[:, zero_from:] = 0.0
    return X, Q


@pytest.mark.parametrize("metric,d", [(m, d) for m in ("angular", "euclidean") for d in (17, 100, 128)])
def test_the_bytes_of_the_default_call(metric, d):
    """the chain order, the carry across slabs on rounded values, and the norms"""
    X, Q = _randn(metric, d)
    ivf = _ivf(X, X[:6], metric)
    dev, qn = ivf.device_index(), ivf._prepare(Q.copy())[0]
    ids, part = dev.knn_brute_dist(qn, 10, wide=True)
    want_ids, want = dev.knn_brute_dist(qn, 10)
    np.testing.assert_array_equal(ids, want_ids)
    assert part.tobytes() == want.tobytes()
    np.testing.assert_array_equal(dev.knn_brute(qn, 10, wide=True), want_ids)


@pytest.mark.parametrize("d", [129, 300])
def test_zero_columns_change_nothing(d):
    """the FMA chain and the einsum order (zero lanes add exactly 0 in the 3, 2, 1, 0 fold) under trailing zeros"""
    X, Q = _randn("euclidean", d, zero_from=100)
    wide, narrow = _ivf(X, X[:6]).device_index(), _ivf(X[:, :100].copy(), X[:6, :100]).device_index()
    ids, part = wide.knn_brute_dist(Q, 10, wide=True)
    want_ids, want = narrow.knn_brute_dist(np.ascontiguousarray(Q[:, :100]), 10)
    np.testing.assert_array_equal(ids, want_ids)
    assert part.tobytes() == want.tobytes()


@pytest.mark.parametrize("metric,d", [(m, d) for m in ("angular", "euclidean") for d in (129, 300, 1536)])
def test_within_the_bound_of_float64(metric, d):
    """every value within B of the float64 distance of its id, ascending, and the k-th returned row at most 2 max B past
    the true k-th distance: the k truly nearest rows all have part <= D_k + max B, so the k-th smallest part is no more"""
    k = 10
    X, Q = _randn(metric, d)
    ivf = _ivf(X, X[:6], metric)
    dev, qn = ivf.device_index(), ivf._prepare(Q.copy())[0]
    ids, part = dev.knn_brute_dist(qn, k, wide=True)
    x, Y = qn.astype(np.float64), ivf.data.astype(np.float64)
    Dt = (x ** 2).sum(axis=1)[:, None] + (Y ** 2).sum(axis=1)[None] - 2 * x @ Y.T
    B = (d + 4) * 2.0 ** -23 * ((x ** 2).sum(axis=1)[:, None] + (Y ** 2).sum(axis=1)[None] + 2 * np.abs(x) @ np.abs(Y).T)
    rows = np.arange(len(qn))[:, None]
    err = np.abs(part.astype(np.float64) - Dt[rows, ids])
    print(f"{metric} d={d}: largest |part - D| / B = {(err / B[rows, ids]).max():.4f}")
    assert (err <= B[rows, ids]).all(), (err / B[rows, ids]).max()
    assert (np.diff(part, axis=1) >= 0).all()
    assert (Dt[rows[:, 0], ids[:, -1]] <= np.partition(Dt, k - 1, axis=1)[:, k - 1] + 2 * B.max(axis=1)).all()


N_R = 2 * 8192          # the sample is every second row


@functools.lru_cache(maxsize=None)
def _restricted():
    dev, Q, D = _integers(300, N_R)
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


@pytest.mark.parametrize("nq", [3, 130])
def test_several_segments(nq):
    n, k = 300_000, 100
    dev, Q, D = _integers(8, n, 130, 100)
    assert segment_rows(k, n) == 2 ** 17 and n % 2 ** 17 and -(-n // 2 ** 17) == 3
    for i in range(nq):
        assert max(within_tau_per_segment(D[i], k)) + k <= CAP, i
    _check(dev, Q[:nq], D[:nq], k)


@pytest.mark.parametrize("case", ["float16", "float64", "both"])
def test_refusals_leave_the_index_usable(case):
    rng = np.random.RandomState(9)
    X = rng.randn(600, 300).astype(np.float32)
    ivf = _ivf_half(X, X[:4]) if case == "float16" else _ivf(X, X[:4], store="float64" if case == "float64" else "float32")
    dev = ivf.device_index()
    qn, qpq = ivf._prepare(X[:8].copy())
    with pytest.raises(ValueError if case == "both" else AssertionError, match="not both" if case == "both" else 'store="float32"'):
        dev.knn_brute(qn, 5, wide=True, matrix=case == "both")
    if case == "both":
        with pytest.raises(AssertionError, match="d <= 128"):
            dev.knn_brute(qn, 5)
        assert (dev.knn_brute(qn, 5, wide=True)[:, 0] == np.arange(8)).all()
    assert (dev.knn_probe(qn, qpq, 5, 2) >= 0).all()
