"""radius_search(wide=True): every row within a radius over all rows of a float32 store of any d <= 4096 on the f32
matrix cores (radius_wide.hip).  On integer data in [-3, 3] every product and sum is exact in float32
(2 * 9 * 4096 < 2^24), so lims, ids and value bytes are radius_csr's over the int64 distances; on other data the values
are the default call's at d <= 128 and knn_brute_dist(wide=True)'s beyond.  RADIUS_WIDE_STAGE = 8 forces every route
(staged, refilled, both) at these small shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from brute_restricted_reference import passes  # noqa: E402
from radius_reference import radius_csr  # noqa: E402
from test_knn_brute_wide_gpu import _integers, _ivf, _randn  # noqa: E402
from test_knn_probe_matrix_gpu import _ivf as _ivf_half  # noqa: E402
from test_radius_gpu import _same  # noqa: E402

pytestmark = pytest.mark.gpu
STAGE = 8


def _check(dev, Q, D, r, oks=None, **kw):
    """sorted result, counts and the unsorted result's sets against radius_csr"""
    want = radius_csr(D, oks, r)
    _same(dev.radius_brute(Q, r, wide=True, **kw), want, "sorted")
    np.testing.assert_array_equal(dev.radius_count(Q, r, wide=True, **kw), np.diff(want[0]))
    lims, ids, part = dev.radius_brute(Q, r, wide=True, sort=False, **kw)
    np.testing.assert_array_equal(lims, want[0])
    for i in range(len(Q)):
        a, b = lims[i], lims[i + 1]
        o = a + np.lexsort((ids[a:b], part[a:b]))
        assert ids[o].tobytes() == want[1][a:b].tobytes() and part[o].tobytes() == want[2][a:b].tobytes(), i


def _cycled(D):
    """per query -1, 0, its median distance, +inf, in turn"""
    r = np.array([np.partition(row, len(row) // 2)[len(row) // 2] for row in D], dtype=np.float32)
    r[0::4], r[1::4], r[3::4] = -1.0, 0.0, np.inf
    return r


@pytest.mark.parametrize("d,n,nq", [(d, 700, 129) for d in (1, 2, 3, 31, 32, 33, 65, 128, 129, 4096)]
                         + [(129, n, 129) for n in (127, 128, 129, 257)]
                         + [(129, 700, nq) for nq in (1, 32, 33, 64, 65, 127, 128)])
def test_slab_block_and_tile_edges(d, n, nq):
    dev, Q, D = _integers(d, n)
    _check(dev, Q[:nq], D[:nq], _cycled(D[:nq]))


def _radius_for(row, most):
    """the largest radius that lists at most `most` rows of this query (-1: even the nearest value lists more)"""
    fit = [v for v in np.unique(row) if (row <= v).sum() <= most]
    return float(fit[-1]) if fit else -1.0


@pytest.mark.parametrize("stage", [STAGE, 0])
@pytest.mark.parametrize("tiles", [(), (0,), (1,), (0, 1), "edge"])
def test_routes(monkeypatch, tiles, stage):
    """which tiles of 128 queries hold a list longer than the stage: none, the first, the second (one query), both;
    edge: one list of exactly the stage and one of one more, every other list empty"""
    dev, Q, D = _integers(129, 700)
    if tiles == "edge":
        r = np.full(len(Q), -1.0, dtype=np.float32)
        for most in (STAGE, STAGE + 1):
            i = next(i for i, row in enumerate(D) if r[i] < 0 and (row <= _radius_for(row, most)).sum() == most)
            r[i] = _radius_for(D[i], most)
        assert sorted((D <= r[:, None]).sum(axis=1))[-2:] == [STAGE, STAGE + 1]
    else:
        r = np.array([_radius_for(row, STAGE) for row in D], dtype=np.float32)
        for t in tiles:
            i = (5, 128)[t]
            r[i] = np.partition(D[i], 20)[20]
        counts = (D <= r[:, None]).sum(axis=1)
        assert tuple(np.unique(np.flatnonzero(counts > STAGE) // 128)) == tiles and (counts > 0).sum() > 64
    monkeypatch.setattr(dev, "RADIUS_WIDE_STAGE", stage)
    _check(dev, Q, D, r)


@pytest.mark.parametrize("which", ["all", "allowed", "exclude", "group", "tags", "between"])
def test_restrictions(monkeypatch, which):
    n = 700
    dev, Q, D = _integers(300, n)
    rng = np.random.RandomState(3)
    nq = len(Q)
    rows = dict(groups=rng.randint(0, 4, size=n).astype(np.int32), row_tags=rng.randint(1, 256, size=n).astype(np.uint64),
                values=rng.randint(0, 100, size=n).astype(np.int64))
    rows["groups"][:5] = 4                                          # a group of 5 rows: fewer than any list would show
    dev.set_groups(rows["groups"])
    dev.set_tags(rows["row_tags"])
    dev.set_values(rows["values"])
    group = rng.randint(-1, 4, size=nq).astype(np.int32)
    group[::7] = 4
    every = dict(allowed=rng.rand(n) < 0.5, exclude=D.argmin(axis=1), group=group,
                 tags=rng.randint(0, 16, size=nq).astype(np.uint64),
                 between=(np.zeros(nq, np.int64), np.full(nq, 60, np.int64)))
    kw = every if which == "all" else {which: every[which]}
    oks = [passes(i, n, **kw, **rows) for i in range(nq)]
    r = _cycled(D)
    r[::7] = np.inf
    if "group" in kw:
        assert all(oks[i].sum() <= 5 for i in range(0, nq, 7))
    monkeypatch.setattr(dev, "RADIUS_WIDE_STAGE", STAGE)
    _check(dev, Q, D, r, oks, **kw)


@pytest.mark.parametrize("metric,d", [(m, d) for m in ("angular", "euclidean") for d in (17, 100, 128, 129, 1536)])
def test_one_part(metric, d):
    """at d <= 128 the bytes of the default call; beyond, knn_brute_dist(wide=True) with k = N gives every row's part, so
    knn_brute(wide=True)'s ids are the first k entries"""
    n = 700
    X, Q = _randn(metric, d)
    ivf = _ivf(X[:n], X[:6], metric)
    dev, qn = ivf.device_index(), ivf._prepare(Q.copy())[0]
    ids, part = dev.knn_brute_dist(qn, n, wide=True)
    P = np.empty((len(qn), n), dtype=np.float32)
    np.put_along_axis(P, ids, part, axis=1)
    for k in (10, 300):
        r = part[:, k - 1].copy()
        want = dev.radius_brute(qn, r) if d <= 128 else radius_csr(P, None, r)
        _same(dev.radius_brute(qn, r, wide=True), want, f"{metric} d={d} k={k}")
    _same(ivf.radius_search(Q.copy(), r, False, True), want, f"IVF {metric} d={d}")


def test_refusals_leave_the_index_usable():
    rng = np.random.RandomState(9)
    X = rng.randn(600, 300).astype(np.float32)
    for other in (_ivf_half(X, X[:4]), _ivf(X, X[:4], store="float64")):
        dev = other.device_index()
        qn, qpq = other._prepare(X[:8].copy())
        for call in (dev.radius_brute, dev.radius_count):
            with pytest.raises(AssertionError, match='store="float32"'):
                call(qn, 1.0, wide=True)
        assert (dev.knn_probe(qn, qpq, 5, 2) >= 0).all()
    ivf = _ivf(X, X[:4])
    for call in (ivf.radius_search, ivf.radius_count):
        with pytest.raises(ValueError, match="not both"):
            call(X[:8], 1.0, wide=True, matrix=True)
        with pytest.raises(ValueError, match="wide=True.*n_probes"):
            call(X[:8], 1.0, wide=True, n_probes=2)
    total = int(ivf.radius_count(X[:8], np.inf, wide=True).sum())
    assert total == 8 * 600
    with pytest.raises(ValueError, match=f"{total} rows lie within the radii, more than max_results = 100"):
        ivf.radius_search(X[:8], np.inf, wide=True, max_results=100)
    lims, ids, part = ivf.radius_search(X[:8], np.inf, wide=True)
    assert lims[-1] == total and (np.diff(part.reshape(8, 600), axis=1) >= 0).all()
