"""radius_search(matrix=True): every row within a radius over all rows of a half store on the f16 matrix cores
(radius_matrix.hip).  On integer data every product and sum is exact in float32, so lims, ids and value
bytes are radius_csr's over the int64 distances; on other data the values are knn_brute_dist(matrix=True)'s dist_m, the
parent's kernel.  RADIUS_MATRIX_STAGE = 8 forces every route (staged, refilled, both) at these small shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from brute_restricted_reference import passes  # noqa: E402
from radius_reference import radius_csr  # noqa: E402
from test_knn_brute_matrix_gpu import _integers  # noqa: E402
from test_knn_probe_matrix_gpu import _ivf  # noqa: E402
from test_radius_gpu import _same  # noqa: E402

pytestmark = pytest.mark.gpu
STAGE = 8


def _check(dev, Q, D, r, oks=None, **kw):
    """sorted result, counts and the unsorted result's sets against radius_csr"""
    want = radius_csr(D, oks, r)
    _same(dev.radius_brute(Q, r, matrix=True, **kw), want, "sorted")
    np.testing.assert_array_equal(dev.radius_count(Q, r, matrix=True, **kw), np.diff(want[0]))
    lims, ids, dist = dev.radius_brute(Q, r, matrix=True, sort=False, **kw)
    np.testing.assert_array_equal(lims, want[0])
    for i in range(len(Q)):
        a, b = lims[i], lims[i + 1]
        o = a + np.lexsort((ids[a:b], dist[a:b]))
        assert ids[o].tobytes() == want[1][a:b].tobytes() and dist[o].tobytes() == want[2][a:b].tobytes(), i


def _cycled(D):
    """per query -1, 0, its median distance, +inf, in turn"""
    r = np.array([np.partition(row, len(row) // 2)[len(row) // 2] for row in D], dtype=np.float32)
    r[0::4], r[1::4], r[3::4] = -1.0, 0.0, np.inf
    return r


@pytest.mark.parametrize("d,n,nq", [(d, 700, 129) for d in (1, 7, 8, 17, 63, 64, 65, 129, 4096)]
                         + [(17, n, 129) for n in (127, 128, 129, 257)]
                         + [(17, 700, nq) for nq in (1, 31, 32, 33, 63, 64, 65, 127, 128)])
def test_slab_block_and_tile_edges(d, n, nq):
    ivf, dev, Q, D = _integers(d, n)
    _check(dev, Q[:nq], D[:nq], _cycled(D[:nq]))


def _radius_for(row, most):
    """the largest radius that lists at most `most` rows of this query (-1: even the nearest value lists more)"""
    vals = np.unique(row)
    fit = [v for v in vals if (row <= v).sum() <= most]
    return float(fit[-1]) if fit else -1.0


@pytest.mark.parametrize("stage", [STAGE, 0])
@pytest.mark.parametrize("tiles", [(), (0,), (1,), (0, 1)])
def test_routes(monkeypatch, tiles, stage):
    """which tiles of 128 queries hold a list longer than the stage: none, the first, the second (one query), both"""
    ivf, dev, Q, D = _integers(17, 700)
    r = np.array([_radius_for(row, STAGE) for row in D], dtype=np.float32)
    for t in tiles:
        i = (5, 128)[t]
        r[i] = np.partition(D[i], 20)[20]
    counts = (D <= r[:, None]).sum(axis=1)
    assert tuple(np.unique(np.flatnonzero(counts > STAGE) // 128)) == tiles and (counts > 0).sum() > 64
    monkeypatch.setattr(dev, "RADIUS_MATRIX_STAGE", stage)
    _check(dev, Q, D, r)


def test_lists_of_exactly_the_stage_and_one_more(monkeypatch):
    ivf, dev, Q, D = _integers(17, 700)
    r = np.full(len(Q), -1.0, dtype=np.float32)
    seen = set()
    for i, row in enumerate(D):
        for most in (STAGE, STAGE + 1):
            v = _radius_for(row, most)
            if most not in seen and (row <= v).sum() == most:
                r[i] = v
                seen.add(most)
                break
    assert seen == {STAGE, STAGE + 1}
    monkeypatch.setattr(dev, "RADIUS_MATRIX_STAGE", STAGE)
    _check(dev, Q, D, r)


@pytest.mark.parametrize("which", ["all", "allowed", "exclude", "group", "tags", "between"])
def test_restrictions(monkeypatch, which):
    n = 700
    ivf, dev, Q, D = _integers(100, n)
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
    monkeypatch.setattr(dev, "RADIUS_MATRIX_STAGE", STAGE)
    _check(dev, Q, D, r, oks, **kw)


@pytest.mark.parametrize("metric,d", [(m, d) for m in ("angular", "euclidean") for d in (17, 100, 1536)])
def test_one_dist_m(metric, d):
    """the values are knn_brute_dist(matrix=True)'s: that call with k = N gives every row's dist_m"""
    rng = np.random.RandomState(d)
    scale = 1.0 if metric == "angular" else 30.0
    n = 700
    X, Q = (scale * rng.randn(n, d)).astype(np.float32), (scale * rng.randn(40, d)).astype(np.float32)
    ivf = _ivf(X, X[:6], metric)
    dev = ivf.device_index()
    qn, _ = ivf._prepare(Q.copy())
    ids, dm = dev.knn_brute_dist(qn, n, matrix=True)
    DM = np.empty((len(qn), n), dtype=np.float32)
    np.put_along_axis(DM, ids, dm, axis=1)
    for k in (10, 300):
        r = dm[:, k - 1].copy()
        want = radius_csr(DM, None, r)
        _same(dev.radius_brute(qn, r, matrix=True), want, f"{metric} d={d} k={k}")
        _same(ivf.radius_search(Q.copy(), r, True), want, f"IVF {metric} d={d} k={k}")


def test_refusals_leave_the_index_usable():
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(9)
    X = rng.randn(600, 20).astype(np.float32)
    f32 = IVF("euclidean", 4, FastPQ(2))
    f32.fit(X).build(X, n_probes=1, device=False)
    with pytest.raises(AssertionError, match='needs store="float16"'):
        f32.radius_search(X[:8], 1.0, matrix=True)
    assert f32.radius_search(X[:8], 1.0)[0][-1] >= 8
    ivf = _ivf(X, X[:4])
    bad = X[:8].copy()
    bad[3, 7] = np.nan
    with pytest.raises(AssertionError, match="NaN or an infinity"):
        ivf.radius_search(bad, 1.0, matrix=True)
    assert ivf.radius_search(X[:8], 1.0, matrix=True)[0][-1] >= 8
    for call in (ivf.radius_search, ivf.radius_count):
        with pytest.raises(ValueError, match="matrix=True.*n_probes"):
            call(X[:8], 1.0, matrix=True, n_probes=2)
    total = int(ivf.radius_count(X[:8], np.inf, matrix=True).sum())
    assert total == 8 * 600
    with pytest.raises(ValueError, match=f"{total} rows lie within the radii, more than max_results = 100"):
        ivf.radius_search(X[:8], np.inf, matrix=True, max_results=100)
    lims, ids, dist = ivf.radius_search(X[:8], np.inf, matrix=True)
    assert lims[-1] == total and (np.diff(dist.reshape(8, 600), axis=1) >= 0).all()
