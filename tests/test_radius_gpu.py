"""Every row within a radius of each query (tk_index_radius_brute) against numpy: lims, ids and dist ==
radius_reference.radius_csr of the exact part values over the rows that pass, byte for byte.  Unless stated the data has
integer coordinates in [-50, 50]: every norm, product sum and part is an integer below 2^24, float32 holds it exactly
in any order of summation, and brute_reference.int_part is the truth (tests/test_brute_restricted_gpu.py's argument;
its base case and attributes are shared)."""
import numpy as np
import pytest

import test_brute_restricted_gpu as tbr
from brute_reference import int_part, numpy_part, pad_chunk
from radius_reference import passes, radius_csr

pytestmark = pytest.mark.gpu

N, D, NQ = tbr.N, tbr.D, tbr.NQ
_index, _ints = tbr._index, tbr._ints


def _same(got, want, what=""):
    """a (lims, ids, dist) result against the reference's: dtypes, shapes and bytes"""
    for g, w, name, dt in zip(got, want, ("lims", "ids", "dist"), (np.int64, np.int64, np.float32)):
        assert g.dtype == dt and g.ndim == 1, (name, g.dtype, g.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")
        assert g.tobytes() == np.ascontiguousarray(w, dtype=dt).tobytes(), f"{what} {name}"


def _kth(part, k):
    """every query's k-th smallest part value"""
    return np.partition(part, k - 1, axis=1)[:, k - 1].astype(np.float32)


def _twins_answer(got):
    """query 0 lies on three identical rows: the failing twin is no hit, the passing ones lead the list in id order"""
    lims, ids, dist = got
    first = ids[lims[0]:lims[1]]
    assert tbr.TWIN_FAILS not in first
    np.testing.assert_array_equal(first[:2], [tbr.TWIN_A, tbr.TWIN_B])
    assert (dist[:2] == 0).all()


# ---- 1. base ----------------------------------------------------------------------------------------------------------
def test_base_per_query_and_scalar_radius_and_counts():
    b = tbr._base()
    part = b["part"]
    r = _kth(part, 50)
    want = radius_csr(part, None, r)
    sizes = np.diff(want[0])
    assert (sizes >= 50).all() and (sizes > 50).any(), sizes           # ties on the boundary: all of them are in
    got = b["dev"].radius_brute(b["X"], r)
    _same(got, want, "per query")
    np.testing.assert_array_equal(b["dev"].radius_count(b["X"], r), sizes)
    scalar = float(np.median(r))
    want = radius_csr(part, None, scalar)
    assert len(set(np.diff(want[0]))) > 10
    _same(b["dev"].radius_brute(b["X"], scalar), want, "scalar")
    np.testing.assert_array_equal(b["dev"].radius_count(b["X"], scalar), np.diff(want[0]))


# ---- 2. each restriction alone, and all five together ----------------------------------------------------------------
def _restricted(oks, **kw):
    b = tbr._base()
    r = _kth(b["part"], 300)
    want = radius_csr(b["part"], oks, r)
    assert 0 < want[0][-1] < 300 * NQ
    got = b["dev"].radius_brute(b["X"], r, **kw)
    _same(got, want)
    np.testing.assert_array_equal(b["dev"].radius_count(b["X"], r, **kw), np.diff(want[0]))
    _twins_answer(got)


@pytest.mark.parametrize("as_ids", [False, True])
def test_allowed_alone(as_ids):
    mask = np.random.RandomState(21).rand(N) < 0.3
    mask[tbr.TWIN_FAILS], mask[tbr.TWIN_A], mask[tbr.TWIN_B] = False, True, True
    _restricted([passes(i, N, allowed=mask) for i in range(NQ)], allowed=np.flatnonzero(mask) if as_ids else mask)


def test_exclude_alone():
    exclude = tbr._base()["own"].copy()
    exclude[5::7] = -1
    _restricted([passes(i, N, exclude=exclude) for i in range(NQ)], exclude=exclude)


def test_group_alone():
    b = tbr._base()
    b["dev"].set_groups(b["groups"])
    group = np.random.RandomState(22).randint(-1, 7, size=NQ).astype(np.int32)
    group[0] = 2
    assert (group == -1).any()
    _restricted([passes(i, N, group=group, groups=b["groups"]) for i in range(NQ)], group=group)


@pytest.mark.parametrize("mode", ["any", "all"])
def test_tags_alone(mode):
    b = tbr._base()
    b["dev"].set_tags(b["row_tags"])
    rng = np.random.RandomState(23)
    tags = np.array([sum(1 << int(t) for t in rng.choice(8, size=rng.randint(1, 3), replace=False))
                     for _ in range(NQ)], dtype=np.uint64)
    tags[3::9] = 0
    tags[0] = 0b0110
    _restricted([passes(i, N, tags=tags, tags_mode=mode, row_tags=b["row_tags"]) for i in range(NQ)],
                tags=tags, tags_mode=mode)


@pytest.mark.parametrize("kind", ["i1", "f4"])
def test_between_alone(kind):
    b = tbr._base()
    values, between = tbr._values_and_ranges(kind, np.random.RandomState(24))
    b["dev"].set_values(values)
    oks = [passes(i, N, between=between, values=values) for i in range(NQ)]
    assert not oks[8].any()
    _restricted(oks, between=between)


def test_all_five_together():
    b = tbr._base()
    rng = np.random.RandomState(25)
    values, between = tbr._values_and_ranges("f4", rng)
    lo, hi = between[0] - 10, between[1] + 10
    lo[8::10, 3], hi[8::10, 3] = 2.0, 1.0
    between = (lo, hi)
    b["dev"].set_groups(b["groups"])
    b["dev"].set_tags(b["row_tags"])
    b["dev"].set_values(values)
    mask = rng.rand(N) < 0.7
    mask[tbr.TWIN_FAILS], mask[tbr.TWIN_A], mask[tbr.TWIN_B] = True, True, True
    exclude = b["own"].copy()                                   # query 0: the twin it lies on is the one excluded
    group = rng.randint(-1, 7, size=NQ).astype(np.int32)
    group[0] = -1
    tags = rng.randint(0, 256, size=NQ).astype(np.uint64)
    tags[0] = 0
    oks = [passes(i, N, allowed=mask, exclude=exclude, group=group, groups=b["groups"], tags=tags, tags_mode="any",
                  row_tags=b["row_tags"], between=between, values=values) for i in range(NQ)]
    _restricted(oks, allowed=mask, exclude=exclude, group=group, tags=tags, tags_mode="any", between=between)


# ---- 3. tile and grid edges: every row of every query --------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(31, 3), (32, 1), (33, 7), (4097, 33), (5000, 100), (3000, 128)])
@pytest.mark.parametrize("nq", [1, 33, 129])
def test_tile_and_grid_edges_list_every_row(n, d, nq):
    """nq = 129 leaves a workgroup with one real and 127 clamped query rows, odd n a tail tile: the smallest shapes at
    which a clamped row or a padded column could be counted"""
    rng = np.random.RandomState(1000 * n + 10 * d + nq)
    Y, X = _ints(rng, n, d), _ints(rng, nq, d)
    X[0] = Y[n - 1]
    part = int_part(X, Y)
    assert np.abs(part).max() < 1 << 24
    dev = _index(Y)
    lims, ids, dist = got = dev.radius_brute(X, np.inf)
    np.testing.assert_array_equal(lims, np.arange(nq + 1) * n)
    _same(got, radius_csr(part, None, np.inf))
    np.testing.assert_array_equal(dev.radius_count(X, np.inf), np.full(nq, n))


# ---- 4. lists longer than an LDS sort, rows split over blockIdx.y --------------------------------------------------
_LONG = {}


def _long():
    if not _LONG:
        rng = np.random.RandomState(400)
        Y = _ints(rng, 40000, D)
        _LONG.update(Y=Y, dev=_index(Y), rng=rng)
    return _LONG


def test_three_lists_of_forty_thousand():
    c = _long()
    X = _ints(np.random.RandomState(401), 3, D)
    got = c["dev"].radius_brute(X, np.inf)
    assert got[0].tolist() == [0, 40000, 80000, 120000]
    _same(got, radius_csr(int_part(X, c["Y"]), None, np.inf))


def test_one_query_and_half_the_rows():
    c = _long()
    X = _ints(np.random.RandomState(402), 1, D)
    part = int_part(X, c["Y"])
    r = float(np.median(part[0]))
    want = radius_csr(part, None, r)
    assert 19000 < want[0][1] < 21000 and want[0][1] > 8192
    _same(c["dev"].radius_brute(X, r), want)
    np.testing.assert_array_equal(c["dev"].radius_count(X, r), np.diff(want[0]))


# ---- 5. ties -----------------------------------------------------------------------------------------------------
def test_nine_thousand_identical_rows_at_radius_zero():
    """the case knn_brute cannot return: more tied rows than its k allows"""
    rng = np.random.RandomState(40)
    Y = _ints(rng, N, D)
    Y[5000:14000] = Y[5000]
    X = _ints(rng, 40, D)
    X[7] = Y[5000]
    dev = _index(Y)
    lims, ids, dist = got = dev.radius_brute(X, 0.0)
    np.testing.assert_array_equal(ids[lims[7]:lims[8]], np.arange(5000, 14000))
    assert (dist[lims[7]:lims[8]] == 0.0).all()
    _same(got, radius_csr(int_part(X, Y), None, 0.0))


# ---- 6. empty results -----------------------------------------------------------------------------------------------
def test_empty_results():
    b = tbr._base()
    dev, X, part = b["dev"], b["X"], b["part"]
    lims, ids, dist = dev.radius_brute(X, -1.0)
    assert lims.dtype == np.int64 and lims.shape == (NQ + 1,) and not lims.any()
    assert ids.dtype == np.int64 and dist.dtype == np.float32 and ids.shape == dist.shape == (0,)
    assert not dev.radius_count(X, -1.0).any()
    dev.set_groups(b["groups"])
    group = np.full(NQ, tbr.GROUP_ABSENT, dtype=np.int32)
    got = dev.radius_brute(X, np.inf, group=group)
    assert not got[0].any() and len(got[1]) == len(got[2]) == 0
    r = _kth(part, 20)
    r[0::2] = -1.0                                              # empty and non-empty queries alternate
    want = radius_csr(part, None, r)
    assert (np.diff(want[0])[0::2] == 0).all() and (np.diff(want[0])[1::2] >= 20).all()
    _same(dev.radius_brute(X, r), want)
    lims, ids, dist = dev.radius_brute(X[:0], 1.0)              # no query at all
    assert lims.tolist() == [0] and lims.dtype == np.int64
    assert ids.dtype == np.int64 and dist.dtype == np.float32 and ids.shape == dist.shape == (0,)
    assert dev.radius_count(X[:0], 1.0).shape == (0,)


# ---- 7. max_results -------------------------------------------------------------------------------------------------
def test_max_results_is_loud_and_the_index_lives_on():
    from tinyknn_amd import _lib
    b = tbr._base()
    dev, X, part = b["dev"], b["X"], b["part"]
    r = _kth(part, 30)
    want = radius_csr(part, None, r)
    T = int(want[0][-1])
    _same(dev.radius_brute(X, r, max_results=T), want)
    with pytest.raises(ValueError, match=rf"\b{T}\b"):
        dev.radius_brute(X, r, max_results=T - 1)
    with pytest.raises(_lib.TinyKnnHipError, match="no result is held"):        # the refused call holds nothing
        _lib.check(_lib.lib().tk_index_radius_fetch(dev._h, None, None))
    np.testing.assert_array_equal(dev.radius_count(X, r), np.diff(want[0]))    # counts answer regardless
    with pytest.raises(_lib.TinyKnnHipError, match="no result is held"):        # ... and hold nothing either
        _lib.check(_lib.lib().tk_index_radius_fetch(dev._h, None, None))
    _same(dev.radius_brute(X, r), want, "the next call")


# ---- 8. unsorted ----------------------------------------------------------------------------------------------------
def test_unsorted_lists_hold_the_same_rows_and_values():
    b = tbr._base()
    r = _kth(b["part"], 200)
    want = radius_csr(b["part"], None, r)
    lims, ids, dist = b["dev"].radius_brute(b["X"], r, sort=False)
    assert ids.dtype == np.int64 and dist.dtype == np.float32
    np.testing.assert_array_equal(lims, want[0])
    for i in range(NQ):
        s = slice(lims[i], lims[i + 1])
        order = np.argsort(ids[s], kind="stable")
        back = np.argsort(want[1][s], kind="stable")
        np.testing.assert_array_equal(ids[s][order], want[1][s][back], err_msg=f"query {i}")
        np.testing.assert_array_equal(dist[s][order], want[2][s][back], err_msg=f"query {i}")


# ---- 9. agreement with knn_brute_dist on data that is not integer ------------------------------------------------------
def test_the_first_k_entries_are_knn_brute_and_the_values_numpys():
    n, d, nq, k = 30000, 100, 100, 10
    rng = np.random.RandomState(90)
    Y = rng.randn(n, d).astype(np.float32)
    X = rng.randn(nq, d).astype(np.float32)
    dev = _index(Y)
    knn_ids, knn_part = dev.knn_brute_dist(X, k)
    r = knn_part[:, k - 1].copy()
    lims, ids, dist = dev.radius_brute(X, r)
    part = numpy_part(pad_chunk(X, rng), Y)[:nq]
    for i in range(nq):
        s = slice(lims[i], lims[i + 1])
        np.testing.assert_array_equal(ids[s][:k], knn_ids[i], err_msg=f"query {i}")
        assert (dist[s] <= r[i]).all()
        assert lims[i + 1] - lims[i] == int((part[i] <= r[i]).sum()), i
        np.testing.assert_array_equal(dist[s], part[i][ids[s]], err_msg=f"query {i}")
    _same((lims, ids, dist), radius_csr(part, None, r))


# ---- 10. mutations --------------------------------------------------------------------------------------------------
def test_add_remove_and_update_are_seen():
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(100)
    Y = _ints(rng, 3000, D)
    ivf = IVF("euclidean", 8, FastPQ(2))
    state = np.random.get_state()
    np.random.seed(100)
    try:
        ivf.fit(Y).build(Y, n_probes=1)
    finally:
        np.random.set_state(state)
    ivf.device_index()
    X = _ints(rng, 20, D)
    r = 9000.0
    _same(ivf.radius_search(X, r), radius_csr(int_part(X, Y), None, r), "built")
    new = _ints(rng, 500, D)
    new[:20] = X                                                # every query now lies on a new row
    ivf.add(new)
    assert len(ivf.data) == 3500
    got = ivf.radius_search(X, r)
    _same(got, radius_csr(int_part(X, ivf.data), None, r), "after add")
    assert all(3000 + i in got[1][got[0][i]:got[0][i + 1]] for i in range(20))
    gone = np.concatenate([np.arange(3000, 3010), rng.choice(3000, 300, replace=False)])
    ivf.remove(gone)
    alive = np.ones(3500, dtype=bool)
    alive[gone] = False
    oks = [alive] * 20
    got = ivf.radius_search(X, r, allowed=alive)
    _same(got, radius_csr(int_part(X, ivf.data), oks, r), "after remove")
    assert not np.isin(got[1], gone).any()
    ids = np.flatnonzero(alive)[::7][:200].astype(np.int64)
    fresh = _ints(rng, len(ids), D)
    fresh[:5] = X[:5] + 1.0
    ivf.update(ids, fresh)
    np.testing.assert_array_equal(ivf.data[ids], fresh)
    got = ivf.radius_search(X, r, allowed=alive)
    _same(got, radius_csr(int_part(X, ivf.data), oks, r), "after update")
    assert all(ids[i] in got[1][got[0][i]:got[0][i + 1]] for i in range(5))
    np.testing.assert_array_equal(ivf.radius_count(X, r, allowed=alive), np.diff(got[0]))


# ---- 11. the IVF layer on an angular index --------------------------------------------------------------------------
def test_raw_queries_on_an_angular_index_cosine_threshold():
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(110)
    n, d, nq = 6000, 20, 100
    cent = rng.randn(12, d)
    Y = (cent[rng.randint(12, size=n)] + 0.5 * rng.randn(n, d)).astype(np.float32)
    Q = (3.0 * (cent[rng.randint(12, size=nq)] + 0.5 * rng.randn(nq, d))).astype(np.float32)     # not normalised
    ivf = IVF("angular", 12, FastPQ(2))
    state = np.random.get_state()
    np.random.seed(110)
    try:
        ivf.fit(Y).build(Y, n_probes=1, device=False)
    finally:
        np.random.set_state(state)
    radius = 2 - 2 * 0.8                                        # cosine >= 0.8
    got = ivf.radius_search(Q, radius)
    qn, _ = ivf._prepare(Q.copy())
    part = numpy_part(np.ascontiguousarray(qn, dtype=np.float32), ivf.data)
    want = radius_csr(part, None, radius)
    assert 1000 < want[0][-1] < nq * n // 2
    _same(got, want)
    np.testing.assert_array_equal(ivf.radius_count(Q, radius), np.diff(want[0]))
    cos = 1 - got[2] / 2
    assert (cos >= 0.8 - 1e-6).all()


# ---- 12. refusals ---------------------------------------------------------------------------------------------------
def test_half_and_float64_stores_are_refused():
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import DeviceIndex
    rng = np.random.RandomState(120)
    Y = _ints(rng, 3000, D)
    X = _ints(rng, 5, D)
    ivf = IVF("euclidean", 8, FastPQ(2))
    state = np.random.get_state()
    np.random.seed(120)
    try:
        ivf.fit(Y).build(Y, n_probes=1, device=False)
    finally:
        np.random.set_state(state)
    half = DeviceIndex(ivf, store="float16")
    for call in (half.radius_brute, half.radius_count):
        with pytest.raises(AssertionError, match="half"):
            call(X, 100.0)
    half.close()
    f64 = _index(Y.astype(np.float64))
    for call in (f64.radius_brute, f64.radius_count):
        with pytest.raises(AssertionError, match="float32 vectors only"):
            call(X, 100.0)


def test_group_without_groups_is_a_state_error_and_the_index_lives_on():
    from tinyknn_amd._lib import TinyKnnHipError
    rng = np.random.RandomState(121)
    Y = _ints(rng, 3000, D)
    X = _ints(rng, 5, D)
    dev = _index(Y)
    for call in (dev.radius_brute, dev.radius_count):
        with pytest.raises(TinyKnnHipError, match="no groups"):
            call(X, 100.0, group=1)
        with pytest.raises(TinyKnnHipError, match="no tags"):
            call(X, 100.0, tags=1)
        with pytest.raises(TinyKnnHipError, match="no values"):
            call(X, 100.0, between=(0, 1))
    part = int_part(X, Y)
    r = _kth(part, 10)
    _same(dev.radius_brute(X, r), radius_csr(part, None, r))


# ---- 13. repeatability ----------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes():
    b = tbr._base()
    r = _kth(b["part"], 500)
    one = b["dev"].radius_brute(b["X"], r)
    two = b["dev"].radius_brute(b["X"], r)
    for a, c in zip(one, two):
        assert a.tobytes() == c.tobytes()
    assert one[0][-1] >= 500 * NQ
