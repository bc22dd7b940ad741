"""The exact k nearest rows under the restrictions of the query calls (tk_index_knn_brute_ex) against
numpy: ids == restricted_k_best of the exact integer part values over the rows that pass, distances == those part
values in float32 (+inf beside -1).  Every case has integer coordinates in [-50, 50]: every norm, product sum and part is
an integer below 2^24, float32 holds it exactly in any order of summation, and brute_reference.int_part is exact."""
import numpy as np
import pytest

from brute_reference import CAP, int_part, k_best, segment_rows
from brute_restricted_reference import (passes, restricted_dist, restricted_k_best, restricted_within_tau_per_segment,
                                        retry_segment_rows)
pytestmark = pytest.mark.gpu

N, D, NQ, K = 20000, 16, 131, 10
TWIN_FAILS, TWIN_A, TWIN_B = 100, 200, 300          # three identical rows: query 0 lies on them; the lowest must fail
GROUP_OF_3, GROUP_OF_K, GROUP_ABSENT = 7, 8, 99


def _index(data):
    """a DeviceIndex that only needs its vectors: one list holding everything (as tests/test_brute_gpu.py makes it)"""
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
    return ivf.device_index()


def _ints(rng, n, d):
    return rng.randint(-50, 51, size=(n, d)).astype(np.float32)


def _check(got, part, oks, k):
    """ids and part values of a knn_brute_dist call against the reference, query by query"""
    ids, dist = got
    assert ids.shape == dist.shape == (len(part), k) and ids.dtype == np.int64 and dist.dtype == np.float32
    for i in range(len(part)):
        want = restricted_k_best(part[i], oks[i], k)
        np.testing.assert_array_equal(ids[i], want, err_msg=f"query {i}")
        np.testing.assert_array_equal(dist[i], restricted_dist(part[i], want), err_msg=f"query {i}")


def _fits_first_attempt(part, oks, k):
    """no query's list exceeds CAP in any segment under the segment rule: k kept rows and what the segment appends"""
    most = max(max(restricted_within_tau_per_segment(part[i], oks[i], k)) for i in range(len(part)))
    assert most + k <= CAP, most
    return most


_BASE = {}


def _base():
    """N = 20 000 rows, 131 queries, the attributes of every restriction; one index for the tests that share it"""
    if not _BASE:
        rng = np.random.RandomState(20)
        Y = _ints(rng, N, D)
        Y[TWIN_A] = Y[TWIN_B] = Y[TWIN_FAILS]
        own = rng.choice(np.arange(400, N), size=NQ, replace=False)          # query i lies on row own[i] ...
        own[0] = TWIN_FAILS                                                 # ... query 0 on the three twins
        X = Y[own].copy()
        X[NQ // 2:] += rng.randint(-3, 4, size=(NQ - NQ // 2, D)).astype(np.float32)    # half next to their row
        groups = rng.randint(0, 7, size=N).astype(np.int32)
        groups[TWIN_FAILS], groups[TWIN_A], groups[TWIN_B] = 1, 2, 2
        free = np.setdiff1d(np.arange(400, N), own)
        special = rng.choice(free, size=3 + K, replace=False)
        groups[special[:3]], groups[special[3:]] = GROUP_OF_3, GROUP_OF_K
        row_tags = np.array([sum(1 << int(b) for b in rng.choice(8, size=rng.randint(1, 4), replace=False))
                             for _ in range(N)], dtype=np.uint64)
        row_tags[TWIN_FAILS], row_tags[TWIN_A], row_tags[TWIN_B] = 0b0001, 0b0110, 0b0110
        _BASE.update(Y=Y, X=X, own=own, groups=groups, row_tags=row_tags, special=special, part=int_part(X, Y),
                     dev=_index(Y), rng=rng)
    return _BASE


def _twins_answer(ids):
    """query 0 lies on three identical rows: the failing twin never appears, the tie goes to the lower passing row"""
    assert TWIN_FAILS not in ids[0]
    np.testing.assert_array_equal(ids[0][:2], [TWIN_A, TWIN_B])


# ---- 1. each restriction alone, and all five together ------------------------------------------------------------
@pytest.mark.parametrize("as_ids", [False, True])
def test_allowed_alone(as_ids):
    b = _base()
    mask = np.random.RandomState(21).rand(N) < 0.3
    mask[TWIN_FAILS], mask[TWIN_A], mask[TWIN_B] = False, True, True
    oks = [passes(i, N, allowed=mask) for i in range(NQ)]
    _fits_first_attempt(b["part"], oks, K)
    got = b["dev"].knn_brute_dist(b["X"], K, allowed=np.flatnonzero(mask) if as_ids else mask)
    _check(got, b["part"], oks, K)
    _twins_answer(got[0])


def test_exclude_alone():
    b = _base()
    exclude = b["own"].copy()
    exclude[5::7] = -1
    oks = [passes(i, N, exclude=exclude) for i in range(NQ)]
    _fits_first_attempt(b["part"], oks, K)
    got = b["dev"].knn_brute_dist(b["X"], K, exclude=exclude)
    _check(got, b["part"], oks, K)
    _twins_answer(got[0])
    assert got[0][5][0] == b["own"][5] and got[0][1][0] != b["own"][1]      # (kept where -1, gone where named)


def test_group_alone():
    b = _base()
    b["dev"].set_groups(b["groups"])
    group = np.random.RandomState(22).randint(-1, 7, size=NQ).astype(np.int32)
    group[0] = 2
    oks = [passes(i, N, group=group, groups=b["groups"]) for i in range(NQ)]
    assert (group == -1).any()
    _fits_first_attempt(b["part"], oks, K)
    got = b["dev"].knn_brute_dist(b["X"], K, group=group)
    _check(got, b["part"], oks, K)
    _twins_answer(got[0])


@pytest.mark.parametrize("mode", ["any", "all"])
def test_tags_alone(mode):
    b = _base()
    b["dev"].set_tags(b["row_tags"])
    rng = np.random.RandomState(23)
    tags = np.array([sum(1 << int(t) for t in rng.choice(8, size=rng.randint(1, 3), replace=False))
                     for _ in range(NQ)], dtype=np.uint64)
    tags[3::9] = 0
    tags[0] = 0b0110
    oks = [passes(i, N, tags=tags, tags_mode=mode, row_tags=b["row_tags"]) for i in range(NQ)]
    _fits_first_attempt(b["part"], oks, K)
    got = b["dev"].knn_brute_dist(b["X"], K, tags=tags, tags_mode=mode)
    _check(got, b["part"], oks, K)
    _twins_answer(got[0])


def _values_and_ranges(kind, rng):
    """(values, (lo, hi)): one int64 column or four float32 columns; per query closed, half-open and open intervals
    and some lo > hi; the failing twin lies outside query 0's range, the passing ones inside"""
    if kind == "i1":
        values = rng.randint(-1000, 1000, size=N).astype(np.int64)
        values[TWIN_FAILS], values[TWIN_A], values[TWIN_B] = 999, 5, 5
        lo = rng.randint(-1000, 400, size=NQ).astype(np.int64)
        hi = lo + rng.randint(100, 900, size=NQ)
        lo[4::10] = np.iinfo(np.int64).min                      # an open lower end
        hi[6::10] = np.iinfo(np.int64).max                      # an open upper end
        lo[8::10], hi[8::10] = 10, -10                          # lo > hi: nothing passes
        lo[0], hi[0] = 0, 10
        return values, (lo, hi)
    values = rng.randint(-100, 100, size=(N, 4)).astype(np.float32) / 4
    values[TWIN_FAILS], values[TWIN_A], values[TWIN_B] = 24.75, 1.5, 1.5
    lo = (rng.randint(-100, 0, size=(NQ, 4)) / 4).astype(np.float32)
    hi = lo + (rng.randint(60, 200, size=(NQ, 4)) / 4).astype(np.float32)
    lo[4::10, 1] = -np.inf
    hi[6::10, 2] = np.inf
    lo[5::10], hi[5::10] = -np.inf, np.inf                      # every column open: unrestricted
    lo[8::10, 3], hi[8::10, 3] = 2.0, 1.0
    lo[0], hi[0] = 0.0, 2.0
    return values, (lo, hi)


@pytest.mark.parametrize("kind", ["i1", "f4"])
def test_between_alone(kind):
    b = _base()
    values, between = _values_and_ranges(kind, np.random.RandomState(24))
    b["dev"].set_values(values)
    oks = [passes(i, N, between=between, values=values) for i in range(NQ)]
    assert not oks[8].any() and any(o.all() for o in oks) == (kind == "f4")
    _fits_first_attempt(b["part"], oks, K)
    got = b["dev"].knn_brute_dist(b["X"], K, between=between)
    _check(got, b["part"], oks, K)
    _twins_answer(got[0])


def test_all_five_together():
    b = _base()
    rng = np.random.RandomState(25)
    values, between = _values_and_ranges("f4", rng)
    lo, hi = between[0] - 10, between[1] + 10                   # (wider: the five together still leave rows)
    lo[8::10, 3], hi[8::10, 3] = 2.0, 1.0                       # ... but for the queries whose interval is empty
    between = (lo, hi)
    b["dev"].set_groups(b["groups"])
    b["dev"].set_tags(b["row_tags"])
    b["dev"].set_values(values)
    mask = rng.rand(N) < 0.7
    mask[TWIN_FAILS], mask[TWIN_A], mask[TWIN_B] = True, True, True
    exclude = b["own"].copy()                                   # query 0: the twin it lies on is the one excluded
    group = rng.randint(-1, 7, size=NQ).astype(np.int32)
    group[0] = -1
    tags = rng.randint(0, 256, size=NQ).astype(np.uint64)
    tags[0] = 0
    oks = [passes(i, N, allowed=mask, exclude=exclude, group=group, groups=b["groups"], tags=tags, tags_mode="any",
                  row_tags=b["row_tags"], between=between, values=values) for i in range(NQ)]
    counts = np.array([o.sum() for o in oks])
    assert (counts >= K).sum() > NQ // 2 and (counts < K).any(), counts
    _fits_first_attempt(b["part"], oks, K)
    got = b["dev"].knn_brute_dist(b["X"], K, allowed=mask, exclude=exclude, group=group, tags=tags, tags_mode="any",
                                  between=between)
    _check(got, b["part"], oks, K)
    _twins_answer(got[0])
    # the same call without the distances
    ids = b["dev"].knn_brute(b["X"], K, allowed=mask, exclude=exclude, group=group, tags=tags, between=between)
    np.testing.assert_array_equal(ids, got[0])


# ---- 2. too few passing rows ----------------------------------------------------------------------------------------
def test_fewer_than_k_passing_rows():
    b = _base()
    b["dev"].set_groups(b["groups"])
    group = np.full(NQ, GROUP_OF_3, dtype=np.int32)
    group[1::3] = GROUP_ABSENT
    group[2::3] = GROUP_OF_K
    oks = [passes(i, N, group=group, groups=b["groups"]) for i in range(NQ)]
    assert oks[0].sum() == 3 and oks[1].sum() == 0 and oks[2].sum() == K
    ids, dist = got = b["dev"].knn_brute_dist(b["X"], K, group=group)
    _check(got, b["part"], oks, K)
    assert (ids[0][:3] >= 0).all() and (ids[0][3:] == -1).all() and np.isposinf(dist[0][3:]).all()
    assert (ids[1] == -1).all() and np.isposinf(dist[1]).all()
    assert sorted(ids[2]) == sorted(b["special"][3:])


# ---- 3. a sample that sees no passing row ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [500, 10000])
def test_group_of_odd_rows_the_sample_never_sees(rows):
    """N = 20 000: the sample is rows 0, 2, 4, ...  A group of odd rows leaves tau at +inf, so the first segment (all
    of N under the rule) appends the whole group: 500 rows fit the list, 10 000 do not and the call repeats the
    selection with segments of 8 160 rows."""
    b = _base()
    assert N // 8192 == 2 and segment_rows(K, N) >= N
    odd = np.arange(1, N, 2)
    groups = np.zeros(N, dtype=np.int32)
    groups[odd if rows == len(odd) else np.random.RandomState(30).choice(odd, size=rows, replace=False)] = 1
    b["dev"].set_groups(groups)
    group = np.ones(NQ, dtype=np.int32)
    oks = [passes(i, N, group=group, groups=groups) for i in range(NQ)]
    assert oks[0].sum() == rows and not oks[0][np.arange(8192) * 2].any()
    first = [restricted_within_tau_per_segment(b["part"][i], oks[i], K) for i in range(NQ)]
    assert all(c == [rows] for c in first)                      # tau = +inf: every passing row is appended
    if rows + K <= CAP:
        _fits_first_attempt(b["part"], oks, K)
    else:
        assert rows > CAP
        seg = retry_segment_rows(K)
        again = [restricted_within_tau_per_segment(b["part"][i], oks[i], K, seg) for i in range(NQ)]
        assert len(again[0]) == 3 and max(max(c) for c in again) + K <= CAP
    _check(b["dev"].knn_brute_dist(b["X"], K, group=group), b["part"], oks, K)


# ---- 4. ties beyond the cap under a filter --------------------------------------------------------------------------
def test_ties_beyond_the_cap_are_answered():
    """9 000 identical rows of one group and a query on them: more rows tied within tau than a list holds — answered
    (the ten lowest of them) by the second attempt, and the queries beside it exactly."""
    rng = np.random.RandomState(40)
    Y = _ints(rng, N, D)
    Y[5000:14000] = Y[5000]
    X = _ints(rng, 40, D)
    X[7] = Y[5000]
    groups = (rng.rand(N) < 0.5).astype(np.int32)
    groups[5000:14000] = 1
    dev = _index(Y)
    dev.set_groups(groups)
    group = np.ones(len(X), dtype=np.int32)
    part = int_part(X, Y)
    oks = [passes(i, N, group=group, groups=groups) for i in range(len(X))]
    assert restricted_within_tau_per_segment(part[7], oks[7], K)[0] >= 9000 > CAP
    seg = retry_segment_rows(K)
    assert max(max(restricted_within_tau_per_segment(part[i], oks[i], K, seg)) for i in range(len(X))) + K <= CAP
    got = dev.knn_brute_dist(X, K, group=group)
    np.testing.assert_array_equal(got[0][7], np.arange(5000, 5010))
    assert (got[1][7] == 0).all()
    _check(got, part, oks, K)


# ---- 5. several segments --------------------------------------------------------------------------------------------
_SEGMENTS = {}


def _segments_case():
    if not _SEGMENTS:
        n, d = 300000, 8
        rng = np.random.RandomState(50)
        Y = _ints(rng, n, d)
        groups = (rng.rand(n) < 0.5).astype(np.int32)
        dev = _index(Y)
        dev.set_groups(groups)
        _SEGMENTS.update(Y=Y, groups=groups, dev=dev)
    return _SEGMENTS


@pytest.mark.parametrize("nq", [3, 200])
def test_several_segments(nq):
    """N = 300 000, k = 100: three segments of 2^17 rows, the last one partial; a group of half the rows; nq = 3 takes
    the split of a segment's rows over gridDim.y."""
    k = 100
    c = _segments_case()
    Y, groups = c["Y"], c["groups"]
    n = len(Y)
    assert segment_rows(k, n) == 1 << 17 and -(-n // (1 << 17)) == 3 and n % (1 << 17) != 0
    rng = np.random.RandomState(51 + nq)
    X = _ints(rng, nq, Y.shape[1])
    X[1] = Y[n - 1]                                             # the last row of the partial segment
    group = np.ones(nq, dtype=np.int32)
    ok = groups == 1
    ids, dist = c["dev"].knn_brute_dist(X, k, group=group)
    for q0 in range(0, nq, 20):
        part = int_part(X[q0:q0 + 20], Y)
        for i in range(len(part)):
            if q0 + i < 20:
                counts = restricted_within_tau_per_segment(part[i], ok, k)
                assert len(counts) == 3 and max(counts) + k <= CAP, counts
            want = restricted_k_best(part[i], ok, k)
            np.testing.assert_array_equal(ids[q0 + i], want, err_msg=f"query {q0 + i}")
            np.testing.assert_array_equal(dist[q0 + i], restricted_dist(part[i], want), err_msg=f"query {q0 + i}")


# ---- 6. odd d and tile edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8191, 8193])
@pytest.mark.parametrize("d", [1, 127])
def test_odd_d_and_tile_edges_one_query(n, d):
    rng = np.random.RandomState(n + d)
    Y = _ints(rng, n, d)
    Y[n - 1] = Y[77]
    values = rng.randint(0, 100, size=n).astype(np.int64)
    values[77], values[n - 1] = 99, 50                          # the lower twin fails, the last row passes
    dev = _index(Y)
    dev.set_values(values)
    between = (np.array([20]), np.array([60]))
    ok = passes(0, n, between=between, values=values)
    for x in (Y[77:78].copy(), _ints(rng, 1, d)):
        part = int_part(x, Y)
        assert np.abs(part).max() < 1 << 24
        for k in (1, 10):
            _check(dev.knn_brute_dist(x, k, between=between), part, [ok], k)


# ---- 7. the unrestricted call of the new entry point ----------------------------------------------------------------
def test_distances_alone_keep_the_ids_of_the_old_call():
    b = _base()
    old = b["dev"].knn_brute(b["X"], K)
    ids, dist = b["dev"].knn_brute_dist(b["X"], K)
    np.testing.assert_array_equal(ids, old)
    for i in range(NQ):
        np.testing.assert_array_equal(old[i], k_best(b["part"][i], K))
        np.testing.assert_array_equal(dist[i], b["part"][i][old[i]].astype(np.float32))


# ---- 8. index state -------------------------------------------------------------------------------------------------
def test_group_without_groups_is_a_state_error_and_the_index_lives_on():
    from tinyknn_amd._lib import TinyKnnHipError
    rng = np.random.RandomState(80)
    Y = _ints(rng, 3000, D)
    X = _ints(rng, 5, D)
    dev = _index(Y)
    with pytest.raises(TinyKnnHipError, match="no groups"):
        dev.knn_brute(X, K, group=1)
    with pytest.raises(TinyKnnHipError, match="no tags"):
        dev.knn_brute(X, K, tags=1)
    with pytest.raises(TinyKnnHipError, match="no values"):
        dev.knn_brute(X, K, between=(0, 1))
    part = int_part(X, Y)
    got = dev.knn_brute(X, K)
    for i in range(len(X)):
        np.testing.assert_array_equal(got[i], k_best(part[i], K))
