"""The radius search over the probed lists without a GPU: its reference (tests/radius_probe_reference.py) against a
slower, obvious form on integer data and — every list probed, nothing removed — against the brute call's reference;
the two ABI symbols against the header; the refusals made before the device is touched; the join of query chunks
against a stand-in device."""
import functools
import os
import re

import numpy as np
import pytest

from brute_reference import int_part
from radius_probe_reference import oracle_probes, passes, radius_probe_csr
from radius_reference import radius_csr
from store_reference import oracle_index

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tinyknn_hip.h")


@functools.lru_cache(maxsize=None)
def _int_case(build_probes):
    """a host-built euclidean index on integer coordinates in [-50, 50] (every squared distance an integer below
    2^24: float32 holds it exactly in any order of summation), its oracle copy, integer queries"""
    from oracle import oracle
    from tinyknn_amd import IVF, FastPQ
    oracle.build()
    rng = np.random.RandomState(90 + build_probes)
    n, d, L, nq = 700, 20, 7, 24
    cent = rng.randint(-40, 41, size=(L, d))
    X = np.clip(cent[rng.randint(L, size=n)] + rng.randint(-9, 10, size=(n, d)), -50, 50).astype(np.float32)
    X[5] = X[3]                                                 # twins
    Q = np.clip(cent[rng.randint(L, size=nq)] + rng.randint(-9, 10, size=(nq, d)), -50, 50).astype(np.float32)
    Q[0] = X[3]
    ivf = IVF("euclidean", L, FastPQ(2))
    state = np.random.get_state()
    np.random.seed(1234)
    try:
        ivf.fit(X).build(X, n_probes=build_probes, device=False)
    finally:
        np.random.set_state(state)
    qn, _ = ivf._prepare(Q.copy())
    np.testing.assert_array_equal(qn, Q)
    return ivf, oracle_index(oracle, ivf, ivf.data), X, np.ascontiguousarray(qn)


def _obvious(ox, X, qn, probes, radius, oks):
    """list by list, row by row, in Python integers"""
    out = []
    for i in range(len(qn)):
        seen, hits = set(), []
        for p in probes[i]:
            l = int(p) if p >= 0 else ox.n_lists - 1
            for pos in range(int(ox.list_n[l])):
                j = int(ox.ids[ox.ids_off[l] + pos])
                if j in seen or not 0 <= j < len(X):
                    continue
                seen.add(j)
                if oks is not None and not oks[i][j]:
                    continue
                dist = sum((int(a) - int(b)) ** 2 for a, b in zip(X[j], qn[i]))
                if dist <= radius[i]:
                    hits.append((dist, j))
        out.append(sorted(hits))
    return out


@pytest.mark.parametrize("build_probes", [1, 2])
@pytest.mark.parametrize("P", [1, 3])
def test_the_reference_is_the_obvious_walk_on_integer_data(build_probes, P):
    from oracle import oracle
    ivf, ox, X, qn = _int_case(build_probes)
    rng = np.random.RandomState(P)
    probes = oracle_probes(ox, qn, P)
    assert probes.shape == (len(qn), P)
    radius = rng.choice([0.0, 900.0, 2500.0, 6000.0, np.inf, -1.0], size=len(qn)).astype(np.float32)
    radius[0] = 0.0
    exclude = np.full(len(qn), -1, dtype=np.int64)
    exclude[0] = 3                                              # the lower twin fails: the other is the hit
    for oks in (None, [passes(i, len(X), allowed=rng.rand(len(X)) < 0.5, exclude=exclude) for i in range(len(qn))]):
        lims, ids, dist = radius_probe_csr(oracle, ox, qn, X, radius, P, oks=oks)
        want = _obvious(ox, X, qn, probes, radius, oks)
        assert lims.dtype == ids.dtype == np.int64 and dist.dtype == np.float32
        np.testing.assert_array_equal(np.diff(lims), [len(w) for w in want])
        np.testing.assert_array_equal(ids, [j for w in want for _, j in w])
        np.testing.assert_array_equal(dist, np.array([dv for w in want for dv, _ in w], dtype=np.float32))
        assert lims[-1] > 0
        if oks is None:
            assert ids[0] == 3 and ids[1] == 5 and dist[0] == dist[1] == 0
    if build_probes == 2:                                       # every row is stored twice: listed once all the same
        lims, ids, _ = radius_probe_csr(oracle, ox, qn, X, np.inf, 7)
        np.testing.assert_array_equal(np.diff(lims), len(X))


@pytest.mark.parametrize("build_probes", [1, 2])
def test_with_every_list_probed_the_sets_are_the_brute_calls_on_integer_data(build_probes):
    from oracle import oracle
    ivf, ox, X, qn = _int_case(build_probes)
    part = int_part(qn, X)
    r = np.partition(part, 40, axis=1)[:, 40].astype(np.float32)
    for P in (ox.n_lists, ox.n_lists + 3):
        got = radius_probe_csr(oracle, ox, qn, X, r, P)
        want = radius_csr(part, None, r)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype
            np.testing.assert_array_equal(g, w)


def _declared_arguments(name):
    text = open(HEADER).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/tinyknn_hip.h"
    return len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))


@pytest.mark.parametrize("name,n_args", [("tk_index_radius_probe", 18), ("tk_index_radius_probe_fetch", 3)])
def test_the_symbols_are_bound_with_the_headers_argument_counts(name, n_args):
    from tinyknn_amd import _lib
    assert name in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES[name]
    assert _declared_arguments(name) == n_args == len(argtypes)


def _host_ivf():
    """an IVF that has no device index and fails loudly if one is asked for"""
    from tinyknn_amd import IVF, FastPQ
    ivf = IVF("angular", 4, FastPQ(2))

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    ivf.device_index = no_device
    ivf._prepare = no_device
    return ivf


@pytest.mark.parametrize("call", ["radius_search", "radius_count"])
def test_refusals_come_before_any_device_call(call):
    from tinyknn_amd.ivf import AllowSet
    ivf = _host_ivf()
    Q = np.zeros((3, 4), np.float32)
    fn = getattr(ivf, call)
    with pytest.raises(TypeError, match="AllowSet"):
        fn(Q, 1.0, allowed=object.__new__(AllowSet), n_probes=2)
    with pytest.raises(ValueError, match="NaN"):
        fn(Q, np.array([0.5, np.nan, 1.0]), n_probes=2)
    with pytest.raises(ValueError, match="one entry per query"):
        fn(Q, np.array([0.5, 1.0]), n_probes=2)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="n_probes"):
            fn(Q, 1.0, n_probes=bad)
    with pytest.raises(AssertionError, match="a device call was made"):       # a good call reaches the device
        fn(Q, np.array([0.5, np.inf, -1.0]), n_probes=2)


def test_max_results_and_n_probes_are_checked_before_the_device_is_asked():
    from tinyknn_amd.ivf import DeviceIndex
    dev = object.__new__(DeviceIndex)
    dev.d, dev.dq, dev.N, dev.world = 4, 4, 10, 1
    Q = np.zeros((2, 4), np.float32)
    for bad in (-1, 2**31):
        with pytest.raises(ValueError, match="max_results"):
            dev.radius_probe(Q, Q, 1.0, 3, max_results=bad)
    with pytest.raises(ValueError, match="n_probes"):
        dev.radius_probe(Q, Q, 1.0, 0)
    with pytest.raises(ValueError, match="n_probes"):
        dev.radius_probe_count(Q, Q, 1.0, 0)


# ---- the join of query chunks ----------------------------------------------------------------------------------------
class _StandIn:
    """A device of `sizes[i]` hits for query i (ids i * 1000 + t): answers a part of queries as the C call does,
    refuses parts of more than `fits` queries as too large, holds one result at a time."""

    def __init__(self, sizes, fits=10**9):
        self.sizes, self.fits = np.asarray(sizes, dtype=np.int64), fits
        self.calls, self.fetched, self.held = [], [], None

    def part(self, o, e, limit):
        self.calls.append((o, e, limit))
        self.held = None
        if e - o > self.fits:
            return None
        lims = np.concatenate([[0], np.cumsum(self.sizes[o:e])]).astype(np.int64)
        if limit is None or lims[-1] > limit:
            return lims, None
        self.held = (o, e)

        def fetch():
            assert self.held == (o, e), "the device no longer holds this part"
            self.fetched.append((o, e))
            ids = np.concatenate([i * 1000 + np.arange(self.sizes[i]) for i in range(o, e)] + [np.zeros(0, np.int64)])
            return ids.astype(np.int64), ids.astype(np.float32) / 2
        return lims, fetch


def test_the_parts_of_a_call_are_joined_in_order():
    from tinyknn_amd.ivf import join_radius_parts
    sizes = [3, 0, 5, 1, 0, 0, 7, 2, 4, 1, 6]
    want_ids = np.concatenate([i * 1000 + np.arange(s) for i, s in enumerate(sizes)])
    for chunk, fits in ((100, 10**9), (4, 10**9), (1, 10**9), (8, 3), (100, 1)):
        dev = _StandIn(sizes, fits)
        lims, ids, dist = join_radius_parts(len(sizes), chunk, 1000, dev.part)
        np.testing.assert_array_equal(lims, np.concatenate([[0], np.cumsum(sizes)]))
        np.testing.assert_array_equal(ids, want_ids)
        np.testing.assert_array_equal(dist, want_ids.astype(np.float32) / 2)
        assert lims.dtype == ids.dtype == np.int64 and dist.dtype == np.float32
        asked = [c for c in dev.calls if c[2] is not None and c[1] - c[0] <= fits]
        assert [c[:2] for c in asked] == dev.fetched and max(e - o for o, e in dev.fetched) <= min(chunk, fits)
        assert [o for o, _ in dev.fetched] == sorted(o for o, _ in dev.fetched) and dev.fetched[-1][1] == len(sizes)
        # a part is asked with what the earlier parts left of the limit
        assert all(limit is None or limit == 1000 - sum(sizes[:o]) for o, _, limit in dev.calls)
        if len(dev.fetched) > 1:        # several parts: every one is counted before the first is fetched
            answered = [c for c in dev.calls if c[1] - c[0] <= fits]
            half = len(answered) // 2
            assert [c[:2] for c in answered[:half]] == dev.fetched and all(c[2] is None for c in answered[:half])
            assert all(c[2] is not None for c in answered[half:])


def test_the_limit_holds_for_the_sum_and_is_checked_before_any_part_is_fetched():
    from tinyknn_amd.ivf import join_radius_parts
    sizes = [3, 0, 5, 1, 0, 0, 7, 2, 4, 1, 6]
    total = sum(sizes)
    dev = _StandIn(sizes)
    lims, ids, dist = join_radius_parts(len(sizes), 4, total, dev.part)                  # exactly the limit: fine
    assert lims[-1] == total == len(ids)
    for limit in (total - 1, 5, 0):
        dev = _StandIn(sizes)
        with pytest.raises(ValueError, match=f"{total} rows lie within the radii, more than max_results = {limit}"):
            join_radius_parts(len(sizes), 4, limit, dev.part)
        assert dev.fetched == [] and dev.calls == [(0, 4, None), (4, 8, None), (8, 11, None)]
        dev = _StandIn(sizes)                                   # one part: the part's own check, the true total
        with pytest.raises(ValueError, match=f"{total} rows lie within the radii, more than max_results = {limit}"):
            join_radius_parts(len(sizes), 100, limit, dev.part)
        assert dev.fetched == [] and dev.calls == [(0, 11, limit)]


def test_counts_alone_and_no_queries():
    from tinyknn_amd.ivf import join_radius_parts
    sizes = [3, 0, 5, 1, 9]
    dev = _StandIn(sizes)
    lims, ids, dist = join_radius_parts(len(sizes), 2, None, dev.part)
    np.testing.assert_array_equal(np.diff(lims), sizes)
    assert ids is None and dist is None and dev.fetched == [] and all(c[2] is None for c in dev.calls)
    dev = _StandIn([])
    lims, ids, dist = join_radius_parts(0, 2, 10, dev.part)
    assert lims.tolist() == [0] and len(ids) == len(dist) == 0 and dist.dtype == np.float32
    assert dev.calls == [(0, 0, 10)]                            # (the device makes the refusals of an empty call too)
    with pytest.raises(MemoryError):
        join_radius_parts(3, 2, 10, _StandIn([1, 1, 1], fits=0).part)
