"""The references of the restricted exact search (tests/brute_restricted_reference.py) against the obvious full-sort
forms, and what IVF.knn_brute / DeviceIndex.knn_brute refuse before any device call.  No GPU."""
import inspect

import numpy as np
import pytest

from brute_reference import CAP, NS, segment_rows, within_tau_per_segment
from brute_restricted_reference import (passes, restricted_dist, restricted_k_best, restricted_within_tau_per_segment,
                                        retry_segment_rows)


def _rows(rng, n):
    groups = rng.randint(0, 5, size=n).astype(np.int32)
    row_tags = np.array([sum(1 << int(b) for b in rng.choice(8, size=rng.randint(1, 4), replace=False))
                         for _ in range(n)], dtype=np.uint64)
    values = np.stack([rng.randint(-20, 20, size=n), rng.randint(0, 100, size=n)], axis=1).astype(np.int64)
    return groups, row_tags, values


def test_passes_is_the_formula_row_by_row():
    rng = np.random.RandomState(0)
    n, nq = 300, 7
    groups, row_tags, values = _rows(rng, n)
    allowed = rng.rand(n) < 0.6
    exclude = np.array([5, -1, 17, 299, -1, 0, 42])
    group = np.array([0, -1, 3, 4, 9, -1, 2])
    tags = np.array([0, 3, 0x81, 4, 0, 0xff, 1], dtype=np.uint64)
    lo = np.stack([rng.randint(-25, 5, size=nq), rng.randint(-5, 60, size=nq)], axis=1)
    hi = np.stack([rng.randint(-5, 25, size=nq), rng.randint(40, 120, size=nq)], axis=1)
    lo[3], hi[3] = (5, 10), (-5, 90)                # lo > hi on one column: nothing passes
    for mode in ("any", "all"):
        for i in range(nq):
            got = passes(i, n, allowed=allowed, exclude=exclude, group=group, groups=groups, tags=tags, tags_mode=mode,
                         row_tags=row_tags, between=(lo, hi), values=values)
            for j in range(n):
                t, m = int(tags[i]), int(row_tags[j])
                want = (bool(allowed[j]) and j != exclude[i] and (group[i] < 0 or groups[j] == group[i])
                        and (t == 0 or ((m & t) == t if mode == "all" else (m & t) != 0))
                        and all(lo[i, c] <= values[j, c] <= hi[i, c] for c in range(2)))
                assert got[j] == want, (mode, i, j)
            if i == 3:
                assert not got.any()
    # nothing given: every row passes; each argument alone is taken alone
    assert passes(0, n).all()
    assert passes(0, n, exclude=exclude).sum() == n - 1 and passes(1, n, exclude=exclude).all()
    np.testing.assert_array_equal(passes(2, n, group=group, groups=groups), groups == 3)


def test_restricted_k_best_is_the_full_sort_over_passing_rows():
    rng = np.random.RandomState(1)
    n = 400
    part = rng.randint(0, 30, size=n).astype(np.float32)         # many ties
    for frac, k in ((0.5, 10), (0.02, 10), (0.0, 4), (1.0, 1), (0.3, 400)):
        ok = rng.rand(n) < frac
        order = np.lexsort((np.arange(n), part))
        order = order[ok[order]][:k]
        want = np.concatenate([order, np.full(k - len(order), -1, dtype=np.int64)])
        got = restricted_k_best(part, ok, k)
        np.testing.assert_array_equal(got, want)
        dist = restricted_dist(part, got)
        assert dist.dtype == np.float32
        np.testing.assert_array_equal(dist[got >= 0], part[got[got >= 0]])
        assert np.isinf(dist[got < 0]).all() and (dist[got < 0] > 0).all()


def _slow_counts(part, ok, k, seg):
    n = len(part)
    ns = min(n, NS)
    sample = sorted(part[e * (n // ns)] for e in range(ns) if ok[e * (n // ns)])
    tau = sample[k - 1] if len(sample) >= k else np.inf
    counts = []
    for s0 in range(0, n, seg):
        end = min(n, s0 + seg)
        counts.append(sum(1 for j in range(s0, end) if ok[j] and part[j] <= tau))
        seen = sorted(part[j] for j in range(end) if ok[j])
        if len(seen) >= k and seen[k - 1] <= tau:
            tau = seen[k - 1]
    return counts


def test_restricted_within_tau_per_segment_against_the_loop():
    rng = np.random.RandomState(2)
    n, k = 700, 5
    part = rng.randint(0, 1000, size=n).astype(np.float32)
    for frac in (1.0, 0.4, 0.01, 0.0):
        ok = rng.rand(n) < frac
        for seg in (None, 32, 96, 256):
            got = restricted_within_tau_per_segment(part, ok, k, seg)
            assert got == _slow_counts(part, ok, k, segment_rows(k, n) if seg is None else seg), (frac, seg)
    # everything passes, the rule's segment: the unrestricted model
    assert restricted_within_tau_per_segment(part, np.ones(n, bool), k) == within_tau_per_segment(part, k)
    # fewer than k passing sample rows: tau is +inf and a segment appends every passing row until k were seen
    ok = np.zeros(n, bool)
    ok[[3, 40, 41, 600]] = True
    assert restricted_within_tau_per_segment(part, ok, k, 32)[:2] == [1, 2]
    assert sum(restricted_within_tau_per_segment(part, ok, k, 32)) == 4


def test_retry_segment_cannot_overflow():
    for k in (1, 10, 100, 1024):
        seg = retry_segment_rows(k)
        assert seg % 32 == 0 and seg + k <= CAP < seg + 32 + k


def test_ivf_knn_brute_refuses_before_any_device_call():
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import AllowSet
    ivf = IVF("angular", 4, FastPQ(2))          # (never fitted: nothing reaches the device)
    qs = np.zeros((2, 4), np.float32)
    with pytest.raises(ValueError, match="without values"):
        ivf.knn_brute(qs, 1, between=(0, 1))
    with pytest.raises(ValueError, match="tags_mode"):
        ivf.knn_brute(qs, 1, tags=1, tags_mode="some")
    with pytest.raises(TypeError, match="AllowSet"):
        ivf.knn_brute(qs, 1, allowed=object.__new__(AllowSet))


def test_device_knn_brute_refuses_an_allow_set():
    from tinyknn_amd.ivf import AllowSet, DeviceIndex
    dev = object.__new__(DeviceIndex)
    dev.d = 4
    with pytest.raises(TypeError, match="AllowSet"):
        dev.knn_brute(np.zeros((2, 4), np.float32), 1, allowed=object.__new__(AllowSet))


def test_the_signatures_carry_the_keywords():
    """IVF.knn_brute takes every keyword.  On the device index the restrictions are keywords of knn_brute and of
    knn_brute_dist, and the part values come from knn_brute_dist alone: tests/test_distances_cpu.py holds that
    DeviceIndex.knn_brute takes no return_distances."""
    from tinyknn_amd import IVF
    from tinyknn_amd.ivf import DeviceIndex
    restrictions = dict(allowed=None, exclude=None, group=None, tags=None, tags_mode="any", between=None)
    for f in (IVF.knn_brute, DeviceIndex.knn_brute, DeviceIndex.knn_brute_dist):
        p = inspect.signature(f).parameters
        for name in restrictions:
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, (f.__qualname__, name)
        assert "per_group" not in p
    assert IVF.knn_brute.__kwdefaults__ == dict(restrictions, return_distances=False)
    assert DeviceIndex.knn_brute.__kwdefaults__ == DeviceIndex.knn_brute_dist.__kwdefaults__ == restrictions


def test_the_library_declares_the_entry_point():
    from tinyknn_amd import _lib
    assert "tk_index_knn_brute_ex" in _lib.SIGNATURES and "tk_index_knn_brute" in _lib.SIGNATURES
