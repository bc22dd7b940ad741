"""The ranking of the staged rescoring kernel (rescore.hip: strict_counts), modelled in numpy.

A lane counts, per value, only `du < dv` over all nc distances.  That count is the value's final rank exactly when every
pair of the nc distances is strictly ordered, and exactly then the counts add up to nc (nc - 1) / 2: an ordered pair
adds 1 to the sum, a pair that is not (equal values, +0 / -0, a pair with a NaN) adds 0.  A short sum sends the wave to
the loop it replaced, `(du < dv) || (du == dv && u < t)`, which breaks ties by position.  The reference is numpy's
stable argsort: ascending, equal values by position.  (A NaN is below nothing and nothing is below it: in the loop
the NaN's own rank is 0, as it always was; every other value's rank is its place in the stable argsort, which sorts
NaNs last.)"""
import numpy as np
import pytest

LENGTHS = [2, 3, 4, 5, 10, 11, 31, 32, 33, 63, 64, 65, 111, 128, 129, 255, 256]


def strict_counts(ds):
    """cnt[t] = #{u : ds[u] < ds[t]} in float32, and whether the wave's sum says that they are the ranks"""
    ds = np.asarray(ds, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        cnt = (ds[None, :] < ds[:, None]).sum(axis=1)
    n = len(ds)
    return cnt, int(cnt.sum()) == n * (n - 1) // 2


def tie_loop(ds):
    """the loop of the parent kernel, the fallback of the new one"""
    ds = np.asarray(ds, dtype=np.float32)
    pos = np.arange(len(ds))
    with np.errstate(invalid="ignore"):
        below = (ds[None, :] < ds[:, None]) | ((ds[None, :] == ds[:, None]) & (pos[None, :] < pos[:, None]))
    return below.sum(axis=1)


def model_ranks(ds):
    cnt, ordered = strict_counts(ds)
    return (cnt if ordered else tie_loop(ds)), not ordered


def top_k(ranks, k):
    """what the kernel writes: out[rank] = position, for rank < k"""
    out = np.full(k, -1, dtype=np.int64)
    for t, r in enumerate(ranks):
        if r < k:
            assert out[r] == -1, "two values of one rank"
            out[r] = t
    return out


def distinct(rng, n):
    """n float32 values, no two equal, none zero"""
    while True:
        v = rng.standard_normal(n).astype(np.float32) ** 2 + np.float32(0.5)
        if len(np.unique(v)) == n:
            return v


def _against_argsort(ds, k, must_fall_back):
    ranks, fell_back = model_ranks(ds)
    assert fell_back == must_fall_back
    order = np.argsort(ds, kind="stable")
    np.testing.assert_array_equal(ranks[order], np.arange(len(ds)))     # a permutation: the stable one
    np.testing.assert_array_equal(top_k(ranks, k), order[:k])
    np.testing.assert_array_equal(tie_loop(ds), ranks)                  # ... and the parent's loop gives it always


@pytest.mark.parametrize("n", LENGTHS)
def test_no_ties_the_counts_are_the_ranks(n):
    rng = np.random.default_rng(n)
    for k in sorted({1, min(10, n - 1), n - 1}):
        _against_argsort(distinct(rng, n), k, must_fall_back=False)


@pytest.mark.parametrize("n", LENGTHS)
def test_one_tie_inside_the_first_k(n):
    rng = np.random.default_rng(100 + n)
    for k in sorted({2, min(10, n), n}):
        ds = distinct(rng, n)
        order = np.argsort(ds, kind="stable")
        a = int(rng.integers(0, k - 1))
        ds[order[a + 1]] = ds[order[a]]                 # places a and a + 1 < k hold one value
        _against_argsort(ds, k, must_fall_back=True)


@pytest.mark.parametrize("n", [n for n in LENGTHS if n >= 3])
def test_one_tie_across_places_k_and_k_plus_1(n):
    rng = np.random.default_rng(200 + n)
    for k in sorted({1, min(10, n - 1), n - 1}):
        for _ in range(4):                              # (either of the two may sit at the lower position)
            ds = distinct(rng, n)
            order = np.argsort(ds, kind="stable")
            lo, hi = order[k - 1], order[k]             # the last place kept and the first one dropped
            ds[hi] = ds[lo]
            _against_argsort(ds, k, must_fall_back=True)
            kept = top_k(model_ranks(ds)[0], k)[-1]
            assert kept == min(lo, hi)


@pytest.mark.parametrize("n", LENGTHS)
def test_all_values_equal(n):
    for k in sorted({1, min(10, n), n}):
        ds = np.full(n, 0.75, dtype=np.float32)
        cnt, ordered = strict_counts(ds)
        assert not ordered and not cnt.any()
        _against_argsort(ds, k, must_fall_back=True)
        np.testing.assert_array_equal(top_k(model_ranks(ds)[0], k), np.arange(k))


@pytest.mark.parametrize("n", LENGTHS)
def test_plus_and_minus_zero_are_an_unordered_pair(n):
    rng = np.random.default_rng(300 + n)
    ds = distinct(rng, n)
    a, b = rng.choice(n, size=2, replace=False)
    ds[a], ds[b] = np.float32(0.0), np.float32(-0.0)
    assert len({x.tobytes() for x in ds}) == n          # all bit patterns differ, yet one pair is not ordered
    ranks, fell_back = model_ranks(ds)
    assert fell_back
    # (numpy's sort compares +0 and -0 equal too, so the stable argsort is still the reference)
    _against_argsort(ds, min(10, n), must_fall_back=True)
    assert top_k(ranks, 2).tolist() == sorted((int(a), int(b)))


@pytest.mark.parametrize("n", LENGTHS)
def test_a_nan_sends_the_wave_to_the_loop(n):
    rng = np.random.default_rng(400 + n)
    ds = distinct(rng, n)
    at = int(rng.integers(0, n))
    ds[at] = np.float32(np.nan)
    cnt, ordered = strict_counts(ds)
    assert not ordered                                  # n - 1 pairs hold the NaN: the sum is short by as many
    assert int(cnt.sum()) == (n - 1) * (n - 2) // 2
    ranks, fell_back = model_ranks(ds)
    assert fell_back
    np.testing.assert_array_equal(ranks, tie_loop(ds))  # the parent's answer, whatever it is
    order = np.argsort(ds, kind="stable")               # NaN last
    assert order[-1] == at
    real = order[:-1]
    np.testing.assert_array_equal(ranks[real], np.arange(n - 1))
    assert ranks[at] == 0


def test_the_sum_check_fires_exactly_where_a_pair_is_unordered():
    """random vectors drawn from few values (many ties), from many (none), with zeros of both signs and NaNs mixed in"""
    rng = np.random.default_rng(7)
    fired = quiet = 0
    for trial in range(400):
        n = int(rng.integers(2, 257))
        pool = int(rng.choice([2, 5, n, 4 * n, 1 << 20]))
        ds = rng.integers(0, pool, size=n).astype(np.float32) + np.float32(1.0)
        if trial % 5 == 0:
            ds[rng.integers(0, n)] = np.float32(-0.0)
            ds[rng.integers(0, n)] = np.float32(0.0)
        if trial % 7 == 0:
            ds[rng.integers(0, n)] = np.float32(np.nan)
        with np.errstate(invalid="ignore"):
            lt = ds[None, :] < ds[:, None]
        unordered = bool((~(lt | lt.T))[np.triu_indices(n, 1)].any())
        _, fell_back = model_ranks(ds)
        assert fell_back == unordered, (trial, n, pool)
        fired += fell_back
        quiet += not fell_back
        if not np.isnan(ds).any():
            _against_argsort(ds, int(rng.integers(1, n + 1)), must_fall_back=unordered)
    assert fired > 50 and quiet > 50
