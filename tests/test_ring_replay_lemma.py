"""The lemma behind the lane replay's per-lane ring (heap.hip, RING), on the CPU with the oracle's loop (no GPU):

A block whose minimum is >= a bound captured EARLIER in the replay is >= the bound at its own start (a bound only
falls): `query_pq` enters it, inserts nothing and leaves the bound where it was.  So leaving such blocks out — here:
overwriting them with the largest value, which nothing is below — gives bit-identical heap arrays, layout included.
The ring picks its blocks against a bound that is 0 .. many blocks old; every age is tried.
"""
import numpy as np
import pytest

R_SIZES = (3, 8, 30, 111)


def tables_and_codes(oracle, values):
    """Two 4-bit blocks whose table entries add up to any int8 without saturating: 16 (c0 - 8) + c1 (and two blocks
    of zeros: the reference's kernels take blocks four at a time)."""
    v = np.asarray(values, dtype=np.int64)
    assert v.min() >= -128 and v.max() <= 127 and len(v) % 16 == 0
    T = np.stack([16 * (np.arange(16) - 8), np.arange(16), np.zeros(16, int), np.zeros(16, int)]).astype(np.int8)
    u = v + 128
    codes = np.stack([u >> 4, u & 15, 0 * u, 0 * u], axis=1).astype(np.uint8)
    return oracle.transform_tables(T.view(np.uint8)), oracle.transform_data(codes)


def replay(oracle, values, R, trace=None):
    """Heap arrays of the reference's loop over `values`; trace[b] = the bound when block b is entered."""
    tt, packed = tables_and_codes(oracle, values)
    out = np.zeros(2 * len(packed), np.uint64)
    oracle.estimate_pq(packed, tt, out, True)
    np.testing.assert_array_equal(out.view(np.int8)[:len(values)], values)      # the rows are what was asked for
    hi, hv = np.zeros(R, np.int64), np.zeros(R, np.int32)
    oracle.init_heap(hi, hv, True)
    if trace is None:
        oracle.query_pq(packed, len(values), tt, hi, hv, True)
        return hi, hv
    for b in range(len(packed)):
        trace[b] = int(np.int8(hv[0] & 0xff))
        oracle.query_pq(packed[b:b + 1], 16, tt, hi, hv, True, labels=np.arange(16 * b, 16 * b + 16, dtype=np.int64))
    return hi, hv


def rows(kind, rng, n):
    if kind == "random":
        return rng.integers(-128, 128, size=n)
    if kind == "clustered":                        # a list of near rows, then far ones: most later blocks never pass
        return np.clip(np.concatenate([rng.normal(-60, 30, n // 4), rng.normal(40, 40, n - n // 4)]), -128, 127).astype(np.int64)
    if kind == "equal":
        return np.full(n, -7)
    if kind == "falling":                          # strictly: all 256 values once, every row passes
        return 127 - np.arange(256)
    if kind == "rising":                           # strictly: nothing passes once the heap is full
        return -128 + np.arange(256)
    if kind == "every40":                          # one passing row every 40 blocks, each lower than the last
        v = np.full(n, 127)
        at = np.arange(0, n, 40 * 16) + 5
        v[at] = 120 - np.arange(len(at))
        return v
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["random", "clustered", "equal", "falling", "rising", "every40"])
def test_blocks_at_or_above_an_earlier_bound_are_no_ops(oracle, kind):
    rng = np.random.default_rng(len(kind))
    n = 16 * 420
    v = rows(kind, rng, n)
    n = len(v)
    mins = v.reshape(-1, 16).min(axis=1)
    dropped = 0
    for R in R_SIZES:
        bounds = np.zeros(len(mins), np.int64)
        hi, hv = replay(oracle, v, R, trace=bounds)
        hi1, hv1 = replay(oracle, v, R)
        np.testing.assert_array_equal(hi, hi1)      # (block by block is the same loop)
        np.testing.assert_array_equal(hv, hv1)
        assert (np.diff(bounds) <= 0).all()         # a bound only falls
        for age in (0, 1, 3, 8, 33, "random"):
            ages = rng.integers(0, 64, size=len(mins)) if age == "random" else np.full(len(mins), age)
            early = bounds[np.maximum(np.arange(len(mins)) - ages, 0)]      # the bound `ages` blocks before
            drop = mins >= early
            w = v.copy().reshape(-1, 16)
            w[drop] = 127
            gi, gv = replay(oracle, w.reshape(-1), R)
            np.testing.assert_array_equal(gi, hi, err_msg=f"{kind} R={R} age={age}")
            np.testing.assert_array_equal(gv, hv, err_msg=f"{kind} R={R} age={age}")
            dropped += int(drop.sum())
    assert dropped > 0 or kind == "falling"
