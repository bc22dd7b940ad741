"""Allowed sets on the CPU: the guarded reference (tests/allowed_reference.py) against the oracle, the equivalence the
device relies on (guarded `insert` == the empty value for every disallowed row), and the Python argument checks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from allowed_reference import guarded_query, replay_blocks  # noqa: E402
from conftest import G6_TAGS, golden, split_lists  # noqa: E402


def _oracle_index(oracle, g):
    codes, ids = split_lists(g)
    R = g["R"] if "R" in g else None
    return oracle.OracleIndex(g["pq_centers"], 2, R, float(g["sqrt_n_blocks"]), g["active_centers"],
                              g["center_codes"], codes, g["list_sizes"], ids, g["data"])


@pytest.mark.parametrize("tag", G6_TAGS)
def test_all_true_mask_is_the_oracle(oracle, tag):
    g = golden(f"g6_ivf_{tag}.npz")
    ox = _oracle_index(oracle, g)
    every = np.ones(len(g["data"]), dtype=bool)
    for n_probes in g["probes_list"]:
        n_probes = int(n_probes)
        for qn in g["qn"]:
            want, wd = ox.query(qn, 10, n_probes, debug=True)
            for allowed in (None, every):
                got, gd = guarded_query(oracle, ox, qn, 10, n_probes, allowed=allowed, debug=True)
                np.testing.assert_array_equal(got, want)
                for key in ("probes", "heap_idx", "heap_val"):
                    np.testing.assert_array_equal(gd[key], wd[key])


def _streams(seed, repeat):
    rng = np.random.default_rng(seed)
    for t in range(60):
        n = int(rng.integers(1, 400))
        chunks = (n + 15) // 16
        kind = t % 4
        if kind == 0:           # random values
            vals = rng.integers(0, 256, size=(chunks, 16))
        elif kind == 1:         # descending: every block refreshes the bound
            vals = np.linspace(255, 0, chunks * 16).astype(np.int64).reshape(chunks, 16)
        elif kind == 2:         # many ties around a few values
            vals = rng.choice([0, 1, 2, 126, 127, 128, 254, 255], size=(chunks, 16))
        else:                   # the nearest rows first, then noise
            vals = rng.integers(0, 256, size=(chunks, 16))
            vals[0] = np.arange(16) * 3
        N = max(8, n // (3 if repeat else 1))
        labels = rng.integers(0, N, size=n) if repeat else rng.permutation(N)[:n]
        sel = [1.0, 0.5, 0.1, 0.01, 0.0][t % 5]
        allowed = rng.random(N) < sel
        if t % 7 == 3:          # adversarial: only every other label, so passing blocks are half disallowed
            allowed = np.arange(N) % 2 == 0
        R = int(rng.integers(1, 40))
        yield vals.astype(np.uint8), n, labels.astype(np.int64), allowed, R


@pytest.mark.parametrize("signd", [True, False])
@pytest.mark.parametrize("repeat", [False, True])
def test_guarded_insert_equals_empty_value(oracle, signd, repeat):
    for vals, n, labels, allowed, R in _streams(7 + 2 * int(signd) + int(repeat), repeat):
        heaps = []
        for substitute in (False, True):
            hidx = np.zeros(R, dtype=np.int64)
            hval = np.zeros(R, dtype=np.int32)
            oracle.init_heap(hidx, hval, signd)
            # several lists through one heap, as the probed lists of a query
            for part in np.array_split(np.arange(len(vals)), 3):
                if len(part) == 0:
                    continue
                lo, hi = int(part[0]), int(part[-1]) + 1
                replay_blocks(oracle, vals[lo:hi], min(n, 16 * hi) - 16 * lo, labels[16 * lo:], hidx, hval, signd,
                              allowed, substitute)
            heaps.append((hidx, hval))
        np.testing.assert_array_equal(heaps[0][0], heaps[1][0])
        np.testing.assert_array_equal(heaps[0][1], heaps[1][1])


def test_allowed_argument_checks():
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import AllowSet, DeviceIndex

    class FakeDev:
        pass

    # the shape / type checks come before any device call
    ivf = IVF("angular", 4, FastPQ(2))
    with pytest.raises(NotImplementedError, match="fast=True"):
        ivf._dev = FakeDev()
        ivf._dev.world, ivf._dev.rank = 1, 0
        ivf.query_batch(np.zeros((1, 4), np.float32), 1, fast=True, allowed=[0])
    with pytest.raises(TypeError, match="prepared set"):
        DeviceIndex.query_batch_dev(object.__new__(DeviceIndex), 0, 0, 0, 1, 1, 1, 0, allowed=np.ones(3, bool))
    assert "allowed" in DeviceIndex.query_batch.__kwdefaults__
    assert "allowed" in IVF.query.__kwdefaults__ and "allowed" in IVF.query_batch.__kwdefaults__
    np.testing.assert_array_equal(AllowSet.mask_of([3, 1, 3], 5), [0, 1, 0, 1, 0])
    np.testing.assert_array_equal(AllowSet.mask_of(np.array([True, False]), 2), [1, 0])
    assert AllowSet.mask_of(np.array([], np.int64), 3).sum() == 0
    with pytest.raises(ValueError, match="shape"):
        AllowSet.mask_of(np.ones(4, bool), 5)
    with pytest.raises(ValueError, match="row ids"):
        AllowSet.mask_of([0, 5], 5)
    with pytest.raises(ValueError, match="row ids"):
        AllowSet.mask_of([-1], 5)
    with pytest.raises(TypeError):
        AllowSet.mask_of(np.ones((2, 2), np.int64), 5)
    with pytest.raises(TypeError):
        AllowSet.mask_of([0.5], 5)
