"""Ranged queries on the awkward indexes of tests/restricted_shapes.py (lists shorter than a chunk and empty ones, a
single list, more probes than lists, probe lists that wrap, repeated labels, the half store, indexes changed by add()
and remove()), composed with whatever restriction the case already carries: tests/between_shapes.py::BetweenCase draws
the values, the query ranges and, for half of the seeds, tags.  Every leg compares ids, probes, heap_idx and heap_val
exactly with tests/between_reference.py::ranged_batch; the census of tests/test_between_cpu.py shows what the default
seeds hold.  No case is skipped here that the census counted: a seed skips only where the host build refused its
shape, and the census counts none of those."""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import between_shapes as bs  # noqa: E402
from restricted_shapes import Case  # noqa: E402,F401  (the cases are its, unchanged)
from store_reference import exact_distances, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("probes", "heap_idx", "heap_val")
MODES = ((0, 0), (1, 1), (2, 2), (0, 2), (3, 0))      # (heap_mode, scan_mode) as tests/test_fuzz_gpu.py
# seeds that failed once, run whatever the range becomes: {seed: why}
NAMED = {}
SEEDS = sorted(set(bs.fuzz_seeds()) | set(NAMED))


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    return tinyknn_amd


def _same(got, gd, want, wd, msg=""):
    np.testing.assert_array_equal(got, want, err_msg=str(msg))
    for key in KEYS:
        np.testing.assert_array_equal(gd[key], wd[key], err_msg=f"{key} {msg}")


@contextlib.contextmanager
def opened(seed):
    """-> (case, a device index of its own with groups, tags and values set, a prepared AllowSet of the case's mask or
    None)"""
    t = bs.fuzz_case(seed)
    if t.skipped is not None:
        pytest.skip(t.skipped)
    from tinyknn_amd.ivf import DeviceIndex
    dev = DeviceIndex(t.case.ivf)       # (its own: the case stays as it was made)
    try:
        if t.case.groups is not None:
            dev.set_groups(t.case.groups)
        if t.tags is not None:
            dev.set_tags(t.tags)
        dev.set_values(t.values)
        aset = None if t.case.allowed is None else dev.allow(t.case.allowed)
        yield t, dev, aset
    finally:
        dev.close()                     # (closes its sets too)


def _restore(dev):
    from tinyknn_amd import _lib
    dev.set_heap_mode(0)
    dev.set_scan_mode(0)
    dev.set_plain_scan(True)
    dev.set_option(_lib.OPT_PAIR_NQ, 4)
    dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)


@pytest.mark.parametrize("seed", SEEDS)
def test_execution_modes(tk, oracle, seed):
    with opened(seed) as (t, dev, aset):
        c = t.case.shape
        want, wd = t.want()
        kw = t.device_kwargs(aset)
        try:
            for plain in (False, "always"):
                dev.set_plain_scan(plain)
                for heap_mode, scan_mode in MODES:
                    dev.set_heap_mode(heap_mode)
                    dev.set_scan_mode(scan_mode)
                    got, gd = dev.query_batch(t.case.qn, t.case.qp, c["k"], c["n_probes"], debug=True, **kw)
                    _same(got, gd, want, wd, f"{t} plain={plain} heap_mode={heap_mode} scan_mode={scan_mode}")
            lo, hi = t.between
            neg, pos = (-np.inf, np.inf) if lo.dtype.kind == "f" else (bs.INT64_MIN, bs.INT64_MAX)
            bounded = bool(((lo != neg) | (hi != pos)).any())       # (one table, made by the first call with a bounded end)
            assert dev.value_table()["builds"] == (1 if bounded else 0)
        finally:
            _restore(dev)


@pytest.mark.parametrize("seed", SEEDS)
def test_forced_flags_and_both_replay_sizes(tk, oracle, seed):
    from tinyknn_amd import _lib
    with opened(seed) as (t, dev, aset):
        c = t.case.shape
        want, wd = t.want()
        try:
            for pair_nq in (4, 8192):
                dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
                for limit in (0x7fffffff, -128):
                    dev.set_plain_scan("always")
                    dev.set_option(_lib.OPT_PLAIN_LIMIT, limit)
                    got, gd = dev.query_batch(t.case.qn, t.case.qp, c["k"], c["n_probes"], debug=True,
                                              **t.device_kwargs(aset))
                    st = dev.plain_stats()
                    _same(got, gd, want, wd, f"{t} pair_nq={pair_nq} limit={limit} {st}")
                    # limit -128: every query with a plain list fails the lemma's check: scanned again exactly, masked again (`only`)
                    if limit == -128 and st["plain_units"] > 0:
                        assert st["flagged_queries"] > 0, (t, st)
        finally:
            _restore(dev)


@pytest.mark.parametrize("seed", SEEDS)
def test_distances(tk, oracle, seed):
    with opened(seed) as (t, dev, aset):
        c = t.case.shape
        want, _ = t.want()
        ids, dist = dev.query_batch(t.case.qn, t.case.qp, c["k"], c["n_probes"], return_distances=True,
                                    **t.device_kwargs(aset))
        np.testing.assert_array_equal(ids, want, err_msg=str(t))
        assert same_bits(dist, exact_distances(oracle, t.case.qn, t.case.ref_data, ids)), t
