"""The radius search without a GPU: its NumPy reference against an obvious form, the two ABI symbols against the
header, and the refusals IVF.radius_search / radius_count make before any device call."""
import os
import re

import numpy as np
import pytest

from radius_reference import passes, radius_csr, radius_list

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tinyknn_hip.h")


@pytest.mark.parametrize("seed", range(6))
def test_radius_list_is_the_lexsort_of_the_rows_within_the_radius(seed):
    rng = np.random.RandomState(seed)
    n = int(rng.choice([1, 40, 500]))
    part = rng.randint(-3, 12, size=n).astype(np.int64)          # many ties, some negative
    ok = rng.rand(n) < 0.6 if seed % 2 else None
    for r in (-5.0, 0.0, 3.0, 3.5, np.inf):
        order = np.lexsort((np.arange(n), part))                # ascending (part, row)
        keep = [j for j in order if part[j] <= r and (ok is None or ok[j])]
        ids, dist = radius_list(part, ok, r)
        assert ids.dtype == np.int64 and dist.dtype == np.float32
        np.testing.assert_array_equal(ids, np.asarray(keep, dtype=np.int64))
        np.testing.assert_array_equal(dist, part[keep].astype(np.float32))


def test_radius_csr_joins_the_lists_and_repeats_limits_of_empty_ones():
    part = np.array([[0, 5, 5, 1], [9, 9, 9, 9], [2, 2, 7, 0]], dtype=np.int64)
    lims, ids, dist = radius_csr(part, None, np.array([5.0, 1.0, 2.0], np.float32))
    np.testing.assert_array_equal(lims, [0, 4, 4, 7])
    np.testing.assert_array_equal(ids, [0, 3, 1, 2, 3, 0, 1])
    np.testing.assert_array_equal(dist, np.array([0, 1, 5, 5, 0, 2, 2], np.float32))
    oks = [passes(i, 4, exclude=np.array([0, -1, 3])) for i in range(3)]
    lims, ids, _ = radius_csr(part, oks, 5.0)
    np.testing.assert_array_equal(lims, [0, 3, 3, 5])
    np.testing.assert_array_equal(ids, [3, 1, 2, 0, 1])
    lims, ids, dist = radius_csr(part[:0], None, 1.0)
    assert lims.tolist() == [0] and ids.dtype == np.int64 and dist.dtype == np.float32 and len(ids) == len(dist) == 0


def _declared_arguments(name):
    text = open(HEADER).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/tinyknn_hip.h"
    return len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))


@pytest.mark.parametrize("name,n_args", [("tk_index_radius_brute", 15), ("tk_index_radius_fetch", 3)])
def test_the_radius_symbols_are_bound_with_the_headers_argument_counts(name, n_args):
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
        fn(Q, 1.0, allowed=object.__new__(AllowSet))
    with pytest.raises(ValueError, match="NaN"):
        fn(Q, np.nan)
    with pytest.raises(ValueError, match="NaN"):
        fn(Q, np.array([0.5, np.nan, 1.0]))
    with pytest.raises(ValueError, match="one entry per query"):
        fn(Q, np.array([0.5, 1.0]))
    with pytest.raises(ValueError, match="tags_mode"):
        fn(Q, 1.0, tags=1, tags_mode="some")
    with pytest.raises(ValueError, match="without values"):
        fn(Q, 1.0, between=(0, 1))
    with pytest.raises(AssertionError, match="a device call was made"):       # a good call reaches the device
        fn(Q, np.array([0.5, np.inf, -1.0]))


def test_query_radius_casts_with_float32_and_takes_inf_and_negative_values():
    from tinyknn_amd.ivf import query_radius
    a = query_radius(0.1, 4)
    assert a.dtype == np.float32 and a.shape == (4,) and (a == np.float32(0.1)).all()
    b = query_radius(np.array([np.inf, -1.0, 2.0 ** 0.5], np.float64), 3)
    np.testing.assert_array_equal(b, np.array([np.inf, -1.0, np.float32(2.0 ** 0.5)], np.float32))
    assert query_radius(1.0, 0).shape == (0,)
    with pytest.raises(TypeError):
        query_radius("near", 2)
    with pytest.raises(TypeError):
        query_radius(np.ones((2, 2)), 2)


def test_max_results_is_checked_before_the_device_is_asked():
    from tinyknn_amd.ivf import DeviceIndex
    dev = object.__new__(DeviceIndex)
    dev.d, dev.N, dev.world = 4, 10, 1
    for bad in (-1, 2**31):
        with pytest.raises(ValueError, match="max_results"):
            dev.radius_brute(np.zeros((2, 4), np.float32), 1.0, max_results=bad)
