"""The exact search inside a query's own group (tk_index_knn_group) without a GPU: the signatures and
the null-index returns of the ABI, what the Python layer refuses before it touches a device, the reference helper
against the restricted exact search's on integer data, the model of the candidate buffer, the split and merge of
IVF.query_batch(exact_below=) against a stand-in device index, and what the compiler reports for the kernels."""
import inspect
import os
import re

import numpy as np
import pytest

from brute_reference import int_part
from brute_restricted_reference import passes, restricted_k_best
from group_exact_reference import (append_model, einsum_distances, knn_group_reference, reference_data, same_bits,
                                   stored_mask)
from kernel_usage import have_hipcc, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tk_index_knn_group", "tk_index_group_sizes", "tk_index_group_rows")


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_and_null_index_is_an_argument_error():
    from tinyknn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tinyknn_hip.h")).read()
    declared = set(re.findall(r"\b(tk_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), f"{name} declared but not exported"
        assert name in _lib.SIGNATURES, name
    # the restricted exact search's arguments, the group moved in front (it is required)
    assert len(_lib.SIGNATURES["tk_index_knn_group"][1]) == len(_lib.SIGNATURES["tk_index_knn_brute_ex"][1])
    out = np.zeros(4, dtype=np.int64)
    assert lib.tk_index_knn_group(None, None, 0, 1, None, None, None, None, 0, None, None, None) == -1
    assert lib.tk_index_group_sizes(None, None, 0, None) == -1
    assert lib.tk_index_group_rows(None, _lib.ptr(out, _lib._i64p)) == -1
    assert (_lib.GROUP_EXACT_TILE, _lib.GROUP_EXACT_CAP) == (256, 2048)
    src = open(os.path.join(ROOT, "tinyknn_amd", "csrc", "group_exact.hip")).read()
    assert "#define GX_TILE 256" in src and "#define GX_CAP 2048" in src


def test_the_signatures_carry_the_keywords():
    from tinyknn_amd import IVF
    from tinyknn_amd.ivf import DeviceIndex
    from tinyknn_amd import multi_gpu
    kw = dict(allowed=None, exclude=None, tags=None, tags_mode="any", between=None, return_distances=False)
    for f in (IVF.knn_group, DeviceIndex.knn_group):
        p = inspect.signature(f).parameters
        assert list(p)[:4] == ["self", list(p)[1], "k", "group"] and f.__kwdefaults__ == kw, f.__qualname__
        assert "per_group" not in p
    p = inspect.signature(IVF.query_batch).parameters
    assert p["exact_below"].kind is inspect.Parameter.KEYWORD_ONLY and p["exact_below"].default is None
    # the calls that do not take it
    for f in (IVF.query, DeviceIndex.query_batch, DeviceIndex.query_batch_dev, multi_gpu.ListShardedIndex.query_batch,
              multi_gpu.ReplicaGroup.query_batch):
        assert "exact_below" not in inspect.signature(f).parameters, f.__qualname__
    assert callable(DeviceIndex.group_sizes) and callable(DeviceIndex.group_rows)


# ---- refusals before any device call -----------------------------------------------------------------------------------
def test_ivf_refuses_before_any_device_call():
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import AllowSet
    ivf = IVF("angular", 4, FastPQ(2))          # (never fitted: nothing reaches the device)
    qs = np.zeros((2, 4), np.float32)
    with pytest.raises(TypeError, match="AllowSet"):
        ivf.knn_group(qs, 1, 0, allowed=object.__new__(AllowSet))
    with pytest.raises(ValueError, match="without values"):
        ivf.knn_group(qs, 1, 0, between=(0, 1))
    with pytest.raises(ValueError, match="tags_mode"):
        ivf.knn_group(qs, 1, 0, tags=1, tags_mode="some")
    with pytest.raises(AssertionError, match=">= 0"):
        ivf.knn_group(qs, 1, [0, -1])
    with pytest.raises(ValueError, match="one entry per query"):
        ivf.knn_group(qs, 1, [0, 1, 2])
    with pytest.raises(TypeError):
        ivf.knn_group(qs, 1, 0.5)
    # exact_below
    with pytest.raises(ValueError, match="needs group="):
        ivf.query_batch(qs, 1, exact_below=10)
    with pytest.raises(ValueError, match="per_group"):
        ivf.query_batch(qs, 1, group=0, per_group=1, exact_below=10)
    with pytest.raises(TypeError, match="AllowSet"):
        ivf.query_batch(qs, 1, group=0, allowed=object.__new__(AllowSet), exact_below=10)
    with pytest.raises(NotImplementedError, match=r"fast=True with exact_below= is not supported"):
        ivf.query_batch(qs, 1, fast=True, group=0, exact_below=10)
    with pytest.raises(TypeError, match="exact_below"):
        ivf.query_batch(qs, 1, group=0, exact_below=1.5)
    with pytest.raises(ValueError, match="exact_below"):
        ivf.query_batch(qs, 1, group=0, exact_below=-1)
    with pytest.raises(ValueError, match="without values"):
        ivf.query_batch(qs, 1, group=0, between=(0, 1), exact_below=10)
    assert ivf._dev is None


def test_device_index_refuses_before_any_device_call():
    from tinyknn_amd.ivf import AllowSet, DeviceIndex
    dev = object.__new__(DeviceIndex)
    dev.d, dev.N, dev.world, dev._f64 = 4, 100, 1, False
    X = np.zeros((2, 4), np.float32)
    with pytest.raises(TypeError, match="AllowSet"):
        dev.knn_group(X, 1, 0, allowed=object.__new__(AllowSet))
    with pytest.raises(AssertionError, match=">= 0"):
        dev.knn_group(X, 1, -1)
    with pytest.raises(ValueError):
        dev.knn_group(X, 1, [0, 2**31 - 1])
    with pytest.raises(ValueError, match="exclude"):
        dev.knn_group(X, 1, 0, exclude=[0, 100])
    with pytest.raises(TypeError):
        dev.group_sizes([0.5])
    with pytest.raises(ValueError):
        dev.group_sizes([2**31])
    dev.world = 2
    with pytest.raises(RuntimeError, match="list-sharded"):
        dev.knn_group(X, 1, 0)


# ---- the references ----------------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_restricted_exact_search_on_integer_data(oracle):
    """Integer coordinates: `part` and the rescoring's distance are the same exact integers, so they order rows alike
    and the reference must return restricted_k_best's ids — on float32, half (small integers are halves) and float64."""
    rng = np.random.RandomState(3)
    n, d, nq = 600, 12, 9
    Y = rng.randint(-20, 21, size=(n, d)).astype(np.float32)
    X = rng.randint(-20, 21, size=(nq, d)).astype(np.float32)
    Y[50] = Y[40] = Y[30]
    X[0] = Y[30]
    groups = rng.randint(0, 4, size=n).astype(np.int32)
    groups[[30, 40, 50]] = 1
    group = rng.randint(0, 5, size=nq).astype(np.int32)         # (4: an id no row carries)
    group[0] = 1
    stored = stored_mask([np.arange(0, 300), np.array([-1, 700]), np.arange(320, 600)], n)
    assert stored.sum() == 580 and not stored[300:320].any()
    mask = rng.rand(n) < 0.7
    mask[30], mask[40], mask[50] = False, True, True           # the lowest of three identical rows fails
    exclude = rng.randint(-1, n, size=nq)
    exclude[0] = -1
    part = int_part(X, Y)
    for store, data in ((None, Y), ("float16", Y), (None, Y.astype(np.float64))):
        ref = reference_data(data, store)
        assert np.array_equal(ref, data)
        for k in (1, 10, 300):
            ids, dist = knn_group_reference(oracle, X, ref, k, group, groups, stored=stored, allowed=mask, exclude=exclude)
            assert dist.dtype == (np.float64 if data.dtype == np.float64 else np.float32)
            for i in range(nq):
                ok = passes(i, n, allowed=mask, exclude=exclude, group=group, groups=groups) & stored
                np.testing.assert_array_equal(ids[i], restricted_k_best(part[i], ok, k))
                live = ids[i] >= 0
                np.testing.assert_array_equal(dist[i][live], part[i][ids[i][live]])
                assert np.isposinf(dist[i][~live]).all()
            assert (ids[group == 4] == -1).all() and list(ids[0][:2]) == ([40, 50] if k > 1 else [40])
            assert same_bits(dist, einsum_distances(X, ref, ids))
    assert not same_bits(np.zeros(2, np.float32), np.zeros(2, np.float64))
    assert not same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    # the half store's reference rounds the rows
    Z = rng.randn(5, 3).astype(np.float32)
    np.testing.assert_array_equal(reference_data(Z, "float16"), Z.astype(np.float16).astype(np.float32))


def test_oracle_distance_is_numpys_einsum_within_one_ulp_at_the_widths_of_the_gpu_tests(oracle):
    rng = np.random.RandomState(4)
    for d in (1, 20, 100, 127, 128):
        Y = rng.randn(500, d).astype(np.float32)
        x = rng.randn(d).astype(np.float32)
        ref = oracle.sqdist_gather(x, Y, np.arange(500)).astype(np.float32)
        np.testing.assert_array_max_ulp(ref, np.einsum("ij,ij->i", Y - x, Y - x), maxulp=1)


def test_append_model():
    tile, cap = 256, 2048
    # ascending distances: after the first cut nothing is within the bound any more
    up = np.arange(6000, dtype=np.float64)
    assert append_model(up, 10, tile, cap) == (3, cap)
    # descending: every row is appended, a cut whenever the bound says the buffer could overflow
    assert append_model(up[::-1], 10, tile, cap) == (3, cap)    # (8 tiles fill it, then 7 beside the k kept)
    assert append_model(up[::-1], 1024, tile, cap) == (4, cap)   # (then 4 tiles beside the k kept)
    # a group that fits the buffer is never cut in front of a tile; dropped rows take a lane and no slot
    assert append_model(up[:2048], 10, tile, cap) == (0, 2048)
    assert append_model(up[:2049], 10, tile, cap)[0] == 1
    holes = up[:2048].copy()
    holes[::2] = np.nan
    assert append_model(holes, 10, tile, cap) == (0, 1024)
    for k in (1, 10, 100, 1024):
        assert k + tile <= cap


# ---- exact_below against a stand-in device index -----------------------------------------------------------------------
class _StandIn:
    """Answers by marker: a query's first coordinate is its number; knn_group returns 1000 + number, query_batch
    2000 + number, in every slot; both record what they were called with."""
    world = 1

    def __init__(self, sizes):
        self.sizes, self.calls = sizes, []

    def group_sizes(self, g):
        self.calls.append(("group_sizes", np.array(g)))
        return np.array([self.sizes.get(int(x), 0) for x in g], dtype=np.int64)

    def _answer(self, base, qn, k, want_dist):
        ids = np.repeat((base + qn[:, 0].astype(np.int64))[:, None], k, axis=1)
        return (ids, ids.astype(np.float32) / 8) if want_dist else ids

    def knn_group(self, qn, k, group, *, return_distances=False, **kw):
        self.calls.append(("knn_group", qn[:, 0].astype(int), np.array(group), kw))
        return self._answer(1000, qn, k, return_distances)

    def query_batch(self, qn, qp, k, n_probes, pass_1=None, *, return_distances=False, **kw):
        self.calls.append(("query_batch", qn[:, 0].astype(int), kw))
        return self._answer(2000, qn, k, return_distances)


def _stand_in_ivf(sizes, values=None):
    from tinyknn_amd import IVF
    ivf = IVF("euclidean", 3, None)
    ivf._dev = _StandIn(sizes)
    ivf._prepare = lambda qs: (qs, qs)
    ivf.data = np.zeros((50, 4), np.float32)
    if values is not None:
        ivf.values = values
    return ivf


def test_exact_below_splits_and_merges_in_query_order():
    sizes = {1: 5, 2: 50, 3: 500}
    nq = 9
    qs = np.zeros((nq, 4), np.float32)
    qs[:, 0] = np.arange(nq)
    group = np.array([1, 3, -1, 2, 9, 3, 1, -1, 2])            # 9: an id no row carries (size 0: routed)
    tags = np.arange(nq, dtype=np.uint64) + 1
    exclude = np.arange(nq) + 10
    lo = np.arange(nq) * 2
    ivf = _stand_in_ivf(sizes, values=np.zeros(50, np.int64))
    for T, routed in ((51, [0, 3, 4, 6, 8]), (50, [0, 4, 6]), (6, [0, 4, 6]), (0, []), (10**6, [0, 1, 3, 4, 5, 6, 8])):
        dev = ivf._dev = _StandIn(sizes)
        ids, dist = ivf.query_batch(qs, 3, 2, group=group, exact_below=T, tags=tags, exclude=exclude, between=(lo, None),
                                    return_distances=True)
        other = [i for i in range(nq) if i not in routed]
        want = np.array([(1000 if i in routed else 2000) + i for i in range(nq)])
        np.testing.assert_array_equal(ids, np.repeat(want[:, None], 3, axis=1))
        np.testing.assert_array_equal(dist, ids.astype(np.float32) / 8)
        assert dist.dtype == np.float32
        names = [c[0] for c in dev.calls]
        assert names == ["group_sizes"] + ["knn_group"] * bool(routed) + ["query_batch"] * bool(other), (T, names)
        np.testing.assert_array_equal(dev.calls[0][1], group[group >= 0])      # sizes are asked for grouped queries only
        for c in dev.calls[1:]:
            rows = np.array(routed if c[0] == "knn_group" else other)
            np.testing.assert_array_equal(c[1], rows)
            kw = c[-1]
            np.testing.assert_array_equal(kw["tags"], tags[rows])
            np.testing.assert_array_equal(kw["exclude"], exclude[rows])
            np.testing.assert_array_equal(kw["between"][0], lo[rows].reshape(-1, 1))
            assert kw["between"][1] is None and kw["tags_mode"] == "any" and kw["allowed"] is None
            if c[0] == "knn_group":
                np.testing.assert_array_equal(c[2], group[rows])
                assert "per_group" not in kw
            else:
                np.testing.assert_array_equal(kw["group"], group[rows])
    # ids alone, and a batch without queries
    dev = ivf._dev = _StandIn(sizes)
    got = ivf.query_batch(qs, 2, 1, group=group, exact_below=6)
    np.testing.assert_array_equal(got[:, 0], [1000, 2001, 2002, 2003, 1004, 2005, 1006, 2007, 2008])
    dev = ivf._dev = _StandIn(sizes)
    ids, dist = ivf.query_batch(qs[:0], 2, 1, group=group[:0], exact_below=6, return_distances=True)
    assert ids.shape == dist.shape == (0, 2) and dev.calls == []
    # without exact_below nothing changes: one restricted call, no sizes asked
    dev = ivf._dev = _StandIn(sizes)
    ivf.query_batch(qs, 2, 1, group=group)
    assert [c[0] for c in dev.calls] == ["query_batch"]


def test_exact_below_parts():
    from tinyknn_amd.ivf import exact_below_parts
    routed = np.array([True, False, True, False])
    lo = np.arange(8).reshape(4, 2)
    parts = exact_below_parts(routed, (lo, None))
    assert [(e, list(r)) for e, r, _ in parts] == [(True, [0, 2]), (False, [1, 3])]
    np.testing.assert_array_equal(parts[0][2][0], lo[[0, 2]])
    assert parts[0][2][1] is None and parts[1][2][1] is None
    assert [(e, list(r), b) for e, r, b in exact_below_parts(np.ones(2, bool), None)] == [(True, [0, 1], None)]
    assert [(e, list(r), b) for e, r, b in exact_below_parts(np.zeros(2, bool), None)] == [(False, [0, 1], None)]
    assert exact_below_parts(np.zeros(0, bool), None) == []


# ---- the kernels ------------------------------------------------------------------------------------------------------
def test_kernels_compile_without_scratch_or_spills():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    usage = kernel_usage("group_exact.hip")
    names = " ".join(usage)
    for kernel in ("group_exact_kernel", "group_span_kernel", "stored_bits_kernel"):
        assert kernel in names, names
    forms = [n for n in usage if "group_exact_kernel" in n]
    assert len(forms) == 3 and len(usage) == 5, sorted(usage)          # float32, half and float64 rows
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    for name in forms:
        assert usage[name]["Occupancy"] >= 4, (name, usage[name])       # (four waves a workgroup: one to a SIMD)
    print({n[:60]: (u["VGPRs"], u.get("TotalSGPRs"), u["Occupancy"]) for n, u in usage.items()})


def test_rescoring_and_group_search_share_one_distance_text():
    csrc = os.path.join(ROOT, "tinyknn_amd", "csrc")
    for f in ("rescore.hip", "group_exact.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "sqdist_row.h"' in src and "T sqdist_row(" not in src, f
    assert open(os.path.join(csrc, "sqdist_row.h")).read().count("T sqdist_row(") == 1
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "group_exact.hip" in make and "sqdist_row.h" in make
