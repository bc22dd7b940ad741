"""The exact search inside a query's value range (tk_index_knn_between) without a GPU: the signatures
and the null-index returns of the ABI, what the Python layer refuses before it touches a device, the reference helper
against the restricted exact search's on integer data, the span model against the range formulas on every fixture of
the GPU tests, the split and merge of IVF.query_batch(between=, exact_below=) against a stand-in device index, what
the compiler reports for the kernels, and that the walk has one text."""
import inspect
import os
import re

import numpy as np
import pytest

from between_exact_reference import knn_between_reference, span_model, value_order
from between_exact_shapes import MAX, MIN, all_fixtures, edges, ties, wide_and_narrow
from between_reference import bounds_of, passing
from brute_reference import int_part
from brute_restricted_reference import passes, restricted_k_best
from group_exact_reference import einsum_distances, reference_data, same_bits, stored_mask
from kernel_usage import have_hipcc, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinyknn_amd", "csrc")
NEW = ("tk_index_knn_between", "tk_index_range_sizes", "tk_index_value_rows")


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
    # knn_group's arguments, the ranges moved in front (they are required) and the group among the others
    assert len(_lib.SIGNATURES["tk_index_knn_between"][1]) == len(_lib.SIGNATURES["tk_index_knn_group"][1])
    out = np.zeros(4, dtype=np.int64)
    assert lib.tk_index_knn_between(None, None, 0, 1, None, None, None, None, None, 0, None, None) == -1
    assert lib.tk_index_range_sizes(None, None, 0, None, None) == -1
    assert lib.tk_index_value_rows(None, _lib.ptr(out, _lib._i64p)) == -1


def test_the_signatures_carry_the_keywords():
    from tinyknn_amd import IVF
    from tinyknn_amd.ivf import DeviceIndex
    from tinyknn_amd import multi_gpu
    kw = dict(allowed=None, exclude=None, group=None, tags=None, tags_mode="any", return_distances=False)
    for f in (IVF.knn_between, DeviceIndex.knn_between):
        p = inspect.signature(f).parameters
        assert list(p)[:4] == ["self", list(p)[1], "k", "between"] and f.__kwdefaults__ == kw, f.__qualname__
        assert all(p[name].kind is inspect.Parameter.KEYWORD_ONLY for name in kw), f.__qualname__
        assert "per_group" not in p
    assert list(inspect.signature(DeviceIndex.range_sizes).parameters) == ["self", "between", "nq"]
    assert inspect.signature(DeviceIndex.range_sizes).parameters["nq"].default is None
    assert callable(DeviceIndex.value_rows)
    # the calls that still do not take exact_below
    for f in (IVF.query, DeviceIndex.query_batch, DeviceIndex.query_batch_dev, multi_gpu.ListShardedIndex.query_batch,
              multi_gpu.ReplicaGroup.query_batch):
        assert "exact_below" not in inspect.signature(f).parameters, f.__qualname__


# ---- refusals before any device call -----------------------------------------------------------------------------------
def test_ivf_refuses_before_any_device_call():
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import AllowSet
    ivf = IVF("angular", 4, FastPQ(2))          # (never fitted: nothing reaches the device)
    qs = np.zeros((3, 4), np.float32)
    with pytest.raises(TypeError, match="AllowSet"):
        ivf.knn_between(qs, 1, (0, 1), allowed=object.__new__(AllowSet))
    with pytest.raises(ValueError, match="without values"):
        ivf.knn_between(qs, 1, (0, 1))
    with pytest.raises(TypeError, match="required"):
        ivf.knn_between(qs, 1, None)
    with pytest.raises(ValueError, match="without values"):
        ivf.query_batch(qs, 1, between=(0, 1), exact_below=10)
    with pytest.raises(ValueError, match="needs group= or between="):
        ivf.query_batch(qs, 1, exact_below=10)
    ivf.data = np.zeros((50, 4), np.float32)
    ivf.values = np.zeros((50, 2), np.int64)
    with pytest.raises(ValueError, match="query 1 bounds no column"):
        ivf.knn_between(qs, 1, (np.array([[0, MIN], [MIN, MIN], [MIN, 3]]), np.array([[5, MAX], [MAX, MAX], [MAX, MAX]])))
    with pytest.raises(ValueError, match="query 0 bounds no column"):
        ivf.knn_between(qs, 1, (None, None))
    ivf.values = np.zeros(50, np.float32)
    with pytest.raises(ValueError, match="query 2 bounds no column"):
        ivf.knn_between(qs, 1, (np.array([0.0, np.inf, -np.inf]), np.array([1.0, np.inf, np.inf])))
    with pytest.raises(ValueError, match="tags_mode"):
        ivf.knn_between(qs, 1, (0.0, 1.0), tags=1, tags_mode="some")
    with pytest.raises(ValueError, match="one entry per query"):
        ivf.knn_between(qs, 1, (0.0, 1.0), group=[0, 1])
    with pytest.raises(TypeError):
        ivf.knn_between(qs, 1, 5)
    # exact_below with between= alone: the refusals that were there stay
    with pytest.raises(ValueError, match="per_group"):
        ivf.query_batch(qs, 1, between=(0.0, 1.0), per_group=1, exact_below=10)
    with pytest.raises(TypeError, match="AllowSet"):
        ivf.query_batch(qs, 1, between=(0.0, 1.0), allowed=object.__new__(AllowSet), exact_below=10)
    with pytest.raises(NotImplementedError, match=r"fast=True with exact_below= is not supported"):
        ivf.query_batch(qs, 1, fast=True, between=(0.0, 1.0), exact_below=10)
    with pytest.raises(TypeError, match="exact_below"):
        ivf.query_batch(qs, 1, between=(0.0, 1.0), exact_below=1.5)
    with pytest.raises(ValueError, match="exact_below"):
        ivf.query_batch(qs, 1, between=(0.0, 1.0), exact_below=-1)
    assert ivf._dev is None


def test_a_list_sharded_index_is_refused_before_any_device_call():
    from tinyknn_amd import IVF

    class Sharded:
        world, rank, calls = 2, 0, []

        def __getattr__(self, name):
            raise AssertionError(f"the device index was asked for {name}")
    ivf = IVF("euclidean", 3, None)
    ivf._dev = Sharded()
    ivf.data = np.zeros((50, 4), np.float32)
    ivf.values = np.zeros(50, np.int64)
    ivf._prepare = lambda qs: (qs, qs)
    qs = np.zeros((2, 4), np.float32)
    with pytest.raises(RuntimeError, match="list-sharded"):
        ivf.knn_between(qs, 1, (0, 1))
    with pytest.raises(RuntimeError, match="list-sharded"):
        ivf.query_batch(qs, 1, between=(0, 1), exact_below=10)


def test_device_index_refuses_before_any_device_call():
    from tinyknn_amd.ivf import AllowSet, DeviceIndex
    dev = object.__new__(DeviceIndex)
    dev.d, dev.N, dev.world, dev._f64 = 4, 100, 1, False
    dev._source = None
    dev._value_kind, dev._value_cols = "i", 2
    X = np.zeros((2, 4), np.float32)
    with pytest.raises(TypeError, match="AllowSet"):
        dev.knn_between(X, 1, (0, 1), allowed=object.__new__(AllowSet))
    with pytest.raises(TypeError, match="required"):
        dev.knn_between(X, 1, None)
    with pytest.raises(ValueError, match="query 1 bounds no column"):
        dev.knn_between(X, 1, (np.array([[0, MIN], [MIN, MIN]]), None))
    with pytest.raises(ValueError, match="exclude"):
        dev.knn_between(X, 1, (0, 1), exclude=[0, 100])
    with pytest.raises(ValueError):
        dev.knn_between(X, 1, (0, 1), group=[0, 2**31 - 1])
    with pytest.raises(ValueError):
        dev.knn_between(X, 1, (np.zeros((3, 2), np.int64), None))          # (bounds for another number of queries)
    dev.world = 2
    with pytest.raises(RuntimeError, match="list-sharded"):
        dev.knn_between(X, 1, (0, 1))


def test_ranges_length_and_unbounded_queries():
    from tinyknn_amd.ivf import query_ranges, ranges_length, unbounded_queries
    assert ranges_length((0, None), 1) == 1 and ranges_length((None, None), 3) == 1
    assert ranges_length((np.zeros(7), 1), 1) == 7 and ranges_length((None, np.zeros((5, 2))), 2) == 5
    assert ranges_length((np.zeros(2), None), 2) == 1           # (one entry per column, for every query)
    with pytest.raises(TypeError):
        ranges_length(3, 1)
    keys = query_ranges((np.array([[0.0, -np.inf], [-np.inf, -np.inf], [-np.inf, -np.inf]]),
                         np.array([[np.inf, np.inf], [np.inf, np.inf], [np.inf, -np.inf]])), 3, 2, "f")
    np.testing.assert_array_equal(unbounded_queries(keys), [False, True, False])
    keys = query_ranges((np.array([MIN, MIN, 1e30]), np.array([MAX, 5, np.inf])), 3, 1, "i")
    np.testing.assert_array_equal(unbounded_queries(keys), [True, False, False])       # (1e30 <= v: empty, not open)


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
    values = rng.randint(0, 40, size=(n, 2)).astype(np.int64)
    values[[30, 40, 50]] = [[3, 7], [20, 7], [3, 7]]
    lo = np.stack([rng.randint(0, 30, size=nq), np.full(nq, MIN)], axis=1).astype(np.int64)
    hi = np.stack([lo[:, 0] + rng.randint(0, 15, size=nq), np.full(nq, MAX)], axis=1).astype(np.int64)
    lo[0], hi[0] = (0, 7), (10, 7)                              # rows 30 and 50 pass, 40 does not
    lo[5], hi[5] = (9, MIN), (3, MAX)                           # lo > hi
    groups = rng.randint(0, 3, size=n).astype(np.int32)
    group = rng.randint(-1, 3, size=nq).astype(np.int32)
    group[0] = groups[30] = groups[50] = 1
    stored = stored_mask([np.arange(0, 300), np.array([-1, 700]), np.arange(320, 600)], n)
    mask = rng.rand(n) < 0.8
    mask[[30, 40, 50]] = True
    exclude = rng.randint(-1, n, size=nq)
    exclude[0] = 30                                             # the lower of the two passing twins is excluded
    part = int_part(X, Y)
    r = dict(allowed=mask, exclude=exclude, group=group, groups=groups)
    for store, data in ((None, Y), ("float16", Y), (None, Y.astype(np.float64))):
        ref = reference_data(data, store)
        for k in (1, 10, 300):
            ids, dist = knn_between_reference(oracle, X, ref, k, (lo, hi), values, stored=stored, **r)
            assert dist.dtype == (np.float64 if data.dtype == np.float64 else np.float32)
            for i in range(nq):
                ok = passes(i, n, between=(lo, hi), values=values, **r) & stored
                np.testing.assert_array_equal(ids[i], restricted_k_best(part[i], ok, k))
                live = ids[i] >= 0
                np.testing.assert_array_equal(dist[i][live], part[i][ids[i][live]])
                assert np.isposinf(dist[i][~live]).all()
            assert ids[0][0] == 50 and (ids[5] == -1).all()
            assert same_bits(dist, einsum_distances(X, ref, ids))


def _column_alone(values, between, i, c):
    """the rows that query i's bounds on column c alone pass"""
    v = np.asarray(values)
    v = v.reshape(len(v), -1)
    lo, hi = bounds_of(between, i)
    lo_c = None if lo is None else np.asarray(lo).reshape(-1)[c]
    hi_c = None if hi is None else np.asarray(hi).reshape(-1)[c]
    return passing(v[:, c], lo_c, hi_c)


def test_span_model_is_the_count_of_the_chosen_column_on_every_fixture():
    from tinyknn_amd.ivf import query_ranges, unbounded_queries, value_keys, value_kind
    fixtures = all_fixtures()
    assert len({f["name"] for f in fixtures}) == len(fixtures) >= 17
    open_queries = 0
    for f in fixtures:
        values, between, nq = f["values"], f["between"], f["nq"]
        v = np.asarray(values).reshape(len(values), -1)
        n, C = v.shape
        length, col = span_model(values, between)
        assert length.shape == col.shape == (nq,), f["name"]
        keys = query_ranges(between, nq, C, value_kind(v.dtype))
        # the Python layer's notion of a query that bounds nothing is the model's
        np.testing.assert_array_equal(col < 0, unbounded_queries(keys), err_msg=f["name"])
        row_keys = value_keys(values, n, "values").reshape(n, C)
        for i in range(nq):
            everything = passing(values, *bounds_of(between, i))
            if col[i] < 0:
                assert length[i] == n and everything.all(), (f["name"], i)
                open_queries += 1
                continue
            per_column = [int(_column_alone(values, between, i, c).sum()) for c in range(C)]
            assert length[i] == per_column[col[i]], (f["name"], i, length[i], per_column)
            assert length[i] >= everything.sum(), (f["name"], i)
            # the shortest among the columns the query bounds, ties to the lowest
            bounded = [c for c in range(C) if keys[i, c, 0] != MIN or keys[i, c, 1] != MAX]
            assert col[i] == min(bounded, key=lambda c: (per_column[c], c)), (f["name"], i, per_column, bounded)
            # ... and what the device's two bounds give on the keys in key order
            sk = np.sort(row_keys[:, col[i]])
            b, e = np.searchsorted(sk, keys[i, col[i], 0], "left"), np.searchsorted(sk, keys[i, col[i], 1], "right")
            assert max(0, e - b) == length[i], (f["name"], i)
    assert open_queries >= 3
    # the fixtures say what they are made to say
    f, lengths = edges()
    np.testing.assert_array_equal(span_model(f["values"], f["between"])[0], lengths)
    for narrow in (0, 1):
        f = wide_and_narrow(narrow)
        assert (span_model(f["values"], f["between"])[1] == narrow).all()
    f = ties()
    assert (span_model(f["values"], f["between"])[1] == 1).all()
    order = value_order(f["values"], 1)
    v = f["values"][order, 1]
    assert (np.diff(v) >= 0).all() and (np.diff(order)[np.diff(v) == 0] > 0).all()


# ---- exact_below against a stand-in device index -----------------------------------------------------------------------
class _StandIn:
    """Answers by marker: a query's first coordinate is its number; knn_between returns 3000 + number, knn_group
    1000 + number, query_batch 2000 + number, in every slot; all record what they were called with.  range_sizes
    answers from the lower bound alone: the length of query i's span is lengths[lo]."""
    world = 1

    def __init__(self, lengths, n=50):
        self.lengths, self.n, self.calls = lengths, n, []

    def range_sizes(self, between, nq=None):
        lo = np.asarray(between[0])
        self.calls.append(("range_sizes", lo.copy(), nq))
        assert lo.ndim == 2 and len(lo) == nq
        return (np.array([self.lengths[int(x)] for x in lo[:, 0]], dtype=np.int64), np.zeros(len(lo), np.int32))

    def group_sizes(self, g):
        self.calls.append(("group_sizes", np.array(g)))
        return np.full(len(g), 5, dtype=np.int64)

    def _answer(self, base, qn, k, want_dist):
        ids = np.repeat((base + qn[:, 0].astype(np.int64))[:, None], k, axis=1)
        return (ids, ids.astype(np.float32) / 8) if want_dist else ids

    def knn_between(self, qn, k, between, *, return_distances=False, **kw):
        self.calls.append(("knn_between", qn[:, 0].astype(int), between, kw))
        return self._answer(3000, qn, k, return_distances)

    def knn_group(self, qn, k, group, *, return_distances=False, **kw):
        self.calls.append(("knn_group", qn[:, 0].astype(int), np.array(group), kw))
        return self._answer(1000, qn, k, return_distances)

    def query_batch(self, qn, qp, k, n_probes, pass_1=None, *, return_distances=False, **kw):
        self.calls.append(("query_batch", qn[:, 0].astype(int), kw))
        return self._answer(2000, qn, k, return_distances)


def _stand_in_ivf(lengths):
    from tinyknn_amd import IVF
    ivf = IVF("euclidean", 3, None)
    ivf._dev = _StandIn(lengths)
    ivf._prepare = lambda qs: (qs, qs)
    ivf.data = np.zeros((50, 4), np.float32)
    ivf.values = np.zeros(50, np.int64)
    return ivf


def test_exact_below_with_between_alone_splits_and_merges_in_query_order():
    lengths = {1: 5, 2: 50, 3: 500}
    nq = 9
    qs = np.zeros((nq, 4), np.float32)
    qs[:, 0] = np.arange(nq)
    lo = np.array([1, 3, MIN, 2, 1, 3, 1, MIN, 2], dtype=np.int64)      # MIN with hi MAX: a query that bounds nothing
    hi = np.full(nq, MAX, dtype=np.int64)
    bounded = lo != MIN
    tags = np.arange(nq, dtype=np.uint64) + 1
    exclude = np.arange(nq) + 10
    ivf = _stand_in_ivf(lengths)
    for T, routed in ((51, [0, 3, 4, 6, 8]), (50, [0, 4, 6]), (6, [0, 4, 6]), (5, []), (0, []),
                      (10**6, [0, 1, 3, 4, 5, 6, 8])):
        dev = ivf._dev = _StandIn(lengths)
        ids, dist = ivf.query_batch(qs, 3, 2, between=(lo, hi), exact_below=T, tags=tags, exclude=exclude,
                                    return_distances=True)
        other = [i for i in range(nq) if i not in routed]
        want = np.array([(3000 if i in routed else 2000) + i for i in range(nq)])
        np.testing.assert_array_equal(ids, np.repeat(want[:, None], 3, axis=1))
        np.testing.assert_array_equal(dist, ids.astype(np.float32) / 8)
        assert dist.dtype == np.float32
        names = [c[0] for c in dev.calls]
        assert names == ["range_sizes"] + ["knn_between"] * bool(routed) + ["query_batch"] * bool(other), (T, names)
        # lengths are asked for the queries that bound a column only: the others are never routed, whatever T
        np.testing.assert_array_equal(dev.calls[0][1][:, 0], lo[bounded])
        assert dev.calls[0][2] == bounded.sum()
        for c in dev.calls[1:]:
            rows = np.array(routed if c[0] == "knn_between" else other)
            np.testing.assert_array_equal(c[1], rows)
            kw = c[-1]
            np.testing.assert_array_equal(kw["tags"], tags[rows])
            np.testing.assert_array_equal(kw["exclude"], exclude[rows])
            assert kw["tags_mode"] == "any" and kw["allowed"] is None
            btw = c[2] if c[0] == "knn_between" else kw["between"]
            np.testing.assert_array_equal(btw[0], lo[rows].reshape(-1, 1))
            np.testing.assert_array_equal(btw[1], hi[rows].reshape(-1, 1))
            if c[0] == "knn_between":
                assert kw["group"] is None and "between" not in kw and "per_group" not in kw
            else:
                assert kw["group"] is None
    # ids alone, and a batch without queries
    dev = ivf._dev = _StandIn(lengths)
    got = ivf.query_batch(qs, 2, 1, between=(lo, hi), exact_below=6)
    np.testing.assert_array_equal(got[:, 0], [3000, 2001, 2002, 2003, 3004, 2005, 3006, 2007, 2008])
    dev = ivf._dev = _StandIn(lengths)
    ids, dist = ivf.query_batch(qs[:0], 2, 1, between=(lo[:0], hi[:0]), exact_below=6, return_distances=True)
    assert ids.shape == dist.shape == (0, 2) and dev.calls == []
    # no query bounds a column: nothing is asked, one restricted call
    dev = ivf._dev = _StandIn(lengths)
    ivf.query_batch(qs[:3], 2, 1, between=(None, None), exact_below=10**6)
    assert [c[0] for c in dev.calls] == ["query_batch"]
    # without exact_below nothing changes: one restricted call, no lengths asked
    dev = ivf._dev = _StandIn(lengths)
    ivf.query_batch(qs, 2, 1, between=(lo, hi))
    assert [c[0] for c in dev.calls] == ["query_batch"]


def test_exact_below_with_group_and_between_still_routes_by_group_size():
    nq = 6
    qs = np.zeros((nq, 4), np.float32)
    qs[:, 0] = np.arange(nq)
    lo = np.array([1, 2, 3, 1, 2, 3], dtype=np.int64)
    group = np.array([4, -1, 4, 7, -1, 7])
    ivf = _stand_in_ivf({1: 5, 2: 50, 3: 500})
    dev = ivf._dev
    ids = ivf.query_batch(qs, 2, 1, group=group, between=(lo, None), exact_below=6)
    names = [c[0] for c in dev.calls]
    assert names == ["group_sizes", "knn_group", "query_batch"] and "range_sizes" not in names
    np.testing.assert_array_equal(ids[:, 0], [1000, 2001, 1002, 1003, 2004, 1005])
    np.testing.assert_array_equal(dev.calls[1][3]["between"][0], lo[group >= 0].reshape(-1, 1))


# ---- the kernels ------------------------------------------------------------------------------------------------------
def test_kernels_compile_without_scratch_or_spills():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    usage = kernel_usage("value_exact.hip")
    forms = [n for n in usage if "range_exact_kernel" in n]
    spans = [n for n in usage if "range_span_kernel" in n]
    assert len(forms) == 3 and len(spans) == 1 and len(usage) == 4, sorted(usage)      # float32, half, float64 rows
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    for name in forms:
        assert usage[name]["Occupancy"] >= 4, (name, usage[name])       # (four waves a workgroup: one to a SIMD)
    print({n[:60]: (u["VGPRs"], u.get("TotalSGPRs"), u["Occupancy"]) for n, u in usage.items()})


def test_the_walk_has_one_text():
    header = open(os.path.join(CSRC, "span_exact.h")).read()
    assert header.count("void span_exact_body(") == 1 and header.count("t0 += GX_TILE") == 1
    assert header.count("struct GxKey<float>") == 1 and header.count("gx_lds_bytes(int d") == 1
    assert "#define GX_TILE 256" in header and "#define GX_CAP 2048" in header
    for f, kernel, form in (("group_exact.hip", "group_exact_kernel", "false"), ("value_exact.hip", "range_exact_kernel", "true")):
        src = open(os.path.join(CSRC, f)).read()
        assert '#include "span_exact.h"' in src, f
        # neither file defines the tile loop, the cut or the key map itself
        for text in ("GX_TILE)", "atomicAdd", "__syncthreads", "struct GxKey", "T sqdist_row(", "gx_lds_bytes(int"):
            assert text not in src, (f, text)
        assert src.count(f"span_exact_body<T, TY, {form}>(") == 1 and src.count("span_exact_body<") == 1, f
        assert src.count(f"void {kernel}(") == 1, f
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "value_exact.hip" in make and "value_rows.hip" in make and "span_exact.h" in make
    # the library's sort is instantiated in value_rows.hip, not beside our kernels
    assert "rocprim" not in open(os.path.join(CSRC, "value_exact.hip")).read()
    assert "radix_sort_pairs" in open(os.path.join(CSRC, "value_rows.hip")).read()
    # one stored-row map for both entry points, its message naming the caller
    internal = open(os.path.join(CSRC, "api_internal.h")).read()
    assert "int stored_bits_ensure(tk_index *ix, const char *call);" in internal
    assert 'stored_bits_ensure(ix, "tk_index_knn_between")' in open(os.path.join(CSRC, "value_exact.hip")).read()
    assert 'stored_bits_ensure(ix, "tk_index_knn_group")' in open(os.path.join(CSRC, "group_exact.hip")).read()
