"""Value ranges without a GPU: the key map (tinyknn_amd.ivf.value_keys / query_ranges) against the formula on the
original values (tests/between_reference.py::passing); the Python layer's validation, add(values=) / update(values=)
bookkeeping and persistence; the ABI's declarations; the equivalence the device relies on (guarded `insert` == the empty
value for every row outside the ranges); and, on the reference alone, the census of what the fuzz cases of
tests/between_shapes.py hold.  (tk_index_create needs a GPU, so the ABI's refusals are in tests/test_between_gpu.py.)"""
import collections
import os
import pickle
import re
import sys
import time
import weakref

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import between_shapes as bs  # noqa: E402
import restricted_shapes as rs  # noqa: E402
from allowed_reference import guarded_batch, replay_blocks  # noqa: E402
from between_reference import bounds_of, passing, ranged_batch  # noqa: E402
from conftest import golden, split_lists  # noqa: E402
from tinyknn_amd.ivf import query_ranges, value_keys, value_kind  # noqa: E402

KEYS = ("probes", "heap_idx", "heap_val")
INT64_MIN, INT64_MAX = bs.INT64_MIN, bs.INT64_MAX


# ---- the key map ----

def _float_samples(dtype):
    rng = np.random.default_rng(1)
    info = np.finfo(dtype)
    edge = np.array([-np.inf, info.min, -1.0, -info.tiny, -info.smallest_subnormal, 0.0, info.smallest_subnormal,
                     info.tiny, np.nextafter(dtype(1), dtype(0)), 1.0, np.nextafter(dtype(1), dtype(2)), info.max,
                     np.inf], dtype=dtype)
    bits = rng.integers(0, 2**(8 * np.dtype(dtype).itemsize), 4000, dtype=np.uint64)
    rand = bits.astype({2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]).view(dtype)
    a = np.concatenate([edge, rand[~np.isnan(rand)]])
    return np.unique(a)                     # sorted, distinct (-0.0 and +0.0 are one value)


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
def test_float_keys_are_strictly_monotone(dtype):
    a = _float_samples(dtype)
    assert len(a) > 3000 and a[0] == -np.inf and a[-1] == np.inf
    k = value_keys(a, len(a), "t")
    assert k.dtype == np.int64 and (np.diff(k.astype(object)) > 0).all()
    assert INT64_MIN < k[0] and k[-1] < INT64_MAX           # the unbounded extremes lie outside every value's key
    # -0.0 and +0.0 are one key; the widening is exact, so a float16 and the float64 of the same value share a key
    z = value_keys(np.array([-0.0, 0.0], dtype=dtype), 2, "t")
    assert z[0] == z[1] == 0
    np.testing.assert_array_equal(k, value_keys(a.astype(np.float64), len(a), "t"))


@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int32, np.uint32, np.int64, np.uint64])
def test_integer_keys_are_the_values(dtype):
    info = np.iinfo(dtype)
    top = min(info.max, INT64_MAX)
    a = np.unique(np.array([info.min, info.min + 1, 0, 1, top - 1, top] +
                           list(np.random.default_rng(2).integers(info.min, top, 500, dtype=np.int64 if info.min else np.uint64)),
                           dtype=dtype))
    k = value_keys(a, len(a), "t")
    assert k.dtype == np.int64 and [int(x) for x in k] == [int(x) for x in a]
    assert (np.diff(k.astype(object)) > 0).all()


def test_key_map_refusals():
    with pytest.raises(ValueError, match="NaN"):
        value_keys(np.array([0.0, np.nan]), 2, "t")
    with pytest.raises(ValueError, match="NaN"):
        value_keys(np.array([[0.0, 1.0], [np.nan, 2.0]], dtype=np.float16), 2, "t")
    with pytest.raises(ValueError, match="uint64"):
        value_keys(np.array([0, 2**63], dtype=np.uint64), 2, "t")
    value_keys(np.array([0, 2**63 - 1], dtype=np.uint64), 2, "t")
    with pytest.raises(ValueError):
        value_keys(np.zeros(3), 4, "t")                     # another length
    with pytest.raises(ValueError):
        value_keys(np.zeros((3, 5)), 3, "t")                # five columns
    with pytest.raises(ValueError):
        value_keys(np.zeros((3, 0)), 3, "t")
    for bad in (np.zeros(3, dtype=bool), np.array(["a", "b", "c"]), np.zeros((3, 1, 1)), 3.0, np.zeros(3, dtype=complex),
                np.array([1, None, 2], dtype=object)):
        with pytest.raises(TypeError):
            value_keys(bad, 3, "t")
    assert value_kind(np.float16) == value_kind(np.float64) == "f" and value_kind(np.uint8) == value_kind(np.int64) == "i"


def test_integer_columns_ceil_and_floor_floating_bounds():
    r = query_ranges((np.array([0.5, -0.5, 2.0, -np.inf, 1e30, np.inf]), np.array([2.5, -0.5, 2.0, np.inf, 1e30, 3.0])),
                     6, 1, "i")[:, 0]
    assert r[0].tolist() == [1, 2]
    assert r[1].tolist() == [0, -1]                         # ceil(-0.5) = 0 > floor(-0.5) = -1: no integer between
    assert r[2].tolist() == [2, 2]
    assert r[3].tolist() == [INT64_MIN, INT64_MAX]          # +-inf: unbounded
    assert r[4][0] > r[4][1] and r[5][0] > r[5][1]          # lo above every int64: no row passes
    r = query_ranges((None, -1e30), 3, 2, "i")
    assert (r[:, :, 0] > r[:, :, 1]).all()                  # hi below every int64
    r = query_ranges((-1e30, 1e30), 3, 2, "i")
    assert (r[:, :, 0] == INT64_MIN).all() and (r[:, :, 1] == INT64_MAX).all()
    # integer bounds on integer columns are themselves; on floating columns they must be exact in float64
    assert query_ranges((INT64_MIN + 1, INT64_MAX - 1), 1, 1, "i")[0, 0].tolist() == [INT64_MIN + 1, INT64_MAX - 1]
    assert query_ranges((3, 2**53 + 2), 1, 1, "f")[0, 0].tolist() == value_keys(np.array([3.0, 2.0**53 + 2]), 2, "t").tolist()
    with pytest.raises(ValueError, match="exactly representable"):
        query_ranges((0, 2**53 + 1), 1, 1, "f")
    with pytest.raises(ValueError, match="exactly representable"):
        query_ranges((np.array([0, -2**53 - 1]), None), 2, 1, "f")
    with pytest.raises(ValueError):
        query_ranges((np.array([2**63], dtype=np.uint64), None), 1, 1, "i")


def test_query_ranges_shapes_and_refusals():
    none = query_ranges((None, None), 4, 3, "f")
    assert none.shape == (4, 3, 2) and none.dtype == np.int64 and none.flags.c_contiguous
    assert (none[:, :, 0] == INT64_MIN).all() and (none[:, :, 1] == INT64_MAX).all()
    one = float(value_keys(np.array([1.0]), 1, "t")[0])
    both = query_ranges((-np.inf, np.inf), 4, 3, "f")       # the ends that admit everything are unbounded ends
    np.testing.assert_array_equal(both, none)
    r = query_ranges((np.inf, -np.inf), 1, 1, "f")[0, 0]    # ... and the ends that admit only themselves are keys
    assert r.tolist() == value_keys(np.array([np.inf, -np.inf]), 2, "t").tolist()
    r = query_ranges((1.0, None), 4, 3, "f")                # a scalar: every query, every column
    assert (r[:, :, 0] == one).all() and (r[:, :, 1] == INT64_MAX).all()
    r = query_ranges((np.arange(4), np.arange(4) + 1), 4, 1, "i")       # (nq,) for one column
    assert r[:, 0, 0].tolist() == [0, 1, 2, 3] and r[:, 0, 1].tolist() == [1, 2, 3, 4]
    r = query_ranges((np.arange(12).reshape(4, 3), None), 4, 3, "i")    # (nq, C)
    assert r[:, :, 0].tolist() == np.arange(12).reshape(4, 3).tolist()
    r = query_ranges(([7, 8, 9], None), 4, 3, "i")          # (C,): every query, where nq != C
    assert (r[:, :, 0] == [7, 8, 9]).all()
    with pytest.raises(ValueError, match="per query or"):
        query_ranges(([7, 8, 9], None), 3, 3, "i")          # nq == C: ambiguous
    query_ranges((np.zeros((3, 3)), None), 3, 3, "i")
    for bad in ((np.arange(4), None), (np.zeros((4, 2)), None), (np.zeros((3, 3)), None), (None, np.zeros((1, 4, 3)))):
        with pytest.raises(ValueError):
            query_ranges(bad, 4, 3, "i")
    with pytest.raises(ValueError):
        query_ranges((np.arange(3), None), 4, 1, "i")
    with pytest.raises(ValueError, match="NaN"):
        query_ranges((np.nan, None), 4, 1, "f")
    with pytest.raises(ValueError, match="NaN"):
        query_ranges((None, np.array([0, np.nan, 0, 0])), 4, 1, "i")
    for bad in (3, None, (1, 2, 3), "ab", np.zeros((2, 4)), (None,)):
        with pytest.raises(TypeError):
            query_ranges(bad, 4, 1, "i")
    for bad in (("a", None), (True, None), (None, np.zeros(4, dtype=bool)), (None, [None] * 4), (1j, None)):
        with pytest.raises(TypeError):
            query_ranges(bad, 4, 1, "i")


def _fixture(oracle, tag):
    g = golden(f"g6_ivf_{tag}.npz")
    codes, ids = split_lists(g)
    R = g["R"] if "R" in g else None
    ox = oracle.OracleIndex(g["pq_centers"], 2, R, float(g["sqrt_n_blocks"]), g["active_centers"],
                            g["center_codes"], codes, g["list_sizes"], ids, g["data"])
    return ox, np.ascontiguousarray(g["qn"]), ids, len(g["data"])


def _key_mask(values, lo, hi, i):
    """the rows query i passes by the int64 KEYS: what the device computes"""
    v = np.asarray(values)
    keys = value_keys(v, len(v), "t").reshape(len(v), -1)
    r = query_ranges((lo, hi), len(lo), keys.shape[1], value_kind(v.dtype))
    return ((keys >= r[i, :, 0]) & (keys <= r[i, :, 1])).all(axis=1)


def test_keys_give_the_mask_of_the_original_values(oracle):
    """every assignment x every range kind: the formula on the original values (Python's exact comparisons) and the
    int64 compare on the keys pass the same rows; the kinds do what their names say"""
    _, qn, ids, N = _fixture(oracle, "an100")
    seen = collections.Counter()
    for a, (name, values) in enumerate(bs.assignments(ids, N, 3).items()):
        lo, hi, kinds = bs.ranges(values, 64, 20 + a)
        assert set(kinds) == set(bs.RANGE_KINDS)
        for i, kind in enumerate(kinds):
            want = passing(values, *bounds_of((lo, hi), i))
            np.testing.assert_array_equal(_key_mask(values, lo, hi, i), want, err_msg=f"{name} {kind} {i}")
            n = int(want.sum())
            if kind == "empty":
                assert n == 0
            if kind == "unbounded":
                assert n == N
            if kind in ("point", "stored"):                 # inclusive on both ends: the rows AT the bounds pass
                v0 = np.asarray(values).reshape(N, -1)[:, 0]
                assert (want & (v0 == lo[i, 0])).any() or name == "two", (name, kind)
                assert n > 0 or name == "two"
            seen[(name, kind, n > 0, n < N)] += 1
    assert all(seen[(name, "two_sided", True, True)] for name in bs.ASSIGNMENTS), seen
    # float32 values against float64 bounds one float64-ulp from a stored value: the widening keeps them apart
    v = np.array([0.1, 0.2, 0.3], dtype=np.float32)
    x = np.float64(v[1])
    lo = np.array([[np.nextafter(x, 1.0)], [x], [np.nextafter(x, 0.0)]])
    hi = np.full((3, 1), np.inf)
    assert [_key_mask(v, lo, hi, i).tolist() for i in range(3)] == [[False, False, True], [False, True, True]] * 1 + \
        [[False, True, True]]
    # the int32 ties take float bounds with a fraction: (a, b], not [a, b]
    t = np.arange(6, dtype=np.int32)
    assert _key_mask(t, np.array([[1.5]]), np.array([[3.5]]), 0).tolist() == [False, False, True, True, False, False]
    assert passing(t, 1.5, 3.5).tolist() == [False, False, True, True, False, False]
    # integers no float64 holds, against float and integer bounds
    big = np.array([2**53, 2**53 + 1, 2**53 + 2], dtype=np.int64)
    for b in (float(2**53), float(2**53 + 2)):
        np.testing.assert_array_equal(_key_mask(big, np.array([[b]]), np.array([[np.inf]]), 0), passing(big, b, None))
    assert passing(big, float(2**53), float(2**53)).tolist() == [True, False, False]


@pytest.mark.parametrize("tag", ["an100b2", "eu20"])
def test_helper_unbounded_is_the_unrestricted_reference_and_a_range_its_set(oracle, tag):
    ox, qn, ids, N = _fixture(oracle, tag)
    values = bs.assignments(ids, N, 1)["two"]
    want = guarded_batch(oracle, ox, qn, 10, 5, debug=True)
    for between in ((None, None), (np.full((len(qn), 2), -np.inf), np.full((len(qn), 2), np.inf))):
        got = ranged_batch(oracle, ox, qn, between, values, 10, 5, debug=True)
        np.testing.assert_array_equal(got[0], want[0])
        for key in KEYS:
            np.testing.assert_array_equal(got[1][key], want[1][key])
    lo, hi = np.tile([0.25, 1.0], (len(qn), 1)), np.tile([0.75, 3.0], (len(qn), 1))
    allowed = (values[:, 0] >= 0.25) & (values[:, 0] <= 0.75) & (values[:, 1] >= 1) & (values[:, 1] <= 3)
    got = ranged_batch(oracle, ox, qn, (lo, hi), values, 10, 5)
    np.testing.assert_array_equal(got, guarded_batch(oracle, ox, qn, 10, 5, allowed=allowed))
    assert (got != want[0]).any() and allowed[got[got != -1]].all()


# ---- the Python layer ----

def _built(kp=1, n=2000, d=40, clusters=20, seed=0):
    from tinyknn_amd import IVF, FastPQ
    X = np.random.RandomState(seed).randn(n + 300, d).astype(np.float32)
    ivf = IVF("angular", clusters, FastPQ(2))
    np.random.seed(seed)
    ivf.fit(X[:1500])
    ivf.build(X[:n], n_probes=kp, device=False)
    return ivf, X[n:]


def test_set_values_validation():
    ivf, _ = _built()
    N = len(ivf.data)
    assert ivf.values is None and "values" not in vars(ivf)
    for bad in (np.zeros(N, dtype=bool), "price", 3, np.zeros((N, 1, 1)), np.zeros(N, dtype=complex)):
        with pytest.raises(TypeError):
            ivf.set_values(bad)
    nan = np.zeros(N)
    nan[5] = np.nan
    for bad in (np.zeros(N - 1), np.zeros((N + 1, 2)), np.zeros((N, 5)), nan, np.full(N, 2**63, dtype=np.uint64)):
        with pytest.raises(ValueError):
            ivf.set_values(bad)
    assert ivf.values is None
    v = np.arange(N, dtype=np.float16)
    assert ivf.set_values(v) is ivf
    assert ivf.values.dtype == np.float16 and np.array_equal(ivf.values, v)         # the caller's dtype
    v[1] = 77                                               # the index keeps its own copy
    assert ivf.values[1] == 1
    ivf.set_values(np.arange(2 * N, dtype=np.int64).reshape(N, 2))
    assert ivf.values.shape == (N, 2) and ivf.values.dtype == np.int64
    ivf.set_values([[0.5, 1, 2, 3]] * N)
    assert ivf.values.shape == (N, 4) and ivf.values.dtype == np.float64
    ivf.set_values(None)
    assert ivf.values is None and "values" not in vars(ivf)


def test_add_and_update_values_bookkeeping():
    ivf, more = _built()
    N = len(ivf.data)
    with pytest.raises(ValueError, match="without values"):
        ivf.add(more[:10], values=np.zeros(10))
    with pytest.raises(ValueError, match="without values"):
        ivf.update(np.arange(3), more[:3], values=np.zeros(3))
    assert len(ivf.data) == N
    v = np.stack([np.arange(N) * 0.5, np.arange(N) % 7], axis=1).astype(np.float32)
    ivf.set_values(v)
    ids_before = [np.array(x, copy=True) for x in ivf.ids[:len(ivf.active_centers)]]
    with pytest.raises(ValueError, match="values"):
        ivf.add(more[:10])
    for bad in (np.zeros((9, 2)), np.zeros(10), np.zeros((10, 3)), np.full((10, 2), np.nan), np.zeros((10, 2), dtype=np.int64)):
        with pytest.raises(ValueError):
            ivf.add(more[:10], values=bad)
    with pytest.raises(TypeError):
        ivf.add(more[:10], values=np.zeros((10, 2), dtype=bool))
    with pytest.raises(ValueError):
        ivf.update(np.arange(3), more[:3], values=np.zeros(3))
    assert len(ivf.data) == N and np.array_equal(ivf.values, v)        # refused before anything changed
    for a, b in zip(ids_before, ivf.ids):
        np.testing.assert_array_equal(a, b)
    new = np.stack([np.arange(10) + 0.25, np.ones(10)], axis=1)         # float64 for a float32 index: the index's dtype
    ivf.add(more[:10], values=new)
    assert len(ivf.data) == N + 10 and ivf.values.dtype == np.float32 and ivf.values.shape == (N + 10, 2)
    np.testing.assert_array_equal(ivf.values, np.concatenate([v, new.astype(np.float32)]))
    # update: without values= the rows keep theirs; with it, those rows change
    before = ivf.values.copy()
    ivf.update(np.array([3, N + 2]), more[20:22])
    np.testing.assert_array_equal(ivf.values, before)
    ivf.update(np.array([3, N + 2]), more[22:24], values=np.array([[-1.0, -2.0], [np.inf, 0.0]]))
    assert ivf.values[3].tolist() == [-1, -2] and ivf.values[N + 2].tolist() == [np.inf, 0]
    rest = np.ones(N + 10, dtype=bool)
    rest[[3, N + 2]] = False
    np.testing.assert_array_equal(ivf.values[rest], before[rest])
    # remove leaves values alone: ids are stable, a removed row keeps its entry
    after = ivf.values.copy()
    ivf.remove(np.array([3, 5]))
    np.testing.assert_array_equal(ivf.values, after)
    # an index with tags and values: add needs both
    ivf.set_tags(np.zeros(N + 10, dtype=np.uint64))
    with pytest.raises(ValueError, match="values"):
        ivf.add(more[:5], tags=np.zeros(5, dtype=np.uint64))
    with pytest.raises(ValueError, match="tags"):
        ivf.add(more[:5], values=np.zeros((5, 2)))
    ivf.add(more[:5], tags=np.ones(5, dtype=np.uint64), values=np.full((5, 2), 6.0))
    assert len(ivf.tags) == len(ivf.values) == N + 15 and ivf.values[-1].tolist() == [6, 6]
    # integer values that do not fit the index's dtype are refused
    ints, more = _built()
    ints.set_values(np.arange(N, dtype=np.int8) % 100)
    with pytest.raises(ValueError, match="fit"):
        ints.add(more[:2], values=np.array([1, 300]))
    ints.add(more[:2], values=np.array([1, 100]))
    assert ints.values.dtype == np.int8 and ints.values[-1] == 100
    # an index without values: add as before; a new build drops the values of the rows before
    plain, more = _built()
    plain.add(more[:10])
    assert plain.values is None and len(plain.data) == N + 10
    ivf.build(np.asarray(ivf.data[:500]), n_probes=1, device=False)
    assert ivf.values is None


def test_save_load_and_pickle_carry_values(tmp_path, monkeypatch):
    from tinyknn_amd import IVF
    stamp = time.localtime(86400 * 365 * 30)
    monkeypatch.setattr(time, "localtime", lambda *a: stamp)     # (the archive's member times: equal for every file)
    ivf, _ = _built(kp=2)
    N = len(ivf.data)
    ivf.save(tmp_path / "never")
    never = open(tmp_path / "never.npz", "rb").read()
    assert "values" not in np.load(tmp_path / "never.npz").files and IVF.load(tmp_path / "never").values is None
    state_never = set(ivf.__getstate__())
    for v in (np.arange(N, dtype=np.float16), np.arange(3 * N, dtype=np.int64).reshape(N, 3) - 2**62,
              bs.FLOAT_POOL[np.arange(N) % len(bs.FLOAT_POOL)]):
        ivf.set_values(v)
        ivf.save(tmp_path / "with")
        back = IVF.load(tmp_path / "with")
        assert back.values.dtype == v.dtype and back.values.shape == v.shape
        assert back.values.tobytes() == v.tobytes()             # (-0.0 stays -0.0 on the host)
        twin = pickle.loads(pickle.dumps(ivf))
        assert twin.values.dtype == v.dtype and twin.values.tobytes() == v.tobytes()
    ivf.set_values(None)
    ivf.save(tmp_path / "cleared")
    assert open(tmp_path / "cleared.npz", "rb").read() == never
    assert set(ivf.__getstate__()) == state_never and pickle.loads(pickle.dumps(ivf)).values is None


N0, D, DQ = 40, 6, 8


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"{name}: a refused call must not reach the library")


@pytest.fixture
def bare(monkeypatch):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    dev = DeviceIndex.__new__(DeviceIndex)
    dev._h, dev.d, dev.dq, dev.dpb, dev.n_lists, dev.N = 0x10, D, DQ, 2, 3, N0
    dev.angular, dev._R, dev._f64, dev.rank, dev.world = False, None, False, 0, 1
    dev._source = None
    dev._streams, dev._live_streams, dev._live_allows = {}, weakref.WeakSet(), weakref.WeakSet()
    yield dev
    dev._h = None


def test_query_refusals_decided_on_the_host(bare):
    from tinyknn_amd import IVF
    qn, qp = np.zeros((5, D), np.float32), np.zeros((5, DQ), np.float32)
    bare._value_kind, bare._value_cols = "f", 2
    for bad in ((np.zeros(4), None), (np.zeros((5, 3)), None), (None, np.zeros(5)), (np.nan, None)):
        with pytest.raises(ValueError):
            bare.query_batch(qn, qp, 3, 1, between=bad)
    for bad in (3, (1, 2, 3), ("a", None), (None, True)):
        with pytest.raises(TypeError):
            bare.query_batch(qn, qp, 3, 1, between=bad)
    with pytest.raises(ValueError):
        bare.set_values(np.zeros(N0 + 1))
    with pytest.raises(TypeError):
        bare.set_values(np.zeros(N0, dtype=bool))
    with pytest.raises(ValueError):
        bare.set_values(np.zeros((N0, 5)))
    bare.world = 2
    with pytest.raises(RuntimeError, match="list-sharded"):
        bare.set_values(np.zeros(N0))
    bare.world = 1
    ivf = IVF("euclidean", 3, None)
    ivf._dev = bare
    ivf.data = np.zeros((N0, D), np.float32)
    with pytest.raises(ValueError, match="without values"):
        ivf.query_batch(qn, 3, between=(0, 1))
    with pytest.raises(ValueError, match="without values"):
        ivf.query(qn[0], 3, between=(0, 1))
    ivf.values = np.zeros((N0, 2), np.float32)
    with pytest.raises(NotImplementedError, match="between"):
        ivf.query_batch(qn, 3, fast=True, between=(0, 1))
    with pytest.raises(ValueError):
        ivf.query_batch(qn, 3, between=(np.zeros(5), None))
    with pytest.raises(ValueError, match="NaN"):
        ivf.query(qn[0], 3, between=([0, np.nan], None))
    with pytest.raises(ValueError):
        ivf.query(qn[0], 3, between=([0, 1, 2], None))
    with pytest.raises(TypeError):
        ivf.query(qn[0], 3, between=5)


def test_new_symbols_declared_and_exported():
    from tinyknn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tinyknn_hip.h")).read()
    declared = set(re.findall(r"\b(tk_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("tk_index_set_values", "tk_index_values", "tk_index_value_columns", "tk_index_value_table",
                 "tk_index_query_batch_ex5", "tk_index_query_batch_dev_ex5"):
        assert name in declared, name
        assert hasattr(lib, name), f"{name} declared but not exported"
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["tk_index_query_batch_ex5"][1]) == len(_lib.SIGNATURES["tk_index_query_batch_ex4"][1]) + 1
    assert len(_lib.SIGNATURES["tk_index_query_batch_dev_ex5"][1]) == \
        len(_lib.SIGNATURES["tk_index_query_batch_dev_ex4"][1]) + 1
    assert lib.tk_index_set_values(None, None, 0, 0) == -1
    assert lib.tk_index_values(None) == -1 and lib.tk_index_value_columns(None) == -1
    assert lib.tk_index_value_table(None, None) == -1


# ---- the equivalence the device relies on, and the census of the fuzz cases ----

def _default_cases():
    return [t for t in (bs.fuzz_case(s) for s in range(bs.FUZZ_DEFAULT_SEEDS)) if t.skipped is None]


def test_empty_value_substitution_gives_the_guarded_heaps(oracle):
    """On the default cases: query_pq's replay over each probed list with the rows outside the query's ranges replaced
    by the heap's empty value, no guard (what the pass does), leaves the heaps of the replay with `insert` guarded."""
    replays = 0
    for t in _default_cases():
        c = t.case
        ox, k, n_probes = c.ox, c.shape["k"], c.shape["n_probes"]
        R = (n_probes + 1) * k + 1
        for i in range(0, len(c.qn), max(1, len(c.qn) // 4)):
            allowed = passing(t.values, *bounds_of(t.between, i))
            _, dbg = ox.query(np.ascontiguousarray(c.qn[i]), k, n_probes, None, debug=True)
            tables = oracle.transform_tables(dbg["table"])
            heaps = []
            for substitute in (False, True):
                hidx, hval = np.full(R, -1, dtype=np.int64), np.full(R, 127, dtype=np.int32)
                for p in dbg["probes"]:
                    cl = int(p) + ox.n_lists if p < 0 else int(p)
                    c0, c1 = int(ox.list_chunk_off[cl]), int(ox.list_chunk_off[cl + 1])
                    if c1 == c0:
                        continue
                    n = int(ox.list_n[cl])
                    labels = ox.ids[ox.ids_off[cl]:ox.ids_off[cl] + n]
                    out = np.zeros(2 * (c1 - c0), dtype=np.uint64)
                    oracle.estimate_pq(np.ascontiguousarray(ox.codes[c0:c1]), tables, out, True, ox._s.order)
                    replay_blocks(oracle, out.view(np.uint8).reshape(-1, 16), n, labels, hidx, hval, True, allowed,
                                  substitute)
                    replays += 1
                heaps.append((hidx, hval))
            np.testing.assert_array_equal(heaps[0][0], heaps[1][0], err_msg=f"{t} query {i}")
            np.testing.assert_array_equal(heaps[0][1], heaps[1][1], err_msg=f"{t} query {i}")
    assert replays > 100


def test_census_of_the_default_seeds(oracle):
    """Counted over the default seeds whatever TINYKNN_FUZZ_SEEDS says, on the reference alone: each of these happens
    in at least two cases (the counts are recorded in DESIGN §3.14)."""
    cases = [bs.fuzz_case(s) for s in range(bs.FUZZ_DEFAULT_SEEDS)]
    built = [t for t in cases if t.skipped is None]
    assert len(cases) - len(built) <= len(cases) // 4, [t.skipped for t in cases]
    count = collections.Counter()
    for t in built:
        c, k = t.case, t.case.shape["k"]
        want, _ = t.want()
        n, n_base = (want != -1).sum(axis=1), (c.base != -1).sum(axis=1)
        f = rs.facts(c, answers=False)
        held = dict(empty_answer=(n == 0).any(), shorter_than_k=((n > 0) & (n < k)).any(),
                    differs_at_the_same_length=((n == n_base) & (want != c.base).any(axis=1)).any(),
                    probes_a_list_shorter_than_a_chunk=f["probes_short"], probes_an_emptied_list=f["probes_empty"],
                    names_a_list_twice=f["wraps"], **bs.chunk_facts(t))
        for name, yes in held.items():
            count[name] += bool(yes)
        count["values:" + t.value_kind] += 1
        count["with_tags"] += t.tags is not None
        for kind in set(t.range_kinds):
            count["range:" + kind] += 1
        # what the ranges promise of the ids, beside the case's own restriction
        for i, row in enumerate(want):
            ids = row[row != -1]
            assert passing(t.values, *bounds_of(t.between, i))[ids].all(), (t, i)
            if c.allowed is not None:
                assert c.allowed[ids].all(), (t, i)
    print(dict(count))
    for name in ("empty_answer", "shorter_than_k", "differs_at_the_same_length", "probes_a_list_shorter_than_a_chunk",
                 "probes_an_emptied_list", "names_a_list_twice", "point_pair", "all_beside_none", "conjunction"):
        assert count[name] >= 2, (name, dict(count))
    for name in ["values:" + kind for kind in bs.VALUE_KINDS] + ["range:" + kind for kind in bs.RANGE_KINDS] + ["with_tags"]:
        assert count[name] >= 1, (name, dict(count))


def test_cases_follow_from_the_seed_and_leave_the_case_alone():
    a, b = bs.BetweenCase(5), bs.fuzz_case(5)
    assert a.case is b.case and a.value_kind == b.value_kind and a.range_kinds == b.range_kinds
    assert a.values.tobytes() == b.values.tobytes()
    for x, y in zip(a.between, b.between):
        assert x.tobytes() == y.tobytes()
    assert len(a.values) == len(a.case.ref_data) and len(a.between[0]) == len(a.case.qn)
    assert a.case.ivf.values is None and "between" not in a.case.device_kwargs()
    assert set(a.case.device_kwargs()) | {"between"} <= set(a.device_kwargs())
