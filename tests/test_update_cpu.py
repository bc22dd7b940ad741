"""IVF.update without a GPU: the numpy path of an index that has no device copy against update_reference.py (the
definition, written out) and against remove + add + relabel, list_columns and persistence, argument errors and the
refusals decided on the host, the ctypes signature."""
import ctypes
import os
import sys
import weakref

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from update_reference import relabelled, updated_data, updated_lists  # noqa: E402


def _built(kp, dtype=np.float32, metric="angular", d=40, n=2000, clusters=20, seed=0):
    from tinyknn_amd import IVF, FastPQ
    X = np.random.RandomState(seed).randn(n + 600, d).astype(dtype)
    ivf = IVF(metric, clusters, FastPQ(2))
    np.random.seed(seed)
    ivf.fit(X[:1500])
    ivf.build(X[:n], n_probes=kp, device=False)
    return ivf, X[n:]


def _snapshot(ivf):
    from tinyknn_amd._transform import unpack
    L = len(ivf.active_centers)
    ids = [np.asarray(ivf.ids[i], np.int64).copy() for i in range(L)]
    M = ivf.pq.centers.shape[1] // ivf.pq.dims_per_block
    lab = [unpack(ivf.pq_transformed_points[i].packed)[:len(ids[i])].copy() if len(ids[i]) else np.zeros((0, M), np.uint8)
           for i in range(L)]
    return ids, lab, np.array(ivf.list_columns, copy=True), None


def _assert_lists(ivf, want):
    from tinyknn_amd._transform import unpack
    ids, lab, cols = want[:3]
    zero = ivf._zero_label()
    np.testing.assert_array_equal(ivf.list_columns, cols)
    assert len(ivf.active_centers) == len(ids)
    for i in range(len(ids)):
        np.testing.assert_array_equal(np.asarray(ivf.ids[i], np.int64), ids[i])
        t = ivf.pq_transformed_points[i]
        if len(ids[i]) == 0:
            assert isinstance(t, np.ndarray) and t.shape[0] == 0     # as FastPQ.transform of no rows
            continue
        assert t.size == len(ids[i])
        got = unpack(t.packed)
        np.testing.assert_array_equal(got[:len(ids[i])], lab[i])
        np.testing.assert_array_equal(got[len(ids[i]):], np.repeat(zero[None], len(got) - len(ids[i]), 0))


def _prepared(ivf, X, kp):
    """The rows as the host build prepares them, from the reference's own functions: (rows, nearest, labels)."""
    from tinyknn_amd._transform import unpack
    from tinyknn_amd.utils import knn_brute
    new = X.astype(ivf.data.dtype)
    if ivf.metric == "angular":
        new = new / np.linalg.norm(new, axis=1, keepdims=True)
    near = knn_brute(new, ivf.all_centers, k=kp, metric=ivf.metric)
    return new, np.asarray(near).reshape(len(new), kp), unpack(ivf.pq.transform(new).packed)[:len(new)]


def _update_set(snap, N, seed, whole_list=3):
    """About a tenth of the rows at random plus every member of one list, shuffled (the ids come in no order)."""
    rng = np.random.RandomState(seed)
    ids = np.union1d(rng.choice(N, N // 10, replace=False), snap[0][whole_list])
    return rng.permutation(ids).astype(np.int64)


@pytest.mark.parametrize("kp", [1, 2, 3])
@pytest.mark.parametrize("metric", ["angular", "euclidean"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_update_equals_the_reference(kp, metric, dtype):
    ivf, extra = _built(kp, dtype, metric)
    N, d = ivf.data.shape
    snap, data0 = _snapshot(ivf), ivf.data.copy()
    ids = _update_set(snap, N, kp)
    X = extra[:len(ids)]
    new, near, lab = _prepared(ivf, X, kp)
    assert ivf.update(ids, X) is ivf
    want = updated_lists(snap, ids, near, lab)
    _assert_lists(ivf, want)
    moved = np.mean([ids[i] not in set(snap[0][near[i, 0]][:snap[2][near[i, 0], 0]].tolist()) for i in range(len(ids))])
    assert moved >= 0.5                                   # (random rows: most change their column-0 list)
    assert ivf.data.shape == (N, d) and ivf.data.dtype == dtype
    np.testing.assert_array_equal(ivf.data, updated_data(data0, ids, new))
    assert set(ivf.last_update_ms) == {"device", "host"} and ivf.last_update_ms["device"] == 0.0
    assert sum(len(x) for x in want[0]) == N * kp         # every row still sits in kp lists
    # rows removed earlier are stored again; the index with every hole refilled holds N * kp entries
    gone = ids[:50]
    ivf.remove(gone)
    assert sum(len(np.asarray(ivf.ids[i])) for i in range(len(want[0]))) == (N - 50) * kp
    snap2 = _snapshot(ivf)
    new2, near2, lab2 = _prepared(ivf, extra[-50:], kp)
    ivf.update(gone, extra[-50:])
    want2 = updated_lists(snap2, gone, near2, lab2)
    _assert_lists(ivf, want2)
    assert sum(len(x) for x in want2[0]) == N * kp


@pytest.mark.parametrize("kp", [1, 2, 3])
@pytest.mark.parametrize("metric", ["angular", "euclidean"])
def test_host_update_equals_remove_add_relabel(kp, metric):
    a, extra = _built(kp, metric=metric)
    b, _ = _built(kp, metric=metric)
    N = len(a.data)
    ids = _update_set(_snapshot(a), N, 10 + kp)
    X = extra[:len(ids)]
    a.update(ids, X)
    b.remove(ids).add(X)
    sb = _snapshot(b)
    _assert_lists(a, (relabelled(sb[0], N, ids), sb[1], sb[2]))
    np.testing.assert_array_equal(a.data[ids], b.data[N:])
    assert len(a.data) == N and len(b.data) == N + len(ids)


def test_update_every_row_in_place_and_nothing():
    ivf, extra = _built(2, n=500)
    N = len(ivf.data)
    snap = _snapshot(ivf)
    ivf.update(np.zeros(0, np.int64), np.zeros((0, 40), np.float32))        # n == 0: a no-op
    _assert_lists(ivf, snap)
    assert not hasattr(ivf, "last_update_ms")
    # rows that all stay in their lists (their own vectors again): each moves to the end of its column block
    ids = np.arange(0, N, 3)
    same = ivf.data[ids].copy()
    _, near, lab = _prepared(ivf, same, 2)
    ivf.update(ids, same)
    want = updated_lists(snap, ids, near, lab)
    _assert_lists(ivf, want)
    np.testing.assert_array_equal(want[2], snap[2])       # the columns keep their sizes
    # every row
    snap = _snapshot(ivf)
    ids = np.random.RandomState(1).permutation(N)
    new, near, lab = _prepared(ivf, extra[:N], 2)
    ivf.update(ids, extra[:N])
    _assert_lists(ivf, updated_lists(snap, ids, near, lab))
    np.testing.assert_array_equal(ivf.data[ids], new)


def test_groups_follow_and_persist(tmp_path):
    from tinyknn_amd import IVF
    ivf, extra = _built(2)
    N = len(ivf.data)
    with pytest.raises(ValueError, match="without groups"):
        ivf.update([1, 2], extra[:2], groups=[0, 1])
    g = (np.arange(N) % 5).astype(np.int32)
    ivf.set_groups(g)
    ivf.update([7, 3], extra[:2])                         # without groups=: the rows keep theirs
    np.testing.assert_array_equal(ivf.groups, g)
    ivf.update([7, 11], extra[2:4], groups=[9, 8])
    want = g.copy()
    want[[7, 11]] = [9, 8]
    np.testing.assert_array_equal(ivf.groups, want)
    with pytest.raises(ValueError):
        ivf.update([1, 2], extra[:2], groups=[0])
    ivf.save(tmp_path / "after_update")
    back = IVF.load(tmp_path / "after_update")
    _assert_lists(back, _snapshot(ivf))
    np.testing.assert_array_equal(back.data, ivf.data)
    np.testing.assert_array_equal(back.groups, want)
    back.update([5], extra[4:5])                          # the loaded copy continues where the original does
    ivf.update([5], extra[4:5])
    _assert_lists(back, _snapshot(ivf))


def test_half_store_refuses_before_anything_changes():
    ivf, extra = _built(2, metric="euclidean")
    ivf.store = "float16"
    snap, data0 = _snapshot(ivf), ivf.data.copy()
    X = extra[:3].copy()
    X[1, 4] = 7e4
    with pytest.raises(ValueError, match="row 1 holds a value whose half is not finite"):
        ivf.update([4, 5, 6], X)
    _assert_lists(ivf, snap)
    np.testing.assert_array_equal(ivf.data, data0)


def test_argument_errors_and_refusals():
    from tinyknn_amd import multi_gpu
    from tinyknn_amd.ivf import DeviceIndex
    ivf, extra = _built(1)
    N, d = ivf.data.shape
    snap, data0 = _snapshot(ivf), ivf.data.copy()
    for bad, exc in ((np.array([0, N]), ValueError), (np.array([-1, 3]), ValueError), (np.array([4, 9, 4]), ValueError),
                     (np.zeros(N, bool), TypeError), (np.zeros((1, 2), np.int64), TypeError),
                     (np.array([0.0, 1.0]), TypeError)):
        with pytest.raises(exc):
            ivf.update(bad, extra[:np.asarray(bad).shape[0]])
    with pytest.raises(AssertionError, match="shape"):
        ivf.update([1, 2], extra[:3])                     # one row per id
    with pytest.raises(AssertionError, match="shape"):
        ivf.update([1, 2], extra[:2, :d - 1])
    _assert_lists(ivf, snap)
    np.testing.assert_array_equal(ivf.data, data0)
    with pytest.raises(NotImplementedError, match="ListShardedIndex.update: replacing rows of a list-sharded index"):
        multi_gpu.ListShardedIndex.update(object.__new__(multi_gpu.ListShardedIndex), [0], extra[:1])
    with pytest.raises(NotImplementedError, match="ReplicaGroup.update: replacing rows of a replicated index"):
        multi_gpu.ReplicaGroup.update(object.__new__(multi_gpu.ReplicaGroup), [0], extra[:1])

    class Sharded:
        world, rank = 2, 0
    ivf._dev = Sharded()                                  # an IVF whose device index was sharded in place
    with pytest.raises(NotImplementedError):
        ivf.update([0], extra[:1])
    ivf._dev = None

    class Session:
        _s = 1
    dev = DeviceIndex.__new__(DeviceIndex)                # (no handle: refused before the library is called)
    dev.world, dev._streams, dev._live_streams = 1, {}, weakref.WeakSet()
    s = Session()
    dev._live_streams.add(s)
    with pytest.raises(RuntimeError, match="stream"):
        dev.update([0], extra[:1], 1)
    dev.world = 2
    with pytest.raises(RuntimeError, match="list-sharded"):
        dev.update([0], extra[:1], 1)

    class Clone:
        _h = 1
    dev.world, dev._live_streams = 1, weakref.WeakSet()
    c = Clone()
    dev._clones = [c]
    with pytest.raises(RuntimeError, match="cloned"):
        dev.update([0], extra[:1], 1)
    _assert_lists(ivf, snap)


def test_update_rows_is_exported():
    from tinyknn_amd import _lib
    assert "tk_index_update_rows" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["tk_index_update_rows"][1]) == 17
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "tk_index_update_rows")
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "tinyknn_hip.h")).read()
    assert "int tk_index_update_rows(" in hdr
