"""IVF.add without a GPU: the bookkeeping build records for it (list_columns), its persistence, the numpy splice
of an index that has no device copy, and the refusals decided on the host."""
import ctypes
import os
import weakref

import numpy as np
import pytest


def _fitted(metric="angular", d=40, n=2000, clusters=20, seed=0):
    from tinyknn_amd import IVF, FastPQ
    X = np.random.RandomState(seed).randn(n, d).astype(np.float32)
    ivf = IVF(metric, clusters, FastPQ(2))
    np.random.seed(seed)
    ivf.fit(X[:1500])
    return ivf, X


def _same_lists_up_to_order(a, b, kp):
    """Lists of two host-built indexes: same members (in the same column blocks) and the same code per member;
    the order inside a block is numpy's unstable argsort's."""
    from tinyknn_amd._transform import unpack
    assert len(a.active_centers) == len(b.active_centers)
    np.testing.assert_array_equal(a.list_columns, b.list_columns)
    for i in range(len(a.active_centers)):
        ia, ib = np.asarray(a.ids[i], dtype=np.int64), np.asarray(b.ids[i], dtype=np.int64)
        assert len(ia) == len(ib)
        if len(ia) == 0:
            continue
        la, lb = unpack(a.pq_transformed_points[i].packed), unpack(b.pq_transformed_points[i].packed)
        o = 0
        for j in range(kp):
            c = int(a.list_columns[i, j])
            sa, sb = np.argsort(ia[o:o + c], kind="stable"), np.argsort(ib[o:o + c], kind="stable")
            np.testing.assert_array_equal(ia[o:o + c][sa], ib[o:o + c][sb])
            np.testing.assert_array_equal(la[o:o + c][sa], lb[o:o + c][sb])
            o += c
        np.testing.assert_array_equal(la[len(ia):], lb[len(ib):])       # padding: the zero vector's code


@pytest.mark.parametrize("kp", [1, 2, 3])
def test_build_records_list_columns(kp):
    from tinyknn_amd.utils import knn_brute
    ivf, X = _fitted()
    ivf.build(X, n_probes=kp, device=False)
    near = knn_brute(ivf.data, ivf.all_centers, k=kp, metric="angular")
    cols = ivf.list_columns
    assert cols.shape == (len(ivf.active_centers), kp) and cols.dtype == np.int64
    for i in range(len(ivf.active_centers)):
        ids = np.asarray(ivf.ids[i], dtype=np.int64)
        assert cols[i].sum() == len(ids)
        o = 0
        for j in range(kp):      # column block j holds exactly the rows whose j-th nearest centre is i
            blk = ids[o:o + cols[i, j]]
            np.testing.assert_array_equal(np.sort(blk), np.nonzero(near[:, j] == i)[0])
            o += cols[i, j]


def test_save_load_round_trips_list_columns(tmp_path):
    from tinyknn_amd import IVF
    ivf, X = _fitted()
    ivf.build(X, n_probes=2, device=False)
    ivf.save(tmp_path / "a")
    back = IVF.load(tmp_path / "a")
    np.testing.assert_array_equal(back.list_columns, ivf.list_columns)
    z = dict(np.load(tmp_path / "a.npz"))
    assert int(z["format_version"]) == 1
    del z["list_columns"]                   # a file written before add() existed
    np.savez(tmp_path / "old.npz", **z)
    assert IVF.load(tmp_path / "old.npz").list_columns is None


@pytest.mark.parametrize("kp", [1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_splice_equals_build_over_all_rows(kp, dtype):
    """An index with no device copy grows by a numpy splice: the lists of build(vstack(...)) up to the order
    inside a column block."""
    from tinyknn_amd import IVF, FastPQ
    ivf, X = _fitted()
    X = X.astype(dtype)
    grown = IVF("angular", 20, FastPQ(2))
    grown.all_centers, grown.pq = ivf.all_centers, ivf.pq
    grown.build(X[:1200], n_probes=kp, device=False)
    for a, b in ((1200, 1201), (1201, 1216), (1216, 1233), (1233, 2000)):
        assert grown.add(X[a:b]) is grown
    assert grown.data.dtype == dtype and grown.data.shape == (2000, 40)
    want = IVF("angular", 20, FastPQ(2))
    want.all_centers, want.pq = ivf.all_centers, ivf.pq
    want.build(X, n_probes=kp, device=False)
    np.testing.assert_array_equal(grown.data, want.data)
    _same_lists_up_to_order(grown, want, kp)


def test_loaded_file_without_list_columns_recovers_them(tmp_path):
    from tinyknn_amd import IVF
    ivf, X = _fitted()
    ivf.build(X[:1500], n_probes=2, device=False)
    ivf.save(tmp_path / "a")
    z = dict(np.load(tmp_path / "a.npz"))
    del z["list_columns"]
    np.savez(tmp_path / "old.npz", **z)
    old = IVF.load(tmp_path / "old.npz")
    old.add(X[1500:])
    ivf.add(X[1500:])
    _same_lists_up_to_order(old, ivf, 2)
    for i in range(len(ivf.active_centers)):       # the same splice: identical, order included
        np.testing.assert_array_equal(np.asarray(old.ids[i], np.int64), np.asarray(ivf.ids[i], np.int64))


def test_host_refusals():
    import tinyknn_amd
    from tinyknn_amd import multi_gpu
    from tinyknn_amd.ivf import DeviceIndex
    ivf, X = _fitted()
    ivf.build(X, n_probes=1, device=False)
    with pytest.raises(AssertionError):
        ivf.add(X[:, :30])                                     # wrong dimension
    with pytest.raises(NotImplementedError):
        multi_gpu.ListShardedIndex.add(object.__new__(multi_gpu.ListShardedIndex), X[:5])
    with pytest.raises(NotImplementedError):
        multi_gpu.ReplicaGroup.add(object.__new__(multi_gpu.ReplicaGroup), X[:5])

    class Sharded:
        world, rank = 2, 0
    ivf._dev = Sharded()                                      # an IVF whose device index was sharded in place
    with pytest.raises(NotImplementedError):
        ivf.add(X[:5])
    ivf._dev = None

    class Session:
        _s = 1
    dev = DeviceIndex.__new__(DeviceIndex)                   # (no handle: refused before the library is called)
    dev.world, dev._streams, dev._live_streams = 1, {}, weakref.WeakSet()
    s = Session()
    dev._live_streams.add(s)
    with pytest.raises(RuntimeError, match="stream"):
        dev.add(X[:5], 1)
    assert len(ivf.data) == 2000 and tinyknn_amd.IVF.add


def test_add_rows_is_exported():
    from tinyknn_amd import _lib
    for name in ("tk_index_add_rows", "tk_index_list_columns"):
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.lib_path()), name)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "tinyknn_hip.h")).read()
    assert "int tk_index_add_rows(" in hdr
