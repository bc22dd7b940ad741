"""IVF.remove without a GPU: the numpy path of an index that has no device copy against a direct filter of the lists,
list_columns bookkeeping and its persistence, add after remove, and the refusals decided on the host."""
import ctypes
import os
import weakref

import numpy as np
import pytest


def _built(kp, dtype=np.float32, metric="angular", d=40, n=2000, clusters=20, seed=0):
    from tinyknn_amd import IVF, FastPQ
    X = np.random.RandomState(seed).randn(n, d).astype(dtype)
    ivf = IVF(metric, clusters, FastPQ(2))
    np.random.seed(seed)
    ivf.fit(X[:1500])
    ivf.build(X, n_probes=kp, device=False)
    return ivf, X


def _snapshot(ivf):
    from tinyknn_amd._transform import unpack
    L = len(ivf.active_centers)
    ids = [np.asarray(ivf.ids[i], np.int64).copy() for i in range(L)]
    lab = [unpack(ivf.pq_transformed_points[i].packed)[:len(ids[i])].copy() for i in range(L)]
    return ids, lab, np.array(ivf.list_columns, copy=True)


def _filtered(snap, dead):
    """The lists of `snap` with the dead rows dropped, everything else in its old order; columns recounted."""
    ids, lab, cols = snap
    out_ids, out_lab, out_cols = [], [], np.zeros_like(cols)
    for i in range(len(ids)):
        keep = ~dead[ids[i]]
        out_ids.append(ids[i][keep])
        out_lab.append(lab[i][keep])
        blk = np.repeat(np.arange(cols.shape[1]), cols[i])
        out_cols[i] = np.bincount(blk[keep], minlength=cols.shape[1])
    return out_ids, out_lab, out_cols


def _assert_lists(ivf, want):
    from tinyknn_amd._transform import unpack
    ids, lab, cols = want
    zero = ivf._zero_label()
    np.testing.assert_array_equal(ivf.list_columns, cols)
    assert len(ivf.active_centers) == len(ids)
    for i in range(len(ids)):
        got_ids = np.asarray(ivf.ids[i], np.int64)
        np.testing.assert_array_equal(got_ids, ids[i])
        t = ivf.pq_transformed_points[i]
        if len(ids[i]) == 0:
            assert isinstance(t, np.ndarray) and t.shape[0] == 0     # as FastPQ.transform of no rows
            continue
        assert t.size == len(ids[i])
        got = unpack(t.packed)
        np.testing.assert_array_equal(got[:len(ids[i])], lab[i])
        np.testing.assert_array_equal(got[len(ids[i]):], np.repeat(zero[None], len(got) - len(ids[i]), 0))


@pytest.mark.parametrize("kp", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_remove_equals_filtered_lists(kp, dtype):
    ivf, X = _built(kp, dtype)
    N = len(ivf.data)
    rng = np.random.RandomState(kp)
    snap = _snapshot(ivf)
    R = rng.choice(N, N // 10, replace=False)
    R = np.concatenate([R, snap[0][3], R[:7]])            # + every member of list 3, + duplicates
    dead = np.zeros(N, bool)
    dead[R] = True
    assert ivf.remove(R) is ivf
    want = _filtered(snap, dead)
    _assert_lists(ivf, want)
    assert len(want[0][3]) == 0 and len(ivf.active_centers) == len(snap[0])      # the emptied list stays
    assert ivf.data.shape == (N, X.shape[1]) and ivf.data.dtype == dtype         # ids are stable
    assert set(ivf.last_remove_ms) == {"device", "host"}
    mask = np.zeros(N, bool)                              # a mask, then an already-removed id: idempotent
    mask[rng.choice(N, 50, replace=False)] = True
    dead |= mask
    ivf.remove(mask)
    want = _filtered(snap, dead)
    _assert_lists(ivf, want)
    ivf.remove(R[:20])
    ivf.remove(np.zeros(0, np.int64))
    ivf.remove(np.zeros(N, bool))
    _assert_lists(ivf, want)


def test_remove_everything_leaves_empty_lists():
    ivf, X = _built(2)
    L = len(ivf.active_centers)
    ivf.remove(np.ones(len(ivf.data), bool))
    assert len(ivf.active_centers) == L
    assert all(isinstance(t, np.ndarray) and t.shape[0] == 0 for t in ivf.pq_transformed_points)
    assert ivf.list_columns.shape == (L, 2) and ivf.list_columns.sum() == 0


def _rebuilt(ivf, X, kp):
    """A fresh index over X with ivf's fitted centres and codebook."""
    from tinyknn_amd import IVF, FastPQ
    out = IVF(ivf.metric, ivf.n_clusters, FastPQ(2))
    out.all_centers, out.pq = ivf.all_centers, ivf.pq
    return out.build(X, n_probes=kp, device=False)


def test_list_columns_persist_and_add_after_remove(tmp_path):
    from tinyknn_amd import IVF
    ivf, X = _built(2)
    base, extra = X[:1700], X[1700:]
    a, b = _rebuilt(ivf, base, 2), _rebuilt(ivf, base, 2)
    R = np.random.RandomState(4).choice(1700, 300, replace=False)
    a.remove(R).add(extra)                                # remove, then add ...
    b.add(extra).remove(R)                                # ... equals add, then remove
    _assert_lists(a, _snapshot(b))
    # a file saved after remove carries list_columns; add on the loaded copy continues where the original does
    c = _rebuilt(ivf, base, 2)
    c.remove(R)
    c.save(tmp_path / "after_remove")
    back = IVF.load(tmp_path / "after_remove")
    np.testing.assert_array_equal(back.list_columns, c.list_columns)
    assert len(back.data) == 1700
    back.add(extra)
    c.add(extra)
    _assert_lists(back, _snapshot(c))
    _assert_lists(back, _snapshot(a))


def test_file_without_list_columns_recovers_them_before_removing(tmp_path):
    from tinyknn_amd import IVF
    ivf, X = _built(2)
    ivf.save(tmp_path / "a")
    z = dict(np.load(tmp_path / "a.npz"))
    del z["list_columns"]                                 # a file written before list_columns existed
    np.savez(tmp_path / "old.npz", **z)
    old = IVF.load(tmp_path / "old.npz")
    assert old.list_columns is None
    R = np.arange(0, 2000, 3)
    old.remove(R)
    ivf.remove(R)
    _assert_lists(old, _snapshot(ivf))


def test_refusals():
    import tinyknn_amd
    from tinyknn_amd import multi_gpu
    from tinyknn_amd.ivf import DeviceIndex
    ivf, X = _built(1)
    N = len(ivf.data)
    snap = _snapshot(ivf)
    for bad, exc in ((np.array([0, N]), ValueError), (np.array([-1]), ValueError),
                     (np.zeros(N - 1, bool), ValueError), (np.zeros((2, 3), np.int64), TypeError),
                     (np.array([0.0, 1.0]), TypeError)):
        with pytest.raises(exc):
            ivf.remove(bad)
    _assert_lists(ivf, snap)                              # nothing changed
    with pytest.raises(NotImplementedError):
        multi_gpu.ListShardedIndex.remove(object.__new__(multi_gpu.ListShardedIndex), [0])
    with pytest.raises(NotImplementedError):
        multi_gpu.ReplicaGroup.remove(object.__new__(multi_gpu.ReplicaGroup), [0])

    class Sharded:
        world, rank = 2, 0
    ivf._dev = Sharded()                                  # an IVF whose device index was sharded in place
    with pytest.raises(NotImplementedError):
        ivf.remove([0])
    ivf._dev = None

    class Session:
        _s = 1
    dev = DeviceIndex.__new__(DeviceIndex)                # (no handle: refused before the library is called)
    dev.world, dev._streams, dev._live_streams = 1, {}, weakref.WeakSet()
    s = Session()
    dev._live_streams.add(s)
    with pytest.raises(RuntimeError, match="stream"):
        dev.remove([0])
    dev.world = 2
    with pytest.raises(RuntimeError, match="list-sharded"):
        dev.remove([0])
    _assert_lists(ivf, snap)
    assert tinyknn_amd.IVF.remove


def test_remove_rows_is_exported():
    from tinyknn_amd import _lib
    assert "tk_index_remove_rows" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "tk_index_remove_rows")
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "tinyknn_hip.h")).read()
    assert "int tk_index_remove_rows(" in hdr
