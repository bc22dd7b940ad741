"""IVF.update on the GPU (tk_index_update_rows; devbuild.hip replace_lists_kernel, scatter_rows_kernel): stored rows
replaced in place, ids kept.  The index afterwards is byte-identical to a fresh upload (tk_index_set_lists + set_data)
of the reference lists and vectors of update_reference.py, and answers as the reference's IVF.query over them (ids,
probe lists, heap arrays; distances bit for bit against the fresh upload).  Equivalence with remove + add, edge cases
and refusals, batches in flight (old lists AND old vectors), every replay mode, allowed sets, query_rows, groups,
streams, persistence."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from allowed_reference import guarded_batch  # noqa: E402
from groups_reference import grouped_batch  # noqa: E402
from rows_reference import excluded_batch  # noqa: E402
from test_remove_gpu import (NC, SEED, SIGMA, _assert_oracle, _assert_same_answers, _assert_same_lists, _fitted,  # noqa: E402
                             _host_index, _oracle_of, _queries, _resident, _snapshot)
from update_reference import assignment_of_added, relabelled, updated_data, updated_lists  # noqa: E402

ROW0 = 1 << 20          # the replacement rows' own stretch of the generator: no stored row, no query


def _fresh(metric, d, n, row0=ROW0):
    from tinyknn_amd.ivf import synth_rows
    return synth_rows(n, d, SEED, _fitted(metric, d)[2], SIGMA, row0=row0)


def _prepared(ivf, X, kp):
    """The rows as the host build prepares them, from the reference's own functions: (rows, nearest, labels)."""
    from tinyknn_amd._transform import unpack
    from tinyknn_amd.utils import knn_brute
    new = X.astype(ivf.data.dtype)
    if ivf.metric == "angular":
        new = new / np.linalg.norm(new, axis=1, keepdims=True)
    near = np.asarray(knn_brute(new, ivf.all_centers, k=kp, metric=ivf.metric)).reshape(len(new), kp)
    return new, near, unpack(ivf.pq.transform(new).packed)[:len(new)]


def _update_set(snap, N, seed, frac=0.1, whole_list=5):
    """About frac of the rows drawn at random plus every member of one list, in no order."""
    rng = np.random.RandomState(seed)
    ids = np.union1d(rng.choice(N, int(frac * N), replace=False), snap[0][whole_list])
    return rng.permutation(ids).astype(np.int64)


def _rows_outside(ivf, n, kp, lst=5):
    """n fresh rows whose kp nearest centres (the host's own knn_brute assignment) all differ from `lst`: drawn with a
    surplus, the others dropped — so a list whose members are all replaced by them provably empties."""
    d = ivf.data.shape[1]
    X = _fresh(ivf.metric, d, n + n // 2 + 64)
    near = _prepared(ivf, X, kp)[1]
    X = X[~(near == lst).any(axis=1)]
    assert len(X) >= n
    return np.ascontiguousarray(X[:n])


def _ref_ivf(ivf, lists, data, zero, L1=None):
    """An IVF whose host lists are the reference's (ids, labels per list) over `data`: what a fresh upload takes
    (DeviceIndex(ref)) and what the oracle runs over."""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd._transform import transform_data
    from tinyknn_amd.fast_pq import TransformedData
    ids_l, lab_l = lists[0], lists[1]
    ref = IVF(ivf.metric, ivf.n_clusters, FastPQ(2))
    ref.pq, ref.all_centers, ref.store = ivf.pq, ivf.all_centers, ivf.store
    ref.active_centers, ref.pq_transformed_centers = ivf.active_centers, ivf.pq_transformed_centers
    if L1 is not None:                                    # lists were appended: their centres and codes as the build makes them
        ref.active_centers = np.ascontiguousarray(ivf.all_centers[:L1], dtype=np.float32)
        ref.pq_transformed_centers = ivf.pq.transform(ref.active_centers)
    ref.data = data
    pts = []
    for i in range(len(ids_l)):
        n1 = len(ids_l[i])
        if n1 == 0:
            pts.append(np.empty((0, data.shape[1])))
            continue
        lab = np.concatenate([lab_l[i], np.repeat(zero[None], (-n1) % 16, axis=0)])
        pts.append(TransformedData(n1, transform_data(np.ascontiguousarray(lab, dtype=np.uint8))))
    ref.pq_transformed_points, ref.ids = pts, list(ids_l)
    return ref


def _assert_same_distances(a, b, qn, qp, probes=(1, 10, 50)):
    for p in probes:
        ia, da = a.query_batch(qn, qp, 10, p, return_distances=True)
        ib, db = b.query_batch(qn, qp, 10, p, return_distances=True)
        np.testing.assert_array_equal(ia, ib)
        assert da.dtype == db.dtype and np.array_equal(da.view(np.uint8), db.view(np.uint8)), f"distances p={p}"


def _stored_as(dev, rows):
    """float32 rows as read_rows gives them back from this index's store."""
    if dev.store == "float16":
        return rows.astype(np.float16).astype(np.float32)
    return np.asarray(rows, dtype=np.float32)


def _lists_of(snap, N):
    """(N, kp): the list in whose column-j block every row sits (-1: not stored)."""
    kp = snap[2].shape[1]
    out = np.full((N, kp), -1, np.int64)
    for l in range(len(snap[0])):
        out[snap[0][l], np.repeat(np.arange(kp), snap[2][l])] = l
    return out


def _moved(snap, N, ids, near):
    """The share of the replaced rows whose column-0 list changes."""
    return np.mean(_lists_of(snap, N)[ids, 0] != near[:, 0])


CASES = [(kp, metric, d, np.float32, None) for kp in (1, 2, 3) for metric in ("angular", "euclidean") for d in (100, 40)]
CASES.append((2, "euclidean", 100, np.float64, None))
CASES.append((2, "euclidean", 100, np.float32, "float16"))


@pytest.mark.parametrize("kp,metric,d,dtype,store", CASES)
def test_update_equals_the_reference_lists(oracle, kp, metric, d, dtype, store):
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import DeviceIndex, synth_rows
    if store is None:
        ivf = _host_index(metric, d, kp, dtype)
    else:
        A, pq, cent = _fitted(metric, d)
        ivf = IVF(metric, NC, FastPQ(2))
        ivf.all_centers, ivf.pq = A, pq
        ivf.build(synth_rows(4000, d, SEED, cent, SIGMA), n_probes=kp, store=store)
    dev = ivf.device_index()
    N = len(ivf.data)
    snap, data0 = _snapshot(dev, ivf.list_columns), ivf.data.copy()
    ids = _update_set(snap, N, 100 * kp + d)
    X = _rows_outside(ivf, len(ids), kp)
    new, near, lab = _prepared(ivf, X, kp)
    assert ivf.update(ids, X) is ivf
    assert ivf.device_index() is dev and dev.N == N and len(ivf.data) == N and dev.store == (store or str(np.dtype(dtype)))
    assert set(ivf.last_update_ms) == {"device", "host"}
    want = updated_lists(snap, ids, near, lab)
    assert len(want[0][5]) == 0                           # the list empties, and stays
    assert _moved(snap, N, ids, near) >= 0.5
    assert sum(len(x) for x in want[0]) == N * kp
    ref = _ref_ivf(ivf, want, updated_data(data0, ids, new), snap[3])
    up = DeviceIndex(ref)                                 # a fresh upload of the reference lists and vectors
    _assert_same_lists(dev, up)
    if kp >= 2:
        assert dev.twin_table_width() > 0
    np.testing.assert_array_equal(dev.list_columns(), want[2])
    np.testing.assert_array_equal(ivf.list_columns, want[2])
    if dtype == np.float32:         # (read_rows reads float32 and half stores; float64 vectors: the distances below)
        got_rows, want_rows = dev.read_rows(ids), _stored_as(dev, new)
        assert np.array_equal(got_rows.view(np.uint32), want_rows.view(np.uint32))
        allrows = np.arange(N)
        np.testing.assert_array_equal(dev.read_rows(allrows), up.read_rows(allrows))
    np.testing.assert_array_equal(ivf.data, ref.data)     # the IVF's host copy is the reference too
    assert ivf.data.dtype == dtype
    for i in range(len(want[0])):
        np.testing.assert_array_equal(np.asarray(ivf.ids[i], np.int64), want[0][i])
    qn, qp = _queries(ivf, d)
    _assert_same_answers(dev, up, qn, qp)
    _assert_same_distances(dev, up, qn, qp)
    if store == "float16":                                # the oracle rescoring over the rows the device holds
        ref.data = _stored_as(dev, ref.data)
    _assert_oracle(oracle, dev, ref, qn, qp)


def _resident_reference(ivf, twin, ids, X):
    """The reference of update(ids, X) on the resident index `ivf` (before the call), with the rows' assignment,
    labels and prepared vectors taken from `twin` — an identical index to which add(X) appends them.
    -> (reference IVF, reference list_columns, prepared rows, nearest)."""
    dev = ivf.device_index()
    N, n = dev.N, len(ids)
    snap = _snapshot(dev)
    data0 = dev.read_rows(np.arange(N))
    twin.add(X)
    td = twin.device_index()
    near, lab = assignment_of_added(_snapshot(td), N, n)
    new = td.read_rows(N + np.arange(n))
    want = updated_lists(snap, ids, near, lab)
    return _ref_ivf(ivf, want, updated_data(data0, ids, new), snap[3]), want[2], new, near, snap


@pytest.mark.parametrize("kp", [1, 2])
@pytest.mark.parametrize("metric,d", [("angular", 100), ("euclidean", 40)])
def test_resident_update(oracle, metric, d, kp):
    from tinyknn_amd.ivf import DeviceIndex
    N = 5003
    ivf, twin = _resident(metric, d, N, kp), _resident(metric, d, N, kp)
    dev = ivf.device_index()
    ids = _update_set(_snapshot(dev), N, 7 + kp, frac=0.3)
    X = _fresh(metric, d, len(ids))
    ref, cols1, new, near, snap = _resident_reference(ivf, twin, ids, X)
    bytes0 = dev.vector_bytes
    assert ivf.update(ids, X) is ivf
    assert ivf.last_update_ms["host"] == 0.0 and ivf.last_update_ms["device"] > 0.0
    assert dev.N == N and dev.vector_bytes == bytes0 and ivf.data.shape == (N, d)
    assert _moved(snap, N, ids, near) >= 0.5
    up = DeviceIndex(ref)
    _assert_same_lists(dev, up)
    np.testing.assert_array_equal(dev.list_columns(), cols1)
    np.testing.assert_array_equal(ivf.list_columns, cols1)
    np.testing.assert_array_equal(ivf.list_sizes, [len(x) for x in ref.ids])
    np.testing.assert_array_equal(dev.read_rows(ids), new)
    np.testing.assert_array_equal(dev.read_rows(np.arange(N)), ref.data)
    qn, qp = _queries(ivf, d)
    _assert_same_answers(dev, up, qn, qp)
    _assert_same_distances(dev, up, qn, qp, probes=(10,))
    _assert_oracle(oracle, dev, ref, qn, qp, probes=(10,))


@pytest.mark.parametrize("kp", [1, 2])
def test_update_equals_remove_then_add_relabelled(kp):
    metric, d, N = "euclidean", 40, 5003
    a, b = _resident(metric, d, N, kp), _resident(metric, d, N, kp)
    ids = _update_set(_snapshot(a.device_index()), N, 20 + kp, frac=0.2)
    X = _fresh(metric, d, len(ids))
    a.update(ids, X)
    assert b.remove(ids).add(X) is b
    da, db = a.device_index(), b.device_index()
    assert da.N == N and db.N == N + len(ids) and da.vector_bytes < db.vector_bytes
    sa, ca, ia = da.export_lists()
    sb, cb, ib = db.export_lists()
    np.testing.assert_array_equal(sa, sb)
    np.testing.assert_array_equal(ca, cb)
    np.testing.assert_array_equal(ia, relabelled([ib], N, ids)[0])
    np.testing.assert_array_equal(da.list_columns(), db.list_columns())
    np.testing.assert_array_equal(da.read_rows(ids), db.read_rows(N + np.arange(len(ids))))
    keep = np.setdiff1d(np.arange(N), ids)
    np.testing.assert_array_equal(da.read_rows(keep), db.read_rows(keep))


def test_holes_are_refilled():
    from tinyknn_amd.ivf import DeviceIndex
    metric, d, N, kp = "angular", 100, 5003, 2
    ivf, twin = _resident(metric, d, N, kp), _resident(metric, d, N, kp)
    dev = ivf.device_index()
    gone = np.random.RandomState(3).choice(N, 600, replace=False)
    ivf.remove(gone)
    twin.remove(gone)
    assert dev.export_lists(codes=False)[0].sum() == (N - 600) * kp
    ids = np.concatenate([gone[::2], np.setdiff1d(np.arange(N), gone)[:211]])    # holes, and rows still stored
    X = _fresh(metric, d, len(ids))
    ref, cols1, new, _, _ = _resident_reference(ivf, twin, ids, X)
    ivf.update(ids, X)
    assert dev.export_lists(codes=False)[0].sum() == (N - 300) * kp
    _assert_same_lists(dev, DeviceIndex(ref))
    rest = gone[1::2]
    ivf.update(rest, _fresh(metric, d, len(rest), row0=2 * ROW0))
    assert dev.export_lists(codes=False)[0].sum() == N * kp         # every hole refilled: total_ids is back
    np.testing.assert_array_equal(np.sort(dev.export_lists(codes=False)[2]), np.repeat(np.arange(N), kp))
    qn, qp = _queries(ivf, d, 16)
    assert (dev.query_batch(qn, qp, 10, 5) >= 0).all()


def test_update_of_every_row_and_of_rows_that_stay(oracle):
    from tinyknn_amd.ivf import DeviceIndex
    metric, d, kp = "euclidean", 100, 2
    ivf = _host_index(metric, d, kp)
    dev = ivf.device_index()
    N = len(ivf.data)
    # rows that all stay in their lists (their own vectors; euclidean: prepared as they are): each moves to the end
    # of its column block, the columns keep their sizes
    snap, data0 = _snapshot(dev, ivf.list_columns), ivf.data.copy()
    ids = np.random.RandomState(2).choice(N, 1000, replace=False)
    ids = ids[(_prepared(ivf, data0[ids], kp)[1] == _lists_of(snap, N)[ids]).all(axis=1)]     # (but for a tie that flipped)
    assert len(ids) >= 900
    same = data0[ids].copy()
    new, near, lab = _prepared(ivf, same, kp)
    assert (near == _lists_of(snap, N)[ids]).all()        # every row stays in its kp lists
    ivf.update(ids, same)
    want = updated_lists(snap, ids, near, lab)
    np.testing.assert_array_equal(want[2], snap[2])
    assert any(not np.array_equal(a, b) for a, b in zip(want[0], snap[0]))
    ref = _ref_ivf(ivf, want, data0, snap[3])
    _assert_same_lists(dev, DeviceIndex(ref))
    np.testing.assert_array_equal(dev.read_rows(np.arange(N)), data0)
    # every row
    snap = _snapshot(dev, ivf.list_columns)
    ids = np.random.RandomState(4).permutation(N).astype(np.int64)
    X = _fresh(metric, d, N)
    new, near, lab = _prepared(ivf, X, kp)
    ivf.update(ids, X)
    want = updated_lists(snap, ids, near, lab)
    ref = _ref_ivf(ivf, want, updated_data(data0, ids, new), snap[3])
    up = DeviceIndex(ref)
    _assert_same_lists(dev, up)
    np.testing.assert_array_equal(dev.list_columns(), want[2])
    np.testing.assert_array_equal(dev.read_rows(np.arange(N)), ref.data)
    qn, qp = _queries(ivf, d)
    _assert_same_answers(dev, up, qn, qp, probes=(10,))
    _assert_oracle(oracle, dev, ref, qn, qp, probes=(10,))


@pytest.mark.parametrize("kp", [1, 2])
def test_update_activates_a_new_list_or_refuses(oracle, kp):
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import DeviceIndex, synth_rows
    A, pq, cent = _fitted("euclidean", 100)
    rng = np.random.RandomState(5)
    far = (A[:6] + 40.0 * rng.randn(6, 100)).astype(A.dtype)          # centres no built row is near
    ivf = IVF("euclidean", NC + 6, FastPQ(2))
    ivf.all_centers, ivf.pq = np.concatenate([A, far]), pq
    ivf.build(synth_rows(4000, 100, SEED, cent, SIGMA), n_probes=kp)
    L = len(ivf.active_centers)
    assert L == NC
    dev = ivf.device_index()
    snap, data0 = _snapshot(dev, ivf.list_columns), ivf.data.copy()
    before = [x.copy() for x in dev.export_lists()] + list(dev.export_centers()) + [dev.read_rows(np.arange(4000))]
    ids = np.array([17, 3999, 0, 1234], dtype=np.int64)
    bad = (ivf.all_centers[L + 5] + 0.01 * rng.randn(4, 100)).astype(np.float32)
    with pytest.raises(AssertionError, match="utils.py:128"):
        ivf.update(ids, bad)
    for x, y in zip(before, list(dev.export_lists()) + list(dev.export_centers()) + [dev.read_rows(np.arange(4000))]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(ivf.data, data0)
    assert len(ivf.active_centers) == L and dev.n_lists == L
    ids = np.random.RandomState(6).choice(4000, 20, replace=False).astype(np.int64)
    good = (ivf.all_centers[L] + 0.01 * rng.randn(20, 100)).astype(np.float32)
    new, near, lab = _prepared(ivf, good, kp)
    assert (near[:, 0] == L).all()
    ivf.update(ids, good)
    assert len(ivf.active_centers) == L + 1 and dev.n_lists == L + 1 and dev.N == 4000
    want = updated_lists(snap, ids, near, lab)
    np.testing.assert_array_equal(want[0][L][:20], ids)
    ref = _ref_ivf(ivf, want, updated_data(data0, ids, new), snap[3], L1=L + 1)
    np.testing.assert_array_equal(ivf.pq_transformed_centers.packed, ref.pq_transformed_centers.packed)
    up = DeviceIndex(ref)
    _assert_same_lists(dev, up)
    np.testing.assert_array_equal(dev.list_columns(), want[2])
    qn, qp = ivf._prepare(np.concatenate([good[:8], data0[:56]]).copy())
    _assert_same_answers(dev, up, qn, qp, probes=(5,))
    _assert_oracle(oracle, dev, ref, qn, qp, probes=(5,))


def _state(dev):
    return [x.copy() for x in dev.export_lists()] + [dev.read_rows(np.arange(dev.N))]


def _assert_state(dev, before):
    for x, y in zip(before, _state(dev)):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_noop_and_refused_updates():
    from tinyknn_amd import IVF, FastPQ, _lib
    from tinyknn_amd.ivf import synth_rows
    metric, d, kp = "euclidean", 100, 2
    ivf = _host_index(metric, d, kp)
    dev = ivf.device_index()
    N = len(ivf.data)
    X = _fresh(metric, d, 8)
    before, data0 = _state(dev), ivf.data.copy()
    aset = dev.allow(np.arange(0, N, 2))
    qn, qp = _queries(ivf, d, 16)
    want = dev.query_batch(qn, qp, 10, 5, allowed=aset)
    ivf.update(np.zeros(0, np.int64), np.zeros((0, d), np.float32))          # n == 0: a no-op
    assert dev.update(np.zeros(0, np.int64), np.zeros((0, d), np.float32), kp, list_columns=ivf.list_columns,
                      all_centers=ivf.all_centers) == dev.n_lists
    for bad in (np.array([3, 9, 3]), np.array([1, N]), np.array([-1, 2])):
        with pytest.raises(ValueError):
            ivf.update(bad, X[:len(bad)])
        with pytest.raises(ValueError):
            dev.update(bad, X[:len(bad)], kp, list_columns=ivf.list_columns, all_centers=ivf.all_centers)
    # the library's own checks, past the Python ones
    A, Y, yn = dev._search_centres(ivf.all_centers)
    cols = np.ascontiguousarray(ivf.list_columns, dtype=np.int64)
    for bad, msg in ((np.array([3, 9, 3], np.int64), "named twice"), (np.array([1, N, 5], np.int64), "outside")):
        out = C.c_int64(-1), C.c_int64(-1)
        with pytest.raises(AssertionError, match=msg):    # (TK_ERR_ARG, as _lib.check maps it)
            _lib.check(_lib.lib().tk_index_update_rows(
                dev.handle, bad.ctypes.data, 3, X.ctypes.data, 0, kp, None, None, cols.ctypes.data, 0, A.ctypes.data,
                Y.ctypes.data, yn.ctypes.data, len(A), None, C.byref(out[0]), C.byref(out[1])))
    _assert_state(dev, before)
    np.testing.assert_array_equal(ivf.data, data0)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, allowed=aset), want)   # the set is still current
    aset.close()
    # a half store refuses a row whose half is not finite: from the host's check, and from the library's own
    A, pq, cent = _fitted(metric, d)
    half = IVF(metric, NC, FastPQ(2))
    half.all_centers, half.pq = A, pq
    half.build(synth_rows(4000, d, SEED, cent, SIGMA), n_probes=kp, store="float16")
    hd = half.device_index()
    before, data0 = _state(hd), half.data.copy()
    Xb = X.copy()
    Xb[5, 3] = 70000.0
    ids = np.arange(100, 108)
    with pytest.raises(ValueError, match=r"row 5\b"):
        half.update(ids, Xb)
    near = np.zeros((8, kp), dtype=np.int64)
    near[:, 1] = 1
    with pytest.raises(ValueError, match=r"row 5\b"):
        hd.update(ids, Xb, kp, nearest=near, labels=np.zeros((8, hd.M), np.uint8), list_columns=half.list_columns)
    _assert_state(hd, before)
    np.testing.assert_array_equal(half.data, data0)
    half.update(ids, X)                                   # ... and takes finite ones, rounded
    assert hd.store == "float16" and hd.vector_bytes == 4000 * d * 2
    np.testing.assert_array_equal(hd.read_rows(ids), X.astype(np.float16).astype(np.float32))


def test_batches_in_flight_answer_the_old_index():
    import torch
    from tinyknn_amd.ivf import DeviceIndex
    metric, d, kp, N = "angular", 100, 2, 6000
    ivf, twin = _resident(metric, d, N, kp), _resident(metric, d, N, kp)
    dev = ivf.device_index()
    ids = _update_set(_snapshot(dev), N, 11, frac=0.25)
    X = _fresh(metric, d, len(ids))
    ref = _resident_reference(ivf, twin, ids, X)[0]
    after = DeviceIndex(ref)
    qn, qp = _queries(ivf, d, 512)
    want_before = dev.query_batch(qn, qp, 10, 10, return_distances=True)
    want_after = after.query_batch(qn, qp, 10, 10, return_distances=True)
    assert (want_before[0] != want_after[0]).any()
    # (queries whose old answer holds a replaced row: their distances show whether the OLD vector was rescored)
    assert np.isin(want_before[0], ids).any(axis=1).sum() > 100
    q_dev = torch.from_numpy(qn).cuda()
    p_dev = torch.from_numpy(np.ascontiguousarray(qp)).cuda()
    f64 = qp.dtype == np.float64
    st = torch.cuda.current_stream().cuda_stream
    dev.set_pipeline(2)
    dev.set_coalesce(2)

    def run():
        outs, dists = [], []
        for a in range(0, 512, 128):
            o = torch.full((128, 10), -1, dtype=torch.int64, device="cuda")
            t = torch.full((128, 10), -1.0, dtype=torch.float32, device="cuda")
            dev.query_batch_dev(q_dev.data_ptr() + a * d * 4, p_dev.data_ptr() + a * qp.shape[1] * qp.itemsize, f64,
                                128, 10, 10, o.data_ptr(), stream=st, dist_ptr=t.data_ptr())
            outs.append(o)
            dists.append(t)
        return outs, dists

    def check(res, want):
        dev.join(st)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(torch.cat(res[0]).cpu().numpy(), want[0])
        got = torch.cat(res[1]).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want[1].view(np.uint32))

    res = run()                                 # calls still owed / held when update() comes
    ivf.update(ids, X)
    check(res, want_before)                     # ids AND distances of the old index: old lists, old vectors
    check(run(), want_after)
    dev.set_coalesce(1)
    dev.set_pipeline(1)


def test_every_replay_mode(oracle):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    N = 20000
    ivf, twin = _resident("angular", 100, N, 2), _resident("angular", 100, N, 2)
    dev = ivf.device_index()
    ids = _update_set(_snapshot(dev), N, 3, frac=0.2)
    X = _fresh("angular", 100, len(ids))
    ref = _resident_reference(ivf, twin, ids, X)[0]
    ivf.update(ids, X)
    qn, qp = _queries(ivf, 100, 256)
    ox = _oracle_of(oracle, ref)
    want, wd = guarded_batch(oracle, ox, qn, 10, 10, debug=True)
    try:
        for heap_mode in (0, 1, 2, 3):
            for plain in (False, "always", True):
                for pair_nq in (4, 8192):
                    if heap_mode != 0 and (plain is not True or pair_nq != 4):
                        continue
                    dev.set_heap_mode(heap_mode)
                    dev.set_plain_scan(plain)
                    dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
                    got, gd = dev.query_batch(qn, qp, 10, 10, debug=True)
                    np.testing.assert_array_equal(got, want, err_msg=str((heap_mode, plain, pair_nq)))
                    for key in ("probes", "heap_idx", "heap_val"):
                        np.testing.assert_array_equal(gd[key], wd[key], err_msg=str((key, heap_mode, plain)))
    finally:
        dev.set_heap_mode(0)
        dev.set_plain_scan(True)
        dev.set_option(_lib.OPT_PAIR_NQ, 4)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 10), DeviceIndex(ref).query_batch(qn, qp, 10, 10))


def _updated_host_index(metric="angular", d=100, kp=2, seed=5):
    """(ivf after update, the reference IVF, ids, N)"""
    ivf = _host_index(metric, d, kp)
    dev = ivf.device_index()
    N = len(ivf.data)
    snap, data0 = _snapshot(dev, ivf.list_columns), ivf.data.copy()
    ids = _update_set(snap, N, seed)
    X = _fresh(metric, d, len(ids))
    new, near, lab = _prepared(ivf, X, kp)
    ivf.update(ids, X)
    ref = _ref_ivf(ivf, updated_lists(snap, ids, near, lab), updated_data(data0, ids, new), snap[3])
    return ivf, ref, ids, N


def test_allowed_sets_streams_and_query_rows(oracle):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import synth_rows
    metric, d, kp = "angular", 100, 2
    ivf = _host_index(metric, d, kp)
    dev = ivf.device_index()
    N = len(ivf.data)
    snap, data0 = _snapshot(dev, ivf.list_columns), ivf.data.copy()
    qn, qp = _queries(ivf, d, 32)
    old = ivf.allow(np.arange(0, N, 2))
    dev.query_batch(qn, qp, 10, 5, allowed=old)
    dev.query_rows(np.arange(8), 10, 5)                   # (the row-position table of the old layout exists)
    ids = _update_set(snap, N, 5)
    X = _fresh(metric, d, len(ids))
    new, near, lab = _prepared(ivf, X, kp)
    st = dev.stream(16, 10, 5)
    before = _state(dev)
    with pytest.raises(RuntimeError, match="stream"):
        ivf.update(ids, X)
    _assert_state(dev, before)
    np.testing.assert_array_equal(ivf.data, data0)
    st.close()
    ivf.update(ids, X)
    with pytest.raises(_lib.TinyKnnHipError, match="earlier layout"):
        dev.query_batch(qn, qp, 10, 5, allowed=old)
    ref = _ref_ivf(ivf, updated_lists(snap, ids, near, lab), updated_data(data0, ids, new), snap[3])
    ox = _oracle_of(oracle, ref)
    mask = np.random.default_rng(2).random(N) < 0.4
    got = dev.query_batch(qn, qp, 10, 5, allowed=ivf.allow(mask))
    np.testing.assert_array_equal(got, guarded_batch(oracle, ox, qn, 10, 5, allowed=mask))
    # query_rows of replaced rows: the new vectors are the queries, the row itself is left out
    rows = np.concatenate([ids[:24], np.setdiff1d(np.arange(N), ids)[:8]])
    rq, rp = dev.gather_queries(rows)
    assert np.array_equal(rq.view(np.uint32), np.ascontiguousarray(ref.data[rows]).view(np.uint32))
    for p in (1, 10):
        got, gd = dev.query_rows(rows, 10, p, debug=True)
        want, wd = excluded_batch(oracle, ox, rq, rows, 10, p, debug=True)
        np.testing.assert_array_equal(got, want)
        for key in ("probes", "heap_idx", "heap_val"):
            np.testing.assert_array_equal(gd[key], wd[key], err_msg=key)
        assert not (got == rows[:, None]).any()
    # a streaming session on the updated index answers as the reference lists do
    qs = synth_rows(32, d, SEED + 1, _fitted(metric, d)[2], SIGMA)
    st = dev.stream(16, 10, 5)
    out = np.full((32, 10), -7, dtype=np.int64)
    st.submit(qs[:16], out[:16])
    st.submit(qs[16:], out[16:])
    st.drain()
    st.close()
    np.testing.assert_array_equal(out, guarded_batch(oracle, ox, qn, 10, 5))


def test_groups_with_and_without_new_ones(oracle):
    metric, d, kp = "euclidean", 40, 2
    ivf = _host_index(metric, d, kp)
    dev = ivf.device_index()
    N = len(ivf.data)
    groups = np.random.RandomState(9).randint(0, 6, size=N).astype(np.int32)
    ivf.set_groups(groups)
    qn, qp = _queries(ivf, d, 32)
    group = np.random.RandomState(10).randint(-1, 6, size=32).astype(np.int32)
    dev.query_batch(qn, qp, 10, 5, group=group)           # (the group table of the old layout exists)
    builds = dev.group_table()["builds"]
    for seed, with_groups in ((5, False), (6, True)):
        snap, data0 = _snapshot(dev, ivf.list_columns), ivf.data.copy()
        ids = _update_set(snap, N, seed)
        X = _fresh(metric, d, len(ids), row0=ROW0 * (1 + seed))
        new, near, lab = _prepared(ivf, X, kp)
        if with_groups:
            g_new = np.random.RandomState(11).randint(0, 6, size=len(ids)).astype(np.int32)
            ivf.update(ids, X, groups=g_new)
            groups = groups.copy()
            groups[ids] = g_new
        else:
            ivf.update(ids, X)                            # the rows keep their groups
        np.testing.assert_array_equal(ivf.groups, groups)
        assert dev.groups_set() == N
        ref = _ref_ivf(ivf, updated_lists(snap, ids, near, lab), updated_data(data0, ids, new), snap[3])
        ox = _oracle_of(oracle, ref)
        got, gd = dev.query_batch(qn, qp, 10, 5, group=group, debug=True)
        want, wd = grouped_batch(oracle, ox, qn, group, groups, 10, 5, debug=True)
        np.testing.assert_array_equal(got, want)
        for key in ("probes", "heap_idx", "heap_val"):
            np.testing.assert_array_equal(gd[key], wd[key], err_msg=key)
        assert dev.group_table()["builds"] > builds       # made again for the new layout
        builds = dev.group_table()["builds"]


def test_persistence_and_update_then_add_then_remove(tmp_path):
    from tinyknn_amd import IVF
    from tinyknn_amd.ivf import DeviceIndex
    ivf, ref, ids, N = _updated_host_index()
    dev = ivf.device_index()
    ivf.save(tmp_path / "after")
    back = IVF.load(tmp_path / "after")
    np.testing.assert_array_equal(back.list_columns, ivf.list_columns)
    np.testing.assert_array_equal(back.data, ivf.data)
    _assert_same_lists(back.device_index(), dev)
    qn, qp = _queries(ivf, 100)
    _assert_same_answers(back.device_index(), dev, qn, qp, probes=(5,))
    # update, then add, then remove: the device index still equals a fresh upload of the host copy, and the loaded
    # index (a plain upload: it knows nothing of the update) continues where the original does
    X = _fresh("angular", 100, 1200, row0=3 * ROW0)
    gone = np.concatenate([ids[:100], np.arange(N, N + 300)])
    for x in (ivf, back):
        x.add(X)
        x.remove(gone)
    _assert_same_lists(dev, DeviceIndex(ivf))
    _assert_same_lists(dev, back.device_index())
    np.testing.assert_array_equal(back.list_columns, ivf.list_columns)
    again = ids[50:150]                                   # half of them holes by now
    Y = _fresh("angular", 100, len(again), row0=4 * ROW0)
    for x in (ivf, back):
        x.update(again, Y)
    _assert_same_lists(dev, DeviceIndex(ivf))
    _assert_same_lists(dev, back.device_index())
    np.testing.assert_array_equal(dev.read_rows(np.arange(dev.N)), back.device_index().read_rows(np.arange(dev.N)))
    _assert_same_answers(dev, DeviceIndex(ivf), qn, qp, probes=(10,))
