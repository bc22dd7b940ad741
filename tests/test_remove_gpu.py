"""IVF.remove on the GPU (tk_index_remove_rows, devbuild.hip compact_lists_kernel): rows deleted from the built lists
in place.  The index afterwards is byte-identical to a fresh upload (tk_index_set_lists) of its lists filtered on the
host, and answers as the reference's IVF.query over those filtered lists (ids, probe lists, heap arrays) — not as an
allowed set on the old index would.  Round trips with add, edge cases, every replay mode, batches in flight, allowed
sets, streams and persistence."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from allowed_reference import guarded_batch  # noqa: E402

SEED, SIGMA, NC = 7, 0.7, 48
_FITTED = {}


def _fitted(metric, d):
    """(all_centers, pq, generator centres) fitted once per (metric, d): d = 100 leaves the PQ unrotated
    (fast_pq.py:77), d = 40 rotates it."""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import synth_rows
    key = (metric, d)
    if key not in _FITTED:
        cent = np.random.RandomState(3).randn(30, d).astype(np.float32)
        ivf = IVF(metric, NC, FastPQ(2))
        np.random.seed(1)
        ivf.fit(synth_rows(4000, d, SEED, cent, SIGMA))
        assert (ivf.pq.R is None) == (d == 100)
        _FITTED[key] = (ivf.all_centers, ivf.pq, cent)
    return _FITTED[key]


def _host_index(metric, d, kp, dtype=np.float32, N=4000):
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import synth_rows
    A, pq, cent = _fitted(metric, d)
    ivf = IVF(metric, NC, FastPQ(2))
    ivf.all_centers, ivf.pq = A, pq
    ivf.build(synth_rows(N, d, SEED, cent, SIGMA).astype(dtype), n_probes=kp)
    return ivf


def _resident(metric, d, N, kp):
    from tinyknn_amd import IVF, FastPQ
    A, pq, cent = _fitted(metric, d)
    ivf = IVF(metric, NC, FastPQ(2))
    ivf.all_centers, ivf.pq = A, pq
    return ivf.build_resident(N, d, SEED, cent, SIGMA, n_probes=kp)


def _queries(ivf, d, nq=64):
    from tinyknn_amd.ivf import synth_rows
    qs = synth_rows(nq, d, SEED + 1, _fitted(ivf.metric, d)[2], SIGMA)
    return ivf._prepare(qs.copy())


def _snapshot(dev, cols=None):
    """The device index's lists on the host: ids and labels per list, members per (list, column) (cols, or the
    index's own), the zero vector's labels as its padding rows carry them."""
    from tinyknn_amd._transform import unpack
    sizes, codes, ids = dev.export_lists()
    coff = np.concatenate([[0], np.cumsum((sizes + 15) // 16)])
    ioff = np.concatenate([[0], np.cumsum(sizes)])
    ids_l, lab_l, zero = [], [], None
    for i in range(len(sizes)):
        lab = unpack(codes[coff[i]:coff[i + 1]])
        ids_l.append(ids[ioff[i]:ioff[i + 1]].copy())
        lab_l.append(lab[:sizes[i]].copy())
        if zero is None and len(lab) > sizes[i]:
            zero = lab[sizes[i]].copy()
    assert zero is not None
    return ids_l, lab_l, dev.list_columns() if cols is None else cols, zero


def _filtered(ivf, snap, dead):
    """(IVF whose host lists are snap's minus the dead rows, in their old order, filtered list_columns): what a fresh
    tk_index_set_lists upload takes (DeviceIndex(ivf)) and what the oracle runs over."""
    from tinyknn_amd._transform import transform_data
    from tinyknn_amd.fast_pq import TransformedData
    from tinyknn_amd import IVF, FastPQ
    ids_l, lab_l, cols, zero = snap
    ref = IVF(ivf.metric, ivf.n_clusters, FastPQ(2))
    ref.pq, ref.all_centers = ivf.pq, ivf.all_centers
    ref.active_centers, ref.pq_transformed_centers = ivf.active_centers, ivf.pq_transformed_centers
    ref.data = ivf.data
    if not isinstance(ivf.data, np.ndarray):            # a resident index: its vectors, read back
        ref.data = ivf.device_index().read_rows(np.arange(len(ivf.data)))
    d = ref.data.shape[1]
    pts, idl, cols1 = [], [], None if cols is None else np.zeros_like(cols)
    for i in range(len(ids_l)):
        keep = ~dead[ids_l[i]]
        n1 = int(keep.sum())
        idl.append(ids_l[i][keep])
        if cols is not None:
            cols1[i] = np.bincount(np.repeat(np.arange(cols.shape[1]), cols[i])[keep], minlength=cols.shape[1])
        if n1 == 0:
            pts.append(np.empty((0, d)))
            continue
        lab = lab_l[i][keep]
        lab = np.concatenate([lab, np.repeat(zero[None], (-n1) % 16, axis=0)])
        pts.append(TransformedData(n1, transform_data(np.ascontiguousarray(lab))))
    ref.pq_transformed_points, ref.ids = pts, idl
    return ref, cols1


def _oracle_of(oracle, ref):
    L = len(ref.active_centers)
    pts = ref.pq_transformed_points
    return oracle.OracleIndex(ref.pq.centers, 2, ref.pq.R, ref.pq.sqrt_n_blocks, ref.active_centers,
                              ref.pq_transformed_centers.packed,
                              [None if isinstance(pts[i], np.ndarray) else pts[i].packed for i in range(L)],
                              [0 if isinstance(pts[i], np.ndarray) else pts[i].size for i in range(L)],
                              [np.asarray(ref.ids[i], np.int64) for i in range(L)], ref.data)


def _assert_same_lists(a, b):
    """Two device indexes hold the same lists, centres and twin table."""
    for x, y in zip(a.export_lists(), b.export_lists()):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a.export_centers(), b.export_centers()):
        np.testing.assert_array_equal(x, y)
    assert a.twin_table_width() == b.twin_table_width()
    np.testing.assert_array_equal(_twins(a), _twins(b))


def _twins(dev):
    """The twin table, each row's (list, offset) entries sorted: the builder hands out the slots of a label's copies
    with an atomic cursor, so their order inside a row is unspecified for any upload (kp >= 3)."""
    lst, off = (np.asarray(x, np.int64) for x in dev.twin_table())
    return np.sort((lst << 32) | off, axis=-1)


def _assert_same_answers(a, b, qn, qp, probes=(1, 10, 50)):
    for p in probes:
        ia, da = a.query_batch(qn, qp, 10, p, debug=True)
        ib, db = b.query_batch(qn, qp, 10, p, debug=True)
        np.testing.assert_array_equal(ia, ib)
        for key in ("probes", "heap_idx", "heap_val"):
            np.testing.assert_array_equal(da[key], db[key], err_msg=key)


def _assert_oracle(oracle, dev, ref, qn, qp, probes=(1, 10, 50)):
    ox = _oracle_of(oracle, ref)
    for p in probes:
        got, gd = dev.query_batch(qn, qp, 10, p, debug=True)
        want, wd = guarded_batch(oracle, ox, qn, 10, p, debug=True)
        np.testing.assert_array_equal(got, want)
        for key in ("probes", "heap_idx", "heap_val"):
            np.testing.assert_array_equal(gd[key], wd[key], err_msg=key)


def _removal(snap, N, seed, frac=0.1, whole_list=5):
    """A random ~frac of the rows plus every member of one list (+ a few duplicates)."""
    rng = np.random.RandomState(seed)
    R = rng.choice(N, int(frac * N), replace=False)
    R = np.concatenate([R, snap[0][whole_list], R[:9]])
    dead = np.zeros(N, bool)
    dead[R] = True
    return R, dead


CASES = [(kp, metric, d, np.float32) for kp in (1, 2, 3) for metric in ("angular", "euclidean") for d in (100, 40)]
CASES.append((2, "euclidean", 100, np.float64))


@pytest.mark.parametrize("kp,metric,d,dtype", CASES)
def test_remove_equals_filtered_lists(oracle, kp, metric, d, dtype):
    from tinyknn_amd.ivf import DeviceIndex
    ivf = _host_index(metric, d, kp, dtype)
    dev = ivf.device_index()
    N = len(ivf.data)
    snap = _snapshot(dev, ivf.list_columns)
    R, dead = _removal(snap, N, 100 * kp + d)
    assert ivf.remove(R) is ivf
    assert ivf.device_index() is dev and dev.N == N and len(ivf.data) == N
    assert set(ivf.last_remove_ms) == {"device", "host"}
    ref, cols1 = _filtered(ivf, snap, dead)
    assert len(ref.ids[5]) == 0
    up = DeviceIndex(ref)                       # a fresh upload of the filtered host lists
    _assert_same_lists(dev, up)
    if kp >= 2:
        assert dev.twin_table_width() > 0       # (the table is rebuilt, not dropped)
    np.testing.assert_array_equal(dev.list_columns(), cols1)
    np.testing.assert_array_equal(ivf.list_columns, cols1)
    for i in range(len(ref.ids)):               # the IVF's host copy is the filtered lists too
        np.testing.assert_array_equal(np.asarray(ivf.ids[i], np.int64), ref.ids[i])
    qn, qp = _queries(ivf, d)
    _assert_same_answers(dev, up, qn, qp)
    _assert_oracle(oracle, dev, ref, qn, qp)


@pytest.mark.parametrize("kp", [1, 2])
@pytest.mark.parametrize("metric,d", [("angular", 100), ("euclidean", 40)])
def test_resident_remove(oracle, metric, d, kp):
    from tinyknn_amd.ivf import DeviceIndex
    ivf = _resident(metric, d, 5003, kp)
    dev = ivf.device_index()
    snap = _snapshot(dev)
    R, dead = _removal(snap, 5003, 7 + kp, frac=0.3)
    ivf.remove(R)
    assert ivf.last_remove_ms["host"] == 0.0
    ref, cols1 = _filtered(ivf, snap, dead)
    up = DeviceIndex(ref)
    _assert_same_lists(dev, up)
    np.testing.assert_array_equal(ivf.list_columns, cols1)
    np.testing.assert_array_equal(ivf.list_sizes, [len(x) for x in ref.ids])
    qn, qp = _queries(ivf, d)
    _assert_same_answers(dev, up, qn, qp)
    _assert_oracle(oracle, dev, ref, qn, qp, probes=(10,))


@pytest.mark.parametrize("kp", [1, 2])
def test_add_then_remove_the_added_rows_is_the_index_before(kp):
    from tinyknn_amd.ivf import synth_rows
    metric, d, N0, n = "angular", 100, 5003, 777
    ivf = _resident(metric, d, N0, kp)
    before = _resident(metric, d, N0, kp)
    L = len(ivf.active_centers)
    ivf.add(synth_rows(n, d, SEED, _fitted(metric, d)[2], SIGMA, row0=N0))
    assert len(ivf.active_centers) == L          # (rows that activate no centre)
    ivf.remove(np.arange(N0, N0 + n))
    dev, bd = ivf.device_index(), before.device_index()
    _assert_same_lists(dev, bd)
    np.testing.assert_array_equal(dev.list_columns(), bd.list_columns())
    qn, qp = _queries(ivf, d)
    _assert_same_answers(dev, bd, qn, qp)


@pytest.mark.parametrize("kp", [1, 2])
def test_remove_then_add_equals_add_then_remove(kp):
    from tinyknn_amd.ivf import synth_rows
    metric, d, N0, n = "euclidean", 40, 4000, 1500
    a, b = _resident(metric, d, N0, kp), _resident(metric, d, N0, kp)
    X = synth_rows(n, d, SEED, _fitted(metric, d)[2], SIGMA, row0=N0)
    R = np.random.RandomState(kp).choice(N0, 900, replace=False)
    a.remove(R).add(X)
    b.add(X).remove(R)
    da, db = a.device_index(), b.device_index()
    assert da.N == db.N == N0 + n
    _assert_same_lists(da, db)
    np.testing.assert_array_equal(da.list_columns(), db.list_columns())
    qn, qp = _queries(a, d)
    _assert_same_answers(da, db, qn, qp)


def test_remove_every_row(oracle):
    ivf = _host_index("angular", 100, 2)
    dev = ivf.device_index()
    snap = _snapshot(dev, ivf.list_columns)
    N = len(ivf.data)
    L = dev.n_lists
    ivf.remove(np.ones(N, bool))
    assert dev.n_lists == L and (dev.export_lists(codes=False, ids=False)[0] == 0).all()
    assert ivf.list_columns.sum() == 0
    qn, qp = _queries(ivf, 100, 32)
    for p in (1, 10):
        assert (dev.query_batch(qn, qp, 10, p) == -1).all()
    ref, _ = _filtered(ivf, snap, np.ones(N, bool))
    _assert_oracle(oracle, dev, ref, qn, qp, probes=(1, 10))
    assert (ivf.query_batch(qn[:4], 10, 5) == -1).all()


def test_noop_and_refused_removals():
    from tinyknn_amd import _lib
    import ctypes as C
    ivf = _host_index("euclidean", 100, 2)
    dev = ivf.device_index()
    N = len(ivf.data)
    R = np.arange(0, N, 7)
    ivf.remove(R)
    before = [x.copy() for x in dev.export_lists()]
    qn, qp = _queries(ivf, 100, 16)
    aset = dev.allow(np.arange(0, N, 2))
    want = dev.query_batch(qn, qp, 10, 5, allowed=aset)
    for again in (R, R[:5], np.concatenate([R, R]), np.zeros(0, np.int64), np.zeros(N, bool)):
        ivf.remove(again)                       # already removed, duplicates, empty: nothing changes
        assert dev.remove(again) == 0
    for x, y in zip(before, dev.export_lists()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, allowed=aset), want)   # the set is still current
    with pytest.raises(ValueError):
        ivf.remove(np.array([1, N]))
    bad = np.array([3, N + 5], dtype=np.int64)  # the library's own check, past the Python one
    removed = C.c_int64(-1)
    with pytest.raises(AssertionError, match="outside"):      # (TK_ERR_ARG, as _lib.check maps it)
        _lib.check(_lib.lib().tk_index_remove_rows(dev.handle, bad.ctypes.data, 2, 2, None, C.byref(removed)))
    for x, y in zip(before, dev.export_lists()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, allowed=aset), want)
    aset.close()


def test_every_replay_mode(oracle):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    ivf = _resident("angular", 100, 20000, 2)
    dev = ivf.device_index()
    snap = _snapshot(dev)
    R, dead = _removal(snap, 20000, 3, frac=0.2)
    ivf.remove(R)
    ref, _ = _filtered(ivf, snap, dead)
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


def test_batches_in_flight_answer_the_old_index():
    import torch
    from tinyknn_amd.ivf import DeviceIndex
    metric, d, kp, N = "angular", 100, 2, 6000
    ivf = _resident(metric, d, N, kp)
    dev = ivf.device_index()
    snap = _snapshot(dev)
    R, dead = _removal(snap, N, 11, frac=0.25)
    ref, _ = _filtered(ivf, snap, dead)
    after = DeviceIndex(ref)
    qn, qp = _queries(ivf, d, 512)
    want_before = dev.query_batch(qn, qp, 10, 10)
    want_after = after.query_batch(qn, qp, 10, 10)
    assert (want_before != want_after).any()
    q_dev = torch.from_numpy(qn).cuda()
    p_dev = torch.from_numpy(np.ascontiguousarray(qp)).cuda()
    f64 = qp.dtype == np.float64
    st = torch.cuda.current_stream().cuda_stream
    dev.set_pipeline(2)
    dev.set_coalesce(2)

    def run():
        outs = []
        for a in range(0, 512, 128):
            o = torch.full((128, 10), -1, dtype=torch.int64, device="cuda")
            dev.query_batch_dev(q_dev.data_ptr() + a * d * 4, p_dev.data_ptr() + a * qp.shape[1] * qp.itemsize, f64,
                                128, 10, 10, o.data_ptr(), stream=st)
            outs.append(o)
        return outs

    outs = run()                                # calls still owed / held when remove() comes
    ivf.remove(R)
    dev.join(st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.cat(outs).cpu().numpy(), want_before)
    outs = run()
    dev.join(st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.cat(outs).cpu().numpy(), want_after)
    dev.set_coalesce(1)
    dev.set_pipeline(1)


def test_allowed_sets_and_streams(oracle):
    from tinyknn_amd import _lib
    ivf = _host_index("angular", 100, 2)
    dev = ivf.device_index()
    snap = _snapshot(dev, ivf.list_columns)
    N = len(ivf.data)
    qn, qp = _queries(ivf, 100, 32)
    old = ivf.allow(np.arange(0, N, 2))
    dev.query_batch(qn, qp, 10, 5, allowed=old)
    st = dev.stream(16, 10, 5)
    R, dead = _removal(snap, N, 5)
    with pytest.raises(RuntimeError, match="stream"):
        ivf.remove(R)
    for x, y in zip(snap[0], _snapshot(dev)[0]):
        np.testing.assert_array_equal(x, y)
    st.close()
    ivf.remove(R)
    with pytest.raises(_lib.TinyKnnHipError, match="earlier layout"):
        dev.query_batch(qn, qp, 10, 5, allowed=old)
    ref, _ = _filtered(ivf, snap, dead)
    ox = _oracle_of(oracle, ref)
    mask = np.random.default_rng(2).random(N) < 0.4
    got = dev.query_batch(qn, qp, 10, 5, allowed=ivf.allow(mask))
    np.testing.assert_array_equal(got, guarded_batch(oracle, ox, qn, 10, 5, allowed=mask))
    assert not dead[got[got != -1]].any()
    # a streaming session on the shrunk index answers as the filtered lists do
    from tinyknn_amd.ivf import synth_rows
    qs = synth_rows(32, 100, SEED + 1, _fitted("angular", 100)[2], SIGMA)
    st = dev.stream(16, 10, 5)
    out = np.full((32, 10), -7, dtype=np.int64)
    st.submit(qs[:16], out[:16])
    st.submit(qs[16:], out[16:])
    st.drain()
    st.close()
    np.testing.assert_array_equal(out, guarded_batch(oracle, ox, qn, 10, 5))


def test_persistence_after_remove(tmp_path):
    from tinyknn_amd import IVF
    from tinyknn_amd.ivf import synth_rows
    ivf = _host_index("angular", 100, 2)
    N = len(ivf.data)
    R = np.random.RandomState(8).choice(N, 700, replace=False)
    ivf.remove(R)
    ivf.save(tmp_path / "after")
    back = IVF.load(tmp_path / "after")
    np.testing.assert_array_equal(back.list_columns, ivf.list_columns)
    qn, qp = _queries(ivf, 100)
    np.testing.assert_array_equal(back.device_index().query_batch(qn, qp, 10, 5),
                                  ivf.device_index().query_batch(qn, qp, 10, 5))
    # add on the loaded index (a plain upload: it knows nothing of the removal) equals add on the original
    X = synth_rows(1200, 100, SEED, _fitted("angular", 100)[2], SIGMA, row0=N)
    back.add(X)
    ivf.add(X)
    np.testing.assert_array_equal(back.list_columns, ivf.list_columns)
    for x, y in zip(back.device_index().export_lists(), ivf.device_index().export_lists()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(back.device_index().query_batch(qn, qp, 10, 5),
                                  ivf.device_index().query_batch(qn, qp, 10, 5))
