"""IVF.add on the GPU (tk_index_add_rows, devbuild.hip merge_lists_kernel): rows merged into the built lists in
place.  A resident index grown row block by row block is byte-identical to build_resident over all its rows; a
host-built index equals the splice of the reference's own functions (knn_brute, pq.transform) and a fresh upload
of its grown host copy; allowed sets, batches in flight, streams and persistence behave."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from allowed_reference import guarded_batch, reference_index  # noqa: E402

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


def _assert_same_index(a, b, qn, qp, probes=(1, 10, 50)):
    """Two device indexes hold the same bytes and answer alike (ids, probe lists, heap arrays)."""
    for x, y in zip(a.export_lists(), b.export_lists()):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a.export_centers(), b.export_centers()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.list_columns(), b.list_columns())
    assert a.twin_table_width() == b.twin_table_width()
    for x, y in zip(a.twin_table(), b.twin_table()):
        np.testing.assert_array_equal(x, y)
    for p in probes:
        ia, da = a.query_batch(qn, qp, 10, p, debug=True)
        ib, db = b.query_batch(qn, qp, 10, p, debug=True)
        np.testing.assert_array_equal(ia, ib)
        for key in ("probes", "heap_idx", "heap_val"):
            np.testing.assert_array_equal(da[key], db[key])


@pytest.mark.parametrize("kp", [1, 2])
@pytest.mark.parametrize("metric,d", [("angular", 100), ("euclidean", 100), ("angular", 40), ("euclidean", 40)])
def test_resident_add_equals_resident_build(metric, d, kp):
    from tinyknn_amd.ivf import synth_rows
    N0 = 5003                                   # not a multiple of 16
    grown = _resident(metric, d, N0, kp)
    cent = _fitted(metric, d)[2]
    N = N0
    for n in (1, 15, 17, 1000):
        assert grown.add(synth_rows(n, d, SEED, cent, SIGMA, row0=N)) is grown
        N += n
    dev = grown.device_index()
    assert dev.N == N and grown.data.shape == (N, d)
    fresh = _resident(metric, d, N, kp)
    fd = fresh.device_index()
    np.testing.assert_array_equal(dev.read_rows(np.arange(N)), fd.read_rows(np.arange(N)))
    np.testing.assert_array_equal(grown.list_columns, fresh.list_columns)
    np.testing.assert_array_equal(grown.active_centers, fresh.active_centers)
    np.testing.assert_array_equal(grown.pq_transformed_centers.packed, fresh.pq_transformed_centers.packed)
    qn, qp = _queries(grown, d)
    _assert_same_index(dev, fd, qn, qp)


def test_resident_add_pipelined_and_with_batches_in_flight():
    import torch
    from tinyknn_amd.ivf import synth_rows
    metric, d, kp, N0, n = "angular", 100, 2, 6000, 2500
    grown = _resident(metric, d, N0, kp)
    before = _resident(metric, d, N0, kp).device_index()
    fresh = _resident(metric, d, N0 + n, kp).device_index()
    dev = grown.device_index()
    qn, qp = _queries(grown, d, 512)
    want_before = before.query_batch(qn, qp, 10, 10)
    want_after = fresh.query_batch(qn, qp, 10, 10)
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

    outs = run()                                # calls still owed / held when add() comes
    grown.add(synth_rows(n, d, SEED, _fitted(metric, d)[2], SIGMA, row0=N0))
    dev.join(st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.cat(outs).cpu().numpy(), want_before)
    outs = run()
    dev.join(st)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(torch.cat(outs).cpu().numpy(), want_after)
    dev.set_coalesce(1)
    dev.set_pipeline(1)
    _assert_same_index(dev, fresh, qn[:64], qp[:64], probes=(10,))


def _host_index(kp, dtype, d=100, n0=3001):
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import synth_rows
    A, pq, cent = _fitted("angular", d)
    X = synth_rows(6000, d, SEED, cent, SIGMA).astype(dtype)
    ivf = IVF("angular", NC, FastPQ(2))
    ivf.all_centers, ivf.pq = A, pq
    ivf.build(X[:n0], n_probes=kp)
    return ivf, X


def _splice_oracle(ivf0, X_new, kp):
    """The lists after add from the reference's own functions: knn_brute on the new rows, pq.transform for their
    codes, the old lists kept in place (column block j = old_j ++ new_j ascending)."""
    from tinyknn_amd._transform import unpack
    from tinyknn_amd.utils import knn_brute
    new = X_new.astype(ivf0.data.dtype)
    new = new / np.linalg.norm(new, axis=1, keepdims=True)
    near = knn_brute(new, ivf0.all_centers, k=kp, metric="angular")
    lab = unpack(ivf0.pq.transform(new).packed)[:len(new)]
    N0, L = len(ivf0.data), len(ivf0.active_centers)
    ids, labels = [], []
    for i in range(L):
        old_ids = np.asarray(ivf0.ids[i], np.int64)
        old_lab = unpack(ivf0.pq_transformed_points[i].packed)[:len(old_ids)] if len(old_ids) else None
        ip, lp, o = [], [], 0
        for j in range(kp):
            c = int(ivf0.list_columns[i, j])
            sel = np.nonzero(near[:, j] == i)[0]
            ip += [old_ids[o:o + c], N0 + sel]
            if c:
                lp.append(old_lab[o:o + c])
            lp.append(lab[sel])
            o += c
        ids.append(np.concatenate(ip))
        labels.append(np.concatenate(lp))
    return ids, labels, near


@pytest.mark.parametrize("kp", [1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_built_add(oracle, kp, dtype):
    import copy
    from tinyknn_amd._transform import unpack
    from tinyknn_amd.ivf import DeviceIndex
    ivf, X = _host_index(kp, dtype)
    dev = ivf.device_index()
    n0 = len(ivf.data)
    for a, b in ((n0, n0 + 1), (n0 + 1, n0 + 17), (n0 + 17, 5000), (5000, 6000)):
        snap = copy.copy(ivf)
        snap.ids, snap.pq_transformed_points = list(ivf.ids), list(ivf.pq_transformed_points)
        want_ids, want_lab, _ = _splice_oracle(snap, X[a:b], kp)
        ivf.add(X[a:b])
        assert ivf.device_index() is dev and ivf.data.dtype == dtype and len(ivf.data) == b
        for i in range(len(want_ids)):
            np.testing.assert_array_equal(np.asarray(ivf.ids[i], np.int64), want_ids[i])
            got = unpack(ivf.pq_transformed_points[i].packed)
            np.testing.assert_array_equal(got[:len(want_ids[i])], want_lab[i])
            np.testing.assert_array_equal(got[len(want_ids[i]):], np.repeat(ivf._zero_label()[None], len(got) - len(want_ids[i]), 0))
    assert set(ivf.last_add_ms) == {"device", "host"}
    up = DeviceIndex(ivf)                       # a fresh upload of the grown host copy: no stale derived state
    for x, y in zip(dev.export_lists(), up.export_lists()):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(dev.export_centers(), up.export_centers()):
        np.testing.assert_array_equal(x, y)
    assert dev.twin_table_width() == up.twin_table_width()
    qn, qp = _queries(ivf, X.shape[1])
    for p in (1, 10, 50):
        np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, p), up.query_batch(qn, qp, 10, p))
    ox = reference_index(ivf)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5), ox.query_batch(qn, 10, 5))


@pytest.mark.parametrize("kp", [1, 2])
def test_inactive_centres_append_lists_or_refuse(kp):
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd._transform import unpack
    A, pq, cent = _fitted("euclidean", 100)
    rng = np.random.RandomState(5)
    far = (A[:6] + 40.0 * rng.randn(6, 100)).astype(A.dtype)          # centres no built row is near
    ivf = IVF("euclidean", NC + 6, FastPQ(2))
    ivf.all_centers, ivf.pq = np.concatenate([A, far]), pq
    from tinyknn_amd.ivf import synth_rows
    X = synth_rows(4000, 100, SEED, cent, SIGMA)          # the rows k-means was fitted on: every centre owns some
    ivf.build(X, n_probes=kp)
    L = len(ivf.active_centers)
    assert L == NC
    dev = ivf.device_index()
    before = [x.copy() for x in dev.export_lists()] + list(dev.export_centers())
    # rows near centre L + 5: centre L .. L + 4 stay empty -> the build's contract error, nothing changes
    bad = (ivf.all_centers[L + 5] + 0.01 * rng.randn(4, 100)).astype(np.float32)
    with pytest.raises(AssertionError, match="utils.py:128"):
        ivf.add(bad)
    for x, y in zip(before, list(dev.export_lists()) + list(dev.export_centers())):
        np.testing.assert_array_equal(x, y)
    assert len(ivf.data) == 4000 and len(ivf.active_centers) == L and dev.N == 4000
    # rows near centre L: list L is appended, the centres' codes are the build's
    good = (ivf.all_centers[L] + 0.01 * rng.randn(20, 100)).astype(np.float32)
    ivf.add(good)
    assert len(ivf.active_centers) == L + 1 and dev.n_lists == L + 1
    np.testing.assert_array_equal(np.asarray(ivf.ids[L], np.int64)[:ivf.list_columns[L, 0]],
                                  np.arange(4000, 4020))
    np.testing.assert_array_equal(ivf.pq_transformed_centers.packed, pq.transform(ivf.all_centers[:L + 1].astype(np.float32)).packed)
    ac, cc = dev.export_centers()
    np.testing.assert_array_equal(ac, ivf.active_centers)
    np.testing.assert_array_equal(cc, ivf.pq_transformed_centers.packed)
    from tinyknn_amd.ivf import DeviceIndex
    up = DeviceIndex(ivf)
    qn, qp = ivf._prepare(np.concatenate([good[:8], X[:56]]).copy())
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5), up.query_batch(qn, qp, 10, 5))


def test_resident_activation_codes_centres_on_the_device():
    from tinyknn_amd import IVF, FastPQ
    A, pq, cent = _fitted("euclidean", 100)
    far = (A[:3] + 40.0 * np.random.RandomState(6).randn(3, 100)).astype(A.dtype)
    ivf = IVF("euclidean", NC + 3, FastPQ(2))
    ivf.all_centers, ivf.pq = np.concatenate([A, far]), pq
    ivf.build_resident(4000, 100, SEED, cent, SIGMA)
    L = len(ivf.active_centers)
    ivf.add((ivf.all_centers[L] + 0.01 * np.random.RandomState(2).randn(5, 100)).astype(np.float32))
    assert len(ivf.active_centers) == L + 1 and ivf.list_sizes[L] == 5
    np.testing.assert_array_equal(ivf.pq_transformed_centers.packed,
                                  pq.transform(ivf.all_centers[:L + 1].astype(np.float32), device=True).packed)
    with pytest.raises(AssertionError):
        ivf.add((ivf.all_centers[L + 2] + 0.01 * np.random.RandomState(2).randn(5, 100)).astype(np.float32))
    assert ivf.device_index().N == 4005


def test_allowed_sets_and_streams(oracle):
    from tinyknn_amd import _lib
    ivf, X = _host_index(2, np.float32)
    dev = ivf.device_index()
    qn, qp = _queries(ivf, X.shape[1], 32)
    old = ivf.allow(np.arange(0, 3001, 2))
    dev.query_batch(qn, qp, 10, 5, allowed=old)
    st = dev.stream(16, 10, 5)
    with pytest.raises(RuntimeError, match="stream"):
        ivf.add(X[3001:3100])
    assert len(ivf.data) == 3001
    st.close()
    ivf.add(X[3001:4000])
    with pytest.raises(_lib.TinyKnnHipError, match="earlier layout"):
        dev.query_batch(qn, qp, 10, 5, allowed=old)
    mask = np.zeros(4000, dtype=bool)
    mask[3001:] = True                                    # only rows added
    mask[::3] = True
    got = dev.query_batch(qn, qp, 10, 5, allowed=ivf.allow(mask))
    want = guarded_batch(oracle, reference_index(ivf), qn, 10, 5, allowed=mask)
    np.testing.assert_array_equal(got, want)
    assert (got >= 3001).any()


def test_persistence_after_add(tmp_path):
    from tinyknn_amd import IVF
    ivf, X = _host_index(2, np.float32)
    ivf.save(tmp_path / "before")
    z = dict(np.load(tmp_path / "before.npz"))
    del z["list_columns"]                                 # a file written before add() existed
    np.savez(tmp_path / "old.npz", **z)
    ivf.add(X[3001:4500])
    ivf.save(tmp_path / "after")
    back = IVF.load(tmp_path / "after")
    qs = X[4500:4564].copy()
    qn, qp = ivf._prepare(qs.copy())
    np.testing.assert_array_equal(back.device_index().query_batch(qn, qp, 10, 5),
                                  ivf.device_index().query_batch(qn, qp, 10, 5))
    old = IVF.load(tmp_path / "old.npz")
    assert old.list_columns is None
    old.device_index()
    old.add(X[3001:4500])
    np.testing.assert_array_equal(old.list_columns, ivf.list_columns)
    for x, y in zip(old.device_index().export_lists(), ivf.device_index().export_lists()):
        np.testing.assert_array_equal(x, y)
