"""Distances beside the ids (tk_index_query_batch[_dev]_dist, tk_index_top_centers_dist): the rescoring's exact
squared distances, bit for bit the oracle's sqdist_gather over the returned ids, with ids identical to the ids-only
call — every golden fixture, every rescoring form, allowed sets, pipelined pairs of calls, batches beyond one
workspace, an index grown by add / shrunk by remove, FlatTop."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from allowed_reference import guarded_batch  # noqa: E402
from conftest import G6_TAGS, golden, split_lists  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    return tinyknn_amd


def _fixture_ivf(g):
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import TransformedData
    codes, ids = split_lists(g)
    pq = FastPQ(2)
    pq.centers = g["pq_centers"]
    pq.sqrt_n_blocks = float(g["sqrt_n_blocks"])
    pq.R = g["R"] if "R" in g else None
    ivf = IVF(str(g["metric"]), len(codes), None)
    ivf.pq = pq
    ivf.active_centers = g["active_centers"]
    ivf.pq_transformed_centers = TransformedData(int(g["center_size"]), g["center_codes"])
    ivf.pq_transformed_points = [TransformedData(int(s), c) for s, c in zip(g["list_sizes"], codes)]
    ivf.ids = ids
    ivf.data = g["data"]
    return ivf


def _oracle_index(oracle, g):
    codes, ids = split_lists(g)
    R = g["R"] if "R" in g else None
    return oracle.OracleIndex(g["pq_centers"], 2, R, float(g["sqrt_n_blocks"]), g["active_centers"],
                              g["center_codes"], codes, g["list_sizes"], ids, g["data"])


def _check_dists(oracle, qn, data, ids, dist, einsum=True):
    """dist equals sqdist_gather bit for bit (+inf at -1), numpy's einsum within 1 ulp, dtype as numpy promotes."""
    want_dtype = np.result_type(data.dtype, np.float32)
    assert dist.dtype == want_dtype and dist.shape == ids.shape
    for i in range(len(ids)):
        row = ids[i]
        live = row != -1
        assert np.isposinf(dist[i][~live]).all(), i
        ref = oracle.sqdist_gather(qn[i], data, row[live])
        np.testing.assert_array_equal(dist[i][live].astype(np.float64), ref, err_msg=f"row {i}")
        if einsum and live.any():
            diff = data[row[live]] - qn[i]
            np.testing.assert_array_max_ulp(dist[i][live], np.einsum("ij,ij->i", diff, diff), maxulp=1)


@pytest.mark.parametrize("tag", G6_TAGS)
def test_fixtures_ids_and_exact_distances(tk, oracle, tag):
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = _fixture_ivf(g)
    ox = _oracle_index(oracle, g)
    dev = ivf.device_index()
    qn, qpq, data = g["qn"], g["qpq"], g["data"]
    short = long_ = 0
    # (k = 100: the one size at which every fixture, eu20 too, has queries whose heap holds <= k ids)
    for n_probes in (1, 2, 5, 10):
        for k in (1, 10, 50, 100):
            ids, dist = dev.query_batch(qn, qpq, k, n_probes, return_distances=True)
            np.testing.assert_array_equal(ids, dev.query_batch(qn, qpq, k, n_probes))
            np.testing.assert_array_equal(ids, ox.query_batch(qn, k, n_probes))
            _check_dists(oracle, qn, data, ids, dist)
            for i in range(len(qn)):
                _, dbg = ox.query(qn[i], k, n_probes, debug=True)
                held = int((dbg["heap_idx"] != -1).sum())
                if held > k:
                    long_ += 1
                    assert (np.diff(dist[i].astype(np.float64)) >= 0).all(), (n_probes, k, i)
                else:
                    short += 1
    assert short > 0 and long_ > 0, (short, long_)     # both branches of the rescoring ran


def test_every_rescore_form_and_heap_mode_agree(tk, oracle):
    from tinyknn_amd import _lib
    g = golden("g6_ivf_an100.npz")
    ivf = _fixture_ivf(g)
    dev = ivf.device_index()
    qn, qpq = g["qn"], g["qpq"]
    for n_probes in (1, 2, 5, 10):
        for k in (1, 10, 50):
            base = None
            for form in (0, 1, 2):
                for mode in (0, 1, 2, 3):
                    dev.set_option(_lib.OPT_RESCORE_FORM, form)
                    dev.set_heap_mode(mode)
                    got = dev.query_batch(qn, qpq, k, n_probes, return_distances=True)
                    np.testing.assert_array_equal(got[0], dev.query_batch(qn, qpq, k, n_probes))
                    if base is None:
                        base = got
                        _check_dists(oracle, qn, g["data"], got[0], got[1])
                    else:
                        np.testing.assert_array_equal(got[0], base[0], err_msg=f"form {form} mode {mode}")
                        np.testing.assert_array_equal(got[1], base[1], err_msg=f"form {form} mode {mode}")
    dev.set_option(_lib.OPT_RESCORE_FORM, 2)
    dev.set_heap_mode(0)


@pytest.mark.parametrize("tag", ["an100", "eu20f64"])
def test_allowed_sets_host_and_device(tk, oracle, tag):
    import torch
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = _fixture_ivf(g)
    ox = _oracle_index(oracle, g)
    dev = ivf.device_index()
    qn, qpq, data = g["qn"], g["qpq"], g["data"]
    N = len(data)
    f64 = qpq.dtype != np.float32
    tdt = torch.float64 if data.dtype == np.float64 else torch.float32
    q_dev, qp_dev = torch.from_numpy(np.ascontiguousarray(qn)).cuda(), torch.from_numpy(np.ascontiguousarray(qpq)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for n_probes in (1, 5, 10):
        for i, sel in enumerate((0.5, 0.01)):
            allowed = np.random.default_rng(10 * n_probes + i).random(N) < sel
            want = guarded_batch(oracle, ox, qn, 10, n_probes, allowed=allowed)
            aset = dev.allow(allowed)
            ids, dist = dev.query_batch(qn, qpq, 10, n_probes, allowed=aset, return_distances=True)
            np.testing.assert_array_equal(ids, want)
            _check_dists(oracle, qn, data, ids, dist)
            ids2, dist2 = dev.query_batch(qn, qpq, 10, n_probes, allowed=allowed, return_distances=True)
            np.testing.assert_array_equal(ids2, want)
            np.testing.assert_array_equal(dist2, dist)
            o = torch.full((len(qn), 10), -7, dtype=torch.int64, device="cuda")
            od = torch.full((len(qn), 10), -7, dtype=tdt, device="cuda")
            dev.query_batch_dev(q_dev.data_ptr(), qp_dev.data_ptr(), f64, len(qn), 10, n_probes, o.data_ptr(),
                                stream=st, allowed=aset, dist_ptr=od.data_ptr())
            dev.join(st)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(o.cpu().numpy(), want)
            np.testing.assert_array_equal(od.cpu().numpy(), dist)
            aset.close()


@pytest.fixture(scope="module")
def synth(tk, oracle):
    from tinyknn_amd import IVF, FastPQ
    np.random.seed(11)
    n, nq, d = 40000, 1800, 100
    cent = np.random.randn(200, d)
    X = (cent[np.random.randint(200, size=n)] + 0.6 * np.random.randn(n, d)).astype(np.float32)
    qs = (cent[np.random.randint(200, size=nq)] + 0.6 * np.random.randn(nq, d)).astype(np.float32)
    ivf = IVF("angular", 180, FastPQ(2))
    ivf.fit(X[:15000]).build(X, n_probes=1)
    qn, qp = ivf._prepare(qs.copy())
    return ivf, qn, np.ascontiguousarray(qp)


def test_pipelined_pairs_mixing_calls_with_and_without_distances(synth, oracle):
    import torch
    ivf, qn, qp = synth
    dev = ivf.device_index()
    want = {p: dev.query_batch(qn, qp, 10, p, return_distances=True) for p in (3, 10)}
    _check_dists(oracle, qn[:200], ivf.data, want[10][0][:200], want[10][1][:200])
    dev.set_pipeline(3)
    dev.set_coalesce(2)
    st = torch.cuda.current_stream().cuda_stream
    q_dev, qp_dev = torch.from_numpy(qn).cuda(), torch.from_numpy(qp).cuda()
    d, dq = qn.shape[1], qp.shape[1]
    esz = qp.dtype.itemsize
    f64 = qp.dtype != np.float32
    # (rows, n_probes, distances?) — pairs (0,1): with + without, (2,3): without + with, (4,5): both, call 6 held
    # and launched alone (other n_probes behind it), (7,8): neither, call 9 alone at the join
    calls = [((0, 900), 10, True), ((900, 1800), 10, False), ((0, 300), 10, False), ((300, 600), 10, True),
             ((600, 1001), 10, True), ((1001, 1400), 10, True), ((1400, 1800), 10, True),
             ((0, 700), 3, False), ((700, 1400), 3, False), ((1400, 1800), 3, True)]
    SENT = -7.0
    outs, dists = [], []
    for rep in range(2):
        for (a, b), p, wd in calls:
            o = torch.full((b - a, 10), -7, dtype=torch.int64, device="cuda")
            od = torch.full((b - a, 10), SENT, dtype=torch.float32, device="cuda")
            outs.append(o)
            dists.append(od)
            dev.query_batch_dev(q_dev.data_ptr() + a * d * 4, qp_dev.data_ptr() + a * dq * esz, f64, b - a, 10, p,
                                o.data_ptr(), stream=st, dist_ptr=od.data_ptr() if wd else None)
    dev.join(st)
    torch.cuda.synchronize()
    for j, (((a, b), p, wd), o, od) in enumerate(zip(calls * 2, outs, dists)):
        np.testing.assert_array_equal(o.cpu().numpy(), want[p][0][a:b], err_msg=f"call {j}")
        if wd:
            np.testing.assert_array_equal(od.cpu().numpy(), want[p][1][a:b], err_msg=f"call {j}")
        else:
            assert (od.cpu().numpy() == SENT).all(), f"call {j} asked for no distances"
    dev.set_coalesce(1)
    dev.set_pipeline(1)


def test_single_query_returns_arrays_of_one_length(synth, oracle):
    ivf, qn, qp = synth
    shorter = 0
    for i in range(0, 60, 3):
        for k, p in ((10, 1), (10, 5), (500, 1)):
            # (the preparation normalises a float32 row in place, as the reference does: every call gets a copy)
            ids, dist = ivf.query(qn[i].copy(), k, n_probes=p, return_distances=True)
            np.testing.assert_array_equal(ids, ivf.query(qn[i].copy(), k, n_probes=p))
            assert len(ids) == len(dist) and dist.dtype == np.float32
            shorter += len(ids) < k
            _check_dists(oracle, ivf._prepare(qn[i][None, :].copy())[0], ivf.data, ids[None, :], dist[None, :])
    assert shorter > 0          # fewer candidates than k: the variable-length arrays
    # the batch form with and without distances
    ids, dist = ivf.query_batch(qn[:50], 10, n_probes=5, return_distances=True)
    np.testing.assert_array_equal(ids, ivf.query_batch(qn[:50], 10, n_probes=5))
    with pytest.raises(NotImplementedError):
        ivf.query_batch(qn[:5], 10, n_probes=5, fast=True, return_distances=True)


def test_after_add_and_remove(tk, oracle):
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(4)
    d = 100
    cent = rng.randn(40, d)
    X = (cent[rng.randint(40, size=6000)] + 0.6 * rng.randn(6000, d)).astype(np.float32)
    Y = (cent[rng.randint(40, size=1500)] + 0.6 * rng.randn(1500, d)).astype(np.float32)
    ivf = IVF("euclidean", 60, FastPQ(2))
    ivf.fit(X[:4000]).build(X, n_probes=1)
    ivf.add(Y)
    gone = np.arange(0, 7500, 5)
    ivf.remove(gone)
    qs = np.concatenate([Y[:100], X[1:200:2]]).astype(np.float32)
    ids, dist = ivf.query_batch(qs, 10, n_probes=5, return_distances=True)
    np.testing.assert_array_equal(ids, ivf.query_batch(qs, 10, n_probes=5))
    assert not np.isin(ids, gone).any()
    assert (ids >= 6000).sum() > 100        # rows the add appended are found, with their distances
    qn = ivf._prepare(qs.copy())[0]
    _check_dists(oracle, qn, ivf.data, ids, dist)


def _oracle_top(O, pq, td, X, q, k):
    rescore = min(2 * k + 10, td.size)
    idx = np.zeros(rescore, np.int64)
    val = np.zeros(rescore, np.int32)
    O.init_heap(idx, val, True)
    O.query_pq(td.packed, td.size, pq.distance_table(q).tables, idx, val, True, None, O.ORDER_AVX)
    if rescore <= k:
        return idx
    return idx[O.knn_brute1(q, X[idx], k)]


# the shapes of test_flat_top_gpu, and a heap beyond the lane replay's limit (2k + 10 > 574: the general replay
# and coarse_replay_probes)
@pytest.mark.parametrize("n,d,k", [(5003, 100, 10), (20000, 128, 10), (37, 100, 10), (9, 100, 10), (3000, 100, 1),
                                   (5003, 100, 300)])
def test_flat_top_distances(tk, oracle, n, d, k):
    from tinyknn_amd import FastPQ
    from tinyknn_amd.fast_pq import FlatTop
    rng = np.random.RandomState(n)
    cent = rng.randn(12, d)
    X = (cent[rng.randint(12, size=n)] + 0.6 * rng.randn(n, d)).astype(np.float32)
    qs = (cent[rng.randint(12, size=70)] + 0.6 * rng.randn(70, d)).astype(np.float32)
    pq = FastPQ(2)
    pq.fit(X[:3000] if n >= 3000 else np.concatenate([X] * (3000 // n + 1)))
    td = pq.transform(X)
    ft = FlatTop(pq, td, X)
    ids, dist = ft.top(qs, k, return_distances=True)
    np.testing.assert_array_equal(ids, ft.top(qs, k))
    assert ids.shape == dist.shape == (70, min(k, n))
    _check_dists(oracle, qs, X, ids, dist)
    for i in range(0, 70, 7):
        np.testing.assert_array_equal(ids[i], _oracle_top(oracle, pq, td, X, qs[i], min(k, n)))
    ft.close()


def test_flat_top_distances_long_rows(tk, oracle):
    """n >= 2^16 rows: the plain scan on the matrix cores behind the exact head, then the lane replay + rescoring"""
    from tinyknn_amd import FastPQ
    from tinyknn_amd.fast_pq import FlatTop
    d, nq, k = 100, 200, 10
    n = 70000 + d
    rng = np.random.RandomState(d + 1)
    cent = rng.randn(40, d)
    X = (cent[rng.randint(40, size=n)] + 0.5 * rng.randn(n, d)).astype(np.float32)
    qs = (cent[rng.randint(40, size=nq)] + 0.5 * rng.randn(nq, d)).astype(np.float32)
    pq = FastPQ(2)
    pq.fit(X[:4000])
    td = pq.transform(X, device=True)
    ft = FlatTop(pq, td, X)
    for rep in range(2):
        ids, dist = ft.top(qs, k, return_distances=True)
        np.testing.assert_array_equal(ids, ft.top(qs, k))
        _check_dists(oracle, qs, X, ids, dist)
        for i in range(0, nq, 19):
            np.testing.assert_array_equal(ids[i], _oracle_top(oracle, pq, td, X, qs[i], k))
    ft.close()


CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from tinyknn_amd import IVF, FastPQ, _lib
from oracle import oracle
assert _lib.device_count() >= 1, "no GPU visible"
np.random.seed(5)
n, d, nq0 = 40000, 48, 1500
cent = np.random.randn(150, d)
X = (cent[np.random.randint(150, size=n)] + 0.6 * np.random.randn(n, d)).astype(np.float32)
qs = (cent[np.random.randint(150, size=nq0)] + 0.6 * np.random.randn(nq0, d)).astype(np.float32)
ivf = IVF("euclidean", 160, FastPQ(2))
ivf.fit(X[:15000]).build(X, n_probes=1)
L = len(ivf.active_centers)
ox = oracle.OracleIndex(ivf.pq.centers, 2, ivf.pq.R, ivf.pq.sqrt_n_blocks, ivf.active_centers,
                        ivf.pq_transformed_centers.packed,
                        [ivf.pq_transformed_points[i].packed for i in range(L)],
                        [ivf.pq_transformed_points[i].size for i in range(L)],
                        [ivf.ids[i] for i in range(L)], ivf.data)
qn0, qp0 = ivf._prepare(qs.copy())
k, n_probes = 10, 100
want0 = ox.query_batch(qn0, k, n_probes)
wd0 = np.full(want0.shape, np.inf)
for i in range(nq0):
    live = want0[i] != -1
    wd0[i, live] = oracle.sqdist_gather(qn0[i], ivf.data, want0[i][live])
dev = ivf.device_index()
ms = dev.max_sub_batch(k, n_probes)
reps = -(-(2 * ms + 5) // nq0)
sel = np.concatenate([np.random.permutation(nq0) for _ in range(reps)])[:2 * ms + 5]     # three parts
qn, qp, want, wd = np.ascontiguousarray(qn0[sel]), np.ascontiguousarray(qp0[sel]), want0[sel], wd0[sel]
nq = len(qn)
assert ms < nq <= 3 * ms, (ms, nq)
ids, dist = dev.query_batch(qn, qp, k, n_probes, return_distances=True)
assert (ids == want).all() and (dist.astype(np.float64) == wd).all(), "host call"
st = torch.cuda.current_stream().cuda_stream
q_dev, qp_dev = torch.from_numpy(qn).cuda(), torch.from_numpy(qp).cuda()
f64 = qp.dtype != np.float32
for depth, co in ((1, 1), (2, 1), (2, 2)):
    dev.set_pipeline(depth)
    dev.set_coalesce(co)
    out = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    od = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    dev.query_batch_dev(q_dev.data_ptr(), qp_dev.data_ptr(), f64, nq, k, n_probes, out.data_ptr(), stream=st,
                        dist_ptr=od.data_ptr())
    dev.join(st)
    torch.cuda.synchronize()
    got, gd = out.cpu().numpy(), od.cpu().numpy().astype(np.float64)
    bad = int((got != want).any(axis=1).sum()) + int((gd != wd).any(axis=1).sum())
    assert bad == 0, (depth, co, bad)
dev.set_pipeline(1)
print("SUB_BATCH_DIST_OK", ms, nq)
'''


def test_distances_of_a_batch_beyond_one_workspace(tmp_path):
    root = os.path.dirname(HERE)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, TINYKNN_WORKSPACE_GB="0.25")
    r = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SUB_BATCH_DIST_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
