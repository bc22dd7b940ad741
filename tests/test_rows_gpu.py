"""Stored rows as queries and one excluded row per query on the device (rows.hip: tk_index_query_batch[_dev]_ex2,
tk_index_gather_queries[_dev], tk_index_query_rows; IVF.query_rows / knn_graph).  Every comparison is exact: ids and,
through debug=True, probes and heap arrays against tests/rows_reference.py — the guarded reference with the allowed
set "every row but e", fed the device-made q_pq where the PQ is rotated."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from allowed_reference import guarded_batch, reference_index  # noqa: E402
from conftest import G6_TAGS, golden  # noqa: E402
from rows_reference import excluded_batch  # noqa: E402
from store_reference import fixture_ivf, oracle_index, rounded  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("probes", "heap_idx", "heap_val")


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    return tinyknn_amd


def _same(got, gd, want, wd, msg=""):
    np.testing.assert_array_equal(got, want, err_msg=str(msg))
    for key in KEYS:
        np.testing.assert_array_equal(gd[key], wd[key], err_msg=f"{key} {msg}")


def _fixture_rows(g):
    """Of every list the rows at positions 0, 15, 16 and last where they exist, plus 24 random rows."""
    sizes = np.asarray(g["list_sizes"], dtype=np.int64)
    ioff = np.concatenate([[0], np.cumsum(sizes)])
    rows = [int(g["ids"][ioff[l] + p]) for l, n in enumerate(sizes) for p in (0, 15, 16, n - 1) if 0 <= p < n]
    rows += np.random.default_rng(len(sizes)).choice(len(g["data"]), 24, replace=False).tolist()
    return np.asarray(rows, dtype=np.int64)


def _rows_against_reference(oracle, dev, ox, data32, rows, probe_counts, k=10):
    """query_rows / gather_queries / exclude= of `dev` on `rows`, against the reference on `ox` fed data32[rows]."""
    qn, qp = dev.gather_queries(rows)
    want_qn = np.ascontiguousarray(data32[rows], dtype=np.float32)
    assert np.array_equal(qn.view(np.uint32), want_qn.view(np.uint32)), "qn != float32(data[rows])"
    assert qp.dtype == (np.float64 if dev.rotated() else np.float32)
    if not dev.rotated():       # unrotated: q_pq is qn padded, the reference is fed qn alone
        assert np.array_equal(qp[:, :dev.d], qn) and not qp[:, dev.d:].any()
    for n_probes in probe_counts:
        want, wd = excluded_batch(oracle, ox, qn, rows, k, n_probes, q_pq=qp if dev.rotated() else None, debug=True)
        got, gd = dev.query_rows(rows, k, n_probes, debug=True)
        _same(got, gd, want, wd, n_probes)
        assert not (got == rows[:, None]).any(), "a row returned itself"
        # the same through the external-query call, and without the exclusion
        np.testing.assert_array_equal(dev.query_batch(qn, qp, k, n_probes, exclude=rows), got)
        np.testing.assert_array_equal(dev.query_rows(rows, k, n_probes, exclude_self=False),
                                      dev.query_batch(qn, qp, k, n_probes))
    return qn, qp


@pytest.mark.parametrize("tag", G6_TAGS)
def test_fixtures_rows_of_every_list(tk, oracle, tag):
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = fixture_ivf(g)
    ox = oracle_index(oracle, ivf, g["data"])
    dev = ivf.device_index()
    rows = _fixture_rows(g)
    assert dev.row_table()["builds"] == 0
    _rows_against_reference(oracle, dev, ox, np.asarray(g["data"]).astype(np.float32), rows, (1, 5, 10))
    t = dev.row_table()
    assert t["built"] and t["builds"] == 1 and t["entries"] == len(g["ids"])
    assert t["bytes"] == 4 * (len(g["data"]) + 2) + 4 * len(g["ids"])


def test_half_store(tk, oracle):
    g = golden("g6_ivf_an100.npz")
    ivf = fixture_ivf(g, store="float16")
    data = rounded(g["data"])
    ox = oracle_index(oracle, ivf, data)
    dev = ivf.device_index()
    assert dev.store == "float16"
    _rows_against_reference(oracle, dev, ox, data, _fixture_rows(g), (1, 5, 10))


def _small_index(tk):
    np.random.seed(11)
    X = np.random.randn(300, 16).astype(np.float32)
    X[7] = X[3]
    ivf = tk.IVF("euclidean", 3, tk.FastPQ(2))
    ivf.fit(X).build(X, n_probes=1)
    return ivf, X


def test_equal_vectors_and_a_list_of_one_row(tk, oracle):
    ivf, X = _small_index(tk)
    ids, dist = ivf.query_rows([3, 7], 10, n_probes=3, return_distances=True)
    assert ids[0, 0] == 7 and dist[0, 0] == 0 and ids[1, 0] == 3 and dist[1, 0] == 0
    assert 3 not in ids[0] and 7 not in ids[1]
    ox = reference_index(ivf)
    dev = ivf.device_index()
    rows = np.arange(0, 300, 7)
    _rows_against_reference(oracle, dev, ox, X, np.concatenate([[3, 7], rows]), (1, 3))
    # a list cut down to its first row, that row's own first probe: as the query it leaves an all-empty chunk
    # (minimum byte 127).  The coarse stage reads the centres alone, so cutting a list leaves the probes as they are.
    first = np.asarray([int(x[0]) for x in ivf.ids])
    own = np.flatnonzero(dev.query_rows(first, 10, 1, debug=True)[1]["probes"][:, 0] == np.arange(len(first)))
    assert own.size > 0
    cut = int(own[0])
    one = tk.IVF("euclidean", 3, tk.FastPQ(2))
    one.all_centers, one.pq, one.data = ivf.all_centers, ivf.pq, ivf.data
    one.active_centers, one.pq_transformed_centers = ivf.active_centers, ivf.pq_transformed_centers
    one.ids = [np.asarray(x) for x in ivf.ids]
    one.pq_transformed_points = list(ivf.pq_transformed_points)
    one.ids[cut] = one.ids[cut][:1]
    one.pq_transformed_points[cut] = one.pq.transform(one.data[one.ids[cut]])
    lone = int(one.ids[cut][0])
    ox1 = reference_index(one)
    dev1 = one.device_index()
    rows1 = np.asarray([lone] + [int(one.ids[l][-1]) for l in range(3) if l != cut])
    _rows_against_reference(oracle, dev1, ox1, X, rows1, (1, 2, 3))
    got, gd = dev1.query_rows([lone], 10, 1, debug=True)
    assert gd["probes"][0, 0] == cut    # its own list is the one probed: nothing else is there
    assert (got == -1).all() and (gd["heap_val"] == 127).all() and (gd["heap_idx"] == -1).all()
    # ... and with every list probed the lone row is in no heap
    got, gd = dev1.query_rows([lone], 10, 3, debug=True)
    assert lone not in gd["heap_idx"] and lone not in got and (got != -1).all()


# ---- every replay form: the synthetic index of test_allowed_gpu.py's SUB_CHILD, built with n_probes 1 and 2 ----

SYN_N, SYN_D, SYN_ROWS = 40000, 48, 256


@pytest.fixture(scope="module")
def synthetic(tk, oracle):
    np.random.seed(5)
    cent = np.random.randn(150, SYN_D)
    X = (cent[np.random.randint(150, size=SYN_N)] + 0.6 * np.random.randn(SYN_N, SYN_D)).astype(np.float32)
    qs = (cent[np.random.randint(150, size=SYN_ROWS)] + 0.6 * np.random.randn(SYN_ROWS, SYN_D)).astype(np.float32)
    base = tk.IVF("euclidean", 160, tk.FastPQ(2, rotate_dim=None))      # unrotated: the reference is fed qn
    base.fit(X[:15000])
    assert base.pq.R is None
    rows = np.random.default_rng(8).choice(SYN_N, SYN_ROWS, replace=False).astype(np.int64)
    made = {}

    def get(kp):
        if kp not in made:
            ivf = tk.IVF("euclidean", 160, None)
            ivf.all_centers, ivf.pq = base.all_centers, base.pq
            ivf.build(X, n_probes=kp)
            ox = reference_index(ivf)
            want = excluded_batch(oracle, ox, X[rows], rows, 10, 10, debug=True)
            made[kp] = (ivf, ox, want)
        return made[kp]
    return get, X, rows, qs


@pytest.mark.parametrize("kp", [1, 2])
def test_every_replay_form(tk, synthetic, kp):
    from tinyknn_amd import _lib
    get, X, rows, _ = synthetic
    ivf, ox, (want, wd) = get(kp)
    dev = ivf.device_index()
    assert (kp == 1) == (dev.twin_table_width() == 0)
    try:
        for heap_mode in (0, 1, 2, 3):
            for plain in (False, "always"):
                for pair_nq in (4, 8192):
                    dev.set_heap_mode(heap_mode)
                    dev.set_plain_scan(plain)
                    dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
                    got, gd = dev.query_rows(rows, 10, 10, debug=True)
                    _same(got, gd, want, wd, (kp, heap_mode, plain, pair_nq))
        # the limit at -128: every query with a plain list fails the lemma's check, is scanned again exactly and masked
        # again through the flag list (exclude_pass_kernel's `only` branch)
        dev.set_heap_mode(0)
        dev.set_plain_scan("always")
        dev.set_option(_lib.OPT_PLAIN_LIMIT, -128)
        for pair_nq in (4, 8192):
            dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
            got, gd = dev.query_rows(rows, 10, 10, debug=True)
            st = dev.plain_stats()
            _same(got, gd, want, wd, (kp, "limit -128", pair_nq, st))
            assert st["plain_units"] > 0 and st["flagged_queries"] > 0, st
    finally:
        dev.set_heap_mode(0); dev.set_plain_scan(True); dev.set_option(_lib.OPT_PAIR_NQ, 4)
        dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)


def test_pipelined_pairs_alternating_kinds(tk, oracle, synthetic):
    import torch
    get, X, rows, qs = synthetic
    ivf, ox, (want_ex, _) = get(1)
    dev = ivf.device_index()
    qn, qp = dev.gather_queries(rows)
    en, ep = ivf._prepare(qs.copy())
    allowed = np.random.default_rng(3).random(SYN_N) < 0.3
    want = dict(ex=want_ex, none=guarded_batch(oracle, ox, qn, 10, 10),
                ex_allow=excluded_batch(oracle, ox, qn, rows, 10, 10, allowed=allowed),
                ex_dist=want_ex, ext=guarded_batch(oracle, ox, en, 10, 10))
    alone = dict(none=dev.query_batch(qn, qp, 10, 10), ext=dev.query_batch(en, ep, 10, 10))
    _, dist_alone = dev.query_batch(qn, qp, 10, 10, exclude=rows, return_distances=True)
    kinds = ["ex", "none", "ex_allow", "ex_dist", "ext", "ex", "ex", "ext", "ex_dist", "none", "none", "ex_allow"]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    qn_d, qp_d, en_d, ep_d, rows_d = cuda(qn), cuda(qp), cuda(en), cuda(ep), cuda(rows)
    outs = [torch.full((SYN_ROWS, 10), -7, dtype=torch.int64, device="cuda") for _ in kinds]
    dists = [torch.full((SYN_ROWS, 10), -7, dtype=torch.float32, device="cuda") for _ in kinds]
    aset = dev.allow(allowed)
    try:
        dev.set_pipeline(3)
        dev.set_coalesce(2)
        torch.cuda.synchronize()
        for kind, out, dist in zip(kinds, outs, dists):
            a, b = (en_d, ep_d) if kind == "ext" else (qn_d, qp_d)
            dev.query_batch_dev(a.data_ptr(), b.data_ptr(), 0, SYN_ROWS, 10, 10, out.data_ptr(),
                                allowed=aset if kind == "ex_allow" else None,
                                dist_ptr=dist.data_ptr() if kind == "ex_dist" else None,
                                exclude_ptr=rows_d.data_ptr() if kind.startswith("ex_") or kind == "ex" else None)
        dev.join()
        torch.cuda.synchronize()
        for i, (kind, out, dist) in enumerate(zip(kinds, outs, dists)):
            got = out.cpu().numpy()
            np.testing.assert_array_equal(got, want[kind], err_msg=f"call {i} {kind}")
            if kind in alone:
                np.testing.assert_array_equal(got, alone[kind], err_msg=f"call {i} {kind} alone")
            if kind == "ex_dist":
                assert np.array_equal(dist.cpu().numpy().view(np.uint32), dist_alone.view(np.uint32))
    finally:
        dev.set_pipeline(1)
        dev.set_coalesce(1)
        aset.close()


def test_device_array_entries_out_of_range_exclude_nothing(tk, synthetic):
    """query_batch_dev does not read exclude_dev on the host: the kernel's guard makes an entry outside [0, N) exclude
    nothing (and read nothing outside the table); the entries in range beside it still exclude."""
    import torch
    get, X, rows, _ = synthetic
    ivf, ox, (want_ex, _) = get(1)
    dev = ivf.device_index()
    qn, qp = dev.gather_queries(rows)
    none = dev.query_batch(qn, qp, 10, 10)
    assert (none != want_ex).any()
    bad = rows.copy()
    bad[0::4], bad[1::4], bad[2::4] = SYN_N, SYN_N + 7, -5
    bad[6::8] = np.iinfo(np.int64).max
    bad[2::8] = np.iinfo(np.int64).min
    expect = np.where(((bad >= 0) & (bad < SYN_N))[:, None], want_ex, none)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    qn_d, qp_d, bad_d = cuda(qn), cuda(qp), cuda(bad)
    out = torch.full((SYN_ROWS, 10), -7, dtype=torch.int64, device="cuda")
    dev.query_batch_dev(qn_d.data_ptr(), qp_d.data_ptr(), 0, SYN_ROWS, 10, 10, out.data_ptr(),
                        exclude_ptr=bad_d.data_ptr())
    dev.join()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), expect)


SUB_CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from tinyknn_amd import IVF, FastPQ, _lib
from oracle import oracle
from allowed_reference import reference_index
from rows_reference import excluded_batch
assert _lib.device_count() >= 1, "no GPU visible"
np.random.seed(5)
n, d, nq0 = 40000, 48, 200
cent = np.random.randn(150, d)
X = (cent[np.random.randint(150, size=n)] + 0.6 * np.random.randn(n, d)).astype(np.float32)
ivf = IVF("euclidean", 160, FastPQ(2))
ivf.fit(X[:15000]).build(X, n_probes=1)
ox = reference_index(ivf)
k, n_probes = 10, 100
rows0 = np.random.default_rng(2).choice(n, nq0, replace=False).astype(np.int64)
dev = ivf.device_index()
qn0, qp0 = dev.gather_queries(rows0)                 # (d = 48 is rotated: the reference is fed the device-made q_pq)
assert dev.rotated() and np.array_equal(qn0, X[rows0])
want0 = excluded_batch(oracle, ox, qn0, rows0, k, n_probes, q_pq=qp0)
ms = dev.max_sub_batch(k, n_probes)
sel = np.arange(2 * ms + 5) % nq0                    # three parts
part = (len(sel) + 2) // 3
assert len(sel) > 2 * ms and part % nq0 != 0         # row i of a part names another row than row i of the call
rows = rows0[sel]
for depth in (1, 3):
    dev.set_pipeline(depth)
    got = dev.query_rows(rows, k, n_probes)
    assert np.array_equal(got, want0[sel]), ("rows differ", depth, np.flatnonzero((got != want0[sel]).any(axis=1))[:5])
    assert not (got == rows[:, None]).any()
print("ok", ms, len(sel))
'''


def test_batch_beyond_one_workspace(tk):
    env = dict(os.environ, TINYKNN_WORKSPACE_GB="0.25")
    r = subprocess.run([sys.executable, "-c", SUB_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("kp", [1, 2])
def test_after_add_and_after_remove(tk, oracle, kp):
    from test_remove_gpu import SEED, SIGMA, _fitted, _host_index, _oracle_of
    from tinyknn_amd.ivf import synth_rows
    d, N0 = 100, 3000
    ivf = _host_index("angular", d, kp, N=N0)
    dev = ivf.device_index()
    rng = np.random.default_rng(kp)
    rows = rng.choice(N0, 96, replace=False).astype(np.int64)
    _rows_against_reference(oracle, dev, _oracle_of(oracle, ivf), ivf.data, rows, (5,))
    assert dev.row_table()["builds"] == 1
    # add: the new rows are queries and neighbours, the table is made again
    ivf.add(synth_rows(500, d, SEED, _fitted("angular", d)[2], SIGMA, row0=N0))
    assert ivf.device_index() is dev and dev.N == N0 + 500 and not dev.row_table()["built"]
    rows = np.concatenate([rows[:48], np.arange(N0, N0 + 500, 9)])
    _rows_against_reference(oracle, dev, _oracle_of(oracle, ivf), ivf.data, rows, (5,))
    assert dev.row_table()["builds"] == 2
    # remove: a removed row is still a query row; nothing of it is stored, so nothing is masked
    dead = np.concatenate([rows[::3], rng.choice(N0, 300, replace=False)])
    ivf.remove(dead)
    assert not dev.row_table()["built"]
    ox = _oracle_of(oracle, ivf)
    qn, qp = _rows_against_reference(oracle, dev, ox, ivf.data, rows, (5,))
    assert dev.row_table()["builds"] == 3
    gone = rows[::3]
    np.testing.assert_array_equal(dev.query_rows(gone, 10, 5), dev.query_batch(qn[::3], qp[::3], 10, 5))
    np.testing.assert_array_equal(dev.query_rows(gone, 10, 5), guarded_batch(oracle, ox, qn[::3], 10, 5))


def test_knn_graph(tk, oracle):
    g = golden("g6_ivf_an100.npz")
    ivf = fixture_ivf(g)
    N = len(g["data"])
    dev = ivf.device_index()
    dev.set_pipeline(2)
    ids, dist = ivf.knn_graph(10, n_probes=5, chunk=333, return_distances=True)
    assert dev.pipeline_settings() == (2, 1)     # (the library's own state)
    dev.set_pipeline(1)
    assert ids.shape == (N, 10) and dist.shape == (N, 10)
    want, wdist = ivf.query_rows(np.arange(N), 10, n_probes=5, return_distances=True)
    np.testing.assert_array_equal(ids, want)
    assert np.array_equal(dist.view(np.uint32), wdist.view(np.uint32))
    np.testing.assert_array_equal(ivf.knn_graph(10, n_probes=5, chunk=333), want)
    assert not (ids == np.arange(N)[:, None]).any()
    # more than k candidates: rescored order
    _, dbg = dev.query_rows(np.arange(N), 10, 5, debug=True)
    many = (dbg["heap_idx"] != -1).sum(axis=1) > 10
    assert many.sum() > N // 2 and (np.diff(dist[many], axis=1) >= 0).all()
    # and a sample against the reference
    ox = oracle_index(oracle, ivf, g["data"])
    sample = np.arange(0, N, 40)
    np.testing.assert_array_equal(ids[sample], excluded_batch(oracle, ox, g["data"][sample], sample, 10, 5))


def test_refusals_and_no_table_without_exclusion(tk):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    from tinyknn_amd.multi_gpu import shard_lists
    g = golden("g6_ivf_an100.npz")
    ivf = fixture_ivf(g)
    dev = ivf.device_index()
    qn, qp, N = g["qn"], g["qpq"], len(g["data"])
    nq = len(qn)
    out = np.zeros((nq, 10), dtype=np.int64)

    def ex2(d, exclude):
        ex = np.ascontiguousarray(exclude, dtype=np.int64)
        return _lib.lib().tk_index_query_batch_ex2(
            d.handle, None, ex.ctypes.data, _lib.ptr(np.ascontiguousarray(qn), _lib._f32p), qp.ctypes.data, 0, nq, 10, 5,
            0, _lib.ptr(out, _lib._i64p), None, None, None, None)
    plain = dev.query_batch(qn, qp, 10, 5)
    # all -1: the unrestricted rows, and no table
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, exclude=np.full(nq, -1)), plain)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, debug=True)[0], plain)
    assert dev.row_table() == dict(built=False, bytes=0, builds=0, entries=0)
    # an entry >= N, below -1: refused by the library, nothing run
    for bad in (N, N + 7, -2):
        out[:] = -9
        e = np.full(nq, -1)
        e[nq // 2] = bad
        with pytest.raises(AssertionError, match="exclude"):
            _lib.check(ex2(dev, e))
        assert (out == -9).all() and dev.row_table()["builds"] == 0
    # one real entry: only that query changes
    e = np.full(nq, -1)
    e[0] = plain[0, 0]
    got = dev.query_batch(qn, qp, 10, 5, exclude=e)
    np.testing.assert_array_equal(got[1:], plain[1:])
    assert plain[0, 0] not in got[0] and dev.row_table()["builds"] == 1
    # a list-sharded index
    owner = shard_lists(np.asarray(g["list_sizes"], dtype=np.int64), 2)
    shard = DeviceIndex(fixture_ivf(g), owner, 0, 2)
    try:
        with pytest.raises(AssertionError, match="list-sharded"):
            _lib.check(ex2(shard, e))
        with pytest.raises(AssertionError, match="list-sharded"):
            shard.query_rows(np.arange(4), 10, 5)
    finally:
        shard.close()
