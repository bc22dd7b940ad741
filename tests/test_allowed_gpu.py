"""Allowed sets on the device (allow.hip, tk_index_query_batch[_dev]_allow): every result equals the guarded reference
(tests/allowed_reference.py: the oracle's query with `insert` only for allowed labels) bit for bit — ids and, through
debug=True, probes and heap arrays."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from allowed_reference import guarded_batch, guarded_query  # noqa: E402
from conftest import G6_TAGS, golden, split_lists  # noqa: E402

pytestmark = pytest.mark.gpu

SELECTIVITIES = (1.0, 0.5, 0.1, 0.01, 0.0)


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


def _mask(N, sel, seed):
    return np.random.default_rng(seed).random(N) < sel


def _check(got, gd, want, wd, allowed):
    np.testing.assert_array_equal(got, want)
    for key in ("probes", "heap_idx", "heap_val"):
        np.testing.assert_array_equal(gd[key], wd[key], err_msg=key)
    ids = got[got != -1]
    assert allowed[ids].all(), "an id outside the allowed set"


@pytest.mark.parametrize("tag", G6_TAGS)
def test_fixtures_every_probe_count_and_selectivity(tk, oracle, tag):
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = _fixture_ivf(g)
    ox = _oracle_index(oracle, g)
    dev = ivf.device_index()
    N = len(g["data"])
    for n_probes in (1, 2, 5, 10):
        for i, sel in enumerate(SELECTIVITIES):
            allowed = _mask(N, sel, 100 * n_probes + i)
            want, wd = guarded_batch(oracle, ox, g["qn"], 10, n_probes, allowed=allowed, debug=True)
            aset = dev.allow(allowed)
            assert len(aset) == int(allowed[np.concatenate(ivf.ids)].sum())
            got, gd = dev.query_batch(g["qn"], g["qpq"], 10, n_probes, debug=True, allowed=aset)
            _check(got, gd, want, wd, allowed)
            # the mask and the ids directly, one set made and freed per call
            np.testing.assert_array_equal(dev.query_batch(g["qn"], g["qpq"], 10, n_probes, allowed=allowed), want)
            np.testing.assert_array_equal(
                dev.query_batch(g["qn"], g["qpq"], 10, n_probes, allowed=np.flatnonzero(allowed)), want)
            if sel == 1.0:      # all allowed: the unrestricted results exactly
                np.testing.assert_array_equal(got, dev.query_batch(g["qn"], g["qpq"], 10, n_probes))
            aset.close()


def test_ivf_query_returns_the_variable_length_array(tk, oracle):
    g = golden("g6_ivf_an100.npz")
    ivf = _fixture_ivf(g)
    ox = _oracle_index(oracle, g)
    allowed = _mask(len(g["data"]), 0.01, 3)
    aset = ivf.allow(allowed)
    lengths = []
    for qi in range(len(g["qn"])):
        q = np.array(g["qn"][qi], copy=True)
        qn, _ = ivf._prepare(q[None, :].copy())
        want = guarded_query(oracle, ox, qn[0], 10, 5, allowed=allowed)
        got = ivf.query(q, 10, n_probes=5, allowed=aset)
        np.testing.assert_array_equal(got, want)
        lengths.append(len(got))
    assert min(lengths) < 10        # the early return (ivf.py:154-156) is taken
    np.testing.assert_array_equal(ivf.query_batch(g["qn"], 10, n_probes=5, allowed=aset),
                                  guarded_batch(oracle, ox, ivf._prepare(np.array(g["qn"], copy=True))[0], 10, 5,
                                                allowed=allowed))
    with pytest.raises(NotImplementedError):
        ivf.query_batch(g["qn"], 10, n_probes=5, fast=True, allowed=aset)
    aset.close()


def test_stale_set_is_refused(tk):
    from tinyknn_amd import _lib
    g = golden("g6_ivf_eu20.npz")
    ivf = _fixture_ivf(g)
    dev = ivf.device_index()
    aset = dev.allow(_mask(len(g["data"]), 0.5, 1))
    dev.query_batch(g["qn"], g["qpq"], 10, 2, allowed=aset)
    # the lists set again (same content, a new layout as far as the set knows)
    codes, ids = split_lists(g)
    sizes = np.ascontiguousarray(g["list_sizes"], dtype=np.int64)
    packed = np.ascontiguousarray(np.concatenate([c for c in codes if len(c)]), dtype=np.uint64)
    allids = np.ascontiguousarray(np.concatenate(ids), dtype=np.int64)
    _lib.check(_lib.lib().tk_index_set_lists(dev.handle, _lib.ptr(sizes, _lib._i64p), _lib.ptr(packed, _lib._u64p),
                                             _lib.ptr(allids, _lib._i64p)))
    with pytest.raises(_lib.TinyKnnHipError, match="earlier layout"):
        dev.query_batch(g["qn"], g["qpq"], 10, 2, allowed=aset)
    aset.close()
    fresh = dev.allow(_mask(len(g["data"]), 0.5, 1))
    dev.query_batch(g["qn"], g["qpq"], 10, 2, allowed=fresh)
    fresh.close()


# ---- the GloVe-shaped index bench.py measures ----

@pytest.fixture(scope="module")
def full(tk, oracle):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    args = argparse.Namespace(n=1183514, d=100, n_clusters=1087, seed=10, build_probes=1,
                              metric="angular", data="glove-like", fit_sample=100000,
                              cache_dir=os.environ.get("TMPDIR", "/tmp"))
    ivf, cent = bench.build_index(args, torch.device("cuda", 0))
    qs = bench.synth_queries(cent, 1024, 777, kind="glove-like")
    ox = bench.oracle_index(ivf)
    qn, qp = ivf._prepare(qs.copy())
    N = ivf.data.shape[0]
    # random sets and one cluster-correlated set (whole lists)
    lists = np.random.default_rng(9).permutation(len(ivf.ids))[:len(ivf.ids) // 10]
    clustered = np.zeros(N, dtype=bool)
    clustered[np.concatenate([ivf.ids[i] for i in lists])] = True
    sets = dict(r10=_mask(N, 0.1, 11), r01=_mask(N, 0.01, 12), c10=clustered)
    want = {name: guarded_batch(oracle, ox, qn, 10, 10, allowed=m, debug=True) for name, m in sets.items()}
    return ivf, ox, qn, qp, sets, want


def test_full_size_every_mode(full):
    from tinyknn_amd import _lib
    ivf, ox, qn, qp, sets, want = full
    dev = ivf.device_index()
    asets = {name: dev.allow(m) for name, m in sets.items()}
    try:
        for heap_mode in (0, 1, 2, 3):
            for plain in (False, "always", True):
                for pair_nq in (4, 8192):
                    if heap_mode != 0 and (plain is not True or pair_nq != 4):
                        continue
                    dev.set_heap_mode(heap_mode)
                    dev.set_plain_scan(plain)
                    dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
                    for name, aset in asets.items():
                        got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, allowed=aset)
                        w, wd = want[name]
                        bad = np.flatnonzero((got != w).any(axis=1))
                        assert bad.size == 0, (heap_mode, plain, pair_nq, name, bad[:5])
                        _check(got, gd, w, wd, sets[name])
        # the limit at -128: every query with a plain list fails the lemma's check, is scanned again exactly and masked
        # again through the flag list (allow_pass_kernel's `only` branch)
        dev.set_heap_mode(0)
        dev.set_plain_scan("always")
        dev.set_option(_lib.OPT_PAIR_NQ, 4)
        dev.set_option(_lib.OPT_PLAIN_LIMIT, -128)
        for name, aset in asets.items():
            got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, allowed=aset)
            st = dev.plain_stats()
            w, wd = want[name]
            _check(got, gd, w, wd, sets[name])
            assert st["plain_units"] > 0 and st["flagged_queries"] > 0, (name, st)
    finally:
        dev.set_heap_mode(0); dev.set_plain_scan(True); dev.set_option(_lib.OPT_PAIR_NQ, 4)
        dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
        for a in asets.values():
            a.close()


def test_full_size_pipelined_pairs_alternating_sets(full):
    import torch
    from tinyknn_amd import _lib
    ivf, ox, qn, qp, sets, want = full
    dev = ivf.device_index()
    names = ["r10", None, "r01", "c10", None, "r10", "r10", "c10", None, None, "r01", "r01"]
    asets = {name: dev.allow(m) for name, m in sets.items()}
    unrestricted = dev.query_batch(qn, qp, 10, 10)
    qn_d = torch.from_numpy(np.ascontiguousarray(qn)).cuda()
    qp_d = torch.from_numpy(np.ascontiguousarray(qp)).cuda()
    outs = [torch.full((len(qn), 10), -7, dtype=torch.int64, device="cuda") for _ in names]
    try:
        dev.set_pipeline(3)
        dev.set_coalesce(2)
        torch.cuda.synchronize()
        for name, out in zip(names, outs):
            dev.query_batch_dev(qn_d.data_ptr(), qp_d.data_ptr(), int(qp.dtype != np.float32), len(qn), 10, 10,
                                out.data_ptr(), allowed=None if name is None else asets[name])
        dev.join()
        torch.cuda.synchronize()
        for name, out in zip(names, outs):
            exp = unrestricted if name is None else want[name][0]
            np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg=str(name))
        # destroying a set with calls pending waits for them; their results stay right
        for out in outs[:2]:
            out.fill_(-7)
            dev.query_batch_dev(qn_d.data_ptr(), qp_d.data_ptr(), int(qp.dtype != np.float32), len(qn), 10, 10,
                                out.data_ptr(), allowed=asets["r01"])
        assert _lib.lib().tk_index_pending(dev.handle) > 0
        asets.pop("r01").close()
        dev.join()
        torch.cuda.synchronize()
        for out in outs[:2]:
            np.testing.assert_array_equal(out.cpu().numpy(), want["r01"][0])
    finally:
        dev.set_pipeline(1)
        dev.set_coalesce(1)
        for a in asets.values():
            a.close()


def test_plain_state_untouched_by_restricted_calls(full):
    ivf, ox, qn, qp, sets, want = full
    dev = ivf.device_index()
    dev.set_plain_scan(True)
    for _ in range(4):              # the unrestricted traffic settles the automatic state
        dev.query_batch(qn, qp, 10, 10)
    before = dev.plain_stats()["state"], dev.plain_stats()["pause_left"]
    aset = dev.allow(sets["r01"])
    try:
        for _ in range(40):
            got = dev.query_batch(qn, qp, 10, 10, allowed=aset)
        np.testing.assert_array_equal(got, want["r01"][0])
        st = dev.plain_stats()
        assert (st["state"], st["pause_left"]) == before, (st, before)
    finally:
        aset.close()


SUB_CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from tinyknn_amd import IVF, FastPQ, _lib
from oracle import oracle
from allowed_reference import guarded_batch
assert _lib.device_count() >= 1, "no GPU visible"
np.random.seed(5)
n, d, nq0 = 40000, 48, 200
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
allowed = np.random.default_rng(3).random(n) < 0.1
want0 = guarded_batch(oracle, ox, qn0, k, n_probes, allowed=allowed)
dev = ivf.device_index()
ms = dev.max_sub_batch(k, n_probes)
sel = np.arange(2 * ms + 5) % nq0                    # three parts
aset = dev.allow(allowed)
for depth in (1, 3):
    dev.set_pipeline(depth)
    got = dev.query_batch(qn0[sel], qp0[sel], k, n_probes, allowed=aset)
    assert np.array_equal(got, want0[sel]), ("rows differ", depth, np.flatnonzero((got != want0[sel]).any(axis=1))[:5])
aset.close()
print("ok", ms, len(sel))
'''


def test_batch_beyond_one_workspace(tk):
    env = dict(os.environ, TINYKNN_WORKSPACE_GB="0.25")
    r = subprocess.run([sys.executable, "-c", SUB_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
