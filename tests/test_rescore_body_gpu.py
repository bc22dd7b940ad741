"""The staged rescoring body (rescore.hip: rescore_staged_body) against the oracle's knn_brute1 / bottom_k, exactly:
a candidate's row resolved once, two lanes per row in the sum, one strict-count walk for the ranks with the tie loop
behind it.  Nothing here has a tolerance: ids array_equal, distances bit for bit.

(a) tk_knn_brute1 — one query, n candidate rows, no -1: every tile count and tail (n), every lane geometry and
    summation tail (d: 1, 4, 5, 25, 32, 64 pieces), heaps of one and of several values per lane (n <= 64, <= 128,
    <= 256), tables whose duplicated rows put exact ties inside the first k, across its edge, everywhere.
(b) a small IVF index whose lists include one of 7 and one of 13 rows: candidates that hold -1, heaps of <= k ids and
    of slightly more, the coarse rescoring with its fused descriptors, float32 and half rows, a batch submitted as a
    pair of calls of unequal size (the second-buffer pointers).
(c) TK_OPT_RESCORE_FORM 0, 1, 2 on (b)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from store_reference import exact_distances, oracle_index, rounded, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

NS = ["k+1", 31, 32, 33, 64, 65, 111, 129, 256]
KS = [1, 10, 64]


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    return tinyknn_amd


# ---- (a) ---------------------------------------------------------------------------------------------------------
def _tables(oracle, rng, n, d, k):
    """(name, x, Y): a table without duplicates, and the same with rows duplicated against the query's own order"""
    x = rng.standard_normal(d).astype(np.float32)
    Y = rng.standard_normal((n, d)).astype(np.float32)
    order = np.argsort(oracle.sqdist_gather(x, Y, np.arange(n)), kind="stable")     # every position, ascending
    out = [("distinct", x, Y)]
    kk = min(k, n)
    if kk >= 2:
        T = Y.copy()
        T[order[kk - 1]] = T[order[kk - 2]]             # the last two places kept
        T[order[kk // 2]] = T[order[0]]                 # ... and the best row once more
        out.append(("tie inside the first k", x, T))
    if n > kk:
        T = Y.copy()
        T[order[kk]] = T[order[kk - 1]]                 # the last place kept and the first one dropped
        out.append(("tie across the edge", x, T))
        T = Y.copy()
        T[order[kk:kk + 3]] = T[order[kk - 1]]          # ... and more rows than fit
        T[order[0]] = T[order[kk - 1]]
        out.append(("ties across the edge, both sides", x, T))
    out.append(("all rows identical", x, np.repeat(Y[:1], n, axis=0)))
    half = Y.copy()
    half[::2] = half[1]                                 # every other row one row
    out.append(("half the rows identical", x, half))
    return out


@pytest.mark.parametrize("d", [4, 16, 20, 100, 128, 256])
def test_knn_brute1_every_size_with_and_without_ties(tk, oracle, d):
    from tinyknn_amd.utils import knn_brute1
    rng = np.random.default_rng(1000 + d)
    seen = set()
    for k in KS:
        for n in NS:
            n = k + 1 if n == "k+1" else n
            for name, x, Y in _tables(oracle, rng, n, d, k):
                want = oracle.knn_brute1(x, Y, k)
                got = knn_brute1(x, Y, k)
                np.testing.assert_array_equal(got, want, err_msg=f"{name}: n {n} d {d} k {k}")
                seen.add(name)
    assert len(seen) == 6


def test_knn_brute1_signed_zero_distances(tk, oracle):
    """rows equal to the query: distances of +0 beside each other and beside the rest"""
    from tinyknn_amd.utils import knn_brute1
    rng = np.random.default_rng(5)
    for n, d, k in ((33, 20, 10), (111, 100, 10), (256, 128, 64)):
        x = rng.standard_normal(d).astype(np.float32)
        Y = rng.standard_normal((n, d)).astype(np.float32)
        Y[[3, n // 2, n - 1]] = x
        np.testing.assert_array_equal(knn_brute1(x, Y, k), oracle.knn_brute1(x, Y, k))


# ---- (b) ---------------------------------------------------------------------------------------------------------
SIZES = [285] * 14 + [7, 13]            # rows per list: N = 4010


@pytest.fixture(scope="module", params=[20, 100])
def small(request, tk):
    """{store: IVF} of one fitted index with 16 lists of SIZES rows, and 96 queries, six beside every list"""
    from tinyknn_amd import IVF, FastPQ
    d = request.param
    rng = np.random.RandomState(50 + d)
    cent = (4.0 * rng.randn(16, d)).astype(np.float32)
    member = rng.permutation(np.repeat(np.arange(16), SIZES))
    X = (cent[member] + 0.5 * rng.randn(len(member), d)).astype(np.float32)
    qs = (cent[np.arange(96) % 16] + 0.5 * rng.randn(96, d)).astype(np.float32)
    first = IVF("euclidean", 16, FastPQ(2))
    np.random.seed(3)
    first.fit(X)
    out = {}
    for store in (None, "float16"):
        ivf = IVF("euclidean", 16, FastPQ(2))
        ivf.pq, ivf.all_centers = first.pq, cent        # the lists are the clusters the rows were drawn from
        ivf.build(X, n_probes=1, device=False, store=store)
        assert sorted(len(i) for i in ivf.ids) == sorted(SIZES)
        out[store or "float32"] = ivf
    qn, qp = first._prepare(qs.copy())
    return out, np.ascontiguousarray(qn, dtype=np.float32), np.ascontiguousarray(qp)


def _reference(oracle, ivf, store):
    data = rounded(ivf.data) if store == "float16" else ivf.data
    return oracle_index(oracle, ivf, data), data


@pytest.mark.parametrize("store", ["float32", "float16"])
@pytest.mark.parametrize("n_probes", [1, 10])
def test_small_index_ids_distances_and_probes(small, oracle, store, n_probes):
    ivfs, qn, qp = small
    ivf = ivfs[store]
    ox, data = _reference(oracle, ivf, store)
    dev = ivf.device_index()
    assert dev.store == store
    k = 10
    held = []
    probes = []
    for q in qn:
        _, dbg = ox.query(q, k, n_probes, debug=True)
        held.append(int((dbg["heap_idx"] != -1).sum()))
        probes.append(dbg["probes"])
    R = (n_probes + 1) * k + 1
    if n_probes == 1:
        # the lists of 7 and 13 rows: heaps that hold <= k ids, and slightly more, beside -1; full heaps of the rest
        assert 7 in held and 13 in held and R in held, sorted(set(held))
    else:
        assert set(held) == {R}
    want = ox.query_batch(qn, k, n_probes)
    ids, dist = dev.query_batch(qn, qp, k, n_probes, return_distances=True)
    np.testing.assert_array_equal(ids, want)
    assert same_bits(dist, exact_distances(oracle, qn, data, want))
    np.testing.assert_array_equal(dev.query_batch(qn, qp, k, n_probes), want)
    got, dbg = dev.query_batch(qn, qp, k, n_probes, debug=True)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(dbg["probes"], np.stack(probes))
    if n_probes == 1:
        assert (want == -1).any() and not (want[:, :7] == -1).any()


@pytest.mark.parametrize("store", ["float32", "float16"])
@pytest.mark.parametrize("n_probes", [1, 10])
def test_small_index_batch_as_a_pair_of_unequal_calls(small, oracle, store, n_probes):
    """the second call's queries, ids and distances come from and go to buffers of its own"""
    import torch
    ivfs, qn, qp = small
    ivf = ivfs[store]
    ox, data = _reference(oracle, ivf, store)
    want = ox.query_batch(qn, 10, n_probes)
    wd = exact_distances(oracle, qn, data, want)
    dev = ivf.device_index()
    dev.set_pipeline(2)
    dev.set_coalesce(2)
    st = torch.cuda.current_stream().cuda_stream
    d, dq = qn.shape[1], qp.shape[1]
    f64 = qp.dtype != np.float32            # (d = 20: the PQ pads to 24 and rotates, its queries are float64)
    calls = [((0, 59), True), ((59, 96), True), ((0, 11), False), ((11, 96), True)]
    held = []
    for (a, b), with_d in calls:
        q_dev, qp_dev = torch.from_numpy(qn[a:b].copy()).cuda(), torch.from_numpy(qp[a:b].copy()).cuda()
        o = torch.full((b - a, 10), -7, dtype=torch.int64, device="cuda")
        od = torch.full((b - a, 10), -7.0, dtype=torch.float32, device="cuda")
        held.append((q_dev, qp_dev, o, od))
        assert qp_dev.shape[1] == dq and q_dev.shape[1] == d
        dev.query_batch_dev(q_dev.data_ptr(), qp_dev.data_ptr(), f64, b - a, 10, n_probes, o.data_ptr(), stream=st,
                            dist_ptr=od.data_ptr() if with_d else None)
    dev.join(st)
    torch.cuda.synchronize()
    dev.set_coalesce(1)
    dev.set_pipeline(1)
    for ((a, b), with_d), (_, _, o, od) in zip(calls, held):
        np.testing.assert_array_equal(o.cpu().numpy(), want[a:b], err_msg=f"call {a}:{b}")
        if with_d:
            assert same_bits(od.cpu().numpy(), wd[a:b]), (a, b)
        else:
            assert (od.cpu().numpy() == -7.0).all()


# ---- (c) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["float32", "float16"])
def test_small_index_every_rescore_form(small, oracle, store):
    from tinyknn_amd import _lib
    ivfs, qn, qp = small
    ivf = ivfs[store]
    ox, data = _reference(oracle, ivf, store)
    dev = ivf.device_index()
    try:
        for n_probes in (1, 10):
            want = ox.query_batch(qn, 10, n_probes)
            wd = exact_distances(oracle, qn, data, want)
            for form in (0, 1, 2):
                dev.set_option(_lib.OPT_RESCORE_FORM, form)
                ids, dist = dev.query_batch(qn, qp, 10, n_probes, return_distances=True)
                np.testing.assert_array_equal(ids, want, err_msg=f"form {form} p{n_probes}")
                assert same_bits(dist, wd), (form, n_probes)
                np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, n_probes), want, err_msg=f"form {form}")
    finally:
        dev.set_option(_lib.OPT_RESCORE_FORM, 2)
