"""store="float16" on the GPU: an index that keeps its rescoring vectors in IEEE half answers, bit for bit, what
the same index answers on float32(float16(x)).  References: the unmodified oracle fed the rounded rows, and the
float32 twin index (tests/store_reference.py).  Every comparison is array_equal on ids and bit equality of the
float32 distances; no row is excluded."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from allowed_reference import guarded_batch  # noqa: E402
from conftest import G6_TAGS, golden  # noqa: E402
from store_reference import (exact_distances, fixture_ivf, host_copy, oracle_index, rounded, same_bits,  # noqa: E402
                             twin)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    return tinyknn_amd


def _f32_fixture(tag):
    """(fixture, its vectors as float32): the float64 fixture's index with its vectors cast to float32 — lists,
    codes and probes do not read them; its queries stay rotated float64 table queries."""
    g = golden(f"g6_ivf_{tag}.npz")
    return g, np.ascontiguousarray(g["data"], dtype=np.float32)


def _assert_answers(oracle, dev, tw, ox, qn, qpq, data_r, k, n_probes, what=""):
    """ids and distances of `dev` (half) against the oracle on the rounded rows and against the float32 twin"""
    ids, dist = dev.query_batch(qn, qpq, k, n_probes, return_distances=True)
    assert dist.dtype == np.float32
    np.testing.assert_array_equal(ids, dev.query_batch(qn, qpq, k, n_probes), err_msg=what)
    np.testing.assert_array_equal(ids, ox.query_batch(qn, k, n_probes), err_msg=what)
    assert same_bits(dist, exact_distances(oracle, qn, data_r, ids)), what
    t_ids, t_dist = tw.query_batch(qn, qpq, k, n_probes, return_distances=True)
    np.testing.assert_array_equal(ids, t_ids, err_msg=what)
    assert same_bits(dist, t_dist), what
    return ids


# ---- rounding ------------------------------------------------------------------------------------------------
def _crafted(n, d, seed=0):
    sub_min, sub_max = 2.0 ** -24, 1023 * 2.0 ** -24
    top = np.nextafter(np.float32(65520.0), np.float32(0.0))            # 65519.99...: rounds to 65504
    vals = [0.0, sub_min, sub_max, 2.0 ** -25, 3 * 2.0 ** -25, 5 * 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
            np.nextafter(np.float32(2.0 ** -25), np.float32(0)), 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1 + 2.0 ** -11,
            1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -10, 2047.0, 2049.0, 2051.0, 65504.0, 65519.0,
            float(top), 1e-8, 1e-40, 0.1, 1 / 3]
    vals = np.array(vals + [-v for v in vals], dtype=np.float32)
    rng = np.random.default_rng(seed)
    X = vals[rng.integers(0, len(vals), size=(n, d))]
    scaled = rng.standard_normal((n - n // 2, d)) * 10.0 ** rng.integers(-9, 5, size=(n - n // 2, d))
    X[n // 2:] = np.clip(scaled, -65000.0, 65000.0).astype(np.float32)
    X.reshape(-1)[:len(vals)] = vals            # every crafted value at least once
    assert (np.abs(X) < 65520).all()
    return np.ascontiguousarray(X, dtype=np.float32)


def test_rounding_of_an_upload_and_of_narrow_is_numpy_s(tk):
    from tinyknn_amd.ivf import DeviceIndex
    g, data = _f32_fixture("eu20")
    X = _crafted(*data.shape)
    want = X.astype(np.float16)
    rows = np.arange(len(X))
    ivf = fixture_ivf(g, X)
    up = DeviceIndex(ivf, store="float16")              # host upload with dtype TK_DATA_F16
    assert up.store == "float16" and up.vector_bytes == X.size * 2
    got = up.read_rows(rows)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.astype(np.float16).view(np.uint16), want.view(np.uint16))
    assert same_bits(got, want.astype(np.float32))
    nar = DeviceIndex(ivf)                              # float32 in HBM, then tk_index_narrow_data
    assert nar.store == "float32" and nar.vector_bytes == X.size * 4
    assert same_bits(nar.read_rows(rows), X)
    nar.narrow()
    assert nar.store == "float16" and nar.vector_bytes == X.size * 2
    assert same_bits(nar.read_rows(rows), want.astype(np.float32))
    nar.narrow()                                        # idempotent
    assert nar.store == "float16" and same_bits(nar.read_rows(rows), want.astype(np.float32))
    # a random order, rows named twice
    pick = np.random.default_rng(1).integers(0, len(X), size=777)
    assert same_bits(up.read_rows(pick), want.astype(np.float32)[pick])
    up.close()
    nar.close()


@pytest.mark.parametrize("bad", [65520.0, -np.inf, np.nan])
def test_narrow_refuses_a_value_whose_half_is_not_finite(tk, bad):
    from tinyknn_amd.ivf import DeviceIndex
    g, data = _f32_fixture("an100")
    X = data.copy()
    X[4321 % len(X), 5] = bad
    X[len(X) - 1, 0] = bad
    ivf = fixture_ivf(g, X)
    dev = DeviceIndex(ivf)
    qn, qpq = g["qn"], g["qpq"]
    before = dev.query_batch(qn, qpq, 10, 5, return_distances=True)
    with pytest.raises(ValueError, match=rf"row {4321 % len(X)}\b"):
        dev.narrow()
    assert dev.store == "float32" and dev.vector_bytes == X.size * 4
    after = dev.query_batch(qn, qpq, 10, 5, return_distances=True)
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1].view(np.uint32), before[1].view(np.uint32))
    assert same_bits(dev.read_rows(np.arange(0, len(X), 7)), X[::7])
    with pytest.raises(ValueError, match=rf"row {4321 % len(X)}\b"):       # the upload refuses the same row
        DeviceIndex(ivf, store="float16")
    dev.close()


def test_narrow_is_refused_on_float64_vectors_and_on_lent_or_borrowed_ones(tk):
    from tinyknn_amd.ivf import DeviceIndex
    g = golden("g6_ivf_eu20f64.npz")
    f64 = DeviceIndex(fixture_ivf(g))
    assert f64.store == "float64"
    with pytest.raises(AssertionError, match="float64"):
        f64.narrow()
    with pytest.raises(ValueError, match="float64"):
        DeviceIndex(fixture_ivf(g), store="float16")
    f64.close()
    g, data = _f32_fixture("an20")
    src = DeviceIndex(fixture_ivf(g, data))
    owner = (np.arange(src.n_lists) % 2).astype(np.int32)
    clone = src.clone_shard(owner, 1, 2)
    assert clone.store == "float32"
    with pytest.raises(AssertionError, match="borrow"):
        clone.narrow()
    with pytest.raises(AssertionError, match="borrow"):
        src.narrow()
    assert src.store == "float32"
    clone.close()
    src.close()
    half = DeviceIndex(fixture_ivf(g, data), store="float16")
    c2 = half.clone_shard(owner, 0, 2)                  # the format travels with the borrowed array
    assert c2.store == "float16" and c2.vector_bytes == data.size * 2
    c2.close()
    half.close()


# ---- queries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", G6_TAGS)
def test_fixtures_against_the_oracle_on_rounded_rows_and_the_twin(tk, oracle, tag):
    g, data = _f32_fixture(tag)
    ivf = fixture_ivf(g, data, store="float16")
    data_r = rounded(data)
    assert not np.array_equal(data_r, data)
    ox = oracle_index(oracle, ivf, data_r)
    dev, tw = ivf.device_index(), twin(ivf).device_index()
    assert dev.store == "float16" and tw.store == "float32"
    assert dev.vector_bytes == data.size * 2 and tw.vector_bytes == data.size * 4
    qn, qpq = g["qn"], g["qpq"]
    short = 0
    for n_probes in (1, 2, 5, 10, 50):
        for k in (1, 10, 50):
            ids = _assert_answers(oracle, dev, tw, ox, qn, qpq, data_r, k, n_probes, f"{tag} p{n_probes} k{k}")
            short += int((ids == -1).any(axis=1).sum())
    # the half index does NOT answer as the unrounded float32 index does everywhere: the rows it holds are the rounded ones
    plain = fixture_ivf(g, data).device_index()
    a = dev.query_batch(qn, qpq, 10, 10, return_distances=True)[1]
    b = plain.query_batch(qn, qpq, 10, 10, return_distances=True)[1]
    assert not same_bits(a, b)
    if tag in ("an100", "an100b2", "eu128"):
        single = fixture_ivf(g, data, store="float16")
        for i in range(0, len(qn), 9):
            got = single.device_index().query_batch(qn[i:i + 1], qpq[i:i + 1], 10, 5)
            np.testing.assert_array_equal(got, ox.query_batch(qn[i:i + 1], 10, 5))


def _synth(tk, d, n, nq, metric, clusters, kp=2, seed=11):
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(seed)
    cent = rng.randn(60, d)
    X = (cent[rng.randint(60, size=n)] + 0.6 * rng.randn(n, d)).astype(np.float32)
    qs = (cent[rng.randint(60, size=nq)] + 0.6 * rng.randn(nq, d)).astype(np.float32)
    ivf = IVF(metric, clusters, FastPQ(2))
    np.random.seed(seed)
    ivf.fit(X[:4000]).build(X, n_probes=kp, store="float16")
    qn, qp = ivf._prepare(qs.copy())
    return ivf, qn, np.ascontiguousarray(qp)


@pytest.mark.parametrize("d,metric", [(30, "euclidean"), (300, "euclidean"), (100, "angular")])
def test_synthetic_indexes_generic_and_staged_paths(tk, oracle, d, metric):
    """d = 30 (d % 4 != 0) and d = 300 (d > 256) take the lane-per-row kernels on half rows; build(n_probes=2)
    lists (labels that repeat); queries far from every centre leave heaps with <= k ids."""
    ivf, qn, qp = _synth(tk, d, 9000, 150, metric, 300)
    assert ivf.store == "float16" and ivf.data.dtype == np.float32
    data_r = rounded(ivf.data)
    assert not np.array_equal(data_r, ivf.data)
    ox = oracle_index(oracle, ivf, data_r)
    dev, tw = ivf.device_index(), twin(ivf).device_index()
    assert dev.store == "float16" and dev.vector_bytes == ivf.data.size * 2
    short = 0
    for n_probes in (1, 2, 5, 10, 50):
        for k in (1, 10, 50):
            ids = _assert_answers(oracle, dev, tw, ox, qn, qp, data_r, k, n_probes, f"d{d} p{n_probes} k{k}")
            short += int((ids == -1).any(axis=1).sum())
    assert short > 0            # some heaps held <= k ids: the heap-order branch and its distances ran
    # the public calls: one query, a batch, fast mode, distances
    for i in range(0, 30, 7):
        got = ivf.query(qn[i].copy(), 10, n_probes=5, return_distances=True)
        w_ids = ox.query_batch(ivf._prepare(qn[i][None, :].copy())[0], 10, 5)[0]
        np.testing.assert_array_equal(got[0], w_ids[w_ids != -1] if w_ids[-1] == -1 else w_ids)
        assert got[1].dtype == np.float32 and len(got[1]) == len(got[0])
    tivf = twin(ivf)
    np.testing.assert_array_equal(ivf.query_batch(qn, 10, n_probes=5), tivf.query_batch(qn, 10, n_probes=5))
    if d <= 128:
        np.testing.assert_array_equal(ivf.query_batch(qn, 10, n_probes=5, fast=True),
                                      tivf.query_batch(qn, 10, n_probes=5, fast=True))


def test_rescore_forms_heap_modes_and_allowed_sets_on_one_index(tk, oracle):
    from tinyknn_amd import _lib
    g, data = _f32_fixture("an100")
    ivf = fixture_ivf(g, data, store="float16")
    data_r = rounded(data)
    ox = oracle_index(oracle, ivf, data_r)
    dev = ivf.device_index()
    qn, qpq = g["qn"], g["qpq"]
    for n_probes in (1, 5, 10, 50):
        for k in (1, 10, 50):
            want = ox.query_batch(qn, k, n_probes)
            wd = exact_distances(oracle, qn, data_r, want)
            for form in (0, 1, 2):
                for mode in (0, 1, 2, 3):
                    dev.set_option(_lib.OPT_RESCORE_FORM, form)
                    dev.set_heap_mode(mode)
                    ids, dist = dev.query_batch(qn, qpq, k, n_probes, return_distances=True)
                    np.testing.assert_array_equal(ids, want, err_msg=f"form {form} mode {mode}")
                    assert same_bits(dist, wd), (form, mode, n_probes, k)
                    np.testing.assert_array_equal(dev.query_batch(qn, qpq, k, n_probes), want)
    dev.set_option(_lib.OPT_RESCORE_FORM, 2)
    dev.set_heap_mode(0)
    N = len(data)
    whole = np.zeros(N, dtype=bool)
    whole[np.asarray(ivf.ids[3], dtype=np.int64)] = True            # one whole list
    for allowed in (np.random.default_rng(5).random(N) < 0.3, whole):
        for n_probes in (1, 10):
            want = guarded_batch(oracle, ox, qn, 10, n_probes, allowed=allowed)
            ids, dist = dev.query_batch(qn, qpq, 10, n_probes, allowed=allowed, return_distances=True)
            np.testing.assert_array_equal(ids, want)
            assert same_bits(dist, exact_distances(oracle, qn, data_r, want))
            aset = dev.allow(allowed)
            np.testing.assert_array_equal(dev.query_batch(qn, qpq, 10, n_probes, allowed=aset), want)
            aset.close()


@pytest.mark.parametrize("d", [256, 132])
def test_rows_of_more_than_32_pieces_under_every_rescore_form(tk, oracle, d):
    """Rows of 33 ... 64 pieces spread over 64 lanes in the staged kernels (32 for every narrower row).  d = 256: 64
    pieces, every lane busy; the float32 tile of 64 rows is (64 + 1) * 65 * 16 = 67 600 bytes, beyond the 64 KB of a
    workgroup, so form 1 on float32 rows falls through to the lane-per-row kernel while the half tile (33 800
    bytes) stays staged.  d = 132: 33 pieces, the first size with 64 lanes per row, 31 of them idle.  The half
    index against the oracle on the rounded rows; float32 indexes on the rounded rows (the twin) and on the
    unrounded ones against the oracle on theirs."""
    from tinyknn_amd import _lib
    ivf, qn, qp = _synth(tk, d, 9000, 150, "euclidean", 300)
    data_r = rounded(ivf.data)
    assert not np.array_equal(data_r, ivf.data)
    plain = twin(ivf)
    plain.data = ivf.data
    for index, data, store in ((ivf, data_r, "float16"), (twin(ivf), data_r, "float32"), (plain, ivf.data, "float32")):
        ox = oracle_index(oracle, index, data)
        dev = index.device_index()
        assert dev.store == store
        for n_probes in (1, 5):
            want = ox.query_batch(qn, 10, n_probes)
            wd = exact_distances(oracle, qn, data, want)
            got = []
            for form in (0, 1, 2):
                dev.set_option(_lib.OPT_RESCORE_FORM, form)
                ids, dist = dev.query_batch(qn, qp, 10, n_probes, return_distances=True)
                np.testing.assert_array_equal(ids, want, err_msg=f"{store} form {form} p{n_probes}")
                assert same_bits(dist, wd), (store, form, n_probes)
                np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, n_probes), want)
                got.append((ids, dist))
            for ids, dist in got[1:]:
                np.testing.assert_array_equal(ids, got[0][0])
                assert same_bits(dist, got[0][1])
        dev.set_option(_lib.OPT_RESCORE_FORM, 2)


# ---- pipelined pairs, the stream session, a captured graph ------------------------------------------------------
@pytest.fixture(scope="module")
def big(tk):
    ivf, qn, qp = _synth(tk, 100, 40000, 1801, "angular", 180, kp=1)
    tw = twin(ivf)
    return ivf, tw, qn, qp


def test_pipelined_pairs_with_and_without_distances(big):
    import torch
    ivf, tw, qn, qp = big
    dev, tdev = ivf.device_index(), tw.device_index()
    want = {p: tdev.query_batch(qn, qp, 10, p, return_distances=True) for p in (3, 10)}
    dev.set_pipeline(2)
    dev.set_coalesce(2)
    st = torch.cuda.current_stream().cuda_stream
    q_dev, qp_dev = torch.from_numpy(qn).cuda(), torch.from_numpy(qp).cuda()
    d, dq = qn.shape[1], qp.shape[1]
    esz = qp.dtype.itemsize
    f64 = qp.dtype != np.float32
    # odd sizes: the second call of a pair starts in the middle of the merged buffers
    calls = [((0, 901), 10, True), ((901, 1801), 10, False), ((0, 333), 10, False), ((333, 600), 10, True),
             ((600, 1001), 10, True), ((1001, 1400), 10, True), ((1400, 1801), 10, True),
             ((0, 701), 3, False), ((701, 1400), 3, False), ((1400, 1801), 3, True)]
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
            assert same_bits(od.cpu().numpy(), want[p][1][a:b]), f"call {j}"
        else:
            assert (od.cpu().numpy() == SENT).all(), f"call {j} asked for no distances"
    for depth in (1, 3):
        dev.set_coalesce(1)
        dev.set_pipeline(depth)
        o = torch.full((len(qn), 10), -7, dtype=torch.int64, device="cuda")
        dev.query_batch_dev(q_dev.data_ptr(), qp_dev.data_ptr(), f64, len(qn), 10, 10, o.data_ptr(), stream=st)
        dev.join(st)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(o.cpu().numpy(), want[10][0], err_msg=f"depth {depth}")
    dev.set_pipeline(1)


def test_stream_session_across_chunks_and_query_stream(big):
    ivf, tw, qn, qp = big
    dev, tdev = ivf.device_index(), tw.device_index()
    want = tdev.query_batch(qn, qp, 10, 10, return_distances=True)[0]
    # the default path of query_batch is the stream session; sessions of 500 rows see 1801 queries in four chunks
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 10), want)
    st = dev.stream(500, 10, 10)
    out = np.full((len(qn), 10), -1, dtype=np.int64)
    for o in range(0, len(qn), 500):
        st.submit_prepared(qn[o:o + 500], None, out[o:o + 500])
    st.drain()
    st.close()
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(ivf.query_batch(qn, 10, n_probes=10), tw.query_batch(qn, 10, n_probes=10))


def test_captured_graph_replay(big):
    import torch
    from tinyknn_amd.ivf import DeviceIndex
    ivf, tw, qn, qp = big
    want = tw.device_index().query_batch(qn, qp, 10, 8, return_distances=True)[0]
    dev = DeviceIndex(ivf)
    assert dev.store == "float16"
    nq = len(qn)
    q_dev, qp_dev = torch.from_numpy(qn).cuda(), torch.from_numpy(qp).cuda()
    out = torch.full((nq, 10), -1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()

    def calls(st):
        dev.query_batch_dev(q_dev.data_ptr(), qp_dev.data_ptr(), False, nq, 10, 8, out.data_ptr(), stream=st)
        dev.join(st)

    with torch.cuda.stream(side):
        calls(side.cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    dev.quiesce()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        calls(torch.cuda.current_stream().cuda_stream)
    dev.quiesce()
    out.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    del g
    dev.close()


# ---- changes in place ------------------------------------------------------------------------------------------
def test_add_and_remove_on_a_host_built_index(tk, oracle):
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(4)
    d = 100
    cent = rng.randn(40, d)
    X = (cent[rng.randint(40, size=6000)] + 0.6 * rng.randn(6000, d)).astype(np.float32)
    Y = (cent[rng.randint(40, size=1500)] + 0.6 * rng.randn(1500, d)).astype(np.float32)
    qs = np.concatenate([Y[:100], X[1:200:2]]).astype(np.float32)
    half = IVF("euclidean", 60, FastPQ(2))
    np.random.seed(2)
    half.fit(X[:4000]).build(X, n_probes=2, store="float16")
    plain = IVF("euclidean", 60, FastPQ(2))
    plain.all_centers, plain.pq = half.all_centers, half.pq
    plain.build(X, n_probes=2)
    tw = twin(plain)                                    # float32 vectors = the rounded rows
    hd, td = half.device_index(), tw.device_index()
    assert hd.store == "float16"
    qn, qp = half._prepare(qs.copy())
    np.testing.assert_array_equal(hd.query_batch(qn, qp, 10, 5), td.query_batch(qn, qp, 10, 5))
    # an add holding an overflowing row raises, and the index answers as before
    before = hd.query_batch(qn, qp, 10, 5, return_distances=True)
    lists0 = hd.export_lists()
    Yb = Y.copy()
    Yb[77, 3] = 70000.0
    for target in (half, hd):
        with pytest.raises(ValueError, match=r"row 6077\b"):
            if target is half:
                half.add(Yb)
            else:       # the library's own check (the host's was passed by: rows handed to the device index)
                near = np.zeros((len(Yb), 2), dtype=np.int64)
                near[:, 1] = 1
                hd.add(Yb, 2, nearest=near, labels=np.zeros((len(Yb), hd.M), np.uint8), list_columns=half.list_columns)
    assert hd.N == 6000 and len(half.data) == 6000
    for a, b in zip(lists0, hd.export_lists()):
        np.testing.assert_array_equal(a, b)
    after = hd.query_batch(qn, qp, 10, 5, return_distances=True)
    np.testing.assert_array_equal(after[0], before[0])
    assert same_bits(after[1], before[1])
    # the same calls on both; the twin appends the ROUNDED rows it would hold, assigned and coded from the float32 ones
    half.add(Y)
    plain.add(Y)                                        # lists and codes of the float32 index (host copy)
    assert hd.N == 7500 and hd.store == "float16" and hd.vector_bytes == 7500 * d * 2
    np.testing.assert_array_equal(half.data, plain.data)                 # unrounded on the host
    assert same_bits(hd.read_rows(np.arange(7500)), rounded(half.data))
    for a, b in zip(hd.export_lists(), plain.device_index().export_lists()):
        np.testing.assert_array_equal(a, b)
    gone = np.arange(0, 7500, 5)
    half.remove(gone)
    plain.remove(gone)
    tw2 = twin(plain)
    data_r = rounded(half.data)
    ox = oracle_index(oracle, half, data_r)
    td2 = tw2.device_index()
    for p in (1, 5, 10):
        ids = _assert_answers(oracle, hd, td2, ox, qn, qp, data_r, 10, p, f"after add+remove p{p}")
        assert not np.isin(ids, gone).any()
    assert (hd.query_batch(qn, qp, 10, 10) >= 6000).sum() > 100
    # a saved and loaded index rounds again at upload: the same bits
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        half.save(os.path.join(tmp, "h"))
        back = IVF.load(os.path.join(tmp, "h"))
    assert back.store == "float16"
    bd = back.device_index()
    assert bd.store == "float16" and same_bits(bd.read_rows(np.arange(7500)), data_r)
    np.testing.assert_array_equal(bd.query_batch(qn, qp, 10, 10), hd.query_batch(qn, qp, 10, 10))


@pytest.mark.parametrize("metric,kp", [("angular", 2), ("euclidean", 1)])
def test_add_and_remove_on_a_resident_index(tk, oracle, metric, kp):
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import synth_rows
    d, N0, n, seed, sigma = 100, 5003, 1200, 7, 0.7
    cent = np.random.RandomState(3).randn(30, d).astype(np.float32)
    fit = IVF(metric, 48, FastPQ(2))
    np.random.seed(1)
    fit.fit(synth_rows(4000, d, seed, cent, sigma))

    def resident(store):
        ivf = IVF(metric, 48, FastPQ(2))
        ivf.all_centers, ivf.pq = fit.all_centers, fit.pq
        return ivf.build_resident(N0, d, seed, cent, sigma, n_probes=kp, store=store)

    half, f32 = resident("float16"), resident(None)
    hd, fd = half.device_index(), f32.device_index()
    assert half.store == "float16" and half.data.store == "float16" and half.data.dtype == np.float32
    assert hd.store == "float16" and fd.store == "float32"
    assert hd.vector_bytes == N0 * d * 2 and fd.vector_bytes == N0 * d * 4
    with pytest.raises(Exception, match="float32 vectors"):
        hd.knn_brute(np.zeros((1, d), np.float32), 5)
    X_new = synth_rows(n, d, seed, cent, sigma, row0=N0)
    qs = synth_rows(200, d, seed + 1, cent, sigma)
    qn, qp = half._prepare(qs.copy())
    if metric == "euclidean":       # (angular rows are normalised on the device before the check: none can overflow)
        before = hd.query_batch(qn, qp, 10, 5, return_distances=True)
        Xb = X_new.copy()
        Xb[5, 1] = -65520.0
        with pytest.raises(ValueError, match=rf"row {N0 + 5}\b"):
            half.add(Xb)
        assert hd.N == N0
        for a, b in zip(hd.export_lists(), fd.export_lists()):
            np.testing.assert_array_equal(a, b)
        after = hd.query_batch(qn, qp, 10, 5, return_distances=True)
        np.testing.assert_array_equal(after[0], before[0])
        assert same_bits(after[1], before[1])
    gone = np.arange(3, N0 + n, 7)
    for ivf in (half, f32):
        ivf.add(X_new)
        ivf.remove(gone)
    N = N0 + n
    assert hd.N == N and hd.store == "float16" and hd.vector_bytes == N * d * 2
    for a, b in zip(hd.export_lists(), fd.export_lists()):          # byte for byte the float32 resident build's
        np.testing.assert_array_equal(a, b)
    for a, b in zip(hd.export_centers(), fd.export_centers()):
        np.testing.assert_array_equal(a, b)
    rows32 = fd.read_rows(np.arange(N))
    data_r = rounded(rows32)
    assert same_bits(hd.read_rows(np.arange(N)), data_r) and not np.array_equal(data_r, rows32)
    assert same_bits(half.data[np.arange(10)], data_r[:10])
    tw_ivf = host_copy(f32, data_r)                     # the float32 twin: the same lists, the rounded rows
    ox = oracle_index(oracle, tw_ivf, data_r)
    td = tw_ivf.device_index()
    for p in (1, 5, 10):
        ids = _assert_answers(oracle, hd, td, ox, qn, qp, data_r, 10, p, f"resident {metric} p{p}")
        assert not np.isin(ids, gone).any()


def test_resident_build_refuses_a_value_whose_half_is_not_finite(tk):
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import synth_rows
    d, N = 100, 4500
    big_c = np.random.RandomState(3).randn(30, d).astype(np.float32)
    big_c[7, 0] += 70000.0                      # the rows of one generator centre hold a value beyond the largest half
    rows = synth_rows(N, d, 7, big_c, 0.7)      # (the generator is a pure function of seed and row: the index's rows)
    first = int(np.argmax((np.abs(rows) >= 65520).any(axis=1)))
    assert np.abs(rows[first]).max() >= 65520 and 0 < first < N
    for metric in ("euclidean", "angular"):
        fit = IVF(metric, 48, FastPQ(2))
        np.random.seed(1)
        fit.fit(rows[:4000])
        ivf = IVF(metric, 48, FastPQ(2))
        ivf.all_centers, ivf.pq = fit.all_centers, fit.pq
        if metric == "euclidean":
            with pytest.raises(ValueError, match=rf"row {first}\b"):
                ivf.build_resident(N, d, 7, big_c, 0.7, n_probes=1, store="float16")
            assert ivf.store is None
        else:       # normalised on the device before the check: every half is finite
            ivf.build_resident(N, d, 7, big_c, 0.7, n_probes=1, store="float16")
            assert ivf.store == "float16" and ivf.device_index().store == "float16"


# ---- sharded, knn_brute ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,world,coarse", [("an100", 3, "home"), ("eu128", 2, "replicated"), ("an100b2", 1, "home")])
def test_ranks_of_a_partition_answer_as_the_unsharded_half_index(tk, tag, world, coarse):
    from test_shard_gpu import simulate_world
    g, data = _f32_fixture(tag)
    ivf = fixture_ivf(g, data, store="float16")
    dev = ivf.device_index()
    for n_probes in (1, 5, 10):
        want = dev.query_batch(g["qn"], g["qpq"], 10, n_probes)
        ids, flags, _ = simulate_world(ivf, world, g["qn"], g["qpq"], 10, n_probes, coarse=coarse)
        assert not flags.any()
        np.testing.assert_array_equal(ids, want)
    # (ranks cloned on one device borrow the half vectors)
    owner = (np.arange(dev.n_lists) % 2).astype(np.int32)
    c = dev.clone_shard(owner, 0, 2)
    assert c.store == "float16"
    c.close()


def test_world1_public_sharded_class(tk):
    from tinyknn_amd.multi_gpu import ListShardedIndex
    g, data = _f32_fixture("eu128")
    ivf = fixture_ivf(g, data, store="float16")
    want = fixture_ivf(g, data, store="float16").device_index().query_batch(g["qn"], g["qpq"], 10, 5)
    idx = ListShardedIndex(ivf)
    np.testing.assert_array_equal(idx.query_batch(g["qs"], 10, n_probes=5), want)


def test_knn_brute_refuses_a_half_index(tk):
    g, data = _f32_fixture("an100")
    dev = fixture_ivf(g, data, store="float16").device_index()
    with pytest.raises(Exception, match="float32 vectors"):
        dev.knn_brute(g["qn"][:4], 5)
    plain = fixture_ivf(g, data).device_index()
    assert plain.knn_brute(g["qn"][:4], 5).shape == (4, 5)
