"""The lane replay without a duplicate test (heap.hip, RING): every lane keeps a ring of staged blocks of its own,
refilled every few insert rounds with the next blocks whose minimum is below the lane's bound.  Heap arrays (layout
included) and ids against the oracle at the smallest shapes that can break a ring: lists of 0, 1, 15, 16, 17 and
~400 rows probed together, lanes that finish far apart, totals that are no multiple of 16 blocks, partial and
several waves, heaps in registers only / with one LDS level / at the kernel's largest, the plain path pinned on and
with every query re-scanned, coalesced pairs of calls, a sharded home replay, and the kernel's own counters."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = (0, 1, 15, 16, 17)        # rows of the lists around centre 0 (the sixth keeps its ~400)


def _oracle_of(oracle, ivf):
    L = len(ivf.active_centers)
    return oracle.OracleIndex(ivf.pq.centers, 2, ivf.pq.R, ivf.pq.sqrt_n_blocks, ivf.active_centers,
                              ivf.pq_transformed_centers.packed,
                              [ivf.pq_transformed_points[i].packed if not isinstance(ivf.pq_transformed_points[i], np.ndarray)
                               else None for i in range(L)],
                              [0 if isinstance(ivf.pq_transformed_points[i], np.ndarray) else ivf.pq_transformed_points[i].size
                               for i in range(L)],
                              [ivf.ids[i] for i in range(L)], ivf.data)


@pytest.fixture(scope="module")
def setup(oracle):
    """20 000 x 100 angular rows in 50 lists of ~400; the five lists nearest to list 0 cut down to 0, 1, 15, 16 and
    17 rows (the rows cut are not in the index).  Queries 0..31: at centre 0 (its ten nearest
    lists hold all the short ones), 32..63: at the short lists' centres (with n_probes = 1 a single block, or none);
    the rest: anywhere."""
    from tinyknn_amd import IVF, FastPQ, _lib
    from tinyknn_amd.utils import group_data_by_indices, knn_brute
    assert _lib.device_count() >= 1, "no GPU visible"
    rng = np.random.default_rng(77)
    np.random.seed(77)                            # (the fit draws from the global generator)
    n, d, C = 20000, 100, 50
    cent = rng.standard_normal((C, d))
    X = (cent[rng.integers(C, size=n)] + 0.7 * rng.standard_normal((n, d))).astype(np.float32)
    ivf = IVF("angular", C, FastPQ(2))
    ivf.fit(X[:4000])
    data = X / np.linalg.norm(X, axis=1, keepdims=True)
    centers = np.ascontiguousarray(ivf.all_centers, dtype=np.float32)
    nearest = knn_brute(data, centers, k=1, metric="angular")
    members = np.bincount(nearest[:, 0], minlength=C)
    unit = centers / np.linalg.norm(centers, axis=1, keepdims=True)
    around = np.argsort(-(unit @ unit[0]), kind="stable")          # the lists a query at centre 0 probes, in order
    around = [int(c) for c in around if c != 0 and members[c] >= max(SMALL)][:len(SMALL)]
    keep = np.ones(n, bool)
    for c, rows in zip(around, SMALL):
        members = np.nonzero(nearest[:, 0] == c)[0]
        keep[members[rows:]] = False
    data, nearest = np.ascontiguousarray(data[keep]), nearest[keep]
    ivf.data = data
    ivf.active_centers = centers
    ivf.pq_transformed_centers = ivf.pq.transform(centers)
    groups, ivf.ids = group_data_by_indices(data, nearest, C)
    for i in range(C):
        ivf.pq_transformed_points[i] = ivf.pq.transform(groups[i])
    sizes = [len(x) for x in ivf.ids]
    assert [sizes[c] for c in around] == list(SMALL) and sizes[0] > 200
    nq = 130
    near = np.array([0] * 32 + [around[i % len(around)] for i in range(32)])
    qs = np.concatenate([centers[near] + 0.01 * rng.standard_normal((64, d)),
                         cent[rng.integers(C, size=nq - 64)] + 0.7 * rng.standard_normal((nq - 64, d))]).astype(np.float32)
    qn, qp = ivf._prepare(qs.copy())
    dev = ivf.device_index()
    dev.set_option(_lib.OPT_PAIR_NQ, 0)          # every batch size to the lane-per-query replay
    dev.set_option(_lib.OPT_REPLAY_LAZY, 0)      # ... in its staged form (short heaps would go lazy)
    return _lib, ivf, dev, _oracle_of(oracle, ivf), qn, np.ascontiguousarray(qp), around


_want = {}


def want(ox, qn, n_probes, R):
    """The oracle's ids, heap arrays and probe lists of all 130 queries, computed once per (n_probes, R)."""
    key = (n_probes, R)
    if key not in _want:
        ids, hi, hv, pr = [], [], [], []
        for q in qn:
            out, dbg = ox.query(q, 10, n_probes=n_probes, pass_1=R, debug=True)
            row = np.full(10, -1, np.int64)
            row[:len(out[:10])] = out[:10]
            ids.append(row), hi.append(dbg["heap_idx"]), hv.append(dbg["heap_val"]), pr.append(dbg["probes"])
        _want[key] = tuple(np.stack(a) for a in (ids, hi, hv, pr))
    return _want[key]


def check(setup, nq, n_probes, R):
    _lib, ivf, dev, ox, qn, qp, around = setup
    ids, hi, hv, pr = want(ox, qn, n_probes, R)
    out, dbg = dev.query_batch(qn[:nq], qp[:nq], 10, n_probes, pass_1=R, debug=True)
    last = dev.last_replay()
    assert last["form"] == _lib.REPLAY_LANES and last["lazy"] == 0, last
    np.testing.assert_array_equal(dbg["probes"], pr[:nq])
    np.testing.assert_array_equal(dbg["heap_val"], hv[:nq])
    np.testing.assert_array_equal(dbg["heap_idx"], hi[:nq])
    np.testing.assert_array_equal(out, ids[:nq])


def test_short_lists_are_probed_together_and_alone(setup):
    _lib, ivf, dev, ox, qn, qp, around = setup
    pr10, pr1 = want(ox, qn, 10, 111)[3], want(ox, qn, 1, 111)[3]
    # a query at centre 0 probes all five short lists beside long ones; alone, each short list is someone's only list
    assert all(set(around) <= set(p.tolist()) for p in pr10[:32])
    assert set(around) <= set(pr1[32:64, 0].tolist())
    sizes = np.array([len(x) for x in ivf.ids])
    blocks = ((sizes + 15) // 16)[pr10].sum(axis=1)
    assert (blocks % 16 != 0).any() and blocks.max() >= 200     # last minima window partly filled; several hundred blocks
    assert ((sizes + 15) // 16)[pr1[32:64, 0]].max() < 8 <= ((sizes + 15) // 16)[pr1[64:, 0]].max()


@pytest.mark.parametrize("nq", [5, 63, 64, 65, 130])
@pytest.mark.parametrize("n_probes", [1, 10])
def test_batch_sizes(setup, nq, n_probes):
    check(setup, nq, n_probes, 111)


@pytest.mark.parametrize("R", [3, 7, 8, 574])
@pytest.mark.parametrize("n_probes", [1, 10])
def test_heap_sizes(setup, R, n_probes):
    """3, 7: register levels only; 8: the first LDS level; 574: TK_LANES_MAX_R."""
    check(setup, 130, n_probes, R)


@pytest.mark.parametrize("limit", [None, -128])
@pytest.mark.parametrize("R", [17, 111])
def test_plain_path(setup, limit, R):
    """Plain sums behind the heads, pinned on; with the limit at -128 every query with a plain list fails the check
    (the bound when its first plain block is reached — often one the ring never staged) and is scanned again."""
    _lib, ivf, dev, ox, qn, qp, around = setup
    dev.set_scan_mode(2)
    dev.set_plain_scan("always")
    if limit is not None:
        dev.set_option(_lib.OPT_PLAIN_LIMIT, limit)
    try:
        check(setup, 130, 10, R)
        st = dev.plain_stats()
        assert st["plain_units"] > 0, st
        assert limit is None or st["flagged_queries"] > 0, st
    finally:
        dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
        dev.set_plain_scan(True)
        dev.set_scan_mode(0)


def test_pipelined_coalesced_pairs_of_unequal_calls(setup):
    import torch
    _lib, ivf, dev, ox, qn, qp, around = setup
    ids = want(ox, qn, 10, 111)[0]
    f64 = qp.dtype != np.float32
    dev.set_pipeline(2)
    dev.set_coalesce(2)
    try:
        st = torch.cuda.current_stream().cuda_stream
        q_dev, qp_dev = torch.from_numpy(qn).cuda(), torch.from_numpy(qp).cuda()
        esz, dq = (8 if f64 else 4), qp.shape[1]
        outs = []
        for a, e in [(0, 5), (5, 130), (0, 64), (64, 65), (65, 130), (0, 130), (3, 66)]:
            o = torch.full((e - a, 10), -1, dtype=torch.int64, device="cuda")
            outs.append((a, e, o))
            dev.query_batch_dev(q_dev.data_ptr() + a * qn.shape[1] * 4, qp_dev.data_ptr() + a * dq * esz, f64,
                                e - a, 10, 10, o.data_ptr(), stream=st)
        dev.join(st)
        torch.cuda.synchronize()
        assert dev.last_replay()["form"] == _lib.REPLAY_LANES
        for a, e, o in outs:
            np.testing.assert_array_equal(o.cpu().numpy(), ids[a:e])
    finally:
        dev.set_coalesce(1)
        dev.set_pipeline(1)


def test_sharded_home_replay(setup):
    """Two simulated ranks on one device: the home rank replays rows that arrived by the exchange."""
    from test_shard_gpu import simulate_world
    _lib, ivf, dev, ox, qn, qp, around = setup
    ids = want(ox, qn, 10, 111)[0]
    got, flags, _ = simulate_world(ivf, 2, qn, qp, 10, 10)
    assert not np.asarray(flags).any()
    np.testing.assert_array_equal(got, ids)


def test_replay_counters(setup, oracle):
    """One wave of 64 queries: the wave ran at least as many insert rounds as its busiest query has inserts (one
    insert per lane and round), and refilled its rings at least once."""
    _lib, ivf, dev, ox, qn, qp, around = setup
    sel = slice(64, 128)
    most = 0
    for q in qn[sel]:
        _, dbg = ox.query(q, 10, n_probes=10, debug=True)
        tt = oracle.transform_tables(dbg["table"])
        hi, hv = np.zeros(111, np.int64), np.zeros(111, np.int32)
        oracle.init_heap(hi, hv, True)
        n_ins = np.zeros(2, np.int64)
        for l in dbg["probes"]:
            t = ivf.pq_transformed_points[int(l)]
            if isinstance(t, np.ndarray) or t.size == 0:
                continue
            oracle.query_pq(t.packed, t.size, tt, hi, hv, True, labels=np.asarray(ivf.ids[int(l)], np.int64), stats=n_ins)
        np.testing.assert_array_equal(hv, dbg["heap_val"])
        most = max(most, int(n_ins[0]))
    assert most > 111
    dev.set_option(_lib.OPT_REPLAY_COUNT, 1)
    try:
        dev.query_batch(qn[sel], qp[sel], 10, 10, debug=True)
        st = dev.replay_stats()
    finally:
        dev.set_option(_lib.OPT_REPLAY_COUNT, 0)
    assert st["waves"] == 1 and st["segments"] >= 1, st
    assert most <= st["rounds"] == st["max_rounds_of_a_wave"], (most, st)
