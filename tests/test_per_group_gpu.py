"""per_group= on the device (cap_select.h, the capped kernels of rescore.hip, tk_index_query_batch[_dev]_ex6;
IVF.query / query_batch / query_rows, DeviceIndex.query_batch / query_rows / query_batch_dev).  Every comparison is
exact — ids, counts and the bits of the distances — against tests/per_group_reference.py: the guarded CPU reference's
heap, oracle.sqdist_gather, a stable argsort and the walk of DESIGN §3.15 in plain Python.  The default cases are those
of tests/per_group_shapes.py, whose census tests/test_per_group_cpu.py asserts."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import per_group_shapes as shapes  # noqa: E402
from conftest import G6_TAGS, golden  # noqa: E402
from per_group_reference import capped_batch, capped_from_heaps, heaps_of  # noqa: E402
from per_group_shapes import K, N_PROBES  # noqa: E402
from store_reference import fixture_ivf, oracle_index, rounded  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    return tinyknn_amd


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got_ids, got_dist, want, msg=""):
    """ids, counts and distance bits against capped_batch's (ids, distances, counts)"""
    ids, dist, counts = want[:3]
    np.testing.assert_array_equal(got_ids, ids, err_msg=f"ids {msg}")
    np.testing.assert_array_equal((got_ids != -1).sum(axis=1), counts, err_msg=f"counts {msg}")
    if got_dist is not None:
        assert got_dist.dtype == dist.dtype, (got_dist.dtype, dist.dtype, msg)
        np.testing.assert_array_equal(_bits(got_dist), _bits(dist), err_msg=f"distance bits {msg}")


def _synthetic_device():
    ivf, ox, qn, qp, groups = shapes.synthetic()
    if ivf.groups is None:
        ivf.set_groups(groups)
    return ivf, ivf.device_index(), ox, qn, qp, groups


# ---- the default cases: every fixture, every assignment, every cap ----------------------------------------------------

@pytest.mark.parametrize("tag", G6_TAGS)
def test_fixtures_every_assignment_and_cap(tk, oracle, tag):
    ivf, ox, qn, qp = shapes.fixture(tag)
    dev = ivf.device_index()
    N = len(ox.data)
    plain = dev.query_batch(qn, qp, K, N_PROBES, return_distances=True)
    for a in shapes.ASSIGNMENTS:
        ivf.set_groups(shapes.assignment(a, N))
        for m in shapes.CAPS:
            case = (tag, a, m, N_PROBES, False)
            want = shapes.reference(case)
            arg = shapes.caps(m, len(qn))
            ids, dist = dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=arg)
            _same(ids, dist, want, case)
            _same(dev.query_batch(qn, qp, K, N_PROBES, per_group=arg), None, want, (case, "ids alone"))
            if a == "own" or m == K:        # all-distinct groups, and a cap no group can reach: the uncapped call
                np.testing.assert_array_equal(ids, plain[0])
                np.testing.assert_array_equal(_bits(dist), _bits(plain[1]))
        # m = 0: the call without per_group=, by the kernels an uncapped call takes
        ids, dist = dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=0)
        np.testing.assert_array_equal(ids, plain[0])
        np.testing.assert_array_equal(_bits(dist), _bits(plain[1]))
    ivf.set_groups(None)


# ---- equal distances (the tie fallback of the staged body) and short heaps -------------------------------------------

@pytest.mark.parametrize("m", shapes.CAPS)
def test_rows_stored_twice(tk, oracle, m):
    ivf, dev, ox, qn, qp, groups = _synthetic_device()
    case = ("syn", "syn8", m, N_PROBES, False)
    ids, dist, counts, ranked = shapes.reference(case, full=True)
    assert sum(len(c) > K and len(np.unique(d)) < len(d) for c, d in ranked) >= 8      # rankings with a tie
    arg = shapes.caps(m, len(qn))
    _same(*dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=arg), (ids, dist, counts), case)
    _same(dev.query_batch(qn, qp, K, N_PROBES, per_group=arg), None, (ids, dist, counts), case)


@pytest.mark.parametrize("m", [1, 2])
def test_short_and_empty_heaps(tk, oracle, m):
    ivf, dev, ox, qn, qp, groups = _synthetic_device()
    case = ("syn", "syn8", m, 1, True)
    ids, dist, counts, ranked = shapes.reference(case, full=True)
    sizes = [len(c) for c, _ in ranked]
    assert min(sizes) == 0 and 0 < max(sizes) <= K          # nc = 0 and 0 < nc <= k: the no-rescoring branch
    few = shapes.synthetic_few()
    _same(*dev.query_batch(qn, qp, K, 1, return_distances=True, allowed=few, per_group=m), (ids, dist, counts), case)
    _same(dev.query_batch(qn, qp, K, 1, allowed=few, per_group=m), None, (ids, dist, counts), case)


# ---- every rescoring form ---------------------------------------------------------------------------------------------

def test_every_rescoring_form(tk, oracle):
    from tinyknn_amd import _lib
    ivf, dev, ox, qn, qp, groups = _synthetic_device()
    m = shapes.caps("mix", len(qn))
    m[:4] = 1
    want = capped_from_heaps(oracle, ox, qn, shapes.heaps("syn", N_PROBES), m, groups, K)
    # pass_1 = 300: a heap beyond the staged kernels' 256 entries: the lane-per-row kernel alone, whatever the form is
    # set to (the staged kernels beyond one chunk: tests/test_per_group_edges_gpu.py)
    big = capped_batch(oracle, ox, qn, m, groups, K, N_PROBES, pass_1=300)
    try:
        for form in (0, 1, 2):
            dev.set_option(_lib.OPT_RESCORE_FORM, form)
            _same(*dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=m), want, ("form", form))
            _same(dev.query_batch(qn, qp, K, N_PROBES, per_group=m), None, want, ("form", form, "ids alone"))
            _same(*dev.query_batch(qn, qp, K, N_PROBES, 300, return_distances=True, per_group=m), big,
                  ("form", form, "pass_1 300"))
    finally:
        dev.set_option(_lib.OPT_RESCORE_FORM, 2)


@pytest.mark.parametrize("d_tag", ["an100", "eu20"])
def test_half_store(tk, oracle, d_tag):
    from tinyknn_amd import _lib
    g = golden(f"g6_ivf_{d_tag}.npz")
    data = rounded(g["data"])
    ivf = fixture_ivf(g, data, store="float16")
    ox = oracle_index(oracle, ivf, data)
    groups = shapes.assignment("mod3", len(data))
    ivf.set_groups(groups)
    dev = ivf.device_index()
    assert dev.store == "float16"
    qn, qp = g["qn"], g["qpq"]
    m = shapes.caps("mix", len(qn))
    want = capped_batch(oracle, ox, qn, m, groups, K, N_PROBES)
    big = capped_batch(oracle, ox, qn, m, groups, K, N_PROBES, pass_1=300)
    try:
        for form in (0, 1, 2):
            dev.set_option(_lib.OPT_RESCORE_FORM, form)
            _same(*dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=m), want, ("half", form))
        _same(*dev.query_batch(qn, qp, K, N_PROBES, 300, return_distances=True, per_group=m), big, "half, pass_1 300")
    finally:
        dev.set_option(_lib.OPT_RESCORE_FORM, 2)


def test_float64_vectors(tk, oracle):
    ivf, ox, qn, qp = shapes.fixture("eu20f64")
    assert ox.data.dtype == np.float64
    groups = shapes.assignment("oct", len(ox.data))
    ivf.set_groups(groups)
    dev = ivf.device_index()
    for pass_1 in (None, 300):
        want = capped_batch(oracle, ox, qn, 1, groups, K, N_PROBES, pass_1=pass_1)
        ids, dist = dev.query_batch(qn, qp, K, N_PROBES, pass_1, return_distances=True, per_group=1)
        assert dist.dtype == np.float64
        _same(ids, dist, want, ("float64", pass_1))
    ivf.set_groups(None)


# ---- with the restrictions -------------------------------------------------------------------------------------------

def test_with_every_restriction(tk, oracle):
    ivf, dev, ox, qn, qp, groups = _synthetic_device()
    nq, N = len(qn), shapes.SYN_N
    rng = np.random.default_rng(12)
    allowed = rng.random(N) < 0.5
    plain = dev.query_batch(qn, qp, K, N_PROBES)
    exclude = plain[:, 0].copy()                    # every query's best row may not come back
    row_tags = (np.uint64(1) << (np.arange(N) % 7).astype(np.uint64)).astype(np.uint64)
    values = (np.arange(N) % 100).astype(np.int64)
    legs = [("allowed", dict(allowed=allowed), dict(allowed=allowed)),
            ("exclude", dict(exclude=exclude), dict(exclude=exclude))]
    for name, kw, ref in legs:
        want = capped_batch(oracle, ox, qn, 1, groups, K, N_PROBES, **ref)
        _same(*dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=1, **kw), want, name)
    # group= restricts by the very ids the cap counts: at most m rows in all
    g_q = (np.arange(nq) % 8).astype(np.int32)
    want = capped_batch(oracle, ox, qn, 2, groups, K, N_PROBES, group=g_q)
    assert want[2].max() <= 2
    _same(*dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=2, group=g_q), want, "group")
    ivf.set_tags(row_tags)
    ivf.set_values(values)
    try:
        t_q = np.full(nq, 0b0010110, dtype=np.uint64)
        want = capped_batch(oracle, ox, qn, 1, groups, K, N_PROBES, tags=t_q, row_tags=row_tags)
        _same(*dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=1, tags=t_q), want, "tags")
        lo, hi = np.full(nq, 20), np.full(nq, 79)
        want = capped_batch(oracle, ox, qn, 1, groups, K, N_PROBES, between=(lo, hi), values=values)
        _same(*dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=1, between=(lo, hi)), want,
              "between")
    finally:
        ivf.set_tags(None)
        ivf.set_values(None)


def test_query_rows_with_exclude_self(tk, oracle):
    ivf, dev, ox, qn, qp, groups = _synthetic_device()
    rows = np.array([0, 3, 27, 30, 1000, 1003, 1020, 555, 555, 1999], dtype=np.int64)       # repeated rows among them
    rq, rp = dev.gather_queries(rows)
    for exclude_self in (True, False):
        want = capped_batch(oracle, ox, rq, 1, groups, K, N_PROBES, exclude=rows if exclude_self else None, q_pq=rp)
        for who in (dev, ivf):
            ids, dist = who.query_rows(rows, K, N_PROBES, exclude_self=exclude_self, return_distances=True, per_group=1)
            _same(ids, dist, want, ("query_rows", exclude_self))
        if exclude_self:
            assert not (want[0] == rows[:, None]).any()
    # (the last leg, nothing excluded: row 0 or its copy, row 1000, leads row 0's answer at distance 0; one group, m = 1:
    #  the other is dropped)
    assert want[1][0, 0] == 0.0 and want[0][0, 0] in (0, 1000) and not {0, 1000} <= set(want[0][0].tolist())


# ---- the call path: pairs, sub-batches, the single query -------------------------------------------------------------

def test_capped_and_uncapped_calls_interleaved_in_the_pipeline(tk, oracle):
    import torch
    ivf, dev, ox, qn, qp, groups = _synthetic_device()
    nq = len(qn)
    m_a = shapes.caps("mix", nq)
    m_b = np.roll(m_a, 1)
    h = shapes.heaps("syn", N_PROBES)
    want = {"a": capped_from_heaps(oracle, ox, qn, h, m_a, groups, K),
            "b": capped_from_heaps(oracle, ox, qn, h, m_b, groups, K),
            None: capped_from_heaps(oracle, ox, qn, h, 0, groups, K)}
    st = torch.cuda.current_stream().cuda_stream
    q_dev, qp_dev = torch.from_numpy(qn).cuda(), torch.from_numpy(qp).cuda()
    caps_dev = {"a": torch.from_numpy(m_a).cuda(), "b": torch.from_numpy(m_b).cuda()}
    f64 = qp.dtype != np.float32
    SENT = -7.0
    # capped + capped pair up (each half its own array), capped / uncapped neighbours do not; with and without distances
    calls = [("a", True), ("b", True), (None, True), ("a", False), (None, False), ("b", True), ("a", True), (None, True),
             (None, False), ("b", False)]
    try:
        dev.set_pipeline(2)
        dev.set_coalesce(2)
        outs = []
        for rep in range(2):
            for which, wd in calls:
                o = torch.full((nq, K), -7, dtype=torch.int64, device="cuda")
                od = torch.full((nq, K), SENT, dtype=torch.float32, device="cuda")
                outs.append((which, wd, o, od))
                dev.query_batch_dev(q_dev.data_ptr(), qp_dev.data_ptr(), f64, nq, K, N_PROBES, o.data_ptr(), stream=st,
                                    dist_ptr=od.data_ptr() if wd else None,
                                    per_group_ptr=None if which is None else caps_dev[which].data_ptr())
        dev.join(st)
        torch.cuda.synchronize()
    finally:
        dev.set_coalesce(1)
        dev.set_pipeline(1)
    for j, (which, wd, o, od) in enumerate(outs):
        if wd:
            _same(o.cpu().numpy(), od.cpu().numpy(), want[which], f"call {j}")
        else:
            _same(o.cpu().numpy(), None, want[which], f"call {j}")
            assert (od.cpu().numpy() == SENT).all(), f"call {j} asked for no distances"


def test_a_call_beyond_one_sub_batch(tk, oracle):
    ivf, dev, ox, qn, qp, groups = _synthetic_device()
    ms = dev.max_sub_batch(K, N_PROBES)
    reps = -(-(ms + 37) // len(qn))
    sel = np.tile(np.arange(len(qn)), reps)[:ms + 37]
    m = (np.arange(len(sel)) % 4).astype(np.int32)           # a cap of its own per row: the parts' offsets matter
    base = {c: capped_from_heaps(oracle, ox, qn, shapes.heaps("syn", N_PROBES), c, groups, K) for c in range(4)}
    want = tuple(np.stack([base[int(c)][part][i] for i, c in zip(sel, m)]) for part in range(3))
    assert len(sel) > ms
    ids, dist = dev.query_batch(np.ascontiguousarray(qn[sel]), np.ascontiguousarray(qp[sel]), K, N_PROBES,
                                return_distances=True, per_group=m)
    _same(ids, dist, want, ("beyond one sub-batch", ms, len(sel)))


def test_single_query_and_the_batch_of_the_ivf(tk, oracle):
    ivf, dev, ox, qn, qp, groups = _synthetic_device()
    h = shapes.heaps("syn", N_PROBES)
    want = capped_from_heaps(oracle, ox, qn, h, 1, groups, K)
    qs = np.array(qn, copy=True)        # (euclidean, unrotated: the preparation leaves the rows as they are)
    np.testing.assert_array_equal(ivf._prepare(qs.copy())[0], qn)
    _same(*ivf.query_batch(qs, K, N_PROBES, return_distances=True, per_group=1), want, "IVF.query_batch")
    shorter = 0
    for i in range(len(qs)):
        n = int(want[2][i])
        ids, dist = ivf.query(qs[i].copy(), K, N_PROBES, return_distances=True, per_group=1)
        np.testing.assert_array_equal(ids, want[0][i][:n])
        np.testing.assert_array_equal(_bits(dist), _bits(want[1][i][:n]))
        np.testing.assert_array_equal(ivf.query(qs[i].copy(), K, N_PROBES, per_group=1), ids)
        shorter += n < K
    assert shorter > 0                  # the variable-length arrays of IVF.query
    np.testing.assert_array_equal(ivf.query(qs[0].copy(), K, N_PROBES, per_group=0), ivf.query(qs[0].copy(), K, N_PROBES))


# ---- after the lists change; without groups ---------------------------------------------------------------------------

def test_after_add_and_remove(tk, oracle):
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(77)
    d, n, n_new = 20, 1500, 300
    cent = rng.randn(12, d) * 2.0
    X = (cent[rng.randint(12, size=n)] + 0.5 * rng.randn(n, d)).astype(np.float32)
    Y = (cent[rng.randint(12, size=n_new)] + 0.5 * rng.randn(n_new, d)).astype(np.float32)
    qs = (cent[rng.randint(12, size=24)] + 0.5 * rng.randn(24, d)).astype(np.float32)
    ivf = IVF("euclidean", 12, FastPQ(2, rotate_dim=None))
    np.random.seed(78)
    ivf.fit(X).build(X, n_probes=1)
    groups = (np.arange(n) % 40).astype(np.int32)
    ivf.set_groups(groups)
    dev = ivf.device_index()
    qn, qp = ivf._prepare(qs.copy())
    dev.query_batch(qn, qp, K, N_PROBES, per_group=1)          # (the tables of the first layout exist)
    new_groups = np.full(n_new, 7, dtype=np.int32)              # every new row in ONE old group
    ivf.add(Y, groups=new_groups)
    ivf.remove(np.arange(0, n, 3))
    all_groups = np.concatenate([groups, new_groups])
    ox = oracle_index(oracle, ivf, ivf.data)
    want = capped_batch(oracle, ox, qn, 1, all_groups, K, N_PROBES)
    ids, dist = dev.query_batch(qn, qp, K, N_PROBES, return_distances=True, per_group=1)
    _same(ids, dist, want, "after add and remove")
    new_seen = (ids >= n).sum(axis=1)
    assert new_seen.max() == 1 and new_seen.sum() > 0           # the added rows are found, one of their group at most
    assert not np.isin(ids, np.arange(0, n, 3)).any()
    uncapped = dev.query_batch(qn, qp, K, N_PROBES)
    assert ((uncapped >= n).sum(axis=1) > 1).any()              # ... where the uncapped call returns several


def test_without_groups_it_raises_what_group_raises(tk, oracle):
    from tinyknn_amd import _lib
    g = golden("g6_ivf_an20.npz")
    ivf = fixture_ivf(g)
    dev = ivf.device_index()
    qn, qp = g["qn"], g["qpq"]
    errors = []
    for kw in (dict(group=1), dict(per_group=1)):
        with pytest.raises(_lib.TinyKnnHipError) as e:
            dev.query_batch(qn, qp, K, N_PROBES, **kw)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "tk_index_set_groups first" in errors[0]
    # an array of zeros caps nothing and needs no groups; a negative entry is the library's argument error
    np.testing.assert_array_equal(dev.query_batch(qn, qp, K, N_PROBES, per_group=0), dev.query_batch(qn, qp, K, N_PROBES))
    out = np.full((len(qn), K), -9, dtype=np.int64)
    bad = np.full(len(qn), -1, dtype=np.int32)
    rc = _lib.lib().tk_index_query_batch_ex6(
        dev._h, None, None, None, None, 0, None, bad.ctypes.data, _lib.ptr(qn, _lib._f32p), qp.ctypes.data,
        int(qp.dtype != np.float32), len(qn), K, N_PROBES, 0, _lib.ptr(out, _lib._i64p), None, None, None, None)
    assert rc == -1 and "per_group" in _lib.lib().tk_last_error().decode() and (out == -9).all()
    # a heap whose ranking does not fit the rescoring's LDS is refused, not truncated
    ivf.set_groups(shapes.assignment("mod3", len(g["data"])))
    with pytest.raises(AssertionError, match="per_group"):
        dev.query_batch(qn, qp, K, N_PROBES, 3000, per_group=1)
    assert dev.query_batch(qn, qp, K, N_PROBES, 3000).shape == (len(qn), K)
