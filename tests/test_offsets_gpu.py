"""Every row-addressed call on an index whose rows lie beyond the offsets where `rows + id * d` wraps in 32 bits
(DESIGN §5c): N = 2^25 + 2^16 rows of 128 float32 generated in HBM (17.2 GB) — the byte offset passes 2^32 at row
8 388 608, the element offset 2^31 at row 16 777 216 and 2^32 at row 33 554 432 — once as float32 and once narrowed to
half.  tests/offset_shapes.py makes the marked set S, the attributes that select it and the references;
tests/test_offsets_cpu.py pins those against the suite's references on a small shape.  Every comparison is exact: ids
equal, distances and part values bit for bit.

The host's copies of S's rows come from the seeded generator one row at a time and are never read from the device; the
first test holds read_rows against them, and from there on read_rows feeds the oracle's sparse vector file.

knn_brute and radius_search without n_probes take float32 vectors only (a half index refuses them), so their tests run
on the float32 index alone.  An exact copy's `part` is a few ulp of |x|^2 from zero on either side (±3e-5 here), so at the
radius 1e-6 the unrestricted radius call lists the row itself for some queries and nothing for the others — the reference
decides which — and at the radius that just admits every own part it lists exactly the row itself for all.
update runs on both stores; add and remove on the float32 index, last, in that order.  Needs 64 GB of HBM."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import offset_shapes as osh  # noqa: E402
from group_exact_reference import same_bits  # noqa: E402
from radius_probe_reference import same_csr  # noqa: E402
from store_reference import rounded  # noqa: E402

pytestmark = pytest.mark.gpu

K, P, ADD = 10, 10, 70_000
both = pytest.mark.parametrize("index", ["float32", "float16"], indirect=True)
f32 = pytest.mark.parametrize("index", ["float32"], indirect=True)


def synth(case, n, seed, row0=0):
    from tinyknn_amd.ivf import synth_rows
    return synth_rows(n, case.d, seed, case.centres, osh.SIGMA, row0=row0)


@pytest.fixture(scope="module")
def case():
    import torch
    if torch.cuda.mem_get_info()[1] < 64e9:
        pytest.skip("the index beyond 2^32 elements needs 64 GB of HBM")
    t0 = time.perf_counter()
    c = osh.Case()
    rows_S = np.concatenate([synth(c, 1, c.seed, row0=int(r)) for r in c.S])
    c.set_rows(rows_S, synth(c, osh.N_ANY, c.seed + 101))
    print(f"offsets: the case (S of {len(c.S)} rows, attributes of {c.n} rows) in {time.perf_counter() - t0:.2f} s")
    return c


class Built:
    pass


@pytest.fixture(scope="module")
def index(request, case, oracle, tmp_path_factory):
    """the index in the store asked for, its attributes set, the oracle on its exported lists and a sparse file"""
    store = request.param
    t0 = time.perf_counter()
    ivf = osh.unbuilt_ivf(case, synth(case, 100_000, case.seed))
    ivf.build_resident(case.n, case.d, case.seed, case.centres, osh.SIGMA, store=None if store == "float32" else store)
    t1 = time.perf_counter()
    b = Built()
    b.store, b.ivf, b.dev = store, ivf, ivf.device_index()
    osh.set_attributes(ivf, case)
    lists = b.dev.export_lists()
    assert lists[0].sum() == case.n and lists[0].min() > 0
    b.path = str(tmp_path_factory.mktemp("offsets") / "rows.f32")
    b.data = np.memmap(b.path, dtype=np.float32, mode="w+", shape=(case.n + ADD, case.d))        # sparse
    b.ox = osh.oracle_of(oracle, ivf, lists, b.data)
    del lists
    b.rows_S = case.rows_S if store == "float32" else rounded(case.rows_S)      # what the store holds of S
    b.rows_now = b.rows_S.copy()                                                # ... after update
    b.fetch = b.dev.read_rows
    qn, qp = ivf._prepare(case.Q_any.copy())
    b.qn, b.qp = np.ascontiguousarray(qn), np.ascontiguousarray(qp)
    print(f"offsets: {store} fixture in {time.perf_counter() - t0:.2f} s (build_resident {t1 - t0:.2f} s)")
    yield b
    b.dev.close()
    del b.ox, b.data
    try:
        os.unlink(b.path)
    except OSError:
        pass


def _prepared(b, q):
    qn, qp = b.ivf._prepare(np.ascontiguousarray(q, dtype=np.float32).copy())
    return np.ascontiguousarray(qn), np.ascontiguousarray(qp)


def _same_knn(got, want, what=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"ids {what}")
    assert same_bits(got[1], want[1]), f"distances {what}"


def _every_band(case, ids, what=""):
    ids = np.asarray(ids).ravel()
    seen = np.unique(osh.band_of(ids[ids >= 0], case.B))
    assert len(seen) == 4, (what, seen)


def _group(case, nq):
    return np.full(nq, osh.GROUP, dtype=np.int32)


# ---- first: the rows themselves ----------------------------------------------------------------------------------------

@both
def test_read_rows_returns_the_generated_rows(index, case):
    b, dev = index, index.dev
    assert dev.N == case.n and dev.store == b.store
    got = dev.read_rows(case.S)
    assert got.dtype == np.float32 and got.tobytes() == b.rows_S.tobytes()
    back = case.S[::-1].copy()
    assert dev.read_rows(back).tobytes() == np.ascontiguousarray(b.rows_S[::-1]).tobytes()
    f32_bytes = case.n * case.d * 4
    assert f32_bytes > 2**32
    assert dev.vector_bytes == (f32_bytes if b.store == "float32" else f32_bytes // 2)


# ---- the exact calls ---------------------------------------------------------------------------------------------------

@both
@pytest.mark.parametrize("k", [1, 10, 100])
def test_knn_group_and_knn_between(oracle, index, case, k):
    b, dev, q = index, index.dev, case.Q_S
    want = osh.group_reference(oracle, case, q, k, b.rows_S)
    _same_knn(dev.knn_group(q, k, _group(case, len(q)), return_distances=True), want, "knn_group")
    _every_band(case, want[0])
    if k == 1:
        np.testing.assert_array_equal(want[0][:, 0], case.src)
    between = case.restrictions(len(q))["between"]["between"]
    _same_knn(dev.knn_between(q, k, between, return_distances=True),
              osh.between_reference(oracle, case, q, k, b.rows_S), "knn_between")


@f32
def test_knn_brute_restricted_to_the_marked_rows(index, case):
    dev, q = index.dev, case.Q_S
    part = osh.part_S(case, q)
    for name, kw in case.restrictions(len(q)).items():
        for k in (1, 10):
            ids, dist = dev.knn_brute_dist(q, k, **kw)
            want = osh.brute_reference(case, q, k, part)
            np.testing.assert_array_equal(ids, want[0], err_msg=name)
            assert dist.dtype == np.float32 and dist.tobytes() == want[1].tobytes(), name
            np.testing.assert_array_equal(dev.knn_brute(q, k, **kw), want[0], err_msg=name)
    _every_band(case, want[0])


@f32
def test_knn_brute_and_radius_search_on_exact_copies(index, case):
    dev, q = index.dev, case.Q0
    part = osh.part_S(case, q)
    own = part[np.arange(len(q)), case.at(case.q0_rows)]
    ids, dist = dev.knn_brute_dist(q, 1)
    np.testing.assert_array_equal(ids[:, 0], case.q0_rows)
    assert dist[:, 0].tobytes() == own.tobytes()
    np.testing.assert_array_equal(dev.knn_brute(q, 1)[:, 0], case.q0_rows)
    for r in (np.float32(1e-6), osh.own_radius(case, part)):
        want = osh.radius_reference(case, part, r)
        same_csr(dev.radius_brute(q, r), want, f"radius {r}")
        np.testing.assert_array_equal(dev.radius_count(q, r), np.diff(want[0]))
        assert (np.diff(want[0]) <= 1).all()
    np.testing.assert_array_equal(want[1], case.q0_rows)        # (the last radius: every query's own row, nothing else)


@f32
def test_radius_search_inside_the_marked_group(index, case):
    dev, q = index.dev, case.Q_S
    part = osh.part_S(case, q)
    r = osh.kth_part(part, 20)
    want = osh.radius_reference(case, part, r)
    assert (np.diff(want[0]) >= 20).all()
    group = _group(case, len(q))
    same_csr(dev.radius_brute(q, r, group=group), want)
    np.testing.assert_array_equal(dev.radius_count(q, r, group=group), np.diff(want[0]))
    _every_band(case, want[1])


# ---- the calls that go through the lists -------------------------------------------------------------------------------

@both
def test_radius_search_over_the_probed_lists(oracle, index, case):
    b, dev = index, index.dev
    qn, qp = b.qn[:16], b.qp[:16]
    everything, probes = osh.probe_reference(oracle, b.ox, qn, np.inf, P, b.data, b.fetch, n=case.n)
    _every_band(case, everything[1])
    r = osh.kth_dist(everything, 10)
    want, _ = osh.probe_reference(oracle, b.ox, qn, r, P, b.data, None, n=case.n)
    assert (np.diff(want[0]) >= 10).all()
    same_csr(dev.radius_probe(qn, qp, r, P), want, "bare")
    np.testing.assert_array_equal(dev.radius_probe_count(qn, qp, r, P), np.diff(want[0]))
    group = osh.nearest_groups(case, everything)
    oks = osh.group_masks(case, group, len(b.data))
    want, _ = osh.probe_reference(oracle, b.ox, qn, np.inf, P, b.data, None, oks=oks, n=case.n)
    assert (np.diff(want[0]) >= 1).all()
    same_csr(dev.radius_probe(qn, qp, np.inf, P, group=group), want, "group=")


@both
def test_query_batch_with_distances(oracle, index, case):
    b, dev, qn, qp = index, index.dev, index.qn, index.qp
    ids, dist, heaps = osh.batch_reference(oracle, b.ox, qn, K, P, b.data, b.fetch)
    _every_band(case, ids, "the compared rows")
    assert (ids >= 0).all()
    _same_knn(dev.query_batch(qn, qp, K, P, return_distances=True), (ids, dist), "query_batch")
    np.testing.assert_array_equal(dev.query_batch(qn, qp, K, P), ids)
    want = osh.capped_reference(oracle, b.ox, qn, heaps, 1, case.groups, K)
    _every_band(case, want[0], "per_group=1")
    _same_knn(dev.query_batch(qn, qp, K, P, per_group=1, return_distances=True), want, "per_group=1")
    tag = 1 << osh.TAG_BIT
    for name, q in (("Q_any", qn[:32]), ("Q_S", case.Q_S)):
        q, p = _prepared(b, q)
        want = osh.tagged_reference(oracle, case, b.ox, q, K, P, b.data, b.rows_S)
        _same_knn(dev.query_batch(q, p, K, P, tags=tag, return_distances=True), want, f"tags= {name}")
    _every_band(case, want[0], "tags= on Q_S")


@both
def test_query_rows_gathers_rows_beyond_every_boundary(oracle, index, case):
    b, dev, rows = index, index.dev, case.src
    qn, qp = dev.gather_queries(rows)
    assert qn.tobytes() == np.ascontiguousarray(b.rows_S[case.at(rows)]).tobytes()
    assert np.array_equal(qp[:, :case.d], qn) and not qp[:, case.d:].any()
    want = osh.rows_reference(oracle, b.ox, rows, qn, qp, K, P, b.data, b.fetch)
    assert not (want[0] == rows[:, None]).any() and (want[0] >= 0).all()
    _same_knn(dev.query_rows(rows, K, P, return_distances=True), want, "query_rows")


# ---- last: the calls that change the index ------------------------------------------------------------------------------

def _updated_rows(case):
    """about 200 rows of S: the four round every boundary and 47 more of every band"""
    rng = np.random.RandomState(case.seed + 20)
    band = osh.band_of(case.S, case.B)
    return np.unique(np.concatenate([osh.around(case.B)] + [rng.choice(case.S[band == i], 47, replace=False)
                                                            for i in range(4)])).astype(np.int64)


@both
def test_update_writes_rows_beyond_every_boundary(oracle, index, case):
    b, dev = index, index.dev
    ids = _updated_rows(case)
    assert 180 <= len(ids) <= 200 and np.isin(osh.around(case.B), ids).all()
    X = synth(case, len(ids), case.seed + 7)
    beside = np.setdiff1d(osh.around(case.B, -3, 2), osh.around(case.B))          # b - 3 and b + 2
    assert len(beside) == 6 and not np.isin(beside, ids).any()
    was = np.concatenate([synth(case, 1, case.seed, row0=int(r)) for r in beside])
    assert b.ivf.update(ids, X) is b.ivf and dev.N == case.n
    new = X if b.store == "float32" else rounded(X)
    assert dev.read_rows(ids).tobytes() == new.tobytes()
    assert dev.read_rows(beside).tobytes() == (was if b.store == "float32" else rounded(was)).tobytes()
    b.rows_now[case.at(ids)] = new
    assert dev.read_rows(case.S).tobytes() == b.rows_now.tobytes()
    q = (X + 1e-3 * np.random.RandomState(3).randn(*X.shape)).astype(np.float32)
    want = osh.group_reference(oracle, case, q, K, b.rows_now)
    np.testing.assert_array_equal(want[0][:, 0], ids)
    _same_knn(dev.knn_group(q, K, _group(case, len(q)), return_distances=True), want, "knn_group after update")
    _same_knn(dev.knn_between(q, K, case.restrictions(len(q))["between"]["between"], return_distances=True),
              osh.between_reference(oracle, case, q, K, b.rows_now), "knn_between after update")


@f32
def test_add_grows_the_store_past_a_multiple_of_65536_rows(oracle, index, case):
    b, dev = index, index.dev
    n0 = dev.N
    assert n0 == case.n and n0 // 2**16 < (n0 + ADD) // 2**16
    X = synth(case, ADD, case.seed + 8)
    b.ivf.add(X, groups=np.full(ADD, osh.GROUP + 1, np.int32), tags=np.zeros(ADD, np.uint64),
              values=np.full(ADD, -1, np.int64))
    assert dev.N == n0 + ADD and dev.vector_bytes == (n0 + ADD) * case.d * 4
    at = np.array([0, ADD // 2, ADD - 1])
    assert dev.read_rows(n0 + at).tobytes() == np.ascontiguousarray(X[at]).tobytes()
    assert dev.read_rows(case.S).tobytes() == b.rows_now.tobytes()         # (the store moved: every old row with it)
    np.testing.assert_array_equal(dev.knn_brute(X[at], 1)[:, 0], n0 + at)
    q = case.Q_S
    _same_knn(dev.knn_group(q, K, _group(case, len(q)), return_distances=True),
              osh.group_reference(oracle, case, q, K, b.rows_now), "knn_group after add")


@f32
def test_removed_rows_leave_knn_group_and_the_probed_radius_search(oracle, index, case):
    b, dev = index, index.dev
    assert dev.N == case.n + ADD, "runs behind the add test"
    gone = np.unique(np.concatenate([case.S[::6][:94], osh.around(case.B)[1::2]])).astype(np.int64)
    assert 90 <= len(gone) <= 100
    b.ivf.remove(gone)
    keep = ~np.isin(case.S, gone)
    q = (b.rows_now[case.at(case.src)] + 1e-3 * np.random.RandomState(4).randn(osh.N_QS, case.d)).astype(np.float32)
    want = osh.group_reference(oracle, case, q, K, b.rows_now, keep=keep)
    assert not np.isin(want[0], gone).any()
    _same_knn(dev.knn_group(q, K, _group(case, len(q)), return_distances=True), want, "knn_group after remove")
    # the lists as they are now, exported again; the sources round the boundaries and four more as queries
    lists = dev.export_lists()
    assert lists[0].sum() == case.n + ADD - len(gone)
    ox = osh.oracle_of(oracle, b.ivf, lists, b.data)
    del lists
    qn, qp = _prepared(b, q[:16])
    want, _ = osh.probe_reference(oracle, ox, qn, np.inf, P, b.data, b.fetch)
    assert not np.isin(want[1], gone).any()
    listed = np.array([case.src[i] in want[1][want[0][i]:want[0][i + 1]] for i in range(16)])
    kept = ~np.isin(case.src[:16], gone)
    assert 4 <= kept.sum() <= 12 and listed[kept].any() and not listed[~kept].any()
    got = dev.radius_probe(qn, qp, np.inf, P)
    assert not np.isin(got[1], gone).any()
    same_csr(got, want, "after remove")
