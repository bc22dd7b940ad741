"""Every row within a radius among the rows of the probed lists (tk_index_radius_probe) against its
reference (tests/radius_probe_reference.py): lims, ids and dist byte for byte unless stated.  The golden fixtures in
every store, radii on the boundary, list lengths at the edges of the 64-row word and the 256-row pass, probe rows that
wrap, every restriction, the lists changing under it, and the calls that must agree with it."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from brute_reference import int_part  # noqa: E402
from conftest import golden  # noqa: E402
from radius_probe_reference import (candidates, oracle_probes, passes, radius_probe_csr, same_csr,  # noqa: E402
                                    same_sets)
from restricted_shapes import probed_lists  # noqa: E402
from store_reference import fixture_ivf, oracle_index, rounded  # noqa: E402

pytestmark = pytest.mark.gpu


def _kth(want_inf, k):
    """Every query's k-th distance of the reference at radius +inf as a float32 radius that admits it (+inf where it
    lists fewer): a float64 distance is rounded UP to the next float32, the call compares dist <= float64(float32(r))"""
    lims, _, dist = want_inf
    kth = np.array([dist[a + k - 1] if b - a >= k else np.inf for a, b in zip(lims[:-1], lims[1:])], dtype=np.float64)
    r = kth.astype(np.float32)
    low = r.astype(np.float64) < kth
    r[low] = np.nextafter(r[low], np.float32(np.inf))
    return r


def _ask(dev, ox, oracle, qn, qpq, data, r, P, probes=None, oks=None, what="", **kw):
    """radius_probe, its unsorted form and its count against the reference; -> (got, want)"""
    want = radius_probe_csr(oracle, ox, qn, data, r, P, oks=oks, probes=probes)
    got = dev.radius_probe(qn, qpq, r, P, **kw)
    same_csr(got, want, what)
    np.testing.assert_array_equal(dev.radius_probe_count(qn, qpq, r, P, **kw), np.diff(want[0]), err_msg=what)
    same_sets(dev.radius_probe(qn, qpq, r, P, sort=False, **kw), want, what)
    return got, want


# ---- 1. the golden fixtures, every store ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(tag, store):
    from oracle import oracle
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = fixture_ivf(g, store=store)
    data = rounded(g["data"]) if store == "float16" else g["data"]
    ox = oracle_index(oracle, ivf, data)
    qn, qpq = np.ascontiguousarray(g["qn"]), np.ascontiguousarray(g["qpq"])
    return ivf, ivf.device_index(), ox, qn, qpq, data


@pytest.mark.parametrize("tag,store", [("eu20", None), ("an20", None), ("an100", None), ("an100b2", None),
                                       ("eu128", None), ("eu20f64", None), ("eu20", "float16"), ("an100", "float16"),
                                       ("an100b2", "float16"), ("eu128", "float16")])
def test_fixtures(oracle, tag, store):
    ivf, dev, ox, qn, qpq, data = _fixture(tag, store)
    dt = np.float64 if tag == "eu20f64" else np.float32
    assert data.dtype == dt
    for P in (1, 2, 5, 10, ox.n_lists, ox.n_lists + 3):
        probes = oracle_probes(ox, qn, P)
        everything = radius_probe_csr(oracle, ox, qn, data, np.inf, P, probes=probes)
        np.testing.assert_array_equal(np.diff(everything[0]), [len(candidates(ox, p, len(data))) for p in probes])
        for k in (1, 50):
            r = _kth(everything, k)
            got, want = _ask(dev, ox, oracle, qn, qpq, data, r, P, probes=probes, what=f"{tag} P={P} k={k}")
            assert got[2].dtype == dt and (np.diff(want[0]) >= np.minimum(k, np.diff(everything[0]))).all()
        _ask(dev, ox, oracle, qn, qpq, data, float(np.median(_kth(everything, 20))), P, probes=probes, what="scalar")
        _ask(dev, ox, oracle, qn, qpq, data, np.inf, P, probes=probes, what="inf")
        got, _ = _ask(dev, ox, oracle, qn, qpq, data, -1.0, P, probes=probes, what="negative")
        assert got[0][-1] == 0 and len(got[1]) == 0


def test_a_row_in_two_probed_lists_is_listed_once(oracle):
    ivf, dev, ox, qn, qpq, data = _fixture("an100b2", None)
    N = len(data)
    where = [[] for _ in range(N)]
    for l in range(ox.n_lists):
        for j in ox.ids[ox.ids_off[l]:ox.ids_off[l + 1]]:
            where[j].append(l)
    assert all(len(w) == 2 for w in where)
    both = 0
    for P in (2, 5, 10):
        probes = oracle_probes(ox, qn, P)
        r = _kth(radius_probe_csr(oracle, ox, qn, data, np.inf, P, probes=probes), 50)
        got, want = _ask(dev, ox, oracle, qn, qpq, data, r, P, probes=probes)
        for i in range(len(qn)):
            hits = got[1][got[0][i]:got[0][i + 1]]
            assert len(np.unique(hits)) == len(hits)
            lists = set(probed_lists(probes[i], ox.n_lists).tolist())
            both += sum(set(where[j]) <= lists for j in hits)
    assert both > 0                     # hits with both their lists probed: a wrong dedupe would list them twice


def test_radius_zero_on_a_query_copied_from_a_stored_row(oracle):
    ivf, dev, ox, qn, qpq, data = _fixture("eu20", None)
    rows = np.array([7, 300, 1200])
    Q = np.ascontiguousarray(data[rows], dtype=np.float32)
    qn2, qp2 = ivf._prepare(Q.copy())
    got, want = _ask(dev, ox, oracle, qn2, qp2, data, 0.0, 5)
    np.testing.assert_array_equal(got[0], [0, 1, 2, 3])
    np.testing.assert_array_equal(got[1], rows)
    assert (got[2] == 0).all()


# ---- 2. list lengths at the edges -------------------------------------------------------------------------------------
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 2049, 300]          # the last list: 300 identical rows


@functools.lru_cache(maxsize=None)
def _edges(d):
    """A euclidean index of len(LENGTHS) lists with well-separated centres, list l of LENGTHS[l] rows around centre
    l (list 0: one row, removed again; the last list: 300 copies of its centre), built by IVF.build on the host from
    centres set by hand: the probes come from the real coarse stage.  -> ivf, oracle copy, data, first row per list"""
    from oracle import oracle
    from tinyknn_amd import IVF, FastPQ
    oracle.build()
    rng = np.random.RandomState(500 + d)
    L = len(LENGTHS)
    cent = np.zeros((L, d), dtype=np.float32)
    if d >= L:                      # every pair of centres equally far apart: no estimate of the coarse stage saturates
        cent[np.arange(L), np.arange(L)] = 8.0
    else:
        cent[:, 0] = 8.0 * np.arange(L)
    sizes = [max(n, 1) for n in LENGTHS]
    member = np.repeat(np.arange(L), sizes)
    X = (cent[member] + 0.5 * rng.randn(len(member), d).astype(np.float32)).astype(np.float32)
    X[member == L - 1] = cent[L - 1]
    perm = rng.permutation(len(X))
    X, member = np.ascontiguousarray(X[perm]), member[perm]
    ivf = IVF("euclidean", L, FastPQ(2))
    ivf.all_centers = cent
    state = np.random.get_state()
    np.random.seed(77)
    try:
        ivf.pq.fit(X)
        ivf.build(X, n_probes=1, device=False)
    finally:
        np.random.set_state(state)
    for l in range(L):
        np.testing.assert_array_equal(np.sort(ivf.ids[l]), np.flatnonzero(member == l))
    ivf.remove(np.flatnonzero(member == 0))
    assert [len(ivf.ids[l]) for l in range(L)] == LENGTHS
    first = np.array([np.flatnonzero(member == l)[0] for l in range(L)])
    return ivf, oracle_index(oracle, ivf, ivf.data), ivf.data, cent, first


@pytest.mark.parametrize("d", [1, 20, 100, 127, 128])
def test_list_lengths_at_the_edges(oracle, d):
    ivf, ox, data, cent, first = _edges(d)
    L = len(LENGTHS)
    dev = ivf.device_index()
    rng = np.random.RandomState(d)
    # one query at every centre: P = 1 probes its own list, and with +inf one wrongly counted row changes lims
    qn, qpq = ivf._prepare(cent + 0.25 * rng.randn(L, d).astype(np.float32))
    probes = oracle_probes(ox, qn, 1)
    np.testing.assert_array_equal(probes[:, 0], np.arange(L))
    got, _ = _ask(dev, ox, oracle, qn, qpq, data, np.inf, 1, probes=probes, what="own list")
    np.testing.assert_array_equal(np.diff(got[0]), LENGTHS)
    probes = oracle_probes(ox, qn, 3)
    assert all(len(set(p)) == 3 and p[0] == l for l, p in enumerate(probes))
    got, _ = _ask(dev, ox, oracle, qn, qpq, data, np.inf, 3, probes=probes, what="three lists")
    np.testing.assert_array_equal(np.diff(got[0]), [sum(LENGTHS[l] for l in p) for p in probes])
    # 300 identical rows at radius 0: all of them, in id order
    qz, qzp = ivf._prepare(cent[L - 1:].copy())
    got, _ = _ask(dev, ox, oracle, qz, qzp, data, 0.0, 2, what="identical rows")
    assert got[0].tolist() == [0, 300] and (np.diff(got[1]) > 0).all() and (got[2] == 0).all()
    # batches of every size, radii inside the lists
    for nq in (0, 1, 4, 1000):
        at = rng.randint(L, size=nq)
        qn, qpq = ivf._prepare((cent[at] + 0.5 * rng.randn(nq, d).astype(np.float32)).astype(np.float32))
        probes = oracle_probes(ox, qn, 2)
        r = _kth(radius_probe_csr(oracle, ox, qn, data, np.inf, 2, probes=probes), 30)
        r[::5] = np.inf
        got, _ = _ask(dev, ox, oracle, qn, qpq, data, r, 2, probes=probes, what=f"nq={nq}")
        assert got[0].shape == (nq + 1,)


# ---- 3. probe rows that wrap -----------------------------------------------------------------------------------------
WRAP_SEEDS = list(range(1, 32, 2))       # the steered shapes of tests/restricted_shapes.py


def test_the_wrap_seeds_hold_rows_that_wrap():
    from restricted_shapes import case, twice
    wraps = minus = 0
    for seed in WRAP_SEEDS:
        c = case(seed)
        if c.skipped is None:
            probes = oracle_probes(c.ox, c.qn, c.shape["n_probes"])
            wraps += any(len(twice(p, c.ox.n_lists)) for p in probes)
            minus += bool((probes < 0).any())
    assert wraps >= 2 and minus >= 2, (wraps, minus)


@pytest.mark.parametrize("seed", WRAP_SEEDS)
def test_wrapped_probe_rows(oracle, seed):
    from restricted_shapes import case
    from tinyknn_amd.ivf import DeviceIndex
    c = case(seed)
    assert c.skipped is None, (c, c.skipped)
    dev = DeviceIndex(c.ivf)
    P = c.shape["n_probes"]
    probes = oracle_probes(c.ox, c.qn, P)
    everything = radius_probe_csr(oracle, c.ox, c.qn, c.ref_data, np.inf, P, probes=probes)
    same_csr(dev.radius_probe(c.qn, c.qp, np.inf, P), everything, repr(c))          # a walked list counts once
    _ask(dev, c.ox, oracle, c.qn, c.qp, c.ref_data, _kth(everything, 10), P, probes=probes, what=repr(c))
    dev.close()


# ---- 4. restrictions --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restricted_case():
    """the eu20 fixture with groups, tags and values by row, and a planted twin pair (TWIN_LO < TWIN_HI, identical
    rows) of which query 0 — a copy of them — sees the lower id fail under every restriction"""
    from oracle import oracle
    g = golden("g6_ivf_eu20.npz")
    data = g["data"].copy()
    ids = np.asarray(g["ids"])
    TWIN_LO, TWIN_HI = sorted(int(j) for j in ids[:2])              # two rows of list 0
    data[TWIN_HI] = data[TWIN_LO]
    ivf = fixture_ivf(g, data=data)
    ox = oracle_index(oracle, ivf, data)
    rng = np.random.RandomState(31)
    N = len(data)
    Q = np.ascontiguousarray(g["qs"], dtype=np.float32).copy()
    Q[0] = data[TWIN_LO]
    qn, qpq = ivf._prepare(Q.copy())
    qn, qpq = np.ascontiguousarray(qn), np.ascontiguousarray(qpq)
    groups = rng.randint(0, 4, size=N).astype(np.int32)
    groups[TWIN_LO], groups[TWIN_HI] = 1, 2
    row_tags = rng.randint(1, 256, size=N).astype(np.uint64)
    row_tags[TWIN_LO], row_tags[TWIN_HI] = 0b0001, 0b0110
    values = rng.randint(0, 100, size=N).astype(np.int64)
    values[TWIN_LO], values[TWIN_HI] = 5, 50
    dev = ivf.device_index()
    dev.set_groups(groups)
    dev.set_tags(row_tags)
    dev.set_values(values)
    return dict(ivf=ivf, dev=dev, ox=ox, data=data, qn=qn, qpq=qpq, groups=groups, row_tags=row_tags, values=values,
                lo=TWIN_LO, hi=TWIN_HI, N=N)


def _restricted(oracle, what, ref_kw, **kw):
    b = _restricted_case()
    nq, N = len(b["qn"]), b["N"]
    P = 5
    probes = oracle_probes(b["ox"], b["qn"], P)
    assert {b["lo"], b["hi"]} <= set(candidates(b["ox"], probes[0], N).tolist())
    oks = [passes(i, N, **ref_kw) for i in range(nq)]
    assert not oks[0][b["lo"]] and oks[0][b["hi"]]
    r = _kth(radius_probe_csr(oracle, b["ox"], b["qn"], b["data"], np.inf, P, probes=probes), 60)
    r[0] = 0.0
    got, want = _ask(b["dev"], b["ox"], oracle, b["qn"], b["qpq"], b["data"], r, P, probes=probes, oks=oks, what=what,
                     **kw)
    unrestricted = radius_probe_csr(oracle, b["ox"], b["qn"], b["data"], r, P, probes=probes)
    assert 0 < want[0][-1] < unrestricted[0][-1]
    assert got[1][got[0][0]:got[0][1]].tolist() == [b["hi"]]        # the failing twin is no hit, the other is


def test_allowed_alone(oracle):
    b = _restricted_case()
    mask = np.random.RandomState(32).rand(b["N"]) < 0.4
    mask[b["lo"]], mask[b["hi"]] = False, True
    _restricted(oracle, "mask", dict(allowed=mask), allowed=mask)
    _restricted(oracle, "ids", dict(allowed=mask), allowed=np.flatnonzero(mask))


def test_exclude_alone(oracle):
    b = _restricted_case()
    probes = oracle_probes(b["ox"], b["qn"], 5)
    exclude = np.array([candidates(b["ox"], p, b["N"])[0] for p in probes], dtype=np.int64)
    exclude[0] = b["lo"]
    exclude[3::4] = -1
    _restricted(oracle, "exclude", dict(exclude=exclude), exclude=exclude)


def test_group_alone(oracle):
    b = _restricted_case()
    group = np.random.RandomState(33).randint(-1, 4, size=len(b["qn"])).astype(np.int32)
    group[0], group[1] = 2, -1
    _restricted(oracle, "group", dict(group=group, groups=b["groups"]), group=group)


@pytest.mark.parametrize("mode", ["any", "all"])
def test_tags_alone(oracle, mode):
    b = _restricted_case()
    tags = np.random.RandomState(34).randint(0, 16, size=len(b["qn"])).astype(np.uint64)
    tags[0], tags[1] = 0b0110, 0
    _restricted(oracle, mode, dict(tags=tags, tags_mode=mode, row_tags=b["row_tags"]), tags=tags, tags_mode=mode)


def test_between_alone(oracle):
    b = _restricted_case()
    nq = len(b["qn"])
    rng = np.random.RandomState(35)
    lo = rng.randint(0, 50, size=nq).astype(np.int64)
    between = (lo, lo + 45)
    between[0][0], between[1][0] = 40, 60
    _restricted(oracle, "between", dict(between=between, values=b["values"]), between=between)


def test_all_five_together(oracle):
    b = _restricted_case()
    nq = len(b["qn"])
    rng = np.random.RandomState(36)
    mask = rng.rand(b["N"]) < 0.8
    mask[b["hi"]] = True
    exclude = np.full(nq, -1, dtype=np.int64)
    exclude[0] = b["lo"]
    group = np.full(nq, -1, dtype=np.int32)
    group[::2] = rng.randint(0, 4, size=len(group[::2]))
    group[0] = 2
    tags = np.full(nq, 0b11111111, dtype=np.uint64)
    tags[0] = 0b0110
    between = (np.zeros(nq, np.int64), np.full(nq, 80, np.int64))
    _restricted(oracle, "all five",
                dict(allowed=mask, exclude=exclude, group=group, groups=b["groups"], tags=tags, tags_mode="any",
                     row_tags=b["row_tags"], between=between, values=b["values"]),
                allowed=mask, exclude=exclude, group=group, tags=tags, tags_mode="any", between=between)


def test_row_values_that_do_not_cover_the_index_are_refused():
    from tinyknn_amd import _lib
    ivf, dev, ox, qn, qpq, data = _fixture("an20", None)
    for kw in (dict(group=1), dict(tags=1), dict(between=(0, 1))):
        with pytest.raises((_lib.TinyKnnHipError, ValueError)):
            dev.radius_probe(qn, qpq, 1.0, 2, **kw)
    same = dev.radius_probe(qn, qpq, 1.0, 2)
    assert same[0].shape == (len(qn) + 1,)


# ---- 5. invariants ----------------------------------------------------------------------------------------------------
def test_max_results_is_loud_and_the_index_stays_usable(oracle):
    ivf, dev, ox, qn, qpq, data = _fixture("an100", None)
    want = radius_probe_csr(oracle, ox, qn, data, np.inf, 5)
    total = int(want[0][-1])
    with pytest.raises(ValueError, match=f"{total} rows lie within the radii, more than max_results = {total - 1}"):
        dev.radius_probe(qn, qpq, np.inf, 5, max_results=total - 1)
    from tinyknn_amd import _lib
    with pytest.raises(_lib.TinyKnnHipError, match="no result is held"):
        _lib.check(_lib.lib().tk_index_radius_probe_fetch(dev._h, None, None))
    same_csr(dev.radius_probe(qn, qpq, np.inf, 5, max_results=total), want)
    same_csr(ivf.radius_search(golden("g6_ivf_an100.npz")["qs"], np.inf, n_probes=5, max_results=total), want)
    np.testing.assert_array_equal(ivf.radius_count(golden("g6_ivf_an100.npz")["qs"], np.inf, n_probes=5),
                                  np.diff(want[0]))


def test_a_call_cut_into_query_chunks_is_the_whole_call(oracle, monkeypatch):
    from tinyknn_amd.ivf import DeviceIndex
    ivf, dev, ox, qn, qpq, data = _fixture("eu128", None)
    want = radius_probe_csr(oracle, ox, qn, data, np.inf, 3)
    r = _kth(want, 25)
    want = radius_probe_csr(oracle, ox, qn, data, r, 3)
    exclude = want[1][want[0][:-1]].copy()                              # every query's nearest hit
    oks = [passes(i, len(data), exclude=exclude) for i in range(len(qn))]
    want_ex = radius_probe_csr(oracle, ox, qn, data, r, 3, oks=oks)
    monkeypatch.setattr(DeviceIndex, "RADIUS_PROBE_CHUNK", 5)
    same_csr(dev.radius_probe(qn, qpq, r, 3), want)
    same_csr(dev.radius_probe(qn, qpq, r, 3, exclude=exclude), want_ex)
    np.testing.assert_array_equal(dev.radius_probe_count(qn, qpq, r, 3, exclude=exclude), np.diff(want_ex[0]))
    with pytest.raises(ValueError, match=f"{int(want[0][-1])} rows"):
        dev.radius_probe(qn, qpq, r, 3, max_results=int(want[0][-1]) - 1)


def test_a_radius_call_of_either_kind_drops_the_others_result():
    from tinyknn_amd import _lib
    ivf, dev, ox, qn, qpq, data = _fixture("eu20", None)
    lib = _lib.lib()
    dev.radius_probe(qn, qpq, 1.0, 2)
    dev.radius_brute(qn, 1.0)
    with pytest.raises(_lib.TinyKnnHipError, match="no result is held"):
        _lib.check(lib.tk_index_radius_probe_fetch(dev._h, None, None))
    dev.radius_probe(qn, qpq, 1.0, 2)
    with pytest.raises(_lib.TinyKnnHipError, match="no result is held"):
        _lib.check(lib.tk_index_radius_fetch(dev._h, None, None))


# ---- 6. the lists change ----------------------------------------------------------------------------------------------
def test_after_remove_add_and_update(oracle):
    from tinyknn_amd import IVF, FastPQ
    rng = np.random.RandomState(41)
    n, d, L = 1200, 20, 8
    cent = rng.randn(L, d) * 3
    X = (cent[rng.randint(L, size=n)] + 0.5 * rng.randn(n, d)).astype(np.float32)
    Q = (cent[rng.randint(L, size=40)] + 0.5 * rng.randn(40, d)).astype(np.float32)
    ivf = IVF("euclidean", L, FastPQ(2))
    state = np.random.get_state()
    np.random.seed(4)
    try:
        ivf.fit(X).build(X, n_probes=2, device=False)
    finally:
        np.random.set_state(state)
    qn, qpq = ivf._prepare(Q.copy())
    dev = ivf.device_index()
    P = 3

    def check(what):
        ox = oracle_index(oracle, ivf, ivf.data)          # (the IVF's host copies of the lists follow every change)
        everything = radius_probe_csr(oracle, ox, qn, ivf.data, np.inf, P)
        got, _ = _ask(dev, ox, oracle, qn, qpq, ivf.data, _kth(everything, 40), P, what=what)
        same_csr(dev.radius_probe(qn, qpq, np.inf, P), everything, what)
        return got

    before = check("built")
    gone = np.unique(before[1])[::3]                                    # a third of the rows that were hits
    ivf.remove(gone)
    after = check("removed")
    assert not np.isin(after[1], gone).any()                            # no allowed= given: a removed row is no hit
    new = (cent[rng.randint(L, size=150)] + 0.5 * rng.randn(150, d)).astype(np.float32)
    ivf.add(new)
    grown = check("added")
    assert (grown[1] >= n).any()
    moved = np.setdiff1d(np.unique(grown[1]), gone)[:60]
    ivf.update(moved, (cent[rng.randint(L, size=len(moved))] + 0.5 * rng.randn(len(moved), d)).astype(np.float32))
    check("updated")


# ---- 7. cross-checks with the existing calls --------------------------------------------------------------------------
def test_on_integer_data_with_every_list_probed_the_ids_are_radius_brutes(oracle):
    import test_radius_probe_cpu as cpu
    for build_probes in (1, 2):
        ivf, ox, X, qn = cpu._int_case(build_probes)
        _, qpq = ivf._prepare(qn.copy())
        from tinyknn_amd.ivf import DeviceIndex
        dev = DeviceIndex(ivf)
        part = int_part(qn, X)
        r = np.partition(part, 40, axis=1)[:, 40].astype(np.float32)
        brute = dev.radius_brute(qn, r)
        for P in (ox.n_lists, ox.n_lists + 3):
            got = dev.radius_probe(qn, qpq, r, P)
            same_csr(got, brute, f"b={build_probes} P={P}")             # ids AND values: part == dist on integers
        dev.close()


def test_query_batchs_ids_within_the_radius_are_listed_with_the_same_distance_bits(oracle):
    for tag in ("an100", "eu20f64", "an100b2"):
        ivf, dev, ox, qn, qpq, data = _fixture(tag, None)
        for P in (2, 10):
            ids, dist = dev.query_batch(qn, qpq, 20, P, return_distances=True)
            r = dist[:, 9].astype(np.float32)
            r[~np.isfinite(r)] = 1.0
            lims, hits, hd = dev.radius_probe(qn, qpq, r, P)
            assert hd.dtype == dist.dtype
            seen = 0
            for i in range(len(qn)):
                mine = dict(zip(hits[lims[i]:lims[i + 1]].tolist(), hd[lims[i]:lims[i + 1]].tolist()))
                for j, dv in zip(ids[i], dist[i]):
                    if j >= 0 and dv <= dist.dtype.type(r[i]):
                        assert mine[int(j)] == dv, (tag, P, i, j)
                        seen += 1
            assert seen >= 5 * len(qn)


def test_without_n_probes_the_call_is_the_brute_calls_bytes():
    ivf, dev, ox, qn, qpq, data = _fixture("eu20", None)
    qs = golden("g6_ivf_eu20.npz")["qs"]
    r = float(np.median(dev.knn_brute_dist(qn, 8)[1][:, -1]))          # about 8 rows a query
    want = dev.radius_brute(qn, r)
    for got in (ivf.radius_search(qs, r), ivf.radius_search(qs, r, n_probes=None)):
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    np.testing.assert_array_equal(ivf.radius_count(qs, r, n_probes=None), np.diff(want[0]))
    assert want[0][-1] > 0
