"""The radius and exact calls through chains of IVF.add / remove / update on the awkward indexes of
tests/list_chain_shapes.py (tests/exact_chain_shapes.py carries a group, a tag mask and a value per row through every
step; tests/test_exact_chain_cpu.py shows what the default seeds cover and holds the references against double loops).
tests/test_list_chain_gpu.py compares the lists themselves after every step; here the calls that READ them and the
by-row tables are asked, each against its reference, bytes for bytes.

Leg A, every default seed, a host-built index with a device copy.  After EVERY step radius_probe, its unsorted form and
its count for P = 1 and the seed's n_probes, at the reference's 10th distance rounded up to float32 (a radius that sits
on a hit's own distance), +inf for every fifth query, and once at a scalar +inf; an empty index answers all-zero lims.
At the two deep steps the same under each restriction alone and all five together; query_batch under tags=, between=
and per_group= with distances; knn_group and knn_between bare and under the other restrictions; group_sizes and
range_sizes against counts over the attribute arrays; and the documented refusal of the `part` calls where the seed's
store or width is outside them.
Leg B, thinned(2) and thinned(3): after IVF.remove has left 100 rows under the label 2999 the index keeps no twin table
(kp = 2) and radius_search(n_probes=) makes its own; the answers stay the reference's.
Leg C, integer coordinates: radius_brute, radius_count and knn_brute_dist against numpy's exact `part`, and radius_probe
with every list probed against radius_brute, byte for byte."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exact_chain_shapes as ec  # noqa: E402
import list_chain_shapes as lc  # noqa: E402
from between_exact_reference import knn_between_reference  # noqa: E402
from between_reference import ranged_batch  # noqa: E402
from brute_reference import int_part  # noqa: E402
from brute_restricted_reference import restricted_dist, restricted_k_best  # noqa: E402
from group_exact_reference import knn_group_reference, same_bits  # noqa: E402
from per_group_reference import capped_batch  # noqa: E402
from radius_probe_reference import oracle_probes, passes, radius_probe_csr, same_csr  # noqa: E402
from radius_reference import radius_csr  # noqa: E402
from store_reference import oracle_index  # noqa: E402
from tags_reference import tagged_batch  # noqa: E402
from test_list_chain_gpu import LIMIT, time_limit  # noqa: E402
from test_radius_probe_gpu import _ask, _kth  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = list(lc.seeds())


def _distances(oracle, qn, data, ids):
    """the rescoring's distances of the ids in the store's type, +inf beside -1"""
    dt = np.float64 if data.dtype == np.float64 else np.float32
    out = np.full(ids.shape, np.inf, dtype=dt)
    for i in range(len(ids)):
        live = ids[i] >= 0
        out[i][live] = oracle.sqdist_gather(qn[i], data, ids[i][live]).astype(dt)
    return out


def _probe_check(oracle, dev, ox, qn, qp, data, P, msg, restricted=None):
    """radius_probe / sort=False / radius_probe_count for P against the reference: the fuzz's radii and a scalar +inf,
    and (restricted: ec.restrictions' dict, or its items to ask) the same radii under each restriction"""
    probes = oracle_probes(ox, qn, P)
    everything = radius_probe_csr(oracle, ox, qn, data, np.inf, P, probes=probes)
    r = _kth(everything, 10)
    r[::5] = np.inf
    got, want = _ask(dev, ox, oracle, qn, qp, data, r, P, probes=probes, what=f"P={P} {msg}")
    same_csr(dev.radius_probe(qn, qp, np.inf, P), everything, f"P={P} +inf {msg}")
    for name, (kw, ref_kw) in (restricted or {}).items():
        oks = [passes(i, len(data), **ref_kw) for i in range(len(qn))]
        _ask(dev, ox, oracle, qn, qp, data, r, P, probes=probes, oks=oks, what=f"P={P} {name} {msg}", **kw)
    return got, want


def _same_knn(got, want, msg):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"ids {msg}")
    assert same_bits(got[1], want[1]), f"distances {msg}"


def _deep_check(oracle, c, dev, ox, qn, qp, data, m, attrs, rs, msg):
    """the restricted batches and the exact calls of a deep step"""
    k, p, nq, N = c["k"], c["n_probes"], len(qn), m.N
    stored = ec.stored_mask(m)
    # query_batch under tags=, between=, per_group=: ids and the rescoring's distances
    for mode in ("any", "all"):
        tags = rs[f"tags {mode}"][0]["tags"]
        want = tagged_batch(oracle, ox, qn, tags, mode, attrs.tags, k, p)
        _same_knn(dev.query_batch(qn, qp, k, p, tags=tags, tags_mode=mode, return_distances=True),
                  (want, _distances(oracle, qn, data, want)), f"tags= {mode} {msg}")
    between = rs["between"][0]["between"]
    want = ranged_batch(oracle, ox, qn, between, attrs.values, k, p)
    _same_knn(dev.query_batch(qn, qp, k, p, between=between, return_distances=True),
              (want, _distances(oracle, qn, data, want)), f"between= {msg}")
    for cap in (1, 3):
        want = capped_batch(oracle, ox, qn, cap, attrs.groups, k, p)
        _same_knn(dev.query_batch(qn, qp, k, p, per_group=cap, return_distances=True), want, f"per_group={cap} {msg}")
    # knn_group: bare, and under the other restrictions.  Both exact calls take 1 <= k <= min(1024, N): a seed whose k
    # is larger than its index is refused in those words, and asked with k = N
    all_kw, all_ref = rs["all five"]
    group = ec.knn_groups(rs)
    if k > N:
        for call in (lambda: dev.knn_group(qn, k, group), lambda: dev.knn_between(qn, k, rs["between"][0]["between"])):
            with pytest.raises(AssertionError, match=r"1 <= k <= min\(1024, N\)"):
                call()
        k = N
    _same_knn(dev.knn_group(qn, k, group, return_distances=True),
              knn_group_reference(oracle, qn, data, k, group, attrs.groups, stored=stored), f"knn_group {msg}")
    others = {a: b for a, b in all_kw.items() if a != "group"}
    others_ref = {a: b for a, b in all_ref.items() if a not in ("group", "groups")}
    _same_knn(dev.knn_group(qn, k, group, return_distances=True, **others),
              knn_group_reference(oracle, qn, data, k, group, attrs.groups, stored=stored, **others_ref),
              f"knn_group, restricted {msg}")
    asked = np.arange(-1, ec.N_GROUPS + 2)
    np.testing.assert_array_equal(dev.group_sizes(asked), [(attrs.groups == g).sum() for g in asked], err_msg=msg)
    # knn_between: bare, and under the other restrictions
    lo, hi = between
    _same_knn(dev.knn_between(qn, k, between, return_distances=True),
              knn_between_reference(oracle, qn, data, k, between, attrs.values, stored=stored), f"knn_between {msg}")
    others = {a: b for a, b in all_kw.items() if a != "between"}
    others_ref = {a: b for a, b in all_ref.items() if a not in ("between", "values")}
    _same_knn(dev.knn_between(qn, k, between, return_distances=True, **others),
              knn_between_reference(oracle, qn, data, k, between, attrs.values, stored=stored, **others_ref),
              f"knn_between, restricted {msg}")
    length, col = dev.range_sizes(between)
    np.testing.assert_array_equal(length, [((attrs.values >= a) & (attrs.values <= b)).sum() for a, b in zip(lo, hi)],
                                  err_msg=msg)
    assert (col == 0).all(), msg
    assert dev.groups_set() == dev.tags_set() == dev.values_set() == N, msg


def _refused_part_calls(c, dev, qn):
    """knn_brute and radius_brute take float32 vectors of at most 128 dimensions: outside, the documented refusal"""
    if c["store"] == "float32" and c["d"] <= 128:
        return
    match = {"float16": "half", "float64": "float32 vectors only"}.get(c["store"], "d <= 128")
    for call in (lambda: dev.radius_brute(qn, 1.0), lambda: dev.radius_count(qn, 1.0), lambda: dev.knn_brute(qn, 1)):
        with pytest.raises(AssertionError, match=match):
            call()


def _chain(oracle, case, restricted_every_step=()):
    """Leg A's checks over one case.  restricted_every_step: names of ec.restrictions asked after every step too."""
    ivf, attrs = ec.fresh(case)
    m = case.model()
    c, qn, qp = case.shape, case.qn, case.qp
    dev = ivf.device_index()
    widths = []
    try:
        deep = ec.deep_steps(len(case.ops))
        for i, op in enumerate(case.ops):
            msg = f"{case} after step {i} of {[(o['kind'], o['sel']) for o in case.ops]}"
            assert ec.apply(ivf, op, ec.step_attrs(case, i), attrs) is ivf
            assert ivf.device_index() is dev, msg
            m.apply(op)
            assert dev.N == m.N and dev.n_lists == m.L, msg
            data = np.asarray(m.stored())
            ox = oracle_index(oracle, ec.ref_ivf(case, m), data)
            rs = ec.restrictions(case, i, m, attrs, len(qn))
            ask = rs if i in deep else {name: rs[name] for name in restricted_every_step}
            for P in sorted({1, c["n_probes"]}):
                got, want = _probe_check(oracle, dev, ox, qn, qp, data, P, msg, ask)
                assert got[2].dtype == (np.float64 if c["store"] == "float64" else np.float32), msg
                if m.sizes.sum() == 0:
                    assert not got[0].any() and len(got[1]) == 0, msg
            widths.append(dev.twin_table_width())
            if i in deep:
                _deep_check(oracle, c, dev, ox, qn, qp, data, m, attrs, rs, msg)
        _refused_part_calls(c, dev, qn)
    finally:
        dev.close()
    return widths


# ---- leg A ----

@pytest.mark.parametrize("seed", SEEDS)
def test_radius_and_exact_calls_through_a_chain(oracle, seed):
    case = lc.case(seed)
    if case.skipped:
        pytest.skip(case.skipped)
    with time_limit(LIMIT, f"seed {seed}"):
        _chain(oracle, case)


# ---- leg B ----

@pytest.mark.parametrize("kp", ec.THINNED)
def test_radius_search_answers_on_an_index_thinned_by_remove(oracle, kp):
    """IVF.build(n_probes=kp), all but 100 of 3000 rows removed: for kp = 2 the index keeps no twin table of its own
    (twin_table_width() == 0, query_batch replays through its hash set) and radius_search(n_probes=) lists every row
    once all the same."""
    case = ec.thinned(kp)
    with time_limit(LIMIT, f"thinned({kp})"):
        widths = _chain(oracle, case, restricted_every_step=("all five",))
    assert widths == ([0, 0, 0] if kp == 2 else [2, 2, 2])


def test_radius_search_still_refuses_what_no_twin_table_can_describe(oracle):
    """What stays refused: a label stored more than 17 times, and copies of a label that carry different codes."""
    import label_shapes as ls
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    c = ls.case_c(oracle, 18)
    dev = DeviceIndex(c["ivf"])
    try:
        assert dev.twin_table_width() == 0
        with pytest.raises(_lib.TinyKnnHipError, match="more than 17 times"):
            dev.radius_probe(c["qn"][:4], c["qp"][:4], 1.0, 3)
        assert dev.query_batch(c["qn"][:4], c["qp"][:4], 3, 3).shape == (4, 3)         # the index lives on
    finally:
        dev.close()
    # one copy of a thinned index's row recoded: the copies disagree
    case = ec.thinned(2)
    m = case.model()
    m.apply(case.ops[0])
    l = int(np.argmax(m.sizes))
    m.labels[l][0] ^= 1
    dev = DeviceIndex(ec.ref_ivf(case, m))
    try:
        assert dev.twin_table_width() == 0
        with pytest.raises(_lib.TinyKnnHipError, match="different codes"):
            dev.radius_probe(case.qn, case.qp, 1.0, 3)
        assert dev.query_batch(case.qn, case.qp, 3, 3).shape == (len(case.qn), 3)
    finally:
        dev.close()


# ---- leg C ----

def _same_part(got, want, msg):
    for g, w, name in zip(got, want, ("lims", "ids", "part")):
        assert g.dtype == w.dtype and g.tobytes() == np.ascontiguousarray(w).tobytes(), f"{name} {msg}"


def _brute_check(dev, qn, part, oks, k, msg, **kw):
    """radius_brute, radius_count and knn_brute_dist under the masks `oks` against numpy's exact part"""
    nq = len(qn)
    r = np.array([np.partition(part[i][oks[i]], 20)[20] if oks[i].sum() > 20 else 4000.0 for i in range(nq)],
                 dtype=np.float32)
    r[::5] = np.inf
    want = radius_csr(part, oks, r)
    _same_part(dev.radius_brute(qn, r, **kw), want, f"radius_brute {msg}")
    np.testing.assert_array_equal(dev.radius_count(qn, r, **kw), np.diff(want[0]), err_msg=f"radius_count {msg}")
    ids, dist = dev.knn_brute_dist(qn, k, **kw)
    want_ids = np.stack([restricted_k_best(part[i], oks[i], k) for i in range(nq)])
    np.testing.assert_array_equal(ids, want_ids, err_msg=f"knn_brute_dist {msg}")
    want_dist = np.stack([restricted_dist(part[i], want_ids[i]) for i in range(nq)])
    assert dist.dtype == np.float32 and dist.tobytes() == want_dist.tobytes(), f"knn_brute_dist's part {msg}"
    return r


@pytest.mark.parametrize("seed", ec.INT_SEEDS)
def test_part_based_calls_through_an_integer_chain(oracle, seed):
    case = ec.int_case(seed)
    ivf, attrs = ec.fresh(case)
    m = case.model()
    c, qn, qp = case.shape, case.qn, case.qp
    dev = ivf.device_index()
    deep = ec.deep_steps(len(case.ops))
    try:
        with time_limit(LIMIT, f"integer seed {seed}"):
            for i, op in enumerate(case.ops):
                msg = f"{case} after step {i} of {[(o['kind'], o['sel']) for o in case.ops]}"
                ec.apply(ivf, op, ec.step_attrs(case, i), attrs)
                m.apply(op)
                X = np.asarray(ivf.data)
                np.testing.assert_array_equal(X, m.data, err_msg=msg)
                part = int_part(qn, X)
                assert np.abs(part).max() < 2 ** 24, msg
                alive = ec.stored_mask(m)
                nq = len(qn)
                r = _brute_check(dev, qn, part, [alive] * nq, c["k"], msg, allowed=alive)
                # every list probed: the probed search is the brute search over the stored rows, bytes and all
                brute = dev.radius_brute(qn, r, allowed=alive)
                for P in (m.L, m.L + 3):
                    same_csr(dev.radius_probe(qn, qp, r, P), brute, f"radius_probe P={P} {msg}")
                if i not in deep:
                    continue
                rs = ec.restrictions(case, i, m, attrs, nq)
                for name in ("group", "tags any", "tags all", "between", "exclude"):
                    kw, ref_kw = rs[name]
                    oks = [passes(q, m.N, allowed=alive, **ref_kw) for q in range(nq)]
                    _brute_check(dev, qn, part, oks, c["k"], f"{name} {msg}", allowed=alive, **kw)
    finally:
        dev.close()
