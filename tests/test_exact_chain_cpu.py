"""tests/exact_chain_shapes.py without a GPU: the attribute arrays the references read are the library's own host copies
after every step; the thinned case is what it is for; the integer cases keep `part` exact; the default seeds reach the
states the exact and radius calls have to be seen on (counted from the model and the oracle alone); and the three
references tests/test_exact_chain_gpu.py trusts reproduce an obvious double loop on chain states, an empty index among
them."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exact_chain_shapes as ec  # noqa: E402
import list_chain_shapes as lc  # noqa: E402
from between_exact_reference import knn_between_reference  # noqa: E402
from brute_reference import int_part  # noqa: E402
from group_exact_reference import knn_group_reference  # noqa: E402
from radius_probe_reference import candidates, oracle_probes, passes, radius_probe_csr  # noqa: E402
from restricted_shapes import probed_lists  # noqa: E402
from store_reference import oracle_index  # noqa: E402
from test_radius_probe_gpu import _kth  # noqa: E402

SEEDS = list(lc.seeds())


def _cases():
    return [lc.case(s) for s in SEEDS] + [ec.thinned(kp) for kp in ec.THINNED] + [ec.int_case(s) for s in ec.INT_SEEDS]


@pytest.mark.parametrize("which", range(len(SEEDS) + len(ec.THINNED) + len(ec.INT_SEEDS)))
def test_the_attribute_arrays_are_the_librarys_host_copies(which):
    case = _cases()[which]
    if case.skipped:
        pytest.skip(case.skipped)
    ivf, attrs = ec.fresh(case)
    m = case.model()
    for i, op in enumerate(case.ops):
        assert ec.apply(ivf, op, ec.step_attrs(case, i), attrs) is ivf
        m.apply(op)
        msg = f"{case} step {i}"
        for name, dt in (("groups", np.int32), ("tags", np.uint64), ("values", np.int64)):
            have, want = getattr(ivf, name), getattr(attrs, name)
            assert have.dtype == dt and want.dtype == dt and have.shape == (m.N,), (name, msg)
            np.testing.assert_array_equal(have, want, err_msg=f"{name} {msg}")
        if case.shape["groups"]:
            np.testing.assert_array_equal(attrs.groups, m.groups, err_msg=msg)      # the chain's own groups
        assert len(ivf.data) == m.N
        np.testing.assert_array_equal(ivf.list_columns, m.cols, err_msg=msg)
    assert (attrs.tags == 0).any() and (attrs.tags < 256).all() and attrs.tags.any()
    assert attrs.values.min() >= 0 and attrs.values.max() < 100 and set(np.unique(attrs.groups)) <= set(range(5))


@pytest.mark.parametrize("kp", ec.THINNED)
def test_thinned(kp):
    """After step 0: 100 rows, each in kp lists, row N - 1 among them; the labels repeat; for kp = 2 the largest label
    lies beyond the 8 T + 1024 up to which the index makes its own twin table, and stays there through the chain.  For
    kp = 3 the bound is 8 * 300 + 1024 = 3424 > 3000: the index keeps a table of width 2 over its nearly empty lists."""
    case = ec.thinned(kp)
    m = case.model()
    assert ec.twin_table_of(m) == (kp * ec.THIN_N, ec.THIN_N, kp, True) and m.L == 16 and m.data.shape[1] == 8
    for i, op in enumerate(case.ops):
        m.apply(op)
        T, bound, copies, own = ec.twin_table_of(m)
        assert copies == kp and T == kp * len(m.stored_ids())       # the labels repeat: every row kp times
        if i == 0:
            assert len(m.stored_ids()) == ec.THIN_KEPT and ec.THIN_N - 1 in m.stored_ids() and bound == ec.THIN_N
        assert (bound > 8 * T + 1024) == (kp == 2) and own == (kp == 3), (i, T, bound)
    assert [o["kind"] for o in case.ops] == ["remove", "add", "update"]
    assert len(case.ops[1]["X"]) == 5 and len(case.ops[2]["ids"]) == 10 and m.N == ec.THIN_N + 5


@pytest.mark.parametrize("seed", ec.INT_SEEDS)
def test_integer_cases_keep_part_exact(seed):
    case = ec.int_case(seed)
    d, kp, L, n, nq = ec.INT_SHAPES[seed]
    assert case.ivf.metric == "euclidean" and case.ivf.data.dtype == np.float32 and case.ivf.store is None
    m = case.model()
    assert (m.kp, m.L, m.N, m.data.shape[1], len(case.qn)) == (kp, L, n, d, nq)
    for i, op in enumerate(case.ops):
        m.apply(op)
        assert np.array_equal(m.data, np.rint(m.data)) and np.abs(m.data).max() <= 50
        assert np.abs(int_part(case.qn, m.data)).max() < 2 ** 24, i
    assert len(case.ops) >= 6
    assert {ec.INT_SHAPES[s][0] for s in ec.INT_SEEDS} == {3, 33, 128}
    assert {ec.INT_SHAPES[s][1] for s in ec.INT_SEEDS} == {1, 2}


# ---- what the default seeds cover ------------------------------------------------------------------------------------

def fuzz_radii(everything):
    """the radii tests/test_exact_chain_gpu.py asks: the reference's 10th distance rounded up, +inf for every fifth"""
    r = _kth(everything, 10)
    r[::5] = np.inf
    return r


def test_default_seeds_cover_what_the_exact_calls_need(oracle):
    """(i) .. (vi) of the module's purpose, counted over the default seeds.  Needs the default seeds: a run with
    TINYKNN_FUZZ_SEEDS below 24 checks what it can."""
    added = removed = twice = empty = moved = 0
    both = {}
    for seed in SEEDS:
        case = lc.case(seed)
        if case.skipped:
            continue
        c, qn = case.shape, case.qn
        deep = ec.deep_steps(len(case.ops))
        for i, op, m, attrs, groups_before in ec.replay(case):
            data = np.asarray(m.stored())
            ox = oracle_index(oracle, ec.ref_ivf(case, m), data)
            stored = ec.stored_mask(m)
            if not stored.any():
                empty += 1
            where = [set() for _ in range(m.N)]
            for l in range(m.L):
                for j in m.ids[l]:
                    where[j].add(l)
            hit_added = hit_removed = hit_twice = False
            for P in sorted({1, c["n_probes"]}):
                probes = oracle_probes(ox, qn, P)
                everything = radius_probe_csr(oracle, ox, qn, data, np.inf, P, probes=probes)
                r = fuzz_radii(everything)
                lims, ids, _ = radius_probe_csr(oracle, ox, qn, data, r, P, probes=probes)
                hit_added |= bool((ids >= case.N0).any())
                gone = np.flatnonzero(~stored)
                for q in range(len(qn)):
                    if np.isfinite(r[q]) and len(gone):
                        dist = oracle.sqdist_gather(qn[q], data, gone).astype(data.dtype)
                        hit_removed |= bool((dist <= data.dtype.type(r[q])).any())
                    if m.kp >= 2:
                        lists = set(probed_lists(probes[q], ox.n_lists).tolist())
                        hit_twice |= any(len(where[j] & lists) >= 2 for j in ids[lims[q]:lims[q + 1]])
            added += hit_added
            removed += hit_removed
            twice += hit_twice
            if i not in deep:
                continue
            rs = ec.restrictions(case, i, m, attrs, len(qn))
            if op["kind"] == "update":
                asked = set(ec.knn_groups(rs).tolist())
                was, now = groups_before[op["ids"]], attrs.groups[op["ids"]]
                moved += bool(((was != now) & (np.isin(was, list(asked)) | np.isin(now, list(asked)))).any())
            probes = oracle_probes(ox, qn, c["n_probes"])
            for name, (_, ref_kw) in rs.items():
                for q in range(len(qn)):
                    cand = candidates(ox, probes[q], m.N)
                    ok = passes(q, m.N, **ref_kw)[cand]
                    if ok.any() and not ok.all():
                        both[name] = both.get(name, 0) + 1
                        break
    counts = dict(added=added, removed=removed, twice=twice, empty=empty, moved=moved, both=both)
    print(counts)
    if len(SEEDS) < lc.DEFAULT_SEEDS:
        return
    assert added >= 3 and removed >= 3 and twice >= 2 and empty >= 2 and moved >= 3, counts
    assert set(both) == set(ec.restrictions(lc.case(0), 0, lc.case(0).model(), ec.initial_attrs(lc.case(0)), 1)), counts
    assert min(both.values()) >= 3, counts


# ---- the references against an obvious double loop -------------------------------------------------------------------

def _state(case, step):
    for i, op, m, attrs, _ in ec.replay(case):
        if i == step:
            return m, attrs
    raise AssertionError(step)


def _int_dist(a, b):
    return sum((int(x) - int(y)) ** 2 for x, y in zip(a, b))


def _obvious_knn(qn, data, k, ok_of):
    """per query the k smallest (distance, row) over the rows ok_of(i, j) lets pass, in Python integers"""
    ids = np.full((len(qn), k), -1, dtype=np.int64)
    dist = np.full((len(qn), k), np.inf, dtype=np.float32)
    for i in range(len(qn)):
        best = sorted((_int_dist(data[j], qn[i]), j) for j in range(len(data)) if ok_of(i, j))[:k]
        for t, (dv, j) in enumerate(best):
            ids[i, t], dist[i, t] = j, dv
    return ids, dist


STATES = [("int", 1, None), ("int", 0, None), ("chain", 1, "empty")]


@pytest.mark.parametrize("kind,seed,want", STATES)
def test_the_references_reproduce_a_double_loop_on_chain_states(oracle, kind, seed, want):
    case = ec.int_case(seed) if kind == "int" else lc.case(seed)
    mixed = [i for i, _, m, _, _ in ec.replay(case) if 0 < len(m.stored_ids()) < m.N]
    step = len(case.ops) - 1 if want == "empty" else mixed[-1]      # (the last state with stored and removed rows)
    m, attrs = _state(case, step)
    data = np.asarray(m.stored())
    stored = ec.stored_mask(m)
    qn, nq, N, k = case.qn, len(case.qn), m.N, 7
    if want == "empty":
        assert not stored.any() and m.sizes.sum() == 0        # (no row is a candidate: no distance is ever formed)
    else:
        assert stored.any() and not stored.all()
    ox = oracle_index(oracle, ec.ref_ivf(case, m), data)
    rs = ec.restrictions(case, step, m, attrs, nq)
    group = ec.knn_groups(rs)
    lo, hi = rs["between"][0]["between"]
    tags = rs["tags any"][0]["tags"]
    mask = rs["allowed"][0]["allowed"]
    # radius over the probed lists: list by list, row by row
    P = 2
    probes = oracle_probes(ox, qn, P)
    radius = np.array([np.inf, 900.0, 2500.0] * nq, dtype=np.float32)[:nq]
    oks = [passes(i, N, allowed=mask) for i in range(nq)]
    lims, ids, dist = radius_probe_csr(oracle, ox, qn, data, radius, P, oks=oks, probes=probes)
    at = 0
    for i in range(nq):
        seen, hits = set(), []
        for p in probes[i]:
            l = int(p) if p >= 0 else m.L - 1
            for j in m.ids[l].tolist():
                if j in seen or not mask[j]:
                    continue
                seen.add(j)
                dv = _int_dist(data[j], qn[i]) if want != "empty" else 0
                if dv <= radius[i]:
                    hits.append((dv, j))
        hits.sort()
        assert lims[i] == at and ids[at:at + len(hits)].tolist() == [j for _, j in hits], i
        assert dist[at:at + len(hits)].tolist() == [float(dv) for dv, _ in hits], i
        at += len(hits)
    assert lims[-1] == at and (at == 0) == (want == "empty")
    # knn_group and knn_between: every row asked
    gi, gd = knn_group_reference(oracle, qn, data, k, group, attrs.groups, stored=stored, allowed=mask, tags=tags,
                                 tags_mode="any", row_tags=attrs.tags)
    wi, wd = _obvious_knn(qn, data, k, lambda i, j: stored[j] and mask[j] and attrs.groups[j] == group[i]
                          and (tags[i] == 0 or int(attrs.tags[j]) & int(tags[i]) != 0))
    np.testing.assert_array_equal(gi, wi)
    np.testing.assert_array_equal(gd, wd)
    bi, bd = knn_between_reference(oracle, qn, data, k, (lo, hi), attrs.values, stored=stored, group=rs["group"][0]["group"],
                                   groups=attrs.groups)
    g = rs["group"][0]["group"]
    wi, wd = _obvious_knn(qn, data, k, lambda i, j: stored[j] and lo[i] <= attrs.values[j] <= hi[i]
                          and (g[i] < 0 or attrs.groups[j] == g[i]))
    np.testing.assert_array_equal(bi, wi)
    np.testing.assert_array_equal(bd, wd)
    assert ((gi >= 0).any() and (bi >= 0).any()) == (want != "empty")
