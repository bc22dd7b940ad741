"""The cases of tests/restricted_shapes.py are what they claim, on the CPU reference alone: the default seeds hold every
category tests/test_restricted_fuzz_gpu.py is there to reach (so a change to the generator cannot silently empty one),
and on every case — short lists, empty lists, wrapped probe lists — guarding `insert` gives the heaps that substituting
the empty value gives, which is the form the device passes rely on (tests/test_allowed_cpu.py shows it on streams and
the fixtures)."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import restricted_shapes as rs  # noqa: E402
from allowed_reference import replay_blocks  # noqa: E402

SEEDS = list(rs.seeds())


def _mask(case, i):
    """the rows query i may return as grouped_batch composes them, None for an unrestricted query"""
    N = len(case.ref_data)
    g = -1 if case.group is None else int(case.group[i])
    e = -1 if case.exclude is None else int(case.exclude[i])
    if g == -1 and case.allowed is None and not 0 <= e < N:
        return None
    mask = np.ones(N, dtype=bool) if g == -1 else case.groups == g
    if case.allowed is not None:
        mask = mask & case.allowed
    if 0 <= e < N:
        mask = mask & (np.arange(N) != e)
    return mask


def _substituted_heap(oracle, case, i):
    """query i's heap with every row outside its mask given the empty value and no guard on `insert`"""
    ox, c = case.ox, case.shape
    _, dbg = ox.query(case.qn[i], c["k"], c["n_probes"], debug=True)
    R = (c["n_probes"] + 1) * c["k"] + 1
    tables = oracle.transform_tables(dbg["table"])
    hidx = np.full(R, -1, dtype=np.int64)
    hval = np.full(R, 127, dtype=np.int32)
    mask = _mask(case, i)
    for p in dbg["probes"]:
        cl = int(p) + ox.n_lists if p < 0 else int(p)
        c0, c1 = int(ox.list_chunk_off[cl]), int(ox.list_chunk_off[cl + 1])
        if c1 == c0:
            continue
        n = int(ox.list_n[cl])
        labels = ox.ids[ox.ids_off[cl]:ox.ids_off[cl] + n]
        out = np.zeros(2 * (c1 - c0), dtype=np.uint64)
        oracle.estimate_pq(np.ascontiguousarray(ox.codes[c0:c1]), tables, out, True, ox._s.order)
        replay_blocks(oracle, out.view(np.uint8).reshape(-1, 16), n, labels, hidx, hval, True, mask, substitute=True)
    return hidx, hval


@pytest.mark.parametrize("seed", SEEDS)
def test_guard_and_substitute_forms_agree(oracle, seed):
    case = rs.case(seed)
    assert case.skipped is None, (case, case.skipped)
    want, wd = case.want()          # the guard form: grouped_batch
    for i in range(len(case.qn)):
        hidx, hval = _substituted_heap(oracle, case, i)
        np.testing.assert_array_equal(hidx, wd["heap_idx"][i], err_msg=f"{case} query {i}")
        np.testing.assert_array_equal(hval, wd["heap_val"][i], err_msg=f"{case} query {i}")
    # what the restriction promises of the ids
    for i, row in enumerate(want):
        ids = row[row != -1]
        mask = _mask(case, i)
        assert mask is None or mask[ids].all(), (case, i)
        assert len(np.unique(ids)) == len(ids)


@pytest.mark.parametrize("seed", SEEDS[::4])
def test_unrestricted_reference_is_the_oracle(oracle, seed):
    """case.base comes from OracleIndex.query; grouped_batch with no restriction gives the same arrays"""
    case = rs.case(seed)
    got, gd = case.reference(allowed=None, exclude=None, group=None)
    np.testing.assert_array_equal(got, case.base)
    for key in ("probes", "heap_idx", "heap_val"):
        np.testing.assert_array_equal(gd[key], case.base_dbg[key], err_msg=key)
    np.testing.assert_array_equal(got, case.ox.query_batch(case.qn, case.shape["k"], case.shape["n_probes"]))


NOTICED = {}        # pair seed -> (rows of the partner's answer that change with exclude_b one row low, with group_b)


def _one_row_low(a):
    return np.concatenate([a[:1], a[:-1]])


def _partner(seed):
    """The partner call of the pipelined pairs (Case.second) can join the case's call, and what its answer owes to its
    own arrays: the rows that change when the array is read one row low — what a pass that took the second call's rows
    from the wrong origin would do."""
    case = rs.case(seed)
    qn, qp, ex, gr, ids = case.second()
    assert qn.shape == case.qn.shape and qp.shape == case.qp.shape and ex.shape == (len(qn),)
    assert (gr is None) == (case.group is None)
    by_ex = (case.reference(qn=qn, exclude=_one_row_low(ex), group=gr)[0] != ids).any(axis=1).sum()
    by_gr = 0 if gr is None else (case.reference(qn=qn, exclude=ex, group=_one_row_low(gr))[0] != ids).any(axis=1).sum()
    NOTICED[seed] = (int(by_ex), int(by_gr))


@pytest.mark.parametrize("seed", rs.pair_seeds(SEEDS))
def test_pair_partner(oracle, seed):
    _partner(seed)


def test_pair_partners_depend_on_their_own_arrays(oracle):
    """Over the default seeds: all seven subsets take part, and enough partners answer differently when exclude_b or
    group_b is read from the wrong row — some of them without groups, so that the exclude array alone decides."""
    default = rs.pair_seeds(range(rs.DEFAULT_SEEDS))
    for seed in default:
        if seed not in NOTICED:
            _partner(seed)
    assert {rs.shape(s)["subset"] for s in default} == {"a", "e", "g", "ae", "ag", "eg", "aeg"}
    by_ex = [s for s in default if NOTICED[s][0] > 0]
    by_gr = [s for s in default if NOTICED[s][1] > 0]
    print("exclude_b decides in", by_ex, "group_b in", by_gr)
    assert len(by_ex) >= 4 and len(by_gr) >= 3, NOTICED
    assert sum("g" not in rs.shape(s)["subset"] for s in by_ex) >= 2, by_ex
    assert sum(NOTICED[s][0] >= 16 for s in default) >= 2, NOTICED     # (not a single row only)


def test_cases_follow_from_the_seed():
    a, b = rs._build(5), rs.case(5)
    assert a.shape == b.shape
    np.testing.assert_array_equal(a.qn, b.qn)
    np.testing.assert_array_equal(a.base, b.base)
    np.testing.assert_array_equal(a.exclude, b.exclude)
    np.testing.assert_array_equal(a.groups, b.groups)
    np.testing.assert_array_equal(a.group, b.group)
    for x, y in zip(a.ivf.ids, b.ivf.ids):
        np.testing.assert_array_equal(x, y)


def test_default_seeds_cover_every_category():
    """Counted over the default seeds whatever TINYKNN_FUZZ_SEEDS says."""
    count = collections.Counter()
    subsets = collections.Counter()
    kinds = collections.Counter()
    for seed in range(rs.DEFAULT_SEEDS):
        case = rs.case(seed)
        assert case.skipped is None, (case, case.skipped)
        c = case.shape
        assert 3 <= c["d"] <= 130 and 1 <= c["n_clusters"] <= 40 and 17 <= len(case.ref_data) <= 3040
        assert 1 <= c["k"] <= 50 and 1 <= c["n_probes"] <= max(5, c["n_clusters"] + 3) and 1 <= len(case.qn) <= 200
        subsets[c["subset"]] += 1
        assert (case.allowed is not None, case.exclude is not None, case.group is not None) == \
            ("a" in c["subset"], "e" in c["subset"], "g" in c["subset"])
        f = rs.facts(case)
        for name, v in f.items():
            if name != "build_probes" and v:
                count[name] += 1
        if f["excluded_in_twice"] and f["build_probes"] >= 2:
            count["excluded_in_twice_built_with_2"] += 1
        kinds[c["change"]] += 1
        kinds[c["store"]] += 1
        kinds["rotated" if case.ivf.pq.R is not None else "unrotated"] += 1
        kinds[c["metric"]] += 1
        for name in ("allowed_kind", "group_kind"):
            if hasattr(case, name):
                kinds[name + ":" + getattr(case, name)] += 1
        for name in set(getattr(case, "exclude_kinds", ())):
            kinds["exclude:" + name] += 1
    print(dict(count), dict(subsets), dict(kinds))
    assert sorted(subsets) == ["a", "ae", "aeg", "ag", "e", "eg", "g"] and min(subsets.values()) >= 3, subsets
    assert count["excluded_in_twice"] >= 4, count
    assert count["excluded_in_twice_built_with_2"] >= 2, count
    assert count["probes_short"] >= 4, count
    assert count["probes_empty"] >= 2, count
    assert count["more_probes_than_lists"] >= 4, count
    assert count["single"] >= 4, count
    assert count["fewer_than_k"] >= 6, count
    assert count["none"] >= 3, count
    assert count["differs_same_length"] >= 6, count
    # every kind of change, store, rotation, metric and restriction is drawn by some default seed
    for name in ("none", "remove", "add", "float32", "float16", "rotated", "unrotated", "euclidean", "angular"):
        assert kinds[name] >= 2, (name, kinds)
    for name in (["allowed_kind:" + x for x in rs.ALLOWED_KINDS] + ["group_kind:" + x for x in rs.GROUP_KINDS]
                 + ["exclude:" + x for x in rs.EXCLUDE_KINDS]):
        assert kinds[name] >= 1, (name, kinds)
