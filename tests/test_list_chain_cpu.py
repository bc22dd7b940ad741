"""The chains of tests/list_chain_shapes.py on the host alone.  ListsModel, which judges the device in
tests/test_list_chain_gpu.py, is first held against an independent implementation: the numpy path of IVF.add / remove /
update (IVF._splice, IVF._filter_lists), step by step and exactly — which also runs that path on one-list indexes, lists
of 0, 1 and 15-17 rows, empty column blocks and chains, where nothing else does.  Then the default seeds are shown to
reach what they are here for, so that a change to the generator cannot silently empty a category, and the model is
checked against itself (update = remove + add relabelled).

Centre activation (a new row whose nearest centre lies past the active prefix) IS reachable from these builds: an index
built over the fitted rows that keep away from the last centre has one list fewer, and the host build accepts it.  Seeds
5 (mod 12) are steered so; the floor is asserted below."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import list_chain_shapes as lc  # noqa: E402
from update_reference import relabelled  # noqa: E402

SEEDS = list(lc.seeds())


@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_the_host_path(seed):
    case = lc.case(seed)
    if case.skipped:
        pytest.skip(case.skipped)
    ivf, m = case.fresh_ivf(), case.model()
    lc.assert_host_lists(ivf, m, f"{case} before the chain")
    assert 5 <= case.shape["n_ops"] <= 8 and len(case.ops) >= case.shape["n_ops"]
    for i, op in enumerate(case.ops):
        assert lc.apply_to_ivf(ivf, op) is ivf
        m.apply(op)
        assert ivf._dev is None                 # (the numpy path: no device index was made on the way)
        lc.assert_host_lists(ivf, m, f"{case} after step {i}: {op['kind']} {op['sel']}")
    # the case's own index is as it was made
    lc.assert_host_lists(case.ivf, case.model(), f"{case}: the shared index changed")
    assert len(case.ivf.data) == case.N0


@pytest.mark.parametrize("seed", SEEDS[::3])
def test_update_is_remove_then_add_relabelled(seed):
    """On the layouts the chains pass through: the model's update equals its own remove + add with the added rows'
    labels N + i turned into ids[i] (update_reference.relabelled), list by list and column by column."""
    case = lc.case(seed)
    if case.skipped:
        pytest.skip(case.skipped)
    m = case.model()
    seen = 0
    for op in case.ops:
        if op["kind"] == "update":
            a, b = m.copy(), m.copy()
            a.apply(op)
            N = b.N
            b.remove(op["ids"]).add(op["new"], op["near"], op["labels"],
                                    None if b.groups is None else np.zeros(len(op["ids"]), np.int32))
            for x, y in zip(a.ids, relabelled(b.ids, N, op["ids"])):
                np.testing.assert_array_equal(x, y)
            for x, y in zip(a.labels, b.labels):
                np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(a.cols, b.cols)
            np.testing.assert_array_equal(a.data[op["ids"]], b.data[N:])
            seen += 1
        m.apply(op)
    if seed < lc.DEFAULT_SEEDS:
        assert seen or not any(op["kind"] == "update" for op in case.ops)


def test_remove_of_every_row_then_add_holds_the_added_rows_alone():
    seen = 0
    for seed in range(lc.DEFAULT_SEEDS):
        case = lc.case(seed)
        if case.skipped:
            continue
        m = case.model()
        for op in case.ops:
            empty = m.sizes.sum() == 0
            N = m.N
            m.apply(op)
            if empty and op["kind"] == "add":
                alone = lc.ListsModel([np.zeros(0, np.int64)] * len(m.ids), [np.zeros((0, len(m.zero)), np.uint8)] * len(m.ids),
                                      np.zeros_like(m.cols), np.zeros((N, m.data.shape[1]), m.data.dtype), m.zero)
                alone.add(op["new"], op["near"], op["labels"])
                for l in range(m.L):
                    np.testing.assert_array_equal(m.ids[l], alone.ids[l])
                    np.testing.assert_array_equal(m.labels[l], alone.labels[l])
                    # column j of list l: the added rows whose j-th nearest centre is l, ascending, and nothing else
                    o = 0
                    for j in range(m.kp):
                        np.testing.assert_array_equal(m.ids[l][o:o + m.cols[l, j]], N + np.flatnonzero(op["near"][:, j] == l))
                        o += m.cols[l, j]
                seen += 1
    assert seen >= 3


def test_cases_follow_from_the_seed():
    a, b = lc._build(5), lc.case(5)         # (an activating seed: every kind of step follows from the seed)
    assert a.shape == b.shape and a.skipped == b.skipped and len(a.ops) == len(b.ops)
    np.testing.assert_array_equal(a.qn, b.qn)
    for x, y in zip(a.ops, b.ops):
        assert x["kind"] == y["kind"] and x["sel"] == y["sel"]
        for key in ("ids", "X", "new", "near", "labels", "groups"):
            np.testing.assert_array_equal(x[key], y[key])


def test_resident_leg_covers_its_categories():
    """The seeds tests/test_list_chain_gpu.py runs on an index built in HBM, where the device assigns and encodes: from
    their shapes alone, so that a change to the generator cannot silently empty the leg."""
    default = lc.resident_seeds(range(lc.DEFAULT_SEEDS))
    shapes = [lc.resident_shape(s) for s in default]
    print({s: {k: c[k] for k in ("d", "n_clusters", "build_probes", "store", "rotate", "metric")}
           for s, c in zip(default, shapes)})
    assert 5 <= len(default) <= 10, default
    assert all(c["d"] <= 128 and c["build_probes"] <= 2 and not c["activate"] for c in shapes)
    rotated = [c["rotate"] and c["d"] != 100 for c in shapes]        # (FastPQ.fit leaves 100-d input unrotated)
    assert sum(r and c["store"] == "float32" for r, c in zip(rotated, shapes)) >= 2, shapes
    assert sum(not r and c["store"] == "float32" for r, c in zip(rotated, shapes)) >= 2, shapes
    assert sum(c["store"] == "float16" for c in shapes) >= 1, shapes
    assert sum(c["build_probes"] == 2 for c in shapes) >= 2, shapes
    assert sum(c["n_clusters"] > 1 for c in shapes) >= 4, shapes
    assert {c["metric"] for c in shapes} == {"euclidean", "angular"}, shapes
    assert sum(c["steered"] for c in shapes) >= 2 and sum(c["empty_then_add"] for c in shapes) >= 1, shapes


def test_the_allocation_rule_is_the_librarys_own():
    """facts() counts the adds that fit the device's vector buffer in place with a copy of DevBuf::ensure's rule
    (list_chain_shapes._allocated); the library shows neither the buffer's capacity nor its address for an uploaded
    index, so the copy is held against the source: should the rule change there, this fails and the copy follows."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "tinyknn_amd", "csrc", "api_internal.h")).read()
    assert "size_t want = bytes + bytes / 8 + 256;" in text
    assert lc._allocated(4000) == 4000 + 500 + 256
    build = open(os.path.join(root, "tinyknn_amd", "csrc", "api_build.hip")).read()
    assert "if ((size_t)N1 * d * esz > ix->data.cap) {" in build


def test_default_seeds_cover_every_category():
    """Counted over the default seeds whatever TINYKNN_FUZZ_SEEDS says; steps are counted per step, the rest per seed."""
    steps = collections.Counter()
    seeds = collections.Counter()
    kinds = collections.Counter()
    skipped = []
    for seed in range(lc.DEFAULT_SEEDS):
        case = lc.case(seed)
        if case.skipped:
            skipped.append(seed)
            continue
        c = case.shape
        assert 3 <= c["d"] <= 130 and 1 <= c["n_clusters"] <= 40 and 17 <= case.N0 <= 3000
        assert len(case.ops) >= 5
        f = lc.facts(case)
        for s, op in zip(f["steps"], case.ops):
            for name, v in s.items():
                if v:
                    steps[name] += 1
            if s["empty_block"]:
                steps[f"empty_block_kp{f['kp']}"] += 1
            kinds[f"{op['kind']}:{op['sel'].split()[0] if op['kind'] != 'add' else op['X'].shape[0]}"] += 1
        seeds["small"] += f["small"]
        seeds["one_list"] += f["one_list"]
        seeds[f["store"]] += 1
        seeds["narrow"] += f["M"] <= 8
        seeds["wide"] += f["M"] >= 64
        seeds["emptied_then_added"] += f["emptied_then_added"]
        seeds["activates"] += any(s["activates"] for s in f["steps"])
        seeds[f"kp{f['kp']}"] += 1
        seeds["rotated" if case.ivf.pq.R is not None else "unrotated"] += 1
        seeds[c["metric"]] += 1
        seeds["groups"] += case.ivf.groups is not None
        steps["adds_in_place"] += f["adds_in_place"]
        steps["adds_grown"] += f["adds_grown"]
    print(dict(steps), dict(seeds), dict(kinds), "skipped", skipped)
    assert steps["up16"] >= 6 and steps["down16"] >= 6, steps
    assert steps["emptied"] >= 4 and steps["refilled"] >= 3, steps
    assert seeds["small"] >= 3 and seeds["one_list"] >= 2, seeds
    assert steps["offsets_shift"] >= 8, steps
    assert steps["empty_block_kp2"] >= 3 and steps["empty_block_kp3"] >= 3, steps
    assert steps["stores_removed_again"] >= 3, steps
    assert steps["names_added"] >= 4, steps
    assert steps["add_into_empty"] >= 3 and seeds["emptied_then_added"] >= 3, (steps, seeds)
    assert steps["noop_remove"] >= 2, steps
    assert steps["big_block"] >= 3, steps
    assert seeds["float16"] >= 4 and seeds["float64"] >= 3, seeds
    assert seeds["narrow"] >= 2 and seeds["wide"] >= 2, seeds
    assert seeds["activates"] >= 2, seeds
    # both branches of tk_index_add_rows' step 1: the rows in the spare eighth behind the old ones, and a larger buffer
    assert steps["adds_in_place"] >= 3 and steps["adds_grown"] >= 3, steps
    assert len(skipped) <= 4, skipped
    # every kind of change and of selection is drawn by some default seed; both metrics, rotations, all kp
    for name in (["remove:" + x for x in lc.REMOVE_KINDS + ("edges",)] + ["update:" + x for x in lc.UPDATE_KINDS]
                 + [f"add:{n}" for n in lc.ADD_SIZES]):
        assert kinds[name] >= 1, (name, kinds)
    for name in ("kp1", "kp2", "kp3", "rotated", "unrotated", "euclidean", "angular"):
        assert seeds[name] >= 2, (name, seeds)
    assert seeds["groups"] >= 4, seeds
