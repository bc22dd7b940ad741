"""per_group= without a GPU: the properties of the CPU reference (tests/per_group_reference.py), the
argument checks that run before the device is touched, and a census of the default cases the GPU test runs
(tests/per_group_shapes.py) — the numbers come from the CPU oracle alone."""
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import per_group_shapes as shapes  # noqa: E402
from per_group_reference import capped_batch, capped_from_heaps, walk  # noqa: E402
from per_group_shapes import K  # noqa: E402


def _is_subsequence(part, whole):
    it = iter(whole)
    return all(any(x == y for y in it) for x in part)


# ---- the reference's properties, on a fixture with a rotation and on the synthetic index with repeated rows ----------

@pytest.mark.parametrize("index", ["an20", "syn"])
def test_reference_properties(oracle, index):
    if index == "syn":
        _, ox, qn, _, _ = shapes.synthetic()
    else:
        _, ox, qn, _ = shapes.fixture(index)
    N = len(ox.data)
    h = shapes.heaps(index, shapes.N_PROBES)
    plain_ids, plain_d, plain_n, ranked = capped_from_heaps(oracle, ox, qn, h, 0, np.zeros(N, np.int32), K, full=True)
    # m = 0 is the uncapped reference: the guarded reference's own answer, the oracle's query
    for i, q in enumerate(qn):
        want = ox.query(q, K, shapes.N_PROBES)
        np.testing.assert_array_equal(plain_ids[i][:len(want)], want)
        assert (plain_ids[i][len(want):] == -1).all() and plain_n[i] == len(want)
    for name in ("mod3", "oct", "one", "own"):
        groups = shapes.assignment(name, N)
        for m in (1, 2, 3, K):
            ids, dist, counts = capped_from_heaps(oracle, ox, qn, h, m, groups, K)
            for i in range(len(qn)):
                got = ids[i][:counts[i]]
                assert (ids[i][counts[i]:] == -1).all() and np.isinf(dist[i][counts[i]:]).all()
                # no group more than m times
                _, per = np.unique(groups[got], return_counts=True)
                assert per.max(initial=0) <= m
                # a subsequence of the full ranking, each id with its distance
                c, d = ranked[i]
                assert _is_subsequence(list(got), list(c))
                where = {int(x): j for j, x in enumerate(c)}
                assert all(dist[i][j] == d[where[int(x)]] for j, x in enumerate(got))
                # maximal: a skipped candidate in front of the last kept one had m of its group kept before it,
                # and a row that ends early skipped only such candidates
                kept = set(int(x) for x in got)
                upto = len(c) if counts[i] < K else where[int(got[-1])]
                seen = {}
                for x in c[:upto]:
                    g = int(groups[int(x)])
                    if int(x) in kept:
                        seen[g] = seen.get(g, 0) + 1
                    else:
                        assert seen.get(g, 0) == m, (name, m, i, int(x))
            if name == "own" or m == 0:
                np.testing.assert_array_equal(ids, plain_ids)       # all-distinct groups: the uncapped reference
                assert np.array_equal(dist.view(np.uint32), plain_d.view(np.uint32))
    # m >= k with any groups keeps at most k of a group: the first k of the ranking, the uncapped answer
    ids, _, _ = capped_from_heaps(oracle, ox, qn, h, K, shapes.assignment("one", N), K)
    np.testing.assert_array_equal(ids, plain_ids)


def test_capped_batch_is_the_guarded_references_heap_then_the_walk(oracle):
    _, ox, qn, _, groups = shapes.synthetic()
    few = shapes.synthetic_few()
    a = capped_batch(oracle, ox, qn, 1, groups, K, 1, allowed=few)
    b = capped_from_heaps(oracle, ox, qn, shapes.heaps("syn", 1, True), 1, groups, K)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert walk([4, 9, 14, 5], np.arange(20) % 5, 1, 3) == [0, 3]
    assert walk([4, 9, 14, 5], np.arange(20) % 5, 0, 3) == [0, 1, 2]
    assert walk([4, 9, 14, 5], np.arange(20) % 5, 2, 3) == [0, 1, 3]


# ---- argument checks that need no device ------------------------------------------------------------------------------

def test_arguments_refused_before_the_device(monkeypatch):
    import tinyknn_amd
    from tinyknn_amd.ivf import query_caps
    ivf, _, qn, _ = shapes.fixture("an20")
    monkeypatch.setattr(type(ivf), "device_index", lambda self: pytest.fail("the device was asked for"))
    qs = np.array(qn[:6], copy=True)
    for bad in (-1, np.array([1, 2, -3, 0, 0, 0])):
        with pytest.raises(ValueError, match="per_group"):
            ivf.query_batch(qs, K, 5, per_group=bad)
    with pytest.raises(ValueError, match=r"one entry per query \(6\), got 5"):
        ivf.query_batch(qs, K, 5, per_group=np.ones(5, dtype=int))
    for bad in (1.5, np.ones(6), np.ones(6, dtype=bool), np.ones((6, 1), dtype=int)):
        with pytest.raises(TypeError, match="per_group"):
            ivf.query_batch(qs, K, 5, per_group=bad)
    with pytest.raises(NotImplementedError, match="fast=True with per_group= is not supported"):
        ivf.query_batch(qs, K, 5, fast=True, per_group=1)
    with pytest.raises(ValueError, match="per_group"):
        ivf.query(qs[0], K, 5, per_group=-2)
    with pytest.raises(ValueError, match="per_group"):
        ivf.query_rows([1, 2, 3], K, 5, per_group=[1, -1, 1])
    with pytest.raises(ValueError, match=r"one entry per query \(3\), got 2"):
        ivf.query_rows([1, 2, 3], K, 5, per_group=[1, 1])
    assert query_caps(3, 4).tolist() == [3, 3, 3, 3] and query_caps(3, 4).dtype == np.int32
    assert query_caps(np.array([0, 2**31 - 1]), 2).tolist() == [0, 2**31 - 1]
    with pytest.raises(ValueError):
        query_caps(2**31, 1)
    assert tinyknn_amd.IVF is type(ivf)


def test_every_query_entry_point_takes_it_and_the_sharded_engines_do_not():
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import IVF, DeviceIndex
    from tinyknn_amd.multi_gpu import ListShardedIndex, ReplicaGroup
    for f in (IVF.query, IVF.query_batch, IVF.query_rows, DeviceIndex.query_batch, DeviceIndex.query_rows):
        assert inspect.signature(f).parameters["per_group"].default is None, f.__qualname__
    assert inspect.signature(DeviceIndex.query_batch_dev).parameters["per_group_ptr"].default is None
    # the sharded engines take no restriction of any kind, this one included: the word is refused as theirs are
    for f in (ListShardedIndex.query_batch, ReplicaGroup.query_batch):
        p = inspect.signature(f).parameters
        assert "per_group" not in p and not any(x.kind == x.VAR_KEYWORD for x in p.values()), f.__qualname__
    # _ex6 is _ex5 with one more pointer
    for stem in ("tk_index_query_batch", "tk_index_query_batch_dev"):
        a5, a6 = _lib.SIGNATURES[stem + "_ex5"][1], _lib.SIGNATURES[stem + "_ex6"][1]
        assert len(a6) == len(a5) + 1 and a6[:7] == a5[:7] and a6[8:] == a5[7:]
    header = open(os.path.join(os.path.dirname(HERE), "include", "tinyknn_hip.h")).read()
    assert "tk_index_query_batch_ex6(" in header and "tk_index_query_batch_dev_ex6(" in header


# ---- the census of the GPU test's default cases ----------------------------------------------------------------------

def test_census_of_the_default_cases(oracle):
    cases = shapes.default_cases()
    assert len(cases) == len(set(cases))
    differ = total = 0
    short_rows = short_heaps = empty_heaps = ties = 0
    for case in cases:
        index, a, m, n_probes, few = case
        ids, dist, counts, ranked = shapes.reference(case, full=True)
        ox, qn, groups, _, h = shapes.case_inputs(case)
        plain = capped_from_heaps(oracle, ox, qn, h, 0, groups, K)[0]
        if m in (1, 2):                 # the cases with 0 < m < k
            total += len(qn)
            differ += int((ids != plain).any(axis=1).sum())
        short_rows += int((counts < K).sum())
        for c, d in ranked:
            short_heaps += len(c) <= K
            empty_heaps += len(c) == 0
            ties += len(c) > K and len(np.unique(d)) < len(d)
    assert differ * 4 >= total, (differ, total)
    assert short_rows >= 1 and short_heaps >= 1 and empty_heaps >= 1 and ties >= 1, \
        (short_rows, short_heaps, empty_heaps, ties)
    print(f"census: {differ}/{total} capped answers differ, {short_rows} rows end early, {short_heaps} heaps <= k "
          f"({empty_heaps} empty), {ties} rankings with equal distances")
    # the repeated rows of the synthetic index come back side by side where they are in one group and m allows it, and
    # the second copy is dropped where m = 1 and they share a group
    _, ox, qn, _, groups = shapes.synthetic()
    twins_same = {src + j: at + j for at, src, n in shapes.SYN_TWINS[:1] for j in range(n)}
    ids1 = shapes.reference(("syn", "syn8", 1, shapes.N_PROBES, False))[0]
    ids2 = shapes.reference(("syn", "syn8", 2, shapes.N_PROBES, False))[0]
    both = [i for i in range(len(qn)) if any(a in ids2[i] and b in ids2[i] for a, b in twins_same.items())]
    assert both, "no query returns a repeated row and its copy"
    for i in both:
        for a, b in twins_same.items():
            if a in ids2[i] and b in ids2[i]:
                assert (a in ids1[i]) != (b in ids1[i])         # equal distances: the lower heap position alone stays
                break
