"""The fuzz cases of tests/tag_shapes.py (TagCase: an awkward index of tests/restricted_shapes.py, its own restriction,
and tags, a mode and query masks drawn on top) are what tests/test_tags_fuzz_gpu.py needs them to be, on the CPU
reference alone: few default seeds are unbuildable, enough of the rest answer differently with the tags than without,
some probe lists wrap, every kind of tags and of mask is drawn, and everything follows from the seed."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import restricted_shapes as rs  # noqa: E402
import tag_shapes as ts  # noqa: E402
from tags_reference import passing  # noqa: E402


def test_default_seeds_hold_the_caps(oracle):
    """Counted over the default seeds whatever TINYKNN_FUZZ_SEEDS says."""
    default = range(ts.FUZZ_DEFAULT_SEEDS)
    cases = [ts.fuzz_case(s) for s in default]
    built = [t for t in cases if t.skipped is None]
    assert len(cases) - len(built) <= len(cases) // 4, [t.skipped for t in cases]
    differs, wraps = [], []
    kinds = collections.Counter()
    for t in built:
        c = t.case
        own, _ = c.want()                   # the case's own answer, without tags
        want, _ = t.want()
        if (want != own).any():
            differs.append(t.seed)
        if rs.facts(c, answers=False)["wraps"]:
            wraps.append(t.seed)
        kinds["tags:" + t.tag_kind] += 1
        kinds["mode:" + t.mode] += 1
        for mk in set(t.mask_kinds):
            kinds["mask:" + mk] += 1
        kinds["change:" + c.shape["change"]] += 1
        kinds["store:" + c.shape["store"]] += 1
        # what the tags promise of the ids, beside the case's own restriction
        for i, row in enumerate(want):
            ids = row[row != -1]
            if t.masks[i] != 0:
                assert passing(t.tags, t.masks[i], t.mode)[ids].all(), (t, i)
            if c.allowed is not None:
                assert c.allowed[ids].all(), (t, i)
    print("differ", differs, "wrap", wraps, dict(kinds))
    assert 3 * len(differs) >= len(built), (differs, len(built))
    assert len(wraps) >= 2, wraps
    for name in (["tags:" + k for k in ts.TAG_KINDS] + ["mode:" + m for m in ts.MODES]
                 + ["mask:" + k for k in ts.MASK_KINDS] + ["change:add", "change:remove", "store:float16"]):
        assert kinds[name] >= 1, (name, kinds)


def test_a_wider_range_of_seeds_builds():
    """TINYKNN_FUZZ_SEEDS widens the GPU file: the generator must make a case of every seed it may be given, whatever
    the kinds drawn — in particular single tags on a large index, where every tag that is drawn is carried, together
    with a query for an absent tag."""
    kinds = collections.Counter()
    for seed in range(64):
        t = ts.TagCase(seed)
        if t.skipped is not None:
            continue
        assert t.tags.dtype == np.uint64 and t.masks.dtype == np.uint64
        carried = ts.carriers(t.tags)
        for m, mk in zip(t.masks, t.mask_kinds):
            if mk == "absent":
                assert m != 0 and carried[int(np.log2(float(m)))] == 0, (t, m)
                if t.tag_kind == "single" and (carried[:63] > 0).all():
                    kinds["absent beside single tags that cover 0 .. 62"] += 1
            elif mk == "none":
                assert m == 0
        kinds[t.tag_kind] += 1
    assert all(kinds[k] >= 4 for k in ts.TAG_KINDS), kinds
    assert kinds["absent beside single tags that cover 0 .. 62"] >= 1, kinds


def test_cases_follow_from_the_seed():
    a, b = ts.TagCase(5), ts.fuzz_case(5)
    assert a.case is b.case and a.mode == b.mode and a.tag_kind == b.tag_kind
    np.testing.assert_array_equal(a.tags, b.tags)
    np.testing.assert_array_equal(a.masks, b.masks)
    assert a.tags.dtype == np.uint64 and len(a.tags) == len(a.case.ref_data) and len(a.masks) == len(a.case.qn)


def test_the_case_is_left_as_it_was_made():
    """the tags live on the TagCase: the shared Case and its IVF know nothing of them"""
    t = ts.fuzz_case(3)
    assert t.case.ivf.tags is None and "tags" not in t.case.device_kwargs()
    assert set(t.device_kwargs()) == set(t.case.device_kwargs()) | {"tags", "tags_mode"}
