"""The order in which the exact calls refuse: every call below is wrong in two ways at once, and the library must name
the fault its checks reach first — the return code and the whole text of tk_last_error.  The eight entry points are
called through the C ABI with the index's handle, past what the Python layer screens off.  Every case is refused before
any device work.  The texts were recorded while each entry point still carried its own copy of the checks; the shared
restriction builder (api_exact.hip: mode, tables, ranges, upload) keeps each call's order:
    knn_brute_ex / _matrix, radius_brute, radius_probe, knn_probe      tag_mode; tables group, tags, values; exclude
    knn_group       tag_mode; group[i] >= 0; tables groups, tags, values; exclude
    knn_between     tag_mode; tables values, groups, tags; "bounds no column"; group[i] >= -1; exclude"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_group_exact_gpu import _index  # noqa: E402

pytestmark = pytest.mark.gpu

N, D, NQ, K = 2000, 16, 5, 3
ARG, STATE = -1, -3

TAG_MODE = "bad argument: tag_mode: 0 (any) or 1 (all)"
EXCLUDE = "bad argument: exclude: entries in [-1, N)"
K_RANGE = "bad argument: 1 <= k <= min(1024, N)"
NO_GROUPS = "a group array was passed but the index has no groups: tk_index_set_groups first"
NO_TAGS = "a tag array was passed but the index has no tags: tk_index_set_tags first"
NO_VALUES = "a value array was passed but the index has no values: tk_index_set_values first"
GROUP_ID = "bad argument: group: every entry must be a group id >= 0"
GROUP_OR_ANY = "bad argument: group: entries must be a group id >= 0 or -1"
UNBOUNDED = ("bad argument: between: query 0 bounds no column (an unrestricted query is tk_index_knn_brute's or "
             "tk_index_query_batch's to answer)")
GROUP_REQUIRED = "bad argument: group: one group id per query is required"
BETWEEN_REQUIRED = "bad argument: between: the ranges of every query are required"

I64 = np.iinfo(np.int64)


class Args:
    """the arrays a call is handed; what a case does not name is NULL (tag_mode 0)"""

    def __init__(self):
        rng = np.random.RandomState(5)
        self.q = rng.randn(NQ, D).astype(np.float32)
        self.q_pq = np.zeros((NQ, D), np.float32)
        self.radius = np.ones(NQ, np.float32)
        self.out = np.full((NQ, K), -7, np.int64)
        self.dist = np.zeros((NQ, K), np.float64)
        self.lims = np.zeros(NQ + 1, np.int64)
        self.total = np.zeros(1, np.int64)
        self.named = dict(
            mask=np.ones(N, np.uint8),
            exclude_ok=np.full(NQ, -1, np.int64), exclude_N=np.full(NQ, N, np.int64),
            exclude_m2=np.full(NQ, -2, np.int64),
            group_ok=np.zeros(NQ, np.int32), group_any=np.full(NQ, -1, np.int32), group_m2=np.full(NQ, -2, np.int32),
            tags=np.ones(NQ, np.uint64),
            between_ok=np.tile(np.array([0, 10], np.int64), (NQ, 1, 1)),
            between_free=np.tile(np.array([I64.min, I64.max], np.int64), (NQ, 1, 1)))

    def p(self, name):
        return None if name is None else self.named[name].ctypes.data


def refusal(a, h, entry, k=K, mask=None, exclude=None, group=None, tags=None, tag_mode=0, between=None):
    """(return code, tk_last_error) of one call of `entry` on the index handle h"""
    from tinyknn_amd import _lib
    lib = _lib.lib()
    f32, i64 = _lib._f32p, _lib._i64p
    q, out, dist = _lib.ptr(a.q, f32), _lib.ptr(a.out, i64), a.dist.ctypes.data
    r6 = (a.p(mask), a.p(exclude), a.p(group), a.p(tags), tag_mode, a.p(between))
    tail = (1, 0, 1 << 20, _lib.ptr(a.lims, i64), _lib.ptr(a.total, i64))
    if entry in ("knn_brute_ex", "knn_brute_matrix"):
        rc = getattr(lib, "tk_index_" + entry)(h, q, NQ, k, *r6, out, dist)
    elif entry == "radius_brute":
        rc = lib.tk_index_radius_brute(h, q, NQ, _lib.ptr(a.radius, f32), *r6, *tail)
    elif entry == "radius_probe":
        rc = lib.tk_index_radius_probe(h, q, a.q_pq.ctypes.data, 0, NQ, 1, _lib.ptr(a.radius, f32), *r6, *tail)
    elif entry in ("knn_probe", "knn_probe_matrix"):
        rc = getattr(lib, "tk_index_" + entry)(h, q, a.q_pq.ctypes.data, 0, NQ, k, 1, *r6, out, dist)
    elif entry == "knn_group":
        rc = lib.tk_index_knn_group(h, q, NQ, k, a.p(group), a.p(mask), a.p(exclude), a.p(tags), tag_mode,
                                    a.p(between), out, dist)
    else:
        assert entry == "knn_between"
        rc = lib.tk_index_knn_between(h, q, NQ, k, a.p(between), a.p(mask), a.p(exclude), a.p(group), a.p(tags),
                                      tag_mode, out, dist)
    assert (a.out == -7).all() and a.lims[1:].sum() == 0          # a refused call writes no answer
    return rc, lib.tk_last_error().decode()


@pytest.fixture(scope="module")
def made():
    """(args, {store: an index of N x D rows without groups, tags or values})"""
    data = np.random.RandomState(4).randn(N, D).astype(np.float32)
    return Args(), {"float32": _index(data), "float16": _index(data, "float16")}


# the calls that hand the restriction to the shared builder as it is, and the store each needs
OVER_ROWS = [("knn_brute_ex", "float32"), ("knn_brute_matrix", "float16"), ("radius_brute", "float32"),
             ("radius_probe", "float32"), ("knn_probe", "float32"), ("knn_probe_matrix", "float16")]

# two faults each, the first in the call's order named: nothing is set on the index
BARE = [
    (dict(tags="tags", exclude="exclude_N"), STATE, NO_TAGS),                           # a table before exclude
    (dict(between="between_ok", tags="tags", tag_mode=2), ARG, TAG_MODE),               # tag_mode before a table
    (dict(group="group_ok", tags="tags"), STATE, NO_GROUPS),                            # groups before tags
    (dict(tags="tags", between="between_ok"), STATE, NO_TAGS),                          # tags before values
    (dict(group="group_ok", between="between_ok", exclude="exclude_m2"), STATE, NO_GROUPS),
    (dict(exclude="exclude_N", tag_mode=-1), ARG, TAG_MODE),                            # tag_mode before exclude
    (dict(mask="mask", exclude="exclude_m2", tag_mode=3), ARG, TAG_MODE),
]


@pytest.mark.parametrize("entry,store", OVER_ROWS)
def test_calls_over_rows_and_probed_lists(made, entry, store):
    a, devs = made
    for kw, code, text in BARE:
        assert refusal(a, devs[store]._h, entry, **kw) == (code, text), (entry, kw)
    assert refusal(a, devs[store]._h, entry, exclude="exclude_N") == (ARG, EXCLUDE)


def test_knn_group_and_knn_between_without_tables(made):
    a, devs = made
    for store in ("float32", "float16"):
        h = devs[store]._h
        for kw, code, text in [
                (dict(group="group_ok", exclude="exclude_m2"), STATE, NO_GROUPS),           # the table before exclude
                (dict(group="group_any", exclude="exclude_N"), ARG, GROUP_ID),              # its entries before the table
                (dict(group="group_any", tags="tags", tag_mode=2), ARG, TAG_MODE),          # tag_mode before its entries
                (dict(group="group_ok", tags="tags", between="between_ok"), STATE, NO_GROUPS),
                (dict(group="group_ok", k=0, tag_mode=2), ARG, K_RANGE),                    # the frame's checks first
                (dict(exclude="exclude_N", tag_mode=2), ARG, GROUP_REQUIRED)]:
            assert refusal(a, h, "knn_group", **kw) == (code, text), kw
        for kw, code, text in [
                (dict(between="between_free", tags="tags"), STATE, NO_VALUES),              # values in front of all
                (dict(between="between_ok", group="group_m2"), STATE, NO_VALUES),
                (dict(between="between_ok", tag_mode=2), ARG, TAG_MODE),                    # tag_mode before values
                (dict(between="between_ok", k=1025, tag_mode=2), ARG, K_RANGE),
                (dict(group="group_m2", tag_mode=2), ARG, BETWEEN_REQUIRED)]:
            assert refusal(a, h, "knn_between", **kw) == (code, text), kw


def test_knn_group_and_knn_between_with_groups_and_values(made):
    """groups and values on the index, no tags: the checks behind the tables"""
    a, devs = made
    dev = devs["float32"]
    dev.set_groups(np.arange(N, dtype=np.int32) % 7)
    dev.set_values(np.arange(N, dtype=np.int64))
    try:
        for kw, code, text in [
                (dict(between="between_free", tags="tags"), STATE, NO_TAGS),                # a table before the bounds
                (dict(between="between_free", group="group_m2"), ARG, UNBOUNDED),           # the bounds before group
                (dict(between="between_ok", group="group_m2", exclude="exclude_N"), ARG, GROUP_OR_ANY),
                (dict(between="between_ok", group="group_any", exclude="exclude_N"), ARG, EXCLUDE),
                (dict(between="between_free", exclude="exclude_m2"), ARG, UNBOUNDED)]:
            assert refusal(a, dev._h, "knn_between", **kw) == (code, text), kw
        for kw, code, text in [
                (dict(group="group_ok", tags="tags", exclude="exclude_m2"), STATE, NO_TAGS),
                (dict(group="group_any", tags="tags"), ARG, GROUP_ID),
                (dict(group="group_ok", between="between_ok", exclude="exclude_m2"), ARG, EXCLUDE)]:
            assert refusal(a, dev._h, "knn_group", **kw) == (code, text), kw
        for entry in ("knn_brute_ex", "radius_brute", "radius_probe", "knn_probe"):
            for kw, code, text in [
                    (dict(group="group_m2", between="between_free", tags="tags", exclude="exclude_N"), STATE, NO_TAGS),
                    (dict(group="group_ok", between="between_ok", exclude="exclude_N"), ARG, EXCLUDE)]:
                assert refusal(a, dev._h, entry, **kw) == (code, text), (entry, kw)
    finally:
        dev.set_groups(None)
        dev.set_values(None)
