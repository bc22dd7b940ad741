"""Row tags on the device (tags.hip: tk_index_set_tags, tk_index_query_batch[_dev]_ex4; IVF.set_tags, tags=,
tags_mode=).  Every comparison is exact: ids and, through debug=True, probes and heap arrays against
tests/tags_reference.py — per query the guarded reference with the allowed set its mask passes.  The inputs come from
tests/tag_shapes.py; tests/test_tags_cpu.py asserts on the reference alone that they can tell a wrong pass (answers
differ from the unrestricted ones, short and full answers, a compare of the low words alone answers differently)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tag_shapes as ts  # noqa: E402
from allowed_reference import guarded_batch  # noqa: E402
from conftest import G6_TAGS, golden  # noqa: E402
from groups_reference import grouped_batch  # noqa: E402
from store_reference import exact_distances, fixture_ivf, oracle_index, same_bits  # noqa: E402
from tags_reference import passing, tagged_batch  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("probes", "heap_idx", "heap_val")
U64 = np.uint64


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    return tinyknn_amd


def _same(got, gd, want, wd, msg=""):
    np.testing.assert_array_equal(got, want, err_msg=str(msg))
    for key in KEYS:
        np.testing.assert_array_equal(gd[key], wd[key], err_msg=f"{key} {msg}")


def _within_tags(got, masks, mode, tags):
    for i, m in enumerate(masks):
        ids = got[i][got[i] != -1]
        if m != 0:
            assert passing(tags, m, mode)[ids].all(), (i, m)


@pytest.mark.parametrize("mode", ts.MODES)
@pytest.mark.parametrize("tag", G6_TAGS)
def test_fixtures_every_probe_count_assignment_and_mode(tk, oracle, tag, mode):
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = fixture_ivf(g)
    ox = oracle_index(oracle, ivf, g["data"])
    dev = ivf.device_index()
    qn, qp, N = g["qn"], g["qpq"], len(g["data"])
    nq = len(qn)
    assert dev.tags_set() == 0 and dev.tag_table()["builds"] == 0
    ids_per_list = ivf.ids[:len(ivf.active_centers)]
    for a, (name, tags) in enumerate(ts.assignments(ids_per_list, N, 3).items()):
        ivf.set_tags(tags)
        assert dev.tags_set() == N and not dev.tag_table()["built"]
        for n_probes in (1, 2, 5, 10):
            masks = ts.query_masks(tags, nq, 10 * n_probes + a)
            want, wd = tagged_batch(oracle, ox, qn, masks, mode, tags, 10, n_probes, debug=True)
            got, gd = dev.query_batch(qn, qp, 10, n_probes, debug=True, tags=masks, tags_mode=mode)
            _same(got, gd, want, wd, (name, mode, n_probes))
            _within_tags(got, masks, mode, tags)
            if name != "some":
                assert (got[2] == -1).all()     # a tag no row carries: no id
            # all 0: the unrestricted call; one mask everywhere (an int): allowed=(the rows it passes)
            plain = dev.query_batch(qn, qp, 10, n_probes, debug=True)
            _same(*dev.query_batch(qn, qp, 10, n_probes, debug=True, tags=np.zeros(nq, dtype=U64), tags_mode=mode),
                  *plain, (name, "all 0"))
            m4 = int(masks[4])
            _same(*dev.query_batch(qn, qp, 10, n_probes, debug=True, tags=m4, tags_mode=mode),
                  *dev.query_batch(qn, qp, 10, n_probes, debug=True, allowed=passing(tags, m4, mode)), (name, "one mask"))
        assert dev.tag_table()["builds"] == a + 1       # one table per set_tags, whatever the calls
    t = dev.tag_table()
    assert t["built"] and t["row_bytes"] == 8 * N
    assert t["bytes"] == 128 * int(((np.asarray(g["list_sizes"], dtype=np.int64) + 15) // 16).sum())


@pytest.mark.parametrize("mode", ts.MODES)
def test_ivf_query_is_the_row_of_query_batch(tk, oracle, mode):
    g = golden("g6_ivf_an100.npz")
    ivf = fixture_ivf(g)
    ox = oracle_index(oracle, ivf, g["data"])
    N = len(g["data"])
    tags = ts.assignments(ivf.ids[:len(ivf.active_centers)], N, 5)["edges"]
    ivf.set_tags(tags)              # (before the device index exists: uploaded when it is made)
    qs = np.array(g["qn"][np.arange(65) % len(g["qn"])], copy=True)     # 65 queries: one more than a wave of lanes
    qn = ivf._prepare(qs.copy())[0]
    masks = ts.query_masks(tags, len(qs), 1)
    want = tagged_batch(oracle, ox, qn, masks, mode, tags, 10, 5)
    batch = ivf.query_batch(qs, 10, n_probes=5, tags=masks, tags_mode=mode)
    np.testing.assert_array_equal(batch, want)
    assert ivf.device_index().tags_set() == N
    lengths = []
    for i in range(len(qs)):
        got = ivf.query(qs[i].copy(), 10, n_probes=5, tags=int(masks[i]), tags_mode=mode)
        w = batch[i]
        np.testing.assert_array_equal(got, w[w != -1] if w[-1] == -1 else w, err_msg=f"query {i}")
        lengths.append(len(got))
    assert lengths[2] == 0 and max(lengths) == 10       # the absent tag; a full answer
    np.testing.assert_array_equal(ivf.query(qs[0].copy(), 10, n_probes=5, tags=0, tags_mode=mode),
                                  ivf.query(qs[0].copy(), 10, n_probes=5))


# ---- every replay form: the synthetic index of tests/tag_shapes.py, built with n_probes 1 and 2 ----

SYN_N, SYN_NQ = ts.SYN_N, ts.SYN_NQ


@pytest.fixture(scope="module")
def synthetic(tk, oracle):
    """get(kp) -> (a copy of the shared index with its tags set, ox, qn, qp, tags, {mode: (masks, want, debug)}):
    every reference is computed once and left unchanged"""
    import copy
    made = {}

    def get(kp):
        if kp not in made:
            shared, qs, tags, _, _ = ts.synthetic(kp)
            ivf = copy.copy(shared)         # (the device index and the tags are kept on the copy)
            ivf._dev = None
            ivf.set_tags(tags)
            ox = oracle_index(oracle, ivf, ivf.data)
            qn, qp = ivf._prepare(qs.copy())
            want = {}
            for mode in ts.MODES:
                masks = ts.synthetic_masks(tags, mode)
                want[mode] = (masks,) + tagged_batch(oracle, ox, qn, masks, mode, tags, 10, 10, debug=True)
            made[kp] = (ivf, ox, qn, qp, tags, want)
        return made[kp]
    return get


@pytest.mark.parametrize("mode", ts.MODES)
@pytest.mark.parametrize("kp", [1, 2])
def test_every_replay_form(tk, synthetic, kp, mode):
    from tinyknn_amd import _lib
    ivf, ox, qn, qp, tags, wants = synthetic(kp)
    masks, want, wd = wants[mode]
    dev = ivf.device_index()
    assert (kp == 1) == (dev.twin_table_width() == 0)
    builds = dev.tag_table()["builds"]
    try:
        for heap_mode in (0, 1, 2, 3):
            for plain in (False, "always"):
                for pair_nq in (4, 8192):
                    dev.set_heap_mode(heap_mode)
                    dev.set_plain_scan(plain)
                    dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
                    got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, tags=masks, tags_mode=mode)
                    _same(got, gd, want, wd, (kp, mode, heap_mode, plain, pair_nq))
        _within_tags(got, masks, mode, tags)
        # the limit at -128: every query with a plain list fails the lemma's check, is scanned again exactly and masked
        # again through the flag list (the pass's `only` branch)
        dev.set_heap_mode(0)
        dev.set_plain_scan("always")
        dev.set_option(_lib.OPT_PLAIN_LIMIT, -128)
        for pair_nq in (4, 8192):
            dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
            got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, tags=masks, tags_mode=mode)
            st = dev.plain_stats()
            _same(got, gd, want, wd, (kp, mode, "limit -128", pair_nq, st))
            assert st["plain_units"] > 0 and st["flagged_queries"] > 0, st
        assert dev.tag_table()["builds"] == max(builds, 1)      # one table for both modes
    finally:
        dev.set_heap_mode(0); dev.set_plain_scan(True); dev.set_option(_lib.OPT_PAIR_NQ, 4)
        dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)


def test_with_an_allowed_set_an_excluded_row_a_group_and_distances(tk, oracle, synthetic):
    from tinyknn_amd import _lib
    ivf, ox, qn, qp, tags, wants = synthetic(1)
    dev = ivf.device_index()
    rng = np.random.default_rng(3)
    allowed = rng.random(SYN_N) < 0.5
    groups = rng.integers(0, 3, SYN_N).astype(np.int32)
    group = rng.integers(-1, 3, SYN_NQ).astype(np.int32)
    dev.set_groups(groups)
    aset = dev.allow(allowed)
    try:
        for mode in ts.MODES:
            masks, want, _ = wants[mode]
            exclude = want[:, 0].copy()         # every query's best id (or -1) may not come back
            assert (exclude >= 0).sum() > SYN_NQ // 3
            ref = dict(allowed=dict(allowed=allowed), exclude=dict(exclude=exclude),
                       group=dict(group=group, groups=groups),
                       everything=dict(allowed=allowed, exclude=exclude, group=group, groups=groups))
            kws = dict(allowed=dict(allowed=aset), exclude=dict(exclude=exclude), group=dict(group=group),
                       everything=dict(allowed=aset, exclude=exclude, group=group))
            legs = [(name, kws[name], tagged_batch(oracle, ox, qn, masks, mode, tags, 10, 10, debug=True, **ref[name]))
                    for name in ref]
            # ("forced": pinned on with the limit at -128 — every query with a plain list is flagged, scanned again
            #  exactly and masked again by all the passes through the flag list)
            for plain in (False, "always", "forced"):
                dev.set_plain_scan("always" if plain == "forced" else plain)
                dev.set_option(_lib.OPT_PLAIN_LIMIT, -128 if plain == "forced" else 0x7fffffff)
                for name, kw, (w, wdbg) in legs:
                    got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, tags=masks, tags_mode=mode, **kw)
                    _same(got, gd, w, wdbg, (mode, name, plain))
                    if plain == "forced":
                        st = dev.plain_stats()
                        assert st["plain_units"] > 0 and st["flagged_queries"] > 0, (mode, name, st)
                    _within_tags(got, masks, mode, tags)
                    if "exclude" in kw:
                        assert not (got == np.where(exclude >= 0, exclude, -2)[:, None]).any()
                    if "allowed" in kw:
                        assert allowed[got[got != -1]].all()
            dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
            dev.set_plain_scan(True)
            # distances: the ids of the tagged call, each with the rescoring's exact distance
            ids, dist = dev.query_batch(qn, qp, 10, 10, tags=masks, tags_mode=mode, return_distances=True)
            np.testing.assert_array_equal(ids, want)
            assert same_bits(dist, exact_distances(oracle, qn, ivf.data, ids))
            ids, dist = dev.query_batch(qn, qp, 10, 10, tags=masks, tags_mode=mode, allowed=aset, exclude=exclude,
                                        group=group, return_distances=True)
            np.testing.assert_array_equal(ids, w)
            assert same_bits(dist, exact_distances(oracle, qn, ivf.data, ids))
    finally:
        dev.set_plain_scan(True)
        dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
        aset.close()
        dev.set_groups(None)
    # the index built with n_probes = 2 (labels repeat: the TWIN form): the tag pass beside the allow pass, and all four
    # passes, behind its flagged re-scan
    ivf2, ox2, qn2, qp2, tags2, wants2 = synthetic(2)
    dev2 = ivf2.device_index()
    dev2.set_groups(groups)
    aset2 = dev2.allow(allowed)
    try:
        dev2.set_plain_scan("always")
        dev2.set_option(_lib.OPT_PLAIN_LIMIT, -128)
        for mode in ts.MODES:
            masks2, want2, _ = wants2[mode]
            exclude2 = want2[:, 0].copy()
            for name, kw, ref in (("allowed", dict(allowed=aset2), dict(allowed=allowed)),
                                  ("everything", dict(allowed=aset2, exclude=exclude2, group=group),
                                   dict(allowed=allowed, exclude=exclude2, group=group, groups=groups))):
                w2, wd2 = tagged_batch(oracle, ox2, qn2, masks2, mode, tags2, 10, 10, debug=True, **ref)
                got, gd = dev2.query_batch(qn2, qp2, 10, 10, debug=True, tags=masks2, tags_mode=mode, **kw)
                st = dev2.plain_stats()
                _same(got, gd, w2, wd2, (2, mode, name, "forced", st))
                assert st["plain_units"] > 0 and st["flagged_queries"] > 0, (mode, name, st)
                _within_tags(got, masks2, mode, tags2)
                assert allowed[got[got != -1]].all()
    finally:
        dev2.set_plain_scan(True)
        dev2.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
        aset2.close()
        dev2.set_groups(None)


def test_pipelined_pairs_alternating_kinds(tk, oracle, synthetic):
    """Device calls in pairs: tagged-any, tagged-all, grouped and unrestricted ones in turn, each equal to its own
    reference.  Whether two calls ran as one batch is read from the lane replay's wave count (200 queries: 4 waves of
    64 alone, 7 for two calls together): two calls of one mode join, a tagged-any and a tagged-all call never do."""
    import torch
    from tinyknn_amd import _lib
    ivf, ox, qn, qp, tags, wants = synthetic(1)
    dev = ivf.device_index()
    nq = 200
    qn, qp = np.ascontiguousarray(qn[:nq]), np.ascontiguousarray(qp[:nq])
    m_any, m_all = wants["any"][0][:nq], wants["all"][0][:nq]
    other = np.roll(m_any, 7)
    groups = np.random.default_rng(8).integers(0, 7, SYN_N).astype(np.int32)
    group = np.random.default_rng(9).integers(-1, 7, nq).astype(np.int32)
    dev.set_groups(groups)
    want = dict(any=wants["any"][1][:nq], all=wants["all"][1][:nq], none=guarded_batch(oracle, ox, qn, 10, 10),
                any_other=tagged_batch(oracle, ox, qn, other, "any", tags, 10, 10),
                grouped=grouped_batch(oracle, ox, qn, group, groups, 10, 10),
                all_grouped=tagged_batch(oracle, ox, qn, m_all, "all", tags, 10, 10, group=group, groups=groups))
    assert (want["any"] != want["all"]).any() and (want["any_other"] != want["any"]).any()
    kinds = ["any", "any_other", "all", "all_grouped", "grouped", "none", "any", "all", "none", "none", "all", "any",
             "grouped", "any"]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    as_i64 = lambda m: cuda(np.ascontiguousarray(m, dtype=U64).view(np.int64))      # noqa: E731
    qn_d, qp_d, gr_d = cuda(qn), cuda(qp), cuda(group)
    masks = dict(any=(as_i64(m_any), "any"), any_other=(as_i64(other), "any"), all=(as_i64(m_all), "all"),
                 all_grouped=(as_i64(m_all), "all"))

    def run(kinds):
        outs = [torch.full((nq, 10), -7, dtype=torch.int64, device="cuda") for _ in kinds]
        torch.cuda.synchronize()
        dev.set_option(_lib.OPT_REPLAY_COUNT, 1)
        for kind, out in zip(kinds, outs):
            m, mode = masks.get(kind, (None, "any"))
            dev.query_batch_dev(qn_d.data_ptr(), qp_d.data_ptr(), 0, nq, 10, 10, out.data_ptr(),
                                group_ptr=gr_d.data_ptr() if "grouped" in kind else None,
                                tags_ptr=None if m is None else m.data_ptr(), tags_mode=mode)
        dev.join()
        torch.cuda.synchronize()
        for i, (kind, out) in enumerate(zip(kinds, outs)):
            np.testing.assert_array_equal(out.cpu().numpy(), want[kind], err_msg=f"call {i} {kind}")
        return dev.replay_stats()["waves"]
    try:
        dev.set_option(_lib.OPT_PAIR_NQ, 0)         # small batches too take the lane kernels, which count waves
        dev.set_pipeline(3)
        dev.set_coalesce(2)
        run(kinds)
        assert dev.last_replay()["form"] == _lib.REPLAY_LANES
        alone, together = 2 * ((nq + 63) // 64), (2 * nq + 63) // 64
        assert together < alone
        assert run(["any", "any_other"]) == together        # two arrays of one mode: one batch
        assert run(["all", "all"]) == together
        assert run(["any", "all"]) == alone                 # never a pair
        assert run(["all", "any"]) == alone
        assert run(["any", "none"]) == alone                # nor a tagged call with an untagged one
    finally:
        dev.join()
        dev.set_option(_lib.OPT_REPLAY_COUNT, 0)
        dev.set_pipeline(1)
        dev.set_coalesce(1)
        dev.set_option(_lib.OPT_PAIR_NQ, 4)
        dev.set_groups(None)


SUB_CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from tinyknn_amd import IVF, FastPQ, _lib
from oracle import oracle
from allowed_reference import reference_index
from tags_reference import tagged_batch
import tag_shapes as ts
assert _lib.device_count() >= 1, "no GPU visible"
np.random.seed(5)
n, d, nq0 = 40000, 48, 200
cent = np.random.randn(150, d)
X = (cent[np.random.randint(150, size=n)] + 0.6 * np.random.randn(n, d)).astype(np.float32)
qs = (cent[np.random.randint(150, size=nq0)] + 0.6 * np.random.randn(nq0, d)).astype(np.float32)
ivf = IVF("euclidean", 160, FastPQ(2))
ivf.fit(X[:15000]).build(X, n_probes=1)
ox = reference_index(ivf)
qn0, qp0 = ivf._prepare(qs.copy())
k, n_probes = 10, 100
tags = ts.assignments(ivf.ids[:len(ivf.active_centers)], n, 3)["some"]
ivf.set_tags(tags)
dev = ivf.device_index()
ms = dev.max_sub_batch(k, n_probes)
sel = np.arange(2 * ms + 5) % nq0                    # three parts
part = (len(sel) + 2) // 3
assert len(sel) > 2 * ms and part % nq0 != 0         # row i of a part has another mask than row i of the call
sample = np.unique(np.concatenate([np.arange(8), part + np.arange(-4, 4), 2 * part + np.arange(-4, 4),
                                   len(sel) - 1 - np.arange(4)]))
for mode, depth in (("any", 1), ("all", 3)):      # (the parts do not depend on the mode: one depth each)
    masks0 = ts.query_masks(tags, nq0, 4 + ts.MODES.index(mode))
    want0 = tagged_batch(oracle, ox, qn0, masks0, mode, tags, k, n_probes)
    assert (want0[1:] != want0[:-1]).any()
    dev.set_pipeline(depth)
    got = dev.query_batch(qn0[sel], qp0[sel], k, n_probes, tags=masks0[sel], tags_mode=mode)
    assert np.array_equal(got[sample], want0[sel][sample]), ("sampled rows differ", mode, depth)
    assert np.array_equal(got, want0[sel]), ("rows differ", mode, depth, np.flatnonzero((got != want0[sel]).any(axis=1))[:5])
assert dev.tag_table()["builds"] == 1
print("ok", ms, len(sel))
'''


def test_batch_beyond_one_workspace(tk):
    env = dict(os.environ, TINYKNN_WORKSPACE_GB="0.25")
    r = subprocess.run([sys.executable, "-c", SUB_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("kp", [1, 2])
def test_after_add_remove_and_update(tk, oracle, kp):
    from test_remove_gpu import SEED, SIGMA, _fitted, _host_index, _oracle_of, _queries
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import synth_rows
    d, N0 = 100, 3000
    ivf = _host_index("angular", d, kp, N=N0)
    dev = ivf.device_index()
    qn, qp = _queries(ivf, d, 96)
    rng = np.random.default_rng(kp)
    # tags 0 .. 4 and 40 .. 43 on the old rows; 50: carried by the added rows only, 60: by the updated rows only
    tags = (ts.bit(0) << rng.integers(0, 5, N0).astype(U64)) | (ts.bit(40) << rng.integers(0, 4, N0).astype(U64))
    pool = np.array([0, ts.bit(2), ts.bit(41), ts.bit(50), ts.bit(60), ts.bit(1) | ts.bit(42), ts.bit(3) | ts.bit(50)],
                    dtype=U64)
    masks = pool[rng.integers(0, len(pool), len(qn))]
    ivf.set_tags(tags)

    def check(builds, mode):
        want, wd = tagged_batch(oracle, _oracle_of(oracle, ivf), qn, masks, mode, ivf.tags, 10, 5, debug=True)
        got, gd = dev.query_batch(qn, qp, 10, 5, debug=True, tags=masks, tags_mode=mode)
        _same(got, gd, want, wd, (builds, mode))
        _within_tags(got, masks, mode, ivf.tags)
        assert dev.tag_table()["built"] and dev.tag_table()["builds"] == builds
        return got
    before = check(1, "any")
    check(1, "all")
    assert (before[masks == ts.bit(50)] == -1).all()
    # add without tags=: refused before anything changes
    new = synth_rows(500, d, SEED, _fitted("angular", d)[2], SIGMA, row0=N0)
    with pytest.raises(ValueError, match="tags"):
        ivf.add(new)
    assert dev.N == N0 and dev.tags_set() == N0
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, tags=masks), before)
    # add: the tags are set again for all rows, the table is made again for the new lists
    ivf.add(new, tags=np.where(rng.random(500) < 0.5, ts.bit(50), ts.bit(2) | ts.bit(50)))
    assert ivf.device_index() is dev and dev.N == N0 + 500 and dev.tags_set() == N0 + 500
    assert len(ivf.tags) == N0 + 500 and not dev.tag_table()["built"]
    after = check(2, "any")
    check(2, "all")
    assert (after[masks == ts.bit(50)] >= N0).any() and (after != before).any()
    # remove: ids are stable, nothing to set; the table is made again for the compacted lists
    dead = np.concatenate([after[:, 0][after[:, 0] >= 0], rng.choice(N0, 300, replace=False)])
    ivf.remove(dead)
    assert dev.tags_set() == N0 + 500 and not dev.tag_table()["built"]
    gone = check(3, "any")
    check(3, "all")
    assert not np.isin(gone, dead).any()
    # update without tags=: new vectors, the rows keep their tags; the table follows the new lists
    live = np.setdiff1d(np.arange(N0), dead)
    ids = rng.choice(live, 200, replace=False)
    kept = ivf.tags.copy()
    ivf.update(ids, synth_rows(200, d, SEED + 3, _fitted("angular", d)[2], SIGMA))
    np.testing.assert_array_equal(ivf.tags, kept)
    assert dev.tags_set() == N0 + 500 and not dev.tag_table()["built"]
    moved = check(4, "any")
    check(4, "all")
    assert (moved != gone).any()
    # update with tags=: those rows carry tag 60 now, and nothing else does
    ivf.update(ids[:100], synth_rows(100, d, SEED + 4, _fitted("angular", d)[2], SIGMA), tags=np.full(100, ts.bit(60)))
    assert (ivf.tags[ids[:100]] == ts.bit(60)).all() and not dev.tag_table()["built"]
    last = check(5, "any")
    check(5, "all")
    sixty = last[masks == ts.bit(60)]
    assert (sixty != -1).any() and np.isin(sixty[sixty != -1], ids[:100]).all()
    # at the ABI, rows added without the tags being set again (the host copy forgotten, so that add() neither asks
    # for tags nor sets them): TK_ERR_STATE, nothing run; a call without a tag array is served
    del ivf.tags
    ivf.add(synth_rows(100, d, SEED, _fitted("angular", d)[2], SIGMA, row0=N0 + 500))
    assert dev.N == N0 + 600 and dev.tags_set() == N0 + 500
    with pytest.raises(_lib.TinyKnnHipError, match="set them again"):
        dev.query_batch(qn, qp, 10, 5, tags=masks)
    assert dev.tag_table()["builds"] == 5
    dev.query_batch(qn, qp, 10, 5)


def test_plain_state_untouched_and_mode_two_identical(tk, synthetic):
    ivf, ox, qn, qp, tags, wants = synthetic(1)
    dev = ivf.device_index()
    dev.set_plain_scan(True)
    for _ in range(4):              # the unrestricted traffic settles the automatic state
        dev.query_batch(qn, qp, 10, 10)
    before = dev.plain_stats()["state"], dev.plain_stats()["pause_left"]
    for mode in ts.MODES:
        masks, want, wd = wants[mode]
        for _ in range(20):
            got = dev.query_batch(qn, qp, 10, 10, tags=masks, tags_mode=mode)
        np.testing.assert_array_equal(got, want)
        st = dev.plain_stats()
        assert (st["state"], st["pause_left"]) == before, (st, before)
    try:
        dev.set_plain_scan("always")
        for mode in ts.MODES:
            masks, want, wd = wants[mode]
            got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, tags=masks, tags_mode=mode)
            assert dev.plain_stats()["plain_units"] > 0
            _same(got, gd, want, wd, ("mode 2", mode))
    finally:
        dev.set_plain_scan(True)


def test_refusals_and_no_table_without_a_tag_array(tk):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    from tinyknn_amd.multi_gpu import shard_lists
    g = golden("g6_ivf_an100.npz")
    ivf = fixture_ivf(g)
    dev = ivf.device_index()
    qn, qp, N = g["qn"], g["qpq"], len(g["data"])
    nq = len(qn)
    out = np.zeros((nq, 10), dtype=np.int64)

    def ex4(d, masks, mode=0):
        m = np.ascontiguousarray(masks, dtype=U64)
        return _lib.lib().tk_index_query_batch_ex4(
            d.handle, None, None, None, m.ctypes.data, mode, _lib.ptr(np.ascontiguousarray(qn), _lib._f32p),
            qp.ctypes.data, 0, nq, 10, 5, 0, _lib.ptr(out, _lib._i64p), None, None, None, None)
    plain = dev.query_batch(qn, qp, 10, 5)
    some = np.ones(nq, dtype=U64)
    # a tagged call while no tags are set: TK_ERR_STATE (-3), nothing run; all 0 is no tag array at all
    out[:] = -9
    assert ex4(dev, some) == -3 and (out == -9).all()
    with pytest.raises(_lib.TinyKnnHipError, match="no tags"):
        dev.query_batch(qn, qp, 10, 5, tags=some)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, tags=0), plain)
    assert ex4(dev, np.zeros(nq, dtype=U64)) == 0
    np.testing.assert_array_equal(out, plain)
    # set_tags: a wrong length (the library's own check, and the Python layer's)
    bad = np.zeros(N - 1, dtype=U64)
    assert _lib.lib().tk_index_set_tags(dev.handle, bad.ctypes.data, N - 1) == -1
    assert dev.tags_set() == 0
    with pytest.raises(ValueError):
        ivf.set_tags(np.zeros(N + 1, dtype=np.int64))
    with pytest.raises(ValueError):
        dev.set_tags(np.full(N, -1))
    # tags set: a call without tags= returns the unrestricted rows and makes no table
    tags = ts.bit(0) << (np.arange(N) % 3 * 31).astype(U64)         # tags 0, 31, 62
    ivf.set_tags(tags)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5), plain)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, debug=True)[0], plain)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, tags=np.zeros(nq, dtype=U64), tags_mode="all"), plain)
    assert dev.tag_table() == dict(built=False, bytes=0, builds=0, row_bytes=8 * N)
    # a bad mode: refused by the library (TK_ERR_ARG) and by the Python layer, nothing run, no table made
    out[:] = -9
    for mode in (2, -1):
        assert ex4(dev, some, mode) == -1 and "tag_mode" in _lib.lib().tk_last_error().decode()
    assert (out == -9).all() and dev.tag_table()["builds"] == 0
    with pytest.raises(ValueError, match="tags_mode"):
        dev.query_batch(qn, qp, 10, 5, tags=some, tags_mode="every")
    with pytest.raises(NotImplementedError):
        ivf.query_batch(np.array(qn, copy=True), 10, n_probes=5, fast=True, tags=1)
    with pytest.raises(ValueError):
        ivf.add(np.zeros((3, qn.shape[1]), np.float32))
    assert dev.tag_table()["builds"] == 0
    # one real entry: only that query changes
    one = np.zeros(nq, dtype=U64)
    one[0] = ts.bit(0) << U64((int(plain[0, 0]) % 3 + 1) % 3 * 31)      # a tag the unrestricted best row does not carry
    got = dev.query_batch(qn, qp, 10, 5, tags=one)
    np.testing.assert_array_equal(got[1:], plain[1:])
    assert plain[0, 0] not in got[0] and dev.tag_table()["builds"] == 1
    # cleared: tagged calls are refused again
    ivf.set_tags(None)
    assert dev.tags_set() == 0 and not dev.tag_table()["built"]
    assert ex4(dev, one) == -3
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5), plain)
    # a list-sharded index
    owner = shard_lists(np.asarray(g["list_sizes"], dtype=np.int64), 2)
    shard = DeviceIndex(fixture_ivf(g), owner, 0, 2)
    try:
        assert _lib.lib().tk_index_set_tags(shard.handle, tags.ctypes.data, N) == -1
        assert "list-sharded" in _lib.lib().tk_last_error().decode()
        with pytest.raises(RuntimeError, match="list-sharded"):
            shard.set_tags(tags)
        with pytest.raises(AssertionError, match="list-sharded"):
            _lib.check(ex4(shard, one))
    finally:
        shard.close()


def test_tags_leave_with_their_rows(tk):
    """build_resident drops the tags of the rows before it, as build does."""
    from tinyknn_amd import IVF, FastPQ, _lib
    X = np.random.default_rng(3).standard_normal((3000, 32)).astype(np.float32)
    ivf = IVF("euclidean", 12, FastPQ(2))
    ivf.fit(X).build(X, n_probes=1)
    ivf.set_tags(np.arange(3000) % 4)
    assert ivf.device_index().tags_set() == 3000
    ivf.build_resident(2000, 32, 7)
    dev = ivf.device_index()
    assert ivf.tags is None and dev.N == 2000 and dev.tags_set() == 0
    qn, qp = ivf._prepare(X[:8].copy())
    plain = dev.query_batch(qn, qp, 5, 3)
    with pytest.raises(_lib.TinyKnnHipError, match="no tags"):
        dev.query_batch(qn, qp, 5, 3, tags=1)
    ivf.set_tags(np.ones(2000, dtype=np.int64))
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 5, 3, tags=1, tags_mode="all"), plain)
