"""Row groups on the device (groups.hip: tk_index_set_groups, tk_index_query_batch[_dev]_ex3; IVF.set_groups,
group=).  Every comparison is exact: ids and, through debug=True, probes and heap arrays against
tests/groups_reference.py — per query the guarded reference with the allowed set `groups == g`."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from allowed_reference import guarded_batch, reference_index  # noqa: E402
from conftest import G6_TAGS, golden  # noqa: E402
from groups_reference import grouped_batch  # noqa: E402
from store_reference import exact_distances, fixture_ivf, oracle_index, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("probes", "heap_idx", "heap_val")
ABSENT = 2**31 - 2      # the largest group id: no test row carries it


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


def _within_groups(got, group, groups):
    for i, g in enumerate(group):
        ids = got[i][got[i] != -1]
        if g >= 0:
            assert (groups[ids] == g).all(), (i, g)


def _first_list(ids_per_list, N):
    """the (lowest) list every row is stored in, -1 -> 0 for a row stored nowhere"""
    first = np.zeros(N, dtype=np.int32)
    for l in reversed(range(len(ids_per_list))):
        first[np.asarray(ids_per_list[l], dtype=np.int64)] = l
    return first


def _assignments(ivf, N, seed):
    return dict(one=np.full(N, 5, dtype=np.int32),
                seven=np.random.default_rng(seed).integers(0, 7, N).astype(np.int32),
                lists=_first_list(ivf.ids[:len(ivf.active_centers)], N),
                own=np.arange(N, dtype=np.int32))


def _query_groups(groups, nq, seed):
    """drawn from the groups present, -1 for every fourth query, one id no row carries"""
    rng = np.random.default_rng(seed)
    q = rng.choice(np.unique(groups), nq).astype(np.int32)
    q[1::4] = -1
    q[2] = ABSENT
    return q


@pytest.mark.parametrize("tag", G6_TAGS)
def test_fixtures_every_probe_count_and_assignment(tk, oracle, tag):
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = fixture_ivf(g)
    ox = oracle_index(oracle, ivf, g["data"])
    dev = ivf.device_index()
    qn, qp, N = g["qn"], g["qpq"], len(g["data"])
    nq = len(qn)
    assert dev.groups_set() == 0 and dev.group_table()["builds"] == 0
    for a, (name, groups) in enumerate(_assignments(ivf, N, 3).items()):
        ivf.set_groups(groups)
        assert dev.groups_set() == N and not dev.group_table()["built"]
        for n_probes in (1, 2, 5, 10):
            group = _query_groups(groups, nq, 10 * n_probes + a)
            want, wd = grouped_batch(oracle, ox, qn, group, groups, 10, n_probes, debug=True)
            got, gd = dev.query_batch(qn, qp, 10, n_probes, debug=True, group=group)
            _same(got, gd, want, wd, (name, n_probes))
            _within_groups(got, group, groups)
            assert (got[2] == -1).all()         # a group no row carries: no id
            # all -1: the unrestricted call; one group everywhere (an int): allowed=(groups == g)
            plain = dev.query_batch(qn, qp, 10, n_probes, debug=True)
            _same(*dev.query_batch(qn, qp, 10, n_probes, debug=True, group=np.full(nq, -1)), *plain, (name, "all -1"))
            g0 = int(group[0])
            _same(*dev.query_batch(qn, qp, 10, n_probes, debug=True, group=g0),
                  *dev.query_batch(qn, qp, 10, n_probes, debug=True, allowed=groups == g0), (name, "one group"))
        assert dev.group_table()["builds"] == a + 1     # one table per set_groups, whatever the calls
    t = dev.group_table()
    assert t["built"] and t["row_bytes"] == 4 * N
    assert t["bytes"] == 64 * int(((np.asarray(g["list_sizes"], dtype=np.int64) + 15) // 16).sum())


def test_ivf_query_and_query_batch(tk, oracle):
    g = golden("g6_ivf_an100.npz")
    ivf = fixture_ivf(g)
    ox = oracle_index(oracle, ivf, g["data"])
    N = len(g["data"])
    groups = np.random.default_rng(5).integers(0, 40, N).astype(np.int32)
    ivf.set_groups(groups)          # (before the device index exists: uploaded when it is made)
    qs = np.array(g["qn"], copy=True)
    qn = ivf._prepare(qs.copy())[0]
    group = _query_groups(groups, len(qs), 1)
    want = grouped_batch(oracle, ox, qn, group, groups, 10, 5)
    np.testing.assert_array_equal(ivf.query_batch(qs, 10, n_probes=5, group=group), want)
    assert ivf.device_index().groups_set() == N
    lengths = []
    for i in range(len(qs)):
        q1 = ivf._prepare(qs[i:i + 1].copy())[0]
        w = grouped_batch(oracle, ox, q1, group[i:i + 1], groups, 10, 5)[0]
        got = ivf.query(qs[i].copy(), 10, n_probes=5, group=int(group[i]))
        np.testing.assert_array_equal(got, w[w != -1] if w[-1] == -1 else w)
        lengths.append(len(got))
    assert lengths[2] == 0 and min(lengths[3:]) < 10        # the absent group; the early return (ivf.py:154-156)
    np.testing.assert_array_equal(ivf.query(qs[0].copy(), 10, n_probes=5, group=-1), ivf.query(qs[0].copy(), 10, n_probes=5))


# ---- every replay form: the synthetic index of test_rows_gpu.py, built with n_probes 1 and 2 ----

SYN_N, SYN_D, SYN_NQ = 40000, 48, 256


@pytest.fixture(scope="module")
def synthetic(tk, oracle):
    np.random.seed(5)
    cent = np.random.randn(150, SYN_D)
    X = (cent[np.random.randint(150, size=SYN_N)] + 0.6 * np.random.randn(SYN_N, SYN_D)).astype(np.float32)
    qs = (cent[np.random.randint(150, size=SYN_NQ)] + 0.6 * np.random.randn(SYN_NQ, SYN_D)).astype(np.float32)
    base = tk.IVF("euclidean", 160, tk.FastPQ(2, rotate_dim=None))      # unrotated: the reference is fed qn
    base.fit(X[:15000])
    assert base.pq.R is None
    groups = np.random.default_rng(8).integers(0, 7, SYN_N).astype(np.int32)
    group = _query_groups(groups, SYN_NQ, 9)
    made = {}

    def get(kp):
        if kp not in made:
            ivf = tk.IVF("euclidean", 160, None)
            ivf.all_centers, ivf.pq = base.all_centers, base.pq
            ivf.build(X, n_probes=kp)
            ivf.set_groups(groups)
            ox = reference_index(ivf)
            qn, qp = ivf._prepare(qs.copy())
            want = grouped_batch(oracle, ox, qn, group, groups, 10, 10, debug=True)
            made[kp] = (ivf, ox, qn, qp, want)
        return made[kp]
    return get, groups, group


@pytest.mark.parametrize("kp", [1, 2])
def test_every_replay_form(tk, synthetic, kp):
    from tinyknn_amd import _lib
    get, groups, group = synthetic
    ivf, ox, qn, qp, (want, wd) = get(kp)
    dev = ivf.device_index()
    assert (kp == 1) == (dev.twin_table_width() == 0)
    try:
        for heap_mode in (0, 1, 2, 3):
            for plain in (False, "always"):
                for pair_nq in (4, 8192):
                    dev.set_heap_mode(heap_mode)
                    dev.set_plain_scan(plain)
                    dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
                    got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, group=group)
                    _same(got, gd, want, wd, (kp, heap_mode, plain, pair_nq))
        _within_groups(got, group, groups)
        # the limit at -128: every query with a plain list fails the lemma's check, is scanned again exactly and masked
        # again through the flag list (the passes' `only` branch)
        dev.set_heap_mode(0)
        dev.set_plain_scan("always")
        dev.set_option(_lib.OPT_PLAIN_LIMIT, -128)
        for pair_nq in (4, 8192):
            dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
            got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, group=group)
            st = dev.plain_stats()
            _same(got, gd, want, wd, (kp, "limit -128", pair_nq, st))
            assert st["plain_units"] > 0 and st["flagged_queries"] > 0, st
        assert dev.group_table()["builds"] == 1
    finally:
        dev.set_heap_mode(0); dev.set_plain_scan(True); dev.set_option(_lib.OPT_PAIR_NQ, 4)
        dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)


def test_with_an_allowed_set_an_excluded_row_and_distances(tk, oracle, synthetic):
    from tinyknn_amd import _lib
    get, groups, group = synthetic
    ivf, ox, qn, qp, (want, _) = get(1)
    dev = ivf.device_index()
    allowed = np.random.default_rng(3).random(SYN_N) < 0.3
    exclude = want[:, 0].copy()             # every query's best id (or -1) may not come back
    assert (exclude >= 0).sum() > SYN_NQ // 2
    aset = dev.allow(allowed)
    legs = [(name, kw, grouped_batch(oracle, ox, qn, group, groups, 10, 10, debug=True, **ref))
            for name, kw, ref in (("allowed", dict(allowed=aset), dict(allowed=allowed)),
                                  ("exclude", dict(exclude=exclude), dict(exclude=exclude)),
                                  ("all three", dict(allowed=aset, exclude=exclude), dict(allowed=allowed, exclude=exclude)))]
    try:
        # ("forced": pinned on with the limit at -128 — every query with a plain list is flagged, scanned again exactly
        #  and masked again by all three passes through the flag list)
        for plain in (False, "always", "forced"):
            dev.set_plain_scan("always" if plain == "forced" else plain)
            dev.set_option(_lib.OPT_PLAIN_LIMIT, -128 if plain == "forced" else 0x7fffffff)
            for name, kw, (w, wdbg) in legs:
                got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, group=group, **kw)
                _same(got, gd, w, wdbg, (name, plain))
                if plain == "forced":
                    st = dev.plain_stats()
                    assert st["plain_units"] > 0 and st["flagged_queries"] > 0, (name, st)
                _within_groups(got, group, groups)
                if "exclude" in kw:
                    assert not (got == np.where(exclude >= 0, exclude, -2)[:, None]).any()
                if "allowed" in kw:
                    assert allowed[got[got != -1]].all()
        dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
        dev.set_plain_scan(True)
        # distances: the ids of the plain grouped call, each with the rescoring's exact distance
        ids, dist = dev.query_batch(qn, qp, 10, 10, group=group, return_distances=True)
        np.testing.assert_array_equal(ids, want)
        assert same_bits(dist, exact_distances(oracle, qn, ivf.data, ids))
        ids, dist = dev.query_batch(qn, qp, 10, 10, group=group, allowed=aset, exclude=exclude, return_distances=True)
        np.testing.assert_array_equal(ids, w)
        assert same_bits(dist, exact_distances(oracle, qn, ivf.data, ids))
    finally:
        dev.set_plain_scan(True)
        dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
        aset.close()
    # the index built with n_probes = 2 (labels repeat: the TWIN form): the allow pass alone and all three passes behind
    # its flagged re-scan
    ivf2, ox2, qn2, qp2, (want2, _) = get(2)
    dev2 = ivf2.device_index()
    exclude2 = want2[:, 0].copy()
    aset2 = dev2.allow(allowed)
    try:
        dev2.set_plain_scan("always")
        dev2.set_option(_lib.OPT_PLAIN_LIMIT, -128)
        for name, kw, ref in (("allowed", dict(allowed=aset2), dict(allowed=allowed)),
                              ("all three", dict(allowed=aset2, exclude=exclude2, group=group),
                               dict(allowed=allowed, exclude=exclude2))):
            w2, wd2 = grouped_batch(oracle, ox2, qn2, group if "group" in kw else -1, groups, 10, 10, debug=True, **ref)
            got, gd = dev2.query_batch(qn2, qp2, 10, 10, debug=True, **kw)
            st = dev2.plain_stats()
            _same(got, gd, w2, wd2, (2, name, "forced", st))
            assert st["plain_units"] > 0 and st["flagged_queries"] > 0, (name, st)
            assert allowed[got[got != -1]].all()
    finally:
        dev2.set_plain_scan(True)
        dev2.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
        aset2.close()


def test_pipelined_pairs_alternating_kinds(tk, oracle, synthetic):
    """Twelve device calls in pairs.  A device array is not read on the host: its entries < -1 leave their queries
    unrestricted, as -1 does (group_pass_kernel returns for every g < 0)."""
    import torch
    get, groups, group = synthetic
    ivf, ox, qn, qp, (want_g, _) = get(1)
    dev = ivf.device_index()
    other = np.roll(group, 7)
    negative = group.copy()
    negative[0::3] = -5
    negative[1::6] = np.iinfo(np.int32).min
    allowed = np.random.default_rng(3).random(SYN_N) < 0.3
    exclude = want_g[:, 0].copy()
    want = dict(g=want_g, none=guarded_batch(oracle, ox, qn, 10, 10),
                g_other=grouped_batch(oracle, ox, qn, other, groups, 10, 10),
                g_allow=grouped_batch(oracle, ox, qn, group, groups, 10, 10, allowed=allowed),
                g_ex=grouped_batch(oracle, ox, qn, group, groups, 10, 10, exclude=exclude),
                g_neg=grouped_batch(oracle, ox, qn, np.where(negative < 0, -1, negative), groups, 10, 10))
    assert (want["g_neg"] != want_g).any()
    aset = dev.allow(allowed)
    alone = dict(g=dev.query_batch(qn, qp, 10, 10, group=group), none=dev.query_batch(qn, qp, 10, 10),
                 g_other=dev.query_batch(qn, qp, 10, 10, group=other),
                 g_allow=dev.query_batch(qn, qp, 10, 10, group=group, allowed=aset),
                 g_ex=dev.query_batch(qn, qp, 10, 10, group=group, exclude=exclude))
    # (pairs: two arrays; an exclude array on one half; none at all; an array with negative entries.  Alone: a grouped call
    #  next to an ungrouped one, or next to one with another allowed set)
    kinds = ["g", "g_other", "none", "g_allow", "g_ex", "g", "none", "none", "g_ex", "g_neg", "g_allow", "none"]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    qn_d, qp_d, ex_d = cuda(qn), cuda(qp), cuda(exclude)
    arrays = dict(g=cuda(group), g_other=cuda(other), g_allow=cuda(group), g_ex=cuda(group), g_neg=cuda(negative))
    outs = [torch.full((SYN_NQ, 10), -7, dtype=torch.int64, device="cuda") for _ in kinds]
    try:
        dev.set_pipeline(3)
        dev.set_coalesce(2)
        torch.cuda.synchronize()
        for kind, out in zip(kinds, outs):
            dev.query_batch_dev(qn_d.data_ptr(), qp_d.data_ptr(), 0, SYN_NQ, 10, 10, out.data_ptr(),
                                allowed=aset if kind == "g_allow" else None,
                                exclude_ptr=ex_d.data_ptr() if kind == "g_ex" else None,
                                group_ptr=arrays[kind].data_ptr() if kind in arrays else None)
        dev.join()
        torch.cuda.synchronize()
        for i, (kind, out) in enumerate(zip(kinds, outs)):
            got = out.cpu().numpy()
            np.testing.assert_array_equal(got, want[kind], err_msg=f"call {i} {kind}")
            if kind in alone:
                np.testing.assert_array_equal(got, alone[kind], err_msg=f"call {i} {kind} alone")
    finally:
        dev.set_pipeline(1)
        dev.set_coalesce(1)
        aset.close()


SUB_CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from tinyknn_amd import IVF, FastPQ, _lib
from oracle import oracle
from allowed_reference import reference_index
from groups_reference import grouped_batch
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
groups = np.random.default_rng(3).integers(0, 7, n).astype(np.int32)
group0 = np.random.default_rng(4).integers(-1, 7, nq0).astype(np.int32)
want0 = grouped_batch(oracle, ox, qn0, group0, groups, k, n_probes)
ivf.set_groups(groups)
dev = ivf.device_index()
ms = dev.max_sub_batch(k, n_probes)
sel = np.arange(2 * ms + 5) % nq0                    # three parts
part = (len(sel) + 2) // 3
assert len(sel) > 2 * ms and part % nq0 != 0         # row i of a part has another group than row i of the call
for depth in (1, 3):
    dev.set_pipeline(depth)
    got = dev.query_batch(qn0[sel], qp0[sel], k, n_probes, group=group0[sel])
    assert np.array_equal(got, want0[sel]), ("rows differ", depth, np.flatnonzero((got != want0[sel]).any(axis=1))[:5])
assert dev.group_table()["builds"] == 1
print("ok", ms, len(sel))
'''


def test_batch_beyond_one_workspace(tk):
    env = dict(os.environ, TINYKNN_WORKSPACE_GB="0.25")
    r = subprocess.run([sys.executable, "-c", SUB_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("kp", [1, 2])
def test_after_add_and_after_remove(tk, oracle, kp):
    from test_remove_gpu import SEED, SIGMA, _fitted, _host_index, _oracle_of, _queries
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import synth_rows
    d, N0 = 100, 3000
    ivf = _host_index("angular", d, kp, N=N0)
    dev = ivf.device_index()
    qn, qp = _queries(ivf, d, 96)
    rng = np.random.default_rng(kp)
    groups = rng.integers(0, 5, N0).astype(np.int32)
    group = rng.integers(-1, 6, len(qn)).astype(np.int32)       # (5: carried by the added rows only)
    ivf.set_groups(groups)

    def check(builds):
        want, wd = grouped_batch(oracle, _oracle_of(oracle, ivf), qn, group, ivf.groups, 10, 5, debug=True)
        got, gd = dev.query_batch(qn, qp, 10, 5, debug=True, group=group)
        _same(got, gd, want, wd, builds)
        _within_groups(got, group, ivf.groups)
        assert dev.group_table()["built"] and dev.group_table()["builds"] == builds
        return got
    before = check(1)
    assert (before[group == 5] == -1).all()
    # add without groups=: refused before anything changes
    new = synth_rows(500, d, SEED, _fitted("angular", d)[2], SIGMA, row0=N0)
    with pytest.raises(ValueError, match="groups"):
        ivf.add(new)
    assert dev.N == N0 and dev.groups_set() == N0
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, group=group), before)
    # add: the groups are set again for all rows, the table is made again for the new lists
    ivf.add(new, groups=rng.integers(0, 6, 500))
    assert ivf.device_index() is dev and dev.N == N0 + 500 and dev.groups_set() == N0 + 500
    assert len(ivf.groups) == N0 + 500 and not dev.group_table()["built"]
    after = check(2)
    assert (after[group == 5] >= N0).any() and (after != before).any()
    # remove: ids are stable, nothing to set; the table is made again for the compacted lists
    dead = np.concatenate([after[:, 0][after[:, 0] >= 0], rng.choice(N0, 300, replace=False)])
    ivf.remove(dead)
    assert dev.groups_set() == N0 + 500 and not dev.group_table()["built"]
    gone = check(3)
    assert not np.isin(gone, dead).any()
    # at the ABI, rows added without the groups being set again (the host copy forgotten, so that add() neither asks
    # for groups nor sets them): TK_ERR_STATE, nothing run; a call without a group array is served
    del ivf.groups
    ivf.add(synth_rows(100, d, SEED, _fitted("angular", d)[2], SIGMA, row0=N0 + 500))
    assert dev.N == N0 + 600 and dev.groups_set() == N0 + 500
    with pytest.raises(_lib.TinyKnnHipError, match="set them again"):
        dev.query_batch(qn, qp, 10, 5, group=group)
    assert dev.group_table()["builds"] == 3
    dev.query_batch(qn, qp, 10, 5)


def test_plain_state_untouched_by_grouped_calls(tk, synthetic):
    get, groups, group = synthetic
    ivf, ox, qn, qp, (want, _) = get(1)
    dev = ivf.device_index()
    dev.set_plain_scan(True)
    for _ in range(4):              # the unrestricted traffic settles the automatic state
        dev.query_batch(qn, qp, 10, 10)
    before = dev.plain_stats()["state"], dev.plain_stats()["pause_left"]
    for _ in range(40):
        got = dev.query_batch(qn, qp, 10, 10, group=group)
    np.testing.assert_array_equal(got, want)
    st = dev.plain_stats()
    assert (st["state"], st["pause_left"]) == before, (st, before)


def test_refusals_and_no_table_without_a_group_array(tk):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    from tinyknn_amd.multi_gpu import shard_lists
    g = golden("g6_ivf_an100.npz")
    ivf = fixture_ivf(g)
    dev = ivf.device_index()
    qn, qp, N = g["qn"], g["qpq"], len(g["data"])
    nq = len(qn)
    out = np.zeros((nq, 10), dtype=np.int64)

    def ex3(d, group):
        gr = np.ascontiguousarray(group, dtype=np.int32)
        return _lib.lib().tk_index_query_batch_ex3(
            d.handle, None, None, gr.ctypes.data, _lib.ptr(np.ascontiguousarray(qn), _lib._f32p), qp.ctypes.data, 0,
            nq, 10, 5, 0, _lib.ptr(out, _lib._i64p), None, None, None, None)
    plain = dev.query_batch(qn, qp, 10, 5)
    some = np.zeros(nq, dtype=np.int32)
    # a grouped call while no groups are set: TK_ERR_STATE (-3), nothing run; all -1 is no group array at all
    out[:] = -9
    assert ex3(dev, some) == -3 and (out == -9).all()
    with pytest.raises(_lib.TinyKnnHipError, match="no groups"):
        dev.query_batch(qn, qp, 10, 5, group=some)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, group=-1), plain)
    # set_groups: a wrong length, an id out of range (the library's own checks, and the Python layer's)
    bad = np.zeros(N - 1, dtype=np.int32)
    assert _lib.lib().tk_index_set_groups(dev.handle, _lib.ptr(bad, _lib._i32p), N - 1) == -1
    neg = np.zeros(N, dtype=np.int32)
    neg[N // 2] = -1
    assert _lib.lib().tk_index_set_groups(dev.handle, _lib.ptr(neg, _lib._i32p), N) == -1
    neg[N // 2] = 2**31 - 1
    assert _lib.lib().tk_index_set_groups(dev.handle, _lib.ptr(neg, _lib._i32p), N) == -1
    assert dev.groups_set() == 0
    with pytest.raises(ValueError):
        ivf.set_groups(np.zeros(N + 1, dtype=np.int64))
    with pytest.raises(ValueError):
        dev.set_groups(np.zeros(N - 1, dtype=np.int64))
    # groups set: a call without group= returns the unrestricted rows and makes no table
    groups = (np.arange(N) % 3).astype(np.int32)
    ivf.set_groups(groups)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5), plain)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, debug=True)[0], plain)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, group=np.full(nq, -1)), plain)
    assert dev.group_table() == dict(built=False, bytes=0, builds=0, row_bytes=4 * N)
    # a host-side query group below -1: refused by the library, nothing run
    out[:] = -9
    some[nq // 2] = -2
    with pytest.raises(AssertionError, match="group"):
        _lib.check(ex3(dev, some))
    assert (out == -9).all() and dev.group_table()["builds"] == 0
    with pytest.raises(NotImplementedError):
        ivf.query_batch(np.array(qn, copy=True), 10, n_probes=5, fast=True, group=1)
    with pytest.raises(ValueError):
        ivf.add(np.zeros((3, qn.shape[1]), np.float32))
    # one real entry: only that query changes
    one = np.full(nq, -1, dtype=np.int32)
    one[0] = (groups[plain[0, 0]] + 1) % 3
    got = dev.query_batch(qn, qp, 10, 5, group=one)
    np.testing.assert_array_equal(got[1:], plain[1:])
    assert plain[0, 0] not in got[0] and dev.group_table()["builds"] == 1
    # cleared: grouped calls are refused again
    ivf.set_groups(None)
    assert dev.groups_set() == 0 and not dev.group_table()["built"]
    assert ex3(dev, one) == -3
    # a list-sharded index
    owner = shard_lists(np.asarray(g["list_sizes"], dtype=np.int64), 2)
    shard = DeviceIndex(fixture_ivf(g), owner, 0, 2)
    try:
        assert _lib.lib().tk_index_set_groups(shard.handle, _lib.ptr(groups, _lib._i32p), N) == -1
        assert "list-sharded" in _lib.lib().tk_last_error().decode()
        with pytest.raises(RuntimeError, match="list-sharded"):
            shard.set_groups(groups)
        with pytest.raises(AssertionError, match="list-sharded"):
            _lib.check(ex3(shard, one))
    finally:
        shard.close()


def test_groups_leave_with_their_rows_and_stay_when_a_sharded_index_refuses(tk):
    """build_resident drops the groups of the rows before it, as build does; set_groups(None) on an index that has
    been list-sharded raises before the host copy changes."""
    from tinyknn_amd import IVF, FastPQ, _lib
    from tinyknn_amd.ivf import DeviceIndex
    from tinyknn_amd.multi_gpu import shard_lists
    X = np.random.default_rng(3).standard_normal((3000, 32)).astype(np.float32)
    ivf = IVF("euclidean", 12, FastPQ(2))
    ivf.fit(X).build(X, n_probes=1)
    ivf.set_groups(np.arange(3000) % 4)
    assert ivf.device_index().groups_set() == 3000
    ivf.build_resident(2000, 32, 7)
    dev = ivf.device_index()
    assert ivf.groups is None and dev.N == 2000 and dev.groups_set() == 0
    qn, qp = ivf._prepare(X[:8].copy())
    plain = dev.query_batch(qn, qp, 5, 3)
    with pytest.raises(_lib.TinyKnnHipError, match="no groups"):
        dev.query_batch(qn, qp, 5, 3, group=1)
    ivf.set_groups(np.zeros(2000, dtype=np.int64))
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 5, 3, group=0), plain)
    # a list-sharded device index behind an IVF that holds groups
    g = golden("g6_ivf_an100.npz")
    held = fixture_ivf(g)
    groups = (np.arange(len(g["data"])) % 3).astype(np.int32)
    held.set_groups(groups)
    held._dev = DeviceIndex(held, shard_lists(np.asarray(g["list_sizes"], dtype=np.int64), 2), 0, 2)
    try:
        with pytest.raises(RuntimeError, match="list-sharded"):
            held.set_groups(None)
        np.testing.assert_array_equal(held.groups, groups)
    finally:
        held._dev.close()
