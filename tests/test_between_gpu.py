"""Value ranges on the device (between.hip: tk_index_set_values, tk_index_query_batch[_dev]_ex5; IVF.set_values,
between=).  Every comparison is exact: ids and, through debug=True, probes and heap arrays against
tests/between_reference.py — per query the guarded reference with the allowed set the formula gives on the ORIGINAL
values.  The inputs come from tests/between_shapes.py; tests/test_between_cpu.py asserts on the reference alone what
they hold."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import between_shapes as bs  # noqa: E402
import tag_shapes as ts  # noqa: E402
from allowed_reference import guarded_batch  # noqa: E402
from between_reference import bounds_of, passing, ranged_batch  # noqa: E402
from conftest import G6_TAGS, golden  # noqa: E402
from store_reference import exact_distances, fixture_ivf, oracle_index, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("probes", "heap_idx", "heap_val")
INT64_MIN, INT64_MAX = bs.INT64_MIN, bs.INT64_MAX


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


def _within(got, between, values):
    for i, row in enumerate(got):
        assert passing(values, *bounds_of(between, i))[row[row != -1]].all(), i


@pytest.mark.parametrize("tag", G6_TAGS)
def test_fixtures_every_probe_count_and_assignment(tk, oracle, tag):
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = fixture_ivf(g)
    ox = oracle_index(oracle, ivf, g["data"])
    dev = ivf.device_index()
    qn, qp, N = g["qn"], g["qpq"], len(g["data"])
    nq = len(qn)
    assert dev.values_set() == 0 and dev.value_table()["builds"] == 0 and dev.value_table()["cols"] == 0
    chunks = int(((np.asarray(g["list_sizes"], dtype=np.int64) + 15) // 16).sum())
    for a, (name, values) in enumerate(bs.assignments(ivf.ids[:len(ivf.active_centers)], N, 3).items()):
        ivf.set_values(values)
        C = 1 if values.ndim == 1 else values.shape[1]
        assert dev.values_set() == N and not dev.value_table()["built"] and dev.value_table()["cols"] == C
        for n_probes in (1, 2, 5, 10):
            lo, hi, kinds = bs.ranges(values, nq, 10 * n_probes + a)
            between = (lo[:, 0], hi[:, 0]) if C == 1 and n_probes == 2 else (lo, hi)        # (nq,) for one column too
            want, wd = ranged_batch(oracle, ox, qn, (lo, hi), values, 10, n_probes, debug=True)
            got, gd = dev.query_batch(qn, qp, 10, n_probes, debug=True, between=between)
            _same(got, gd, want, wd, (name, n_probes))
            _within(got, (lo, hi), values)
            assert (got[[i for i, kind in enumerate(kinds) if kind == "empty"]] == -1).all()
            # nothing bounded: the unrestricted call; one range everywhere: allowed=(the rows it passes)
            plain = dev.query_batch(qn, qp, 10, n_probes, debug=True)
            _same(*dev.query_batch(qn, qp, 10, n_probes, debug=True, between=(None, None)), *plain, (name, "none"))
            one = (np.tile(lo[0], (nq, 1)), np.tile(hi[0], (nq, 1)))
            _same(*dev.query_batch(qn, qp, 10, n_probes, debug=True, between=one),
                  *dev.query_batch(qn, qp, 10, n_probes, debug=True, allowed=passing(values, lo[0], hi[0])), (name, "one"))
        assert dev.value_table()["builds"] == a + 1         # one table per set_values, whatever the calls
        t = dev.value_table()
        assert t["built"] and t["row_bytes"] == 8 * C * N and t["bytes"] == 128 * C * chunks


@pytest.mark.parametrize("cols", [1, 2, 4])
def test_one_two_and_four_columns_and_ivf_query_is_the_row_of_query_batch(tk, oracle, cols):
    g = golden("g6_ivf_an100.npz")
    ivf = fixture_ivf(g)
    ox = oracle_index(oracle, ivf, g["data"])
    N = len(g["data"])
    rng = np.random.default_rng(cols)
    values = rng.integers(-3, 4, (N, cols)).astype(np.int64) if cols > 1 else rng.integers(-3, 4, N).astype(np.int64)
    ivf.set_values(values)              # (before the device index exists: uploaded when it is made)
    qs = np.array(g["qn"][np.arange(65) % len(g["qn"])], copy=True)     # 65 queries: one more than a wave of lanes
    qn = ivf._prepare(qs.copy())[0]
    lo, hi, kinds = bs.ranges(values, len(qs), 1)
    if cols == 4:                       # every column its own window, the last one-sided; some queries bound column 3 alone
        lo[:, 1:], hi[:, 1:] = rng.integers(-3, 1, (65, 3)), rng.integers(0, 4, (65, 3))
        hi[:, 3] = INT64_MAX
        lo[::5, :3], hi[::5, :3] = INT64_MIN, INT64_MAX
    want = ranged_batch(oracle, ox, qn, (lo, hi), values, 10, 5)
    batch = ivf.query_batch(qs, 10, n_probes=5, between=(lo, hi))
    np.testing.assert_array_equal(batch, want)
    dev = ivf.device_index()
    assert dev.values_set() == N and dev.value_table()["cols"] == cols and dev.value_table()["bytes"] % (128 * cols) == 0
    lengths = []
    for i in range(len(qs)):
        between = (lo[i, 0], hi[i, 0]) if cols == 1 else (lo[i], hi[i])
        got = ivf.query(qs[i].copy(), 10, n_probes=5, between=between)
        w = batch[i]
        np.testing.assert_array_equal(got, w[w != -1] if w[-1] == -1 else w, err_msg=f"query {i}")
        lengths.append(len(got))
    assert min(lengths) == 0 and max(lengths) == 10         # an empty range; a full answer
    np.testing.assert_array_equal(ivf.query(qs[0].copy(), 10, n_probes=5, between=(None, None)),
                                  ivf.query(qs[0].copy(), 10, n_probes=5))
    # a scalar for every query and column; (C,) for every query
    np.testing.assert_array_equal(ivf.query_batch(qs, 10, n_probes=5, between=(0, None)),
                                  ranged_batch(oracle, ox, qn, (np.zeros((65, cols)), None), values, 10, 5))
    if cols > 1:
        np.testing.assert_array_equal(ivf.query_batch(qs, 10, n_probes=5, between=(lo[1], hi[1])),
                                      ranged_batch(oracle, ox, qn, (np.tile(lo[1], (65, 1)), np.tile(hi[1], (65, 1))),
                                                   values, 10, 5))


# ---- every replay form: the synthetic index of tests/tag_shapes.py, built with n_probes 1 and 2, two columns ----

SYN_N, SYN_NQ = bs.SYN_N, bs.SYN_NQ


@pytest.fixture(scope="module")
def synthetic(tk, oracle):
    """get(kp) -> (a copy of the shared index with its values set, ox, qn, qp, values, between, want, debug): every
    reference is computed once and left unchanged"""
    import copy
    made = {}

    def get(kp):
        if kp not in made:
            shared, qs, values, between, _, _ = bs.synthetic(kp)
            ivf = copy.copy(shared)         # (the device index and the values are kept on the copy)
            ivf._dev = None
            ivf.set_values(values)
            ox = oracle_index(oracle, ivf, ivf.data)
            qn, qp = ivf._prepare(qs.copy())
            want, wd = ranged_batch(oracle, ox, qn, between, values, 10, 10, debug=True)
            made[kp] = (ivf, ox, qn, qp, values, between, want, wd)
        return made[kp]
    return get


@pytest.mark.parametrize("kp", [1, 2])
def test_every_replay_form(tk, synthetic, kp):
    from tinyknn_amd import _lib
    ivf, ox, qn, qp, values, between, want, wd = synthetic(kp)
    dev = ivf.device_index()
    assert (kp == 1) == (dev.twin_table_width() == 0)
    builds = dev.value_table()["builds"]
    try:
        for heap_mode, scan_mode in ((0, 0), (1, 1), (2, 2), (0, 2), (3, 0)):
            for plain in (False, "always"):
                for pair_nq in (4, 8192):
                    dev.set_heap_mode(heap_mode)
                    dev.set_scan_mode(scan_mode)
                    dev.set_plain_scan(plain)
                    dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
                    got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, between=between)
                    _same(got, gd, want, wd, (kp, heap_mode, scan_mode, plain, pair_nq))
        _within(got, between, values)
        # the limit at -128: every query with a plain list fails the lemma's check, is scanned again exactly and masked
        # again through the flag list (the pass's `only` branch)
        dev.set_heap_mode(0)
        dev.set_scan_mode(0)
        dev.set_plain_scan("always")
        dev.set_option(_lib.OPT_PLAIN_LIMIT, -128)
        for pair_nq in (4, 8192):
            dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
            got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, between=between)
            st = dev.plain_stats()
            _same(got, gd, want, wd, (kp, "limit -128", pair_nq, st))
            assert st["plain_units"] > 0 and st["flagged_queries"] > 0, st
        assert dev.value_table()["builds"] == max(builds, 1)
    finally:
        dev.set_heap_mode(0); dev.set_scan_mode(0); dev.set_plain_scan(True); dev.set_option(_lib.OPT_PAIR_NQ, 4)
        dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)


def test_all_five_restrictions_and_distances(tk, oracle, synthetic):
    from tinyknn_amd import _lib
    rng = np.random.default_rng(3)
    allowed = rng.random(SYN_N) < 0.6
    groups = rng.integers(0, 2, SYN_N).astype(np.int32)
    group = rng.integers(-1, 2, SYN_NQ).astype(np.int32)
    tags = ts.bit(0) << rng.integers(0, 3, SYN_N).astype(np.uint64)
    masks = np.where(rng.random(SYN_NQ) < 0.5, ts.U64(3), ts.U64(0))
    for kp in (1, 2):
        ivf, ox, qn, qp, values, between, want, _ = synthetic(kp)
        dev = ivf.device_index()
        dev.set_groups(groups)
        dev.set_tags(tags)
        aset = dev.allow(allowed)
        exclude = want[:, 0].copy()             # every query's best id (or -1) may not come back
        assert (exclude >= 0).sum() > SYN_NQ // 3
        ref = dict(allowed=allowed, exclude=exclude, group=group, groups=groups, mask=masks, mode="any", tags=tags)
        kw = dict(allowed=aset, exclude=exclude, group=group, tags=masks, tags_mode="any", between=between)
        w, wdbg = ranged_batch(oracle, ox, qn, between, values, 10, 10, debug=True, **ref)
        assert (w != want).any() and (w != -1).any()
        try:
            # ("forced": pinned on with the limit at -128 — every query with a plain list is flagged, scanned again
            #  exactly and masked again by all five passes through the flag list)
            for plain in (False, "always", "forced"):
                dev.set_plain_scan("always" if plain == "forced" else plain)
                dev.set_option(_lib.OPT_PLAIN_LIMIT, -128 if plain == "forced" else 0x7fffffff)
                got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, **kw)
                _same(got, gd, w, wdbg, (kp, plain))
                if plain == "forced":
                    st = dev.plain_stats()
                    assert st["plain_units"] > 0 and st["flagged_queries"] > 0, (kp, st)
            _within(got, between, values)
            assert allowed[got[got != -1]].all()
            assert not (got == np.where(exclude >= 0, exclude, -2)[:, None]).any()
            dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
            dev.set_plain_scan(True)
            ids, dist = dev.query_batch(qn, qp, 10, 10, between=between, return_distances=True)
            np.testing.assert_array_equal(ids, want)
            assert same_bits(dist, exact_distances(oracle, qn, ivf.data, ids))
            ids, dist = dev.query_batch(qn, qp, 10, 10, return_distances=True, **kw)
            np.testing.assert_array_equal(ids, w)
            assert same_bits(dist, exact_distances(oracle, qn, ivf.data, ids))
        finally:
            dev.set_plain_scan(True)
            dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
            aset.close()
            dev.set_groups(None)
            dev.set_tags(None)


def test_pipelined_pairs_in_both_orders(tk, oracle, synthetic):
    """Device calls in pairs, each with its own range array, each equal to its own reference.  Whether two calls ran as
    one batch is read from the lane replay's wave count (200 queries: 4 waves of 64 alone, 7 for two calls together):
    two ranged calls join, a ranged call and an unranged one never do."""
    import torch
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import query_ranges
    ivf, ox, qn, qp, values, between, want_all, _ = synthetic(1)
    dev = ivf.device_index()
    nq = 200
    qn, qp = np.ascontiguousarray(qn[:nq]), np.ascontiguousarray(qp[:nq])
    first = (between[0][:nq], between[1][:nq])
    other = (np.roll(first[0], 3, axis=0), np.roll(first[1], 3, axis=0))
    want = dict(first=want_all[:nq], other=ranged_batch(oracle, ox, qn, other, values, 10, 10),
                none=guarded_batch(oracle, ox, qn, 10, 10))
    assert (want["first"] != want["other"]).any(axis=1).sum() > nq // 4
    # (row nq - 1 of the first call and row 0 of the second, either side of n_a, answer differently from each other's ranges)
    assert (want["first"][-1] != want["other"][-1]).any() and (want["first"][0] != want["other"][0]).any()
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    qn_d, qp_d = cuda(qn), cuda(qp)
    keys = dict(first=cuda(query_ranges(first, nq, 2, "f")), other=cuda(query_ranges(other, nq, 2, "f")))

    def run(kinds):
        outs = [torch.full((nq, 10), -7, dtype=torch.int64, device="cuda") for _ in kinds]
        torch.cuda.synchronize()
        dev.set_option(_lib.OPT_REPLAY_COUNT, 1)
        for kind, out in zip(kinds, outs):
            dev.query_batch_dev(qn_d.data_ptr(), qp_d.data_ptr(), 0, nq, 10, 10, out.data_ptr(),
                                between_ptr=keys[kind].data_ptr() if kind in keys else None)
        dev.join()
        torch.cuda.synchronize()
        for i, (kind, out) in enumerate(zip(kinds, outs)):
            np.testing.assert_array_equal(out.cpu().numpy(), want[kind], err_msg=f"call {i} {kind}")
        return dev.replay_stats()["waves"]
    try:
        dev.set_option(_lib.OPT_PAIR_NQ, 0)         # small batches too take the lane kernels, which count waves
        dev.set_pipeline(3)
        dev.set_coalesce(2)
        run(["first", "other", "none", "first", "none", "none", "other", "first", "other"])
        assert dev.last_replay()["form"] == _lib.REPLAY_LANES
        alone, together = 2 * ((nq + 63) // 64), (2 * nq + 63) // 64
        assert together < alone
        assert run(["first", "other"]) == together          # two range arrays: one batch, in both orders
        assert run(["other", "first"]) == together
        assert run(["none", "none"]) == together
        assert run(["first", "none"]) == alone              # never a ranged call with an unranged one
        assert run(["none", "other"]) == alone
    finally:
        dev.join()
        dev.set_option(_lib.OPT_REPLAY_COUNT, 0)
        dev.set_pipeline(1)
        dev.set_coalesce(1)
        dev.set_option(_lib.OPT_PAIR_NQ, 4)


SUB_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from tinyknn_amd import IVF, FastPQ, _lib
from oracle import oracle
from allowed_reference import reference_index
from between_reference import ranged_batch
import between_shapes as bs
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
values = bs.assignments(ivf.ids[:len(ivf.active_centers)], n, 3)["two"]
ivf.set_values(values)
dev = ivf.device_index()
ms = dev.max_sub_batch(k, n_probes)
sel = np.arange(2 * ms + 5) % nq0                    # three parts
part = (len(sel) + 2) // 3
assert len(sel) > 2 * ms and part % nq0 != 0         # row i of a part has other ranges than row i of the call
sample = np.unique(np.concatenate([np.arange(8), part + np.arange(-4, 4), 2 * part + np.arange(-4, 4),
                                   len(sel) - 1 - np.arange(4)]))
lo, hi, _ = bs.ranges(values, nq0, 4)
want0 = ranged_batch(oracle, ox, qn0, (lo, hi), values, k, n_probes)
assert (want0[1:] != want0[:-1]).any()
for depth in (1, 3):
    dev.set_pipeline(depth)
    got = dev.query_batch(qn0[sel], qp0[sel], k, n_probes, between=(lo[sel], hi[sel]))
    assert np.array_equal(got[sample], want0[sel][sample]), ("sampled rows differ", depth)
    assert np.array_equal(got, want0[sel]), ("rows differ", depth, np.flatnonzero((got != want0[sel]).any(axis=1))[:5])
assert dev.value_table()["builds"] == 1
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
    # timestamps 0 .. 999 on the old rows, 2000 .. 2999 on the added rows, 5000 on the updated ones
    ivf.set_values(rng.integers(0, 1000, N0).astype(np.int64))
    pool = np.array([[INT64_MIN, INT64_MAX], [100, 700], [2000, INT64_MAX], [5000, 5000], [INT64_MIN, 499], [900, 2500]])
    pick = rng.integers(0, len(pool), len(qn))
    between = (pool[pick, 0], pool[pick, 1])

    def check(builds):
        want, wd = ranged_batch(oracle, _oracle_of(oracle, ivf), qn, between, ivf.values, 10, 5, debug=True)
        got, gd = dev.query_batch(qn, qp, 10, 5, debug=True, between=between)
        _same(got, gd, want, wd, builds)
        _within(got, between, ivf.values)
        assert dev.value_table()["built"] and dev.value_table()["builds"] == builds
        return got
    before = check(1)
    assert (before[pick == 2] == -1).all() and (before[pick == 3] == -1).all()
    # add without values=: refused before anything changes
    new = synth_rows(500, d, SEED, _fitted("angular", d)[2], SIGMA, row0=N0)
    with pytest.raises(ValueError, match="values"):
        ivf.add(new)
    assert dev.N == N0 and dev.values_set() == N0
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, between=between), before)
    # add: the values are set again for all rows, the table is made again for the new lists
    ivf.add(new, values=rng.integers(2000, 3000, 500))
    assert ivf.device_index() is dev and dev.N == N0 + 500 and dev.values_set() == N0 + 500
    assert len(ivf.values) == N0 + 500 and not dev.value_table()["built"]
    after = check(2)
    assert (after[pick == 2] >= N0).any() and (after != before).any()
    # remove: ids are stable, nothing to set; the table is made again for the compacted lists
    dead = np.concatenate([after[:, 0][after[:, 0] >= 0], rng.choice(N0, 300, replace=False)])
    ivf.remove(dead)
    assert dev.values_set() == N0 + 500 and not dev.value_table()["built"]
    gone = check(3)
    assert not np.isin(gone, dead).any()
    # update without values=: new vectors, the rows keep their values; the table follows the new lists
    live = np.setdiff1d(np.arange(N0), dead)
    ids = rng.choice(live, 200, replace=False)
    kept = ivf.values.copy()
    ivf.update(ids, synth_rows(200, d, SEED + 3, _fitted("angular", d)[2], SIGMA))
    np.testing.assert_array_equal(ivf.values, kept)
    assert dev.values_set() == N0 + 500 and not dev.value_table()["built"]
    moved = check(4)
    assert (moved != gone).any()
    # update with values=: those rows are at 5000 now, and nothing else is
    ivf.update(ids[:100], synth_rows(100, d, SEED + 4, _fitted("angular", d)[2], SIGMA), values=np.full(100, 5000))
    assert (ivf.values[ids[:100]] == 5000).all() and not dev.value_table()["built"]
    last = check(5)
    point = last[pick == 3]
    assert (point != -1).any() and np.isin(point[point != -1], ids[:100]).all()
    # at the ABI, rows added without the values being set again (the host copy forgotten, so that add() neither asks
    # for values nor sets them): TK_ERR_STATE, nothing run; a call without a range array is served
    del ivf.values
    ivf.add(synth_rows(100, d, SEED, _fitted("angular", d)[2], SIGMA, row0=N0 + 500))
    assert dev.N == N0 + 600 and dev.values_set() == N0 + 500
    with pytest.raises(_lib.TinyKnnHipError, match="set them again"):
        dev.query_batch(qn, qp, 10, 5, between=between)
    assert dev.value_table()["builds"] == 5
    dev.query_batch(qn, qp, 10, 5)


def test_plain_state_untouched_mode_two_identical_and_the_half_store(tk, oracle, synthetic):
    from tinyknn_amd.ivf import DeviceIndex
    from store_reference import rounded
    ivf, ox, qn, qp, values, between, want, wd = synthetic(1)
    dev = ivf.device_index()
    dev.set_plain_scan(True)
    for _ in range(4):              # the unrestricted traffic settles the automatic state
        dev.query_batch(qn, qp, 10, 10)
    before = dev.plain_stats()["state"], dev.plain_stats()["pause_left"]
    for _ in range(20):
        got = dev.query_batch(qn, qp, 10, 10, between=between)
    np.testing.assert_array_equal(got, want)
    st = dev.plain_stats()
    assert (st["state"], st["pause_left"]) == before, (st, before)
    assert st["plain_units"] == 0, st       # a ranged batch in the automatic mode: the exact scan
    # an all-unbounded host array is no array: the library takes the call as an unrestricted one — the plain scan in
    # the automatic mode — and launches no pass; -inf below and +inf above are unbounded ends too
    plain = dev.query_batch(qn, qp, 10, 10, debug=True)
    units = dev.plain_stats()["plain_units"]
    assert units > 0, dev.plain_stats()
    _same(*dev.query_batch(qn, qp, 10, 10, debug=True, between=(None, None)), *plain, "unbounded")
    assert dev.plain_stats()["plain_units"] == units
    none = np.full((SYN_NQ, 2), -np.inf), np.full((SYN_NQ, 2), np.inf)
    _same(*dev.query_batch(qn, qp, 10, 10, debug=True, between=none), *plain, "+-inf")
    assert dev.plain_stats()["plain_units"] == units
    try:
        dev.set_plain_scan("always")
        got, gd = dev.query_batch(qn, qp, 10, 10, debug=True, between=between)
        assert dev.plain_stats()["plain_units"] > 0
        _same(got, gd, want, wd, "mode 2")
    finally:
        dev.set_plain_scan(True)
    # the half store: the same heaps; the rescoring reads the rounded rows
    half = DeviceIndex(ivf, store="float16")
    try:
        half.set_values(values)
        ref = ranged_batch(oracle, oracle_index(oracle, ivf, rounded(ivf.data)), qn, between, values, 10, 10, debug=True)
        _same(*half.query_batch(qn, qp, 10, 10, debug=True, between=between), *ref, "half store")
        for key in KEYS:
            np.testing.assert_array_equal(ref[1][key], wd[key])
    finally:
        half.close()


def test_refusals_and_no_table_without_a_range_array(tk):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex, query_ranges
    from tinyknn_amd.multi_gpu import shard_lists
    g = golden("g6_ivf_an100.npz")
    ivf = fixture_ivf(g)
    dev = ivf.device_index()
    qn, qp, N = g["qn"], g["qpq"], len(g["data"])
    nq = len(qn)
    out = np.zeros((nq, 10), dtype=np.int64)

    def ex5(d, keys):
        r = None if keys is None else np.ascontiguousarray(keys, dtype=np.int64)
        return _lib.lib().tk_index_query_batch_ex5(
            d.handle, None, None, None, None, 0, None if r is None else r.ctypes.data,
            _lib.ptr(np.ascontiguousarray(qn), _lib._f32p), qp.ctypes.data, 0, nq, 10, 5, 0, _lib.ptr(out, _lib._i64p),
            None, None, None, None)
    plain = dev.query_batch(qn, qp, 10, 5)
    some = np.tile(np.array([[0, 5]], dtype=np.int64), (nq, 1, 1))
    # a ranged call while no values are set: TK_ERR_STATE (-3), nothing run; no array is an unrestricted call
    out[:] = -9
    assert ex5(dev, some) == -3 and (out == -9).all()
    with pytest.raises(_lib.TinyKnnHipError, match="no values"):
        dev.query_batch(qn, qp, 10, 5, between=(0, 5))
    assert ex5(dev, None) == 0
    np.testing.assert_array_equal(out, plain)
    # set_values: a wrong length, 0 and 5 columns (the library's own checks, and the Python layer's)
    keys = np.zeros((5, N), dtype=np.int64)
    lib = _lib.lib()
    assert lib.tk_index_set_values(dev.handle, keys.ctypes.data, N - 1, 1) == -1
    for cols in (0, 5, -1):
        assert lib.tk_index_set_values(dev.handle, keys.ctypes.data, N, cols) == -1
        assert "columns" in lib.tk_last_error().decode()
    assert dev.values_set() == 0 and dev.value_table()["cols"] == 0
    with pytest.raises(ValueError):
        ivf.set_values(np.zeros(N + 1))
    with pytest.raises(ValueError):
        dev.set_values(np.zeros((N, 5)))
    # values set: a call without between= returns the unrestricted rows and makes no table
    values = (np.arange(N) % 3).astype(np.int32)
    ivf.set_values(values)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5), plain)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, debug=True)[0], plain)
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5, between=(None, None)), plain)
    assert ex5(dev, query_ranges((None, None), nq, 1, "i")) == 0
    np.testing.assert_array_equal(out, plain)
    assert dev.value_table() == dict(built=False, bytes=0, builds=0, row_bytes=8 * N, cols=1)
    with pytest.raises(NotImplementedError):
        ivf.query_batch(np.array(qn, copy=True), 10, n_probes=5, fast=True, between=(0, 1))
    with pytest.raises(ValueError):
        ivf.add(np.zeros((3, qn.shape[1]), np.float32))
    assert dev.value_table()["builds"] == 0
    # one real entry: only that query changes
    lo, hi = np.full(nq, -np.inf), np.full(nq, np.inf)
    lo[0] = hi[0] = (int(plain[0, 0]) % 3 + 1) % 3              # a value the unrestricted best row does not have
    got = dev.query_batch(qn, qp, 10, 5, between=(lo, hi))
    np.testing.assert_array_equal(got[1:], plain[1:])
    assert plain[0, 0] not in got[0] and dev.value_table()["builds"] == 1
    # cleared: ranged calls are refused again
    ivf.set_values(None)
    assert dev.values_set() == 0 and not dev.value_table()["built"] and dev.value_table()["cols"] == 0
    assert ex5(dev, some) == -3
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 10, 5), plain)
    # a list-sharded index
    owner = shard_lists(np.asarray(g["list_sizes"], dtype=np.int64), 2)
    shard = DeviceIndex(fixture_ivf(g), owner, 0, 2)
    try:
        assert lib.tk_index_set_values(shard.handle, keys.ctypes.data, N, 1) == -1
        assert "list-sharded" in lib.tk_last_error().decode()
        with pytest.raises(RuntimeError, match="list-sharded"):
            shard.set_values(values)
        assert ex5(shard, some) == -1 and "list-sharded" in lib.tk_last_error().decode()
    finally:
        shard.close()


def test_values_leave_with_their_rows(tk):
    """build_resident drops the values of the rows before it, as build does."""
    from tinyknn_amd import IVF, FastPQ, _lib
    X = np.random.default_rng(3).standard_normal((3000, 32)).astype(np.float32)
    ivf = IVF("euclidean", 12, FastPQ(2))
    ivf.fit(X).build(X, n_probes=1)
    ivf.set_values(np.arange(3000) % 4)
    assert ivf.device_index().values_set() == 3000
    ivf.build_resident(2000, 32, 7)
    dev = ivf.device_index()
    assert ivf.values is None and dev.N == 2000 and dev.values_set() == 0
    qn, qp = ivf._prepare(X[:8].copy())
    plain = dev.query_batch(qn, qp, 5, 3)
    with pytest.raises(_lib.TinyKnnHipError, match="no values"):
        dev.query_batch(qn, qp, 5, 3, between=(0, 1))
    ivf.set_values(np.ones(2000, dtype=np.float16))
    np.testing.assert_array_equal(dev.query_batch(qn, qp, 5, 3, between=(1, 1)), plain)
    assert (dev.query_batch(qn, qp, 5, 3, between=(1.5, None)) == -1).all()
