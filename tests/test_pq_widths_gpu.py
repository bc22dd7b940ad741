"""The device index at every PQ width and dims_per_block the C ABI takes (tk_index_set_pq: dims_per_block 1 .. 32,
up to 512 blocks), against the CPU oracle: ids, probe lists and heap arrays (layout included), bit for bit.

An index fitted the usual way has M <= 32 blocks (rotated to 64 dims) or M = 52 (d = 100), always 2 dims per block;
the kernels change form with M = dq / dims_per_block.  The indexes here are made by hand (pq_shapes.py) at the widths
where a form begins or ends:

    M 8, 12                      the guarded 8-pair form of the plain (matrix-core) kernel
    M 36 (dims_per_block 2, 1 — F-ordered centres —, 4), 48      its guarded 26-pair form, P = 18 / 24
    M 52 from d = 104            the unguarded P = 26 form from an index that is not 100-d
    M 56                         the first width the plain kernel refuses (tk_plain_fits): exact scans only
    M 32 from dims_per_block 8 / 16       dims_per_block through stage_tables (einsum's group loop inside an index)
    M 156 | 160, 208 | 212       scan_form_gmax: the last width an LDS form of the list-major scan takes (form 1: 9984 B,
                                 form 2: 13312 B per wave, 64 M bytes per group of four queries) | the first it declines
    M 256 | 260                  the M <= 256 paths of build_tables_kernel
    M 472, 512 (also 1 dim per block)     the limits; float64 tables of 474 .. 512 blocks need more than 64 KiB of LDS
"""
from collections import namedtuple

import numpy as np
import pytest

from pq_shapes import handmade_index, oracle_answers, oracle_index

pytestmark = pytest.mark.gpu

K, NQ, N, LISTS = 10, 200, 6000, 24         # 250 rows = 16 chunks per list
# (n_probes, pass_1): default heaps, and a heap of 7 that is full after a few rows (more slots go the plain way)
TRIPLES = ((4, None), (8, 7), (8, None))
# (heap mode, scan mode) as test_hip_parity.py::test_ivf_vs_oracle_larger pairs them
HEAP_SCAN = ((0, 2), (0, 1), (1, 1), (2, 2), (0, 0), (2, 0), (3, 0), (3, 2), (3, 1))

Case = namedtuple("Case", "M metric d dpb f64 rot")


def _cases():
    out = []

    def add(M, d, dpb, metric="euclidean", f64=False, rot=None):
        out.append(Case(M, metric, d, dpb, f64, rot))

    add(8, 16, 2)
    add(12, 24, 2)
    add(36, 72, 2)
    add(36, 72, 2, "angular")
    add(36, 72, 2, f64=True)
    add(36, 36, 1)
    add(36, 144, 4)
    add(48, 96, 2)
    add(52, 104, 2)
    add(56, 112, 2)
    add(56, 112, 2, "angular")
    add(56, 112, 2, f64=True)
    add(32, 256, 8)
    add(32, 512, 16)
    for M in (156, 160, 208, 212, 256):
        add(M, 2 * M, 2)
    add(260, 520, 2)
    add(260, 520, 2, f64=True)
    add(472, 944, 2)
    add(472, 944, 2, f64=True)
    add(512, 1024, 2)
    add(512, 1024, 2, f64=True)
    add(512, 512, 1)
    add(24, 72, 2, rot=48)                  # rotated (and cut) to 48 dims: float64 q_pq through a real rotation
    return out


CASES = _cases()


def _id(c):
    return "M%d-%s-d%d-dpb%d-%s%s" % (c.M, c.metric, c.d, c.dpb, "f64" if c.f64 else "f32",
                                      "-rot%d" % c.rot if c.rot else "")


def _same(got, dbg, ref, what):
    np.testing.assert_array_equal(dbg["probes"], ref["probes"], err_msg=what)
    np.testing.assert_array_equal(dbg["heap_idx"], ref["heap_idx"], err_msg=what)
    np.testing.assert_array_equal(dbg["heap_val"], ref["heap_val"], err_msg=what)
    np.testing.assert_array_equal(got, ref["ids"], err_msg=what)


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_index_equals_oracle_at_width(oracle, c):
    from tinyknn_amd import _lib
    ivf, qs = handmade_index(c.metric, c.d, c.dpb, LISTS, N, NQ, seed=c.M * 131 + c.dpb, f64=c.f64, rot=c.rot, M=c.M)
    ox = oracle_index(oracle, ivf)
    qn, qp = ivf._prepare(qs.copy())
    assert (qp.dtype == np.float64) == (c.f64 or c.rot is not None)
    assert ivf.pq.centers.flags.c_contiguous == (c.dpb != 1)
    dev = ivf.device_index()
    assert dev.M == c.M and dev.dpb == c.dpb
    try:
        for n_probes, pass_1 in TRIPLES:
            ref = oracle_answers(ox, qn, K, n_probes, pass_1)
            # the index is not degenerate: the heaps fill (at 512 blocks one query's sums all sit on the int8 rail
            # and its heap keeps its -1 sentinels: that row is compared like every other)
            assert (ref["ids"][:, :min(K, pass_1 or K)] >= 0).all(axis=1).mean() >= 0.99

            def run(what):
                got, dbg = dev.query_batch(qn, qp, K, n_probes, pass_1=pass_1, debug=True)
                _same(got, dbg, ref, "%s p%d R%s %s" % (_id(c), n_probes, pass_1, what))

            dev.set_plain_scan(False)
            for heap_mode, scan_mode in HEAP_SCAN:
                dev.set_heap_mode(heap_mode)
                dev.set_scan_mode(scan_mode)
                run("heap %d scan %d" % (heap_mode, scan_mode))
            # list-major: the table rows through LDS (form 1 up to M = 156, form 2 up to M = 208: beyond, the
            # launcher falls to form 0, whose run is the (0, 2) pair above)
            dev.set_heap_mode(0)
            dev.set_scan_mode(2)
            for form in (1, 2):
                dev.set_option(_lib.OPT_SCAN_FORM, form)
                run("form %d" % form)
            dev.set_option(_lib.OPT_SCAN_FORM, 0)
            # the plain kernel pinned on; then with every query's limit below any bound: all re-scanned exactly
            dev.set_plain_scan("always")
            run("plain")
            units = dev.plain_stats()["plain_units"]
            if c.M > 52:
                assert units == 0, (_id(c), units)
            elif pass_1 == 7:
                assert units > 0, (_id(c), dev.plain_stats())
            dev.set_option(_lib.OPT_PLAIN_LIMIT, -128)
            try:
                run("plain, all re-scanned")
            finally:
                dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)
            dev.set_plain_scan(False)
            # pipelined workspaces and streams, through the streaming session (which pads on the device)
            dev.set_scan_mode(0)
            dev.set_pipeline(2)
            outs = [dev.query_batch(qn, qp, K, n_probes, pass_1=pass_1) for _ in range(4)]
            dev.set_pipeline(1)
            for o in outs:
                np.testing.assert_array_equal(o, ref["ids"], err_msg="%s p%d pipelined" % (_id(c), n_probes))
    finally:
        dev.set_option(_lib.OPT_SCAN_FORM, 0)
        dev.close()


@pytest.mark.parametrize("M", [36, 56])
def test_list_sharded_at_width(oracle, M):
    """Three simulated ranks, dense and filtered exchange, room for the worst case: the oracle's ids.  At M = 36 the
    shard path scans in two phases with the plain kernel; at M = 56 it must decline it (api_shard.hip: M <= 52) and
    answer all the same."""
    from test_shard_gpu import simulate_world
    nq, n_probes = 65, 8
    ivf, qs = handmade_index("euclidean", 2 * M, 2, LISTS, N, nq, seed=M, M=M)
    ox = oracle_index(oracle, ivf)
    qn, qp = ivf._prepare(qs.copy())
    want = ox.query_batch(qn, K, n_probes)
    worst = nq * min(n_probes, LISTS) * (N // 16 + 2)
    for ex in ("dense", "filtered"):
        st = {}
        ids, flags, _ = simulate_world(ivf, 3, qn, qp, K, n_probes, capacity=worst, exchange=ex, stats=st)
        assert not flags.any()
        assert bool(st.get("two_phase")) == (M <= 52), (M, ex, st.keys())
        np.testing.assert_array_equal(ids, want, err_msg="M=%d %s" % (M, ex))


@pytest.mark.parametrize("M", [56, 260])
def test_fast_front_end_at_width(M):
    """Euclidean, unrotated: the device front end only pads, so fast=True returns the exact path's ids."""
    ivf, qs = handmade_index("euclidean", 2 * M, 2, LISTS, N, NQ, seed=M + 7, M=M)
    try:
        for n_probes in (4, 8):
            exact = ivf.query_batch(qs, K, n_probes)
            assert (exact >= 0).all(axis=1).mean() >= 0.99
            np.testing.assert_array_equal(ivf.query_batch(qs, K, n_probes, fast=True), exact)
    finally:
        ivf.device_index().close()
