"""per_group= on the awkward indexes of tests/restricted_shapes.py (lists shorter than a chunk and empty ones, a single
list, more probes than lists, probe lists that wrap, repeated labels, odd d, the half store, k = 1 and k = 50 beside
heaps of 3 to 2201 entries, indexes changed by add() and remove()), composed with whatever restriction the case already
carries: tests/per_group_edge_shapes.py::CapCase draws the groups and a cap per query.  Every leg compares ids, counts
and the bits of the distances with per_group_reference.capped_from_heaps over the guarded reference's heap;
tests/test_per_group_edges_cpu.py shows what the default seeds hold."""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import per_group_edge_shapes as es  # noqa: E402
import restricted_shapes as rs  # noqa: E402
from per_group_reference import capped_batch  # noqa: E402

pytestmark = pytest.mark.gpu

# seeds that failed once, run whatever the range becomes: {seed: why}
NAMED = {}
SEEDS = sorted(set(es.fuzz_seeds()) | set(NAMED))


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    return tinyknn_amd


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got_ids, got_dist, want, msg=""):
    ids, dist, counts = want[:3]
    np.testing.assert_array_equal(got_ids, ids, err_msg=f"ids {msg}")
    np.testing.assert_array_equal((got_ids != -1).sum(axis=1), counts, err_msg=f"counts {msg}")
    if got_dist is not None:
        assert got_dist.dtype == dist.dtype, (got_dist.dtype, dist.dtype, msg)
        np.testing.assert_array_equal(_bits(got_dist), _bits(dist), err_msg=f"distance bits {msg}")


@contextlib.contextmanager
def opened(seed):
    """-> (cap case, a device index of its own with its groups set, a prepared AllowSet of the case's mask or None)"""
    t = es.fuzz_case(seed)
    assert t.skipped is None, (t, t.skipped)
    from tinyknn_amd.ivf import DeviceIndex
    dev = DeviceIndex(t.case.ivf)       # (its own: the case stays as it was made)
    try:
        dev.set_groups(t.groups)
        aset = None if t.case.allowed is None else dev.allow(t.case.allowed)
        yield t, dev, aset
    finally:
        dev.close()                     # (closes its sets too)


@pytest.mark.parametrize("seed", SEEDS)
def test_forms_outputs_and_both_kinds_of_allowed_set(tk, oracle, seed):
    from tinyknn_amd import _lib
    with opened(seed) as (t, dev, aset):
        c = t.case.shape
        want = t.want()
        try:
            for form in (0, 1, 2):
                dev.set_option(_lib.OPT_RESCORE_FORM, form)
                for prepared in ((False, True) if aset is not None else (False,)):
                    kw = t.case.device_kwargs(aset if prepared else None)
                    leg = f"{t} form={form} prepared={prepared}"
                    _same(*dev.query_batch(t.case.qn, t.case.qp, c["k"], c["n_probes"], return_distances=True,
                                           per_group=t.caps, **kw), want, leg)
                    _same(dev.query_batch(t.case.qn, t.case.qp, c["k"], c["n_probes"], per_group=t.caps, **kw), None,
                          want, leg + " ids alone")
        finally:
            dev.set_option(_lib.OPT_RESCORE_FORM, 2)


@pytest.mark.parametrize("seed", [s for s in SEEDS if "e" in rs.shape(s)["subset"]])
def test_stored_rows_as_queries(tk, oracle, seed):
    with opened(seed) as (t, dev, aset):
        case, c = t.case, t.case.shape
        rows = case.rows
        qn, qp = dev.gather_queries(rows)
        # (a rotated PQ: the reference is fed the device-made q_pq, so that both build the same tables)
        want = capped_batch(oracle, case.ox, qn, t.caps, t.groups, c["k"], c["n_probes"], exclude=rows,
                            q_pq=qp if dev.rotated() else None, allowed=case.allowed)
        ids, dist = dev.query_rows(rows, c["k"], c["n_probes"], allowed=aset, return_distances=True, per_group=t.caps)
        _same(ids, dist, want, t)
        assert not (ids == rows[:, None]).any(), "a row returned itself"
        _same(dev.query_rows(rows, c["k"], c["n_probes"], allowed=aset, per_group=t.caps), None, want, (t, "ids alone"))


@pytest.mark.parametrize("seed", rs.pair_seeds(SEEDS))
def test_pipelined_pairs(tk, oracle, seed):
    """The case's call and its partner (Case.second), each with a cap array of its own, enqueued as a coalesced pair
    in both orders: the second call's rows start at n_a, where the capped kernels turn to m_b."""
    import torch
    with opened(seed) as (t, dev, aset):
        case, c = t.case, t.case.shape
        nq, k, n_probes = len(case.qn), c["k"], c["n_probes"]
        qn_b, qp_b, ex_b, gr_b, caps_b, want_b = t.second()
        cuda = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
        f64 = int(case.qp.dtype != np.float32)
        first = dict(qn=cuda(case.qn), qp=cuda(case.qp), ex=cuda(case.exclude), gr=cuda(case.group), m=cuda(t.caps),
                     want=t.want())
        second = dict(qn=cuda(qn_b), qp=cuda(qp_b), ex=cuda(ex_b), gr=cuda(gr_b), m=cuda(caps_b), want=want_b)
        try:
            dev.set_pipeline(2)
            dev.set_coalesce(2)
            for order in ((first, second), (second, first)):
                outs = [(torch.full((nq, k), -7, dtype=torch.int64, device="cuda"),
                         torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")) for _ in order]
                for call, (o, od) in zip(order, outs):
                    dev.query_batch_dev(call["qn"].data_ptr(), call["qp"].data_ptr(), f64, nq, k, n_probes,
                                        o.data_ptr(), allowed=aset, dist_ptr=od.data_ptr(),
                                        exclude_ptr=None if call["ex"] is None else call["ex"].data_ptr(),
                                        group_ptr=None if call["gr"] is None else call["gr"].data_ptr(),
                                        per_group_ptr=call["m"].data_ptr())
                dev.join()
                torch.cuda.synchronize()
                name = "AB" if order[0] is first else "BA"
                for j, (call, (o, od)) in enumerate(zip(order, outs)):
                    _same(o.cpu().numpy(), od.cpu().numpy(), call["want"], f"{t} call {j} of {name}")
        finally:
            dev.join()
            dev.set_pipeline(1)
            dev.set_coalesce(1)
