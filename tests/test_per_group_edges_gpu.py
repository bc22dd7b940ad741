"""per_group= on the device where the capped walk leaves its first 64 ranks (cap_select.h; capped_tile_kernel and
capped_rows_kernel of rescore.hip): heaps of 63 to 257 entries — pass_1 sets R — on both sides of every chunk of 64
ranks and of the staged body's three ranking widths, k from 1 to 100, under the three rescoring forms; d % 4 != 0,
d = 256, the half store and float64 vectors at the same edges; the pipelined pair, a call beyond one sub-batch, and the
largest heap the library's own LDS check admits.  The shapes are those of tests/per_group_edge_shapes.py, whose census
tests/test_per_group_edges_cpu.py asserts.  Every comparison is exact — ids, counts and the bits of the distances —
against tests/per_group_reference.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import per_group_edge_shapes as es  # noqa: E402
from per_group_edge_shapes import N_PROBES, NQ  # noqa: E402

pytestmark = pytest.mark.gpu

# grid points that failed once, run whatever the grid becomes: {(index, R): why}
NAMED = {}
POINTS = sorted({(name, R) for name in es.INDEXES for R, _ in es.grid(name)} | set(NAMED))
_devices = {}


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    yield tinyknn_amd
    for dev in _devices.values():
        dev.close()
    _devices.clear()


def _device(name):
    """a device index of this file's own: the IVF of "twins" is shared with tests/test_per_group_gpu.py and stays as
    it was made (groups are set on the device copy alone)"""
    if name not in _devices:
        from tinyknn_amd.ivf import DeviceIndex
        _devices[name] = DeviceIndex(es.index(name)[0])
    return _devices[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got_ids, got_dist, want, msg=""):
    """ids, counts and distance bits against the reference's (ids, distances, counts)"""
    ids, dist, counts = want[:3]
    np.testing.assert_array_equal(got_ids, ids, err_msg=f"ids {msg}")
    np.testing.assert_array_equal((got_ids != -1).sum(axis=1), counts, err_msg=f"counts {msg}")
    if got_dist is not None:
        assert got_dist.dtype == dist.dtype, (got_dist.dtype, dist.dtype, msg)
        np.testing.assert_array_equal(_bits(got_dist), _bits(dist), err_msg=f"distance bits {msg}")


# ---- the grid: every leg under every form, with distances and ids alone ----------------------------------------------

@pytest.mark.parametrize("name,R", POINTS)
def test_every_leg_under_every_form(tk, oracle, name, R):
    from tinyknn_amd import _lib
    _, ox, qn, qp = es.index(name)
    dev = _device(name)
    assert dev.store == (es.INDEXES[name][2] or np.dtype(es.INDEXES[name][1]).name)
    ks = es.ks_of(name, R)
    try:
        for a in sorted({a for a, _ in es.LEGS}):
            dev.set_groups(es.groups(name, a))
            for m in [m for b, m in es.LEGS if b == a]:
                arg = es.caps(m)
                for k in ks:
                    want = es.reference(name, R, k, a, m)
                    for form in es.FORMS:
                        dev.set_option(_lib.OPT_RESCORE_FORM, form)
                        leg = (name, R, k, a, m, "form", form)
                        _same(*dev.query_batch(qn, qp, k, N_PROBES, R, return_distances=True, per_group=arg), want, leg)
                        _same(dev.query_batch(qn, qp, k, N_PROBES, R, per_group=arg), None, want, (leg, "ids alone"))
    finally:
        dev.set_option(_lib.OPT_RESCORE_FORM, 2)


@pytest.mark.parametrize("name,R", POINTS)
def test_a_cap_beyond_any_group_is_the_uncapped_call(tk, oracle, name, R):
    from tinyknn_amd import _lib
    _, ox, qn, qp = es.index(name)
    dev = _device(name)
    dev.set_groups(es.groups(name, "own"))
    try:
        for k in es.ks_of(name, R):
            want = es.reference(name, R, k, "own", 1)           # all-distinct groups: the first k of the ranking
            for form in es.FORMS:
                dev.set_option(_lib.OPT_RESCORE_FORM, form)
                plain = dev.query_batch(qn, qp, k, N_PROBES, R, return_distances=True)
                _same(*plain, want, (name, R, k, "uncapped", form))
                ids, dist = dev.query_batch(qn, qp, k, N_PROBES, R, return_distances=True, per_group=k)
                np.testing.assert_array_equal(ids, plain[0], err_msg=str((name, R, k, form)))
                np.testing.assert_array_equal(_bits(dist), _bits(plain[1]), err_msg=str((name, R, k, form)))
                np.testing.assert_array_equal(dev.query_batch(qn, qp, k, N_PROBES, R, per_group=k), plain[0])
    finally:
        dev.set_option(_lib.OPT_RESCORE_FORM, 2)


# ---- the call path at the edges: the pipelined pair, a call beyond one sub-batch -------------------------------------

@pytest.mark.parametrize("R,k", [(129, 64), (256, 65)])
@pytest.mark.parametrize("name", list(es.INDEXES))
def test_pipelined_pair_with_two_cap_arrays(tk, oracle, name, R, k):
    """as test_per_group_gpu.py::test_capped_and_uncapped_calls_interleaved_in_the_pipeline"""
    import torch
    _, ox, qn, qp = es.index(name)
    dev = _device(name)
    a = "near5"
    dev.set_groups(es.groups(name, a))
    m_a = es.caps("mix")
    m_b = np.roll(m_a, 1)
    h = es.heaps(name, k, R)
    from per_group_reference import capped_from_heaps
    want = {"a": es.reference(name, R, k, a, "mix"),
            "b": capped_from_heaps(oracle, ox, qn, h, m_b, es.groups(name, a), k),
            None: es.reference(name, R, k, "own", 1)}
    st = torch.cuda.current_stream().cuda_stream
    q_dev, qp_dev = torch.from_numpy(qn).cuda(), torch.from_numpy(qp).cuda()
    caps_dev = {"a": torch.from_numpy(m_a).cuda(), "b": torch.from_numpy(np.ascontiguousarray(m_b)).cuda()}
    f64 = qp.dtype != np.float32
    dist_dtype = torch.float64 if ox.data.dtype == np.float64 else torch.float32
    SENT = -7.0
    calls = [("a", True), ("b", True), (None, True), ("a", False), ("b", False), (None, False), ("b", True), ("a", True)]
    outs = []
    try:
        dev.set_pipeline(2)
        dev.set_coalesce(2)
        for which, wd in calls:
            o = torch.full((NQ, k), -7, dtype=torch.int64, device="cuda")
            od = torch.full((NQ, k), SENT, dtype=dist_dtype, device="cuda")
            outs.append((which, wd, o, od))
            dev.query_batch_dev(q_dev.data_ptr(), qp_dev.data_ptr(), f64, NQ, k, N_PROBES, o.data_ptr(), R, stream=st,
                                dist_ptr=od.data_ptr() if wd else None,
                                per_group_ptr=None if which is None else caps_dev[which].data_ptr())
        dev.join(st)
        torch.cuda.synchronize()
    finally:
        dev.set_coalesce(1)
        dev.set_pipeline(1)
    for j, (which, wd, o, od) in enumerate(outs):
        if wd:
            _same(o.cpu().numpy(), od.cpu().numpy(), want[which], f"{name} R {R} call {j}")
        else:
            _same(o.cpu().numpy(), None, want[which], f"{name} R {R} call {j}")
            assert (od.cpu().numpy() == SENT).all(), f"call {j} asked for no distances"


def test_a_call_beyond_one_sub_batch(tk, oracle):
    name, R, k, a = "twins", 129, 64, "near5"
    _, ox, qn, qp = es.index(name)
    dev = _device(name)
    dev.set_groups(es.groups(name, a))
    ms = dev.max_sub_batch(k, N_PROBES, R)
    sel = np.tile(np.arange(NQ), -(-(ms + 37) // NQ))[:ms + 37]
    m = (np.arange(len(sel)) % 4).astype(np.int32)           # a cap of its own per row: the parts' offsets matter
    from per_group_reference import capped_from_heaps
    base = {c: capped_from_heaps(oracle, ox, qn, es.heaps(name, k, R), c, es.groups(name, a), k) for c in range(4)}
    want = tuple(np.stack([base[int(c)][part][i] for i, c in zip(sel, m)]) for part in range(3))
    assert len(sel) > ms
    ids, dist = dev.query_batch(np.ascontiguousarray(qn[sel]), np.ascontiguousarray(qp[sel]), k, N_PROBES, R,
                                return_distances=True, per_group=m)
    _same(ids, dist, want, ("beyond one sub-batch", ms, len(sel)))


# ---- the largest heap the library's own check admits -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["twins", "f64"])
def test_the_largest_admitted_heap(tk, oracle, name):
    """pass_1 = the largest R of api_index.hip's `per_group:` check (2336 for float32 at d = 20, 1815 for float64): a
    launch within 48 bytes of 64 KiB of LDS, every probed row of the index walked; one more is the argument error"""
    from tinyknn_amd import _lib
    d, dtype, _ = es.INDEXES[name]
    _, ox, qn, qp = es.index(name)
    dev = _device(name)
    R = es.largest_admitted_heap(d, np.dtype(dtype).itemsize)
    assert R == {"twins": 2336, "f64": 1815}[name]
    k, n_probes = es.LARGEST_K, es.LARGEST_PROBES
    for a, m in es.LARGEST_LEGS:
        dev.set_groups(es.groups(name, a))
        want = es.reference(name, R, k, a, m, n_probes)
        _same(*dev.query_batch(qn, qp, k, n_probes, R, return_distances=True, per_group=m), want, (name, R, a, m))
        _same(dev.query_batch(qn, qp, k, n_probes, R, per_group=m), None, want, (name, R, a, m, "ids alone"))
    # one more entry: refused before anything is launched, the output as it was
    with pytest.raises(AssertionError, match="per_group"):
        dev.query_batch(qn, qp, k, n_probes, R + 1, per_group=1)
    out = np.full((NQ, k), -9, dtype=np.int64)
    ones = np.ones(NQ, dtype=np.int32)
    rc = _lib.lib().tk_index_query_batch_ex6(
        dev._h, None, None, None, None, 0, None, ones.ctypes.data, _lib.ptr(qn, _lib._f32p), qp.ctypes.data,
        int(qp.dtype != np.float32), NQ, k, n_probes, R + 1, _lib.ptr(out, _lib._i64p), None, None, None, None)
    assert rc == -1 and "per_group" in _lib.lib().tk_last_error().decode() and (out == -9).all()
    # (the uncapped call takes that heap: the check is the capped kernels' alone)
    assert dev.query_batch(qn, qp, k, n_probes, R + 1).shape == (NQ, k)
