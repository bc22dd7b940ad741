"""The device front end ("fast mode": tk_index_prepare_dev, tk_index_query_batch_raw; normalise_rows_kernel,
pad_rows_kernel and rotate_rows_kernel in build.hip) against plain references of the same operations
(tests/front_reference.py, themselves checked on the CPU by tests/test_fast_front_end_cpu.py):
  the normalisation bit for bit against the stated summation order, and within a derived bound of float64;
  the padding exactly; the rotation bit for bit against an exact FMA chain, and within a derived bound of the
  float64 product; fast mode == the exact pipeline run on the device-prepared rows; refusals leave the index usable.
normalise_rows_kernel is also what IVF.build(device=True) and IVF.add normalise angular rows with."""
import os
import subprocess
import sys

import numpy as np
import pytest

from front_reference import (bits32, bits64, front_rows, normalise_bound, normalise_rows, normalise_rows_f64,  # noqa: E402
                             ordinary, pad_rows, rotate_rows_f64, rotate_rows_fma, rotation_bound)

pytestmark = pytest.mark.gpu


def _index(d, dq, R=None, n=16):
    """a DeviceIndex that only needs its PQ geometry (as test_brute_gpu.py::_index: one list holding everything),
    plus pq.R (dq, d_pad) when the table-build query is rotated"""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import TransformedData
    from tinyknn_amd._transform import transform_data
    ivf = IVF("euclidean", 1, FastPQ(2))
    ivf.pq.centers = np.zeros((16, dq), np.float32)
    ivf.pq.sqrt_n_blocks = float(np.sqrt(dq // 2))
    ivf.pq.R = R
    ivf.active_centers = np.zeros((1, d), np.float32)
    ivf.pq_transformed_centers = TransformedData(1, transform_data(np.zeros((16, dq // 2), np.uint8)))
    ivf.pq_transformed_points = [TransformedData(n, transform_data(np.zeros((n + (-n) % 16, dq // 2), np.uint8)))]
    ivf.ids = [np.arange(n, dtype=np.int64)]
    ivf.data = np.zeros((n, d), np.float32)
    return ivf.device_index()


def _prepare_dev(dev, raw, angular, in_place=False, handle=None):
    """tk_index_prepare_dev on torch buffers, stream 0 -> (rc, qn, q_pq) back on the host.  The outputs start as
    a sentinel, so an element the kernels do not write shows."""
    import torch
    from tinyknn_amd import _lib
    nq, d = raw.shape
    f64 = getattr(dev, "_R", None) is not None
    raw_dev = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).cuda()
    qn_dev = raw_dev if in_place else torch.full((nq, d), 7.0, dtype=torch.float32, device="cuda")
    qpq_dev = torch.full((nq, dev.dq), 7.0, dtype=torch.float64 if f64 else torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = _lib.lib().tk_index_prepare_dev(dev._h if handle is None else handle, raw_dev.data_ptr(), nq, int(angular),
                                         qn_dev.data_ptr(), qpq_dev.data_ptr(), 0)
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(raw_dev.cpu().numpy().view(np.uint32), bits32(raw)), "the input was written to"
    return rc, qn_dev.cpu().numpy(), qpq_dev.cpu().numpy()


def _canon32(a):
    """uint32 view with every nan as one pattern: IEEE 754 leaves the sign and payload of the nan an invalid
    operation (0/0) returns to the implementation, and x86 and the GPU choose differently"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


NQS = [1, 128, 129, 1000]       # normalise_rows_kernel: 128 rows per workgroup


# ---- A1 / A2 / A3 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("nq", NQS)
def test_normalisation_bit_for_bit_and_padding(nq, in_place):
    """every d in 1..128: qn == the stated order in float32 (uint32 views; rows whose squares underflow or
    overflow, zero rows and one-element rows included) and q_pq == qn followed by zeros, exactly"""
    for d in range(1, 129):
        dq = d + (-d) % 8
        dev = _index(d, dq)
        raw = front_rows(nq, d, 1000 * d + nq)
        want = normalise_rows(raw)
        rc, qn, qpq = _prepare_dev(dev, raw, True, in_place)
        assert rc == 0
        bad = np.flatnonzero((_canon32(qn) != _canon32(want)).any(axis=1))
        assert len(bad) == 0, (d, nq, bad[:10], raw[bad[0]], qn[bad[0]], want[bad[0]])
        assert qpq.dtype == np.float32 and qpq.shape == (nq, dq)
        assert np.array_equal(_canon32(qpq), _canon32(pad_rows(want, dq))), (d, nq)
        dev.close()


def test_normalisation_within_the_derived_bound_of_float64():
    """ordinary rows against x / sqrt(sum x^2) in float64; the bound comes from the depth of the summation
    (front_reference.normalise_bound), not from a measurement — NumPy and the kernel cannot share a flaw here"""
    for d in range(1, 129):
        dev = _index(d, d + (-d) % 8)
        raw = front_rows(1000, d, d)[ordinary(1000)]
        ref = normalise_rows_f64(raw)
        rc, qn, _ = _prepare_dev(dev, raw, True)
        assert rc == 0
        err = np.abs(qn.astype(np.float64) - ref)
        assert (err <= normalise_bound(d) * np.abs(ref)).all(), (d, (err / np.abs(ref)).max(), normalise_bound(d))
        dev.close()


@pytest.mark.parametrize("d,dq", [(16, 16), (24, 24), (20, 24), (100, 104), (1, 8), (128, 128), (127, 128), (300, 304)])
@pytest.mark.parametrize("nq", [1, 257])
def test_padding_and_copy_are_exact(d, dq, nq):
    """unrotated: q_pq (nq, dq) float32 = qn then zeros (dq = d included); the euclidean case copies the raw
    rows exactly, into another buffer and in place"""
    dev = _index(d, dq)
    raw = front_rows(nq, d, d + nq)
    for in_place in (False, True):
        rc, qn, qpq = _prepare_dev(dev, raw, False, in_place)
        assert rc == 0
        assert np.array_equal(bits32(qn), bits32(raw))
        assert qpq.dtype == np.float32 and np.array_equal(bits32(qpq), bits32(pad_rows(raw, dq)))
    if d <= 128:
        rc, qn, qpq = _prepare_dev(dev, raw, True)
        assert rc == 0 and np.array_equal(_canon32(qpq), _canon32(pad_rows(qn, dq)))


# ---- A4 ----------------------------------------------------------------------------------------------------------------
ROTATIONS = [(128, 0, 64, False, 131), (128, 0, 64, True, 131), (100, 4, 64, True, 131), (20, 4, 16, False, 131),
             (11, 5, 8, True, 131), (300, 4, 64, False, 131),      # test_front_end.py's shapes
             (100, 4, 128, True, 131),                               # two passes of the 64-lane loop
             (40, 0, 72, False, 131),                                # a partial second pass
             (100, 4, 64, True, 1), (20, 4, 72, False, 1)]           # one query


@pytest.mark.parametrize("d,pad,rd,angular,nq", ROTATIONS)
def test_rotation_bit_for_bit_and_within_bound(d, pad, rd, angular, nq):
    """q_pq[i][j] = the float64 FMA chain over t ascending of (double) qn[i][t] * R[j][t]: bit for bit against exact
    rational FMAs on a subset of rows (all columns), and every output within gamma_{d_pad} * sum |x_t R_jt| of the
    float64 product.  Rows: one of zeros, rows mixing 1e-20 and 1e20 (cancellation), ordinary ones."""
    rng = np.random.RandomState(d + rd + nq)
    d_pad = d + pad
    R = rng.randn(rd, d_pad)
    raw = rng.randn(nq, d).astype(np.float32)
    exact_rows = [0]
    if nq > 1:
        if not angular:
            raw[1] = 0                                               # (a zero row normalises to nan)
        for i in (2, 3, 70):
            raw[i] = np.where(rng.rand(d) < 0.5, 1e-20, 1e20) * np.sign(rng.randn(d))
        raw[3, ::2] = rng.randn(len(raw[3, ::2]))                    # 1e-20, 1e20 and ordinary entries in one row
        exact_rows = [0, 1, 2, 3, 64, 70, nq - 1]
    dev = _index(d, rd, R)
    rc, qn, qpq = _prepare_dev(dev, raw, angular)
    assert rc == 0 and qpq.dtype == np.float64 and qpq.shape == (nq, rd)
    if angular:
        assert np.array_equal(_canon32(qn), _canon32(normalise_rows(raw)))
    else:
        assert np.array_equal(bits32(qn), bits32(raw))
    assert np.isfinite(qn).all()
    want = rotate_rows_fma(qn[exact_rows], R, d_pad)
    assert np.array_equal(bits64(qpq[exact_rows]), bits64(want)), np.argwhere(qpq[exact_rows] != want)[:5]
    if nq > 1 and not angular:
        assert not qpq[1].any()
    # the float64 product's own rounding obeys the same bound; the requirement is kept at one gamma, not two
    assert (np.abs(qpq - rotate_rows_f64(qn, R, d_pad)) <= rotation_bound(qn, R, d_pad)).all()


# ---- A5 ----------------------------------------------------------------------------------------------------------------
def _fixture_index(tag):
    from conftest import golden
    from test_hip_parity import ivf_from_fixture
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = ivf_from_fixture(None, g)
    return g, ivf, ivf.device_index()


@pytest.mark.parametrize("tag", ["an100", "an20", "eu20", "eu128"])
def test_fast_mode_is_the_exact_pipeline_on_device_prepared_rows(tag):
    g, ivf, dev = _fixture_index(tag)
    qs = np.ascontiguousarray(g["qs"], dtype=np.float32)
    rc, qn, qpq = _prepare_dev(dev, qs, dev.angular)
    assert rc == 0 and qpq.dtype == (np.float64 if "R" in g else np.float32)
    for n_probes in (1, 5, 10):
        fast = dev.query_batch_raw(qs, 10, n_probes)
        np.testing.assert_array_equal(fast, dev.query_batch(qn, qpq, 10, n_probes), err_msg=f"{tag} {n_probes}")
        assert (fast >= 0).any()


CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import conftest  # noqa: F401  (the suite's defaults)
from tinyknn_amd import _lib
from test_fast_front_end_gpu import _fixture_index, _prepare_dev
assert _lib.device_count() >= 1, "no GPU visible"
seen = []
for tag in ("an100", "an20", "eu20", "eu128"):
    g, ivf, dev = _fixture_index(tag)
    rng = np.random.RandomState(len(tag))
    for n_probes in (1, 5, 10):
        ms = dev.max_sub_batch(10, n_probes)
        nq = 2 * ms + 5                                    # three parts
        base = np.asarray(g["qs"], dtype=np.float32)
        qs = (base[rng.randint(len(base), size=nq)] * (1 + 0.05 * rng.randn(nq, base.shape[1]))).astype(np.float32)
        rc, qn, qpq = _prepare_dev(dev, qs, dev.angular)
        assert rc == 0
        fast = dev.query_batch_raw(qs, 10, n_probes)
        exact = dev.query_batch(qn, qpq, 10, n_probes)
        bad = int((fast != exact).any(axis=1).sum())
        assert bad == 0, (tag, n_probes, bad)
        assert len(np.unique(fast[:, 0])) > 10
        seen.append((ms, nq))
    dev.close()
print("FAST_SUB_BATCH_OK", min(nq - ms for ms, nq in seen), max(ms for ms, nq in seen))
'''


def test_fast_mode_over_several_sub_batches(tmp_path):
    """the same with a batch of 2 * max_sub_batch + 5 rows and the smallest workspace (read once per process,
    hence the child, as tests/test_sub_batch_gpu.py): tk_index_query_batch_raw prepares the whole batch, then
    the pipeline cuts it"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, TINYKNN_WORKSPACE_GB="0.25")
    r = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "FAST_SUB_BATCH_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert int(r.stdout.split("FAST_SUB_BATCH_OK")[1].split()[0]) > 0


# ---- A6 ----------------------------------------------------------------------------------------------------------------
def _answers_the_goldens(g, dev):
    for n_probes in (1, 10):
        np.testing.assert_array_equal(dev.query_batch(g["qn"], g["qpq"], 10, n_probes), g[f"ids_p{n_probes}"])


def test_refusals_leave_the_index_usable():
    import torch
    from tinyknn_amd import _lib
    L = _lib.lib()
    # angular normalisation beyond d = 128 (one thread sums a row)
    dev = _index(136, 136)
    raw = front_rows(10, 136, 0)
    rc, qn, qpq = _prepare_dev(dev, raw, True)
    assert rc != 0 and b"d <= 128" in L.tk_last_error()
    assert (qn == 7.0).all() and (qpq == 7.0).all()                  # nothing was written
    rc, qn, qpq = _prepare_dev(dev, raw, False)                       # the same index, euclidean: fine
    assert rc == 0 and np.array_equal(bits32(qpq), bits32(raw))
    # a NULL buffer, on an index that then answers its goldens
    g, ivf, fdev = _fixture_index("an100")
    buf = torch.zeros((24, 104), dtype=torch.float32, device="cuda")
    for args in ((0, buf.data_ptr(), buf.data_ptr()), (buf.data_ptr(), 0, buf.data_ptr()),
                 (buf.data_ptr(), buf.data_ptr(), 0)):
        rc = L.tk_index_prepare_dev(fdev._h, args[0], 24, 1, args[1], args[2], 0)
        assert rc != 0 and b"buffers" in L.tk_last_error()
    _answers_the_goldens(g, fdev)
    np.testing.assert_array_equal(fdev.query_batch_raw(g["qs"], 10, 5).shape, (24, 10))
    # before set_pq / set_centers
    h = L.tk_index_create()
    assert h
    try:
        rc = L.tk_index_prepare_dev(h, buf.data_ptr(), 24, 1, buf.data_ptr(), buf.data_ptr(), 0)
        assert rc != 0 and b"set_pq" in L.tk_last_error()
    finally:
        L.tk_index_destroy(h)
    _answers_the_goldens(g, fdev)
