"""store="float16" without a GPU: the argument and its persistence, what a host build keeps (everything but the
device copy of the vectors is the store=None build's), the refusals decided on the host, the C ABI's declarations
and the register budget of the half rescoring kernel."""
import os
import pickle
import re

import numpy as np
import pytest

from kernel_usage import have_hipcc, kernel_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fitted(metric="euclidean", d=40, n=2000, clusters=20, seed=0):
    from tinyknn_amd import IVF, FastPQ
    X = np.random.RandomState(seed).randn(n, d).astype(np.float32)
    ivf = IVF(metric, clusters, FastPQ(2))
    np.random.seed(seed)
    ivf.fit(X[:1500])
    return ivf, X


def _built(ivf, X, **kw):
    from tinyknn_amd import IVF, FastPQ
    out = IVF(ivf.metric, ivf.n_clusters, FastPQ(2))
    out.all_centers, out.pq = ivf.all_centers, ivf.pq
    return out.build(X, n_probes=2, device=False, **kw)


@pytest.mark.parametrize("metric", ["euclidean", "angular"])
def test_host_build_keeps_everything_but_the_device_format(metric):
    ivf, X = _fitted(metric)
    X = X * np.float32(1.0 + 2.0 ** -12)           # values that are no halfs
    plain = _built(ivf, X, store=None)
    half = _built(ivf, X, store="float16")
    named = _built(ivf, X, store="float32")
    assert (plain.store, half.store, named.store) == (None, "float16", "float32")
    # IVF.data: the caller's dtype, unrounded
    assert half.data.dtype == np.float32
    np.testing.assert_array_equal(half.data, plain.data)
    assert not np.array_equal(half.data, half.data.astype(np.float16).astype(np.float32))
    # lists, codes, ids, centres: those of the store=None build
    L = len(plain.active_centers)
    assert len(half.active_centers) == L
    np.testing.assert_array_equal(half.active_centers, plain.active_centers)
    np.testing.assert_array_equal(half.pq_transformed_centers.packed, plain.pq_transformed_centers.packed)
    np.testing.assert_array_equal(half.list_columns, plain.list_columns)
    for i in range(L):
        np.testing.assert_array_equal(half.ids[i], plain.ids[i])
        np.testing.assert_array_equal(half.pq_transformed_points[i].packed, plain.pq_transformed_points[i].packed)


def test_store_survives_save_load_and_pickle(tmp_path):
    from tinyknn_amd import IVF
    ivf, X = _fitted()
    X = X * np.float32(1.0 + 2.0 ** -12)
    half = _built(ivf, X, store="float16")
    half.save(tmp_path / "h")
    back = IVF.load(tmp_path / "h")
    assert back.store == "float16"
    np.testing.assert_array_equal(back.data, half.data)             # the host vectors, unrounded
    assert str(np.load(tmp_path / "h.npz")["store"]) == "float16"
    again = pickle.loads(pickle.dumps(half))
    assert again.store == "float16"
    np.testing.assert_array_equal(again.data, half.data)
    # store=None writes no key, and a file without the key (written before store= existed) loads as None
    plain = _built(ivf, X, store=None)
    plain.save(tmp_path / "p")
    assert "store" not in np.load(tmp_path / "p.npz").files
    assert IVF.load(tmp_path / "p").store is None
    z = dict(np.load(tmp_path / "h.npz"))
    del z["store"]
    np.savez(tmp_path / "old.npz", **z)
    assert IVF.load(tmp_path / "old").store is None
    assert pickle.loads(pickle.dumps(plain)).store is None


@pytest.mark.parametrize("bad", [65520.0, -65520.0, np.inf, -np.inf, np.nan])
def test_a_value_whose_half_is_not_finite_is_refused_and_names_its_row(bad):
    ivf, X = _fitted()
    Xb = X.copy()
    Xb[1234, 7] = bad
    Xb[1500, 0] = bad               # (the FIRST offending row is named)
    before = dict(ivf.__dict__)
    with pytest.raises(ValueError, match=r"row 1234\b"):
        ivf.build(Xb, n_probes=2, device=False, store="float16")
    assert ivf.__dict__.keys() == before.keys() and all(ivf.__dict__[k] is before[k] for k in before), \
        "a refused build changes nothing"
    assert ivf.store is None and not hasattr(ivf, "data")


def test_the_largest_value_that_rounds_to_a_finite_half_is_accepted():
    from tinyknn_amd.ivf import half_rows
    ivf, X = _fitted()
    Xa = X.copy()
    Xa[3, 3] = 65519.0              # rounds to 65504, the largest half
    Xa[4, 4] = np.nextafter(np.float32(-65520.0), np.float32(0.0))
    got = _built(ivf, Xa, store="float16")
    assert got.store == "float16" and got.data[3, 3] == np.float32(65519.0)
    h = half_rows(Xa, "test")
    assert h.dtype == np.float16 and h[3, 3] == np.float16(65504.0) and h[4, 4] == np.float16(-65504.0)
    np.testing.assert_array_equal(h, Xa.astype(np.float16))         # numpy's rounding: ties to even, subnormals kept
    tiny = np.array([[2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -0.0]], np.float32)
    np.testing.assert_array_equal(half_rows(tiny, "test").view(np.uint16),
                                  np.array([[0x0001, 0x0000, 0x0002, 0x3c00, 0x3c02, 0x8000]], np.uint16))


def test_float64_vectors_and_unknown_formats_are_refused():
    ivf, X = _fitted()
    with pytest.raises(ValueError, match="float64"):
        ivf.build(X.astype(np.float64), n_probes=2, device=False, store="float16")
    for what in ("float8", "half", "bfloat16", 16, ""):
        with pytest.raises(ValueError, match="store"):
            ivf.build(X, n_probes=2, device=False, store=what)
    assert ivf.store is None and not hasattr(ivf, "data")
    # float64 vectors stay what they are under the other two values
    assert _built(ivf, X.astype(np.float64), store=None).data.dtype == np.float64
    assert _built(ivf, X.astype(np.float64), store="float32").data.dtype == np.float64


def test_host_add_on_a_half_index_refuses_before_anything_changes():
    ivf, X = _fitted()
    half = _built(ivf, X, store="float16")
    ids0 = [np.array(i, copy=True) for i in half.ids[:len(half.active_centers)]]
    Y = X[:50].copy()
    Y[17, 2] = np.inf
    with pytest.raises(ValueError, match=r"row 2017\b"):
        half.add(Y)
    assert len(half.data) == len(X)
    for a, b in zip(ids0, half.ids):
        np.testing.assert_array_equal(a, b)
    half.add(X[:50] * np.float32(1.0 + 2.0 ** -12))
    assert len(half.data) == len(X) + 50 and half.store == "float16"
    np.testing.assert_array_equal(half.data[len(X):], X[:50] * np.float32(1.0 + 2.0 ** -12))    # unrounded


def test_header_declares_and_the_bindings_know_the_new_entries():
    from tinyknn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyknn_hip.h")).read()
    assert re.search(r"^#define TK_DATA_F16 2$", hdr, flags=re.M)
    assert re.search(r"^#define TK_DATA_F32 0$", hdr, flags=re.M) and re.search(r"^#define TK_DATA_F64 1$", hdr, flags=re.M)
    assert re.search(r"^int tk_index_narrow_data\(tk_index \*ix\);$", hdr, flags=re.M)
    assert re.search(r"^int tk_index_store\(tk_index \*ix\);$", hdr, flags=re.M)
    assert re.search(r"^int tk_index_set_data\(tk_index \*ix, const void \*data, int dtype, int64_t N, int d\);$", hdr,
                     flags=re.M)
    assert (_lib.DATA_F32, _lib.DATA_F64, _lib.DATA_F16) == (0, 1, 2)
    lib = _lib.lib()
    for name in ("tk_index_narrow_data", "tk_index_store"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes is not None


def test_half_rescoring_kernels_meet_the_float32_kernel_s_budget():
    """The default instantiation of the half staged kernel under its float32 sibling's pin (<= 128 VGPRs, >= 4 waves
    per SIMD, zero scratch, no spills); every half kernel of rescore.hip without scratch or spills."""
    if not have_hipcc():
        pytest.skip("hipcc not found")
    usage = kernel_usage("rescore.hip")
    pinned = {k: v for k, v in usage.items() if "rescore_staged_half_kernelILi32EE" in k}
    assert len(pinned) == 1, sorted(usage)
    for name, u in pinned.items():
        assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (name, u)
        assert u["Occupancy"] >= 4, (name, u)
    half = {k: v for k, v in usage.items() if "half" in k or "DF16_" in k}
    # staged ids / distances at tiles of 32 and 64, the lane-per-row kernel's two forms on half rows
    assert len(half) == 6, sorted(half)
    for name, u in half.items():
        assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
