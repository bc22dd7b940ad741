"""Row groups without a GPU: the reference helper is the guarded reference with the set `groups == g` per query; the
Python layer's validation, add(groups=) bookkeeping and persistence; the ABI's declarations; the kernels of groups.hip
compile for gfx950 without scratch or spills.  (tk_index_create needs a GPU, so the ABI's TK_ERR_STATE refusals are
in tests/test_groups_gpu.py.)"""
import os
import pickle
import re
import sys
import time
import weakref

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from allowed_reference import guarded_batch  # noqa: E402
from conftest import golden, split_lists  # noqa: E402
from groups_reference import grouped_batch  # noqa: E402
from kernel_usage import kernel_usage  # noqa: E402

KEYS = ("probes", "heap_idx", "heap_val")


@pytest.fixture(scope="module")
def fixture(oracle):
    g = golden("g6_ivf_an100b2.npz")
    codes, ids = split_lists(g)
    R = g["R"] if "R" in g else None
    ox = oracle.OracleIndex(g["pq_centers"], 2, R, float(g["sqrt_n_blocks"]), g["active_centers"],
                            g["center_codes"], codes, g["list_sizes"], ids, g["data"])
    groups = np.random.default_rng(1).integers(0, 7, len(g["data"])).astype(np.int32)
    return ox, np.ascontiguousarray(g["qn"][:24]), groups


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    for key in KEYS:
        np.testing.assert_array_equal(a[1][key], b[1][key], err_msg=key)


def test_helper_all_unrestricted_is_the_unrestricted_reference(oracle, fixture):
    ox, qn, groups = fixture
    want = guarded_batch(oracle, ox, qn, 10, 5, debug=True)
    _same(grouped_batch(oracle, ox, qn, np.full(len(qn), -1), groups, 10, 5, debug=True), want)
    _same(grouped_batch(oracle, ox, qn, -1, groups, 10, 5, debug=True), want)


def test_helper_one_group_is_the_guarded_reference_of_that_set(oracle, fixture):
    ox, qn, groups = fixture
    N = len(groups)
    want = guarded_batch(oracle, ox, qn, 10, 5, allowed=groups == 3, debug=True)
    got = grouped_batch(oracle, ox, qn, np.full(len(qn), 3), groups, 10, 5, debug=True)
    _same(got, want)
    ids = got[0][got[0] != -1]
    assert ids.size and (groups[ids] == 3).all()
    assert (want[0] != guarded_batch(oracle, ox, qn, 10, 5)).any()
    # mixed: every row is its own group's; a group nobody carries returns nothing
    mixed = np.arange(len(qn)) % 9 - 1         # -1, 0 .. 6 and 7, which no row carries
    got = grouped_batch(oracle, ox, qn, mixed, groups, 10, 5)
    for g in range(-1, 7):
        sel = mixed == g
        np.testing.assert_array_equal(
            got[sel], guarded_batch(oracle, ox, qn[sel], 10, 5, allowed=None if g == -1 else groups == g))
    assert (got[mixed == 7] == -1).all()
    # with a set and an excluded row as well: the intersection
    allowed = np.arange(N) % 2 == 0
    first = grouped_batch(oracle, ox, qn, 3, groups, 10, 5, allowed=allowed)[:, 0]
    assert (first >= 0).all()
    got = grouped_batch(oracle, ox, qn, 3, groups, 10, 5, allowed=allowed, exclude=first)
    for i in range(len(qn)):
        m = (groups == 3) & allowed
        m[first[i]] = False
        np.testing.assert_array_equal(got[i:i + 1], guarded_batch(oracle, ox, qn[i:i + 1], 10, 5, allowed=m))


# ---- the Python layer ----

def _built(kp=1, n=2000, d=40, clusters=20, seed=0):
    from tinyknn_amd import IVF, FastPQ
    X = np.random.RandomState(seed).randn(n + 300, d).astype(np.float32)
    ivf = IVF("angular", clusters, FastPQ(2))
    np.random.seed(seed)
    ivf.fit(X[:1500])
    ivf.build(X[:n], n_probes=kp, device=False)
    return ivf, X[n:]


def test_set_groups_validation():
    ivf, _ = _built()
    N = len(ivf.data)
    assert ivf.groups is None and "groups" not in vars(ivf)
    for bad in (np.zeros(N), np.zeros(N, dtype=bool), np.zeros((N, 1), dtype=np.int64), "tenants", 3):
        with pytest.raises(TypeError):
            ivf.set_groups(bad)
    for bad in (np.zeros(N - 1, dtype=np.int64), np.zeros(N + 1, dtype=np.int32), np.full(N, -1),
                np.full(N, 2**31 - 1, dtype=np.int64), np.full(N, 2**40, dtype=np.int64)):
        with pytest.raises(ValueError):
            ivf.set_groups(bad)
    assert ivf.groups is None
    g = np.arange(N, dtype=np.int64) % 5
    g[0] = 2**31 - 2                    # the largest id
    assert ivf.set_groups(g) is ivf
    assert ivf.groups.dtype == np.int32 and np.array_equal(ivf.groups, g)
    g32 = g.astype(np.int32)
    ivf.set_groups(g32)
    g32[1] = 77                         # the index keeps its own copy
    assert ivf.groups[1] == 1
    ivf.set_groups(None)
    assert ivf.groups is None and "groups" not in vars(ivf)


def test_add_groups_bookkeeping():
    ivf, more = _built()
    N = len(ivf.data)
    with pytest.raises(ValueError, match="without groups"):
        ivf.add(more[:10], groups=np.zeros(10, dtype=np.int64))
    assert len(ivf.data) == N
    g = (np.arange(N) % 4).astype(np.int32)
    ivf.set_groups(g)
    ids_before = [np.array(x, copy=True) for x in ivf.ids[:len(ivf.active_centers)]]
    with pytest.raises(ValueError, match="groups"):
        ivf.add(more[:10])
    with pytest.raises(ValueError):
        ivf.add(more[:10], groups=np.zeros(9, dtype=np.int64))
    with pytest.raises(ValueError):
        ivf.add(more[:10], groups=np.full(10, -1))
    with pytest.raises(TypeError):
        ivf.add(more[:10], groups=np.zeros(10))
    assert len(ivf.data) == N and np.array_equal(ivf.groups, g)      # refused before anything changed
    for a, b in zip(ids_before, ivf.ids):
        np.testing.assert_array_equal(a, b)
    ivf.add(more[:10], groups=np.arange(10) + 100)
    assert len(ivf.data) == N + 10 and ivf.groups.dtype == np.int32
    np.testing.assert_array_equal(ivf.groups, np.concatenate([g, np.arange(10) + 100]))
    ivf.add(more[:0], groups=np.zeros(0, dtype=np.int64))
    assert len(ivf.groups) == N + 10
    # an index without groups: add as before
    plain, more = _built()
    plain.add(more[:10])
    assert plain.groups is None and len(plain.data) == N + 10
    # a new build drops the groups of the rows before
    ivf.build(np.asarray(ivf.data[:500]), n_probes=1, device=False)
    assert ivf.groups is None


def test_save_load_and_pickle_carry_groups(tmp_path, monkeypatch):
    from tinyknn_amd import IVF
    stamp = time.localtime(86400 * 365 * 30)
    monkeypatch.setattr(time, "localtime", lambda *a: stamp)     # (the archive's member times: equal for every file)
    ivf, _ = _built(kp=2)
    N = len(ivf.data)
    ivf.save(tmp_path / "never")
    never = open(tmp_path / "never.npz", "rb").read()
    assert "groups" not in np.load(tmp_path / "never.npz").files
    assert IVF.load(tmp_path / "never").groups is None
    state_never = set(ivf.__getstate__())
    g = (np.arange(N) % 11).astype(np.int32)
    ivf.set_groups(g)
    ivf.save(tmp_path / "with")
    back = IVF.load(tmp_path / "with")
    assert back.groups.dtype == np.int32
    np.testing.assert_array_equal(back.groups, g)
    np.testing.assert_array_equal(back.list_columns, ivf.list_columns)
    twin = pickle.loads(pickle.dumps(ivf))
    np.testing.assert_array_equal(twin.groups, g)
    # cleared again: exactly the file, and the pickled state, of an index whose groups were never set
    ivf.set_groups(None)
    ivf.save(tmp_path / "cleared")
    assert open(tmp_path / "cleared.npz", "rb").read() == never
    assert set(ivf.__getstate__()) == state_never
    assert pickle.loads(pickle.dumps(ivf)).groups is None


N0, D, DQ = 40, 6, 8


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"{name}: a refused call must not reach the library")


@pytest.fixture
def bare(monkeypatch):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    dev = DeviceIndex.__new__(DeviceIndex)
    dev._h, dev.d, dev.dq, dev.dpb, dev.n_lists, dev.N = 0x10, D, DQ, 2, 3, N0
    dev.angular, dev._R, dev._f64, dev.rank, dev.world = False, None, False, 0, 1
    dev._streams, dev._live_streams, dev._live_allows = {}, weakref.WeakSet(), weakref.WeakSet()
    yield dev
    dev._h = None


def test_query_refusals_decided_on_the_host(bare):
    from tinyknn_amd import IVF
    qn, qp = np.zeros((5, D), np.float32), np.zeros((5, DQ), np.float32)
    with pytest.raises(ValueError, match="one entry per query"):
        bare.query_batch(qn, qp, 3, 1, group=[1, 2, 3])
    with pytest.raises(ValueError):
        bare.query_batch(qn, qp, 3, 1, group=[0, 1, 2, 3, -2])
    with pytest.raises(ValueError):
        bare.query_batch(qn, qp, 3, 1, group=-2)
    with pytest.raises(ValueError):
        bare.query_batch(qn, qp, 3, 1, group=2**31 - 1)
    for bad in (np.zeros((5, 1), np.int64), np.zeros(5), 0.5, np.zeros(5, dtype=bool)):
        with pytest.raises(TypeError):
            bare.query_batch(qn, qp, 3, 1, group=bad)
    with pytest.raises(ValueError):
        bare.set_groups(np.zeros(N0 + 1, dtype=np.int64))
    with pytest.raises(TypeError):
        bare.set_groups(np.zeros(N0))
    bare.world = 2
    with pytest.raises(RuntimeError, match="list-sharded"):
        bare.set_groups(np.zeros(N0, dtype=np.int64))
    bare.world = 1
    ivf = IVF("euclidean", 3, None)
    ivf._dev = bare
    ivf.data = np.zeros((N0, D), np.float32)
    with pytest.raises(NotImplementedError, match="group"):
        ivf.query_batch(qn, 3, fast=True, group=1)
    with pytest.raises(ValueError, match="one entry per query"):
        ivf.query_batch(qn, 3, group=np.arange(4))


# ---- the ABI and the kernels ----

def test_new_symbols_declared_and_exported():
    from tinyknn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tinyknn_hip.h")).read()
    declared = set(re.findall(r"\b(tk_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("tk_index_set_groups", "tk_index_groups", "tk_index_query_batch_ex3",
                 "tk_index_query_batch_dev_ex3", "tk_index_group_table"):
        assert name in declared, name
        assert hasattr(lib, name), f"{name} declared but not exported"
        assert name in _lib.SIGNATURES, name
    # the earlier entry points keep their signatures
    assert len(_lib.SIGNATURES["tk_index_query_batch_ex3"][1]) == len(_lib.SIGNATURES["tk_index_query_batch_ex2"][1]) + 1
    assert len(_lib.SIGNATURES["tk_index_query_batch_dev_ex3"][1]) == \
        len(_lib.SIGNATURES["tk_index_query_batch_dev_ex2"][1]) + 1
    # without a GPU no index exists to refuse anything: a null index is an argument error, nothing more
    assert lib.tk_index_set_groups(None, None, 0) == -1
    assert lib.tk_index_groups(None) == -1


def test_groups_kernels_compile_without_scratch_or_spills():
    usage = kernel_usage("groups.hip")
    names = " ".join(usage)
    for kernel in ("group_table_kernel", "group_pass_kernel"):
        assert kernel in names, names
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    # the allow pass shares the masking body (chunk_mask.h): still no scratch
    for name, u in kernel_usage("allow.hip").items():
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0, (name, u)
