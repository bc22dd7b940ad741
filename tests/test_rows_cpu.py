"""Excluded rows and stored rows as queries, without a GPU: the reference helper is the guarded reference with the set
"every row but e"; the Python layer's refusals; the kernels of rows.hip compile for gfx950 without scratch or spills."""
import os
import sys
import weakref

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from allowed_reference import guarded_batch, guarded_query  # noqa: E402
from conftest import golden, split_lists  # noqa: E402
from kernel_usage import kernel_usage  # noqa: E402
from rows_reference import excluded_batch, excluded_query  # noqa: E402


def _oracle_index(oracle, g):
    codes, ids = split_lists(g)
    R = g["R"] if "R" in g else None
    return oracle.OracleIndex(g["pq_centers"], 2, R, float(g["sqrt_n_blocks"]), g["active_centers"],
                              g["center_codes"], codes, g["list_sizes"], ids, g["data"])


@pytest.mark.parametrize("tag", ["an100b2", "eu20"])
def test_helper_is_the_guarded_reference_of_all_but_e(oracle, tag):
    g = golden(f"g6_ivf_{tag}.npz")
    ox = _oracle_index(oracle, g)
    N = len(g["data"])
    rows = np.random.default_rng(4).choice(N, 24, replace=False)
    qn = np.ascontiguousarray(g["data"][rows], dtype=np.float32)
    returned_itself = 0
    for n_probes in (1, 5):
        for q, r in zip(qn, rows):
            allowed = np.ones(N, dtype=bool)
            allowed[r] = False
            want, wd = guarded_query(oracle, ox, q, 10, n_probes, allowed=allowed, debug=True)
            got, gd = excluded_query(oracle, ox, q, r, 10, n_probes, debug=True)
            np.testing.assert_array_equal(got, want)
            for key in ("probes", "heap_idx", "heap_val"):
                np.testing.assert_array_equal(gd[key], wd[key], err_msg=key)
            assert r not in got
            returned_itself += int(r in guarded_query(oracle, ox, q, 10, n_probes))
            # e = -1: the unrestricted query; with a set as well: the intersection
            np.testing.assert_array_equal(excluded_query(oracle, ox, q, -1, 10, n_probes),
                                          guarded_query(oracle, ox, q, 10, n_probes))
    assert returned_itself > 0      # (the unrestricted query of a stored row does return the row)
    half = np.arange(N) % 2 == 0
    both = half.copy()
    both[rows[0]] = False
    np.testing.assert_array_equal(excluded_query(oracle, ox, qn[0], rows[0], 10, 5, allowed=half),
                                  guarded_query(oracle, ox, qn[0], 10, 5, allowed=both))
    assert "pq_query" not in vars(ox)
    # a given q_pq replaces the oracle's own for that call only: its own q_pq changes nothing
    np.testing.assert_array_equal(
        excluded_batch(oracle, ox, qn, rows, 10, 5, q_pq=ox.pq_query(qn)), excluded_batch(oracle, ox, qn, rows, 10, 5))
    assert "pq_query" not in vars(ox)
    np.testing.assert_array_equal(excluded_batch(oracle, ox, qn, None, 10, 5), guarded_batch(oracle, ox, qn, 10, 5))


N, D, DQ = 40, 6, 8


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"{name}: a refused call must not reach the library")


@pytest.fixture
def bare(monkeypatch):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    dev = DeviceIndex.__new__(DeviceIndex)
    dev._h, dev.d, dev.dq, dev.dpb, dev.n_lists, dev.N = 0x10, D, DQ, 2, 3, N
    dev.angular, dev._R, dev._f64, dev.rank, dev.world = False, None, False, 0, 1
    dev._streams, dev._live_streams, dev._live_allows = {}, weakref.WeakSet(), weakref.WeakSet()
    yield dev
    dev._h = None


def test_python_refusals(bare):
    from tinyknn_amd import IVF
    qn, qp = np.zeros((5, D), np.float32), np.zeros((5, DQ), np.float32)
    for rows in ([N], [-1], [0, N + 3]):
        with pytest.raises(ValueError):
            bare.query_rows(rows, 3, 1)
        with pytest.raises(ValueError):
            bare.gather_queries(rows)
    with pytest.raises(TypeError):
        bare.query_rows(np.zeros(N, dtype=bool), 3, 1)
    with pytest.raises(TypeError):
        bare.query_rows([0.5], 3, 1)
    with pytest.raises(ValueError, match="one entry per query"):
        bare.query_batch(qn, qp, 3, 1, exclude=[1, 2, 3])
    with pytest.raises(ValueError):
        bare.query_batch(qn, qp, 3, 1, exclude=[0, 1, 2, 3, N])
    with pytest.raises(ValueError):
        bare.query_batch(qn, qp, 3, 1, exclude=[0, 1, 2, 3, -2])
    with pytest.raises(TypeError):
        bare.query_batch(qn, qp, 3, 1, exclude=np.zeros((5, 1), np.int64))
    ivf = IVF("euclidean", 3, None)
    ivf._dev = bare
    ivf.data = np.zeros((N, D), np.float32)
    with pytest.raises(NotImplementedError):
        ivf.query_batch(qn, 3, fast=True, exclude=np.arange(5))
    with pytest.raises(ValueError):
        ivf.query_rows([N], 3)
    with pytest.raises(ValueError, match="one entry per query"):
        ivf.query_batch(qn, 3, exclude=np.arange(4))


def test_rows_kernels_compile_without_scratch_or_spills():
    usage = kernel_usage("rows.hip")
    names = " ".join(usage)
    for kernel in ("row_pos_fill_kernel", "exclude_pass_kernel"):
        assert kernel in names, names
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
