"""Distances beside the ids, CPU side: the C ABI declares and binds the three entry points, the Python calls refuse
the combinations they do not support before any device work, and the distance-writing rescoring kernels stay within
the staged kernel's register budget, without scratch (read from the compiler, as test_kernel_resources does)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from kernel_usage import have_hipcc, kernel_usage

ENTRY_POINTS = {
    "tk_index_query_batch_dist": 11,
    "tk_index_query_batch_dev_dist": 13,
    "tk_index_top_centers_dist": 8,
}


def test_header_declares_and_lib_binds_the_entry_points():
    from tinyknn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tinyknn_hip.h")).read()
    for name, n_args in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} not declared in tinyknn_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == n_args, name
        assert hasattr(_lib.lib(), name), f"{name} not exported"
    # the header states the element type of the distances and the padding
    i = header.index("tk_index_query_batch_dist")
    doc = header[header.rindex("/*", 0, i):i]
    assert "float64" in doc and "+inf" in doc


def test_unsupported_combinations_are_refused_before_device_work():
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import FlatTop
    from tinyknn_amd.ivf import DeviceIndex
    ivf = IVF("angular", 4, FastPQ(2))          # (never fitted: nothing reaches the device)
    with pytest.raises(NotImplementedError, match="fast=True"):
        ivf.query_batch(np.zeros((2, 4), np.float32), 1, fast=True, return_distances=True)
    with pytest.raises(ValueError, match="debug"):
        DeviceIndex.query_batch(object.__new__(DeviceIndex), np.zeros((1, 4), np.float32),
                                np.zeros((1, 4), np.float32), 1, 1, debug=True, return_distances=True)
    # keyword-only, off by default
    assert IVF.query.__kwdefaults__["return_distances"] is False
    assert IVF.query_batch.__kwdefaults__["return_distances"] is False
    assert DeviceIndex.query_batch.__kwdefaults__["return_distances"] is False
    assert DeviceIndex.query_batch_dev.__kwdefaults__["dist_ptr"] is None
    assert FlatTop.top.__kwdefaults__["return_distances"] is False


def test_out_of_scope_calls_do_not_take_the_option():
    from tinyknn_amd.ivf import DeviceIndex, QueryStream
    from tinyknn_amd.multi_gpu import ListShardedIndex, ReplicaGroup
    for f in (QueryStream.submit, DeviceIndex.query_raw, DeviceIndex.query_batch_raw, DeviceIndex.knn_brute,
              ListShardedIndex.query_batch, ReplicaGroup.query_batch):
        code = f.__code__
        names = code.co_varnames[:code.co_argcount + code.co_kwonlyargcount]
        assert "return_distances" not in names and not (code.co_flags & 0x08), f.__qualname__


def test_distance_kernels_resources():
    if not have_hipcc():
        pytest.skip("hipcc not found")
    usage = kernel_usage("rescore.hip")
    staged = {k: v for k, v in usage.items() if "rescore_staged_dist_kernelILi32EE" in k}
    assert staged, sorted(usage)
    for name, u in staged.items():
        assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u["VGPRs"] + u.get("AGPRs", 0) <= 128, (name, u)
        assert u["Occupancy"] >= 4, (name, u)
    dist = {k: v for k, v in usage.items() if "dist_kernel" in k}
    assert len(dist) == 6, sorted(dist)        # staged tiles of 32 and 64, the lane kernel's four dtype forms
    for name, u in dist.items():
        assert u.get("ScratchSize") == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
