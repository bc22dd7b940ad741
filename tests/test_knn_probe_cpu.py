"""IVF.knn_probe / DeviceIndex.knn_probe: what Python refuses, before any device call."""
import numpy as np
import pytest


def test_refusals_come_before_any_device_call():
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.ivf import AllowSet, DeviceIndex
    ivf = IVF("angular", 4, FastPQ(2))

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    ivf.device_index = ivf._prepare = no_device
    Q = np.zeros((3, 4), np.float32)
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="k in"):
            ivf.knn_probe(Q, bad, 2)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="n_probes"):
            ivf.knn_probe(Q, 5, bad)
    with pytest.raises(TypeError, match="AllowSet"):
        ivf.knn_probe(Q, 5, 2, allowed=object.__new__(AllowSet))
    with pytest.raises(AssertionError, match="a device call was made"):       # a good call reaches the device
        ivf.knn_probe(Q, 5, 2)
    dev = object.__new__(DeviceIndex)
    dev.d, dev.dq, dev.N, dev.world, dev._source = 4, 4, 10, 1, None
    with pytest.raises(ValueError, match="k in"):
        dev.knn_probe(Q, Q, 0, 2)
    with pytest.raises(ValueError, match="n_probes"):
        dev.knn_probe(Q, Q, 5, 0)
    with pytest.raises(TypeError, match="AllowSet"):
        dev.knn_probe(Q, Q, 5, 2, allowed=object.__new__(AllowSet))
    dev.world = 2                                                               # a rank of a list-sharded index
    with pytest.raises(RuntimeError, match="list-sharded"):
        dev.knn_probe(Q, Q, 5, 2)
