"""References of the half store (store="float16"): an index that keeps its rescoring vectors in IEEE half answers,
bit for bit, what the same index answers on float32(float16(x)).  So the references are the unmodified oracle fed
the rounded rows, and the float32 "twin": the same IVF with `data` replaced by the rounded rows."""
import copy

import numpy as np

from conftest import split_lists


def rounded(X):
    """float32(float16(X)): numpy's round-to-nearest-even, subnormal halves kept"""
    return np.asarray(X, dtype=np.float32).astype(np.float16).astype(np.float32)


def fixture_ivf(g, data=None, store=None):
    """A g6_ivf_*.npz fixture as an IVF; data: its rescoring vectors (default: the fixture's)."""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import TransformedData
    codes, ids = split_lists(g)
    pq = FastPQ(2)
    pq.centers = g["pq_centers"]
    pq.sqrt_n_blocks = float(g["sqrt_n_blocks"])
    pq.R = g["R"] if "R" in g else None
    ivf = IVF(str(g["metric"]), len(codes), None)
    ivf.pq = pq
    ivf.active_centers = g["active_centers"]
    ivf.pq_transformed_centers = TransformedData(int(g["center_size"]), g["center_codes"])
    ivf.pq_transformed_points = [TransformedData(int(s), c) for s, c in zip(g["list_sizes"], codes)]
    ivf.ids = ids
    ivf.data = g["data"] if data is None else data
    ivf.store = store
    return ivf


def oracle_index(oracle, ivf, data):
    """The oracle's copy of a host-built IVF with `data` as its rescoring vectors."""
    L = len(ivf.active_centers)
    M = ivf.pq.centers.shape[1] // ivf.pq.dims_per_block
    pts = ivf.pq_transformed_points
    empty = np.zeros((0, M), dtype=np.uint64)
    return oracle.OracleIndex(ivf.pq.centers, 2, ivf.pq.R, ivf.pq.sqrt_n_blocks, ivf.active_centers,
                              ivf.pq_transformed_centers.packed,
                              [empty if isinstance(pts[i], np.ndarray) else pts[i].packed for i in range(L)],
                              [0 if isinstance(pts[i], np.ndarray) else pts[i].size for i in range(L)],
                              [np.asarray(ivf.ids[i], dtype=np.int64) for i in range(L)], data)


def host_copy(res, data):
    """A host IVF holding what an index built in HBM (build_resident) holds now — its centres, its exported lists
    and codes — with `data` as its vectors."""
    from tinyknn_amd import IVF
    from tinyknn_amd.ivf import _split_lists
    dev = res.device_index()
    ivf = IVF(res.metric, res.n_clusters, None)
    ivf.pq, ivf.all_centers = res.pq, res.all_centers
    ivf.active_centers, ivf.pq_transformed_centers = res.active_centers, res.pq_transformed_centers
    ivf.pq_transformed_points, ivf.ids = _split_lists(*dev.export_lists(), dev.d)
    ivf.list_columns = dev.list_columns()
    ivf.data = data
    return ivf


def twin(ivf):
    """The float32 twin of a host-built IVF: the same lists, codes and centres (shared), the rounded rows as
    float32 vectors, no device copy yet."""
    t = copy.copy(ivf)
    t._dev = None
    t.store = None
    t.data = rounded(ivf.data)
    return t


def exact_distances(oracle, qn, data, ids):
    """knn_brute1's float32 distances of the ids (+inf beside -1) on `data`, as the oracle sums them."""
    out = np.full(ids.shape, np.inf, dtype=np.float32)
    for i in range(len(ids)):
        live = ids[i] != -1
        out[i][live] = oracle.sqdist_gather(qn[i], data, ids[i][live]).astype(np.float32)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
