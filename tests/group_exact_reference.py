"""References of the exact search inside a query's own group (tk_index_knn_group), NumPy and the CPU
oracle, no GPU.  Query i ranks the rows that carry its group, are stored and pass its other restrictions by the
rescoring's distance (oracle.sqdist_gather: numpy's einsum order) and returns the k smallest (distance, row id)."""
import numpy as np

from brute_restricted_reference import passes
from store_reference import rounded


def stored_mask(ids_per_list, n):
    """bool (n,): some list holds the row's id (labels outside [0, n) are no rows)"""
    out = np.zeros(n, dtype=bool)
    for ids in ids_per_list:
        ids = np.asarray(ids, dtype=np.int64)
        out[ids[(ids >= 0) & (ids < n)]] = True
    return out


def reference_data(data, store=None):
    """The vectors the index ranks by: float32(float16(data)) for the half store, else the data as they are"""
    return rounded(data) if store == "float16" else np.asarray(data)


def knn_group_reference(oracle, qn, data, k, group, groups, stored=None, **restrictions):
    """(ids (nq, k) int64, dist (nq, k)) — dist float32, float64 for float64 data; -1 / +inf behind fewer than k rows.
    restrictions: the keywords of brute_restricted_reference.passes but group / groups."""
    qn = np.ascontiguousarray(qn, dtype=np.float32)
    data = np.ascontiguousarray(data)
    n = len(data)
    group, groups = np.asarray(group), np.asarray(groups)
    stored = np.ones(n, dtype=bool) if stored is None else np.asarray(stored, dtype=bool)
    dt = np.float64 if data.dtype == np.float64 else np.float32
    ids = np.full((len(qn), k), -1, dtype=np.int64)
    dist = np.full((len(qn), k), np.inf, dtype=dt)
    for i in range(len(qn)):
        assert group[i] >= 0
        rows = np.flatnonzero(passes(i, n, **restrictions) & (groups == group[i]) & stored)
        if not len(rows):
            continue
        dv = oracle.sqdist_gather(qn[i], data, rows).astype(dt)
        order = np.lexsort((rows, dv))[:k]
        ids[i, :len(order)] = rows[order]
        dist[i, :len(order)] = dv[order]
    return ids, dist


def same_bits(a, b):
    """equal shapes, dtypes and bit patterns (float32 or float64)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return np.array_equal(a.view(u), b.view(u))


def einsum_distances(qn, data, ids):
    """numpy's own einsum("ij,ij->i") squared distances of the ids (+inf beside -1), in numpy's promotion"""
    data = np.asarray(data)
    dt = np.float64 if data.dtype == np.float64 else np.float32
    out = np.full(ids.shape, np.inf, dtype=dt)
    for i in range(len(ids)):
        live = ids[i] >= 0
        diff = data[ids[i][live]] - qn[i]
        out[i][live] = np.einsum("ij,ij->i", diff, diff)
    return out


def append_model(dist_rows, k, tile, cap):
    """What the kernel's candidate buffer sees for ONE query: dist_rows — the distances of the surviving rows at their
    positions in the group's span, NaN at the positions of dropped rows (they take a lane and no slot).  A lane appends
    its row where the distance is not above the bound; in front of a tile, when the entries the buffer may hold (those
    after the last cut + `tile` per tile since) plus one more tile would pass `cap`, the buffer is cut to its k best
    and the bound becomes the k-th distance.  -> (cuts in front of tiles, the most entries the buffer ever held)."""
    dist_rows = np.asarray(dist_rows, dtype=np.float64)
    held = np.zeros(0)
    tau, kept, cuts, most = np.inf, 0, 0, 0
    for t0 in range(0, len(dist_rows), tile):
        if kept + tile > cap:
            held = np.sort(held)[:k]
            if len(held) >= k:
                tau = held[k - 1]
            kept = len(held)
            cuts += 1
        kept += tile
        seg = dist_rows[t0:t0 + tile]
        seg = seg[~np.isnan(seg)]
        held = np.concatenate([held, seg[seg <= tau]])
        most = max(most, len(held))
    return cuts, most
