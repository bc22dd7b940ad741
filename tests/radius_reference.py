"""Reference for the radius search (tk_index_radius_brute), plain NumPy, no GPU.
tests/test_radius_cpu.py checks it against a slower, more obvious form."""
import numpy as np

from brute_restricted_reference import passes  # noqa: F401  (the restrictions are knn_brute's)


def radius_list(part_row, ok, r):
    """The hits of one query: the passing rows with float32(part) <= float32(r), ascending by (part, row) -> (ids
    int64, part float32).  part_row: the query's part values over all rows (exact integers or float32), ok: bool mask
    of the rows the query may return (or None: all)."""
    part = np.asarray(part_row).astype(np.float32)
    hit = part <= np.float32(r)
    if ok is not None:
        hit &= np.asarray(ok, dtype=bool)
    rows = np.flatnonzero(hit)                                  # ascending by row; the stable sort keeps that in ties
    rows = rows[np.argsort(part[rows], kind="stable")]
    return rows.astype(np.int64), part[rows]


def radius_csr(part, oks, radius):
    """radius_list for every query, as the call returns it: (lims (nq + 1,) int64, ids int64, part float32).
    oks: one mask per query, or None; radius: a scalar or one value per query."""
    nq = len(part)
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,))
    lists = [radius_list(part[i], None if oks is None else oks[i], radius[i]) for i in range(nq)]
    lims = np.zeros(nq + 1, dtype=np.int64)
    lims[1:] = np.cumsum([len(ids) for ids, _ in lists])
    ids = np.concatenate([ids for ids, _ in lists]) if nq else np.zeros(0, np.int64)
    dist = np.concatenate([d for _, d in lists]) if nq else np.zeros(0, np.float32)
    return lims, ids.astype(np.int64), dist.astype(np.float32)
