"""Reference for the radius search over the probed lists (tk_index_radius_probe): numpy and the oracle, no
GPU.  Per query, in this order: the oracle's probes for P; the lists they name (restricted_shapes.probed_lists: a -1
names the last list); the union of the labels in [0, N) at positions < list_n of those lists, without repeats;
brute_restricted_reference.passes; oracle.sqdist_gather in the store's type (the caller hands the rows the rescoring
reads: store_reference.rounded for the half store); <= radius; lexsort((rows, dist)).
tests/test_radius_probe_cpu.py checks it against a slower, more obvious form."""
import numpy as np

from brute_restricted_reference import passes  # noqa: F401  (the restrictions are knn_brute's)
from restricted_shapes import probed_lists


def oracle_probes(ox, qn, n_probes):
    """(nq, min(P, n_lists)) int64: every query's probes row as the oracle's coarse stage gives it (it depends on P
    alone; k = 1 is the cheapest query that reports it)"""
    kc = min(int(n_probes), ox.n_lists)
    out = np.zeros((len(qn), kc), dtype=np.int64)
    for i, q in enumerate(qn):
        out[i] = ox.query(q, 1, int(n_probes), debug=True)[1]["probes"]
    return out


def list_labels(ox, l):
    """the labels list l of the oracle's index holds at positions < list_n"""
    return ox.ids[ox.ids_off[l]:ox.ids_off[l] + ox.list_n[l]] if ox.list_n[l] > 0 else np.zeros(0, np.int64)


def candidates(ox, probes_row, N):
    """the candidate rows of one probes row: ascending, each once"""
    lists = np.unique(probed_lists(probes_row, ox.n_lists))
    rows = np.concatenate([list_labels(ox, int(l)) for l in lists] + [np.zeros(0, np.int64)])
    rows = np.unique(rows)
    return rows[(rows >= 0) & (rows < N)]


def dist_dtype(data):
    return np.float64 if np.asarray(data).dtype == np.float64 else np.float32


def radius_probe_list(oracle, q, data, rows, ok, r):
    """The hits of one query among its candidate rows: (ids int64, dist in the store's type) ascending by (dist, id).
    ok: the bool mask over all N rows the query may return, or None."""
    dt = dist_dtype(data)
    if ok is not None:
        rows = rows[np.asarray(ok, dtype=bool)[rows]]
    dist = oracle.sqdist_gather(q, data, rows).astype(dt)      # (exact: float32 values where the store's type is float32)
    hit = dist <= dt(np.float32(r))
    rows, dist = rows[hit], dist[hit]
    order = np.lexsort((rows, dist))
    return rows[order].astype(np.int64), dist[order]


def radius_probe_csr(oracle, ox, qn, data, radius, n_probes, oks=None, probes=None):
    """The call's answer: (lims (nq + 1,) int64, ids int64, dist float32 — float64 on float64 vectors).  data: the rows
    the rescoring reads; radius: a scalar or one value per query; oks: one mask per query, or None; probes: the rows of
    oracle_probes where the caller has them already."""
    nq, N = len(qn), len(data)
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,))
    probes = oracle_probes(ox, qn, n_probes) if probes is None else probes
    lists = [radius_probe_list(oracle, qn[i], data, candidates(ox, probes[i], N), None if oks is None else oks[i],
                               radius[i]) for i in range(nq)]
    lims = np.zeros(nq + 1, dtype=np.int64)
    lims[1:] = np.cumsum([len(ids) for ids, _ in lists])
    dt = dist_dtype(data)
    ids = np.concatenate([ids for ids, _ in lists]) if nq else np.zeros(0, np.int64)
    dist = np.concatenate([d for _, d in lists]) if nq else np.zeros(0, dt)
    return lims, ids.astype(np.int64), dist.astype(dt)


def same_csr(got, want, what=""):
    """a (lims, ids, dist) result against the reference's: dtypes, shapes and bytes"""
    for g, w, name in zip(got, want, ("lims", "ids", "dist")):
        assert g.dtype == w.dtype and g.ndim == 1, (what, name, g.dtype, w.dtype, g.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), f"{what} {name}"


def same_sets(got, want, what=""):
    """an unsorted result against the sorted reference: equal lims, and per query the same (id, dist) pairs"""
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what} lims")
    assert got[2].dtype == want[2].dtype
    for i in range(len(want[0]) - 1):
        a, b = want[0][i], want[0][i + 1]
        order = np.lexsort((got[1][a:b], got[2][a:b]))
        np.testing.assert_array_equal(got[1][a:b][order], want[1][a:b], err_msg=f"{what} query {i}")
        assert got[2][a:b][order].tobytes() == want[2][a:b].tobytes(), f"{what} query {i}"
