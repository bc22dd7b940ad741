"""The reference of a query with one excluded row (rows.hip): the guarded reference of
tests/allowed_reference.py with the allowed set "every row but e" — IVF.query (ivf.py:106-163) with `insert` run
only for labels != e.  q_pq: the table-build query to use instead of the oracle's own (numpy's DGEMV for a rotated
PQ) — the device-made one of DeviceIndex.gather_queries, so that a rotated index is compared on the same tables."""
import numpy as np

from allowed_reference import guarded_query


def excluded_query(oracle, ox, qn, e, k, n_probes=1, pass_1=None, q_pq=None, allowed=None, debug=False):
    """guarded_query(allowed & (labels != e)); e = -1 (or None): nothing excluded."""
    N = len(ox.data)
    mask = None if allowed is None else np.array(allowed, dtype=bool, copy=True)
    if e is not None and 0 <= int(e) < N:
        if mask is None:
            mask = np.ones(N, dtype=bool)
        mask[int(e)] = False
    if q_pq is None:
        return guarded_query(oracle, ox, qn, k, n_probes, pass_1, mask, debug)
    fixed = np.ascontiguousarray(q_pq)
    ox.pq_query = lambda _qn: fixed         # OracleIndex.query calls self.pq_query(qn): the instance's wins
    try:
        return guarded_query(oracle, ox, qn, k, n_probes, pass_1, mask, debug)
    finally:
        del ox.pq_query


def excluded_batch(oracle, ox, qn, exclude, k, n_probes=1, pass_1=None, q_pq=None, allowed=None, debug=False):
    """excluded_query for every row, padded with -1 to k columns as guarded_batch pads (oracle None: the module
    under oracle/).  exclude: one row id or -1 per query, or None."""
    if oracle is None:
        from oracle import oracle
    R = pass_1 if pass_1 else (n_probes + 1) * k + 1
    out = np.full((len(qn), k), -1, dtype=np.int64)
    probes = np.zeros((len(qn), min(n_probes, ox.n_lists)), dtype=np.int64)
    hidx = np.zeros((len(qn), R), dtype=np.int64)
    hval = np.zeros((len(qn), R), dtype=np.int32)
    for i, q in enumerate(qn):
        ids, d = excluded_query(oracle, ox, q, -1 if exclude is None else exclude[i], k, n_probes, pass_1,
                                None if q_pq is None else q_pq[i], allowed, debug=True)
        out[i, :len(ids)] = ids
        probes[i, :len(d["probes"])] = d["probes"]
        hidx[i], hval[i] = d["heap_idx"], d["heap_val"]
    if debug:
        return out, dict(probes=probes, heap_idx=hidx, heap_val=hval)
    return out
