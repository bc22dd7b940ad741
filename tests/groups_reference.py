"""The reference of a batch whose queries are each restricted to their own group of rows (groups.hip):
per query the guarded reference of tests/allowed_reference.py with the allowed set `groups == group[i]` — IVF.query
(ivf.py:106-163) with `insert` run only for labels of the query's group — and-ed with an allowed set and with
"every row but exclude[i]" where those are given."""
import numpy as np

from allowed_reference import guarded_query


def grouped_batch(oracle, ox, qn, group, groups, k, n_probes, pass_1=None, allowed=None, exclude=None, debug=False):
    """guarded_query for every row, padded with -1 to k columns as guarded_batch pads (oracle None: the module under
    oracle/).  group: an int, or one entry per query (-1: unrestricted); groups: the group id of every row;
    allowed: None or a bool mask over the rows; exclude: None, or one row id (or -1) per query."""
    if oracle is None:
        from oracle import oracle
    groups = np.asarray(groups)
    N = len(groups)
    group = np.broadcast_to(np.asarray(group), (len(qn),))
    rows = np.arange(N)
    R = pass_1 if pass_1 else (n_probes + 1) * k + 1
    out = np.full((len(qn), k), -1, dtype=np.int64)
    probes = np.zeros((len(qn), min(n_probes, ox.n_lists)), dtype=np.int64)
    hidx = np.zeros((len(qn), R), dtype=np.int64)
    hval = np.zeros((len(qn), R), dtype=np.int32)
    for i, q in enumerate(qn):
        e = -1 if exclude is None else int(exclude[i])
        if group[i] == -1 and allowed is None and not 0 <= e < N:
            mask = None
        else:
            mask = np.ones(N, dtype=bool) if group[i] == -1 else groups == group[i]
            if allowed is not None:
                mask = mask & np.asarray(allowed, dtype=bool)
            if 0 <= e < N:
                mask = mask & (rows != e)
        ids, d = guarded_query(oracle, ox, q, k, n_probes, pass_1, mask, debug=True)
        out[i, :len(ids)] = ids
        probes[i, :len(d["probes"])] = d["probes"]
        hidx[i], hval[i] = d["heap_idx"], d["heap_val"]
    if debug:
        return out, dict(probes=probes, heap_idx=hidx, heap_val=hval)
    return out
