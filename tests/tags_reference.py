"""The reference of a batch whose queries are each restricted to the rows that carry their tags (tags.hip, DESIGN
§3.13): per query the guarded reference of tests/allowed_reference.py with the allowed set made in numpy from the two
formulas — "any": (tags & m) != 0, "all": (tags & m) == m, m == 0: every row — and-ed with an allowed set, with "every
row but exclude[i]" and with `groups == group[i]` where those are given."""
import numpy as np

from allowed_reference import guarded_query


def passing(tags, m, mode):
    """the bool mask over the rows that a query mask m passes under `mode`, None for m == 0 (unrestricted)"""
    assert mode in ("any", "all"), mode
    m = np.uint64(m)
    if m == 0:
        return None
    hit = np.asarray(tags, dtype=np.uint64) & m
    return hit == m if mode == "all" else hit != 0


def tagged_batch(oracle, ox, qn, mask, mode, tags, k, n_probes, pass_1=None, allowed=None, exclude=None, group=None,
                 groups=None, debug=False):
    """guarded_query for every row, padded with -1 to k columns as guarded_batch pads (oracle None: the module under
    oracle/).  mask: an int, or one uint64 per query (0: unrestricted); mode: "any" / "all"; tags: the uint64 mask of
    every row; allowed: None or a bool mask over the rows; exclude: None, or one row id (or -1) per query; group: None,
    an int or one group id (or -1) per query, with groups: the group id of every row."""
    if oracle is None:
        from oracle import oracle
    tags = np.asarray(tags, dtype=np.uint64)
    N = len(tags)
    mask = np.broadcast_to(np.asarray(mask, dtype=np.uint64), (len(qn),))
    group = None if group is None else np.broadcast_to(np.asarray(group), (len(qn),))
    rows = np.arange(N)
    R = pass_1 if pass_1 else (n_probes + 1) * k + 1
    out = np.full((len(qn), k), -1, dtype=np.int64)
    probes = np.zeros((len(qn), min(n_probes, ox.n_lists)), dtype=np.int64)
    hidx = np.zeros((len(qn), R), dtype=np.int64)
    hval = np.zeros((len(qn), R), dtype=np.int32)
    for i, q in enumerate(qn):
        parts = [passing(tags, mask[i], mode)]
        if allowed is not None:
            parts.append(np.asarray(allowed, dtype=bool))
        if exclude is not None and 0 <= int(exclude[i]) < N:
            parts.append(rows != int(exclude[i]))
        if group is not None and group[i] != -1:
            parts.append(np.asarray(groups) == group[i])
        parts = [p for p in parts if p is not None]
        row_mask = None if not parts else np.logical_and.reduce(parts)
        ids, d = guarded_query(oracle, ox, q, k, n_probes, pass_1, row_mask, debug=True)
        out[i, :len(ids)] = ids
        probes[i, :len(d["probes"])] = d["probes"]
        hidx[i], hval[i] = d["heap_idx"], d["heap_val"]
    if debug:
        return out, dict(probes=probes, heap_idx=hidx, heap_val=hval)
    return out
