"""The guarded reference of an allowed set, built from the unmodified oracle's primitives: IVF.query
(ivf.py:106-163) with `insert` (_fast_pq_256.pyx:114-118) run only for labels in the set.

  OracleIndex.query(debug=True)            probes and distance table (coarse stage unchanged)
  transform_tables + estimate_pq            each probed list's block distances
  the stale bound per 16-row block          replayed here, `insert` only for allowed labels
  -1 removal / early return / knn_brute1    ivf.py:152-163
"""
import numpy as np


def replay_blocks(oracle, dist, n, labels, hidx, hval, signd, allowed=None, substitute=False):
    """query_pq's replay (_fast_pq_256.pyx:96-123) over `dist` ((chunks, 16) block values, row r of chunk c =
    position 16 c + r < n, label labels[pos]) into the heap (hidx, hval).  allowed: None or a bool array over
    labels.  substitute=False: `insert` guarded by `allowed[label]`; True: every disallowed row's value replaced by
    the heap's empty value (127 signed, 255 unsigned) and no guard — the form the device uses."""
    empty = 127 if signd else 255
    dist = np.asarray(dist)
    vals = dist.astype(np.int8 if signd else np.uint8).astype(np.int32)
    pos = np.arange(vals.size).reshape(vals.shape)
    valid = pos < n
    ok = valid.copy()
    if allowed is not None:
        lab = np.full(vals.size, -1, dtype=np.int64)
        lab[:n] = np.asarray(labels)[:n]
        lab = lab.reshape(vals.shape)
        inside = (lab >= 0) & (lab < len(allowed))
        ok &= inside & allowed[np.where(inside, lab, 0)]
        if substitute:
            vals = np.where(valid & ~ok, empty, vals)
            ok = valid
    mins = vals.min(axis=1) if len(vals) else np.zeros(0, np.int32)
    c = 0
    bound = int(hval[0])
    while c < len(vals):
        nxt = np.flatnonzero(mins[c:] < bound)        # blocks with no passing row change nothing
        if nxt.size == 0:
            break
        c += int(nxt[0])
        for r in np.flatnonzero(vals[c] < bound):
            if ok[c, r]:
                oracle.insert(hidx, hval, int(labels[16 * c + r]), int(vals[c, r]))
        bound = int(hval[0])
        c += 1


def guarded_query(oracle, ox, qn, k, n_probes=1, pass_1=None, allowed=None, debug=False):
    """One query (normalised float32 qn) on OracleIndex `ox`: the reference's result with `insert` only for the
    labels where `allowed` (bool over row ids, or None = all) holds; the reference's variable-length array."""
    qn = np.ascontiguousarray(qn, dtype=np.float32)
    _, dbg = ox.query(qn, k, n_probes, pass_1, debug=True)
    R = pass_1 if pass_1 else (n_probes + 1) * k + 1
    tables = oracle.transform_tables(dbg["table"])
    hidx = np.full(R, -1, dtype=np.int64)
    hval = np.full(R, 127, dtype=np.int32)
    order = ox._s.order
    for p in dbg["probes"]:
        cl = int(p) + ox.n_lists if p < 0 else int(p)
        c0, c1 = int(ox.list_chunk_off[cl]), int(ox.list_chunk_off[cl + 1])
        if c1 == c0:
            continue
        n = int(ox.list_n[cl])
        labels = ox.ids[ox.ids_off[cl]:ox.ids_off[cl] + n]
        out = np.zeros(2 * (c1 - c0), dtype=np.uint64)
        oracle.estimate_pq(np.ascontiguousarray(ox.codes[c0:c1]), tables, out, True, order)
        replay_blocks(oracle, out.view(np.uint8).reshape(-1, 16), n, labels, hidx, hval, True, allowed)
    heap_idx, heap_val = hidx.copy(), hval.copy()
    idx = hidx[hidx != -1]                                   # ivf.py:152-153
    if len(idx) <= k:                                        # :154-156, heap order
        ids = idx
    else:                                                    # :157-163
        ids = idx[oracle.knn_brute1(qn, ox.data[idx], k)]
    if debug:
        return ids, dict(probes=dbg["probes"], heap_idx=heap_idx, heap_val=heap_val)
    return ids


def reference_index(ivf):
    """The CPU reference's copy of a built IVF (as bench.py builds it for its parity leg)."""
    from oracle import oracle
    L = len(ivf.active_centers)
    return oracle.OracleIndex(ivf.pq.centers, 2, ivf.pq.R, ivf.pq.sqrt_n_blocks, ivf.active_centers,
                              ivf.pq_transformed_centers.packed,
                              [ivf.pq_transformed_points[i].packed for i in range(L)],
                              [ivf.pq_transformed_points[i].size for i in range(L)],
                              [ivf.ids[i] for i in range(L)], ivf.data)


def guarded_batch(oracle, ox, qn, k, n_probes=1, pass_1=None, allowed=None, debug=False):
    """guarded_query for every row, padded with -1 to k columns as IVF.query_batch does (oracle None: the module
    under oracle/)."""
    if oracle is None:
        from oracle import oracle
    R = pass_1 if pass_1 else (n_probes + 1) * k + 1
    out = np.full((len(qn), k), -1, dtype=np.int64)
    probes = np.zeros((len(qn), min(n_probes, ox.n_lists)), dtype=np.int64)
    hidx = np.zeros((len(qn), R), dtype=np.int64)
    hval = np.zeros((len(qn), R), dtype=np.int32)
    for i, q in enumerate(qn):
        ids, d = guarded_query(oracle, ox, q, k, n_probes, pass_1, allowed, debug=True)
        out[i, :len(ids)] = ids
        probes[i, :len(d["probes"])] = d["probes"]
        hidx[i], hval[i] = d["heap_idx"], d["heap_val"]
    if debug:
        return out, dict(probes=probes, heap_idx=hidx, heap_val=hval)
    return out
