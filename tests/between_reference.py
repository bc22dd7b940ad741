"""The reference of a batch whose queries are each restricted to the rows whose values lie in their ranges (between.hip,
DESIGN §3.14): per query the guarded reference of tests/allowed_reference.py with the allowed set made in numpy from
the formula lo_c <= values[row, c] <= hi_c for every column c — on the ORIGINAL values and bounds, never on the int64
keys the device compares, so that the key map (tinyknn_amd.ivf.value_keys / query_ranges) is under test too — and-ed
with an allowed set, with "every row but exclude[i]", with `groups == group[i]` and with the tag formulas of
tests/tags_reference.py where those are given."""
import numpy as np

from allowed_reference import guarded_query
from tags_reference import passing as tag_passing


def _exact(a):
    """a numeric numpy array as Python numbers: ints stay ints, floats widen exactly to float — Python compares an int
    with a float exactly, which numpy (int64 -> float64) does not"""
    return np.asarray(a).tolist()


def _column_passes(v, lo, hi):
    """bool over the rows of ONE column v: lo <= v <= hi, None = unbounded"""
    v = np.asarray(v)
    ok = np.ones(len(v), dtype=bool)
    for bound, low in ((lo, True), (hi, False)):
        if bound is None:
            continue
        b = np.asarray(bound)
        assert b.ndim == 0 and not (b.dtype.kind == "f" and np.isnan(b)), bound
        if v.dtype.kind == "f" and b.dtype.kind == "f":
            w, x = v.astype(np.float64), np.float64(b)          # (exact widenings: the comparison is exact)
            ok &= (w >= x) if low else (w <= x)
        elif v.dtype.kind in "iu" and b.dtype.kind in "iu":
            x = int(b)                                            # (Python ints: no wrap whatever the two dtypes)
            if v.dtype == np.uint64 or not -2**63 <= x < 2**63:
                ok &= np.array([(w >= x) if low else (w <= x) for w in _exact(v)], dtype=bool)
            else:
                ok &= (v.astype(np.int64) >= x) if low else (v.astype(np.int64) <= x)
        elif v.dtype.kind in "iu" and (len(v) == 0 or (int(v.min()) > -2**53 and int(v.max()) < 2**53)):
            w, x = v.astype(np.float64), np.float64(b)          # (integers a float64 holds exactly)
            ok &= (w >= x) if low else (w <= x)
        elif v.dtype.kind == "f" and abs(int(b)) < 2**53:
            w, x = v.astype(np.float64), np.float64(int(b))
            ok &= (w >= x) if low else (w <= x)
        else:                                                     # an integer against a float: exact in Python
            x = _exact(b)
            ok &= np.array([(w >= x) if low else (w <= x) for w in _exact(v)], dtype=bool)
    return ok


def passing(values, lo, hi):
    """The bool mask over the rows that one query's ranges pass: values (N,) or (N, C) in their own dtype; lo, hi:
    None (every column unbounded), a scalar (C == 1) or one entry per column, each a number or None."""
    v = np.asarray(values)
    v = v.reshape(len(v), -1)
    C = v.shape[1]

    def per_column(b):
        if b is None:
            return [None] * C
        if np.ndim(b) == 0:
            assert C == 1, "a scalar bound needs one column"
            return [b]
        assert len(b) == C, (len(b), C)
        return list(b)
    lo, hi = per_column(lo), per_column(hi)
    ok = np.ones(len(v), dtype=bool)
    for c in range(C):
        ok &= _column_passes(v[:, c], lo[c], hi[c])
    return ok


def bounds_of(between, i):
    """query i's (lo, hi) of a batch's between = (lo, hi), each None or an (nq, C) / (nq,) array"""
    lo, hi = between
    return (None if lo is None else np.asarray(lo)[i]), (None if hi is None else np.asarray(hi)[i])


def ranged_batch(oracle, ox, qn, between, values, k, n_probes, pass_1=None, allowed=None, exclude=None, group=None,
                 groups=None, mask=None, mode="any", tags=None, debug=False):
    """guarded_query for every row, padded with -1 to k columns as guarded_batch pads (oracle None: the module under
    oracle/).  between: (lo, hi), each None or one row of bounds per query ((nq,) for one column, (nq, C)); values: the
    values of every row; allowed: None or a bool mask over the rows; exclude: None, or one row id (or -1) per query;
    group / groups, mask / mode / tags: as tags_reference.tagged_batch."""
    if oracle is None:
        from oracle import oracle
    N = len(values)
    nq = len(qn)
    group = None if group is None else np.broadcast_to(np.asarray(group), (nq,))
    mask = None if mask is None else np.broadcast_to(np.asarray(mask, dtype=np.uint64), (nq,))
    rows = np.arange(N)
    R = pass_1 if pass_1 else (n_probes + 1) * k + 1
    out = np.full((nq, k), -1, dtype=np.int64)
    probes = np.zeros((nq, min(n_probes, ox.n_lists)), dtype=np.int64)
    hidx = np.zeros((nq, R), dtype=np.int64)
    hval = np.zeros((nq, R), dtype=np.int32)
    for i, q in enumerate(qn):
        parts = [passing(values, *bounds_of(between, i))]
        if allowed is not None:
            parts.append(np.asarray(allowed, dtype=bool))
        if exclude is not None and 0 <= int(exclude[i]) < N:
            parts.append(rows != int(exclude[i]))
        if group is not None and group[i] != -1:
            parts.append(np.asarray(groups) == group[i])
        if mask is not None:
            parts.append(tag_passing(tags, mask[i], mode))
        parts = [p for p in parts if p is not None]
        ids, d = guarded_query(oracle, ox, q, k, n_probes, pass_1, np.logical_and.reduce(parts), debug=True)
        out[i, :len(ids)] = ids
        probes[i, :len(d["probes"])] = d["probes"]
        hidx[i], hval[i] = d["heap_idx"], d["heap_val"]
    if debug:
        return out, dict(probes=probes, heap_idx=hidx, heap_val=hval)
    return out
