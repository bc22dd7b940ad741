"""References of the exact search inside a query's value range (tk_index_knn_between), NumPy and the
CPU oracle, no GPU.  Query i ranks the rows that pass its ranges — on the ORIGINAL values and bounds, never on the int64
keys the device compares, so the key map is under test too — and its other restrictions and are stored, by the
rescoring's distance (oracle.sqdist_gather: numpy's einsum order), and returns the k smallest (distance, row id).
span_model: the span the device walks for a query — which column, how many rows — from np.searchsorted on each sorted
original column."""
import math

import numpy as np

from brute_restricted_reference import passes


def knn_between_reference(oracle, qn, data, k, between, values, stored=None, **restrictions):
    """(ids (nq, k) int64, dist (nq, k)) — dist float32, float64 for float64 data; -1 / +inf behind fewer than k rows.
    between: (lo, hi), each None or one row of bounds per query; values: the ORIGINAL values.  restrictions: the other
    keywords of brute_restricted_reference.passes."""
    qn = np.ascontiguousarray(qn, dtype=np.float32)
    data = np.ascontiguousarray(data)
    n = len(data)
    stored = np.ones(n, dtype=bool) if stored is None else np.asarray(stored, dtype=bool)
    dt = np.float64 if data.dtype == np.float64 else np.float32
    ids = np.full((len(qn), k), -1, dtype=np.int64)
    dist = np.full((len(qn), k), np.inf, dtype=dt)
    for i in range(len(qn)):
        rows = np.flatnonzero(passes(i, n, between=between, values=values, **restrictions) & stored)
        if not len(rows):
            continue
        dv = oracle.sqdist_gather(qn[i], data, rows).astype(dt)
        order = np.lexsort((rows, dv))[:k]
        ids[i, :len(order)] = rows[order]
        dist[i, :len(order)] = dv[order]
    return ids, dist


def _number(b):
    """a bound as a Python number: ints stay ints (no wrap), floats widen exactly"""
    return np.asarray(b).tolist()


def _end_is_open(b, low, integer_column):
    """an end that admits every value the column can hold: None, -inf below / +inf above, and on an integer column a
    bound at or beyond the int64 extreme"""
    if b is None:
        return True
    b = _number(b)
    if isinstance(b, float) and math.isinf(b):
        return (b < 0) if low else (b > 0)
    if integer_column:
        return b <= -2**63 if low else b >= 2**63 - 1
    return False


def _column_span(sorted_col, lo, hi):
    """rows of ONE sorted column (int64, or float64 with -0.0 folded into +0.0) with lo <= v <= hi, by np.searchsorted"""
    if sorted_col.dtype == np.int64:
        # integer columns: a floating bound is ceil'ed (lo) / floor'ed (hi), exactly, as Python integers
        lo = -2**63 if lo is None or lo == -math.inf else (2**63 if lo == math.inf else math.ceil(_number(lo)))
        hi = 2**63 - 1 if hi is None or hi == math.inf else (-2**63 - 1 if hi == -math.inf else math.floor(_number(hi)))
        if lo > 2**63 - 1 or hi < -2**63 or lo > hi:
            return 0
        lo, hi = np.int64(max(lo, -2**63)), np.int64(min(hi, 2**63 - 1))
    else:
        lo = -np.inf if lo is None else np.float64(_number(lo))
        hi = np.inf if hi is None else np.float64(_number(hi))
        assert not (np.isnan(lo) or np.isnan(hi))
    b = np.searchsorted(sorted_col, lo, side="left")
    e = np.searchsorted(sorted_col, hi, side="right")
    return max(0, int(e) - int(b))


def span_model(values, between, nq=None):
    """(len (nq,) int64, col (nq,) int32): per query the shortest span among the columns it bounds, ties to the lowest
    column; (N, -1) for a query that bounds no column.  values: (N,) or (N, C) in their own dtype; between: (lo, hi),
    each None or one row of bounds per query ((nq,) for one column, (nq, C))."""
    v = np.asarray(values)
    v = v.reshape(len(v), -1)
    n, C = v.shape
    integer = v.dtype.kind in "iu"
    cols = [np.sort(v[:, c].astype(np.int64)) if integer else np.sort(v[:, c].astype(np.float64) + 0.0) for c in range(C)]
    lo, hi = between
    if nq is None:
        nq = len(lo) if lo is not None else len(hi)
    length = np.full(nq, n, dtype=np.int64)
    col = np.full(nq, -1, dtype=np.int32)
    for i in range(nq):
        for c in range(C):
            lo_c = None if lo is None else np.asarray(lo)[i].reshape(-1)[c]
            hi_c = None if hi is None else np.asarray(hi)[i].reshape(-1)[c]
            if _end_is_open(lo_c, True, integer) and _end_is_open(hi_c, False, integer):
                continue
            span = _column_span(cols[c], lo_c, hi_c)
            if col[i] < 0 or span < length[i]:
                length[i], col[i] = span, c
    return length, col


def value_order(values, c=0):
    """the row ids ascending by (value of column c, row id): the order the device walks a span of that column in"""
    v = np.asarray(values)
    v = v.reshape(len(v), -1)[:, c]
    key = v.astype(np.int64) if v.dtype.kind in "iu" else v.astype(np.float64) + 0.0
    return np.lexsort((np.arange(len(v)), key))
