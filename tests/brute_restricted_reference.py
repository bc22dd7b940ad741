"""References for the restricted exact search (tk_index_knn_brute_ex), plain NumPy, no GPU.
tests/test_brute_restricted_cpu.py checks them against slower, more obvious forms."""
import numpy as np

from between_reference import bounds_of, passing as range_passing
from brute_reference import CAP, NS, k_best, segment_rows
from tags_reference import passing as tag_passing


def passes(i, n, allowed=None, exclude=None, group=None, groups=None, tags=None, tags_mode="any", row_tags=None,
           between=None, values=None):
    """The bool mask over the n rows that query i may return.  allowed: a bool mask over the rows; exclude: one row id
    (or -1) per query; group: one id (or -1) per query against `groups`; tags: one mask (or 0) per query against
    `row_tags` under tags_mode (tags_reference.passing); between: (lo, hi), each None or one row of bounds per query,
    against the ORIGINAL `values` (between_reference.passing)."""
    ok = np.ones(n, dtype=bool)
    if allowed is not None:
        ok &= np.asarray(allowed, dtype=bool)
    if exclude is not None and exclude[i] >= 0:
        ok[exclude[i]] = False
    if group is not None and group[i] >= 0:
        ok &= np.asarray(groups) == group[i]
    if tags is not None:
        hit = tag_passing(row_tags, tags[i], tags_mode)
        if hit is not None:
            ok &= hit
    if between is not None:
        ok &= range_passing(values, *bounds_of(between, i))
    return ok


def restricted_k_best(part_row, ok, k):
    """k_best over the passing rows: their ids ascending by (part, row), padded with -1 to k"""
    rows = np.flatnonzero(ok)
    out = np.full(k, -1, dtype=np.int64)
    if len(rows):
        kk = min(k, len(rows))
        out[:kk] = rows[k_best(np.asarray(part_row)[rows], kk)]
    return out


def restricted_dist(part_row, ids):
    """the float32 part values beside restricted_k_best's ids, +inf beside -1"""
    out = np.full(len(ids), np.inf, dtype=np.float32)
    out[ids >= 0] = np.asarray(part_row)[ids[ids >= 0]].astype(np.float32)
    return out


def retry_segment_rows(k):
    """The segment length of the second attempt: the largest multiple of 32 not above CAP - k"""
    return (CAP - k) // 32 * 32


def restricted_within_tau_per_segment(part_row, ok, k, seg=None):
    """What the selection pass appends for one query under a restriction: per segment of `seg` rows (default: the
    segment rule) the number of PASSING rows with part <= tau.  tau starts as the k-th smallest over the passing rows
    among the sampled rows e * (n // ns), +inf where fewer than k of them pass, and after each segment becomes the
    k-th smallest of the passing rows seen so far once k of them lie within it."""
    part_row, ok = np.asarray(part_row), np.asarray(ok, dtype=bool)
    n = len(part_row)
    ns = min(n, NS)
    seg = segment_rows(k, n) if seg is None else seg
    at = np.arange(ns) * (n // ns)
    sample = part_row[at][ok[at]]
    tau = np.partition(sample, k - 1)[k - 1] if len(sample) >= k else np.inf
    counts = []
    for s0 in range(0, n, seg):
        end = min(n, s0 + seg)
        counts.append(int(((part_row[s0:end] <= tau) & ok[s0:end]).sum()))
        seen = part_row[:end][ok[:end]]
        if len(seen) >= k:
            kth = np.partition(seen, k - 1)[k - 1]
            if kth <= tau:
                tau = kth
    return counts
