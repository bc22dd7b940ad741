"""The reference of a batch whose queries return at most m rows of any one group (per_group=, cap_select.h, DESIGN
§3.15).  Up to the heap it is one of the existing guarded references, called with debug=True and not copied:
grouped_batch / tagged_batch / ranged_batch / excluded_batch, whichever takes the restrictions given.  From the heap on
it is IVF.query's last lines (ivf.py:152-163) with the cap between the ranking and the cut:

  c      the heap's ids in heap order, -1 dropped                                ivf.py:154-155
  order  nc > k: ascending oracle.sqdist_gather distance, ties to the lower position in c (a stable argsort: what
         knn_brute1 / bottom_k return for the first k); nc <= k: position           ivf.py:157-163 / :158-159
  walk   in that order; a candidate is kept if fewer than m of its group have been kept; stop at k kept

in plain Python.  A candidate's group is groups[id]; m = 0: no cap (the walk keeps the first k)."""
import numpy as np

from between_reference import ranged_batch
from groups_reference import grouped_batch
from rows_reference import excluded_batch
from tags_reference import tagged_batch


def heaps_of(oracle, ox, qn, k, n_probes, pass_1=None, allowed=None, exclude=None, group=None, groups=None, tags=None,
             tags_mode="any", row_tags=None, between=None, values=None, q_pq=None):
    """heap_idx (nq, R) of the guarded reference that takes these restrictions (none: the unrestricted query)"""
    if between is not None:
        assert q_pq is None
        return ranged_batch(oracle, ox, qn, between, values, k, n_probes, pass_1, allowed=allowed, exclude=exclude,
                            group=group, groups=groups, mask=tags, mode=tags_mode, tags=row_tags, debug=True)[1]["heap_idx"]
    if tags is not None:
        assert q_pq is None
        return tagged_batch(oracle, ox, qn, tags, tags_mode, row_tags, k, n_probes, pass_1, allowed=allowed,
                            exclude=exclude, group=group, groups=groups, debug=True)[1]["heap_idx"]
    if group is not None:
        assert q_pq is None
        return grouped_batch(oracle, ox, qn, group, groups, k, n_probes, pass_1, allowed=allowed, exclude=exclude,
                             debug=True)[1]["heap_idx"]
    return excluded_batch(oracle, ox, qn, exclude, k, n_probes, pass_1, q_pq=q_pq, allowed=allowed,
                          debug=True)[1]["heap_idx"]


def ranking(oracle, ox, q, heap_row, k):
    """(ids, distances) of one query's candidates in the order the rescoring ranks them: ALL nc of them"""
    c = heap_row[heap_row != -1]
    d = oracle.sqdist_gather(q, ox.data, c)
    if ox.data.dtype != np.float64:
        d = d.astype(np.float32)
    if len(c) > k:
        order = np.argsort(d, kind="stable")
        c, d = c[order], d[order]
    return c, d


def walk(ids, row_groups, m, k):
    """positions of `ids` (in rank order) that the cap keeps: rule 3, serially"""
    kept, seen = [], {}
    for pos, i in enumerate(ids):
        if len(kept) == k:
            break
        g = int(row_groups[int(i)])         # (a negative id addresses from the end, as numpy and the device do)
        if m == 0 or seen.get(g, 0) < m:
            seen[g] = seen.get(g, 0) + 1
            kept.append(pos)
    return kept


def capped_batch(oracle, ox, qn, per_group, groups, k, n_probes, pass_1=None, allowed=None, exclude=None, group=None,
                 tags=None, tags_mode="any", row_tags=None, between=None, values=None, q_pq=None, full=False):
    """(ids (nq, k) padded with -1, distances (nq, k) padded with +inf — float32, float64 for float64 vectors —,
    counts (nq,)).  per_group: an int or one entry per query, 0 for no cap; groups: the group id of every row; the
    restrictions as the guarded references take them (tags: the query masks, row_tags: every row's; between / values
    likewise; q_pq: excluded_batch's).  full=True: also the list of every query's whole ranking (ids, distances)."""
    if oracle is None:
        from oracle import oracle
    heaps = heaps_of(oracle, ox, qn, k, n_probes, pass_1, allowed, exclude, group, groups, tags, tags_mode, row_tags,
                     between, values, q_pq)
    return capped_from_heaps(oracle, ox, qn, heaps, per_group, groups, k, full=full)


def capped_from_heaps(oracle, ox, qn, heaps, per_group, groups, k, full=False):
    """capped_batch from the guarded reference's heap_idx on: a heap depends on neither the groups nor the caps, so
    tests that vary those compute it once (heaps_of)."""
    nq = len(qn)
    m = np.broadcast_to(np.asarray(per_group), (nq,))
    assert (m >= 0).all()
    f64 = ox.data.dtype == np.float64
    ids = np.full((nq, k), -1, dtype=np.int64)
    dist = np.full((nq, k), np.inf, dtype=np.float64 if f64 else np.float32)
    counts = np.zeros(nq, dtype=np.int64)
    ranked = []
    for i in range(nq):
        c, d = ranking(oracle, ox, qn[i], heaps[i], k)
        ranked.append((c, d))
        kept = walk(c, groups, int(m[i]), k)
        counts[i] = len(kept)
        ids[i, :len(kept)] = c[kept]
        dist[i, :len(kept)] = d[kept]
    return (ids, dist, counts, ranked) if full else (ids, dist, counts)
