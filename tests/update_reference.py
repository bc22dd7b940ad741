"""What IVF.update must leave behind, in numpy alone: the lists of a snapshot filtered (the replaced rows dropped,
everything else in its old order) and then spliced (list l's column-j block = kept_j ++ the new rows whose j-th
nearest centre is l, ascending, labelled with the ids they replace), the members per (list, column) that follow,
and the vectors with their rows replaced.  Written against the definition, not against the library's own
_filter_lists / _splice.

A snapshot is (ids per list, PQ labels (n_l, M) per list, list_columns (L, kp), the zero vector's labels) — what
test_remove_gpu.py::_snapshot takes off a device index; its fourth entry is not read here."""
import numpy as np


def updated_lists(snap, ids, nearest, labels):
    """-> (ids per list, labels per list, list_columns (L1, kp)) after update(ids, X), where row i of X was assigned
    nearest[i] (kp centre ids) and coded labels[i] (M).  L1 = the old lists, or more where a row's centre lies
    past them."""
    ids_l, lab_l, cols = snap[0], snap[1], np.asarray(snap[2], np.int64)
    ids = np.asarray(ids, np.int64)
    nearest = np.asarray(nearest, np.int64).reshape(len(ids), -1)
    L0, kp = cols.shape
    assert nearest.shape[1] == kp and len(np.unique(ids)) == len(ids)
    L1 = max(L0, int(nearest.max()) + 1) if len(ids) else L0
    M = labels.shape[1]
    top = max([int(ids.max()) if len(ids) else -1] + [int(np.max(a)) for a in ids_l if len(a)])
    dead = np.zeros(top + 1, bool)
    dead[ids] = True
    out_ids, out_lab, cols1 = [], [], np.zeros((L1, kp), np.int64)
    for l in range(L1):
        ip, lp, o = [], [], 0
        for j in range(kp):
            c = int(cols[l, j]) if l < L0 else 0
            blk_ids = np.asarray(ids_l[l][o:o + c], np.int64) if l < L0 else np.zeros(0, np.int64)
            keep = ~dead[blk_ids]
            new = np.nonzero(nearest[:, j] == l)[0]             # ascending i
            ip += [blk_ids[keep], ids[new]]
            lp += [np.asarray(lab_l[l][o:o + c]).reshape(c, M)[keep] if l < L0 else np.zeros((0, M), np.uint8),
                   labels[new]]
            cols1[l, j] = int(keep.sum()) + len(new)
            o += c
        assert l >= L0 or o == len(ids_l[l])
        out_ids.append(np.concatenate(ip).astype(np.int64))
        out_lab.append(np.concatenate(lp).astype(np.uint8))
    return out_ids, out_lab, cols1


def updated_data(data, ids, rows):
    """The vectors with rows `ids` replaced by the prepared `rows` (a copy, in data's dtype)."""
    out = np.array(data, copy=True)
    out[np.asarray(ids, np.int64)] = rows
    return out


def relabelled(ids_l, N, ids):
    """Lists after remove(ids) + add(X) with the added rows' labels N + i turned into ids[i]."""
    ids = np.asarray(ids, np.int64)
    out = []
    for a in ids_l:
        a = np.array(a, dtype=np.int64, copy=True)
        new = a >= N
        a[new] = ids[a[new] - N]
        out.append(a)
    return out


def assignment_of_added(snap, N, n):
    """(nearest (n, kp), labels (n, M)) of the rows N .. N + n - 1 as the lists of `snap` hold them — an index to
    which add() appended them: row N + i sits in list nearest[i, j]'s column-j block and carries labels[i] there."""
    ids_l, lab_l, cols = snap[0], snap[1], np.asarray(snap[2], np.int64)
    L, kp = cols.shape
    nearest = np.full((n, kp), -1, np.int64)
    labels = None
    for l in range(L):
        col_of = np.repeat(np.arange(kp), cols[l])
        a = np.asarray(ids_l[l], np.int64)
        sel = np.nonzero(a >= N)[0]
        if labels is None:
            labels = np.zeros((n, lab_l[l].shape[1]), np.uint8)
        assert (nearest[a[sel] - N, col_of[sel]] == -1).all()
        nearest[a[sel] - N, col_of[sel]] = l
        labels[a[sel] - N] = lab_l[l][sel]
    assert (nearest >= 0).all()
    return nearest, labels
