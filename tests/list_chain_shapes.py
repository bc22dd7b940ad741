"""Chains of IVF.add / IVF.remove / IVF.update on the awkward indexes of tests/test_fuzz_gpu.py, made on the host without
a GPU: case(seed) draws an index shape, builds it with device=False, and draws 5-8 changes with their arguments, each
from the layout the one before left.  Everything follows from the seed.  ListsModel is what the three docstrings in
tinyknn_amd/ivf.py define, in numpy alone (not through IVF._splice / IVF._filter_lists): ids and PQ labels per list,
members per (list, column), the vectors, the groups.  tests/test_list_chain_cpu.py holds the model against the host path
and asserts that the default seeds reach what they are here for (lists of 0, 1, 15-17 rows, emptied and refilled lists,
a one-tile code array, empty column blocks, rows removed and stored again, ...); tests/test_list_chain_gpu.py runs the
device through the same chains.

Shapes: the ranges of test_fuzz_gpu._case.  Odd seeds are steered towards the edges: step 0 of their chain removes rows
until every list has 15, 16, 17, 31, 32 or 33 rows (where it had that many), so that the changes after it cross the
16-row chunk boundaries; every fourth seed removes every stored row somewhere in its chain and adds into the empty
index; seeds 6 and 2 (mod 12) take the widest and the narrowest codes; seeds 5 (mod 12) build over the rows that leave
the last centre inactive and add rows that activate it (floor: tests/test_list_chain_cpu.py)."""
import copy
import functools
import os

import numpy as np

from update_reference import updated_data, updated_lists

DEFAULT_SEEDS = 24
# Where the seeds' random streams start.  Chosen, with the steering below, so that the default seeds hold every
# condition tests/test_list_chain_cpu.py::test_default_seeds_cover_every_category asserts.
STREAM = 9100
EDGE_SIZES = (15, 16, 17, 31, 32, 33)
ADD_SIZES = (1, 5, 40, 300)
REMOVE_KINDS = ("tenth", "list", "all", "gone", "dups", "added")
UPDATE_KINDS = ("random", "removed", "added", "all", "same", "one")
STORES = ("float32", "float32", "float16", "float64")      # float64: the data's dtype, store=None


def seeds():
    """the seeds of a run: DEFAULT_SEEDS, or TINYKNN_FUZZ_SEEDS as in tests/test_fuzz_gpu.py"""
    return range(int(os.environ.get("TINYKNN_FUZZ_SEEDS", str(DEFAULT_SEEDS))))


def shape(seed):
    rng = np.random.RandomState(STREAM + seed)
    steered = seed % 2 == 1
    d = int(rng.choice([3, 8, 17, 20, 33, 100, 130]))
    n_clusters = int(rng.choice([1, 2, 7, 16, 17, 40]))
    n = int(rng.choice([n_clusters + 1, 60, 333, 1500, 3000]))
    n = max(n, 17 * max(1, n_clusters // 8))       # FastPQ.fit wants >= 16 distinct points
    c = dict(
        d=d, n=n, n_clusters=n_clusters,
        metric=str(rng.choice(["euclidean", "angular"])),
        build_probes=int(min(n_clusters, rng.choice([1, 1, 2, 3]))),
        k=int(rng.choice([1, 5, 10, 50])),
        n_probes=int(rng.choice([1, 2, 5, n_clusters, n_clusters + 3])),
        nq=int(rng.choice([1, 3, 65])),
        spread=float(rng.choice([0.3, 1.0, 6.0])),
        rotate=bool(rng.rand() < 0.5),
        store=str(rng.choice(STORES)),
        n_ops=int(rng.randint(5, 9)),
        steered=steered,
        groups=seed % 3 == 0,
        empty_then_add=seed % 4 == 3,
        activate=seed % 12 == 5,
    )
    if seed % 12 == 6:          # the widest codes: M = 68
        c["d"], c["rotate"] = 130, False
    if seed % 12 == 2:          # the narrowest: M = 4
        c["d"] = int(rng.choice([3, 8]))
    if c["activate"]:           # (a centre to leave out, rows enough around the others)
        c["n_clusters"] = max(c["n_clusters"], 2)
        c["n"] = max(c["n"], 60)
        c["build_probes"] = 1   # (with more, leaving the last centre out can empty another centre's column: refused)
        c["n_probes"] = max(1, min(c["n_probes"], c["n_clusters"] + 3))
    return c


def resident_seeds(seeds):
    """The seeds of the leg on an index built in HBM (build_resident): every third, where the device build takes the
    shape (d <= 128) and no centre is left out.  From 0, where the default seeds hold rotated codes, two lists per
    row, a half store and more than one list (tests/test_list_chain_cpu.py counts them)."""
    return [s for s in seeds if s % 3 == 0 and shape(s)["d"] <= 128 and not shape(s)["activate"]]


def resident_shape(seed):
    """What the resident leg takes of shape(seed), and what it changes: the device build assigns a row to at most
    two lists, and keeps float32 vectors or halfs of them (a float64 seed is a float32 index there)."""
    c = shape(seed)
    return dict(c, build_probes=min(c["build_probes"], 2), store="float16" if c["store"] == "float16" else "float32")


# ---- the model ----

def _blocks(cols_l):
    """the (start, stop) of a list's column blocks"""
    o = np.concatenate([[0], np.cumsum(cols_l)])
    return [(int(o[j]), int(o[j + 1])) for j in range(len(cols_l))]


class ListsModel:
    """An IVF's lists after add / remove / update, by the definitions in their docstrings.  ids[l] (n_l,) int64 and
    labels[l] (n_l, M) uint8: list l's members and their PQ labels; cols (L, kp): members per (list, column) — list l
    is its kp column blocks one behind the other; data (N, d): the vectors in the dtype of IVF.data (a half store
    holds float16 of them: stored()); zero (M,): the zero vector's labels, which the rows that pad a list's codes to a
    multiple of 16 carry; groups (N,) int32 or None."""

    def __init__(self, ids, labels, cols, data, zero, half=False, groups=None):
        self.ids = [np.array(a, dtype=np.int64) for a in ids]
        self.labels = [np.array(a, dtype=np.uint8).reshape(len(i), len(zero)) for a, i in zip(labels, self.ids)]
        self.cols = np.array(cols, dtype=np.int64)
        self.data = np.array(data)
        self.zero = np.array(zero, dtype=np.uint8)
        self.half = half
        self.groups = None if groups is None else np.array(groups, dtype=np.int32)
        self.check()

    @classmethod
    def of(cls, ivf):
        """the model of a host-built IVF as it stands"""
        from tinyknn_amd._transform import unpack
        L = len(ivf.active_centers)
        ids, labels = [], []
        for l in range(L):
            a = np.asarray(ivf.ids[l], dtype=np.int64)
            t = ivf.pq_transformed_points[l]
            ids.append(a)
            labels.append(unpack(t.packed)[:len(a)] if len(a) else np.zeros((0, 0), np.uint8))
        zero = zero_labels(ivf)
        labels = [x if len(x) else np.zeros((0, len(zero)), np.uint8) for x in labels]
        return cls(ids, labels, ivf.list_columns, ivf.data, zero, ivf.store == "float16", ivf.groups)

    def copy(self):
        return ListsModel(self.ids, self.labels, self.cols, self.data, self.zero, self.half, self.groups)

    def check(self):
        assert len(self.ids) == len(self.labels) == len(self.cols)
        for l in range(len(self.ids)):
            assert self.cols[l].sum() == len(self.ids[l]) == len(self.labels[l]), l

    # ---- what it holds ----
    @property
    def N(self):
        return len(self.data)

    @property
    def L(self):
        return len(self.ids)

    @property
    def kp(self):
        return self.cols.shape[1]

    @property
    def sizes(self):
        return np.array([len(a) for a in self.ids], dtype=np.int64)

    def snap(self):
        """the snapshot form of update_reference.py"""
        return self.ids, self.labels, self.cols, self.zero

    def stored_ids(self):
        return np.unique(np.concatenate(self.ids)) if self.L else np.zeros(0, np.int64)

    def stored(self):
        """the vectors as the device's store gives them back (float32; rounded through half for a half store)"""
        if self.half:
            return np.asarray(self.data, np.float32).astype(np.float16).astype(np.float32)
        return self.data

    def chunk_off(self):
        return np.concatenate([[0], np.cumsum((self.sizes + 15) // 16)])

    # ---- the three changes ----
    def add(self, rows, nearest, labels, groups=None):
        """IVF.add: the rows get ids N .. N + n - 1; list l's column-j block becomes old_j ++ (the new rows whose j-th
        nearest centre is l, ascending); a centre past the lists appends lists up to it."""
        n, N = len(rows), self.N
        nearest = np.asarray(nearest, np.int64).reshape(n, self.kp)
        labels = np.asarray(labels, np.uint8).reshape(n, len(self.zero))
        L1 = max(self.L, int(nearest.max()) + 1) if n else self.L
        new_ids = N + np.arange(n, dtype=np.int64)
        ids, labs, cols = [], [], np.zeros((L1, self.kp), np.int64)
        for l in range(L1):
            old = l < self.L
            ip, lp = [], []
            for j, (a, b) in enumerate(_blocks(self.cols[l] if old else np.zeros(self.kp, np.int64))):
                new = np.flatnonzero(nearest[:, j] == l)
                ip += [self.ids[l][a:b] if old else np.zeros(0, np.int64), new_ids[new]]
                lp += [self.labels[l][a:b] if old else np.zeros((0, len(self.zero)), np.uint8), labels[new]]
                cols[l, j] = b - a + len(new)
            ids.append(np.concatenate(ip))
            labs.append(np.concatenate(lp))
        self.ids, self.labels, self.cols = ids, labs, cols
        self.data = np.concatenate([self.data, np.asarray(rows, dtype=self.data.dtype)])
        if self.groups is not None:
            self.groups = np.concatenate([self.groups, np.asarray(groups, np.int32)])
        self.check()
        return self

    def remove(self, ids):
        """IVF.remove: every copy of the rows named leaves its list, the others keep their order; each column block
        shrinks in place; ids not stored are ignored; the vectors stay."""
        dead = np.zeros(self.N, dtype=bool)
        dead[np.asarray(ids, np.int64)] = True
        for l in range(self.L):
            keep = ~dead[self.ids[l]]
            self.cols[l] = [int(keep[a:b].sum()) for a, b in _blocks(self.cols[l])]
            self.ids[l], self.labels[l] = self.ids[l][keep], self.labels[l][keep]
        self.check()
        return self

    def update(self, ids, rows, nearest, labels, groups=None):
        """IVF.update, through update_reference.py"""
        self.ids, self.labels, self.cols = updated_lists(self.snap(), ids, nearest, labels)
        self.data = updated_data(self.data, ids, rows)
        if groups is not None:
            self.groups = self.groups.copy()
            self.groups[np.asarray(ids, np.int64)] = groups
        self.check()
        return self

    def apply(self, op):
        if op["kind"] == "add":
            return self.add(op["new"], op["near"], op["labels"], op["groups"])
        if op["kind"] == "remove":
            return self.remove(op["ids"])
        return self.update(op["ids"], op["new"], op["near"], op["labels"], op["groups"])


def zero_labels_of(pq, d, dtype):
    """the zero vector's labels, from the PQ's own transform of a zero row of d dimensions"""
    from tinyknn_amd._transform import unpack
    return unpack(pq.transform(np.zeros((1, d), dtype=dtype), device=False).packed)[0]


def zero_labels(ivf):
    return zero_labels_of(ivf.pq, ivf.data.shape[1], ivf.data.dtype)


def prepared(ivf, X, kp):
    """New rows as the host build prepares its rows, from the reference's own functions:
    -> (rows in IVF.data's dtype, normalised for angular; nearest (n, kp); PQ labels (n, M))"""
    from tinyknn_amd._transform import unpack
    from tinyknn_amd.utils import knn_brute
    new = np.asarray(X).astype(ivf.data.dtype)
    if ivf.metric == "angular":
        new = new / np.linalg.norm(new, axis=1, keepdims=True)
    near = np.asarray(knn_brute(new, ivf.all_centers, k=kp, metric=ivf.metric)).reshape(len(new), kp)
    return new, near.astype(np.int64), unpack(ivf.pq.transform(new, device=False).packed)[:len(new)]


def apply_to_ivf(ivf, op):
    """the change `op` through the library"""
    if op["kind"] == "add":
        return ivf.add(op["X"], groups=op["groups"])
    if op["kind"] == "remove":
        return ivf.remove(op["ids"])
    return ivf.update(op["ids"], op["X"], groups=op["groups"])


def assert_host_lists(ivf, m, msg=""):
    """the host copy of an IVF holds exactly the model's lists, columns, vectors and groups"""
    from tinyknn_amd._transform import unpack
    assert len(ivf.active_centers) == m.L, msg
    np.testing.assert_array_equal(ivf.list_columns, m.cols, err_msg=f"list_columns {msg}")
    for l in range(m.L):
        t = ivf.pq_transformed_points[l]
        n = 0 if isinstance(t, np.ndarray) else t.size
        assert n == len(m.ids[l]), f"size of list {l} {msg}"
        np.testing.assert_array_equal(np.asarray(ivf.ids[l], np.int64)[:n], m.ids[l], err_msg=f"ids of list {l} {msg}")
        if n:
            want = np.concatenate([m.labels[l], np.repeat(m.zero[None], (-n) % 16, axis=0)])
            np.testing.assert_array_equal(unpack(t.packed), want, err_msg=f"codes of list {l} {msg}")
    assert ivf.data.dtype == m.data.dtype and ivf.data.shape == m.data.shape, msg
    assert np.array_equal(np.ascontiguousarray(ivf.data).view(np.uint8), np.ascontiguousarray(m.data).view(np.uint8)), \
        f"data {msg}"
    if m.groups is None:
        assert ivf.groups is None, msg
    else:
        np.testing.assert_array_equal(ivf.groups, m.groups, err_msg=f"groups {msg}")


# ---- the cases ----

class Case:
    """One case.  shape: the dict of shape(seed); ivf: the host-built index before the chain, its groups set, no
    device copy — fresh_ivf() gives a copy to change; N0: the rows it was built over; ops: the chain, each a dict(kind
    'add' | 'remove' | 'update', sel: how its rows were chosen, ids (remove, update), X: the raw rows and new, near,
    labels: prepared() of them (add, update), groups: the rows' groups or None); qs, qn, qp: the queries, raw and as
    IVF._prepare makes them; cent: the generator's centres; skipped: why the case could not be built, or None."""
    skipped = None

    def __init__(self, seed):
        self.seed = seed
        self.shape = shape(seed)

    def __repr__(self):
        return f"seed {self.seed} {self.shape}"

    def fresh_ivf(self):
        ivf = copy.copy(self.ivf)
        ivf._dev = None
        ivf.data = self.ivf.data.copy()
        return ivf

    def model(self):
        """the model before the chain"""
        return ListsModel.of(self.ivf)

    def replay(self):
        """(step, op, the model after it) for every step of the chain; the model is one object, changed in place"""
        m = self.model()
        for i, op in enumerate(self.ops):
            yield i, op, m.apply(op)

    def rows_near(self, rng, n, centre=None):
        """n rows round the generator's centres, or (centre given: the one the build left inactive) n of the fitted
        rows the build left out because that centre is their nearest — the generator's own rows, so that they too
        follow from the seed bit for bit"""
        cent = self.cent
        if centre is not None:
            return np.ascontiguousarray(self.left_out[np.arange(n) % len(self.left_out)], dtype=self.ivf.data.dtype)
        return (cent[rng.randint(len(cent), size=n)] + 0.5 * rng.randn(n, cent.shape[1])).astype(self.ivf.data.dtype)


def _index(c, seed):
    """-> (the built index, the generator's centres, raw queries, the fitted rows an activating build left out or
    None), or why not (a string)"""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.utils import knn_brute
    rng = np.random.RandomState(STREAM + 100000 + seed)
    cent = rng.randn(max(c["n_clusters"], 3), c["d"]) * c["spread"]
    X = (cent[rng.randint(len(cent), size=c["n"])] + 0.5 * rng.randn(c["n"], c["d"])).astype(np.float32)
    qs = (cent[rng.randint(len(cent), size=c["nq"])] + 0.5 * rng.randn(c["nq"], c["d"])).astype(np.float32)
    if c["store"] == "float64":
        X = X.astype(np.float64)
    ivf = IVF(c["metric"], c["n_clusters"], FastPQ(2) if c["rotate"] else FastPQ(2, rotate_dim=None))
    state = np.random.get_state()
    np.random.seed(STREAM + 200000 + seed)      # (both k-means, centres and codebook, draw from the global generator)
    want = c["n_clusters"]
    left_out = None
    try:
        ivf.fit(X)
        if c["activate"]:       # built over the rows none of whose build_probes nearest centres is the last one
            Xn = X / np.linalg.norm(X, axis=1, keepdims=True) if c["metric"] == "angular" else X
            near = np.asarray(knn_brute(Xn, ivf.all_centers, k=c["build_probes"], metric=c["metric"]))
            out = (near.reshape(len(X), -1) == want - 1).any(axis=1)
            X, left_out = np.ascontiguousarray(X[~out]), np.ascontiguousarray(X[out])
            want -= 1
            if len(X) < 17 or len(left_out) == 0:
                return "too few rows are left beside the last centre's"
        ivf.build(X, n_probes=c["build_probes"], device=False, store="float16" if c["store"] == "float16" else None)
    except AssertionError:
        return "the host build rejects this shape exactly as the reference does"
    finally:
        np.random.set_state(state)
    if len(ivf.active_centers) != want:
        return "inactive centres: the reference's grouping asserts on them"
    return ivf, cent, qs, left_out


def edge_removal(m, rng):
    """Rows to remove so that the lists have sizes in EDGE_SIZES (a list shorter than 15 stays; with kp >= 2 a row
    leaves all its lists, so lists met later may end below their size — exact for kp = 1)."""
    dead = np.zeros(m.N, dtype=bool)
    settled = np.zeros(m.N, dtype=bool)         # members of the lists already at their size
    for l in rng.permutation(m.L):
        live = m.ids[l][~dead[m.ids[l]]]
        fit = [s for s in EDGE_SIZES if s <= len(live)]
        if not fit:
            continue
        target = int(rng.choice(fit))
        free = np.unique(live[~settled[live]])
        rng.shuffle(free)
        for r in free:
            if len(live) <= target:
                break
            dead[r] = True
            live = live[live != r]
        settled[live] = True
    return np.flatnonzero(dead).astype(np.int64)


def draw_op(case, m, rng, state, force=None, prepare=True):
    """One change drawn against the model's present state -> the op dict.  state: what is still owed (activate: the
    centre the next add brings in).  prepare=False: the rows alone (X), for an index that assigns and encodes them
    itself."""
    ivf, kp = case.ivf, m.kp
    stored = m.stored_ids()
    gone = np.setdiff1d(np.arange(m.N), stored)
    added = np.arange(case.N0, m.N)
    kind = force or str(rng.choice(["add", "remove", "remove", "update", "update"]))
    op = dict(kind=kind, sel=None, ids=None, X=None, new=None, near=None, labels=None, groups=None)

    def some(a, frac=0.1):
        return rng.choice(a, max(1, int(frac * len(a))), replace=False).astype(np.int64)

    if kind == "add":
        n = int(rng.choice(ADD_SIZES))
        op["sel"] = f"n={n}"
        centre = None
        if state.get("activate"):               # the rows that activate the centre the build left out
            centre, op["sel"] = state.pop("activate"), f"n={n} activating"
        op["X"] = case.rows_near(rng, n, centre)
    elif kind == "remove":
        sel = str(rng.choice(REMOVE_KINDS)) if force is None else "all"
        if sel == "gone" and len(gone) == 0 or sel == "added" and len(added) == 0 or len(stored) == 0 and sel != "gone":
            sel = "tenth" if len(stored) else "gone"
        if sel == "tenth":
            ids = some(stored)
        elif sel == "list":
            full = np.flatnonzero(m.sizes > 0)
            ids = rng.permutation(m.ids[int(rng.choice(full))])
        elif sel == "all":
            ids = rng.permutation(stored)
        elif sel == "gone":
            ids = some(gone, 0.5) if len(gone) else np.zeros(0, np.int64)
        elif sel == "dups":
            ids = some(stored)
            ids = np.concatenate([ids, ids[:max(1, len(ids) // 2)], ids[:1], gone[:3]])
        else:
            ids = some(added, 0.5)
        op["sel"], op["ids"] = sel, np.ascontiguousarray(ids, dtype=np.int64)
    else:
        sel = str(rng.choice(UPDATE_KINDS))
        if sel == "removed" and len(gone) == 0 or sel == "added" and len(added) == 0:
            sel = "random"
        if sel in ("random", "all", "same", "one") and len(stored) == 0:
            sel = "removed"
        if sel == "random":
            ids = some(stored)
        elif sel == "removed":
            ids = some(gone, 0.5)
        elif sel == "added":
            ids = some(added, 0.5)
        elif sel == "all":
            ids = rng.permutation(stored)
        elif sel == "same":
            ids = some(stored, 0.3)
        else:
            ids = some(stored)[:1]
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        op["sel"], op["ids"] = sel, ids
        # (their own vectors as IVF.data holds them: prepared again, they go back to their lists)
        op["X"] = m.data[ids].copy() if sel == "same" else case.rows_near(rng, len(ids))
    if op["X"] is not None:
        if prepare:
            op["new"], op["near"], op["labels"] = prepared(ivf, op["X"], kp)
        if m.groups is not None:
            op["groups"] = rng.randint(0, 5, size=len(op["X"])).astype(np.int32)
    return op


def _build(seed):
    case = Case(seed)
    c = case.shape
    made = _index(c, seed)
    if isinstance(made, str):
        case.skipped = made
        return case
    ivf, case.cent, qs, case.left_out = made
    case.ivf, case.N0 = ivf, len(ivf.data)
    rng = np.random.RandomState(STREAM + 300000 + seed)
    if c["groups"]:
        ivf.set_groups(rng.randint(0, 5, size=case.N0).astype(np.int32))
    case.qs = qs
    qn, qp = ivf._prepare(qs.copy())
    case.qn, case.qp = np.ascontiguousarray(qn), np.ascontiguousarray(qp)
    m = case.model()
    state = {}
    if c["activate"]:
        state["activate"] = c["n_clusters"] - 1
    case.ops = ops = []

    def take(op):
        ops.append(op)
        m.apply(op)

    if c["steered"]:            # step 0: down to the edge sizes
        take(dict(kind="remove", sel="edges", ids=edge_removal(m, rng), X=None, new=None, near=None, labels=None,
                  groups=None))
    n_ops = c["n_ops"]
    empty_at = int(rng.randint(0, n_ops - 1)) if c["empty_then_add"] else -1
    act_at = int(rng.randint(0, n_ops)) if c["activate"] else -1
    i = 0
    while i < n_ops:
        if i == empty_at:
            take(draw_op(case, m, rng, state, force="remove"))
            take(draw_op(case, m, rng, state, force="add"))
            i += 2
            continue
        take(draw_op(case, m, rng, state, force="add" if i == act_at and "activate" in state else None))
        i += 1
    if "activate" in state:     # (its step was taken by the pair above)
        take(draw_op(case, m, rng, state, force="add"))
    return case


@functools.lru_cache(maxsize=None)
def case(seed):
    """The case of a seed: built once per process and shared; its users change nothing in it (fresh_ivf() is theirs)."""
    return _build(int(seed))


# ---- what a case holds: the coverage conditions of tests/test_list_chain_cpu.py ----

def _chunks(sizes):
    return (np.asarray(sizes) + 15) // 16


def step_facts(before, op, after, N0):
    """dict of booleans over one step; before / after: dict(sizes, cols, off, stored) of the model around it"""
    s0, s1 = before["sizes"], after["sizes"]
    L0 = len(s0)
    s0 = np.concatenate([s0, np.zeros(len(s1) - L0, np.int64)])
    c0, c1 = _chunks(s0), _chunks(s1)
    off0 = np.concatenate([[0], np.cumsum(c0)])[:-1]
    off1 = np.concatenate([[0], np.cumsum(c1)])[:-1]
    cols = after["cols"]
    out = dict(
        up16=bool(((c1 > c0) & (s0 > 0)).any()),
        down16=bool(((c1 < c0) & (s1 > 0)).any()),
        emptied=bool(((s0 > 0) & (s1 == 0)).any()),
        refilled=bool(((s0[:L0] == 0) & (s1[:L0] > 0)).any()),
        offsets_shift=bool(((off0 % 8 != off1 % 8) & (s1 > 0))[1:].any()),
        empty_block=bool(((cols == 0).any(axis=1) & (cols > 0).any(axis=1)).any()) if cols.shape[1] > 1 else False,
        stores_removed_again=op["kind"] == "update" and bool((~np.isin(op["ids"], before["stored"])).any()),
        names_added=op["kind"] != "add" and bool((op["ids"] >= N0).any()),
        add_into_empty=op["kind"] == "add" and s0.sum() == 0,
        noop_remove=op["kind"] == "remove" and len(op["ids"]) > 0 and not np.isin(op["ids"], before["stored"]).any(),
        removes_all=op["kind"] == "remove" and s0.sum() > 0 and s1.sum() == 0,
        activates=len(s1) > L0,
        big_block=False,
    )
    if op["near"] is not None:
        near = op["near"]
        out["big_block"] = any(np.bincount(near[:, j]).max() > 16 for j in range(near.shape[1]))
    return out


def _view(m):
    return dict(sizes=m.sizes, cols=m.cols.copy(), stored=m.stored_ids())


def _allocated(nbytes):
    """what the library allocates for a buffer of nbytes (api_internal.h: DevBuf::ensure leaves an eighth + 256 spare)"""
    return nbytes + nbytes // 8 + 256


def facts(case):
    """dict over one case, from the model alone: steps: the step_facts of every step; small: the whole code array was
    at most 7 chunks at some point; one_list; kp; M; store; adds_in_place / adds_grown: the adds whose rows fit behind
    the old ones in the device's vector buffer as an upload of the built index allocates it, and those that need a
    larger one (the two branches of tk_index_add_rows' step 1)."""
    m = case.model()
    views = [_view(m)]
    steps = []
    row_bytes = m.data.shape[1] * {"float32": 4, "float16": 2, "float64": 8}[case.shape["store"]]
    cap, in_place, grown = _allocated(m.N * row_bytes), 0, 0
    for op in case.ops:
        if op["kind"] == "add":
            need = (m.N + len(op["X"])) * row_bytes
            in_place += need <= cap
            grown += need > cap
            cap = cap if need <= cap else _allocated(need)
        m.apply(op)
        views.append(_view(m))
        steps.append(step_facts(views[-2], op, views[-1], case.N0))
    emptied_then_added = any(a["removes_all"] and any(b["add_into_empty"] for b in steps[i + 1:])
                             for i, a in enumerate(steps))
    return dict(
        steps=steps,
        small=any(1 <= _chunks(v["sizes"]).sum() <= 7 for v in views),
        one_list=case.shape["n_clusters"] == 1,
        kp=m.kp, M=len(m.zero), store=case.shape["store"],
        emptied_then_added=emptied_then_added,
        adds_in_place=in_place, adds_grown=grown,
    )
