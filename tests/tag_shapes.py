"""What tests/test_tags_gpu.py runs the device on, made without a GPU so that tests/test_tags_cpu.py can assert on the
reference alone that these inputs can tell a right tag pass from a wrong one: the four tag assignments over an index's
rows, the query masks of a batch, and the synthetic index of the replay-form legs."""
import numpy as np

MODES = ("any", "all")
ASSIGNMENTS = ("edges", "some", "lists", "nested")
EDGE_BITS = (0, 31, 32, 63)         # the two words of a mask and their edges
ACROSS = (1 << 31) | (1 << 32)      # two bits, one in each word
U64 = np.uint64
RARE = 47                           # "some": the tag only the rows with all 64 carry


def bit(t):
    return U64(1) << U64(t)


def first_list(ids_per_list, N):
    """the (lowest) list every row is stored in, 0 for a row stored nowhere"""
    first = np.zeros(N, dtype=np.int64)
    for l in reversed(range(len(ids_per_list))):
        first[np.asarray(ids_per_list[l], dtype=np.int64)] = l
    return first


def assignments(ids_per_list, N, seed):
    """name -> (N,) uint64:
    edges   every row one random bit of {0, 31, 32, 63};
    some    every row 1 to 3 random bits, a tenth of the rows none, a few rows all 64 (the random bits are drawn from
            the 63 tags other than RARE, so that one tag is carried by those few rows alone: the nearest thing to
            "a bit no row carries" that an assignment with rows carrying every tag allows);
    lists   bit = the lowest list the row is stored in, mod 64: whole lists pass or fail;
    nested  every row bit 5, half of them bit 40 too: in "all" mode a two-bit mask separates superset from subset."""
    rng = np.random.default_rng(seed)
    edges = bit(0) << rng.choice(np.array(EDGE_BITS, dtype=U64), N)
    some = np.zeros(N, dtype=U64)
    others = np.array([t for t in range(64) if t != RARE], dtype=U64)
    for j in range(3):
        some |= np.where(rng.random(N) < (1.0 if j == 0 else 0.5), bit(0) << others[rng.integers(0, 63, N)], U64(0))
    some[rng.random(N) < 0.1] = 0
    some[rng.choice(N, max(2, N // 1000), replace=False)] = U64(0xffffffffffffffff)
    lists = bit(0) << (first_list(ids_per_list, N) % 64).astype(U64)
    nested = np.where(rng.random(N) < 0.5, bit(5) | bit(40), bit(5))
    return dict(edges=edges, some=some, lists=lists, nested=nested)


def carriers(tags):
    """rows per tag, 64 counts"""
    return np.array([int(((tags >> U64(t)) & U64(1)).sum()) for t in range(64)])


def absent_bit(tags):
    """The tag the fewest rows carry, the highest such: no row at all where the assignment leaves a tag free (edges,
    lists below 64 lists, nested), else only the rows that carry every tag (some).  In the high word where it can be:
    a compare of the low words alone sees no mask at all for it."""
    n = carriers(tags)
    return int(np.flatnonzero(n == n.min())[-1])


def query_masks(tags, nq, seed):
    """One mask per query, the kinds in turn: one tag that rows carry; 0; the absent tag; one tag of each word
    (1 << 31 | 1 << 32); two carried tags, one of each word where both words have one; one carried tag of the high
    word where it has one."""
    rng = np.random.default_rng(seed)
    present = np.flatnonzero(carriers(tags) > 0)
    low, high = present[present < 32], present[present >= 32]
    m = np.zeros(nq, dtype=U64)
    for i in range(nq):
        kind = i % 6
        if kind == 0:
            m[i] = bit(rng.choice(present))
        elif kind == 2:
            m[i] = bit(absent_bit(tags))
        elif kind == 3:
            m[i] = U64(ACROSS)
        elif kind == 4:
            a, b = (rng.choice(low), rng.choice(high)) if len(low) and len(high) else rng.choice(present, 2)
            m[i] = bit(a) | bit(b)
        elif kind == 5:
            m[i] = bit(rng.choice(high if len(high) else present))
    return m


def low_words(a):
    """what a compare of the low dwords alone would see"""
    return np.asarray(a, dtype=U64) & U64(0xffffffff)


# ---- the synthetic index of tests/test_groups_gpu.py's `synthetic` fixture, with one list emptied and one cut to
# exactly 16 rows (one whole chunk, no padding row) ----

SYN_N, SYN_D, SYN_NQ = 40000, 48, 256
_made = {}


def synthetic(kp):
    """-> (ivf built on the host with n_probes = kp then trimmed, raw queries, tags of its rows, the emptied list, the
    list of 16 rows); made once per process, its users change nothing in it"""
    if "base" not in _made:
        import tinyknn_amd as tk
        state = np.random.get_state()
        np.random.seed(5)
        try:
            cent = np.random.randn(150, SYN_D)
            X = (cent[np.random.randint(150, size=SYN_N)] + 0.6 * np.random.randn(SYN_N, SYN_D)).astype(np.float32)
            qs = (cent[np.random.randint(150, size=SYN_NQ)] + 0.6 * np.random.randn(SYN_NQ, SYN_D)).astype(np.float32)
            base = tk.IVF("euclidean", 160, tk.FastPQ(2, rotate_dim=None))      # unrotated: the reference is fed qn
            base.fit(X[:15000])
        finally:
            np.random.set_state(state)
        assert base.pq.R is None
        _made["base"] = (base, X, qs)
    if kp not in _made:
        import tinyknn_amd as tk
        base, X, qs = _made["base"]
        ivf = tk.IVF("euclidean", 160, None)
        ivf.all_centers, ivf.pq = base.all_centers, base.pq
        ivf.build(X, n_probes=kp, device=False)
        L = len(ivf.active_centers)
        sizes = np.array([len(ivf.ids[l]) for l in range(L)])
        emptied = int(np.argsort(sizes)[L // 2])
        ivf.remove(np.asarray(ivf.ids[emptied], dtype=np.int64))
        sizes = np.array([len(ivf.ids[l]) for l in range(L)])
        cut = int(np.argmax(sizes))
        ivf.remove(np.asarray(ivf.ids[cut], dtype=np.int64)[16:])
        sizes = np.array([len(ivf.ids[l]) for l in range(L)])
        assert sizes[emptied] == 0 and sizes[cut] == 16 and (sizes % 16 != 0).sum() > L // 2, sizes
        tags = assignments([ivf.ids[l] for l in range(L)], SYN_N, 8)["some"]
        _made[kp] = (ivf, qs, tags, emptied, cut)
    return _made[kp]


def synthetic_masks(tags, mode):
    return query_masks(tags, SYN_NQ, 9 + MODES.index(mode))


# ---- the fuzz cases: the awkward indexes of tests/restricted_shapes.py, each with tags drawn on top ----

FUZZ_DEFAULT_SEEDS = 16
# Where the fuzz seeds start among the cases of tests/restricted_shapes.py (seed i here is its case FUZZ_FIRST + i),
# and where the tags' own random streams start.  Chosen so that the default seeds hold what
# tests/test_tags_fuzz_cpu.py asserts.
FUZZ_FIRST = 0
FUZZ_STREAM = 5100
TAG_KINDS = ("single", "some", "lists", "zero")
MASK_KINDS = ("none", "one", "across", "absent")
_fuzz = {}


def fuzz_seeds():
    """the seeds of a run: FUZZ_DEFAULT_SEEDS, or TINYKNN_FUZZ_SEEDS as in the other fuzz files"""
    import os
    return range(int(os.environ.get("TINYKNN_FUZZ_SEEDS", str(FUZZ_DEFAULT_SEEDS))))


class TagCase:
    """case: the restricted_shapes.Case (unchanged, shared); tags (uint64 per row of its index after the layout
    change), tag_kind, mode, masks (uint64 per query), mask_kinds: drawn from the seed's own stream"""

    def __init__(self, seed):
        import restricted_shapes as rs
        self.seed = seed
        self.case = case = rs.case(FUZZ_FIRST + seed)
        self.skipped = case.skipped
        if self.skipped is not None:
            return
        rng = np.random.RandomState(FUZZ_STREAM + seed)
        N, nq, L = len(case.ref_data), len(case.qn), case.shape["n_clusters"]
        self.tag_kind = kind = TAG_KINDS[rng.randint(len(TAG_KINDS))]
        self.mode = MODES[rng.randint(2)]
        # (every kind draws from tags 0 .. 62: tag 63 is carried by no row, so an "absent" mask always has a tag to ask for)
        if kind == "single":
            tags = bit(0) << rng.randint(0, 63, N).astype(U64)
        elif kind == "some":
            tags = np.zeros(N, dtype=U64)
            for j in range(3):
                tags |= np.where(rng.rand(N) < (1.0 if j == 0 else 0.5), bit(0) << rng.randint(0, 63, N).astype(U64), U64(0))
        elif kind == "lists":
            tags = bit(0) << (first_list([case.ivf.ids[l] for l in range(L)], N) % 63 * 9 % 63).astype(U64)
        else:
            tags = np.zeros(N, dtype=U64)
        self.tags = tags
        present = np.flatnonzero(carriers(tags) > 0)
        low, high = present[present < 32], present[present >= 32]
        free = np.flatnonzero(carriers(tags) == 0)
        assert len(free) and free[-1] == 63, (seed, kind)
        self.mask_kinds = [MASK_KINDS[rng.randint(len(MASK_KINDS))] for _ in range(nq)]
        masks = np.zeros(nq, dtype=U64)
        for i, mk in enumerate(self.mask_kinds):
            if mk == "one":
                masks[i] = bit(rng.choice(present) if len(present) else rng.randint(64))
            elif mk == "across":    # one tag of each word: carried ones where both words have some
                a, b = (rng.choice(low), rng.choice(high)) if len(low) and len(high) else (rng.randint(32), 32 + rng.randint(32))
                masks[i] = bit(a) | bit(b)
            elif mk == "absent":    # (never empty: tag 63 at the least)
                masks[i] = bit(rng.choice(free))
        self.masks = masks

    def __repr__(self):
        return f"tags seed {self.seed} {self.tag_kind} {self.mode} on {self.case}"

    def device_kwargs(self, aset=None):
        kw = self.case.device_kwargs(aset)
        kw.update(tags=self.masks, tags_mode=self.mode)
        return kw

    def want(self):
        """the reference answer under the case's own restriction and the tags (ids, debug): computed once"""
        if "_want" not in self.__dict__:
            from oracle import oracle
            from tags_reference import tagged_batch
            c = self.case
            self.__dict__["_want"] = tagged_batch(oracle, c.ox, c.qn, self.masks, self.mode, self.tags, c.shape["k"],
                                                 c.shape["n_probes"], allowed=c.allowed, exclude=c.exclude,
                                                 group=c.group, groups=c.groups, debug=True)
        return self.__dict__["_want"]


def fuzz_case(seed):
    if seed not in _fuzz:
        _fuzz[seed] = TagCase(int(seed))
    return _fuzz[seed]
