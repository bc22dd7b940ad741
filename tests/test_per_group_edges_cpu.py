"""A census, from the CPU reference alone, of what tests/test_per_group_edges_gpu.py and
tests/test_per_group_fuzz_gpu.py run the device on (tests/per_group_edge_shapes.py): a change to the generators cannot
silently empty a category.  The conditions are on the INPUTS — where in a query's ranking the capped walk
(cap_select.h) ends, which ranking of the staged body a shape takes, which kernel launch_float_sums picks — none is a
measurement of the device.

"last kept rank": the rank of a query's last returned id within its full ranking; chunk c holds the ranks
64 c .. 64 c + 63."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import per_group_edge_shapes as es  # noqa: E402
import restricted_shapes as rs  # noqa: E402


def _facts(name, R, k, a, m):
    """of one leg: per query the last kept rank, the count, the candidates; the queries the cap changes"""
    ids, _, counts, ranked = ref = es.reference(name, R, k, a, m)
    plain = es.reference(name, R, k, "own", 1)[0]          # all-distinct groups: the uncapped answer
    return dict(last=es.last_kept_ranks(ref), counts=counts, nc=np.array([len(c) for c, _ in ranked]),
                changed=int((ids != plain).any(axis=1).sum()))


def _ties(name, R, k):
    return sum(len(np.unique(d)) < len(d) for _, d in es.reference(name, R, k, "own", 1)[3])


def test_the_grid_is_the_one_asked_for():
    assert es.R_GRID == (63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257) and es.K_GRID == (1, 10, 63, 64, 65, 100)
    assert set(es.LEGS) >= {("mod3", 1), ("lists", 2), ("near5", 1), ("near5", 3), ("oct", 1)}
    assert any(m == "mix" for _, m in es.LEGS) and set(es.caps("mix").tolist()) == {0, 1, 3}
    assert len(es.grid("twins")) == sum(k < R for R in es.R_GRID for k in es.K_GRID)
    for name in es.INDEXES:
        if name != "twins":
            assert set(es.grid(name)) >= {(R, k) for R in (65, 128, 129, 256, 257) for k in (1, 10, 64, 65) if k < R}
    assert es.NQ == 32 and es.N_PROBES == 5


def test_census_of_twins(oracle):
    """the conditions of the full grid, on the index with rows stored twice"""
    name = "twins"
    by_chunk, full_late, short_late = {}, {}, {}
    tails = {64: 0, 65: 0, 100: 0}
    sixty_five = 0
    for R, k in es.grid(name):
        assert (es.heaps(name, k, R) != -1).all()       # every heap is full: nc = R, pass_1 sets what the kernels walk
        for a, m in es.LEGS:
            f = _facts(name, R, k, a, m)
            last, counts, nc = f["last"], f["counts"], f["nc"]
            for c in range(5):
                by_chunk[R, c] = max(by_chunk.get((R, c), 0), int((last // 64 == c).sum()))
            full_late[R] = max(full_late.get(R, 0), int(((counts == k) & (last >= 64)).sum()))
            short_late[R] = max(short_late.get(R, 0), int(((counts < k) & (nc > k) & (last >= 64)).sum()))
            # "Between 1 and 63 slots of -1 after a kept id at position >= 64", asked at k = 64 and 65, is read here as
            # RANK >= 64: an output position >= 64 needs 65 kept ids, which k = 64 cannot hold and which at k = 65 leaves
            # no -1.  So at k = 64, 65: a row whose walk went beyond rank 63 ends with 1 to 63 slots of -1, one partial
            # stride of the fill; the literal condition, output position >= 64 with such a tail, is asserted at k = 100
            late_tail = (last >= 64) & (k - counts >= 1) & (k - counts <= 63)
            if k in (64, 65):
                tails[k] += int(late_tail.sum())
            if k == 100:
                tails[k] += int((late_tail & (counts >= 65)).sum())
            if k == 65:
                sixty_five += int((counts == 65).sum())
            # changed answers.  (oct, 1) at k = 10 is left out of the half: rows of one id // 8 are unrelated rows, and
            # among a query's ten nearest two of them meet on 3 or 4 queries of 32 (asserted: at least 3); from k = 63
            # on it changes all 32
            if k >= 10:
                if (a, k) == ("oct", 10):
                    assert f["changed"] >= 3, (R, k, a, m, f["changed"])
                else:
                    assert 2 * f["changed"] >= es.NQ, (R, k, a, m, f["changed"])
        ties = _ties(name, R, k)
        if R >= 192:
            assert ties == es.NQ, (R, k, ties)          # every ranking holds a tie: the positional walk
        assert ties >= 8, (R, k, ties)
    for R in es.R_GRID:
        if R <= 64:
            continue
        for c in (1, 2, 3, 4):
            reached = R - 64 * c                        # ranks of chunk c that R holds
            if reached <= 0:
                continue
            # chunks 1 to 3: 8 queries of some leg, also where R reaches the chunk with one rank alone (R = 65, 129,
            # 193: the near2 leg); chunk 4 is the single rank 256: 3 queries
            need = 3 if c == 4 else 8
            assert by_chunk[R, c] >= need, (R, c, by_chunk[R, c])
        if R >= 127:
            assert full_late[R] >= 8 and short_late[R] >= 8, (R, full_late[R], short_late[R])
    assert sixty_five >= 1 and min(tails.values()) >= 1, (sixty_five, tails)
    print("census twins: queries ending in chunk c, best leg per R:",
          {R: [by_chunk[R, c] for c in range(5)] for R in es.R_GRID},
          "| full late", full_late, "| short late", short_late, "| rows with 65 kept at k = 65:", sixty_five,
          "| partial fill strides behind a late rank at k = 64 / 65, behind position 64 at k = 100:", tails)


@pytest.mark.parametrize("name", [n for n in es.INDEXES if n != "twins"])
def test_census_of_the_thin_grids(oracle, name):
    best = {}
    for R, k in es.grid(name):
        assert (es.heaps(name, k, R) != -1).all()
        ties = _ties(name, R, k)
        if name in es.NO_TIES:
            assert ties == 0, (name, R, k, ties)        # no two candidates at one distance: the strict-count ranking
        for a, m in es.LEGS:
            f = _facts(name, R, k, a, m)
            if k >= 10 and (a, k) != ("oct", 10):
                assert 2 * f["changed"] >= es.NQ, (name, R, k, a, m, f["changed"])
            for c in range(5):
                best[R, c] = max(best.get((R, c), 0), int((f["last"] // 64 == c).sum()))
    # the walks end in every chunk the heap reaches, as on twins
    for R in es.THIN_R:
        for c in (1, 2, 3, 4):
            reached = R - 64 * c
            if reached > 0:
                assert best[R, c] >= (3 if c == 4 else 8), (name, R, c, best[R, c])
    print(f"census {name}: queries ending in chunk c, best leg per R:", {R: [best[R, c] for c in range(5)] for R in es.THIN_R})


def test_which_kernel_a_shape_takes():
    """the label es.staged (the rule of rescore.hip's launch_float_sums, stated there once)"""
    table = {}
    for name in es.INDEXES:
        for R in sorted({R for R, _ in es.grid(name)}):
            table[name, R] = "".join("s" if es.staged(name, R, form) else "r" for form in es.FORMS)
            assert not es.staged(name, R, 0)
            if R == 257 or name in es.ODD or name == "f64":
                assert table[name, R] == "rrr", (name, R)
    # d = 256: form 1's tile of 65 rows is 67 600 bytes by itself, so it is staged at no R; form 2 is up to R = 256
    assert es.staged("wide", 256, 2) and not es.staged("wide", 256, 1)
    assert not any(es.staged("wide", R, 1) for R in range(1, 258))
    # the staged kernel under both tile forms on both sides of every ranking width, float32 and half rows
    for name in ("twins", "distinct", "distinct16"):
        for R in (65, 128, 129, 256):
            assert table[name, R] == "rss", (name, R)
    print("staged (s) or lane-per-row (r) under forms 0, 1, 2:", {f"{n} {R}": v for (n, R), v in table.items()})


def test_the_largest_admitted_heap():
    """es.largest_admitted_heap is the last R of the formula it restates (api_index.hip, the `per_group:` check; the
    GPU test shows that the library admits this R and refuses the next)"""

    def lds(R, d, dsz):
        return R * (8 + dsz) + d * dsz + 32 + R * (8 + dsz + 4)
    for d, dsz in ((20, 4), (20, 8), (100, 4), (17, 4)):
        R = es.largest_admitted_heap(d, dsz)
        assert lds(R, d, dsz) <= 64 * 1024 < lds(R + 1, d, dsz)
    assert es.largest_admitted_heap(20, 4) == 2336 and es.largest_admitted_heap(20, 8) == 1815


@pytest.mark.parametrize("name", ["twins", "f64"])
def test_census_of_the_largest_heap(oracle, name):
    d, dtype, _ = es.INDEXES[name]
    R = es.largest_admitted_heap(d, np.dtype(dtype).itemsize)
    for a, m in es.LARGEST_LEGS:
        ref = es.reference(name, R, es.LARGEST_K, a, m, es.LARGEST_PROBES)
        nc = np.array([len(c) for c, _ in ref[3]])
        last = es.last_kept_ranks(ref)
        early = int((ref[2] < es.LARGEST_K).sum())
        print(f"census largest heap {name} ({a}, {m}): R = {R}, candidates {nc.min()} .. {nc.max()}, last kept rank "
              f"{last.min()} .. {last.max()}, rows that end early {early}")
        # every list probed: every heap holds min(R, the 2000 rows) candidates
        assert nc.min() == min(R, es.N), nc.min()
        if a == "lists":        # one row of each of a query's ten nearest lists: kept rows beyond the staged kernels' 256 ranks
            assert early == 0 and (last >= 256).sum() >= 16, last
        else:                   # three groups: every walk goes through all 29 / 32 chunks and ends early
            assert early == es.NQ


# ---- the fuzz cases (tests/test_per_group_fuzz_gpu.py): counted over the 32 default cases of restricted_shapes -------

def test_census_of_the_fuzz_cases(oracle):
    changed, odd, half, short_late, late_big, k50_short, k1 = [], [], [], [], [], [], []
    for seed in range(rs.DEFAULT_SEEDS):
        t = es.fuzz_case(seed)
        assert t.skipped is None, (seed, t.skipped)
        c = t.case.shape
        ids, _, counts, ranked = want = t.want()
        nc = np.array([len(r[0]) for r in ranked])
        last = es.last_kept_ranks(want)
        assert set(np.unique(t.caps).tolist()) <= {0, 1, 2, 3} and len(t.groups) == len(t.case.ref_data)
        if (ids != t.uncapped()[0]).any():
            changed.append(seed)
            if c["d"] % 4:
                odd.append(seed)
            if c["store"] == "float16":
                half.append(seed)
        if ((counts < c["k"]) & (nc > c["k"])).any():
            short_late.append(seed)
        if t.R > 256 and last.max(initial=-1) >= 128:
            late_big.append((seed, t.R, int(last.max())))
        if c["k"] == 50 and (nc <= c["k"]).any():
            k50_short.append(seed)
        if c["k"] == 1:
            k1.append(seed)
    print(f"census fuzz: the cap changes {len(changed)} cases {changed}, {len(odd)} of them d % 4 != 0, {len(half)} on "
          f"the half store; {len(short_late)} cases with a row ending in -1 with nc > k {short_late}; R > 256 and a "
          f"last kept rank >= 128: {late_big}; k = 50 with nc <= k: {k50_short}; k = 1: {k1}")
    assert len(changed) >= 10 and len(odd) >= 6 and len(half) >= 5, (changed, odd, half)
    assert len(short_late) >= 6 and late_big and k50_short and k1
