"""The helpers of tests/label_shapes.py and the conditions of tests/test_label_shapes_gpu.py, from the CPU oracle alone.

Renaming the rows of an index must change nothing but the names: the oracle over the relabelled arrays answers perm of
what it answered before, heap layout included.  And every GPU case there is written for one branch of one replay form;
what sends a batch into that branch — labels that overfill the hash set, a label at 0xffffff, every label arriving
build_probes times, two probed lists that share a row and a number modulo 64 — is asserted here from the reference's
own heaps and probe lists, so that no GPU case can pass without meeting its branch."""
import numpy as np
import pytest

import label_shapes as ls
from pq_shapes import oracle_answers


def _assert_equivariant(oracle, base, ox, rel, perm, qn, k, n_probes, pass_1=None):
    want = oracle_answers(ox, qn, k, n_probes, pass_1)
    got = oracle_answers(ls.oracle_of(oracle, rel), qn, k, n_probes, pass_1)
    np.testing.assert_array_equal(got["probes"], want["probes"])
    np.testing.assert_array_equal(got["heap_val"], want["heap_val"])
    np.testing.assert_array_equal(got["heap_idx"], ls.through(perm, want["heap_idx"]))
    np.testing.assert_array_equal(got["ids"], ls.through(perm, want["ids"]))
    assert (want["ids"] >= 0).any()


def test_the_exported_buckets_leave_enough_colliding_labels():
    """properties of tk_label_buckets, the kernel's own function: the counts the GPU cases need below 65 536"""
    l4, c4 = ls.labels_in_buckets(range(4), 65536)
    l8, c8 = ls.labels_in_buckets(range(8), 65536)
    assert (c4, c8) == (20, 36)
    assert len(l4) >= 200 and len(l8) >= 900
    assert set(l4.tolist()) <= set(l8.tolist())
    every, c64 = ls.labels_in_buckets(range(64), 4096)
    np.testing.assert_array_equal(every, np.arange(4096))
    assert c64 == 260


def test_perm_onto_is_a_bijection_that_keeps_the_other_rows_in_order():
    perm = ls.perm_onto([5, 2], [0, 9], 10)
    np.testing.assert_array_equal(perm, [1, 2, 9, 3, 4, 0, 5, 6, 7, 8])
    perm = ls.perm_onto([1], [2 ** 24 + 15], 2 ** 24 + 16, n=4)
    np.testing.assert_array_equal(perm, [0, 2 ** 24 + 15, 1, 2])
    for bad in (([1, 1], [2, 3]), ([1, 2], [3, 3]), ([1], [10]), ([10], [1])):
        with pytest.raises(AssertionError):
            ls.perm_onto(bad[0], bad[1], 10)


def test_relabelling_by_a_random_permutation_is_exact(oracle):
    a = ls.case_a(oracle)
    n = len(a["ivf"].data)
    perm = np.random.RandomState(7).permutation(n).astype(np.int64)
    rel = ls.relabelled(a["ivf"], perm, n)
    np.testing.assert_array_equal(rel.data[perm[:100]], a["ivf"].data[:100])
    _assert_equivariant(oracle, a["ivf"], a["ox"], rel, perm, a["qn"][:64], ls.A_K, ls.A_PROBES)
    # into more rows than there were: the unused ones are zero and never named
    wide = np.sort(np.random.RandomState(8).choice(3 * n, n, replace=False)).astype(np.int64)[perm]
    _assert_equivariant(oracle, a["ivf"], a["ox"], ls.relabelled(a["ivf"], wide, 3 * n), wide, a["qn"][:16], ls.A_K, 3)


@pytest.mark.parametrize("buckets,n_probes,pass_1", ls.A_SETTINGS)
def test_a_the_targets_heaps_overfill_the_hash_set(oracle, buckets, n_probes, pass_1):
    a = ls.case_a(oracle)
    c = a[buckets]
    _assert_equivariant(oracle, a["ivf"], a["ox"], c["ivf"], c["perm"], a["qn"], ls.A_K, n_probes, pass_1)
    assert c["capacity"] == 4 * buckets + 4
    colliding = set(c["labels"].tolist())
    ox = ls.oracle_of(oracle, c["ivf"])
    tq = a["qn"][:ls.A_TARGETS]
    final = ls.heap_rows(ox, tq, ls.A_K, n_probes, pass_1=pass_1)
    held = [sum(int(x) in colliding for x in h) for h in final]
    # more of them in one heap than both of their buckets' entries and the stash hold: the set overflows
    assert min(held) > c["capacity"], held
    if buckets == 8:
        # ... and, behind the first probed list, labels that leave the heap again (removal of labels the set never took)
        R = pass_1 or (n_probes + 1) * ls.A_K + 1
        first = ls.heap_rows(ox, tq, ls.A_K, 1, pass_1=R)
        held1 = [sum(int(x) in colliding for x in h) for h in first]
        gone = [sum(int(x) in colliding and int(x) not in set(f.tolist()) for x in h) for h, f in zip(first, final)]
        assert min(held1) > c["capacity"], held1
        assert sum(g > 0 for g in gone) >= 3, gone


@pytest.mark.parametrize("which", [0, 1, 2])
def test_b_the_labels_straddle_the_24_bit_boundary(oracle, which):
    b = ls.case_b(oracle, which)
    ids = np.concatenate(b["ivf"].ids)
    T = len(ids)
    assert ids.max() == (0xfffffe, ls.B_ROWS - 1, 0xffffff)[which]
    assert (ids == 0xffffff).any() == (which > 0)
    assert (ids.max() < 0xffffff) == (which == 0)               # install_lists' rule for label24 entries
    assert ids.max() + 1 > 8 * T + 1024                          # build_twins' rule: labels too sparse for a twin table
    assert b["ivf"].data.shape == (ls.B_ROWS, 8)
    base = b["base"]
    for n_probes in ls.B_PROBES:
        _assert_equivariant(oracle, base["ivf"], base["ox"], b["ivf"], b["perm"], b["qn"][:32], ls.B_K, n_probes)
    final = ls.heap_rows(ls.oracle_of(oracle, b["ivf"]), b["qn"], ls.B_K, ls.B_PROBES[0])
    for label in [int(ids.max())] + ([0xffffff] if which else []):
        assert sum(label in set(h.tolist()) for h in final) >= 8, hex(label)


@pytest.mark.parametrize("build_probes", [9, 17, 18])
def test_c_every_label_arrives_build_probes_times(oracle, build_probes):
    c = ls.case_c(oracle, build_probes)
    ivf = c["ivf"]
    assert len(ivf.active_centers) == 40
    ids, counts = np.unique(np.concatenate(ivf.ids), return_counts=True)
    assert len(ids) == 3000 and (counts == build_probes).all()
    for i in range(40):                                          # a label at most once per list: TWIN's premise
        assert len(np.unique(ivf.ids[i])) == len(ivf.ids[i])
    for k, n_probes in ls.C_SETTINGS:
        want = oracle_answers(c["ox"], c["qn"], k, n_probes)
        if n_probes == 40:
            assert (np.sort(want["probes"], axis=1) == np.arange(40)).all()      # every list: every copy arrives
        full = 0
        for h, got in zip(want["heap_idx"], want["ids"]):
            held = h[h >= 0]
            assert len(np.unique(held)) == len(held)             # `insert` let no label in twice
            full += len(np.unique(got[got >= 0])) == k
        assert 2 * full >= len(c["qn"]), (k, n_probes, full)


@pytest.mark.parametrize("n_lists", [4096, 4097])
def test_d_probed_lists_that_share_a_row_and_a_number_modulo_64(oracle, n_lists):
    d = ls.case_d(oracle, n_lists)
    ivf = d["ivf"]
    assert len(ivf.active_centers) == n_lists and sum(len(x) for x in ivf.ids) == 140000
    want = oracle_answers(d["ox"], d["qn"], ls.D_K, ls.D_PROBES[1])
    assert want["heap_idx"].shape[1] == 102                      # R = (100 + 1) * 1 + 1
    # where every stored row's copies are: lists_of[row] = its two lists
    lists_of = np.full((70000, 2), -1, dtype=np.int64)
    for i in range(n_lists):
        rows = np.asarray(ivf.ids[i], dtype=np.int64)
        col = (lists_of[rows, 0] >= 0).astype(np.int64)
        lists_of[rows, col] = i
    assert (lists_of >= 0).all() and (lists_of[:, 0] != lists_of[:, 1]).all()
    shared = masked = 0
    for probes in want["probes"]:
        # two probed lists with one number modulo 64, one holding a copy of a row of the other: the search of the
        # probe list has to tell them apart
        found = False
        for r in np.unique(probes & 63):
            same = probes[(probes & 63) == r]
            for i in range(len(same)):
                for j in range(i + 1, len(same)):
                    found |= bool(np.intersect1d(ivf.ids[same[i]], ivf.ids[same[j]]).size)
        shared += found
        # a row whose other copy lies in a list NOT replayed before, which the 64-bit mask takes for one that was
        fooled = False
        for s in range(1, len(probes)):
            rows = np.asarray(ivf.ids[probes[s]], dtype=np.int64)
            other = np.where(lists_of[rows, 0] == probes[s], lists_of[rows, 1], lists_of[rows, 0])
            before = probes[:s]
            fooled |= bool((~np.isin(other, before) & np.isin(other & 63, before & 63)).any())
        masked += fooled
    assert shared >= 50 and masked >= 50, (shared, masked)
