"""The replays' duplicate test (`insert`, _fast_pq.pyx:284-287) on labels and lists chosen against it
(tests/label_shapes.py; the conditions each case rests on: tests/test_label_shapes_cpu.py):

  A. the hash set of the lane replay with more colliding labels in a heap than its buckets and stash hold: the full scan
     of the heap's labels, the removal of labels the set never took, entries freed in the same round
  B. labels on both sides of 0xffffff: the register heap's label24 entries and their "no row" value, the hash on labels
     with high bits, no twin table
  C. 9, 17 and 18 copies of every label: twin tables of width 8 and 16, none at 18 — and there the LDS rule that hands a
     heap of 124 entries over 40 probed lists to the packed kernel
  D. 4 096 and 4 097 lists: the largest per-list bitmap of the TWIN form, and the 64-bit mask + search that replaces it

Every batch first asserts the replay form it was written for (DeviceIndex.last_replay), then compares the probe lists, the
heap arrays with their layout and the ids of EVERY query with the CPU oracle's, exactly."""
import numpy as np
import pytest

import label_shapes as ls
from pq_shapes import oracle_answers

pytestmark = pytest.mark.gpu


class _Case:
    """one index on the device, its oracle, its queries, and the oracle's answers per setting (computed once)"""

    def __init__(self, oracle, ivf, qn, qp):
        from tinyknn_amd import _lib
        assert _lib.device_count() >= 1, "no GPU visible"
        self.lib, self.ivf, self.qn, self.qp = _lib, ivf, qn, qp
        self.ox = ls.oracle_of(oracle, ivf)
        self.dev = ivf.device_index()
        self._want = {}

    def want(self, k, n_probes, pass_1=None):
        key = (k, n_probes, pass_1)
        if key not in self._want:
            self._want[key] = oracle_answers(self.ox, self.qn, k, n_probes, pass_1)
        return self._want[key]

    def check(self, k, n_probes, pass_1=None, *, form, plain_ran=None, **reported):
        """one batch: the form it took (and what else last_replay reports about it; plain_ran: whether the plain kernel
        scored lists of it), then everything against the oracle"""
        out, dbg = self.dev.query_batch(self.qn, self.qp, k, n_probes, pass_1=pass_1, debug=True)
        took = self.dev.last_replay()
        assert took["form"] == form, (took, self.lib.REPLAY_NAMES[form])
        for what, value in reported.items():
            assert took[what] == value, (what, took)
        if plain_ran is not None:
            stats = self.dev.plain_stats()
            assert (stats["plain_units"] > 0) == plain_ran, (plain_ran, stats)
        want = self.want(k, n_probes, pass_1)
        np.testing.assert_array_equal(dbg["probes"], want["probes"])
        np.testing.assert_array_equal(dbg["heap_val"], want["heap_val"])
        np.testing.assert_array_equal(dbg["heap_idx"], want["heap_idx"])
        np.testing.assert_array_equal(out, want["ids"])

    def reset(self):
        self.dev.set_option(self.lib.OPT_REPLAY_LAZY, -1)
        self.dev.set_option(self.lib.OPT_REPLAY_TWIN, 1)
        self.dev.set_heap_mode(0)
        self.dev.set_scan_mode(0)
        self.dev.set_plain_scan(True)

    def close(self):
        self.dev.close()
        self.ivf._dev = None


# ---- A. the hash set over its capacity --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case_a(oracle):
    a = ls.case_a(oracle)
    cases = {nb: _Case(oracle, a[nb]["ivf"], a["qn"], a["qp"]) for nb in (8, 4)}
    yield cases
    for c in cases.values():
        c.close()


@pytest.mark.parametrize("plain", [False, "always"])
@pytest.mark.parametrize("buckets,n_probes,pass_1", ls.A_SETTINGS)
def test_a_hash_set_over_capacity(case_a, buckets, n_probes, pass_1, plain):
    """heaps of 111 and 149 (the form's largest) with more labels of 8 buckets in every target's heap than the 36 those
    buckets and the stash hold, heaps of 21 whose 21 labels all belong to 4 buckets (capacity 20: over by one); the exact
    scan alone, and the plain sums behind the heads (the re-scan + second replay of the queries the hash-set form flags:
    asserted to have run — and not to have where the packed kernel takes the batch).
    A heap of 149 fits the form's LDS rule (tk_lanes_dedupe_fits: heap, label slots, set, slot table and staging of a
    64-query wave within 160 KiB, so that two 32-query workgroups share a CU) beside 8 probed lists, 163 584 B; beside
    10 it is 164 608 B and the batch is the packed kernel's — same labels, same answers."""
    c = case_a[buckets]
    fits = not (pass_1 == 149 and n_probes > 8)
    c.dev.set_option(c.lib.OPT_REPLAY_TWIN, 0)
    c.dev.set_plain_scan(plain)
    try:
        c.check(ls.A_K, n_probes, pass_1, form=c.lib.REPLAY_LANES_DEDUPE if fits else c.lib.REPLAY_PACKED, twin_w=0,
                plain_ran=bool(plain) and fits)
    finally:
        c.reset()


@pytest.mark.parametrize("heap_mode,form", [(0, "REPLAY_LANES_TWIN"), (1, "REPLAY_GENERAL"), (2, "REPLAY_PACKED"),
                                            (3, "REPLAY_PAIR")])
def test_a_the_other_replays_on_the_same_labels(case_a, heap_mode, form):
    c = case_a[8]
    c.dev.set_heap_mode(heap_mode)
    try:
        c.check(ls.A_K, ls.A_PROBES, form=getattr(c.lib, form))
    finally:
        c.reset()


# ---- B. the 24-bit boundary -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[0, 1, 2], ids=["max_0xfffffe", "max_above_0xffffff", "max_0xffffff"])
def case_b(request, oracle):
    b = ls.case_b(oracle, request.param)
    c = _Case(oracle, b["ivf"], b["qn"], b["qp"])
    c.labels24 = int(request.param == 0)
    yield c
    c.close()                     # (512 MB of vectors: an index goes before the next is made)


def test_b_labels_too_sparse_for_a_twin_table(case_b):
    assert case_b.dev.twin_table_width() == 0


@pytest.mark.parametrize("n_probes", ls.B_PROBES)
def test_b_register_heap_entries_follow_the_largest_label(case_b, n_probes):
    """heaps of 111 / 211 / 411 entries: two / four / eight nodes per lane; value8 << 24 | label24 entries up to a largest
    label of 0xfffffe, (value, label64) entries from 0xffffff on — which as a label24 would read "no row" """
    c = case_b
    c.dev.set_heap_mode(3)
    try:
        c.check(ls.B_K, n_probes, form=c.lib.REPLAY_PAIR, labels24=c.labels24)
    finally:
        c.reset()


def test_b_hash_set_on_labels_with_high_bits(case_b):
    c = case_b
    try:
        c.check(ls.B_K, ls.B_PROBES[0], form=c.lib.REPLAY_LANES_DEDUPE)
    finally:
        c.reset()


@pytest.mark.parametrize("heap_mode,form", [(1, "REPLAY_GENERAL"), (2, "REPLAY_PACKED")])
def test_b_wave_kernels(case_b, heap_mode, form):
    c = case_b
    c.dev.set_heap_mode(heap_mode)
    try:
        c.check(ls.B_K, ls.B_PROBES[0], form=getattr(c.lib, form))
    finally:
        c.reset()


# ---- C. copies per label ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def c_cases(oracle):
    made = {}

    def get(build_probes):
        if build_probes not in made:
            x = ls.case_c(oracle, build_probes)
            made[build_probes] = _Case(oracle, x["ivf"], x["qn"], x["qp"])
            made[build_probes].build_probes = build_probes
        return made[build_probes]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module", params=[9, 17, 18])
def case_c(request, c_cases):
    return c_cases(request.param)


@pytest.fixture(scope="module", params=[9, 17])
def case_c_twin(request, c_cases):
    return c_cases(request.param)


def test_c_twin_table_width(case_c):
    """2 .. 17 copies of a label: a table of the other 1 .. 16; 18 copies: none"""
    assert case_c.dev.twin_table_width() == (case_c.build_probes - 1 if case_c.build_probes <= 17 else 0)


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("k,n_probes", ls.C_SETTINGS)
def test_c_twin_form_at_every_width(case_c_twin, k, n_probes, lazy):
    """tables of 8 and 16 other copies per row (the suite's other indexes have 1 or 2)"""
    c = case_c_twin
    c.dev.set_option(c.lib.OPT_REPLAY_LAZY, lazy)
    try:
        c.check(k, n_probes, form=c.lib.REPLAY_LANES_TWIN, lazy=lazy, twin_w=c.build_probes - 1)
    finally:
        c.reset()


@pytest.mark.parametrize("k,n_probes,form", [(10, 3, "REPLAY_LANES_DEDUPE"), (2, 40, "REPLAY_LANES_DEDUPE"),
                                             (3, 40, "REPLAY_PACKED")])
def test_c_label_forms(case_c, k, n_probes, form):
    """without the table (switched off at 9 and 17 copies, refused at 18): the hash set up to a heap of 83 entries over
    40 probed lists, and the packed kernel at 124, where heap, label slots, set and slot table no longer fit the LDS"""
    c = case_c
    c.dev.set_option(c.lib.OPT_REPLAY_TWIN, 0)
    try:
        c.check(k, n_probes, form=getattr(c.lib, form), twin_w=0)
    finally:
        c.reset()


@pytest.mark.parametrize("heap_mode,form", [(1, "REPLAY_GENERAL"), (2, "REPLAY_PACKED"), (3, "REPLAY_PAIR")])
def test_c_wave_kernels(case_c, heap_mode, form):
    c = case_c
    c.dev.set_heap_mode(heap_mode)
    try:
        for k, n_probes in ls.C_SETTINGS:
            c.check(k, n_probes, form=getattr(c.lib, form))
    finally:
        c.reset()


# ---- D. more lists than the bitmap holds ------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[4096, 4097])
def case_d(request, oracle):
    x = ls.case_d(oracle, request.param)
    c = _Case(oracle, x["ivf"], x["qn"], x["qp"])
    yield c
    c.close()


@pytest.mark.parametrize("lazy", [0, 1])
@pytest.mark.parametrize("plain", [False, "always"])
@pytest.mark.parametrize("n_probes", ls.D_PROBES)
def test_d_twin_form_with_the_largest_bitmap_and_with_none(case_d, n_probes, plain, lazy):
    """4 096 lists: 128 bitmap words per query, 32 KB per wave; 4 097: a 64-bit mask of `list & 63` and a search of the
    probe list — at 100 probed lists most of the 64 bits are set and the search decides.
    Plain sums need the list-major scan, which 300 queries over 4 096 lists do not get by themselves (it starts at 8
    probed lists per list of the index): the "always" runs ask for it, and assert that the plain kernel scored lists."""
    c = case_d
    assert c.dev.twin_table_width() == 1
    c.dev.set_option(c.lib.OPT_REPLAY_LAZY, lazy)
    c.dev.set_plain_scan(plain)
    if plain:
        c.dev.set_scan_mode(2)
    try:
        c.check(ls.D_K, n_probes, form=c.lib.REPLAY_LANES_TWIN, lazy=lazy, twin_w=1, plain_ran=bool(plain))
    finally:
        c.reset()
