"""The HIP engine of the list-sharded index against the CPU engine, byte for byte, stage by stage
(tests/shard_wire.py runs W ranks of each in lock step; exact equality throughout).

What is compared per rank: the home form's probe lists; every owned segment of the dense scan, its overflow flag
and usage, and that no byte outside the rank's segments (4096 guard bytes behind the last region included) lost its
0xAB; the bound bytes and their MIN; counts and the SETS of filter records per home group, compact and in regions,
with regions one record too small flagged on both sides; the two-phase scan (first lists exact; behind them
clip(plain sum) where the model's rule says plain, exact elsewhere) and the device's books of it, which pin its table
limits C to the numpy ones; the one-phase forms per 16-byte block (exact or plain, the head of the first list exact)
and the head bounds.  Then the exchange crossed: the model's buffers and records through the device's finish calls
(ids of the oracle), the device's through the model's, whose own assertions check every received byte.

Both scan kernels write whole 16-byte blocks of their own segments only (the plain kernel masks the chunks past a
list and the pairs past a tile: plain_scan.hip `flush`), so the strict form holds: outside a rank's segments nothing
is written unless a region overflowed (then the plain kernel scores the segment that did not fit to the buffer's
tail: api_shard.hip).

Where the one-phase form does not apply to a leg (tk_index_shard_scan_head_dev then IS tk_index_shard_scan_dev and
answers 255 for every query) the whole buffer must be the dense scan's; legs with distinct labels where the form's
conditions hold must not take that way out."""
import numpy as np
import pytest

import shard_wire as sw

pytestmark = pytest.mark.gpu
_cases = {}


def case(oracle, name):
    if name not in _cases:
        _cases[name] = sw.fuzz_case(oracle, name) if isinstance(name, int) else sw.fixture_case(oracle, name)
    return _cases[name]


def lock_step(oracle, c, world, n_probes, coarse, capacity=None, want=None):
    """All stages on both engines, every comparison, the crossed exchange both ways."""
    plan, hip, orc = sw.run_both(c["ivf"], c["ox"], world, c["qn"], c["qp"], c["k"], n_probes, O=oracle, coarse=coarse,
                                 capacity=capacity)
    try:
        sw.check_all(plan, hip.out, orc.out, coarse)
        eng = plan.eng
        R = eng._heap_size(c["k"], n_probes, None)
        if eng.ids_unique and plan.S >= 2 and c["ox"].M <= 52:
            assert plan.two_phase, "tk_index_shard_plain: distinct labels, two probed lists, M <= 52 — the two-phase form applies"
        if plan.two_phase and eng.ids_unique and R <= 574 and world * plan.capacity >= int(plan.chunks.max()):
            assert not plan.fell_back, "the one-phase form applies here: the head scan must not answer 255 throughout"
        if want is None:
            want = c["ox"].query_batch(c["qn"], c["k"], n_probes)
        # the model's bytes and records through the device's finish calls
        np.testing.assert_array_equal(hip.cross_finish(orc.out["dense"]["send"]), want)
        f = orc.out["filter"]
        for reverse in (False, True):
            np.testing.assert_array_equal(hip.cross_finish_filtered(f["counts"], f["records"], reverse=reverse), want)
        if plan.two_phase:
            np.testing.assert_array_equal(hip.cross_finish(orc.out["two"]["send"]), want)
        # the device's through the model's, which checks every byte it receives against its own rule
        np.testing.assert_array_equal(orc.cross_finish(hip.out["dense"]["send"]), want)
        if plan.two_phase:
            plain = eng.plain_queries(plan.raw, plan.f["tables_raw"], hip.out["two"]["reduced"], plan.capacity)
            assert int(plain.sum()) == hip.out["two"]["books"][0][1]
            np.testing.assert_array_equal(orc.cross_finish(hip.out["two"]["send"], plain=plain), want)
        for what in ("one", "head"):
            np.testing.assert_array_equal(orc.cross_finish(hip.out[what]["send"], plain="blocks"), want)
        f = hip.out["filter"]
        np.testing.assert_array_equal(orc.cross_finish_filtered(f["counts"], f["records"]), want)
        # what the leg met, for whoever measures (tests/test_shard_wire_cpu.py holds the conditions on it)
        plan.met = dict(two_phase=plan.two_phase, plain_queries=hip.out["two"]["books"][0][1] if plan.two_phase else 0,
                        plain_pairs=sum(b[0] for b in hip.out["two"]["books"]) if plan.two_phase else 0,
                        fell_back=plan.fell_back, repeated=not eng.ids_unique,
                        bounds_below_rail=int((hip.out["bound"]["reduced"] != 255).sum()),
                        head_bounds_below_rail=int((hip.out["head"]["reduced"] != 255).sum()),
                        records=int(sum(c_[:world].sum() for c_ in hip.out["filter"]["counts"])),
                        blocks=int(sum(c_[2 * world:].sum() for c_ in hip.out["filter"]["counts"])))
        return plan, hip.out["dense"]["usage"]
    finally:
        sw.close_engines(hip.engines)


@pytest.mark.parametrize("tag,n_probes,world,coarse", sw.FIXTURE_LEGS)
def test_wire_fixture(oracle, tag, n_probes, world, coarse):
    c = case(oracle, tag)
    lock_step(oracle, c, world, n_probes, coarse, want=c["goldens"][n_probes])


@pytest.mark.parametrize("seed", sw.FUZZ_SEEDS)
def test_wire_fuzz(oracle, seed):
    """n_probes above the list count, wrapped probe lists, empty and sub-chunk lists, repeated labels, nq below W."""
    c = case(oracle, seed)
    assert c is not None, "the host build rejects this shape"
    lock_step(oracle, c, c["world"], c["n_probes"], "home", capacity=c["capacity"])


@pytest.mark.parametrize("tag", sw.FIXTURE_TAGS)
def test_wire_tight_fit_and_overflow(oracle, tag):
    """capacity == usage: every region exactly full somewhere, neighbours' segments intact, nothing flagged;
    a quarter of it: both sides flag, and what fitted is equal."""
    c = case(oracle, tag)
    world, n_probes = 3, 5
    plan, usage = lock_step(oracle, c, world, n_probes, "home", want=c["goldens"][n_probes])
    assert max(usage) == plan.usage           # (per rank: its own streams; the callers max-reduce)
    tight, _ = lock_step(oracle, c, world, n_probes, "home", capacity=plan.usage, want=c["goldens"][n_probes])
    assert not (tight.pos < 0).any() and int((tight.pos + tight.chunks[tight.probes]).max()) == tight.capacity
    plan, hip, orc = sw.run_both(c["ivf"], c["ox"], world, c["qn"], c["qp"], c["k"], n_probes, O=oracle,
                                 capacity=max(1, plan.usage // 4), stages=("dense",))
    try:
        assert sw.check_send(plan, hip.out, orc.out), "a quarter of the longest stream must overflow"
        assert any(f & 1 for f in hip.out["dense"]["flag"]) and any(f & 1 for f in orc.out["dense"]["flag"])
        assert (plan.pos >= 0).any()            # (some segments did fit and were compared)
    finally:
        sw.close_engines(hip.engines)
