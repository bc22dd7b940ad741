"""The wire harness without a GPU (tests/shard_wire.py): the oracle engine on BOTH sides, planted faults that
the comparisons must catch, and — from the oracle alone — that the legs tests/test_shard_wire_gpu.py runs hold
the categories its comparisons are meant to meet."""
import numpy as np
import pytest

import shard_wire as sw

from shard_wire import FIXTURE_LEGS, FUZZ_SEEDS

_cases = {}


def case(oracle, name):
    """fixture tag or fuzz seed -> the case, built once per session"""
    if name not in _cases:
        _cases[name] = sw.fuzz_case(oracle, name) if isinstance(name, int) else sw.fixture_case(oracle, name, with_ivf=False)
    return _cases[name]


def both_oracle(oracle, c, world, n_probes, coarse="home", capacity=None, stages=sw.ALL_STAGES):
    return sw.run_both(None, c["ox"], world, c["qn"], c["qp"], c["k"], n_probes, O=oracle, coarse=coarse,
                       capacity=capacity, stages=stages, sides=("oracle", "oracle"))


def crossed(plan, a, b, want):
    """side a's bytes into side b's finish calls: the engine's own assertions are the check, ids the oracle's"""
    np.testing.assert_array_equal(b.cross_finish(a.out["dense"]["send"]), want)
    if "two" in a.out:
        plain = plan.eng.plain_queries(plan.raw, plan.f["tables_raw"], a.out["two"]["reduced"], plan.capacity)
        np.testing.assert_array_equal(b.cross_finish(a.out["two"]["send"], plain=plain), want)
    for what in ("one", "head"):
        np.testing.assert_array_equal(b.cross_finish(a.out[what]["send"], plain="blocks"), want)
    f = a.out["filter"]
    for reverse in (False, True):
        np.testing.assert_array_equal(b.cross_finish_filtered(f["counts"], f["records"], reverse=reverse), want)


@pytest.mark.parametrize("tag,n_probes,world,coarse", [("an100", 5, 3, "home"), ("eu20", 2, 2, "replicated"),
                                                       ("an100b2", 5, 2, "home")])
def test_harness_oracle_against_oracle_fixture(oracle, tag, n_probes, world, coarse):
    c = case(oracle, tag)
    plan, a, b = both_oracle(oracle, c, world, n_probes, coarse)
    sw.check_all(plan, a.out, b.out, coarse, one_phase_content=True)
    assert not any(a.out["dense"]["flag"]) and max(a.out["dense"]["usage"]) == plan.usage
    crossed(plan, a, b, c["goldens"][n_probes])
    # exactly as much room as the longest stream: nothing overflows, neighbours intact; a quarter: flagged
    plan, a, b = both_oracle(oracle, c, world, n_probes, coarse, capacity=plan.usage, stages=("dense",))
    assert not sw.check_send(plan, a.out, b.out)
    plan, a, b = both_oracle(oracle, c, world, n_probes, coarse, capacity=max(1, plan.usage // 4), stages=("dense",))
    assert sw.check_send(plan, a.out, b.out)


@pytest.mark.parametrize("seed", [1, 6, 12, 15])
def test_harness_oracle_against_oracle_fuzz(oracle, seed):
    c = case(oracle, seed)
    assert c is not None
    plan, a, b = both_oracle(oracle, c, c["world"], c["n_probes"], "home", capacity=c["capacity"])
    sw.check_all(plan, a.out, b.out, "home", one_phase_content=True)
    crossed(plan, a, b, c["ox"].query_batch(c["qn"], c["k"], c["n_probes"]))


def test_planted_faults_fail_the_comparison(oracle):
    """One byte of one segment flipped, one record dropped, one segment written one block further on: each must
    fail (and the untouched copy must pass)."""
    import copy
    c = case(oracle, "an100")
    plan, a, b = both_oracle(oracle, c, 3, 5, "home")
    sw.check_all(plan, a.out, b.out, "home", one_phase_content=True)
    rank = max(range(3), key=lambda r: len(plan.segments(r)))
    i, s, at, n = [x for x in plan.segments(rank) if x[3] >= 32][-1]

    bad = copy.deepcopy(b.out)
    bad["dense"]["send"][rank][at + n - 1] ^= 0x01
    with pytest.raises(AssertionError, match=f"query {i} slot {s} .* block {n // 16 - 1}"):
        sw.check_send(plan, a.out, bad)

    bad = copy.deepcopy(b.out)
    cnt, rec = bad["filter"]["counts"][rank], bad["filter"]["records"][rank]
    h = int(np.flatnonzero(cnt[:3])[0])
    o = int(cnt[:h].sum())
    bad["filter"]["records"][rank] = np.concatenate([rec[:o], rec[o + 1:], rec[:1]])     # (same room, one record gone)
    with pytest.raises(AssertionError, match="keys only on side a"):
        sw.check_filter(plan, a.out, bad)
    cnt[h] -= 1                                                                          # ... and with its count
    with pytest.raises(AssertionError, match="records per home"):
        sw.check_filter(plan, a.out, bad)

    bad = copy.deepcopy(b.out)
    buf = bad["dense"]["send"][rank]
    seg = buf[at:at + n].copy()
    buf[at:at + 16] = sw.FILL
    buf[at + 16:at + 16 + n] = seg                  # pos + 1
    with pytest.raises(AssertionError):
        sw.check_send(plan, a.out, bad)
    # the same shift on BOTH sides (ranks that agree with each other, not with the layout): the bytes that belong to
    # no segment give it away
    with pytest.raises(AssertionError, match="outside its segments|query"):
        sw.check_send(plan, bad, bad)


def test_default_legs_hold_the_categories(oracle):
    """Conditions on the legs of tests/test_shard_wire_gpu.py, from the oracle alone."""
    facts = []
    for tag, n_probes, world, coarse in FIXTURE_LEGS:
        c = case(oracle, tag)
        ox = c["ox"]
        owner = sw.shard_lists(np.asarray(ox.list_n), world)
        cap = sw.shard_capacity(np.asarray(ox.list_n), owner, world, len(c["qn"]), n_probes)
        plan = sw.Plan(oracle, ox, owner, world, c["qn"], c["k"], n_probes, None, cap)
        facts.append(((tag, n_probes, world, coarse), plan, sw.leg_facts(plan, c["k"], n_probes, None)))
    for seed in FUZZ_SEEDS:
        c = case(oracle, seed)
        assert c is not None, f"fuzz seed {seed} builds no index"
        owner = sw.shard_lists(np.asarray(c["ox"].list_n), c["world"])
        plan = sw.Plan(oracle, c["ox"], owner, c["world"], c["qn"], c["k"], c["n_probes"], None, c["capacity"])
        facts.append(((seed,), plan, sw.leg_facts(plan, c["k"], c["n_probes"], None)))
    count = lambda key: sum(1 for _, _, f in facts if f[key])
    assert count("mixed") >= 10, count("mixed")
    assert count("wrapped") >= 4, count("wrapped")
    assert count("short") >= 4, count("short")
    assert count("repeated") >= 3, count("repeated")
    assert count("no_home") >= 2, count("no_home")
    assert sum(1 for _, _, f in facts if f["rows_above_127"] > 0) >= 1
    assert facts[len(FIXTURE_LEGS) + 15][2]["rows_above_127"] > 0           # (fuzz seed 15)
    for leg, plan, f in facts:
        assert not (plan.pos < 0).any(), leg                                # no default leg overflows
        assert sum(f["segments"]) >= 1, leg
        for r in range(plan.world):
            assert f["segments"][r] >= 1 or not f["owns"][r], (leg, r)
