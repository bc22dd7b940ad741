"""hipGraph capture of every kind of query_batch_dev call (BASELINE configs[3]: "hipGraph-captured batch").

tests/test_graph_capture_gpu.py, test_hip_parity.py::test_hipgraph_captured_batch and
test_store_gpu.py::test_captured_graph_replay capture one kind of call — unrestricted, ids only, the lane replay,
uncoalesced — and replay it with the bytes it was captured with.  Here every leg captures after ONE warm-up pass of the
same calls, and replays at least twice: with the inputs of the capture, and after a second input set of the same shape
has been copied into the SAME device buffers (queries, q_pq, every restriction array), against the reference's answer
for that set — whatever the host decided from capture-time data would show there.  Outputs hold a sentinel before
every replay.  Every comparison is exact: ids by assert_array_equal, distances bit for bit.

  leg 1   the replay forms (register heap, lanes / lanes_twin, general, packed) on the golden fixtures, plain scan off
          and "always", batches of 1, 3, 65 and all of a fixture's queries; the form is asserted
  leg 2   allowed / exclude / group on the awkward indexes of tests/restricted_shapes.py, replayed with the partner
          call's inputs (Case.second); tags, ranges and per_group caps replayed with a permutation of the queries and
          their arrays — each at depth 1, at depth 2 with two captured calls, at depth 2 as a coalesced pair, and at
          depth 1 with the plain limit at -128 (the exact re-scan of flagged queries inside the graph)
  leg 3   leg 2's depth-1 arrangement with dist_ptr (float32; float64 on float64 vectors; the half store)
  leg 4   gather_queries_dev + query_batch_dev(exclude_ptr=rows) in one graph, other rows written for replay 2
  leg 5   a first restricted call inside a capture is refused and enqueues nothing; knn_group / knn_between right
          after a capture has ended are not; the graph still answers after their tables were made; a held call
          flushed inside the capture by an entry point that takes no stream is captured like any other
  leg 6   tk_index_reserve: a 200-query call captured behind a 3-query warm-up

No leg runs a call larger than the captured one on an index between its capture and its last replay, no graph outlives
its index, and one index is in use at a time (the internal streams belong to the process)."""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import between_shapes as bs  # noqa: E402
import per_group_shapes as pgs  # noqa: E402
import restricted_shapes as rs  # noqa: E402
import tag_shapes as ts  # noqa: E402
from between_exact_reference import knn_between_reference  # noqa: E402
from conftest import golden  # noqa: E402
from group_exact_reference import knn_group_reference, stored_mask  # noqa: E402
from groups_reference import grouped_batch  # noqa: E402
from rows_reference import excluded_batch  # noqa: E402
from store_reference import exact_distances, oracle_index, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -7
REFUSAL = "cannot be made inside a stream capture"
PAIR_SEEDS = rs.pair_seeds(range(rs.DEFAULT_SEEDS))
TAG_SEEDS = list(ts.fuzz_seeds())[:4]
BETWEEN_SEEDS = list(bs.fuzz_seeds())[:4]
PER_GROUP_CASES = [("an100", "mod3", "mix", pgs.N_PROBES, False), ("syn", "syn8", 1, pgs.N_PROBES, False)]
ARRANGEMENTS = ("depth1", "depth2", "coalesced", "flagged")
# The plain scan finds units on the indexes of three of the ten pair seeds (11, 17, 29), stream-launched and captured
# alike; over the 32 default seeds on seven (tests/test_restricted_fuzz_gpu.py asks for six of those).  The other four
# run the forced-limit arrangement here beside the ten, so that six captured re-scans can be asked for.
FLAG_SEEDS = (16, 22, 28, 31)
# what leg 2 saw, by seed: the forms its captures took, the plain units of the forced-limit arrangement, whether
# the coalesced pair provably ran as one batch inside the graph (test_what_the_restricted_captures_ran asserts on them)
SEEN = {}


@pytest.fixture(scope="module")
def tk():
    import tinyknn_amd
    from tinyknn_amd import _lib
    assert _lib.device_count() >= 1, "no GPU visible"
    return tinyknn_amd


# ---- the harness -----------------------------------------------------------------------------------------------------

def _host(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.uint64 else a      # (tag masks travel as their bits)


def _dist_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.float64:
        return want.dtype == np.float64 and got.shape == want.shape and np.array_equal(got.view(np.uint64),
                                                                                      want.view(np.uint64))
    return got.dtype == np.float32 and same_bits(got, want)


class Call:
    """One query_batch_dev call: its device buffers, allocated once, and the input sets it is replayed with.  A set is
    a dict of numpy arrays: qn, qp, want (the reference's ids), want_dist where the call returns distances, and any of
    exclude / group / tags / between / per_group; every set names the same arrays with the same shapes.  queries: the
    (qn, qp) device tensors of a call whose queries another captured call writes (gather_queries_dev)."""
    ARRAYS = ("qn", "qp", "exclude", "group", "tags", "between", "per_group")

    def __init__(self, sets, k, n_probes, allowed=None, tags_mode="any", dist=None, queries=None, f64=None):
        import torch
        first = sets[0]
        self.sets, self.k, self.n_probes, self.allowed, self.tags_mode = sets, int(k), int(n_probes), allowed, tags_mode
        self.names = [a for a in self.ARRAYS if first.get(a) is not None]
        for s in sets:
            assert [a for a in self.ARRAYS if s.get(a) is not None] == self.names
            for a in self.names:
                assert _host(s[a]).shape == _host(first[a]).shape and _host(s[a]).dtype == _host(first[a]).dtype, a
        self.buf = {a: torch.from_numpy(_host(first[a]).copy()).cuda() for a in self.names}
        self.gathered = queries is not None
        if self.gathered:
            self.buf["qn"], self.buf["qp"] = queries
        self.nq = len(first["want"])
        self.f64 = int(first["qp"].dtype != np.float32) if f64 is None else int(f64)
        self.out = torch.full((self.nq, self.k), SENT, dtype=torch.int64, device="cuda")
        self.dist = None if dist is None else torch.full((self.nq, self.k), float(SENT), dtype=dist, device="cuda")

    def load(self, i):
        """input set i into the call's buffers, the sentinel into its outputs"""
        import torch
        for a in self.names:
            self.buf[a].copy_(torch.from_numpy(_host(self.sets[i][a]).copy()))
        if self.gathered:
            self.buf["qn"].fill_(float("nan"))
            self.buf["qp"].fill_(float("nan"))
        self.out.fill_(SENT)
        if self.dist is not None:
            self.dist.fill_(float(SENT))

    def enqueue(self, dev, st):
        p = lambda a: self.buf[a].data_ptr() if a in self.buf else None      # noqa: E731
        dev.query_batch_dev(p("qn"), p("qp"), self.f64, self.nq, self.k, self.n_probes, self.out.data_ptr(), stream=st,
                            allowed=self.allowed, dist_ptr=None if self.dist is None else self.dist.data_ptr(),
                            exclude_ptr=p("exclude"), group_ptr=p("group"), tags_ptr=p("tags"),
                            tags_mode=self.tags_mode, between_ptr=p("between"), per_group_ptr=p("per_group"))

    def untouched(self):
        return bool((self.out == SENT).all().item())

    def check(self, i, what):
        s = self.sets[i]
        ids = self.out.cpu().numpy()
        np.testing.assert_array_equal(ids, s["want"], err_msg=f"{what}, input set {i}")
        if self.dist is not None:
            d = self.dist.cpu().numpy()
            assert np.isposinf(d[ids == -1]).all(), f"{what}, input set {i}: a distance beside -1"
            assert _dist_bits(d, s["want_dist"]), f"{what}, input set {i}: distance bits"


def _enqueue(dev, calls, st, before=None, flush=None):
    if before is not None:
        before(st)
    for c in calls:
        c.enqueue(dev, st)
    if flush is not None:
        flush()
    dev.join(st)


def _capture(dev, calls, what, before=None, flush=None, warm_up=True, after_warm_up=None, quiesce_after=True):
    """tests/test_graph_capture_gpu.py's order: the calls once on a side stream, synchronize, quiesce, the same calls
    captured with join, quiesce -> the graph (the caller drops it before the index is closed).  before(stream): what is
    enqueued in front of the calls; flush(): an entry point that takes no stream, called between the calls and join."""
    import torch
    for c in calls:
        c.load(0)
    if warm_up:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            _enqueue(dev, calls, side.cuda_stream, before, flush)
        torch.cuda.synchronize()
        for c in calls:
            c.check(0, f"{what}: warm-up")
        if after_warm_up is not None:
            after_warm_up()
        for c in calls:
            c.load(0)
    dev.quiesce()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _enqueue(dev, calls, torch.cuda.current_stream().cuda_stream, before, flush)
    if quiesce_after:
        dev.quiesce()
    torch.cuda.synchronize()
    ran = not all(c.untouched() for c in calls)
    if ran:
        g = None            # (no graph outlives its index, on this path either)
    assert not ran, f"{what}: the capture ran something"
    return g


def _replay(g, calls, i, what, after=None):
    import torch
    for c in calls:
        c.load(i)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for c in calls:
        c.check(i, f"{what}: replay")
    if after is not None:
        after(i)


def _restore(dev):
    from tinyknn_amd import _lib
    dev.set_option(_lib.OPT_REPLAY_COUNT, 0)
    dev.set_pipeline(1)
    dev.set_coalesce(1)
    dev.set_heap_mode(0)
    dev.set_scan_mode(0)
    dev.set_plain_scan(True)
    dev.set_option(_lib.OPT_PAIR_NQ, 4)
    dev.set_option(_lib.OPT_PLAIN_LIMIT, 0x7fffffff)


@contextlib.contextmanager
def _opened(ivf, groups=None, tags=None, values=None, allowed=None):
    """-> (a device index of its own with the row attributes set, a prepared AllowSet or None); closed behind"""
    from tinyknn_amd.ivf import DeviceIndex
    dev = DeviceIndex(ivf)
    try:
        if groups is not None:
            dev.set_groups(groups)
        if tags is not None:
            dev.set_tags(tags)
        if values is not None:
            dev.set_values(values)
        yield dev, None if allowed is None else dev.allow(allowed)
    finally:
        dev.close()


# ---- leg 1: the replay forms ------------------------------------------------------------------------------------------

def _settings():
    from tinyknn_amd import _lib as L
    # name -> (OPT_PAIR_NQ, heap_mode, the forms the batch may take)
    return {"pair": (8192, 0, (L.REPLAY_PAIR,)),                            # the product default
            "lanes": (0, 0, (L.REPLAY_LANES, L.REPLAY_LANES_TWIN)),
            "general": (4, 1, (L.REPLAY_GENERAL,)),
            "packed": (4, 2, (L.REPLAY_PACKED, L.REPLAY_PACKED_DISTINCT))}


# (queries, n_probes, scan_mode): one query, three, more than a wave of lanes (the fixture's queries over again), the
# fixture's; every batch size under the automatic, the query-major (1) and the list-major (2) scan
SIZES = ((1, 10, 0), (1, 5, 1), (1, 10, 2), (3, 1, 1), (3, 5, 2), (3, 10, 0), (65, 5, 0), (65, 10, 1), (65, 5, 2),
         (None, 1, 2), (None, 5, 0), (None, 10, 1), (None, 10, 2))


@pytest.mark.parametrize("setting", ("pair", "lanes", "general", "packed"))
@pytest.mark.parametrize("tag", ("an100", "an100b2", "eu20f64"))
def test_replay_forms(tk, tag, setting):
    from tinyknn_amd import _lib
    from test_hip_parity import ivf_from_fixture
    fx = golden(f"g6_ivf_{tag}.npz")
    qn, qp = np.ascontiguousarray(fx["qn"]), np.ascontiguousarray(fx["qpq"])
    pair_nq, heap_mode, forms = _settings()[setting]
    with _opened(ivf_from_fixture(tk, fx)) as (dev, _):
        g = None
        try:
            dev.set_option(_lib.OPT_PAIR_NQ, pair_nq)
            dev.set_heap_mode(heap_mode)
            for n, n_probes, scan_mode in SIZES:
                n = len(qn) if n is None else n
                dev.set_scan_mode(scan_mode)
                want = fx[f"ids_p{n_probes}"]
                # replay 1: the fixture's queries in order, replay 2: in reverse order
                sets = [dict(qn=qn[i], qp=qp[i], want=want[i])
                        for i in (np.arange(n) % len(qn), (len(qn) - 1 - np.arange(n)) % len(qn))]
                for plain in (False, "always"):
                    what = f"{tag} {setting} nq={n} n_probes={n_probes} scan_mode={scan_mode} plain={plain}"
                    dev.set_plain_scan(plain)
                    calls = [Call(sets, 10, n_probes)]
                    g = _capture(dev, calls, what)
                    got = dev.last_replay()
                    assert got["form"] in forms, (what, got)
                    if setting == "lanes":
                        assert got["form"] == (_lib.REPLAY_LANES_TWIN if tag == "an100b2" else _lib.REPLAY_LANES), what
                    for i in (0, 1):
                        _replay(g, calls, i, what)
                    g = None
        finally:
            g = None
            _restore(dev)


# ---- leg 2: restrictions ---------------------------------------------------------------------------------------------

def _arrangements(open_dev, s0, s1, k, n_probes, what, tags_mode="any", arrangements=ARRANGEMENTS):
    """The call with input sets (s0, s1) captured in each arrangement on a fresh index; at depth 2 a second captured
    call takes the sets the other way round.  -> what was seen: forms, plain_units, joined"""
    from tinyknn_amd import _lib
    nq = len(s0["want"])
    seen = dict(forms=set(), plain_units=0, joined=False)
    for arrangement in arrangements:
        with open_dev() as (dev, aset):
            g = None
            name = f"{what} {arrangement}"
            make = lambda sets: Call(sets, k, n_probes, allowed=aset, tags_mode=tags_mode)     # noqa: E731
            try:
                if arrangement == "depth1":
                    dev.set_option(_lib.OPT_PAIR_NQ, 8192)      # the product default
                    calls = [make([s0, s1])]
                elif arrangement == "flagged":
                    dev.set_plain_scan("always")
                    dev.set_option(_lib.OPT_PLAIN_LIMIT, -128)  # every query with a plain list fails the lemma's check
                    calls = [make([s0, s1])]
                else:
                    dev.set_option(_lib.OPT_PAIR_NQ, 0)         # the lane kernels, which count waves
                    dev.set_pipeline(2)
                    if arrangement == "coalesced":
                        dev.set_coalesce(2)
                        dev.set_option(_lib.OPT_REPLAY_COUNT, 1)
                    calls = [make([s0, s1]), make([s1, s0])]
                launched = {}
                if arrangement == "flagged":        # (what the same call does stream-launched: the warm-up)
                    g = _capture(dev, calls, name, after_warm_up=lambda: launched.update(dev.plain_stats()))
                else:
                    g = _capture(dev, calls, name)
                form = dev.last_replay()
                seen["forms"].add(form["name"])
                if arrangement == "coalesced":
                    dev.replay_stats()                          # (counts from here)
                _replay(g, calls, 0, name)
                if arrangement == "coalesced":
                    # one launch over 2 nq rows has fewer waves of 64 than two launches (tests/test_restricted_fuzz_gpu.py)
                    alone, together = 2 * ((nq + 63) // 64), (2 * nq + 63) // 64
                    if form["form"] in (_lib.REPLAY_LANES, _lib.REPLAY_LANES_TWIN) and together < alone:
                        seen["joined"] = dev.replay_stats()["waves"] == together
                _replay(g, calls, 1, name)
                if arrangement == "flagged":
                    st = dev.plain_stats()
                    if st["plain_units"] > 0:
                        assert st["flagged_queries"] > 0, (name, st)
                    # the graph holds the plain scan the stream-launched call ran, unit for unit
                    assert st["plain_units"] == launched["plain_units"], (name, st, launched)
                    assert (st["flagged_queries"] > 0) == (launched["flagged_queries"] > 0), (name, st, launched)
                    seen["plain_units"] = st["plain_units"]
                g = None
            finally:
                g = None
                _restore(dev)
    return seen


def _pair_sets(case, oracle=None):
    """the case's call and its partner's (Case.second) as two input sets of one call: an exclude array in both (the
    case's own, or -1 for every query where it has none: the buffer is the partner's to fill), groups in both or
    neither; with the oracle, the exact distances of the answers too"""
    qn_b, qp_b, ex_b, gr_b, want_b = case.second()
    none = np.full(len(case.qn), -1, dtype=np.int64)
    s0 = dict(qn=case.qn, qp=case.qp, exclude=none if case.exclude is None else case.exclude, group=case.group,
              want=case.want()[0])
    s1 = dict(qn=qn_b, qp=qp_b, exclude=ex_b, group=gr_b, want=want_b)
    if oracle is not None:
        for s in (s0, s1):
            s["want_dist"] = exact_distances(oracle, s["qn"], case.ref_data, s["want"])
    return s0, s1


def _permuted(s0, seed):
    """the set with its queries — and every per-query array with them — in another order"""
    perm = np.random.RandomState(seed).permutation(len(s0["want"]))
    return {a: None if v is None else np.ascontiguousarray(v[perm]) for a, v in s0.items()}


def _case_opener(case, tags=None, values=None):
    return lambda: _opened(case.ivf, groups=case.groups, tags=tags, values=values, allowed=case.allowed)


def _restricted_case(seed):
    case = rs.case(seed)
    assert case.skipped is None, (case, case.skipped)
    return case


@pytest.mark.parametrize("seed", PAIR_SEEDS)
def test_allowed_exclude_group(tk, oracle, seed):
    case = _restricted_case(seed)
    s0, s1 = _pair_sets(case)
    SEEN[seed] = _arrangements(_case_opener(case), s0, s1, case.shape["k"], case.shape["n_probes"], str(case))


@pytest.mark.parametrize("seed", FLAG_SEEDS)
def test_flagged_rescan_on_further_indexes(tk, oracle, seed):
    case = _restricted_case(seed)
    s0, s1 = _pair_sets(case)
    SEEN[seed] = _arrangements(_case_opener(case), s0, s1, case.shape["k"], case.shape["n_probes"], str(case),
                               arrangements=("flagged",))


def _tag_sets(t, oracle=None):
    c = t.case
    s0 = dict(qn=c.qn, qp=c.qp, exclude=c.exclude, group=c.group, tags=t.masks, want=t.want()[0])
    if oracle is not None:
        s0["want_dist"] = exact_distances(oracle, c.qn, c.ref_data, s0["want"])
    return s0, _permuted(s0, 100 + t.seed)


@pytest.mark.parametrize("seed", TAG_SEEDS)
def test_tags(tk, oracle, seed):
    t = ts.fuzz_case(seed)
    assert t.skipped is None, t
    s0, s1 = _tag_sets(t)
    _arrangements(_case_opener(t.case, tags=t.tags), s0, s1, t.case.shape["k"], t.case.shape["n_probes"], str(t),
                  tags_mode=t.mode)


def _between_sets(t, dev, oracle=None):
    """(the ranges as the int64 keys the host path makes of them: DeviceIndex._ranges_of on an index with the values)"""
    c = t.case
    s0 = dict(qn=c.qn, qp=c.qp, exclude=c.exclude, group=c.group, tags=t.masks,
              between=dev._ranges_of(t.between, len(c.qn)), want=t.want()[0])
    if oracle is not None:
        s0["want_dist"] = exact_distances(oracle, c.qn, c.ref_data, s0["want"])
    return s0, _permuted(s0, 200 + t.seed)


@pytest.mark.parametrize("seed", BETWEEN_SEEDS)
def test_between(tk, oracle, seed):
    t = bs.fuzz_case(seed)
    assert t.skipped is None, t
    opener = _case_opener(t.case, tags=t.tags, values=t.values)
    with opener() as (dev, _):
        s0, s1 = _between_sets(t, dev)
    _arrangements(opener, s0, s1, t.case.shape["k"], t.case.shape["n_probes"], str(t), tags_mode=t.mode or "any")


def _per_group_sets(case):
    index = case[0]
    ivf, _, qn, qp = pgs.synthetic()[:4] if index == "syn" else pgs.fixture(index)
    _, _, groups, m, _ = pgs.case_inputs(case)
    ids, dist = pgs.reference(case)[:2]
    caps = np.ascontiguousarray(np.broadcast_to(np.asarray(m, dtype=np.int32), (len(qn),)))
    s0 = dict(qn=np.ascontiguousarray(qn), qp=np.ascontiguousarray(qp), per_group=caps, want=ids, want_dist=dist)
    return ivf, groups, s0, _permuted(s0, 300)


@pytest.mark.parametrize("case", PER_GROUP_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_per_group(tk, oracle, case):
    ivf, groups, s0, s1 = _per_group_sets(case)
    _arrangements(lambda: _opened(ivf, groups=groups), s0, s1, pgs.K, case[3], str(case))


def test_what_the_restricted_captures_ran(tk, oracle):
    """Nothing in an answer says which kernels a graph holds, so the takers are counted.  Over the ten pair seeds:
    every one ran; the register heap, both lane replays without a hash set and a replay with the duplicate test on
    labels were each captured; of the coalesced arrangements at least six provably replayed their pair as one batch
    (the number tests/test_restricted_fuzz_gpu.py::test_the_pairs_were_pairs asks of the same seeds stream-launched:
    the host decides a pair by the same rules inside a capture; measured: nine).  The forced-limit arrangement
    scanned plain units, flagged queries there (asserted where it ran) and so replayed the exact re-scan and the
    passes' `only` branch inside the graph on at least six seeds of the ten and FLAG_SEEDS together — measured: 11,
    17, 29 of the ten and all four of FLAG_SEEDS; per seed the arrangement asserts that the graph holds as many plain
    units as the same call stream-launched (its warm-up), so the three are the plain scan's, not the capture's."""
    for seed in PAIR_SEEDS:
        if seed not in SEEN:
            test_allowed_exclude_group(tk, oracle, seed)
    for seed in FLAG_SEEDS:
        if seed not in SEEN:
            test_flagged_rescan_on_further_indexes(tk, oracle, seed)
    assert all(s in SEEN for s in PAIR_SEEDS) and len(PAIR_SEEDS) == 10
    plain = [s for s in sorted(SEEN) if SEEN[s]["plain_units"] > 0]
    joined = [s for s in PAIR_SEEDS if SEEN[s]["joined"]]
    forms = set().union(*(SEEN[s]["forms"] for s in PAIR_SEEDS))
    print("captured restricted calls: plain units under the forced limit: seeds", plain, "| coalesced pairs proven:",
          joined, "| forms:", sorted(forms), {s: sorted(SEEN[s]["forms"]) for s in PAIR_SEEDS})
    assert len(plain) >= 6, plain
    assert {"pair", "lanes", "lanes_twin"} <= forms and forms & {"lanes_dedupe", "packed"}, forms
    assert len(joined) >= 6, joined


# ---- leg 3: distances ------------------------------------------------------------------------------------------------

def _depth1_with_distances(open_dev, s0, s1, k, n_probes, what, tags_mode="any", f64=False):
    import torch
    from tinyknn_amd import _lib
    with open_dev() as (dev, aset):
        g = None
        try:
            dev.set_option(_lib.OPT_PAIR_NQ, 8192)
            calls = [Call([s0, s1], k, n_probes, allowed=aset, tags_mode=tags_mode,
                          dist=torch.float64 if f64 else torch.float32)]
            g = _capture(dev, calls, what)
            for i in (0, 1):
                _replay(g, calls, i, what)
            g = None
        finally:
            g = None
            _restore(dev)


@pytest.mark.parametrize("seed", PAIR_SEEDS)
def test_distances_allowed_exclude_group(tk, oracle, seed):
    """(seeds 5, 8, 14, 26 and 29 keep their vectors in half precision: the distances of float32(float16(data)))"""
    case = _restricted_case(seed)
    s0, s1 = _pair_sets(case, oracle)
    _depth1_with_distances(_case_opener(case), s0, s1, case.shape["k"], case.shape["n_probes"], f"{case} distances")


def test_the_distance_leg_holds_a_half_store():
    assert any(rs.shape(s)["store"] == "float16" for s in PAIR_SEEDS)


@pytest.mark.parametrize("seed", TAG_SEEDS)
def test_distances_tags(tk, oracle, seed):
    t = ts.fuzz_case(seed)
    s0, s1 = _tag_sets(t, oracle)
    _depth1_with_distances(_case_opener(t.case, tags=t.tags), s0, s1, t.case.shape["k"], t.case.shape["n_probes"],
                           f"{t} distances", tags_mode=t.mode)


@pytest.mark.parametrize("seed", BETWEEN_SEEDS)
def test_distances_between(tk, oracle, seed):
    t = bs.fuzz_case(seed)
    opener = _case_opener(t.case, tags=t.tags, values=t.values)
    with opener() as (dev, _):
        s0, s1 = _between_sets(t, dev, oracle)
    _depth1_with_distances(opener, s0, s1, t.case.shape["k"], t.case.shape["n_probes"], f"{t} distances",
                           tags_mode=t.mode or "any")


@pytest.mark.parametrize("case", PER_GROUP_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_distances_per_group(tk, oracle, case):
    ivf, groups, s0, s1 = _per_group_sets(case)
    _depth1_with_distances(lambda: _opened(ivf, groups=groups), s0, s1, pgs.K, case[3], f"{case} distances")


def test_distances_float64_vectors(tk, oracle):
    """float64 vectors (eu20f64): the call writes float64 distances, numpy's promotion of float64 rows and float32
    queries; half of the rows allowed, each query's unrestricted top-1 excluded, then its top-2"""
    from test_hip_parity import ivf_from_fixture
    fx = golden("g6_ivf_eu20f64.npz")
    ivf = ivf_from_fixture(tk, fx)
    assert ivf.data.dtype == np.float64
    ox = oracle_index(oracle, ivf, ivf.data)
    qn, qp = np.ascontiguousarray(fx["qn"]), np.ascontiguousarray(fx["qpq"])
    allowed = np.random.RandomState(64).rand(len(ivf.data)) < 0.5
    sets = []
    for col in (0, 1):
        ex = np.ascontiguousarray(fx["ids_p5"][:, col], dtype=np.int64)
        want = excluded_batch(oracle, ox, qn, ex, 10, 5, allowed=allowed)
        wd = np.full(want.shape, np.inf, dtype=np.float64)
        for i in range(len(want)):
            live = want[i] != -1
            wd[i][live] = oracle.sqdist_gather(qn[i], ivf.data, want[i][live])
        sets.append(dict(qn=qn, qp=qp, exclude=ex, want=want, want_dist=wd))
    assert (sets[0]["want"] != sets[1]["want"]).any()
    _depth1_with_distances(lambda: _opened(ivf, allowed=allowed), sets[0], sets[1], 10, 5, "eu20f64 distances", f64=True)


# ---- leg 4: stored rows as queries -----------------------------------------------------------------------------------

ROW_SEEDS = (5, 11, 17)         # subsets with an exclude array; 5 and 11 rotate their PQ, 5 keeps half vectors


@pytest.mark.parametrize("seed", ROW_SEEDS)
def test_stored_rows_as_queries(tk, oracle, seed):
    import torch
    case = _restricted_case(seed)
    assert "e" in case.shape["subset"] and (seed != 5 or case.ivf.pq.R is not None)
    c = case.shape
    nq, N = len(case.rows), len(case.ref_data)
    other = np.random.RandomState(400 + seed).randint(N, size=nq).astype(np.int64)
    other[-1] = other[0]
    with _case_opener(case)() as (dev, aset):
        g = None
        try:
            assert dev.rotated() == (case.ivf.pq.R is not None)
            sets, made = [], []
            for rows in (case.rows, other):
                qn, qp = dev.gather_queries(rows)
                assert same_bits(qn, case.ref_data[rows]), "qn != float32(data[rows])"
                # (a rotated PQ: the reference is fed the device-made q_pq, so that both build the same tables)
                want = excluded_batch(oracle, case.ox, qn, rows, c["k"], c["n_probes"],
                                      q_pq=qp if dev.rotated() else None, allowed=case.allowed)
                sets.append(dict(exclude=rows, want=want))
                made.append((qn, qp))
            assert (sets[0]["want"] != sets[1]["want"]).any() or nq == 0
            qn_t = torch.zeros((nq, dev.d), dtype=torch.float32, device="cuda")
            qp_t = torch.zeros((nq, dev.dq), dtype=torch.float64 if dev.rotated() else torch.float32, device="cuda")
            call = Call(sets, c["k"], c["n_probes"], allowed=aset, queries=(qn_t, qp_t), f64=dev.rotated())
            rows_ptr = call.buf["exclude"].data_ptr()
            gather = lambda st: dev.gather_queries_dev(rows_ptr, nq, qn_t.data_ptr(), qp_t.data_ptr(), st)  # noqa: E731

            def queries_too(i):
                assert same_bits(qn_t.cpu().numpy(), made[i][0]), f"{case}: gathered qn, input set {i}"
                np.testing.assert_array_equal(qp_t.cpu().numpy(), made[i][1], err_msg=f"{case}: q_pq, input set {i}")

            g = _capture(dev, [call], str(case), before=gather)
            for i in (0, 1):
                _replay(g, [call], i, str(case), after=queries_too)
                assert not (call.out.cpu().numpy() == sets[i]["exclude"][:, None]).any(), "a row returned itself"
            g = None
        finally:
            g = None
            _restore(dev)


# ---- leg 5: table builds and the capture state -----------------------------------------------------------------------

def _first_restricted_call(kind):
    """-> (opener, the restricted call's set, k, n_probes, tags_mode, the unrestricted set) of an index on which a
    call of this kind needs a table that does not exist yet"""
    if kind == "exclude":
        case = _restricted_case(17)
        s = dict(qn=case.qn, qp=case.qp, exclude=case.exclude, want=case.want()[0])
        opener, mode = _case_opener(case), "any"
    elif kind == "group":
        case = _restricted_case(26)
        s = dict(qn=case.qn, qp=case.qp, group=case.group, want=case.want()[0])
        opener, mode = _case_opener(case), "any"
    elif kind == "tags":
        t = ts.fuzz_case(TAG_SEEDS[0])
        case, mode = t.case, t.mode
        s = _tag_sets(t)[0]
        opener = _case_opener(case, tags=t.tags)
    else:
        t = bs.fuzz_case(BETWEEN_SEEDS[0])
        case, mode = t.case, t.mode or "any"
        opener = _case_opener(case, tags=t.tags, values=t.values)
        with opener() as (dev, _):
            s = _between_sets(t, dev)[0]
    return opener, s, case.shape["k"], case.shape["n_probes"], mode, dict(qn=case.qn, qp=case.qp, want=case.base)


@pytest.mark.parametrize("kind", ("exclude", "group", "tags", "between"))
def test_first_restricted_call_inside_a_capture_is_refused(tk, oracle, kind):
    import torch
    opener, s, k, n_probes, mode, bare = _first_restricted_call(kind)
    with opener() as (dev, aset):
        g = None
        try:
            # the workspaces exist: an unrestricted call (no table of any kind is made by it)
            warm = Call([bare], k, n_probes)
            st = torch.cuda.current_stream().cuda_stream
            warm.enqueue(dev, st)
            dev.join(st)
            torch.cuda.synchronize()
            warm.check(0, f"{kind}: unrestricted warm-up")
            dev.quiesce()
            call = Call([s], k, n_probes, allowed=aset, tags_mode=mode)
            x = torch.zeros(8, dtype=torch.int64, device="cuda")
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                x.add_(1)           # (the graph is not empty)
                cs = torch.cuda.current_stream().cuda_stream
                with pytest.raises(AssertionError, match=REFUSAL):
                    call.enqueue(dev, cs)
                dev.join(cs)
            dev.quiesce()
            torch.cuda.synchronize()
            assert int(x.sum().item()) == 0 and call.untouched()
            g.replay()
            torch.cuda.synchronize()
            assert x.cpu().numpy().tolist() == [1] * 8, "the captured torch op"
            assert call.untouched(), "the refused call enqueued something"
            g = None
            # the same call stream-launched: the tables are made now, the answer is the reference's
            call.enqueue(dev, st)
            dev.join(st)
            torch.cuda.synchronize()
            call.check(0, f"{kind}: stream-launched after the capture")
        finally:
            g = None
            _restore(dev)


def test_exact_searches_right_after_a_capture_and_the_graph_after_them(tk, oracle):
    """The capture state belongs to the call that was given the capturing stream, not to the index: with no quiesce
    behind the capture, the first knn_group and the first knn_between — which take no stream and make their tables —
    answer as their references, and the graph captured before replays as before."""
    from test_hip_parity import ivf_from_fixture
    fx = golden("g6_ivf_an100.npz")
    ivf = ivf_from_fixture(tk, fx)
    N = len(ivf.data)
    qn, qp = np.ascontiguousarray(fx["qn"]), np.ascontiguousarray(fx["qpq"])
    groups = (np.arange(N) % 3).astype(np.int32)
    values = bs.assignments(ivf.ids, N, 71)["uniform"]
    stored = stored_mask(ivf.ids, N)
    want = fx["ids_p5"]
    sets = [dict(qn=qn, qp=qp, want=want), dict(qn=qn[::-1], qp=qp[::-1], want=want[::-1])]
    q16 = qn[:16]
    group = (np.arange(16) % 3).astype(np.int32)
    lo, hi, _ = bs.ranges(values, 16, 72, kinds=["two_sided", "low", "high", "point"] * 4)
    with _opened(ivf, groups=groups, values=values) as (dev, _):
        g = None
        try:
            calls = [Call(sets, 10, 5)]
            g = _capture(dev, calls, "an100", quiesce_after=False)
            ids, dist = dev.knn_group(q16, 10, group, return_distances=True)
            w_ids, w_dist = knn_group_reference(oracle, q16, ivf.data, 10, group, groups, stored=stored)
            np.testing.assert_array_equal(ids, w_ids)
            assert _dist_bits(dist, w_dist)
            ids, dist = dev.knn_between(q16, 10, (lo, hi), return_distances=True)
            w_ids, w_dist = knn_between_reference(oracle, q16, ivf.data, 10, (lo, hi), values, stored=stored)
            np.testing.assert_array_equal(ids, w_ids)
            assert _dist_bits(dist, w_dist)
            assert dev.group_rows()["built"] and dev.value_rows()["built"]
            for i in (0, 1):
                _replay(g, calls, i, "an100 after the tables were made")
            g = None
        finally:
            g = None
            _restore(dev)


@pytest.mark.parametrize("seed", (11, 17))
def test_held_call_flushed_by_an_entry_point_without_a_stream(tk, oracle, seed):
    """A call still owed keeps the capture state of the stream it was issued on: the first call of a coalesced pair is
    only held, set_coalesce — which takes no stream — launches it, and join on the capturing stream closes the graph.
    Launched as outside a capture, the held batch would query events and allocate its descriptor pool inside one.
    (Seeds whose index the plain scan finds units on: the verdict event and the pool are on that path.)"""
    from tinyknn_amd import _lib
    case = _restricted_case(seed)
    s0, s1 = _pair_sets(case)
    with _case_opener(case)() as (dev, aset):
        g = None
        try:
            dev.set_pipeline(2)
            dev.set_coalesce(2)
            calls = [Call([s0, s1], case.shape["k"], case.shape["n_probes"], allowed=aset)]
            held = []

            def flush():
                held.append(int(_lib.lib().tk_index_pending(dev._h)))
                dev.set_coalesce(2)

            g = _capture(dev, calls, f"{case} held", flush=flush)
            assert held == [1, 1], held         # (warm-up and capture: the call was held when set_coalesce came)
            for i in (0, 1):
                _replay(g, calls, i, f"{case} held")
            g = None
        finally:
            g = None
            _restore(dev)


# ---- leg 6: tk_index_reserve -----------------------------------------------------------------------------------------

def _reserve_inputs(tk, oracle, restricted):
    from test_hip_parity import ivf_from_fixture
    fx = golden("g6_ivf_an100.npz")
    ivf = ivf_from_fixture(tk, fx)
    N, n = len(ivf.data), len(fx["qn"])
    groups = (np.arange(N) % 3).astype(np.int32)
    base = dict(qn=np.ascontiguousarray(fx["qn"]), qp=np.ascontiguousarray(fx["qpq"]), want=fx["ids_p5"])
    if restricted:
        ox = oracle_index(oracle, ivf, ivf.data)
        base["exclude"] = np.ascontiguousarray(fx["ids_p5"][:, 0], dtype=np.int64)
        base["group"] = np.where(np.arange(n) % 4 == 3, -1, np.arange(n) % 3).astype(np.int32)
        base["want"] = grouped_batch(oracle, ox, base["qn"], base["group"], groups, 10, 5, exclude=base["exclude"])
        base["want_dist"] = exact_distances(oracle, base["qn"], ivf.data, base["want"])
    take = lambda idx: {a: np.ascontiguousarray(v[idx]) for a, v in base.items()}      # noqa: E731
    # 200 queries: the fixture's over and over, in order and in reverse order; the warm-up: its first three
    return ivf, groups, take(np.arange(3)), [take(np.arange(200) % n), take((n - 1 - np.arange(200)) % n)]


@pytest.mark.parametrize("restricted", (False, True), ids=("unrestricted", "exclude+group+distances"))
def test_reserve_then_capture_a_larger_call(tk, oracle, restricted):
    """include/tinyknn_hip.h: after tk_index_reserve a tk_index_query_batch_dev "never allocates, e.g. under stream
    capture".  Three queries warm the index up (streams, events, the restriction's tables), reserve sizes the workspace
    for 200, and the 200-query call is captured without ever having run."""
    import torch
    ivf, groups, small, sets = _reserve_inputs(tk, oracle, restricted)
    dist = torch.float32 if restricted else None
    with _opened(ivf, groups=groups if restricted else None) as (dev, _):
        g = None
        try:
            warm = Call([small], 10, 5, dist=dist)
            st = torch.cuda.current_stream().cuda_stream
            warm.enqueue(dev, st)
            dev.join(st)
            torch.cuda.synchronize()
            warm.check(0, "warm-up with 3 queries")
            dev.reserve(200, 10, 5)
            calls = [Call(sets, 10, 5, dist=dist)]
            g = _capture(dev, calls, "200 queries behind reserve", warm_up=False)
            for i in (0, 1):
                _replay(g, calls, i, "200 queries behind reserve")
            g = None
        finally:
            g = None
            _restore(dev)
