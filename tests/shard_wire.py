"""Lock-step harness for the list-sharded wire protocol (no tests in here; tests/test_shard_wire_gpu.py and
tests/test_shard_wire_cpu.py use it).

The project states the protocol of include/tinyknn_hip.h ("list-sharded index over `world` ranks") twice: in HIP
(shard.hip, api_shard.hip and the scan kernels behind the tk_index_shard_*_dev entry points: _HipShardEngine) and
in numpy over the oracle (tests/shard_cpu_engine.py: OracleShardEngine).  `run_both` plays W ranks of each on the
same inputs, stage by stage, and returns what every rank of either side wrote — send buffers with their guard,
flags, usage, bound bytes, counts, records, books of the plain scan — as numpy arrays; the `check_*` functions
compare two such results byte for byte and name the first (rank, query, slot, block) that differs.  Either side
may be the oracle engine, so the harness itself runs without a GPU.

Stage order of one side (every stage on buffers of its own, all prefilled with 0xAB):
  one-phase scan -> head scan + one-phase scan behind the reduced head bounds -> two-phase scan (first / rest) ->
  dense scan -> bound -> filter (compact) -> filter (regions: roomy, then one record too small); in the home form
  the coarse call in front of every scan form, as in a batch of its own.  The dense scan comes last among the
  scans so that the engines are left in the state the finish calls of a crossed exchange (`cross_finish*`) expect.
"""
import numpy as np

from shard_cpu_engine import OracleShardEngine
from tinyknn_amd.multi_gpu import shard_capacity, shard_lists, shard_positions

FILL = 0xAB
GUARD = 4096            # bytes behind the last region of every send buffer
ALL_STAGES = ("one", "head", "two", "dense", "bound", "filter", "regions")

# the default legs of tests/test_shard_wire_gpu.py (tests/test_shard_wire_cpu.py shows what they hold)
FIXTURE_TAGS = ("eu20", "an20", "an100", "an100b2", "eu128", "eu20f64")
FIXTURE_LEGS = [(tag, p, w, c) for tag in FIXTURE_TAGS for p in (2, 5) for w in (1, 2, 3) for c in ("home", "replicated")]
# seeds of _case(500 + seed): 0-15, and seven more — of 0-15 only seed 5 has a probe list that wraps (42, 58, 74,
# 78 do) and only seed 8 a rank without a home query (17, 22, 24 do)
FUZZ_SEEDS = list(range(16)) + [17, 22, 24, 42, 58, 74, 78]


# ---------------------------------------------------------------------------------------------------------
# cases

def fixture_case(O, tag, with_ivf=True):
    from conftest import golden
    from test_oracle_golden import load_oracle_index
    g = golden(f"g6_ivf_{tag}.npz")
    ivf = None
    if with_ivf:
        from test_hip_parity import ivf_from_fixture
        ivf = ivf_from_fixture(None, g)
    return dict(name=tag, ivf=ivf, ox=load_oracle_index(O, g), qn=np.ascontiguousarray(g["qn"], dtype=np.float32),
                qp=np.ascontiguousarray(g["qpq"]), k=10, goldens={int(p): g[f"ids_p{int(p)}"] for p in g["probes_list"]})


def fuzz_case(O, seed, nq_cap=65):
    """The index, queries and world of tests/test_fuzz_gpu.py::test_random_index_sharded_both_exchanges[seed]
    (same draws in the same order), the batch cut to nq_cap queries.  None where that test skips."""
    from test_fuzz_gpu import _case
    from test_hip_parity import _oracle_index
    from tinyknn_amd import IVF, FastPQ
    c = _case(500 + seed)
    rng = np.random.RandomState(2000 + seed)
    cent = rng.randn(max(c["n_clusters"], 3), c["d"]) * c["spread"]
    X = (cent[rng.randint(len(cent), size=c["n"])] + 0.5 * rng.randn(c["n"], c["d"])).astype(np.float32)
    qs = (cent[rng.randint(len(cent), size=c["nq"])] + 0.5 * rng.randn(c["nq"], c["d"])).astype(np.float32)
    ivf = IVF(c["metric"], c["n_clusters"], FastPQ(2))
    # (the k-means fits and the rotation draw from numpy's global generator: pinned here, so that a seed names the
    #  same index in every run and order of tests — the categories test_shard_wire_cpu.py counts depend on it)
    state = np.random.get_state()
    np.random.seed(3000 + seed)
    try:
        ivf.fit(X).build(X, n_probes=c["build_probes"])
    except AssertionError:
        return None
    finally:
        np.random.set_state(state)
    if len(ivf.active_centers) != c["n_clusters"]:
        return None
    qn, qp = ivf._prepare(qs.copy())
    world = int(rng.choice([1, 2, 3, 4]))
    qn, qp = np.ascontiguousarray(qn[:nq_cap], dtype=np.float32), np.ascontiguousarray(qp[:nq_cap])
    worst = len(qn) * min(c["n_probes"], c["n_clusters"]) * (c["n"] // 16 + 2)
    return dict(name=f"fuzz{seed}", ivf=ivf, ox=_oracle_index(O, ivf), qn=qn, qp=qp, k=c["k"], n_probes=c["n_probes"],
                world=world, capacity=worst, case=c)


# ---------------------------------------------------------------------------------------------------------
# the model's view of a leg: where every segment lies

class Plan:
    """Probe lists and segment positions of a batch, from the oracle and shard_positions."""

    def __init__(self, O, ox, owner, world, qn, k, n_probes, pass_1, capacity):
        self.eng = OracleShardEngine(O, ox, owner, 0, world)
        self.qn = qn
        self.f = self.eng._front_all(qn, k, n_probes, pass_1)
        self.probes, self.raw = self.f["probes"], self.f["raw"]
        self.world, self.capacity, self.owner = world, int(capacity), owner
        self.nq, self.S = self.probes.shape
        self.qh = -(-self.nq // world)
        self.chunks = self.eng.chunks
        self.src, self.pos = shard_positions(self.probes, self.chunks, owner, world, capacity)
        _, free = shard_positions(self.probes, self.chunks, owner, world, 10 ** 12)
        self.usage = int((free + self.chunks[self.probes]).max()) if self.probes.size else 0

    def segments(self, rank):
        """(query, slot, first byte in the rank's send buffer, bytes) of every fitted segment the rank owns"""
        out = []
        for i in range(self.nq):
            for s in range(self.S):
                if self.src[i, s] == rank and self.pos[i, s] >= 0:
                    n = int(self.chunks[self.probes[i, s]])
                    out.append((i, s, ((i // self.qh) * self.capacity + int(self.pos[i, s])) * 16, n * 16))
        return out

    def mask(self, rank):
        """bytes of the rank's send buffer (guard included) that belong to one of its segments"""
        m = np.zeros(self.world * self.capacity * 16 + GUARD, dtype=bool)
        for _, _, a, n in self.segments(rank):
            m[a:a + n] = True
        return m


def leg_facts(plan, k, n_probes, pass_1):
    """What a leg holds of the categories the comparisons are meant to meet, from the oracle alone."""
    eng, f = plan.eng, plan.f
    import torch
    one = OracleShardEngine(eng.O, eng.ox, np.zeros_like(plan.owner), 0, 1)       # owns every first list: B1 of all
    b1 = torch.zeros(plan.nq, dtype=torch.uint8)
    one.bound(0, torch.from_numpy(plan.qn), k, n_probes, pass_1, plan.capacity, None, b1)
    pq = eng.plain_queries(f["raw"], f["tables_raw"], b1.numpy(), plan.capacity)
    above = 0
    for i in np.flatnonzero(pq):
        for s in range(1, plan.S):
            above += int((eng.plain_sums(plan.probes[i, s], f["tables_raw"][i]) > 127).sum())
    segs = [sum(1 for x in plan.segments(r) if x[3] > 0) for r in range(plan.world)]
    owns = [bool(((plan.src == r) & (plan.chunks[plan.probes] > 0)).any()) for r in range(plan.world)]
    return dict(plain=pq, mixed=plan.S >= 2 and bool(pq.any()) and not bool(pq.all()),
                wrapped=bool((f["raw"] < 0).any()), short=bool((eng.ox.list_n < 16).any()),
                repeated=not eng.ids_unique, no_home=plan.nq <= (plan.world - 1) * plan.qh,
                rows_above_127=above, segments=segs, owns=owns)


# ---------------------------------------------------------------------------------------------------------
# one side, stage by stage

def make_engines(kind, ivf, O, ox, owner, world):
    """kind "oracle": W OracleShardEngines; "hip": ONE uploaded index and a clone shard of it per rank
    (DeviceIndex.clone_shard).  -> (engines, what to keep alive beside them)"""
    if kind == "oracle":
        return [OracleShardEngine(O, ox, owner, r, world) for r in range(world)], None
    from tinyknn_amd.multi_gpu import _HipShardEngine
    base = ivf.device_index()
    return [_HipShardEngine(ivf, owner, r, world, 1, dev=base.clone_shard(owner, r, world)) for r in range(world)], base


def close_engines(engines):
    for e in engines:
        if e.device != "cpu":
            e.dev.close()


class Side:
    """The engines of one side, the batch on their device, and what the stages wrote (numpy, per rank)."""

    def __init__(self, engines, qn, qp, k, n_probes, pass_1, capacity, n_lists):
        import torch
        self.torch = torch
        self.engines, self.dev = engines, engines[0].device
        self.oracle = self.dev == "cpu"
        self.W, self.nq = len(engines), len(qn)
        self.qh = -(-self.nq // self.W)
        self.k, self.n_probes, self.pass_1, self.capacity = k, n_probes, pass_1, int(capacity)
        self.kc = min(n_probes, n_lists)
        self.qn = torch.from_numpy(np.ascontiguousarray(qn, dtype=np.float32)).to(self.dev)
        self.qp = torch.from_numpy(np.ascontiguousarray(qp)).to(self.dev)
        self.p_all = None
        self.out = {}
        self.plain_kw = dict(plain=True) if self.oracle else {}

    # buffers: every byte 0xAB before a stage writes
    def fill(self, nbytes, dtype=None):
        t = self.torch.full((int(nbytes),), FILL, dtype=self.torch.uint8, device=self.dev)
        return t if dtype is None else t.view(dtype)

    def send_buffers(self):
        full = [self.fill(self.W * self.capacity * 16 + GUARD) for _ in self.engines]
        return full, [f[:self.W * self.capacity * 16].view(self.W, self.capacity * 16) for f in full]

    def flags(self):
        return [self.torch.zeros(1, dtype=self.torch.int32, device=self.dev) for _ in self.engines]

    def to(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    @staticmethod
    def np_(ts):
        return [t.cpu().numpy().copy() for t in ts]

    def args(self):
        return self.k, self.n_probes, self.pass_1

    def coarse(self):
        homes = [self.fill(self.qh * self.kc * 8, self.torch.int64) for _ in self.engines]
        for e, h in zip(self.engines, homes):
            e.coarse(0, self.qn, self.qp, *self.args(), h)
        self.out["probes_home"] = [h.reshape(self.qh, self.kc) for h in self.np_(homes)]
        self.p_all = self.torch.cat(homes).contiguous()                             # all-gather

    def scan_dense(self, key="dense"):
        full, send = self.send_buffers()
        fl = self.flags()
        for e, s, f in zip(self.engines, send, fl):
            e.scan(0, self.qn, self.qp, *self.args(), self.capacity, s, f, probes_all=self.p_all)
        self._sync()
        self.out[key] = dict(send=self.np_(full), flag=[int(f.item()) for f in fl],
                             usage=[int(e.usage(0)) for e in self.engines])
        self._scan = send

    def bound(self):
        b = [self.fill(self.nq) for _ in self.engines]
        for e, s, x in zip(self.engines, self._scan, b):
            e.bound(0, self.qn, *self.args(), self.capacity, s.reshape(-1), x)
        self._bmin = self.torch.stack(b).min(dim=0).values.contiguous()            # all-reduce(MIN)
        self.out["bound"] = dict(bound=self.np_(b), reduced=self._bmin.cpu().numpy().copy())

    def filter(self):
        W = self.W
        cnt = [self.fill(3 * W * 4, self.torch.int32) for _ in self.engines]
        rec = [self.fill(W * self.capacity * 20, self.torch.int32).view(W * self.capacity, 5) for _ in self.engines]
        for e, s, c, r in zip(self.engines, self._scan, cnt, rec):
            e.filter(0, self.qn, *self.args(), self.capacity, s.reshape(-1), self._bmin, c, r)
        self._sync()
        self.out["filter"] = dict(counts=self.np_(cnt), records=self.np_(rec))

    def regions(self):
        """The record-region form twice: regions as large as `capacity` (can never overflow), then one record
        smaller than the largest count (where that is above 1)."""
        W = self.W
        need = max(int(c[:W].max()) for c in self.out["filter"]["counts"])
        for key, region in (("regions", self.capacity), ("regions_tight", need - 1)):
            if region < 1:
                continue
            cnt = [self.fill(3 * W * 4, self.torch.int32) for _ in self.engines]
            rec = [self.fill(W * region * 20, self.torch.int32).view(W * region, 5) for _ in self.engines]
            fl = self.flags()
            for e, s, c, r, f in zip(self.engines, self._scan, cnt, rec, fl):
                e.filter_regions(0, self.qn, *self.args(), self.capacity, s.reshape(-1), self._bmin, c, r, region, f)
            self._sync()
            self.out[key] = dict(counts=self.np_(cnt), records=self.np_(rec), flag=[int(f.item()) for f in fl],
                                 region=region)

    def two_phase(self):
        full, send = self.send_buffers()
        fl = self.flags()
        first = [self.fill(self.nq) for _ in self.engines]
        for e, s, f, b in zip(self.engines, send, fl, first):
            e.scan_first(0, self.qn, self.qp, *self.args(), self.capacity, s, f, b, probes_all=self.p_all)
        red = self.torch.stack(first).min(dim=0).values.contiguous()
        for e, s in zip(self.engines, send):
            e.scan_rest(0, self.qn, *self.args(), self.capacity, s, red, **self.plain_kw)
        self._sync()
        if self.oracle:
            books = [(e.last_plain_pairs, int(e.last_plain.sum())) for e in self.engines]
        else:
            st = [e.dev.shard_plain_stats(0) for e in self.engines]
            books = [(x["plain_pairs"], x["plain_queries"]) for x in st]
        self.out["two"] = dict(send=self.np_(full), flag=[int(f.item()) for f in fl], first=self.np_(first),
                               reduced=red.cpu().numpy().copy(), books=books)

    def one_phase(self):
        full, send = self.send_buffers()
        fl = self.flags()
        for e, s, f in zip(self.engines, send, fl):
            e.scan_plain(0, self.qn, self.qp, *self.args(), self.capacity, s, f, probes_all=self.p_all, **self.plain_kw)
        self._sync()
        self.out["one"] = dict(send=self.np_(full), flag=[int(f.item()) for f in fl])

    def head(self):
        full, send = self.send_buffers()
        fl = self.flags()
        heads = [self.fill(self.nq) for _ in self.engines]
        for e, s, f, b in zip(self.engines, send, fl, heads):
            e.scan_head(0, self.qn, self.qp, *self.args(), self.capacity, s, f, b, probes_all=self.p_all)
        red = self.torch.stack(heads).min(dim=0).values.contiguous()
        for e, s, f in zip(self.engines, send, fl):
            e.scan_plain(0, self.qn, self.qp, *self.args(), self.capacity, s, f, probes_all=self.p_all, bound=red,
                         **self.plain_kw)
        self._sync()
        self.out["head"] = dict(send=self.np_(full), flag=[int(f.item()) for f in fl], heads=self.np_(heads),
                                reduced=red.cpu().numpy().copy())

    def _sync(self):
        if not self.oracle:
            self.torch.cuda.synchronize()

    def run(self, coarse, stages, two_phase):
        # one batch = coarse -> scan -> ...: the home form's coarse call in front of EVERY scan form (it builds the
        # slot's tables and their limits, and the scan behind the head bounds masks those limits in place)
        for name, scan in (("one", self.one_phase), ("head", self.head), ("two", self.two_phase), ("dense", self.scan_dense)):
            if name in stages and (name != "two" or two_phase):
                if coarse == "home":
                    self.coarse()
                scan()
        if "bound" in stages:
            self.bound()
        if "filter" in stages:
            self.filter()
        if "regions" in stages:
            self.regions()
        return self.out

    # ---- a crossed exchange: the OTHER side's bytes into this side's finish calls (after a dense scan here)
    def cross_finish(self, sends, plain=None):
        """sends: per source rank the (guarded) send buffer of the other side.  The all-to-all by hand, then
        finish on every home rank -> ids (nq, k).  plain: for the oracle engine's finish."""
        W, cap = self.W, self.capacity
        regions = [np.asarray(s)[:W * cap * 16].reshape(W, cap * 16) for s in sends]
        homes = []
        for h, e in enumerate(self.engines):
            recv = self.to(np.stack([regions[s][h] for s in range(W)]))
            out = self.torch.zeros(self.qh * self.k, dtype=self.torch.int64, device=self.dev)
            kw = dict(plain=plain) if self.oracle else {}
            e.finish(0, self.qn, *self.args(), cap, recv, out, **kw)
            homes.append(out.view(self.qh, self.k))
        self._sync()
        return self.torch.cat(homes).cpu().numpy()[:self.nq]

    def cross_finish_filtered(self, counts, records, reverse=False):
        """counts / records of the other side's compact filter; reverse: the records of every source in
        reversed order (the order inside a group is nobody's contract)."""
        W = self.W
        homes = []
        for h, e in enumerate(self.engines):
            parts = []
            for s in range(W):
                o = int(counts[s][:h].sum())
                part = records[s][o:o + int(counts[s][h])]
                parts.append(part[::-1] if reverse else part)
            rrec = self.to(np.concatenate(parts).astype(np.int32).reshape(-1, 5))
            out = self.torch.zeros(self.qh * self.k, dtype=self.torch.int64, device=self.dev)
            fl = self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)
            e.finish_filtered(0, self.qn, *self.args(), rrec, rrec.shape[0], out, fl)
            self._sync()
            assert int(fl.item()) == 0, f"home rank {h} refused a record (flag {int(fl.item())})"
            homes.append(out.view(self.qh, self.k))
        return self.torch.cat(homes).cpu().numpy()[:self.nq]


def run_both(ivf, ox, world, qn, qp, k, n_probes, O=None, pass_1=None, coarse="home", capacity=None,
             stages=ALL_STAGES, sides=("hip", "oracle"), owner=None):
    """-> (plan, side_a, side_b): both sides' raw outputs per rank in side.out (see Side), the engines left
    alive for a crossed exchange (close_engines(side.engines) when done)."""
    if O is None:
        from oracle import oracle as O
    sizes = np.asarray(ox.list_n, dtype=np.int64)
    if owner is None:
        owner = shard_lists(sizes, world)
    if capacity is None:
        capacity = shard_capacity(sizes, owner, world, len(qn), n_probes)
    plan = Plan(O, ox, owner, world, qn, k, n_probes, pass_1, capacity)
    made = []
    for kind in sides:
        engines, keep = make_engines(kind, ivf, O, ox, owner, world)
        s = Side(engines, qn, qp, k, n_probes, pass_1, capacity, ox.n_lists)
        s.keep = keep
        made.append(s)
    two_phase = all(s.engines[0].plain_ok(k, n_probes, pass_1) for s in made)
    plan.two_phase = two_phase
    for s in made:
        s.run(coarse, stages, two_phase)
    return plan, made[0], made[1]


# ---------------------------------------------------------------------------------------------------------
# comparisons: exact equality, the first difference named

def _first_wrong(plan, rank, a, b):
    for i, s, at, n in plan.segments(rank):
        if not np.array_equal(a[at:at + n], b[at:at + n]):
            blk = int(np.flatnonzero((a[at:at + n] != b[at:at + n]).reshape(-1, 16).any(axis=1))[0])
            return (f"rank {rank} -> home {i // plan.qh}: query {i} slot {s} (list {plan.probes[i, s]}) block {blk}: "
                    f"{a[at + 16 * blk:at + 16 * blk + 16].view(np.int8)} != {b[at + 16 * blk:at + 16 * blk + 16].view(np.int8)}")
    return "no segment differs"


def check_probes_home(a, b):
    for r, (x, y) in enumerate(zip(a["probes_home"], b["probes_home"])):
        np.testing.assert_array_equal(x, y, err_msg=f"probes_home of rank {r}")


def check_send(plan, a, b, what="dense", content=True):
    """Every fitted segment a rank owns: the same bytes on both sides (content=False: not compared — the
    one-phase forms, whose contract is per block, see OracleShardEngine.finish(plain="blocks")); flag bit 1
    alike; where no rank overflowed every byte outside the segments still 0xAB; the guard always."""
    A, B = a[what], b[what]
    end = plan.world * plan.capacity * 16
    overflowed = any(f & 1 for f in A["flag"] + B["flag"])
    for r in range(plan.world):
        assert (A["flag"][r] & 1) == (B["flag"][r] & 1), f"{what}: overflow flag of rank {r}: {A['flag'][r]} / {B['flag'][r]}"
        m = plan.mask(r)
        x, y = A["send"][r], B["send"][r]
        assert x.shape == y.shape == m.shape
        if content and not np.array_equal(x[m], y[m]):
            raise AssertionError(f"{what}: " + _first_wrong(plan, r, x, y))
        for side, z in (("a", x), ("b", y)):
            assert (z[end:] == FILL).all(), f"{what}: side {side} rank {r} wrote behind its last region"
            if not overflowed:
                stray = np.flatnonzero(~m & (z != FILL))
                assert stray.size == 0, (f"{what}: side {side} rank {r} wrote outside its segments: byte {int(stray[0])} "
                                         f"(region {int(stray[0]) // (plan.capacity * 16)}, block {int(stray[0]) % (plan.capacity * 16) // 16})")
    if "usage" in A:
        assert A["usage"] == B["usage"], f"{what}: usage {A['usage']} / {B['usage']}"
    return overflowed


def check_bytes(a, b, key, field, what):
    """(nq,) bytes per rank (255 where the rank has no say) and their MIN over the ranks"""
    for r, (x, y) in enumerate(zip(a[key][field], b[key][field])):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} of rank {r}")
    np.testing.assert_array_equal(a[key]["reduced"], b[key]["reduced"], err_msg=f"{what}, min-reduced")


def _groups(counts, records, W, region=None):
    """records of one rank by home group, each sorted by its key (rec[0]: unique)"""
    out, o = [], 0
    for h in range(W):
        n = int(counts[h])
        g = records[h * region: h * region + min(n, region)] if region else records[o:o + n]
        o += n
        out.append(g[np.argsort(g[:, 0], kind="stable")] if len(g) else g)
    return out


def check_filter(plan, a, b, key="filter"):
    """counts[:W] and counts[2W:] alike; every home group the same SET of records (device order is whatever
    the atomics gave).  Region form: the same per region where nothing overflowed, else both flag."""
    W = plan.world
    A, B = a[key], b[key]
    region = A.get("region")
    for r in range(W):
        ca, cb = A["counts"][r], B["counts"][r]
        np.testing.assert_array_equal(ca[:W], cb[:W], err_msg=f"{key}: records per home of rank {r}")
        np.testing.assert_array_equal(ca[2 * W:], cb[2 * W:], err_msg=f"{key}: blocks scored per home of rank {r}")
        if region:
            over = bool((ca[:W] > region).any())
            assert bool(A["flag"][r] & 1) == over and bool(B["flag"][r] & 1) == over, \
                f"{key}: region {region}, counts {ca[:W]}: flags {A['flag'][r]} / {B['flag'][r]}"
            if over:
                continue
        for h, (x, y) in enumerate(zip(_groups(ca, A["records"][r], W, region), _groups(cb, B["records"][r], W, region))):
            assert len(np.unique(x[:, 0])) == len(x), f"{key}: rank {r} home {h}: a key twice on side a"
            if not np.array_equal(x, y):
                ka, kb = set(x[:, 0].tolist()), set(y[:, 0].tolist())
                raise AssertionError(f"{key}: rank {r} -> home {h}: keys only on side a {sorted(ka - kb)[:4]}, only on "
                                     f"side b {sorted(kb - ka)[:4]}, {int((x != y).any(axis=1).sum()) if x.shape == y.shape else '?'} "
                                     f"records differ")


def check_books(a, b):
    assert a["two"]["books"] == b["two"]["books"], \
        f"plain (pairs, queries) per rank: {a['two']['books']} / {b['two']['books']}"


def check_all(plan, a, b, coarse="home", one_phase_content=False):
    """Every stage both sides ran.  one_phase_content: the one-phase send buffers byte for byte too (two model
    engines make the same choice per block; the device's documented fallbacks leave it per block)."""
    if coarse == "home":
        check_probes_home(a, b)
    for what in ("dense", "two", "one", "head"):
        if what in a:
            assert what in b
            check_send(plan, a, b, what, content=one_phase_content or what in ("dense", "two"))
    if "bound" in a:
        check_bytes(a, b, "bound", "bound", "bound after the first list")
    if "two" in a:
        check_bytes(a, b, "two", "first", "bound after the first list (scan_first)")
        check_books(a, b)
    plan.fell_back = False
    if "head" in a:
        unsaid = all((h == 255).all() for h in a["head"]["heads"]) and not all((h == 255).all() for h in b["head"]["heads"])
        if unsaid and not one_phase_content:
            # side a answered 255 for every query: where the one-phase form does not apply, tk_index_shard_scan_head_dev
            # IS tk_index_shard_scan_dev (and the plain call behind it does nothing) — then every byte is the dense scan's
            plan.fell_back = True
            for what in ("head", "one"):
                for r in range(plan.world):
                    np.testing.assert_array_equal(a[what]["send"][r], a["dense"]["send"][r],
                                                  err_msg=f"{what}: rank {r} fell back to the exact scan, but not whole")
        else:
            check_bytes(a, b, "head", "heads", "bound after the head")
    for key in ("filter", "regions", "regions_tight"):
        if key in a:
            assert key in b
            check_filter(plan, a, b, key)
