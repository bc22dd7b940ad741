"""The handout of the persistent scan kernels (tickets.h) on the GPU: the plain scan's waves start at the work counter
of the XCD they run on and take EVERY unit, their first included, from the counters; the exact launch keeps a static
first block per wave.  Wherever the workgroups land, every unit must be scored exactly once — a unit handed out twice
is harmless (same bytes), a unit left out leaves stale distances behind and changes heaps.  Plain pinned on
(tk_index_set_plain_scan 2), list-major; probes, heap arrays (layout included) and ids equal to the CPU oracle's, row
for row, at the shapes where a handout can go wrong:

  (i)   fewer units than counters (most ranges empty, every wave walks all eight);
  (ii)  more units than counters, fewer than waves (most waves find nothing);
  (iii) more units than the pipelined launch has waves (1 024): every range is drawn from to its end and waves move
        on to the neighbours' ranges; through the host call (512 workgroups) and through pipelined pairs of calls (256);
  (iv)  lists of very unequal length, longest first: the first ranges hold the units of 12 chunk pairs, the last ones
        units of one — the waves of most XCDs run dry early and finish the others' ranges;
  (v)   the exact launch's pool of three jobs with jobs absent: no list job (first step of a pipeline), no coarse job
        (its last step; batches under 16 queries), no head job (plain off), and n_probes = 1.

The indexes are made by hand (pq_shapes.py's codebook recipe, no k-means) over clusters so far apart that every list
is exactly one cluster: d = 16, M = 8 blocks, the guarded 8-pair form of the plain kernel."""
import numpy as np
import pytest

from pq_shapes import oracle_answers, oracle_index

pytestmark = pytest.mark.gpu

K = 10


def _index(sizes, nq, seed, d=16):
    """-> (ivf, qs): list i holds exactly sizes[i] rows (cluster i; the coarse centre is its first row)."""
    from tinyknn_amd import IVF, FastPQ
    from tinyknn_amd.fast_pq import dpad
    from tinyknn_amd.utils import pad2
    rng = np.random.RandomState(seed)
    sizes = np.asarray(sizes)
    L = len(sizes)
    cent = 6.0 * rng.randn(L, d)
    owner = np.repeat(np.arange(L), sizes)
    X = (cent[owner] + 0.5 * rng.randn(len(owner), d)).astype(np.float32)
    qs = (cent[rng.randint(L, size=nq)] + 0.5 * rng.randn(nq, d)).astype(np.float32)
    pq = FastPQ(2, rotate_dim=None)
    ivf = IVF("euclidean", L, pq)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    ivf.all_centers = np.ascontiguousarray(X[first])
    P = pad2(X, 16, dpad * 2)
    blocks = P.shape[1] // 2
    pick = rng.randint(len(X), size=(blocks, 16))
    books = P.reshape(len(P), blocks, 2)[pick, np.arange(blocks)[:, None]] + 0.01 * rng.randn(blocks, 16, 2)
    pq.centers = np.array(list(books), dtype=np.float32).transpose(1, 0, 2).reshape(16, 2 * blocks)
    pq.sqrt_n_blocks = np.sqrt(blocks)
    ivf.build(X, n_probes=1, device=False)
    assert len(ivf.active_centers) == L and blocks == 8
    assert [len(ivf.ids[i]) for i in range(L)] == list(sizes)
    return ivf, qs


class _Case:
    """one index on the device, its oracle, its queries, and the oracle's answers per setting (computed once)"""

    def __init__(self, oracle, sizes, nq, seed):
        self.ivf, qs = _index(sizes, nq, seed)
        self.sizes = np.asarray(sizes)
        self.qn, self.qp = self.ivf._prepare(qs.copy())
        self.qp = np.ascontiguousarray(self.qp)
        self.ox = oracle_index(oracle, self.ivf)
        self.dev = self.ivf.device_index()
        self.dev.set_scan_mode(2)
        self.dev.set_plain_scan("always")
        self._want = {}

    def want(self, n_probes, pass_1):
        key = (n_probes, pass_1)
        if key not in self._want:
            self._want[key] = oracle_answers(self.ox, self.qn, K, n_probes, pass_1)
        return self._want[key]

    def host(self, n_probes, pass_1=None):
        """one host call (the stages back to back, 512 plain workgroups) -> the plain kernel's tiles of 32 pairs"""
        out, dbg = self.dev.query_batch(self.qn, self.qp, K, n_probes, pass_1=pass_1, debug=True)
        stats = self.dev.plain_stats()
        want = self.want(n_probes, pass_1)
        np.testing.assert_array_equal(dbg["probes"], want["probes"])
        np.testing.assert_array_equal(dbg["heap_val"], want["heap_val"])
        np.testing.assert_array_equal(dbg["heap_idx"], want["heap_idx"])
        np.testing.assert_array_equal(out, want["ids"])
        self.stats = stats
        return stats["plain_units"]

    def units_at_least(self):
        """A lower bound on the units of the last host call: a unit is a tile times a range of at most K chunk pairs,
        and K is 12 for batches of this size (api_index.hip: plain_k), so the chunk pairs of all units / 12."""
        return -(-self.stats["plain_unit_chunk_pairs"] // 12)

    def pipelined(self, n_probes, pass_1=None, calls=5, coalesce=2):
        """`calls` device calls in flight, in pairs (256 plain workgroups per launch); the first step's exact launch
        has no list job, the last one's no coarse job"""
        import torch
        nq = len(self.qn)
        self.dev.set_pipeline(2)
        self.dev.set_coalesce(coalesce)
        try:
            q_dev, qp_dev = torch.from_numpy(self.qn).cuda(), torch.from_numpy(self.qp).cuda()
            st = torch.cuda.current_stream().cuda_stream
            outs = [torch.full((nq, K), -1, dtype=torch.int64, device="cuda") for _ in range(calls)]
            for o in outs:
                self.dev.query_batch_dev(q_dev.data_ptr(), qp_dev.data_ptr(), self.qp.dtype == np.float64, nq, K,
                                         n_probes, o.data_ptr(), pass_1=pass_1, stream=st)
            self.dev.join(st)
            torch.cuda.synchronize()
            want = self.want(n_probes, pass_1)["ids"]
            for i, o in enumerate(outs):
                np.testing.assert_array_equal(o.cpu().numpy(), want, err_msg=f"call {i}")
        finally:
            self.dev.set_coalesce(1)
            self.dev.set_pipeline(1)


@pytest.fixture(scope="module")
def tiny(oracle):
    return _Case(oracle, [40, 40, 40], 5, seed=1)


@pytest.fixture(scope="module")
def small(oracle):
    return _Case(oracle, [100] * 20, 200, seed=2)


@pytest.fixture(scope="module")
def wide(oracle):
    return _Case(oracle, [800 - 7 * (i % 5) for i in range(100)], 4000, seed=3)


@pytest.fixture(scope="module")
def uneven(oracle):
    return _Case(oracle, [max(1, int(6000 * 0.8 ** i)) for i in range(40)], 4000, seed=4)


# ---- (i) fewer units than counters ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_probes", [1, 2, 3])
@pytest.mark.parametrize("pass_1", [None, 3])
def test_fewer_units_than_counters(tiny, n_probes, pass_1):
    tiles = tiny.host(n_probes, pass_1)
    # one probed list: no plain job at all (the exact launch alone).  Heaps of 3: every slot is plain (the first list
    # in head mode); lists of 3 chunks and 5 queries: a unit per probed list
    if n_probes == 1:
        assert tiles == 0
    else:
        # (a list is 2 chunk pairs: a tile is one unit)
        assert tiles < 8 and (pass_1 is None or 1 <= tiles <= 3), tiles
    tiny.pipelined(n_probes, pass_1)


# ---- (ii) fewer units than waves --------------------------------------------------------------------------------------

@pytest.mark.parametrize("pass_1", [None, 3])
def test_fewer_units_than_waves(small, pass_1):
    tiles = small.host(4, pass_1)
    # (a list is 4 chunk pairs: a tile is one unit)
    assert tiles < 1024 and (pass_1 is None or tiles > 8), tiles
    small.pipelined(4, pass_1)


# ---- (iii) more units than waves --------------------------------------------------------------------------------------

@pytest.mark.parametrize("pass_1", [None, 17])
def test_more_units_than_waves(wide, pass_1):
    wide.host(5, pass_1)
    # 100 lists x 25 chunk pairs in ranges of 12 x tiles of 32 of the ~200 pairs a list gets
    assert pass_1 is None or wide.units_at_least() > 1024, wide.stats
    wide.pipelined(5, pass_1)


def test_more_units_than_waves_one_call_per_batch(wide):
    wide.pipelined(5, 17, calls=3, coalesce=1)


# ---- (iv) ranges of very unequal cost ---------------------------------------------------------------------------------

@pytest.mark.parametrize("pass_1", [None, 17])
def test_lists_of_very_unequal_length(uneven, pass_1):
    assert uneven.sizes[0] == 6000 and uneven.sizes[-1] == 1
    uneven.host(6, pass_1)
    assert pass_1 is None or uneven.units_at_least() > 1024, uneven.stats
    uneven.pipelined(6, pass_1)


# ---- (v) the exact launch's pool with jobs absent ---------------------------------------------------------------------

def test_exact_launch_with_jobs_absent(tiny, small):
    # under 16 queries the coarse scan is not a job of the pool (tiny: 5 queries); n_probes = 1: one slot per query,
    # no plain job and no head job
    for case in (tiny, small):
        assert case.host(1) == 0
        case.pipelined(1, calls=1)              # one batch: a step without a list job, then one without a coarse job
        case.pipelined(1, calls=4)
    # plain off: no plain launch and no head job beside the list job
    for case, n_probes in ((tiny, 2), (small, 1), (small, 4)):
        case.dev.set_plain_scan(False)
        try:
            assert case.host(n_probes) == 0
            case.pipelined(n_probes, calls=3)
        finally:
            case.dev.set_plain_scan("always")
