"""Which entry point of the library a DeviceIndex call reaches, and with what: the library is replaced by a recorder
(no GPU, no .so), so the Python layer's choices are visible — the foreign function, its scalars, the dtype and shape
of every buffer, the life of a temporary allowed set, the fill of what is returned.  Also: the three ways a
DeviceIndex is made give objects with the same attributes, and query_batch_dev (inside the benchmark's timed loop)
makes no more Python-level calls than it did."""
import ctypes as C
import itertools
import sys
import types
import weakref

import numpy as np
import pytest

from tinyknn_amd import _front, _lib
from tinyknn_amd import ivf as ivf_mod
from tinyknn_amd.ivf import AllowSet, DeviceIndex

N, D, DQ, DPB, L = 40, 6, 8, 2, 3
NQ, K, NP = 5, 3, 2
HANDLE = 0xABC0
SUB = 2             # the recorder's tk_index_max_sub_batch


class Recorder:
    """Stands where the loaded library stands: every attribute is a function that records (name, args), returns 0
    (a fresh non-zero handle from the creating calls) and fills in the few outputs the Python layer reads back."""

    def __init__(self):
        self.calls = []
        self.handles = itertools.count(0x5000, 0x10)

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            if name == "tk_index_info":
                args[1][6] = N
            if name == "tk_allow_create":
                args[3]._obj.value = next(self.handles)
            if name == "tk_index_max_sub_batch":
                return SUB
            if name in ("tk_index_create", "tk_index_alloc_data", "tk_index_clone_shard", "tk_stream_create"):
                return next(self.handles)
            if name == "tk_last_error":
                return b""
            return 0
        return f

    def named(self, *names):
        return [c for c in self.calls if c[0] in names]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: r)
    monkeypatch.setattr(_lib, "owns_handles", lambda: True)
    monkeypatch.setattr(_front, "bind", lambda: False)
    yield r
    # what was made on the recorder's handles must never reach the real library (a late __del__): forget the handles
    for dev in MADE:
        for a in list(getattr(dev, "_live_allows", ())):
            a._h = None
        for st in list(dev._live_streams):
            st._s = None
        dev._h = None
    del MADE[:]


MADE = []       # every DeviceIndex a test of this file made


def made(dev):
    MADE.append(dev)
    return dev


def bare_index(f64=False):
    dev = DeviceIndex.__new__(DeviceIndex)
    dev._h, dev.d, dev.dq, dev.dpb, dev.n_lists, dev.N = HANDLE, D, DQ, DPB, L, N
    dev.angular, dev._R, dev._f64, dev.rank, dev.world = False, None, f64, 0, 1
    dev._streams, dev._live_streams, dev._live_allows = {}, weakref.WeakSet(), weakref.WeakSet()
    return made(dev)


def addr(x):
    """the address a foreign argument carries: None, an integer, a c_void_p or a typed pointer of _lib.ptr"""
    if x is None or isinstance(x, int):
        return x
    return C.cast(x, C.c_void_p).value


def is_buffer(p, a, dtype, shape):
    """p points at the first element of `a`, which has this dtype and shape and is C-contiguous"""
    assert addr(p) == a.ctypes.data
    assert a.dtype == dtype and a.shape == shape and a.flags.c_contiguous
    return True


def queries(q64):
    rng = np.random.RandomState(3)
    qn = np.ascontiguousarray(rng.randn(NQ, D), dtype=np.float32)
    q_pq = np.ascontiguousarray(rng.randn(NQ, DQ), dtype=np.float64 if q64 else np.float32)
    return qn, q_pq


def allowed_arg(dev, kind):
    if kind == "none":
        return None
    mask = np.zeros(N, dtype=bool)
    mask[::3] = True
    return dev.allow(mask) if kind == "set" else mask


@pytest.mark.parametrize("q64", [False, True])
@pytest.mark.parametrize("return_distances", [False, True])
@pytest.mark.parametrize("kind", ["none", "set", "mask"])
@pytest.mark.parametrize("debug", [False, True])
@pytest.mark.parametrize("pass_1", [None, 7])
def test_query_batch_reaches_one_entry_point(rec, debug, kind, return_distances, q64, pass_1):
    dev = bare_index(f64=q64)
    qn, q_pq = queries(q64)
    allowed = allowed_arg(dev, kind)
    made_before = len(rec.named("tk_allow_create"))
    rec.calls.clear()
    if debug and return_distances:
        with pytest.raises(ValueError, match="debug=True cannot be combined with return_distances=True"):
            dev.query_batch(qn, q_pq, K, NP, pass_1, debug, allowed=allowed, return_distances=True)
        assert rec.calls == []
        return
    got = dev.query_batch(qn, q_pq, K, NP, pass_1, debug, allowed=allowed, return_distances=return_distances)

    # ---- what comes back
    R = pass_1 if pass_1 else (NP + 1) * K + 1
    dbg = dist = None
    if return_distances:
        out, dist = got
        assert dist.dtype == (np.float64 if q64 else np.float32) and dist.shape == (NQ, K) and np.isposinf(dist).all()
    elif debug:
        out, dbg = got
        assert sorted(dbg) == ["heap_idx", "heap_val", "probes"]
        assert dbg["probes"].dtype == np.int64 and dbg["probes"].shape == (NQ, min(NP, L))
        assert dbg["heap_idx"].dtype == np.int64 and dbg["heap_idx"].shape == (NQ, R)
        assert dbg["heap_val"].dtype == np.int32 and dbg["heap_val"].shape == (NQ, R)
    else:
        out = got
    assert out.dtype == np.int64 and out.shape == (NQ, K) and (out == -1).all()

    # ---- the allowed set: a prepared one is used and left open, a mask becomes a set that is closed again
    created = rec.named("tk_allow_create")
    destroyed = [a[0] for _, a in rec.named("tk_allow_destroy")]
    if kind == "set":
        assert made_before == 1 and created == [] and destroyed == []
        aset = allowed.handle
    elif kind == "mask":
        assert len(created) == 1
        h, mask_p, n, _ = created[0][1]
        assert h == HANDLE and n == N
        assert mask_p._arr.dtype == np.uint8 and mask_p._arr.shape == (N,)
        assert np.array_equal(mask_p._arr, allowed.astype(np.uint8))
        aset = created[0][1][3]._obj.value
        assert destroyed == [aset]
        assert rec.calls[-1][0] == "tk_allow_destroy"        # ... after the query ran
    else:
        assert created == [] and destroyed == []
        aset = None

    # ---- the entry point and its arguments
    entry = [c for c in rec.calls if c[0].startswith("tk_index_query_batch")]
    scalars = (int(q64), K, NP, pass_1 or 0)
    if return_distances:
        assert [c[0] for c in entry] == ["tk_index_query_batch_dist"]
        h, a, qn_p, qpq_p, is64, nq, k, n_probes, p1, out_p, dist_p = entry[0][1]
        assert (h, a, nq) == (HANDLE, aset, NQ) and (is64, k, n_probes, p1) == scalars
        assert is_buffer(qn_p, qn, np.float32, (NQ, D)) and is_buffer(qpq_p, q_pq, q_pq.dtype, (NQ, DQ))
        assert is_buffer(out_p, out, np.int64, (NQ, K)) and is_buffer(dist_p, dist, dist.dtype, (NQ, K))
        return
    if kind == "none":
        assert [c[0] for c in entry] == ["tk_index_query_batch"]
        spans = [(0, NQ)]
    else:
        # (one sub-batch at a time under debug keeps the debug outputs of every row)
        step = SUB if debug else NQ
        spans = [(o, min(NQ, o + step)) for o in range(0, NQ, step)]
        assert [c[0] for c in entry] == ["tk_index_query_batch_allow"] * len(spans)
        assert [(n, a[0], a[1:]) for n, a in rec.named("tk_index_max_sub_batch")] == (
            [("tk_index_max_sub_batch", HANDLE, (K, NP, pass_1 or 0))] if debug else [])
    for (o, e), (_, args) in zip(spans, entry):
        if kind != "none":
            assert args[1] == aset
            args = args[:1] + args[2:]
        h, qn_p, qpq_p, is64, nq, k, n_probes, p1, out_p, probes_p, hidx_p, hval_p = args
        assert (h, nq) == (HANDLE, e - o) and (is64, k, n_probes, p1) == scalars
        assert addr(qn_p) == qn[o:e].ctypes.data and qn_p._arr.dtype == np.float32 and qn_p._arr.shape == (e - o, D)
        assert addr(qpq_p) == q_pq[o:e].ctypes.data
        assert addr(out_p) == out[o:e].ctypes.data and out_p._arr.dtype == np.int64 and out_p._arr.shape == (e - o, K)
        if debug:
            for p, a in ((probes_p, dbg["probes"]), (hidx_p, dbg["heap_idx"]), (hval_p, dbg["heap_val"])):
                assert addr(p) == a[o:e].ctypes.data
                assert p._arr.dtype == a.dtype and p._arr.shape == (e - o,) + a.shape[1:]
        else:
            assert probes_p is None and hidx_p is None and hval_p is None


def test_query_batch_streams_prepared_rows_where_it_can(rec, monkeypatch):
    """no debug, no allowed set, no distances, nq > 0, q_pq = pad(qn), a BLAS bound: the streaming session"""
    monkeypatch.setattr(_front, "bind", lambda: True)
    dev = bare_index()
    qn, _ = queries(False)
    q_pq = np.zeros((NQ, DQ), dtype=np.float32)
    q_pq[:, :D] = qn
    out = dev.query_batch(qn, q_pq, K, NP)
    assert out.dtype == np.int64 and out.shape == (NQ, K) and (out == -1).all()
    names = [c[0] for c in rec.calls]
    assert "tk_index_query_batch" not in names
    assert names.count("tk_stream_create") == 1 and names[-1] == "tk_stream_drain"
    sub = rec.named("tk_stream_submit_prepared")
    step = min(NQ, SUB)
    assert len(sub) == -(-NQ // step)
    for i, (_, (s, qn_a, qpq_a, n, out_a)) in enumerate(sub):
        o = i * step
        assert (qn_a, qpq_a, n, out_a) == (qn[o:].ctypes.data, None, min(step, NQ - o), out[o:].ctypes.data)
    # rotated / otherwise prepared table queries, a debug call, an empty batch: the plain entry point
    for kw, q2, n in ((dict(), q_pq + 1, NQ), (dict(debug=True), q_pq, NQ), (dict(), q_pq[:0], 0)):
        rec.calls.clear()
        dev.query_batch(qn[:n], q2, K, NP, **kw)
        assert [c[0] for c in rec.calls if c[0].startswith(("tk_index_query", "tk_stream_submit"))] == ["tk_index_query_batch"]


def test_query_batch_prepares_its_inputs(rec):
    """non-contiguous / other-dtype inputs are made contiguous float32 (float64 table queries stay float64)"""
    dev = bare_index()
    qn = np.asfortranarray(np.ones((NQ, D), dtype=np.float64))
    q_pq = np.asfortranarray(np.ones((NQ, DQ), dtype=np.float64))
    for kw, name in ((dict(), "tk_index_query_batch"), (dict(allowed=np.arange(4)), "tk_index_query_batch_allow"),
                     (dict(return_distances=True), "tk_index_query_batch_dist")):
        rec.calls.clear()
        dev.query_batch(qn, q_pq, K, NP, **kw)
        (_, args), = rec.named(name)
        args = args if name == "tk_index_query_batch" else args[:1] + args[2:]
        assert args[1]._arr.dtype == np.float32 and args[1]._arr.flags.c_contiguous and args[1]._arr.shape == (NQ, D)
        assert args[3] == 1 and isinstance(args[2], int)
    with pytest.raises(AssertionError):
        dev.query_batch(np.ones((NQ, D + 1), np.float32), np.ones((NQ, DQ), np.float32), K, NP)
    with pytest.raises(AssertionError):
        dev.query_batch(np.ones((NQ, D), np.float32), np.ones((NQ + 1, DQ), np.float32), K, NP, allowed=np.arange(4))
    other = bare_index()
    with pytest.raises(ValueError, match="another index"):
        dev.query_batch(np.ones((NQ, D), np.float32), np.ones((NQ, DQ), np.float32), K, NP, allowed=other.allow([1]))


QN, QPQ, OUT, DIST, EVENT, STREAM = 0x10000, 0x20000, 0x30000, 0x40000, 0xE0, 0x77


@pytest.mark.parametrize("done_event", [None, EVENT])
@pytest.mark.parametrize("dist_ptr", [None, DIST])
@pytest.mark.parametrize("prepared", [False, True])
def test_query_batch_dev_makes_one_foreign_call(rec, prepared, dist_ptr, done_event):
    dev = bare_index()
    aset = dev.allow(np.arange(0, N, 2)) if prepared else None
    rec.calls.clear()
    r = dev.query_batch_dev(QN, QPQ, 1, NQ, K, NP, OUT, pass_1=9, stream=STREAM, done_event=done_event,
                            allowed=aset, dist_ptr=dist_ptr)
    assert r is None
    (name, args), = rec.calls
    front = (QN, QPQ, 1, NQ, K, NP, 9, OUT)
    ev = addr(args[-2]) if len(args) > 10 else None
    assert ev == done_event and (done_event is None or isinstance(args[-2], C.c_void_p))
    assert args[0] == HANDLE and args[-1] == STREAM
    if dist_ptr is not None:
        assert name == "tk_index_query_batch_dev_dist"
        assert args[1] == (aset.handle if prepared else None) and args[2:10] == front and args[10] == DIST and len(args) == 13
    elif prepared:
        assert name == "tk_index_query_batch_dev_allow"
        assert args[1] == aset.handle and args[2:10] == front and args[10] is None and len(args) == 13
    elif name == "tk_index_query_batch_dev":
        assert done_event is None and args[1:9] == front and len(args) == 10
    else:       # the same C function with a NULL pinned buffer and the event (or none)
        assert name == "tk_index_query_batch_dev_ex"
        assert args[1:9] == front and args[9] is None and len(args) == 12
    assert rec.named("tk_allow_destroy") == []      # a prepared set stays open


def test_query_batch_dev_takes_prepared_sets_only(rec):
    dev = bare_index()
    for kw in (dict(), dict(dist_ptr=DIST)):
        with pytest.raises(TypeError, match="prepared set"):
            dev.query_batch_dev(QN, QPQ, 0, NQ, K, NP, OUT, allowed=np.ones(N, bool), **kw)
        with pytest.raises(ValueError, match="another index"):
            dev.query_batch_dev(QN, QPQ, 0, NQ, K, NP, OUT, allowed=bare_index().allow([0]), **kw)
    assert [c for c in rec.calls if c[0].startswith("tk_index_query")] == []


def python_calls(fn):
    n = [0]

    def prof(frame, event, arg):
        if event == "call":
            n[0] += 1
    sys.setprofile(prof)
    try:
        fn()
    finally:
        sys.setprofile(None)
    return n[0]


def test_query_batch_dev_python_calls_do_not_grow(rec):
    """Python-level calls (frames entered, the recorder's three included) of one query_batch_dev without allowed= /
    dist_ptr=, as counted with sys.setprofile before the host paths were folded: the method itself, _lib.lib, the
    recorder's __getattr__ and function, _lib.check.  The benchmark times this call; it must not get more."""
    dev = bare_index()
    assert python_calls(lambda: dev.query_batch_dev(QN, QPQ, 0, NQ, K, NP, OUT)) <= 6
    assert python_calls(lambda: dev.query_batch_dev(QN, QPQ, 0, NQ, K, NP, OUT, None, STREAM, EVENT)) <= 6


def fake_ivf():
    M = DQ // DPB
    pq = types.SimpleNamespace(centers=np.zeros((16, DQ), np.float32), dims_per_block=DPB, sqrt_n_blocks=2.0, R=None)
    lists = [types.SimpleNamespace(size=4, packed=np.zeros((1, M), np.uint64)) for _ in range(L)]
    return types.SimpleNamespace(
        pq=pq, active_centers=np.zeros((L, D), np.float32), pq_transformed_centers=(L, np.zeros((1, M), np.uint64)),
        pq_transformed_points=lists, ids=[np.arange(4 * i, 4 * i + 4) for i in range(L)],
        data=np.zeros((N, D), np.float64), metric="euclidean")


def test_three_constructors_one_state(rec):
    """uploaded, resident and cloned indexes have the same attributes (whatever a method reads is there), the clone
    inherits what describes the vectors, and allow() works on each"""
    up = made(DeviceIndex(fake_ivf()))
    res = made(DeviceIndex.resident(fake_ivf(), N, D))
    clone = made(up.clone_shard(np.zeros(L, np.int32), 0, 1))
    names = [set(dir(x)) for x in (up, res, clone)]
    assert names[0] == names[1] == names[2]
    assert up._f64 and clone._f64 and not res._f64
    assert clone._source is up and clone in up._clones
    for x in (up, res, clone):
        a = x.allow(np.ones(N, bool))
        assert isinstance(a, AllowSet) and a in x._live_allows
        h = a.handle
        x.close()
        assert a._h is None and h in [c[1][0] for c in rec.named("tk_allow_destroy")]


def test_mask_or_ids_parsers_keep_their_words():
    for fn, word in ((ivf_mod.removal_rows, "remove:"), (AllowSet.mask_of, "allowed:")):
        with pytest.raises(ValueError, match=word + ".*shape"):
            fn(np.ones(N + 1, bool), N)
        with pytest.raises(ValueError, match=word + ".*row ids"):
            fn(np.array([0, N]), N)
        with pytest.raises(TypeError, match=word):
            fn(np.array([0.5]), N)
        with pytest.raises(TypeError, match=word):
            fn(np.zeros((2, 2), np.int64), N)
    r = ivf_mod.removal_rows(np.array([3, 1, 3], np.int32), N)
    assert r.dtype == np.int64 and r.tolist() == [3, 1, 3] and r.flags.c_contiguous
    m = np.zeros(N, bool)
    m[[1, 3]] = True
    assert ivf_mod.removal_rows(m, N).tolist() == [1, 3]
    for arg in (m, np.array([3, 1, 3]), [1, 3]):
        got = AllowSet.mask_of(arg, N)
        assert got.dtype == np.uint8 and got.shape == (N,) and got.flags.c_contiguous and np.array_equal(got, m)
    assert ivf_mod.removal_rows([], N).shape == (0,) and not AllowSet.mask_of([], N).any()
