"""Which entry point of the library a DeviceIndex call reaches, and with what: the library is replaced by a recorder
(no GPU, no .so), so the Python layer's choices are visible — the foreign function, its scalars, the dtype and shape
of every buffer, the life of a temporary allowed set, the fill of what is returned.  Also: the three ways a
DeviceIndex is made give objects with the same attributes, and query_batch_dev (inside the benchmark's timed loop)
makes no more Python-level calls than it did.  The restricted calls (exclude / group / tags / between, host and device,
every subset) are compared in one normal form, the argument order of the _ex5 entry points, so the same assertions
held while the Python layer still chose among _ex2 .. _ex5.  Last, the words of every refusal of add / update / set_* /
query_batch(fast=True) about groups, tags and values, as they were before the three shared one body."""
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
        self.on_call = None         # on_call(name, args) while the call runs: its temporaries are still alive

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            if self.on_call is not None:
                self.on_call(name, args)
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


VKIND, VCOLS = "i", 2       # what set_values leaves behind for an (N, 2) integer array


def bare_index(f64=False, values=False):
    dev = DeviceIndex.__new__(DeviceIndex)
    dev._h, dev.d, dev.dq, dev.dpb, dev.n_lists, dev.N = HANDLE, D, DQ, DPB, L, N
    dev.angular, dev._R, dev._f64, dev.rank, dev.world = False, None, f64, 0, 1
    dev._streams, dev._live_streams, dev._live_allows = {}, weakref.WeakSet(), weakref.WeakSet()
    if values:
        dev._value_kind, dev._value_cols = VKIND, VCOLS
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


# ---- restricted calls: exclude / group / tags / between ----

def ex5_form(name, args, stem):
    """A recorded restricted call in the argument order of <stem>_ex5 — (handle, allowed set, exclude, group, tags,
    tag_mode, between, the queries ..., the outputs ...) — whichever of <stem>_ex2 .. _ex5 took it: the places an
    older entry point does not have are None (tag_mode: 0), which is what the library makes of them."""
    places = {stem + "_ex2": 0, stem + "_ex3": 1, stem + "_ex4": 3, stem + "_ex5": 4}[name]
    return args[:3] + args[3:3 + places] + (None, None, 0, None)[places:] + args[3 + places:]


# every subset of (allowed: none / prepared set / mask, exclude, group, tags under "any" / "all", between) with a restriction
RESTRICTED = [(a, x, g, t, b) for a in ("none", "set", "mask") for x in (False, True) for g in (False, True)
              for t in (None, "any", "all") for b in (False, True) if x or g or t or b]
TAG_MODE = {None: 0, "any": 0, "all": 1}


def restrictions(x, g, t, b):
    """(the keywords of a host call, the array the library must be handed for each restriction)"""
    kw, want = {}, dict(exclude=None, group=None, tags=None, between=None)
    if x:
        kw["exclude"] = np.array([-1, 3, 0, N - 1, 7], dtype=np.int32)
        want["exclude"] = np.array([-1, 3, 0, N - 1, 7], dtype=np.int64)
    if g:
        kw["group"] = np.array([2, -1, 0, 5, 2**31 - 2], dtype=np.int64)
        want["group"] = np.array([2, -1, 0, 5, 2**31 - 2], dtype=np.int32)
    if t:
        kw["tags"], kw["tags_mode"] = [1, 0, 2**64 - 1, 6, 2**63], t
        want["tags"] = np.array([1, 0, 2**64 - 1, 6, 2**63], dtype=np.uint64)
    if b:
        hi = np.arange(NQ * VCOLS).reshape(NQ, VCOLS) - 4
        kw["between"] = (3, hi)
        want["between"] = np.stack([np.full((NQ, VCOLS), 3), hi], axis=2).astype(np.int64)     # (NQ, VCOLS, 2)
    return kw, want


ROW_BYTES = dict(exclude=8, group=4, tags=8, between=16 * VCOLS)
PLACE = dict(exclude=2, group=3, tags=4, between=6)


def watch_restrictions(rec):
    """Per restricted host call, while it runs: {restriction: None or (address, the bytes of its nq rows)}"""
    seen = []

    def on_call(name, args):
        if name.startswith("tk_index_query_batch_ex"):
            a = ex5_form(name, args, "tk_index_query_batch")
            seen.append({w: None if a[i] is None else (addr(a[i]), C.string_at(addr(a[i]), a[10] * ROW_BYTES[w]))
                         for w, i in PLACE.items()})
    rec.on_call = on_call
    return seen


@pytest.mark.parametrize("q64", [False, True])
@pytest.mark.parametrize("return_distances,debug", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("kind,x,g,t,b", RESTRICTED)
def test_restricted_query_batch_hands_the_library_one_form(rec, kind, x, g, t, b, return_distances, debug, q64):
    dev = bare_index(f64=q64, values=True)
    qn, q_pq = queries(q64)
    allowed = allowed_arg(dev, kind)
    kw, want = restrictions(x, g, t, b)
    rec.calls.clear()
    seen = watch_restrictions(rec)
    if debug and return_distances:
        with pytest.raises(ValueError, match="debug=True cannot be combined with return_distances=True"):
            dev.query_batch(qn, q_pq, K, NP, 7, debug, allowed=allowed, return_distances=True, **kw)
        assert rec.calls == []
        return
    got = dev.query_batch(qn, q_pq, K, NP, 7, debug, allowed=allowed, return_distances=return_distances, **kw)

    # ---- what comes back, and its fills
    dbg = dist = None
    if return_distances:
        out, dist = got
        assert dist.dtype == (np.float64 if q64 else np.float32) and dist.shape == (NQ, K) and np.isposinf(dist).all()
    elif debug:
        out, dbg = got
        assert sorted(dbg) == ["heap_idx", "heap_val", "probes"]
        assert dbg["probes"].dtype == np.int64 and dbg["probes"].shape == (NQ, min(NP, L))
        assert dbg["heap_idx"].dtype == np.int64 and dbg["heap_idx"].shape == (NQ, 7)
        assert dbg["heap_val"].dtype == np.int32 and dbg["heap_val"].shape == (NQ, 7)
        assert not any(a.any() for a in dbg.values())
    else:
        out = got
    assert out.dtype == np.int64 and out.shape == (NQ, K) and (out == -1).all()

    # ---- the allowed set: a prepared one is used and left open, a mask becomes a set that is closed after the last call
    created = rec.named("tk_allow_create")
    destroyed = [a[0] for _, a in rec.named("tk_allow_destroy")]
    if kind == "set":
        assert created == [] and destroyed == []
        aset = allowed.handle
    elif kind == "mask":
        assert len(created) == 1 and created[0][1][0] == HANDLE
        assert np.array_equal(created[0][1][1]._arr, allowed.astype(np.uint8))
        aset = created[0][1][3]._obj.value
        assert destroyed == [aset] and rec.calls[-1][0] == "tk_allow_destroy"
    else:
        assert created == [] and destroyed == []
        aset = None

    # ---- one kind of entry point, one call per sub-batch (only debug splits), the _ex5 form of each
    entry = [c for c in rec.calls if c[0].startswith(("tk_index_query", "tk_stream"))]
    assert len({c[0] for c in entry}) == 1
    assert {c[0] for c in entry} == {"tk_index_query_batch_ex5"}         # (one entry point since the fold)
    step = SUB if debug else NQ
    spans = [(o, min(NQ, o + step)) for o in range(0, NQ, step)]
    assert len(entry) == len(spans) == len(seen)
    assert [a for _, a in rec.named("tk_index_max_sub_batch")] == ([(HANDLE, K, NP, 7)] if debug else [])
    for (o, e), (name, args), mem in zip(spans, entry, seen):
        a = ex5_form(name, args, "tk_index_query_batch")
        assert len(a) == 19 and (a[0], a[1]) == (HANDLE, aset)
        for w in PLACE:
            if want[w] is None:
                assert mem[w] is None
            else:       # one array for the batch, each call at its rows of it
                assert mem[w][1] == want[w][o:e].tobytes()
                assert mem[w][0] == seen[0][w][0] + o * ROW_BYTES[w]
        assert a[5] == TAG_MODE[t] and isinstance(a[5], int)
        qn_p, qpq_p, out_p, dist_p, probes_p, hidx_p, hval_p = a[7], a[8], a[14], a[15], a[16], a[17], a[18]
        assert a[9:14] == (int(q64), e - o, K, NP, 7)
        assert addr(qn_p) == qn[o:e].ctypes.data and qn_p._arr.dtype == np.float32 and qn_p._arr.shape == (e - o, D)
        assert addr(qpq_p) == q_pq[o:e].ctypes.data
        assert addr(out_p) == out[o:e].ctypes.data and out_p._arr.dtype == np.int64 and out_p._arr.shape == (e - o, K)
        assert addr(dist_p) == (dist[o:e].ctypes.data if return_distances else None)
        if debug:
            for p, arr in ((probes_p, dbg["probes"]), (hidx_p, dbg["heap_idx"]), (hval_p, dbg["heap_val"])):
                assert addr(p) == arr[o:e].ctypes.data
                assert p._arr.dtype == arr.dtype and p._arr.shape == (e - o,) + arr.shape[1:]
        else:
            assert probes_p is None and hidx_p is None and hval_p is None


def test_restricted_query_batch_details(rec):
    """tags_mode counts only beside tags; a scalar group / tags is one entry per query; without values a between= call
    hands over an array the library refuses; bad arguments reach nothing"""
    dev = bare_index(values=True)
    qn, q_pq = queries(False)
    seen = watch_restrictions(rec)
    dev.query_batch(qn, q_pq, K, NP, exclude=np.full(NQ, -1), tags_mode="all")
    dev.query_batch(qn, q_pq, K, NP, group=4, tags=9, tags_mode="all")
    (_, a0), (_, a1) = [(n, ex5_form(n, a, "tk_index_query_batch")) for n, a in rec.calls]
    assert a0[5] == 0 and a1[5] == 1
    assert seen[1]["group"][1] == np.full(NQ, 4, np.int32).tobytes()
    assert seen[1]["tags"][1] == np.full(NQ, 9, np.uint64).tobytes()
    del seen[:]
    plain = bare_index()
    plain.query_batch(qn, q_pq, K, NP, between=(0, 1))
    (name, args), = rec.calls[2:]
    assert addr(ex5_form(name, args, "tk_index_query_batch")[6]) is not None
    n = len(rec.calls)
    for kw, exc in ((dict(tags=1, tags_mode="some"), ValueError), (dict(exclude=np.zeros(NQ + 1, np.int64)), ValueError),
                    (dict(exclude=np.full(NQ, N)), ValueError), (dict(exclude=np.zeros(NQ)), TypeError),
                    (dict(group=np.zeros(NQ - 1, np.int64)), ValueError), (dict(group=0.5), TypeError),
                    (dict(tags=-1), ValueError), (dict(between=(np.zeros(NQ - 1), None)), ValueError),
                    (dict(between=3), TypeError)):
        with pytest.raises(exc):
            dev.query_batch(qn, q_pq, K, NP, allowed=np.arange(4), **kw)
    assert len(rec.calls) == n


EXCL, GRP, TAGS, BETW = 0x50000, 0x60000, 0x70000, 0x80000


@pytest.mark.parametrize("done_event", [None, EVENT])
@pytest.mark.parametrize("dist_ptr", [None, DIST])
@pytest.mark.parametrize("prepared,x,g,t,b", [(a == "set", x, g, t, b) for a, x, g, t, b in RESTRICTED if a != "mask"])
def test_restricted_query_batch_dev_makes_one_foreign_call(rec, prepared, x, g, t, b, dist_ptr, done_event):
    dev = bare_index()
    aset = dev.allow(np.arange(0, N, 2)) if prepared else None
    rec.calls.clear()
    kw = dict(exclude_ptr=EXCL if x else None, group_ptr=GRP if g else None, tags_ptr=TAGS if t else None,
              between_ptr=BETW if b else None)
    if t:
        kw["tags_mode"] = t
    r = dev.query_batch_dev(QN, QPQ, 1, NQ, K, NP, OUT, pass_1=9, stream=STREAM, done_event=done_event,
                            allowed=aset, dist_ptr=dist_ptr, **kw)
    assert r is None
    (name, args), = rec.calls
    assert name == "tk_index_query_batch_dev_ex5"                        # (one entry point since the fold)
    a = ex5_form(name, args, "tk_index_query_batch_dev")
    assert a[:16] == (HANDLE, aset.handle if prepared else None, kw["exclude_ptr"], kw["group_ptr"], kw["tags_ptr"],
                      TAG_MODE[t], kw["between_ptr"], QN, QPQ, 1, NQ, K, NP, 9, OUT, dist_ptr)
    assert isinstance(a[5], int) and len(a) == 18
    assert addr(a[16]) == done_event and (done_event is None or isinstance(a[16], C.c_void_p))
    assert a[17] == STREAM
    assert rec.named("tk_allow_destroy") == []      # a prepared set stays open


def test_restricted_query_batch_dev_details(rec):
    """tags_mode counts only beside tags_ptr, and is checked there before anything is called"""
    dev = bare_index()
    dev.query_batch_dev(QN, QPQ, 0, NQ, K, NP, OUT, exclude_ptr=EXCL, tags_mode="all")
    dev.query_batch_dev(QN, QPQ, 0, NQ, K, NP, OUT, between_ptr=BETW, tags_mode="all")
    assert [ex5_form(n, a, "tk_index_query_batch_dev")[5] for n, a in rec.calls] == [0, 0]
    with pytest.raises(ValueError, match="tags_mode"):
        dev.query_batch_dev(QN, QPQ, 0, NQ, K, NP, OUT, tags_ptr=TAGS, tags_mode="some")
    with pytest.raises(TypeError, match="prepared set"):
        dev.query_batch_dev(QN, QPQ, 0, NQ, K, NP, OUT, group_ptr=GRP, allowed=np.ones(N, bool))
    assert len(rec.calls) == 2


def test_restricted_query_batch_dev_python_calls_do_not_grow(rec):
    """As test_query_batch_dev_python_calls_do_not_grow, for a call with each restriction pointer alone and with all
    four.  The bounds are the counts of the commit before the restricted calls were folded onto one entry point
    (exclude, group, between: 6; tags, and all four: 7 — tag_mode_of is one more frame)."""
    dev = bare_index()
    ptrs = dict(exclude_ptr=EXCL, group_ptr=GRP, tags_ptr=TAGS, between_ptr=BETW)
    for kw, bound in [({k: v}, BOUNDS[k]) for k, v in ptrs.items()] + [(ptrs, BOUNDS["all"])]:
        assert python_calls(lambda: dev.query_batch_dev(QN, QPQ, 0, NQ, K, NP, OUT, None, STREAM, EVENT, **kw)) <= bound


BOUNDS = dict(exclude_ptr=6, group_ptr=6, tags_ptr=7, between_ptr=6, all=7)      # (measured on that commit)


# ---- refusals: who refuses what, in which words ----

ROWS = 4        # rows of an add / update below


def host_ivf(*has):
    """An IVF with N rows and the row attributes named, nothing else: what add / update / set_* / query_batch decide
    before they need centres, lists or a device"""
    ivf = ivf_mod.IVF("euclidean", 3, None)
    ivf.data = np.zeros((N, D), np.float32)
    for name, a in (("groups", np.arange(N, dtype=np.int32)), ("tags", np.arange(N, dtype=np.uint64)),
                    ("values", np.arange(N * VCOLS, dtype=np.int16).reshape(N, VCOLS))):
        if name in has:
            setattr(ivf, name, a)
    return ivf


X, IDS = np.zeros((ROWS, D), np.float32), np.arange(ROWS)
GOOD = dict(groups=np.zeros(ROWS, np.int64), tags=np.zeros(ROWS, np.int64), values=np.zeros((ROWS, VCOLS), np.int64))
NO_CENTRES = "the index has no all_centers (fit, or a file written with them)"
ALL3 = ("groups", "tags", "values")

# (the index's attributes, the call, the exception, its whole text) — as recorded before the three attributes shared one body
ADD_UPDATE_REFUSALS = [
    # add: an attribute the index lacks is not taken, one it has is needed; groups, tags, values in this order, all
    # after X's shape and before the centres are asked for
    ((), lambda i: i.add(X, groups=GOOD["groups"]), ValueError, "IVF.add: groups= on an index without groups (set_groups first)"),
    ((), lambda i: i.add(X, tags=GOOD["tags"]), ValueError, "IVF.add: tags= on an index without tags (set_tags first)"),
    ((), lambda i: i.add(X, values=GOOD["values"]), ValueError, "IVF.add: values= on an index without values (set_values first)"),
    ((), lambda i: i.add(X, **GOOD), ValueError, "IVF.add: groups= on an index without groups (set_groups first)"),
    (("values",), lambda i: i.add(X, tags=GOOD["tags"]), ValueError, "IVF.add: tags= on an index without tags (set_tags first)"),
    (("groups",), lambda i: i.add(X), ValueError, "IVF.add: this index has groups (set_groups): pass the new rows' with groups="),
    (("tags",), lambda i: i.add(X), ValueError, "IVF.add: this index has tags (set_tags): pass the new rows' with tags="),
    (("values",), lambda i: i.add(X), ValueError, "IVF.add: this index has values (set_values): pass the new rows' with values="),
    (ALL3, lambda i: i.add(X), ValueError, "IVF.add: this index has groups (set_groups): pass the new rows' with groups="),
    (ALL3, lambda i: i.add(X, groups=GOOD["groups"], values=GOOD["values"]), ValueError,
     "IVF.add: this index has tags (set_tags): pass the new rows' with tags="),
    (ALL3, lambda i: i.add(X[:, :-1], groups=[0.5]), AssertionError, f"IVF.add: X must have shape (n, {D}), got ({ROWS}, {D - 1})"),
    (("groups",), lambda i: i.add(X, groups=np.zeros(ROWS - 1, int)), ValueError, f"IVF.add: groups: one group id per row ({ROWS}), got {ROWS - 1}"),
    (("groups",), lambda i: i.add(X, groups=np.zeros(ROWS)), TypeError, "IVF.add: groups: a 1-d integer array, one group id per row"),
    (("groups",), lambda i: i.add(X, groups=np.full(ROWS, -1)), ValueError, "IVF.add: groups: group ids must lie in [0, 2**31 - 1)"),
    (("tags",), lambda i: i.add(X, tags=np.zeros(ROWS + 1, int)), ValueError, f"IVF.add: tags: one tag mask per row ({ROWS}), got {ROWS + 1}"),
    (("tags",), lambda i: i.add(X, tags=np.zeros(ROWS, bool)), TypeError, "IVF.add: tags: a 1-d integer array, one tag mask per row"),
    (("tags",), lambda i: i.add(X, tags=[-1] * ROWS), ValueError, "IVF.add: tags: tag masks must lie in [0, 2**64)"),
    (("values",), lambda i: i.add(X, values=np.zeros(ROWS, int)), ValueError,
     f"IVF.add: values: shape (n,) + ({VCOLS},) as the index's values, got ({ROWS},)"),
    (("values",), lambda i: i.add(X, values=np.zeros((ROWS, VCOLS))), ValueError, "IVF.add: values: int16 as the index's values, got float64"),
    (("values",), lambda i: i.add(X, values=np.full((ROWS, VCOLS), 2**15)), ValueError, "IVF.add: values: values that do not fit the index's int16"),
    (("values",), lambda i: i.add(X, values=np.zeros((ROWS - 1, VCOLS), int)), ValueError,
     f"IVF.add: values: one row of values per row ({ROWS}), got {ROWS - 1}"),
    (("values",), lambda i: i.add(X, values="price"), TypeError, "IVF.add: values: a (n,) or (n, C) array of one integer or floating dtype"),
    (ALL3, lambda i: i.add(X, **GOOD), AssertionError, "IVF.add: " + NO_CENTRES),
    ((), lambda i: i.add(X), AssertionError, "IVF.add: " + NO_CENTRES),
    # update: an attribute the index lacks is not taken, one it has may be left out (the rows keep theirs)
    ((), lambda i: i.update(IDS, X, groups=GOOD["groups"]), ValueError, "IVF.update: groups= on an index without groups (set_groups first)"),
    ((), lambda i: i.update(IDS, X, tags=GOOD["tags"]), ValueError, "IVF.update: tags= on an index without tags (set_tags first)"),
    ((), lambda i: i.update(IDS, X, values=GOOD["values"]), ValueError, "IVF.update: values= on an index without values (set_values first)"),
    (("tags",), lambda i: i.update(IDS, X, **GOOD), ValueError, "IVF.update: groups= on an index without groups (set_groups first)"),
    ((), lambda i: i.update(IDS, X[:-1], groups=GOOD["groups"]), AssertionError,
     f"IVF.update: X must have shape ({ROWS}, {D}), got ({ROWS - 1}, {D})"),
    ((), lambda i: i.update([0, 0], X[:2], groups=GOOD["groups"]), ValueError, "update: row ids must be pairwise distinct"),
    (ALL3, lambda i: i.update(IDS, X, groups=np.zeros(ROWS - 1, int)), ValueError, f"IVF.update: groups: one group id per row ({ROWS}), got {ROWS - 1}"),
    (ALL3, lambda i: i.update(IDS, X, tags=np.zeros(ROWS)), TypeError, "IVF.update: tags: a 1-d integer array, one tag mask per row"),
    (ALL3, lambda i: i.update(IDS, X, values=np.zeros((ROWS, VCOLS + 1), int)), ValueError,
     f"IVF.update: values: shape (n,) + ({VCOLS},) as the index's values, got ({ROWS}, {VCOLS + 1})"),
    (ALL3, lambda i: i.update(IDS, X), AssertionError, "IVF.update: " + NO_CENTRES),
    (ALL3, lambda i: i.update(IDS, X, **GOOD), AssertionError, "IVF.update: " + NO_CENTRES),
]

SET_REFUSALS = [
    (lambda o: o.set_groups(np.zeros(N - 1, int)), ValueError, "{}set_groups: one group id per row (40), got 39"),
    (lambda o: o.set_groups(np.zeros(N)), TypeError, "{}set_groups: a 1-d integer array, one group id per row"),
    (lambda o: o.set_groups(np.zeros((N, 1), int)), TypeError, "{}set_groups: a 1-d integer array, one group id per row"),
    (lambda o: o.set_groups(np.full(N, 2**31 - 1)), ValueError, "{}set_groups: group ids must lie in [0, 2**31 - 1)"),
    (lambda o: o.set_tags(np.zeros(N + 1, int)), ValueError, "{}set_tags: one tag mask per row (40), got 41"),
    (lambda o: o.set_tags(np.zeros(N, bool)), TypeError, "{}set_tags: a 1-d integer array, one tag mask per row"),
    (lambda o: o.set_tags([2**64] * N), ValueError, "{}set_tags: tag masks must lie in [0, 2**64)"),
    (lambda o: o.set_values(np.zeros(N - 1)), ValueError, "{}set_values: one row of values per row (40), got 39"),
    (lambda o: o.set_values(np.zeros((N, 5))), ValueError, "{}set_values: 1 to 4 columns, got 5"),
    (lambda o: o.set_values(np.full(N, np.nan)), ValueError, "{}set_values: NaN has no place in an order"),
    (lambda o: o.set_values(np.full(N, 2**63, np.uint64)), ValueError, "{}set_values: uint64 values above 2**63 - 1 have no int64 key"),
    (lambda o: o.set_values(np.zeros(N, bool)), TypeError, "{}set_values: a (n,) or (n, C) array of one integer or floating dtype"),
    (lambda o: o.set_values(np.zeros(N, complex)), TypeError, "{}set_values: a (n,) or (n, C) array of one integer or floating dtype"),
]
SHARDED = [("set_groups", "DeviceIndex.set_groups: a list-sharded index takes no row groups"),
           ("set_tags", "DeviceIndex.set_tags: a list-sharded index takes no row tags"),
           ("set_values", "DeviceIndex.set_values: a list-sharded index takes no row values")]
IVF_SHARDED = ("this IVF's device index has been list-sharded in place (ListShardedIndex on an index built in HBM: "
               "rank 0 of 2); query it through the ListShardedIndex")

FAST = "IVF.query_batch: fast=True with {} is not supported; use the exact default (fast=False)"
IN_RANGE, TAG, GROUP, NOT_ROW0 = dict(between=(0, 1)), dict(tags=1), dict(group=1), dict(exclude=np.zeros(NQ, np.int64))
FAST_REFUSALS = [       # between, tags, group, exclude, return_distances, allowed: the first of these that is given
    (IN_RANGE, "between="), (TAG, "tags="), (GROUP, "group="), (NOT_ROW0, "exclude="),
    (dict(return_distances=True), "return_distances=True"), (dict(allowed=np.arange(3)), "allowed="),
    (dict(allowed=np.arange(3), **IN_RANGE), "between="), (dict(return_distances=True, **NOT_ROW0), "exclude="),
    (dict(**GROUP, **TAG, tags_mode="some"), "tags="), (dict(return_distances=True, allowed=np.arange(3)), "return_distances=True"),
    (dict(between="not a pair", **GROUP), "between="),
]


def state_of(ivf):
    return {k: (v.dtype, v.tobytes()) if isinstance(v, np.ndarray) else v for k, v in vars(ivf).items() if k != "pq"}


@pytest.mark.parametrize("has,call,exc,text", ADD_UPDATE_REFUSALS)
def test_add_and_update_refusals_keep_their_words(rec, has, call, exc, text):
    ivf = host_ivf(*has)
    before = state_of(ivf)
    with pytest.raises(exc) as e:
        call(ivf)
    assert str(e.value) == text
    assert state_of(ivf) == before and rec.calls == []          # a refused call changes nothing


@pytest.mark.parametrize("call,exc,text", SET_REFUSALS)
def test_set_refusals_keep_their_words(rec, call, exc, text):
    ivf = host_ivf(*ALL3)
    ivf._dev = bare_index()
    before = state_of(ivf)
    for obj, prefix in ((ivf, "IVF."), (ivf._dev, "")):
        with pytest.raises(exc) as e:
            call(obj)
        assert str(e.value) == text.format(prefix)
    assert state_of(ivf) == before and rec.calls == []
    assert (ivf._dev._value_kind, ivf._dev._value_cols) == (None, 0)


@pytest.mark.parametrize("name,text", SHARDED)
def test_set_on_a_list_sharded_index_keeps_its_words(rec, name, text):
    ivf = host_ivf(*ALL3)
    dev = ivf._dev = bare_index()
    before = state_of(ivf)
    arg = {"set_groups": np.zeros(N, int), "set_tags": np.zeros(N, int), "set_values": np.zeros(N)}[name]
    for shard in (lambda: setattr(dev, "world", 2), lambda: setattr(dev, "_sharded_as", (None, 0, 2)),
                  lambda: setattr(dev, "_source", bare_index())):
        dev.world, dev._sharded_as, dev._source = 1, None, None
        shard()
        for a in (arg, None):
            with pytest.raises(RuntimeError) as e:
                getattr(dev, name)(a)
            assert str(e.value) == text
    dev.world, dev._sharded_as, dev._source = 2, None, None
    for a in (arg, None):               # the IVF refuses before its host copy changes
        with pytest.raises(RuntimeError) as e:
            getattr(ivf, name)(a)
        assert str(e.value) == IVF_SHARDED
    assert state_of(ivf) == before and rec.calls == []


@pytest.mark.parametrize("kw,word", FAST_REFUSALS)
def test_fast_query_batch_refusals_keep_their_words_and_order(rec, kw, word):
    ivf = host_ivf("values")
    ivf._dev = bare_index(values=True)
    with pytest.raises(NotImplementedError) as e:
        ivf.query_batch(np.zeros((NQ, D), np.float32), K, NP, fast=True, **kw)
    assert str(e.value) == FAST.format(word) and rec.calls == []


def test_exact_query_batch_checks_keep_their_order(rec):
    """between's ranges, then tags_mode, before the device index is asked for; exclude's length after it"""
    ivf, qs = host_ivf(), np.zeros((NQ, D), np.float32)
    ivf._dev = bare_index()
    ivf._dev.world = 2              # (asking for the device index raises)
    for kw, exc, text in (
            (dict(between=(0, 1), tags=1, tags_mode="some"), ValueError, "between= on an index without values (set_values first)"),
            (dict(tags=1, tags_mode="some", exclude=np.zeros(NQ + 1, int)), ValueError, "tags_mode: \"any\" or \"all\", got 'some'"),
            (dict(exclude=np.zeros(NQ + 1, int)), RuntimeError, IVF_SHARDED)):
        with pytest.raises(exc) as e:
            ivf.query_batch(qs, K, NP, **kw)
        assert str(e.value) == text
    ivf._dev.world = 1
    with pytest.raises(ValueError) as e:
        ivf.query_batch(qs, K, NP, exclude=np.zeros(NQ + 1, int), group=np.zeros(NQ + 2, int))
    assert str(e.value) == f"exclude: one entry per query ({NQ}), got {NQ + 1}"
    assert rec.calls == []


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
