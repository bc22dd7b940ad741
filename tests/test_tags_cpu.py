"""Row tags without a GPU: the reference helper is the guarded reference with the set the two formulas give per query;
the Python layer's validation, add(tags=) / update(tags=) bookkeeping and persistence; the ABI's declarations; the
kernels of tags.hip compile for gfx950 without scratch or spills; and, on the reference alone, that the inputs of
tests/test_tags_gpu.py (tests/tag_shapes.py) can tell a right tag pass from a wrong one — restricted answers that
differ from the unrestricted ones, short and full answers, and answers that change when only the low words of the
masks are compared.  (tk_index_create needs a GPU, so the ABI's TK_ERR_STATE refusals are in tests/test_tags_gpu.py.)"""
import os
import pickle
import re
import sys
import time
import weakref

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tag_shapes as ts  # noqa: E402
from allowed_reference import guarded_batch  # noqa: E402
from conftest import G6_TAGS, golden, split_lists  # noqa: E402
from groups_reference import grouped_batch  # noqa: E402
from kernel_usage import kernel_usage  # noqa: E402
from store_reference import oracle_index  # noqa: E402
from tags_reference import passing, tagged_batch  # noqa: E402

KEYS = ("probes", "heap_idx", "heap_val")
U64 = np.uint64


def _fixture(oracle, tag):
    g = golden(f"g6_ivf_{tag}.npz")
    codes, ids = split_lists(g)
    R = g["R"] if "R" in g else None
    ox = oracle.OracleIndex(g["pq_centers"], 2, R, float(g["sqrt_n_blocks"]), g["active_centers"],
                            g["center_codes"], codes, g["list_sizes"], ids, g["data"])
    return ox, np.ascontiguousarray(g["qn"]), ids, len(g["data"])


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    for key in KEYS:
        np.testing.assert_array_equal(a[1][key], b[1][key], err_msg=key)


@pytest.mark.parametrize("tag", ["an100b2", "eu20"])
def test_helper_all_zero_is_the_unrestricted_reference(oracle, tag):
    ox, qn, ids, N = _fixture(oracle, tag)
    tags = ts.assignments(ids, N, 1)["some"]
    want = guarded_batch(oracle, ox, qn, 10, 5, debug=True)
    for mode in ts.MODES:
        _same(tagged_batch(oracle, ox, qn, np.zeros(len(qn), dtype=U64), mode, tags, 10, 5, debug=True), want)
        _same(tagged_batch(oracle, ox, qn, 0, mode, tags, 10, 5, debug=True), want)


@pytest.mark.parametrize("tag", ["an100b2", "eu20"])
def test_helper_one_mask_is_the_guarded_reference_of_that_set(oracle, tag):
    ox, qn, ids, N = _fixture(oracle, tag)
    tags = ts.assignments(ids, N, 1)["nested"]
    both = ts.bit(5) | ts.bit(40)
    sets = {("any", both): np.ones(N, dtype=bool), ("all", both): tags == both,
            ("any", ts.bit(40)): tags == both, ("all", ts.bit(40)): tags == both,
            ("any", ts.bit(63)): np.zeros(N, dtype=bool), ("all", ts.bit(5) | ts.bit(63)): np.zeros(N, dtype=bool),
            ("any", ts.bit(5) | ts.bit(63)): np.ones(N, dtype=bool)}
    plain = guarded_batch(oracle, ox, qn, 10, 5)
    for (mode, m), allowed in sets.items():
        np.testing.assert_array_equal(passing(tags, m, mode), allowed)
        want = guarded_batch(oracle, ox, qn, 10, 5, allowed=allowed, debug=True)
        got = tagged_batch(oracle, ox, qn, np.full(len(qn), m, dtype=U64), mode, tags, 10, 5, debug=True)
        _same(got, want)
        got_ids = got[0][got[0] != -1]
        assert allowed[got_ids].all() and (allowed.any() or got_ids.size == 0)
    assert (tagged_batch(oracle, ox, qn, both, "all", tags, 10, 5) != plain).any()
    # mixed: every query is its own mask's
    mixed = np.array([0, ts.bit(40), ts.bit(63), both], dtype=U64)[np.arange(len(qn)) % 4]
    got = tagged_batch(oracle, ox, qn, mixed, "all", tags, 10, 5)
    for m in np.unique(mixed):
        sel = mixed == m
        np.testing.assert_array_equal(got[sel], guarded_batch(oracle, ox, qn[sel], 10, 5, allowed=passing(tags, m, "all")))
    assert (got[mixed == ts.bit(63)] == -1).all()
    # with a set, an excluded row and a group as well: the intersection
    allowed = np.arange(N) % 2 == 0
    groups = (np.arange(N) % 3).astype(np.int32)
    first = tagged_batch(oracle, ox, qn, both, "all", tags, 10, 5, allowed=allowed, group=1, groups=groups)[:, 0]
    assert (first >= 0).any()
    got = tagged_batch(oracle, ox, qn, both, "all", tags, 10, 5, allowed=allowed, exclude=first, group=1, groups=groups)
    for i in range(len(qn)):
        m = (tags == both) & allowed & (groups == 1)
        if first[i] >= 0:
            m[first[i]] = False
        np.testing.assert_array_equal(got[i:i + 1], guarded_batch(oracle, ox, qn[i:i + 1], 10, 5, allowed=m))
    # no tag mask at all: grouped_batch
    np.testing.assert_array_equal(tagged_batch(oracle, ox, qn, 0, "any", tags, 10, 5, exclude=first, group=1, groups=groups),
                                  grouped_batch(oracle, ox, qn, 1, groups, 10, 5, exclude=first))


# ---- the Python layer ----

def _built(kp=1, n=2000, d=40, clusters=20, seed=0):
    from tinyknn_amd import IVF, FastPQ
    X = np.random.RandomState(seed).randn(n + 300, d).astype(np.float32)
    ivf = IVF("angular", clusters, FastPQ(2))
    np.random.seed(seed)
    ivf.fit(X[:1500])
    ivf.build(X[:n], n_probes=kp, device=False)
    return ivf, X[n:]


def test_set_tags_validation():
    ivf, _ = _built()
    N = len(ivf.data)
    assert ivf.tags is None and "tags" not in vars(ivf)
    for bad in (np.zeros(N), np.zeros(N, dtype=bool), np.zeros((N, 1), dtype=np.int64), "acl", 3,
                np.zeros(N, dtype=np.float32)):
        with pytest.raises(TypeError):
            ivf.set_tags(bad)
    for bad in (np.zeros(N - 1, dtype=np.int64), np.zeros(N + 1, dtype=np.uint64), np.full(N, -1),
                np.where(np.arange(N) == 7, -1, 1), [2**64] + [0] * (N - 1)):
        with pytest.raises(ValueError):
            ivf.set_tags(bad)
    assert ivf.tags is None
    t = np.arange(N, dtype=np.int64) % 5
    assert ivf.set_tags(t) is ivf
    assert ivf.tags.dtype == np.uint64 and np.array_equal(ivf.tags, t.astype(np.uint64))
    big = np.full(N, 2**63, dtype=np.uint64)            # the top bit: no int64 holds it
    big[1] = 2**64 - 1
    ivf.set_tags(big)
    assert ivf.tags[0] == 2**63 and ivf.tags[1] == 2**64 - 1
    big[1] = 77                                         # the index keeps its own copy
    assert ivf.tags[1] == 2**64 - 1
    ivf.set_tags([2**63, 1] + [0] * (N - 2))            # Python ints on both sides of 2**63
    assert ivf.tags.dtype == np.uint64 and ivf.tags[0] == 2**63 and ivf.tags[1] == 1
    ivf.set_tags(np.arange(N, dtype=np.int8) % 3)       # any integer dtype
    assert ivf.tags.dtype == np.uint64
    ivf.set_tags(None)
    assert ivf.tags is None and "tags" not in vars(ivf)


def test_add_and_update_tags_bookkeeping():
    ivf, more = _built()
    N = len(ivf.data)
    with pytest.raises(ValueError, match="without tags"):
        ivf.add(more[:10], tags=np.zeros(10, dtype=np.uint64))
    with pytest.raises(ValueError, match="without tags"):
        ivf.update(np.arange(3), more[:3], tags=np.zeros(3, dtype=np.uint64))
    assert len(ivf.data) == N
    t = (np.arange(N) % 4).astype(np.uint64)
    ivf.set_tags(t)
    ids_before = [np.array(x, copy=True) for x in ivf.ids[:len(ivf.active_centers)]]
    with pytest.raises(ValueError, match="tags"):
        ivf.add(more[:10])
    with pytest.raises(ValueError):
        ivf.add(more[:10], tags=np.zeros(9, dtype=np.uint64))
    with pytest.raises(ValueError):
        ivf.add(more[:10], tags=np.full(10, -1))
    with pytest.raises(TypeError):
        ivf.add(more[:10], tags=np.zeros(10))
    with pytest.raises(ValueError):
        ivf.update(np.arange(3), more[:3], tags=np.full(3, -1))
    assert len(ivf.data) == N and np.array_equal(ivf.tags, t)      # refused before anything changed
    for a, b in zip(ids_before, ivf.ids):
        np.testing.assert_array_equal(a, b)
    ivf.add(more[:10], tags=np.arange(10) + 100)
    assert len(ivf.data) == N + 10 and ivf.tags.dtype == np.uint64
    np.testing.assert_array_equal(ivf.tags, np.concatenate([t, np.arange(10, dtype=np.uint64) + 100]))
    ivf.add(more[:0], tags=np.zeros(0, dtype=np.uint64))
    assert len(ivf.tags) == N + 10
    # update: without tags= the rows keep theirs; with it, those rows change
    before = ivf.tags.copy()
    ivf.update(np.array([3, N + 2]), more[20:22])
    np.testing.assert_array_equal(ivf.tags, before)
    ivf.update(np.array([3, N + 2]), more[22:24], tags=np.array([2**63, 9], dtype=np.uint64))
    assert ivf.tags[3] == 2**63 and ivf.tags[N + 2] == 9
    before[[3, N + 2]] = 0
    assert np.array_equal(np.where(np.isin(np.arange(N + 10), [3, N + 2]), 0, ivf.tags), before)
    # remove leaves tags alone: a removed row keeps its entry
    after = ivf.tags.copy()
    ivf.remove(np.array([3, 5]))
    np.testing.assert_array_equal(ivf.tags, after)
    # an index with groups and tags: add needs both
    ivf.set_groups(np.zeros(N + 10, dtype=np.int32))
    with pytest.raises(ValueError, match="tags"):
        ivf.add(more[:5], groups=np.zeros(5, dtype=np.int32))
    with pytest.raises(ValueError, match="groups"):
        ivf.add(more[:5], tags=np.zeros(5, dtype=np.uint64))
    assert len(ivf.data) == N + 10
    ivf.add(more[:5], groups=np.ones(5, dtype=np.int32), tags=np.full(5, 6))
    assert len(ivf.tags) == len(ivf.groups) == N + 15 and ivf.tags[-1] == 6
    # an index without tags: add as before
    plain, more = _built()
    plain.add(more[:10])
    assert plain.tags is None and len(plain.data) == N + 10
    # a new build drops the tags of the rows before
    ivf.build(np.asarray(ivf.data[:500]), n_probes=1, device=False)
    assert ivf.tags is None


def test_save_load_and_pickle_carry_tags(tmp_path, monkeypatch):
    from tinyknn_amd import IVF
    stamp = time.localtime(86400 * 365 * 30)
    monkeypatch.setattr(time, "localtime", lambda *a: stamp)     # (the archive's member times: equal for every file)
    ivf, _ = _built(kp=2)
    N = len(ivf.data)
    ivf.save(tmp_path / "never")
    never = open(tmp_path / "never.npz", "rb").read()
    assert "tags" not in np.load(tmp_path / "never.npz").files
    assert IVF.load(tmp_path / "never").tags is None
    state_never = set(ivf.__getstate__())
    t = (np.arange(N) % 11).astype(np.uint64) | (np.uint64(1) << np.uint64(63))
    ivf.set_tags(t)
    ivf.save(tmp_path / "with")
    back = IVF.load(tmp_path / "with")
    assert back.tags.dtype == np.uint64
    np.testing.assert_array_equal(back.tags, t)
    twin = pickle.loads(pickle.dumps(ivf))
    np.testing.assert_array_equal(twin.tags, t)
    # cleared again: exactly the file, and the pickled state, of an index whose tags were never set
    ivf.set_tags(None)
    ivf.save(tmp_path / "cleared")
    assert open(tmp_path / "cleared.npz", "rb").read() == never
    assert set(ivf.__getstate__()) == state_never
    assert pickle.loads(pickle.dumps(ivf)).tags is None


N0, D, DQ = 40, 6, 8


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"{name}: a refused call must not reach the library")


@pytest.fixture
def bare(monkeypatch):
    from tinyknn_amd import _lib
    from tinyknn_amd.ivf import DeviceIndex
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    dev = DeviceIndex.__new__(DeviceIndex)
    dev._h, dev.d, dev.dq, dev.dpb, dev.n_lists, dev.N = 0x10, D, DQ, 2, 3, N0
    dev.angular, dev._R, dev._f64, dev.rank, dev.world = False, None, False, 0, 1
    dev._source = None
    dev._streams, dev._live_streams, dev._live_allows = {}, weakref.WeakSet(), weakref.WeakSet()
    yield dev
    dev._h = None


def test_query_refusals_decided_on_the_host(bare):
    from tinyknn_amd import IVF
    qn, qp = np.zeros((5, D), np.float32), np.zeros((5, DQ), np.float32)
    with pytest.raises(ValueError, match="one entry per query"):
        bare.query_batch(qn, qp, 3, 1, tags=[1, 2, 3])
    with pytest.raises(ValueError):
        bare.query_batch(qn, qp, 3, 1, tags=[0, 1, 2, 3, -2])
    with pytest.raises(ValueError):
        bare.query_batch(qn, qp, 3, 1, tags=-1)
    with pytest.raises(ValueError):
        bare.query_batch(qn, qp, 3, 1, tags=2**64)
    for bad in (np.zeros((5, 1), np.int64), np.zeros(5), 0.5, np.zeros(5, dtype=bool)):
        with pytest.raises(TypeError):
            bare.query_batch(qn, qp, 3, 1, tags=bad)
    for bad in ("some", "ANY", 1, None):
        with pytest.raises(ValueError, match="tags_mode"):
            bare.query_batch(qn, qp, 3, 1, tags=1, tags_mode=bad)
        with pytest.raises(ValueError, match="tags_mode"):
            bare.query_batch_dev(0, 0, 0, 5, 3, 1, 0, tags_ptr=64, tags_mode=bad)
    with pytest.raises(ValueError):
        bare.set_tags(np.zeros(N0 + 1, dtype=np.uint64))
    with pytest.raises(TypeError):
        bare.set_tags(np.zeros(N0))
    bare.world = 2
    with pytest.raises(RuntimeError, match="list-sharded"):
        bare.set_tags(np.zeros(N0, dtype=np.uint64))
    bare.world = 1
    ivf = IVF("euclidean", 3, None)
    ivf._dev = bare
    ivf.data = np.zeros((N0, D), np.float32)
    with pytest.raises(NotImplementedError, match="tags"):
        ivf.query_batch(qn, 3, fast=True, tags=1)
    with pytest.raises(ValueError, match="tags_mode"):
        ivf.query_batch(qn, 3, tags=1, tags_mode="both")
    with pytest.raises(ValueError, match="one entry per query"):
        ivf.query_batch(qn, 3, tags=np.arange(4))


# ---- the ABI and the kernels ----

def test_new_symbols_declared_and_exported():
    from tinyknn_amd import _lib
    header = open(os.path.join(ROOT, "include", "tinyknn_hip.h")).read()
    declared = set(re.findall(r"\b(tk_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("tk_index_set_tags", "tk_index_tags", "tk_index_tag_table", "tk_index_query_batch_ex4",
                 "tk_index_query_batch_dev_ex4"):
        assert name in declared, name
        assert hasattr(lib, name), f"{name} declared but not exported"
        assert name in _lib.SIGNATURES, name
    # _ex3 plus the tag array and the mode; the earlier entry points keep their signatures
    assert len(_lib.SIGNATURES["tk_index_query_batch_ex4"][1]) == len(_lib.SIGNATURES["tk_index_query_batch_ex3"][1]) + 2
    assert len(_lib.SIGNATURES["tk_index_query_batch_dev_ex4"][1]) == \
        len(_lib.SIGNATURES["tk_index_query_batch_dev_ex3"][1]) + 2
    assert len(_lib.SIGNATURES["tk_index_query_batch_ex3"][1]) == len(_lib.SIGNATURES["tk_index_query_batch_ex2"][1]) + 1
    # without a GPU no index exists to refuse anything: a null index is an argument error, nothing more
    assert lib.tk_index_set_tags(None, None, 0) == -1
    assert lib.tk_index_tags(None) == -1
    assert lib.tk_index_tag_table(None, None) == -1


def test_tags_kernels_compile_without_scratch_or_spills():
    usage = kernel_usage("tags.hip")
    names = " ".join(usage)
    assert "tag_table_kernel" in names, names
    passes = [n for n in usage if "tag_pass_kernel" in n]
    assert len(passes) == 4, names                  # signed or not, any or all
    for name, u in usage.items():
        assert u["ScratchSize"] == 0, (name, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (name, u)
    print({n: usage[n] for n in passes})


# ---- what keeps the GPU tests honest, on the reference alone ----

def _answers(oracle, ox, qn, tags, masks, mode, k, n_probes):
    return tagged_batch(oracle, ox, qn, masks, mode, tags, k, n_probes)


def _honest(want, base, k, what):
    n = (want != -1).sum(axis=1)
    assert (want != base).any(axis=1).any(), f"{what}: no restricted answer differs from the unrestricted one"
    assert (n < k).any(), f"{what}: no query returns fewer than k ids"
    assert (n == k).any(), f"{what}: no query returns all k ids"


@pytest.mark.parametrize("tag", G6_TAGS)
def test_fixture_inputs_can_tell_a_wrong_pass(oracle, tag):
    """every (fixture, assignment, mode) of test_fixtures_every_probe_count_assignment_and_mode, at every probe count it
    runs: answers differ from the unrestricted ones, some are short, some full; and at one probe count at least, the
    expected answer changes when tags and masks are cut to their low words"""
    ox, qn, ids, N = _fixture(oracle, tag)
    for a, (name, tags) in enumerate(ts.assignments(ids, N, 3).items()):
        for mode in ts.MODES:
            cut = False
            for n_probes in (1, 2, 5, 10):
                masks = ts.query_masks(tags, len(qn), 10 * n_probes + a)
                want = _answers(oracle, ox, qn, tags, masks, mode, 10, n_probes)
                base = guarded_batch(oracle, ox, qn, 10, n_probes)
                _honest(want, base, 10, (tag, name, mode, n_probes))
                low = _answers(oracle, ox, qn, ts.low_words(tags), ts.low_words(masks), mode, 10, n_probes)
                cut = cut or bool((low != want).any())
            assert cut, f"{tag} {name} {mode}: a 32-bit compare would pass"


@pytest.mark.parametrize("kp", [1, 2])
def test_synthetic_inputs_can_tell_a_wrong_pass(oracle, kp):
    ivf, qs, tags, emptied, cut = ts.synthetic(kp)
    ox = oracle_index(oracle, ivf, ivf.data)
    qn = ivf._prepare(qs.copy())[0]
    base, bd = guarded_batch(oracle, ox, qn, 10, 10, debug=True)
    probed = np.unique(bd["probes"])
    assert emptied in probed and cut in probed, (emptied, cut)      # the empty list and the list of one whole chunk are probed
    for mode in ts.MODES:
        masks = ts.synthetic_masks(tags, mode)
        want = _answers(oracle, ox, qn, tags, masks, mode, 10, 10)
        _honest(want, base, 10, (kp, mode))
        low = _answers(oracle, ox, qn, ts.low_words(tags), ts.low_words(masks), mode, 10, 10)
        assert (low != want).any(), (kp, mode)
