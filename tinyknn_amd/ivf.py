"""IVF with the reference's API (tinyknn/ivf.py); queries run on the MI355X.

fit / build are offline host code with the reference's semantics.  After build the
index (PQ codebook, coded coarse centres, inverted lists, ids, rescoring vectors)
is uploaded once into HBM (`DeviceIndex`); `query` and `query_batch` then run the
kernel pipeline of libtinyknn_hip.so: distance tables -> coarse scan + heap +
rescoring -> probed-list scan -> exact heap replay -> exact rescoring.
"""
import collections
import ctypes as C
import time
import warnings
import weakref

import numpy as np

from . import _front, _lib
from . import fast_pq as _fp
from ._transform import transform_data, unpack
from .fast_pq import FastPQ, TransformedData, avx, dpad
from .utils import group_data_by_indices, knn_brute, timer


def synth_rows(n, d, seed, centres=None, sigma=1.0, row0=0):
    """Rows [row0, row0 + n) of the seeded device generator (devbuild.hip synth_rows_kernel:
    a pure function of (seed, row)), copied to the host — the vectors IVF.build_resident
    generates in HBM, e.g. to fit centres on a sample or to draw queries."""
    out = np.zeros((n, d), dtype=np.float32)
    c = None if centres is None else np.ascontiguousarray(centres, dtype=np.float32)
    _lib.check(_lib.lib().tk_synth_rows(_lib.ptr(out, _lib._f32p), int(row0), int(n), int(d), int(seed),
                                        None if c is None else c.ctypes.data,
                                        0 if c is None else len(c), float(sigma)))
    return out


class QueryStream:
    """Streaming session on a DeviceIndex (C ABI: tk_stream_*): raw float32 queries on the
    host in, ids on the host out, batch after batch; the exact host preparation
    (ivf.py:125-128 through numpy's own BLAS, see _front.py), the copies and the kernels of
    consecutive batches overlap.  submit() returns a ticket; the ids land in the array given
    to submit() by wait(ticket) / drain()."""

    def __init__(self, dev, max_nq, k, n_probes, pass_1=None, slots=8):
        if not _front.bind():
            raise _lib.TinyKnnHipError("no BLAS bound for the exact host front end: " +
                                       str(_front.info()["why"]))
        self._dev = dev                 # keeps the index alive
        dev._live_streams.add(self)     # ... and the index closes its sessions before it goes
        self.max_nq, self.k = int(max_nq), int(k)
        R = dev._R
        self._s = _lib.lib().tk_stream_create(
            dev.handle, self.max_nq, self.k, int(n_probes), int(pass_1 or 0), int(dev.angular),
            None if R is None else R.ctypes.data, 0 if R is None else R.shape[1], int(slots))
        if not self._s:
            raise _lib.TinyKnnHipError(_lib.lib().tk_last_error().decode())
        self._keep = {}

    def submit(self, qs, out):
        """qs (nq, d) float32 C-contiguous raw queries (not modified); out (nq, k) int64."""
        assert qs.dtype == np.float32 and qs.flags.c_contiguous and qs.shape[1] == self._dev.d
        assert out.dtype == np.int64 and out.flags.c_contiguous and out.shape == (len(qs), self.k)
        t = _lib.check(_lib.lib().tk_stream_submit(self._s, qs.ctypes.data, len(qs), out.ctypes.data))
        self._keep[t % 64] = (qs, out)
        return t

    def submit_prepared(self, qn, q_pq, out):
        """Already prepared rows (what DeviceIndex.query_batch takes)."""
        assert qn.dtype == np.float32 and qn.flags.c_contiguous and qn.shape[1] == self._dev.d
        assert out.dtype == np.int64 and out.flags.c_contiguous and out.shape == (len(qn), self.k)
        t = _lib.check(_lib.lib().tk_stream_submit_prepared(
            self._s, qn.ctypes.data, None if q_pq is None else q_pq.ctypes.data, len(qn),
            out.ctypes.data))
        self._keep[t % 64] = (qn, q_pq, out)
        return t

    def set_probes(self, n_probes, pass_1=None):
        _lib.check(_lib.lib().tk_stream_set_probes(self._s, int(n_probes), int(pass_1 or 0)))

    def wait(self, ticket):
        _lib.check(_lib.lib().tk_stream_wait(self._s, int(ticket)))

    def drain(self):
        _lib.check(_lib.lib().tk_stream_drain(self._s))
        self._keep.clear()

    def prepare_seconds(self):
        return _lib.lib().tk_stream_prepare_seconds(self._s)

    def close(self):
        if getattr(self, "_s", None):
            if _lib.owns_handles():
                _lib.lib().tk_stream_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


STORES = (None, "float32", "float16")
_STORE_NAMES = {_lib.DATA_F32: "float32", _lib.DATA_F64: "float64", _lib.DATA_F16: "float16"}


def check_store(store):
    """The `store=` argument: None (the vectors as they are today: the caller's dtype), "float32" (the same,
    said out loud) or "float16" (the device copy of the rescoring vectors in IEEE half)."""
    if store not in STORES:
        raise ValueError(f"store must be one of {STORES}, got {store!r}")
    return store


def half_rows(X, what, row0=0):
    """X (float32) rounded to IEEE half as the device stores it: numpy's astype (round-to-nearest-even,
    subnormals kept).  ValueError naming the first row with a value whose half is not finite (|x| >= 65520,
    inf, NaN), or for float64 vectors — those callers asked for float64 rescoring."""
    X = np.asarray(X)
    if X.dtype != np.float32:
        raise ValueError(f"{what}: store=\"float16\" takes float32 vectors, got {X.dtype} "
                         "(float64 vectors are rescored in float64)")
    bad = ~(np.abs(X) < np.float32(65520.0))
    if bad.any():
        row = int(np.argmax(bad.reshape(len(X), -1).any(axis=1)))
        raise ValueError(f"{what}: half storage: row {row0 + row} holds a value whose half is not finite "
                         "(|x| >= 65520, inf or NaN)")
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(X).astype(np.float16)


def _half_refusal(call, *args):
    """The library's refusal of a row whose half is not finite (TK_ERR_ARG) as the ValueError the host checks raise."""
    try:
        return _lib.check(call(*args))
    except AssertionError as e:
        if "half is not finite" in str(e):
            raise ValueError(str(e)) from None
        raise


class ResidentData:
    """Stands where IVF.data stood when the vectors live in HBM only (IVF.build_resident):
    shape, dtype and rows by id (tk_index_read_rows).  dtype stays float32 for a half store (`store`):
    rows come back widened."""

    def __init__(self, dev):
        self._dev = dev
        self.shape = (dev.N, dev.d)
        self.dtype = np.dtype(np.float32)
        self.store = dev.store

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, rows):
        rows = np.asarray(rows, dtype=np.int64)
        return self._dev.read_rows(rows).reshape(rows.shape + (self.shape[1],))


def _mask_or_ids(arg, N, what, takes):
    """(True, the bool mask of length N) or (False, the int64 row ids, all in [0, N), duplicates allowed) that `arg` is;
    `what` and `takes` word the refusals."""
    a = np.asarray(arg)
    if a.dtype == np.bool_:
        if a.shape != (N,):
            raise ValueError(f"{what}: a bool mask must have shape ({N},), got {a.shape}")
        return True, a
    if a.ndim == 1 and (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
        a = np.ascontiguousarray(a, dtype=np.int64)
        if a.size and (a.min() < 0 or a.max() >= N):
            raise ValueError(f"{what}: row ids must lie in [0, {N})")
        return False, a
    raise TypeError(f"{what}: {takes}")


def removal_rows(ids_or_mask, N):
    """int64 row ids of remove()'s argument: a bool mask of length N, or a 1-d integer array of ids in [0, N)
    (duplicates allowed)."""
    is_mask, a = _mask_or_ids(ids_or_mask, N, "remove", "a bool mask of length N or a 1-d integer array of row ids")
    return np.ascontiguousarray(np.flatnonzero(a), dtype=np.int64) if is_mask else a


def update_ids(ids, N):
    """int64 row ids of update()'s argument: a 1-d integer array of ids in [0, N), pairwise distinct (TypeError for
    another kind of value — a bool mask names no order —, ValueError for an id outside or named twice)."""
    is_mask, a = _mask_or_ids(ids, N, "update", "a 1-d integer array of row ids")
    if is_mask:
        raise TypeError("update: a 1-d integer array of row ids (a mask does not say which row takes which vector)")
    if len(np.unique(a)) != len(a):
        raise ValueError("update: row ids must be pairwise distinct")
    return a


def group_ids(groups, n, what):
    """The int32 group ids a `groups` argument is: a 1-d integer array of length n, every id in [0, 2**31 - 1)
    (TypeError for another kind of value, ValueError for another length or an id outside)."""
    a = np.asarray(groups)
    if a.ndim != 1 or a.dtype == np.bool_ or not (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
        raise TypeError(f"{what}: a 1-d integer array, one group id per row")
    if a.shape[0] != n:
        raise ValueError(f"{what}: one group id per row ({n}), got {a.shape[0]}")
    if a.size and (a.min() < 0 or a.max() >= 2**31 - 1):
        raise ValueError(f"{what}: group ids must lie in [0, 2**31 - 1)")
    return np.ascontiguousarray(a, dtype=np.int32)


def exact_below_parts(routed, between):
    """The parts a batch is split into by query_batch(exact_below=): [(exact?, query rows ascending, that part's
    between=)], the exact part (routed: bool per query) first, an empty part left out.  between: None, or (lo, hi) with
    each end None or (nq, C) (_bound_array's form, which a part of any size keeps unambiguous), cut to the part's rows."""
    routed = np.asarray(routed, dtype=bool)
    parts = []
    for exact, rows in ((True, np.flatnonzero(routed)), (False, np.flatnonzero(~routed))):
        if len(rows):
            parts.append((exact, rows, None if between is None else
                          tuple(None if b is None else np.asarray(b)[rows] for b in between)))
    return parts


def query_groups(group, nq):
    """The int32 array a `group=` argument is: an int for every query, or a 1-d integer array with one entry per
    query; each a group id or -1 (unrestricted)."""
    a = np.asarray(group)
    if a.dtype == np.bool_ or not (a.size == 0 or np.issubdtype(a.dtype, np.integer)) or a.ndim > 1:
        raise TypeError("group: an int, or a 1-d integer array with one group id (or -1) per query")
    if a.ndim == 0:
        a = np.full(nq, a[()])
    if a.shape[0] != nq:
        raise ValueError(f"group: one entry per query ({nq}), got {a.shape[0]}")
    if a.size and (a.min() < -1 or a.max() >= 2**31 - 1):
        raise ValueError("group: entries must be a group id in [0, 2**31 - 1) or -1")
    return np.ascontiguousarray(a, dtype=np.int32)


def query_caps(per_group, nq):
    """The int32 array a `per_group=` argument is: a non-negative int for every query, or a 1-d integer array with one
    entry per query; each the most rows of any one group the query may return, 0 for no cap."""
    a = np.asarray(per_group)
    if a.dtype == np.bool_ or not (a.size == 0 or np.issubdtype(a.dtype, np.integer)) or a.ndim > 1:
        raise TypeError("per_group: an int, or a 1-d integer array with one count (or 0) per query")
    if a.ndim == 0:
        a = np.full(nq, a[()])
    if a.shape[0] != nq:
        raise ValueError(f"per_group: one entry per query ({nq}), got {a.shape[0]}")
    if a.size and (a.min() < 0 or a.max() > 2**31 - 1):
        raise ValueError("per_group: entries must be a count in [0, 2**31 - 1], 0 for no cap")
    return np.ascontiguousarray(a, dtype=np.int32)


def _u64(a):
    """the integer array `a` as uint64 where every value lies in [0, 2**64), else None"""
    if a.dtype == np.uint64:
        return np.ascontiguousarray(a)
    if a.size == 0:
        return np.zeros(a.shape, dtype=np.uint64)
    if a.dtype == object:           # (Python ints beyond int64 among smaller ones)
        if not all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in a.flat):
            return None
        if min(a.flat) < 0 or max(a.flat) >= 2**64:
            return None
        return np.array([int(v) for v in a.flat], dtype=np.uint64).reshape(a.shape)
    if a.min() < 0:
        return None
    return np.ascontiguousarray(a, dtype=np.uint64)


def _mask_array(x):
    """np.asarray(x) — a sequence of Python ints that numpy would make floats of (values on both sides of 2**63) as objects"""
    a = np.asarray(x)
    if a.dtype.kind == "f" and not isinstance(x, np.ndarray) and a.ndim == 1 and \
            all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in x):
        a = np.asarray(x, dtype=object)
    return a


def tag_masks(tags, n, what):
    """The uint64 tag masks a `tags` argument is: a 1-d integer array of length n, uint64 or any integer dtype with
    every value in [0, 2**64) (TypeError for another kind of value, ValueError for another length or a value outside)."""
    a = _mask_array(tags)
    integral = a.size == 0 or np.issubdtype(a.dtype, np.integer) or a.dtype == object
    if a.ndim != 1 or a.dtype == np.bool_ or not integral:
        raise TypeError(f"{what}: a 1-d integer array, one tag mask per row")
    if a.shape[0] != n:
        raise ValueError(f"{what}: one tag mask per row ({n}), got {a.shape[0]}")
    u = _u64(a)
    if u is None:
        if a.dtype == object and not all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
                                         for v in a.flat):
            raise TypeError(f"{what}: a 1-d integer array, one tag mask per row")
        raise ValueError(f"{what}: tag masks must lie in [0, 2**64)")
    return u


TAG_MODES = {"any": 0, "all": 1}


def join_radius_parts(nq, chunk, max_results, part):
    """The CSR result of a radius call made in parts of at most `chunk` queries.  part(o, e, limit) answers queries
    [o, e): (lims, fetch) — lims (e - o + 1,) int64 from 0; fetch() -> (ids, dist) while the device still holds the
    part, or None where the part was only counted (limit None, or its total above limit) — or None where the part is
    too large for the device's work memory: it is asked again in halves.  max_results None: counts alone.  The limit
    holds for the sum and is checked before any part is fetched: a call of several parts counts them all first (the
    device holds one result at a time), then asks each again for its rows; a call of one part is checked by the part
    itself.  Above the limit: ValueError naming the true total, nothing returned."""
    lims = np.zeros(nq + 1, dtype=np.int64)

    def walk(spans, limit_of):
        """every span in order, halved where it is too large -> (the spans as answered, their fetches)"""
        todo, done, fetches = spans[::-1], [], []
        while todo:
            o, e = todo.pop()
            got = part(o, e, limit_of(o))
            if got is None:
                if e - o <= 1:
                    raise MemoryError("radius_search(n_probes=): one query's candidate bitmap exceeds the workspace "
                                      "budget")
                mid = (o + e) // 2
                todo += [(mid, e), (o, mid)]
                continue
            lims[o + 1:e + 1] = lims[o] + got[0][1:]
            done.append((o, e))
            fetches.append(None if got[1] is None else got[1]())
        return done, fetches

    def refuse():
        raise ValueError(f"radius_search: {int(lims[nq])} rows lie within the radii, more than max_results = "
                         f"{max_results}; nothing is returned (raise max_results, or ask radius_count first)")

    spans = [(o, min(o + chunk, nq)) for o in range(0, nq, chunk)] if nq > 0 else [(0, 0)]
    if max_results is not None and len(spans) == 1:
        got = part(*spans[0], max_results)                      # one part: its own check
        if got is not None:
            lims[1:] = got[0][1:]
            if got[1] is None:
                refuse()
            return (lims,) + tuple(got[1]())
    spans, _ = walk(spans, lambda o: None)                      # the counts alone (a part too large goes in halves)
    if max_results is None:
        return lims, None, None
    if lims[nq] > max_results:
        refuse()
    _, fetches = walk(spans, lambda o: max_results - int(lims[o]))
    if any(f is None for f in fetches):
        refuse()
    return lims, np.concatenate([f[0] for f in fetches]), np.concatenate([f[1] for f in fetches])


def query_radius(radius, nq):
    """The float32 array a `radius=` argument is: a scalar for every query, or one radius per query, cast with
    np.float32; +inf and negative values are allowed, NaN and a wrong length are a ValueError."""
    a = np.asarray(radius)
    if a.dtype == np.bool_ or a.dtype == object or not np.issubdtype(a.dtype, np.number) or a.ndim > 1:
        raise TypeError("radius: a number, or a 1-d array with one radius per query")
    if np.iscomplexobj(a):
        raise TypeError("radius: a number, or a 1-d array with one radius per query")
    if a.ndim == 0:
        a = np.full(nq, a[()])
    if a.shape[0] != nq:
        raise ValueError(f"radius: one entry per query ({nq}), got {a.shape[0]}")
    with np.errstate(over="ignore"):
        a = np.ascontiguousarray(a.astype(np.float32))
    if np.isnan(a).any():
        raise ValueError(f"radius: query {int(np.flatnonzero(np.isnan(a))[0])} has a NaN radius")
    return a


def tag_mode_of(tags_mode):
    """0 / 1 for tags_mode "any" / "all" (ValueError for anything else)"""
    if not isinstance(tags_mode, str) or tags_mode not in TAG_MODES:
        raise ValueError(f"tags_mode: \"any\" or \"all\", got {tags_mode!r}")
    return TAG_MODES[tags_mode]


def query_tags(tags, nq):
    """The uint64 array a `tags=` argument is: an int for every query, or a 1-d integer array with one mask per query;
    each in [0, 2**64), 0 for an unrestricted query."""
    a = _mask_array(tags)
    integral = a.size == 0 or np.issubdtype(a.dtype, np.integer) or a.dtype == object
    if a.dtype == np.bool_ or not integral or a.ndim > 1:
        raise TypeError("tags: an int, or a 1-d integer array with one tag mask (or 0) per query")
    if a.ndim == 0:
        a = np.full(nq, a[()], dtype=a.dtype)
    if a.shape[0] != nq:
        raise ValueError(f"tags: one entry per query ({nq}), got {a.shape[0]}")
    u = _u64(a)
    if u is None:
        raise ValueError("tags: entries must be a tag mask in [0, 2**64)")
    return u


INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


def value_kind(dtype):
    """"i" / "f": the kind of value column a dtype makes (TypeError for anything but integers and floats)"""
    dtype = np.dtype(dtype)
    if dtype.kind in "iu":
        return "i"
    if dtype.kind == "f" and dtype.itemsize <= 8:
        return "f"
    raise TypeError(f"values: an integer or floating dtype (float16 / 32 / 64), got {dtype}")


def _float_keys(x):
    """float64 array -> int64 keys, strictly monotone over the finite values and +-inf (the caller refused NaN):
    -0.0 folded into +0.0, then the bits b where b >= 0, else b ^ 0x7FFFFFFFFFFFFFFF"""
    b = (np.ascontiguousarray(x, dtype=np.float64) + 0.0).view(np.int64)
    return np.where(b >= 0, b, b ^ np.int64(INT64_MAX))


def value_keys(values, n, what):
    """The int64 keys the device compares for a `values` argument, in its shape: a (n,) or (n, C) array, 1 <= C <= 4,
    of ONE integer or floating dtype (n None: any length).  Integers: the key is int64(v); uint64 values above
    2**63 - 1 raise ValueError.  Floats (float16 / 32 / 64): widened exactly to float64, NaN raises ValueError, -0.0
    is +0.0, then with b = the bits as int64 the key is b if b >= 0 else b ^ 0x7FFFFFFFFFFFFFFF — strictly monotone
    over all finite values and +-inf.  TypeError for another kind of value or shape."""
    a = np.asarray(values)
    if a.dtype == np.bool_ or a.dtype.kind not in "iuf" or a.ndim not in (1, 2):
        raise TypeError(f"{what}: a (n,) or (n, C) array of one integer or floating dtype")
    kind = value_kind(a.dtype)
    if a.ndim == 2 and not 1 <= a.shape[1] <= 4:
        raise ValueError(f"{what}: 1 to 4 columns, got {a.shape[1]}")
    if n is not None and a.shape[0] != n:
        raise ValueError(f"{what}: one row of values per row ({n}), got {a.shape[0]}")
    if kind == "i":
        if a.dtype == np.uint64 and a.size and a.max() > INT64_MAX:
            raise ValueError(f"{what}: uint64 values above 2**63 - 1 have no int64 key")
        return np.ascontiguousarray(a, dtype=np.int64)
    if np.isnan(a).any():
        raise ValueError(f"{what}: NaN has no place in an order")
    return _float_keys(a)


def _bound_array(x, which, nq, cols):
    """One end of `between=` as an (nq, cols) array of its own dtype, or None (unbounded).  The shape rule: a scalar
    is for every query and column; 2-d is (nq, cols); 1-d of length nq is per query where cols == 1; 1-d of length
    cols is per column, for every query, where cols > 1 — unless nq == cols, where it could be either: ValueError."""
    if x is None:
        return None
    a = np.asarray(x)
    if a.dtype == np.bool_ or a.dtype.kind not in "iuf":
        raise TypeError(f"between: {which} must be None, a number or an array of numbers, got dtype {a.dtype}")
    if a.ndim == 0:
        return np.full((nq, cols), a[()], dtype=a.dtype)
    if a.ndim == 2:
        if a.shape != (nq, cols):
            raise ValueError(f"between: {which} must have shape ({nq}, {cols}), got {a.shape}")
        return a
    if a.ndim != 1:
        raise ValueError(f"between: {which} must be a scalar, 1-d or 2-d, got {a.ndim} dimensions")
    if cols == 1:
        if a.shape[0] != nq:
            raise ValueError(f"between: {which}: one entry per query ({nq}), got {a.shape[0]}")
        return a.reshape(nq, 1)
    if a.shape[0] != cols:
        raise ValueError(f"between: {which}: with {cols} columns pass ({nq}, {cols}) or one entry per column, "
                         f"got {a.shape[0]}")
    if nq == cols:
        raise ValueError(f"between: {which}: {cols} entries for {nq} queries of {cols} columns could be per query or "
                         f"per column: pass ({nq}, {cols})")
    return np.broadcast_to(a, (nq, cols))


def _bound_keys(a, kind, low):
    """(keys, empty) of one end's (nq, cols) array on columns of `kind`: the int64 keys, and where no value can pass
    that end (the caller empties the interval there).  NaN raises ValueError."""
    none = INT64_MIN if low else INT64_MAX
    if a is None:
        return none, False
    if a.dtype.kind == "f":
        if np.isnan(a).any():
            raise ValueError("between: a NaN bound")
        if kind == "f":         # (an end that admits every value, -inf below / +inf above, is unbounded)
            return np.where(a == (-np.inf if low else np.inf), none, _float_keys(a)), False
        r = np.ceil(a.astype(np.float64)) if low else np.floor(a.astype(np.float64))
        above, below = r >= 2.0**63, r < -2.0**63          # (beyond every int64: unbounded on one side, empty on the other)
        keys = np.where(above | below, 0, r).astype(np.int64)
        keys = np.where(below if low else above, none, keys)
        return keys, (above if low else below)
    if a.dtype == np.uint64 and a.size and a.max() > INT64_MAX:
        if kind == "i":
            raise ValueError("between: an integer bound above 2**63 - 1")
    if kind == "i":
        return a.astype(np.int64), False
    f = a.astype(np.float64)
    big = np.abs(f) >= 2.0**53          # (below, every integer is a float64)
    if big.any() and any(int(v) != int(w) for v, w in zip(a[big].tolist(), f[big].tolist())):
        raise ValueError("between: an integer bound on floating columns must be exactly representable in float64")
    return _float_keys(f), False


def query_ranges(between, nq, cols, kind):
    """The (nq, cols, 2) int64 keys a `between=` argument is on `cols` columns of `kind` ("i" / "f": value_kind of the
    values that were set): between = (lo, hi), each None (unbounded), a scalar for every query, (nq,) for one column,
    (nq, cols), or (cols,) for every query where nq != cols (_bound_array); both ends inclusive.  Bounds become keys as
    the column's values did (value_keys); None — and -inf for lo, +inf for hi — is INT64_MIN / INT64_MAX.  On integer columns a floating bound is
    ceil'ed (lo) / floor'ed (hi), +-inf is unbounded where it admits everything and empties the interval where it
    admits nothing.  On floating columns an integer bound must be exactly representable in float64.  TypeError for
    another kind of argument, ValueError for a wrong shape, a NaN, or such an integer."""
    if not isinstance(between, (tuple, list)) or len(between) != 2:
        raise TypeError("between: a pair (lo, hi), each None, a number or an array")
    lo, lo_empty = _bound_keys(_bound_array(between[0], "lo", nq, cols), kind, True)
    hi, hi_empty = _bound_keys(_bound_array(between[1], "hi", nq, cols), kind, False)
    out = np.empty((nq, cols, 2), dtype=np.int64)
    out[:, :, 0] = lo
    out[:, :, 1] = hi
    empty = np.broadcast_to(np.logical_or(lo_empty, hi_empty), (nq, cols))
    out[empty] = (1, 0)
    return out


def unbounded_queries(keys):
    """bool (nq,) of query_ranges' (nq, cols, 2) keys: the query bounds no column (every end INT64_MIN / INT64_MAX) —
    what knn_between refuses and query_batch(between=, exact_below=) never routes"""
    keys = np.asarray(keys)
    return ((keys[:, :, 0] == INT64_MIN) & (keys[:, :, 1] == INT64_MAX)).all(axis=1)


def ranges_length(between, cols):
    """The number of queries a `between=` argument speaks for by itself on `cols` columns (_bound_array's shape rule):
    the rows of a 2-d end, the length of a 1-d end of one column; 1 where every end is None, a scalar or per column."""
    if not isinstance(between, (tuple, list)) or len(between) != 2:
        raise TypeError("between: a pair (lo, hi), each None, a number or an array")
    for b in between:
        a = None if b is None else np.asarray(b)
        if a is not None and (a.ndim == 2 or (a.ndim == 1 and cols == 1)):
            return a.shape[0]
    return 1


def host_values(values, n, what, like=None):
    """The host copy of a `values` argument for n rows: the caller's array in its own dtype, checked as the device will
    take it (value_keys).  like (the index's values, for new rows): in its shape and of its kind (ValueError),
    converted to its dtype."""
    a = np.asarray(values)
    value_keys(a, n, what)
    if like is None:
        return a
    if a.shape[1:] != like.shape[1:]:
        raise ValueError(f"{what}: shape (n,) + {like.shape[1:]} as the index's values, got {a.shape}")
    if value_kind(a.dtype) != value_kind(like.dtype):
        raise ValueError(f"{what}: {like.dtype} as the index's values, got {a.dtype}")
    b = a.astype(like.dtype)
    if value_kind(a.dtype) == "i" and a.size and not np.array_equal(b.astype(object), a.astype(object)):
        raise ValueError(f"{what}: values that do not fit the index's {like.dtype}")
    return b


def _value_columns(keys):
    """tk_index_set_values' arguments for value_keys' array: the keys column-major (C, N), N, C"""
    kt = np.ascontiguousarray(keys.reshape(len(keys), -1).T)
    return _lib.ptr(kt, C.c_void_p), kt.shape[1], kt.shape[0]


# The per-row attributes a query can be restricted by (group=, tags=, between=), and what differs between them.
# name: the IVF attribute, the keyword of add / update, the .npz key, the word of the messages, and with `one` the
# library's names (tk_index_set_<name>, the counter tk_index_<name>, the reader tk_index_<one>_table); rows: the parser
# of per-row input -> what the device takes; host: the host copy where it is not that (values: the caller's array);
# dtype: the host copy's (None: the caller's); upload / clear: tk_index_set_<name>'s arguments behind the handle.
RowAttr = collections.namedtuple("RowAttr", "name one rows host dtype upload clear")
ROW_ATTRS = GROUPS, TAGS, VALUES = (
    RowAttr("groups", "group", group_ids, None, np.int32, lambda g: (_lib.ptr(g, _lib._i32p), len(g)), (None, 0)),
    RowAttr("tags", "tag", tag_masks, None, np.uint64, lambda t: (_lib.ptr(t, C.c_void_p), len(t)), (None, 0)),
    RowAttr("values", "value", value_keys, host_values, None, _value_columns, (None, 0, 0)),
)


def _stored(t):
    """Stored rows of one list's codes: a TransformedData, or the raw empty array FastPQ.transform returns for no rows."""
    return 0 if isinstance(t, np.ndarray) else t.size


def _split_lists(sizes, codes, ids, d):
    """Lists concatenated list-major (save's and export_lists' form) as per-list objects -> (codes per list as
    FastPQ.transform gives them for vectors of d dimensions, ids per list)."""
    coff = np.concatenate([[0], np.cumsum((sizes + 15) // 16)])
    ioff = np.concatenate([[0], np.cumsum(sizes)])
    pts = [TransformedData(int(sizes[i]), codes[coff[i]:coff[i + 1]]) if sizes[i] else np.empty((0, d))
           for i in range(len(sizes))]
    return pts, [ids[ioff[i]:ioff[i + 1]] for i in range(len(sizes))]


def _pack_labels(lab, zero):
    """One list's codes from its rows' labels (n, M): the rows that pad it to a multiple of 16 carry the code of the
    zero vector, as pad2 + transform give them (fast_pq.py:165)."""
    n = len(lab)
    if n % 16:
        lab = np.concatenate([lab, np.repeat(zero[None], (-n) % 16, axis=0)])
    return TransformedData(n, transform_data(np.ascontiguousarray(lab, dtype=np.uint8)))


def _dev_is_sharded(dev):
    """Has this device index been list-sharded (uploaded as a rank's shard, or sharded in place)?"""
    return dev.world != 1 or getattr(dev, "_sharded_as", None) is not None


def _copies_carry_one_code(ivf, n_lists):
    """Rows with equal ids lie in different lists and carry equal codes — what IVF.build's lists have by construction
    (ivf.py:77-102) and what the lane replay's TWIN form rests on (heap.hip).  The library checks it on the device
    where it holds every list's codes; a rank of a list-sharded index uploads only its own lists, so this is the
    same check on the host, over all lists, before the rank vouches (TK_OPT_TWIN_VOUCH)."""
    # Two independent multilinear hashes (mod 2^64, fixed odd-seeded multipliers) per row instead of the M / 2 code bytes
    # themselves: 16 B per stored row on every rank at construction, not 3 x M / 2 (a 100M-row build(n_probes=2) index
    # is 200M stored rows).  Unequal codes hash alike with probability < 2^-100.
    labels, lists, sigs = [], [], []
    mult = None
    for i in range(n_lists):
        td = ivf.pq_transformed_points[i]
        if _stored(td) == 0:
            continue
        pk = np.ascontiguousarray(td.packed, dtype=np.uint64)              # (chunks, M): per chunk M / 2 groups of 16 bytes
        P = pk.shape[1] // 2
        if mult is None or mult.shape[0] != P:
            mult = np.random.RandomState(0x7151).randint(0, 2 ** 63, size=(P, 2), dtype=np.int64).astype(np.uint64) * 2 + 1
        h = np.empty((td.size, 2), dtype=np.uint64)
        by = pk.view(np.uint8).reshape(pk.shape[0], P, 16)                 # [chunk][pair][row of the chunk]
        for lo in range(0, pk.shape[0], 4096):                              # (bounded temporaries)
            part = by[lo:lo + 4096].transpose(0, 2, 1).reshape(-1, P)      # rows of these chunks, a code per row
            n = min(part.shape[0], td.size - 16 * lo)
            if n > 0:
                h[16 * lo:16 * lo + n] = part[:n].astype(np.uint64) @ mult
        labels.append(np.asarray(ivf.ids[i], dtype=np.int64)[:td.size])
        lists.append(np.full(td.size, i, dtype=np.int32))
        sigs.append(h)
    if not labels:
        return True
    labels, lists, sigs = np.concatenate(labels), np.concatenate(lists), np.concatenate(sigs)
    order = np.lexsort((lists, labels))
    la, li = labels[order], lists[order]
    same = la[1:] == la[:-1]
    if (same & (li[1:] == li[:-1])).any():          # two copies in one list
        return False
    del la, li
    sg = sigs[order]
    return bool((sg[1:][same] == sg[:-1][same]).all())


class AllowSet:
    """The rows a query may return (tinyknn_hip.h: tk_allow_create): a bool mask of length N or an array of row
    ids, turned once into a device bitmap over the index's stored rows.  Reuse it across calls; close() frees it
    (after the index's calls still owed have run).  len() = allowed stored rows (a row stored in two lists counts
    twice).  A set belongs to the lists it was made for: once they are set again, queries with it fail."""

    def __init__(self, dev, ids_or_mask):
        info = np.zeros(8, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_info(dev.handle, _lib.ptr(info, _lib._i64p)))
        N = int(info[6])
        mask = self.mask_of(ids_or_mask, N)
        self._dev = dev
        h = C.c_void_p()
        _lib.check(_lib.lib().tk_allow_create(dev.handle, _lib.ptr(mask, _lib._u8p), N, C.byref(h)))
        self._h = h.value

    @staticmethod
    def mask_of(ids_or_mask, N):
        """uint8 (N,) mask of a bool mask of length N or of an array of row ids in [0, N)"""
        is_mask, a = _mask_or_ids(ids_or_mask, N, "allowed",
                                  "a bool mask of length N, a 1-d integer array of row ids, or an AllowSet")
        if is_mask:
            return np.ascontiguousarray(a, dtype=np.uint8)
        mask = np.zeros(N, dtype=np.uint8)
        mask[a] = 1
        return mask

    @property
    def handle(self):
        if not self._h:
            raise ValueError("allowed set is closed")
        return self._h

    def __len__(self):
        return int(_lib.check(_lib.lib().tk_allow_count(self.handle)))

    def close(self):
        if getattr(self, "_h", None):
            if _lib.owns_handles() and getattr(self._dev, "_h", None):
                _lib.check(_lib.lib().tk_allow_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceIndex:
    """HBM-resident copy of a built IVF (C ABI: tk_index_*)."""

    # What an index has however it was made (__init__, resident, clone_shard): these, the containers of _new_state,
    # and the shape its maker sets (dq, dpb, d, n_lists, N, angular, rank, world).
    _h = None               # the library's handle; None once closed
    _R = None               # the PQ's rotation (float64), for the streaming sessions
    _f64 = False            # float64 vectors (rescored in float64)
    _sharded_as = None      # (owner, rank, world) once shard_resident made this index a rank's shard in place
    _source = None          # clone_shard: the index whose arrays this one borrows
    _clones = ()            # ... and the shards cloned from this one
    data_ptr = None         # resident: the device address of the vectors
    _value_kind = None      # set_values: "i" / "f", the kind of the value columns (value_kind); None: no values
    _value_cols = 0         # ... and how many
    list_sizes = None
    code_bytes = 0

    def _new_state(self):
        """the containers every instance owns"""
        self._streams = {}                          # query_raw's sessions, per k
        self._live_streams = weakref.WeakSet()      # every open session, the callers' included
        self._live_allows = weakref.WeakSet()
        self._clones = weakref.WeakSet()

    @property
    def M(self):
        """PQ blocks = bytes per code"""
        return self.dq // self.dpb

    def __init__(self, ivf, owner=None, rank=0, world=1, store=None):
        """owner (n_lists,) int32 + rank/world: list-sharded index — only the codes of the
        lists with owner[l] == rank are uploaded (tinyknn_hip.h, tk_index_set_lists_shard).
        store: None = ivf.store; "float16": the vectors are rounded to half here and only the halfs are
        uploaded (ValueError for a value whose half is not finite, or float64 vectors)."""
        L = _lib.lib()
        store = check_store(store) or getattr(ivf, "store", None)
        half = half_rows(ivf.data, "DeviceIndex") if store == "float16" else None      # (refused before anything is made)
        pq = ivf.pq
        self._new_state()
        self._h = L.tk_index_create()
        if not self._h:
            raise _lib.TinyKnnHipError(L.tk_last_error().decode() or "tk_index_create failed")
        centers = pq.centers
        f_order = int(not centers.flags.c_contiguous)
        c32 = np.ascontiguousarray(centers, dtype=np.float32)
        self.dq = c32.shape[1]
        self.dpb = pq.dims_per_block
        order = _lib.ORDER_AVX if avx else _lib.ORDER_SSE
        _lib.check(L.tk_index_set_pq(self._h, _lib.ptr(c32, _lib._f32p), self.dq, self.dpb,
                                     f_order, float(pq.sqrt_n_blocks), order))
        ac = np.ascontiguousarray(ivf.active_centers, dtype=np.float32)
        self.n_lists, self.d = ac.shape
        csize, cpacked = ivf.pq_transformed_centers
        assert csize == self.n_lists
        cpacked = np.ascontiguousarray(cpacked, dtype=np.uint64)
        _lib.check(L.tk_index_set_centers(self._h, _lib.ptr(ac, _lib._f32p), self.n_lists, self.d,
                                          _lib.ptr(cpacked, _lib._u64p), cpacked.shape[0]))
        sizes, packed, ids = [], [], []
        for i in range(self.n_lists):
            td = ivf.pq_transformed_points[i]
            sizes.append(_stored(td))
            if sizes[-1] == 0:
                continue
            if owner is None or owner[i] == rank:
                packed.append(np.ascontiguousarray(td.packed, dtype=np.uint64))
            ids.append(np.asarray(ivf.ids[i], dtype=np.int64)[:td.size])
        sizes = np.array(sizes, dtype=np.int64)
        codes = (np.ascontiguousarray(np.concatenate(packed)) if packed
                 else np.zeros((1, self.M), dtype=np.uint64))
        allids = (np.ascontiguousarray(np.concatenate(ids)) if ids else np.zeros(1, np.int64))
        self.list_sizes = sizes
        self.rank, self.world = int(rank), int(world)
        if owner is None:
            _lib.check(L.tk_index_set_lists(self._h, _lib.ptr(sizes, _lib._i64p),
                                            _lib.ptr(codes, _lib._u64p),
                                            _lib.ptr(allids, _lib._i64p)))
        else:
            own = np.ascontiguousarray(owner, dtype=np.int32)
            assert own.shape == (self.n_lists,)
            _lib.check(L.tk_index_set_lists_shard(self._h, _lib.ptr(sizes, _lib._i64p),
                                                  _lib.ptr(own, _lib._i32p), self.rank,
                                                  self.world, _lib.ptr(codes, _lib._u64p),
                                                  _lib.ptr(allids, _lib._i64p)))
        # IVF.data keeps the dtype of the X passed to build (ivf.py:77); float64 vectors
        # are rescored in float64 like numpy would
        is64 = ivf.data.dtype != np.float32
        if half is not None:
            data = half
            _lib.check(L.tk_index_set_data(self._h, data.ctypes.data, _lib.DATA_F16, data.shape[0], data.shape[1]))
        else:
            data = np.ascontiguousarray(ivf.data, dtype=np.float64 if is64 else np.float32)
            _lib.check(L.tk_index_set_data(self._h, data.ctypes.data, int(is64), data.shape[0],
                                           data.shape[1]))
        self._f64 = bool(is64)
        self.N = int(data.shape[0])
        self.code_bytes = int(codes.nbytes)
        self.angular = ivf.metric == "angular"
        if pq.R is not None:    # fast mode (device front end) needs the rotation on the device
            R = np.ascontiguousarray(pq.R, dtype=np.float64)
            _lib.check(L.tk_index_set_rotation(self._h, R.ctypes.data, R.shape[1]))
            self._R = R
        # labels that repeat on a list-sharded rank: the library cannot check the twin table's premises against codes
        # it was not given — the host can (all lists are here), and vouches
        if owner is not None and self.twin_table_width() > 0 and _copies_carry_one_code(ivf, self.n_lists):
            self.set_option(_lib.OPT_TWIN_VOUCH, 1)

    @classmethod
    def resident(cls, ivf, N, d):
        """An index whose N float32 vectors are produced IN HBM and never visit the host
        (tk_index_alloc_data; filled by synth_data or through `data_ptr`, then build_dev)."""
        L = _lib.lib()
        pq = ivf.pq
        self = cls.__new__(cls)
        self._new_state()
        self._h = L.tk_index_create()
        if not self._h:
            raise _lib.TinyKnnHipError(L.tk_last_error().decode() or "tk_index_create failed")
        c32 = np.ascontiguousarray(pq.centers, dtype=np.float32)
        self.dq, self.dpb = c32.shape[1], pq.dims_per_block
        _lib.check(L.tk_index_set_pq(self._h, _lib.ptr(c32, _lib._f32p), self.dq, self.dpb,
                                     int(not pq.centers.flags.c_contiguous), float(pq.sqrt_n_blocks),
                                     _lib.ORDER_AVX if avx else _lib.ORDER_SSE))
        self.data_ptr = L.tk_index_alloc_data(self._h, int(N), int(d))
        if not self.data_ptr:
            raise _lib.TinyKnnHipError(L.tk_last_error().decode() or "tk_index_alloc_data failed")
        self.N, self.d, self.n_lists = int(N), int(d), 0
        self.rank, self.world = 0, 1
        self.angular = ivf.metric == "angular"
        self._R = None if pq.R is None else np.ascontiguousarray(pq.R, dtype=np.float64)
        return self

    @property
    def store(self):
        """How the rescoring vectors sit in HBM: "float32", "float64" or "float16" (tk_index_store)."""
        return _STORE_NAMES.get(_lib.lib().tk_index_store(self._h))

    @property
    def vector_bytes(self):
        """Bytes of the rescoring vectors in HBM: N * d * the stored element's size."""
        return self.N * self.d * {"float64": 8, "float16": 2}.get(self.store, 4)

    def narrow(self):
        """The float32 vectors this index holds in HBM become halfs (tk_index_narrow_data): checked first
        (ValueError naming the first row with a value whose half is not finite; the index stays float32),
        converted into a new buffer, the float32 one freed.  Nothing to do on a half index."""
        _half_refusal(_lib.lib().tk_index_narrow_data, self._h)

    def synth_data(self, seed, centres=None, sigma=1.0, row0=0, n=None):
        """rows [row0, row0 + n) = centres[c(row)] + sigma * N(0, 1) from the seeded
        counter-based generator (devbuild.hip): a pure function of (seed, row)."""
        n = self.N - row0 if n is None else n
        c = None if centres is None else np.ascontiguousarray(centres, dtype=np.float32)
        _lib.check(_lib.lib().tk_index_synth_data(
            self._h, int(row0), int(n), int(seed), None if c is None else c.ctypes.data,
            0 if c is None else len(c), float(sigma)))

    def build_dev(self, all_centers, n_probes=1):
        """IVF.build(n_probes=1 or 2) on the resident vectors (tk_index_build_dev) -> n_active."""
        A, Y, ynorm2 = self._search_centres(all_centers)
        n_active = C.c_int64(0)
        R = self._R
        _lib.check(_lib.lib().tk_index_build_dev(
            self._h, int(self.angular), _lib.ptr(A, _lib._f32p), _lib.ptr(Y, _lib._f32p),
            _lib.ptr(ynorm2, _lib._f32p), len(Y), int(n_probes),
            None if R is None else R.ctypes.data, 0 if R is None else R.shape[1], C.byref(n_active)))
        self.n_lists = int(n_active.value)
        self._refresh_lists()
        return self.n_lists

    def _search_centres(self, all_centers):
        """(all_centers as float32, the centres the assignment searches — normalised for angular —, their squared norms)"""
        A = np.ascontiguousarray(all_centers, dtype=np.float32)
        Y = A
        if self.angular:
            Y = np.ascontiguousarray(Y / np.linalg.norm(Y, axis=1, keepdims=True))   # utils.py:75
        return A, Y, np.ascontiguousarray(np.einsum("ij,ij->i", Y, Y))    # utils.py:80

    def _refresh_lists(self):
        """The host's view of lists that changed on the device: N, the list sizes, the bytes of their codes."""
        info = np.zeros(8, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_info(self._h, _lib.ptr(info, _lib._i64p)))
        self.N = int(info[6])
        self.list_sizes = self.export_lists(codes=False, ids=False)[0]
        self.code_bytes = int(((self.list_sizes + 15) // 16).sum()) * self.M * 8

    def shard_resident(self, owner, rank, world):
        """This complete index becomes rank `rank`'s shard of a list-sharded index, in place
        (tk_index_shard_resident): only the codes of the lists it owns stay in HBM."""
        own = np.ascontiguousarray(owner, dtype=np.int32)
        assert own.shape == (self.n_lists,)
        prev = self._sharded_as
        if prev is not None:        # a second ListShardedIndex on the same IVF: same partition only
            if prev[1:] == (int(rank), int(world)) and np.array_equal(prev[0], own):
                return
            raise RuntimeError("this index is already list-sharded in place with another partition")
        _lib.check(_lib.lib().tk_index_shard_resident(self._h, _lib.ptr(own, _lib._i32p), int(rank), int(world)))
        self.rank, self.world = int(rank), int(world)
        self._sharded_as = (own.copy(), int(rank), int(world))

    def export_lists(self, codes=True, ids=True):
        """(list_sizes, packed codes (chunks, M) uint64 or None, ids or None) back on the host
        in the reference's formats (tk_index_export_lists)."""
        L = _lib.lib()
        sizes = np.zeros(self.n_lists, dtype=np.int64)
        _lib.check(L.tk_index_export_lists(self._h, sizes.ctypes.data, None, None))
        pk = np.zeros((int(((sizes + 15) // 16).sum()), self.M), dtype=np.uint64) if codes else None
        lab = np.zeros(int(sizes.sum()), dtype=np.int64) if ids else None
        if codes or ids:
            _lib.check(L.tk_index_export_lists(self._h, None, None if pk is None else pk.ctypes.data,
                                               None if lab is None else lab.ctypes.data))
        return sizes, pk, lab

    def export_centers(self):
        """(active_centers (n_lists, d) float32, their packed codes) (tk_index_export_centers)."""
        ac = np.zeros((self.n_lists, self.d), dtype=np.float32)
        cc = np.zeros(((self.n_lists + 15) // 16, self.M), dtype=np.uint64)
        _lib.check(_lib.lib().tk_index_export_centers(self._h, ac.ctypes.data, cc.ctypes.data))
        return ac, cc

    def read_rows(self, rows):
        """IVF.data[rows] for float32 vectors held in HBM, or half vectors widened (tk_index_read_rows)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        out = np.zeros((len(rows), self.d), dtype=np.float32)
        _lib.check(_lib.lib().tk_index_read_rows(self._h, _lib.ptr(rows, _lib._i64p), len(rows),
                                                 _lib.ptr(out, _lib._f32p)))
        return out

    def list_columns(self):
        """(n_lists, kp) int64 members per (list, column of the build's nearest), or None where the index does
        not know them (a host upload; tk_index_list_columns)."""
        kp = C.c_int32(0)
        _lib.check(_lib.lib().tk_index_list_columns(self._h, C.byref(kp), None))
        if kp.value == 0:
            return None
        out = np.zeros((self.n_lists, kp.value), dtype=np.int64)
        _lib.check(_lib.lib().tk_index_list_columns(self._h, C.byref(kp), out.ctypes.data))
        return out

    def add(self, rows, kp, nearest=None, labels=None, list_columns=None, normalise=False, all_centers=None,
            center_codes=None):
        """Append rows (ids N .. N + n - 1) to the built lists in place (tk_index_add_rows) -> n_lists.
        nearest (n, kp) / labels (n, M) / list_columns (n_lists, kp): None = found on the device as the
        device build finds them (all_centers needed) / encoded on the device / the index's own.
        center_codes: packed codes of all_centers[:n_lists'] where the rows activate new centres (None:
        coded on the device).  Batches in flight finish first; allowed sets made before stop working.
        A half index takes float32 rows: assigned and coded from their float32 values, stored rounded
        (ValueError for a row whose half is not finite: nothing changes)."""
        self._lists_may_change("add", "takes no rows")
        is64 = self._f64
        rows = np.ascontiguousarray(rows, dtype=np.float64 if is64 else np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.d:
            raise AssertionError(f"add: rows must have shape (n, {self.d}), got {rows.shape}")
        n, kp = rows.shape[0], int(kp)
        near_p, lab_p, cols_p, cc_p, A, Y, yn, C_, keep = self._new_row_args("add", n, kp, nearest, labels,
                                                                           list_columns, all_centers, center_codes)
        n_active = C.c_int64(0)
        _half_refusal(
            _lib.lib().tk_index_add_rows,
            self._h, rows.ctypes.data, int(is64), n, kp, near_p, lab_p, cols_p, int(bool(normalise)),
            None if A is None else A.ctypes.data, None if Y is None else Y.ctypes.data,
            None if yn is None else yn.ctypes.data, C_, cc_p, C.byref(n_active))
        self.n_lists = int(n_active.value)
        self._refresh_lists()
        return self.n_lists

    def update(self, ids, rows, kp, nearest=None, labels=None, list_columns=None, normalise=False, all_centers=None,
               center_codes=None):
        """Replace the stored rows `ids` (distinct, in [0, N)) by `rows` (n, d) in place, ids kept
        (tk_index_update_rows) -> n_lists: remove(ids) and add(rows) in one pass over the code array, the new
        entries labelled ids[i], their vectors written over rows ids[i]; N and the store's size stay.  The other
        arguments as in add().  Batches in flight finish first, on the old lists and the old vectors; allowed sets
        made before stop working.  ValueError for an id outside [0, N) or named twice, or (a half index) a row
        whose half is not finite; a refused call changes neither the lists nor the vectors."""
        self._lists_may_change("update", "replaces no rows")
        ids = update_ids(ids, self.N)
        is64 = self._f64
        rows = np.ascontiguousarray(rows, dtype=np.float64 if is64 else np.float32)
        if rows.ndim != 2 or rows.shape != (len(ids), self.d):
            raise AssertionError(f"update: rows must have shape ({len(ids)}, {self.d}), got {rows.shape}")
        n, kp = rows.shape[0], int(kp)
        near_p, lab_p, cols_p, cc_p, A, Y, yn, C_, keep = self._new_row_args("update", n, kp, nearest, labels,
                                                                           list_columns, all_centers, center_codes)
        n_active, removed = C.c_int64(0), C.c_int64(0)
        _half_refusal(
            _lib.lib().tk_index_update_rows,
            self._h, ids.ctypes.data, n, rows.ctypes.data, int(is64), kp, near_p, lab_p, cols_p, int(bool(normalise)),
            None if A is None else A.ctypes.data, None if Y is None else Y.ctypes.data,
            None if yn is None else yn.ctypes.data, C_, cc_p, C.byref(n_active), C.byref(removed))
        self.n_lists = int(n_active.value)
        self._refresh_lists()
        return self.n_lists

    def _new_row_args(self, what, n, kp, nearest, labels, list_columns, all_centers, center_codes):
        """The optional arguments add and update share, as the library takes them: the addresses of nearest (n, kp),
        labels (n, M), list_columns (n_lists, kp) and center_codes (None: None), the centres (all_centers, the ones
        the assignment searches, their norms; None: None) and their number, and the arrays to keep alive."""
        keep = []

        def opt(a, dtype, shape=None):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if shape is not None and a.shape != shape:
                raise AssertionError(f"{what}: expected shape {shape}, got {a.shape}")
            keep.append(a)
            return a.ctypes.data

        near_p = opt(nearest, np.int64, (n, kp))
        lab_p = opt(labels, np.uint8, (n, self.M))
        cols_p = opt(list_columns, np.int64, (self.n_lists, kp))
        cc_p = opt(center_codes, np.uint64)
        A = Y = yn = None
        C_ = self.n_lists
        if all_centers is not None:
            A, Y, yn = self._search_centres(all_centers)
            C_ = len(A)
        return near_p, lab_p, cols_p, cc_p, A, Y, yn, C_, keep

    def _lists_may_change(self, what, sharded):
        """The refusals of add / remove / update: a list-sharded index or its clones, an open stream() session (the internal
        sessions of query_raw are closed: made again on demand)."""
        if _dev_is_sharded(self) or self._source is not None:
            raise RuntimeError(f"DeviceIndex.{what}: a list-sharded index {sharded}")
        if any(c._h for c in self._clones):
            raise RuntimeError(f"DeviceIndex.{what}: shards cloned from this index borrow its arrays; close them first")
        for st in list(self._streams.values()):
            st.close()
        self._streams = {}
        if any(getattr(st, "_s", None) for st in self._live_streams):
            raise RuntimeError(f"DeviceIndex.{what}: a stream() session is open on this index; close it first")

    def remove(self, ids_or_mask, list_columns=None):
        """Delete every stored copy of the rows named by ids_or_mask (row ids in [0, N), duplicates allowed, or a
        bool mask of length N) in place (tk_index_remove_rows) -> stored entries removed.  Surviving entries keep
        their order; ids, N and the vectors stay; emptied lists stay.  list_columns (n_lists, kp): the members per
        (list, column) where the index does not know them (a host upload; None: compacted all the same, the columns
        stay unknown).  Batches in flight finish first; allowed sets made before stop working (unless nothing
        stored was named)."""
        self._lists_may_change("remove", "removes no rows")
        rows = removal_rows(ids_or_mask, self.N)
        cols_p, keep, kp = None, None, 1
        if list_columns is not None:
            keep = np.ascontiguousarray(list_columns, dtype=np.int64)
            if keep.ndim != 2 or keep.shape[0] != self.n_lists:
                raise AssertionError(f"remove: list_columns must have shape ({self.n_lists}, kp), got {keep.shape}")
            cols_p, kp = keep.ctypes.data, keep.shape[1]
        else:
            known = C.c_int32(0)
            _lib.check(_lib.lib().tk_index_list_columns(self._h, C.byref(known), None))
            kp = max(1, known.value)
        removed = C.c_int64(0)
        _lib.check(_lib.lib().tk_index_remove_rows(self._h, rows.ctypes.data, len(rows), kp, cols_p,
                                                   C.byref(removed)))
        self._refresh_lists()
        return int(removed.value)

    @property
    def handle(self):
        return self._h

    def allow(self, ids_or_mask):
        """A prepared allowed set for the `allowed=` argument of the query calls (AllowSet)."""
        a = AllowSet(self, ids_or_mask)
        self._live_allows.add(a)
        return a

    def _set_rows(self, at, x):
        """set_groups / set_tags / set_values: x parsed (at.rows) and uploaded, or cleared for None -> what was uploaded"""
        if _dev_is_sharded(self) or self._source is not None:
            raise RuntimeError(f"DeviceIndex.set_{at.name}: a list-sharded index takes no row {at.name}")
        a = None if x is None else at.rows(x, self.N, f"set_{at.name}")
        _lib.check(getattr(_lib.lib(), f"tk_index_set_{at.name}")(self._h, *(at.clear if a is None else at.upload(a))))
        return a

    def _rows_set(self, at):
        """groups_set / tags_set / values_set: the rows the device's attribute covers (tk_index_<name>)"""
        return int(_lib.check(getattr(_lib.lib(), f"tk_index_{at.name}")(self._h)))

    def _table_info(self, one, fourth="row_bytes"):
        """group_table / tag_table / value_table / row_table: the four numbers of tk_index_<one>_table as a dict"""
        o = np.zeros(4, dtype=np.int64)
        _lib.check(getattr(_lib.lib(), f"tk_index_{one}_table")(self._h, _lib.ptr(o, _lib._i64p)))
        return {"built": bool(o[0]), "bytes": int(o[1]), "builds": int(o[2]), fourth: int(o[3])}

    def set_groups(self, groups):
        """One group id per row (int, [0, 2**31 - 1)) for the `group=` argument of the query calls, uploaded once
        (tk_index_set_groups); None clears.  After add() they must be set again for all N rows.  Batches in flight
        finish first.  Not for a list-sharded index."""
        self._set_rows(GROUPS, groups)

    def groups_set(self):
        """The number of rows the device's groups cover, 0 for none (tk_index_groups)."""
        return self._rows_set(GROUPS)

    def group_table(self):
        """The group table behind group= (tk_index_group_table): dict(built, bytes, builds, row_bytes)."""
        return self._table_info(GROUPS.one)

    def set_tags(self, tags):
        """One 64-bit tag mask per row (bit t set: the row carries tag t) for the `tags=` argument of the query
        calls, uploaded once (tk_index_set_tags); None clears.  After add() they must be set again for all N rows.
        Batches in flight finish first.  Not for a list-sharded index."""
        self._set_rows(TAGS, tags)

    def tags_set(self):
        """The number of rows the device's tags cover, 0 for none (tk_index_tags)."""
        return self._rows_set(TAGS)

    def tag_table(self):
        """The tag table behind tags= (tk_index_tag_table): dict(built, bytes, builds, row_bytes)."""
        return self._table_info(TAGS.one)

    def set_values(self, values):
        """1 to 4 numeric columns per row, (N,) or (N, C) of one integer or floating dtype, for the `between=` argument
        of the query calls: mapped to int64 keys (value_keys) and uploaded once, column-major (tk_index_set_values);
        None clears.  After add() they must be set again for all N rows.  Batches in flight finish first.  Not for a
        list-sharded index."""
        keys = self._set_rows(VALUES, values)
        if keys is None:
            self._value_kind, self._value_cols = None, 0
        else:
            self._value_kind, self._value_cols = value_kind(np.asarray(values).dtype), int(np.prod(keys.shape[1:]))

    def values_set(self):
        """The number of rows the device's values cover, 0 for none (tk_index_values)."""
        return self._rows_set(VALUES)

    def value_table(self):
        """The value table behind between= (tk_index_value_table): dict(built, bytes, builds, row_bytes, cols)."""
        return dict(self._table_info(VALUES.one), cols=int(_lib.check(_lib.lib().tk_index_value_columns(self._h))))

    def _ranges_of(self, between, nq):
        """the (nq, C, 2) int64 keys of a `between=` argument (query_ranges); without values, an array the library
        refuses (its TK_ERR_STATE names what to do)"""
        if self._value_kind is None:
            return np.zeros((nq, 1, 2), dtype=np.int64)
        return query_ranges(between, nq, self._value_cols, self._value_kind)

    def _allow_of(self, allowed):
        """(set, temporary) for an `allowed=` argument: a prepared set of this index, or a mask / ids made into one"""
        if isinstance(allowed, AllowSet):
            if allowed._dev is not self:
                raise ValueError("allowed: the set was prepared for another index")
            return allowed, False
        return AllowSet(self, allowed), True

    def close(self):
        # every session on this index, the caller's own included: a session that outlived the
        # index would drain and join a freed handle
        for st in list(getattr(self, "_live_streams", ())):
            st.close()
        for a in list(getattr(self, "_live_allows", ())):
            a.close()
        self._streams = {}
        if getattr(self, "_h", None):
            if _lib.owns_handles():
                _lib.lib().tk_index_destroy(self._h)
            self._h = None

    # ---- streaming (exact) ---------------------------------------------------
    def max_sub_batch(self, k, n_probes, pass_1=None):
        return _lib.check(_lib.lib().tk_index_max_sub_batch(self._h, int(k), int(n_probes),
                                                            int(pass_1 or 0)))

    def stream(self, max_nq, k, n_probes, pass_1=None, slots=8):
        """A new streaming session (see QueryStream); the caller closes it."""
        return QueryStream(self, max_nq, k, n_probes, pass_1, slots)

    CHUNK = 10000       # queries per sub-batch of the chunked host API

    def _cached_stream(self, nq, k, n_probes, pass_1):
        """One session per k: its page-locked staging does not depend on n_probes, so a sweep
        over n_probes only re-sizes the index's workspaces (tk_stream_set_probes)."""
        key = int(k)
        chunk = min(self.CHUNK, self.max_sub_batch(k, n_probes, pass_1))
        want = min(int(nq), chunk)
        st = self._streams.get(key)
        if st is not None and (st.max_nq < want or st.max_nq > chunk):
            st.close()
            st = None
        if st is None:
            cap = min(chunk, max(64, 1 << (want - 1).bit_length()))
            st = self._streams[key] = QueryStream(self, cap, k, n_probes, pass_1)
        else:
            st.set_probes(n_probes, pass_1)
        return st

    def query_raw(self, qs, k, n_probes, pass_1=None):
        """Exact IVF.query for every row of qs (raw float32 queries on the host): chunks of
        up to CHUNK rows through a streaming session, so that the host preparation and the
        copies of a chunk overlap the kernels of the chunks before it."""
        qs = np.ascontiguousarray(qs, dtype=np.float32)
        nq = qs.shape[0]
        assert qs.shape[1] == self.d
        out = np.full((nq, k), -1, dtype=np.int64)
        if nq == 0:
            return out
        st = self._cached_stream(nq, k, n_probes, pass_1)
        for o in range(0, nq, st.max_nq):
            st.submit(qs[o:o + st.max_nq], out[o:o + st.max_nq])
        st.drain()
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _exclude_of(self, exclude, nq):
        """the int64 array an `exclude=` argument is: 1-d, one entry per query, each a row id or -1 (nothing)"""
        a = np.asarray(exclude)
        if a.ndim != 1 or not (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
            raise TypeError("exclude: a 1-d integer array, one row id (or -1) per query")
        if a.shape[0] != nq:
            raise ValueError(f"exclude: one entry per query ({nq}), got {a.shape[0]}")
        a = np.ascontiguousarray(a, dtype=np.int64)
        if a.size and (a.min() < -1 or a.max() >= self.N):
            raise ValueError(f"exclude: entries must lie in [-1, {self.N})")
        return a

    def _query_host(self, call, nq, k, n_probes, pass_1, debug, return_distances, allowed, split, always=False):
        """A host query call from its outputs to what it returns.  The outputs: ids filled with -1, with
        return_distances the distances filled with +inf in the index's precision, with debug the probes and the two
        heap arrays.  The sub-batches: call(o, e, allowed set's handle, out, dist, probes, heap_idx, heap_val) — each
        output's rows [o, e) as the library takes it, or None — for all nq rows at once, or under `split` for
        max_sub_batch rows at a time (which keeps the debug outputs of every row); `always`: once even for nq = 0.
        A mask or ids in `allowed` are a set for as long as that takes."""
        if return_distances and debug:
            raise ValueError("query_batch: debug=True cannot be combined with return_distances=True")
        out = np.full((nq, k), -1, dtype=np.int64)
        dist = probes = hidx = hval = None
        if return_distances:
            dist = np.full((nq, k), np.inf, dtype=np.float64 if self._f64 else np.float32)
        if debug:
            R = pass_1 if pass_1 else (n_probes + 1) * k + 1
            probes = np.zeros((nq, min(n_probes, self.n_lists)), dtype=np.int64)
            hidx = np.zeros((nq, R), dtype=np.int64)
            hval = np.zeros((nq, R), dtype=np.int32)
        aset, temp = (None, False) if allowed is None else self._allow_of(allowed)
        try:
            step = max(1, self.max_sub_batch(k, n_probes, pass_1)) if split else max(1, nq)
            for o in range(0, max(nq, 1) if always else nq, step):
                e = min(nq, o + step)
                _lib.check(call(o, e, None if aset is None else aset.handle,
                                _lib.ptr(out[o:e], _lib._i64p), None if dist is None else dist[o:e].ctypes.data,
                                None if probes is None else _lib.ptr(probes[o:e], _lib._i64p),
                                None if hidx is None else _lib.ptr(hidx[o:e], _lib._i64p),
                                None if hval is None else _lib.ptr(hval[o:e], _lib._i32p)))
        finally:
            if temp:
                aset.close()
        if debug:
            return out, dict(probes=probes, heap_idx=hidx, heap_val=hval)
        return (out, dist) if return_distances else out

    def query_batch(self, qn, q_pq, k, n_probes, pass_1=None, debug=False, *, allowed=None, return_distances=False,
                    exclude=None, group=None, tags=None, tags_mode="any", between=None, per_group=None):
        """qn: (nq, d) float32 normalised queries; q_pq: (nq, dq) table-build queries.
        per_group: None, an int for every query, or a 1-d integer array of length nq: the most rows of any one group
        (set_groups) a query returns, 0 for no cap — the ranking the rescoring makes is walked and a candidate kept
        while fewer than that many of its group have been kept, up to k; rows may end in -1.  The
        candidates are the heap's: a larger pass_1 or n_probes widens the pool, nothing does by itself.  A call with it
        takes tk_index_query_batch_ex6.
        between: None, or (lo, hi): the inclusive interval of values (set_values) each query's rows must lie in, per
        column — each end None, a scalar, (nq,) for one column, (nq, C), or (C,) where nq != C (query_ranges; the
        reference's `insert` only for labels that pass).
        tags: None, an int for every query, or a 1-d integer array of length nq: the 64-bit tag mask each query is
        restricted by, 0 for none; tags_mode "any": a row passes where it carries one of the mask's tags (set_tags),
        "all": where it carries every one (the reference's `insert` only for labels that pass).
        group: None, an int for every query, or a 1-d integer array of length nq: the group of rows (set_groups) each
        query may return, -1 for any (the reference's `insert` only for labels of that group).
        exclude: None, or a 1-d integer array of length nq: the row each query may not return, -1 for none (the
        reference's `insert` only for labels != that row).
        A call with between, tags, group or exclude takes the library's one restricted entry point
        (tk_index_query_batch_ex5, NULL for what is not given), not the cached streaming session.
        allowed: None, or the rows the queries may return — an AllowSet (allow()), a bool mask of length N or row
        ids (the library's _allow entry point: the reference's `insert` only for those labels).
        return_distances: (ids, dists) — the same ids, and beside each the exact squared distance the rescoring
        ranked it by (the library's _dist entry point): float32, float64 for float64 vectors, +inf beside -1."""
        if return_distances and debug:
            raise ValueError("query_batch: debug=True cannot be combined with return_distances=True")
        qn = np.ascontiguousarray(qn, dtype=np.float32)
        is64 = q_pq.dtype != np.float32
        q_pq = np.ascontiguousarray(q_pq, dtype=np.float64 if is64 else np.float32)
        nq = qn.shape[0]
        assert qn.shape[1] == self.d and q_pq.shape == (nq, self.dq)
        L, knobs = _lib.lib(), (int(k), int(n_probes), int(pass_1 or 0))

        def queries(o, e):
            return _lib.ptr(qn[o:e], _lib._f32p), q_pq[o:e].ctypes.data, int(is64), e - o, *knobs

        if (group is not None or exclude is not None or tags is not None or between is not None
                or per_group is not None):
            group = None if group is None else query_groups(group, nq)
            per_group = None if per_group is None else query_caps(per_group, nq)
            tags, mode = (None, 0) if tags is None else (query_tags(tags, nq), tag_mode_of(tags_mode))
            between = None if between is None else self._ranges_of(between, nq)
            exclude = None if exclude is None else self._exclude_of(exclude, nq)

            def rows(a, o, e):
                return None if a is None else a[o:e].ctypes.data

            def restricted(o, e, aset, *outs):
                r = (self._h, aset, rows(exclude, o, e), rows(group, o, e), rows(tags, o, e), mode, rows(between, o, e))
                if per_group is None:
                    return L.tk_index_query_batch_ex5(*r, *queries(o, e), *outs)
                return L.tk_index_query_batch_ex6(*r, rows(per_group, o, e), *queries(o, e), *outs)

            return self._query_host(restricted, nq, k, n_probes, pass_1, debug, return_distances, allowed, split=debug)
        if allowed is None and not return_distances and not debug and nq > 0:
            # the session pads unrotated queries on the device: only for q_pq = pad1(qn)
            plain = is64 or (np.array_equal(q_pq[:, :self.d], qn) and not q_pq[:, self.d:].any())
            if plain and _front.bind():
                # prepared rows through the streaming session (pinned staging, async copies)
                out = np.full((nq, k), -1, dtype=np.int64)
                st = self._cached_stream(nq, k, n_probes, pass_1)
                for o in range(0, nq, st.max_nq):
                    st.submit_prepared(qn[o:o + st.max_nq],
                                       q_pq[o:o + st.max_nq] if is64 else None, out[o:o + st.max_nq])
                st.drain()
                return out
        if return_distances:
            def call(o, e, aset, out, dist, *dbg):
                return L.tk_index_query_batch_dist(self._h, aset, *queries(o, e), out, dist)
        elif allowed is None:
            def call(o, e, aset, out, dist, *dbg):
                return L.tk_index_query_batch(self._h, *queries(o, e), out, *dbg)
        else:
            def call(o, e, aset, out, dist, *dbg):
                return L.tk_index_query_batch_allow(self._h, aset, *queries(o, e), out, *dbg)
        # (only with a set is a debug call split; without one, and for distances, the library is called even for no query)
        return self._query_host(call, nq, k, n_probes, pass_1, debug, return_distances, allowed,
                                split=debug and allowed is not None, always=return_distances or allowed is None)

    def _rows_of(self, rows, what):
        """int64 row ids in [0, N), duplicates allowed (validated like remove's ids)"""
        is_mask, a = _mask_or_ids(rows, self.N, what, "a 1-d integer array of row ids")
        if is_mask:
            raise TypeError(f"{what}: a 1-d integer array of row ids")
        return a

    def pipeline_settings(self):
        """(pipeline depth, coalesce) as the library holds them (tk_index_info, tk_index_coalesce)"""
        info = np.zeros(8, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_info(self._h, _lib.ptr(info, _lib._i64p)))
        return int(info[5]), int(_lib.check(_lib.lib().tk_index_coalesce(self._h)))

    def rotated(self):
        """True where the device holds the PQ's rotation: its q_pq (gather_queries, the fast front end) is float64"""
        info = np.zeros(8, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_info(self._h, _lib.ptr(info, _lib._i64p)))
        return bool(info[4] > 0)

    def gather_queries(self, rows):
        """(qn, q_pq) on the host as the device makes them from the stored rows (tk_index_gather_queries):
        qn = float32(data[rows]), not normalised again; q_pq = qn padded (float32), or rotated by the device's
        float64 FMA chain where the PQ has a rotation (float64)."""
        rows = self._rows_of(rows, "gather_queries")
        qn = np.zeros((len(rows), self.d), dtype=np.float32)
        qp = np.zeros((len(rows), self.dq), dtype=np.float64 if self.rotated() else np.float32)
        _lib.check(_lib.lib().tk_index_gather_queries(self._h, _lib.ptr(rows, _lib._i64p), len(rows),
                                                      _lib.ptr(qn, _lib._f32p), qp.ctypes.data))
        return qn, qp

    def gather_queries_dev(self, rows_ptr, nq, qn_ptr, qpq_ptr, stream=0):
        """Device pointers: nq int64 row ids (in [0, N): not checked) -> qn (nq, d) float32 and q_pq (nq, dq),
        float64 iff the PQ has a rotation; enqueued on `stream` (tk_index_gather_queries_dev)."""
        _lib.check(_lib.lib().tk_index_gather_queries_dev(self._h, rows_ptr, int(nq), qn_ptr, qpq_ptr, stream))

    def query_rows(self, rows, k, n_probes, pass_1=None, debug=False, *, exclude_self=True, allowed=None,
                   return_distances=False, per_group=None):
        """The neighbours of stored rows (tk_index_query_rows): gather_queries(rows) as the queries, each leaving
        its own row out where exclude_self.  Outputs as query_batch.  per_group: as query_batch's — that call, on
        gather_queries(rows) with exclude=rows where exclude_self."""
        rows = self._rows_of(rows, "query_rows")
        if per_group is not None:
            qn, qp = self.gather_queries(rows)
            return self.query_batch(qn, qp, k, n_probes, pass_1, debug, allowed=allowed, exclude=rows if exclude_self else None,
                                    return_distances=return_distances, per_group=per_group)
        L, knobs = _lib.lib(), (int(k), int(n_probes), int(pass_1 or 0))
        return self._query_host(
            lambda o, e, aset, *outs: L.tk_index_query_rows(
                self._h, aset, _lib.ptr(rows[o:e], _lib._i64p), e - o, int(bool(exclude_self)), *knobs, *outs),
            len(rows), k, n_probes, pass_1, debug, return_distances, allowed, split=debug)

    def row_table(self):
        """The row-position table behind exclude= (tk_index_row_table): dict(built, bytes, builds, entries)."""
        return self._table_info("row", "entries")

    def query_batch_raw(self, qs, k, n_probes, pass_1=None):
        """Fast mode: raw float32 queries, normalisation / padding / rotation on the device
        (tk_index_prepare_dev: not bit-identical to the host's BLAS results — normalised rows within 4 float32
        ulp of them, rotated ones within 7.5 * 2^-53 * sum |x_t R_jt|; measured)."""
        qs = np.ascontiguousarray(qs, dtype=np.float32)
        assert qs.shape[1] == self.d
        out = np.full((qs.shape[0], k), -1, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_query_batch_raw(
            self._h, _lib.ptr(qs, _lib._f32p), qs.shape[0], int(self.angular), int(k), int(n_probes),
            int(pass_1 or 0), _lib.ptr(out, _lib._i64p)))
        return out

    def knn_brute(self, qn, k, *, allowed=None, exclude=None, group=None, tags=None, tags_mode="any", between=None):
        """Exact k nearest rows of IVF.data for normalised queries (ground truth of recall;
        tk_index_knn_brute: f32 MFMA, numpy's distances bit for bit), ascending.  Float32 vectors only:
        refused on a float64 and on a half index.
        allowed / exclude / group / tags, tags_mode / between: the restrictions of query_batch, with its meanings — the
        k nearest among the rows that pass all of them, exactly, the row ending in -1 where fewer than k pass
        (tk_index_knn_brute_ex: the ground truth of restricted recall, and the answer for a filter so selective that
        the probed lists hold too few passing rows).  allowed: a bool mask of length N or row ids; an AllowSet is
        laid out by list position and refused (TypeError).  A mask of the surviving rows is the truth after remove():
        the vectors of removed rows stay in HBM and the unrestricted call still returns them.
        With nothing given the call is tk_index_knn_brute's.  The values the rows were ranked by: knn_brute_dist."""
        return self._knn_brute(qn, k, False, allowed, exclude, group, tags, tags_mode, between)

    def knn_brute_dist(self, qn, k, *, allowed=None, exclude=None, group=None, tags=None, tags_mode="any",
                       between=None):
        """knn_brute's ids and, beside each, the float32 `part` value it was ranked by: (ids, part), part = (|q|^2 +
        |y|^2) - 2 q.y as numpy's knn_brute sums it (utils.py:84; rounding can make it slightly negative), +inf
        beside -1.  Not the knn_brute1 distance that query_batch(return_distances=True) returns.  Always
        tk_index_knn_brute_ex; with no restriction the ids are knn_brute's."""
        return self._knn_brute(qn, k, True, allowed, exclude, group, tags, tags_mode, between)

    def _knn_brute(self, qn, k, want_dist, allowed, exclude, group, tags, tags_mode, between):
        """knn_brute / knn_brute_dist: the old entry point where nothing is asked beyond it, else tk_index_knn_brute_ex
        with the arguments parsed as query_batch parses them"""
        qn = np.ascontiguousarray(qn, dtype=np.float32)
        assert qn.shape[1] == self.d
        nq = qn.shape[0]
        out = np.empty((nq, k), dtype=np.int64)
        if (allowed is None and exclude is None and group is None and tags is None and between is None
                and not want_dist):
            _lib.check(_lib.lib().tk_index_knn_brute(self._h, _lib.ptr(qn, _lib._f32p), nq, int(k),
                                                     _lib.ptr(out, _lib._i64p)))
            return out
        restrict = self._brute_restrictions("knn_brute", nq, allowed, exclude, group, tags, tags_mode, between)
        dist = np.full((nq, k), np.inf, dtype=np.float32) if want_dist else None
        out[:] = -1
        _lib.check(_lib.lib().tk_index_knn_brute_ex(
            self._h, _lib.ptr(qn, _lib._f32p), nq, int(k), *self._host_pointers(restrict),
            _lib.ptr(out, _lib._i64p), None if dist is None else dist.ctypes.data))
        return (out, dist) if want_dist else out

    def _brute_restrictions(self, call, nq, allowed, exclude, group, tags, tags_mode, between):
        """The host arrays of a restricted exact call (knn_brute, radius_search), parsed as query_batch parses them:
        (mask, exclude, group, tags, tag mode, ranges), None for what was not given.  An AllowSet is refused
        (TypeError) and so is a list-sharded index, before the device is touched."""
        if isinstance(allowed, AllowSet):
            raise TypeError(f"{call}: allowed= takes a bool mask of length N or row ids; an AllowSet is laid out by "
                            "list position")
        if _dev_is_sharded(self):
            raise RuntimeError(f"{call} with restrictions is not supported on a list-sharded index")
        mask = None if allowed is None else AllowSet.mask_of(allowed, self.N)
        exclude = None if exclude is None else self._exclude_of(exclude, nq)
        group = None if group is None else query_groups(group, nq)
        tags, mode = (None, 0) if tags is None else (query_tags(tags, nq), tag_mode_of(tags_mode))
        between = None if between is None else np.ascontiguousarray(self._ranges_of(between, nq))
        return mask, exclude, group, tags, mode, between

    @staticmethod
    def _host_pointers(restrict):
        """_brute_restrictions' arrays as the C ABI takes them (NULL for None; the caller keeps the arrays alive)"""
        return [a if isinstance(a, int) else (None if a is None else a.ctypes.data) for a in restrict]

    def radius_brute(self, qn, radius, *, allowed=None, exclude=None, group=None, tags=None, tags_mode="any",
                     between=None, sort=True, max_results=None):
        """Every row within a radius of each normalised query, exactly (tk_index_radius_brute): CSR
        (lims, ids, part) — lims (nq + 1,) int64, query i's hits ids[lims[i]:lims[i + 1]] int64 with their float32
        `part` values beside them.  Row j is a hit of query i iff it passes the query's restrictions (allowed /
        exclude / group / tags, tags_mode / between: knn_brute's, parsed alike; an AllowSet is refused) and
        part(i, j) <= radius[i] in float32, inclusive; part is knn_brute_dist's value bit for bit, so for every k the
        ids of knn_brute_dist(k) are the first k entries of the list at radius = part[k - 1].
        radius: a scalar or (nq,), cast with np.float32; +inf: every passing row; negative: normally nothing; NaN and a
        wrong length: ValueError.  sort=True: every list ascending by (part, id), knn_brute's order, the same bytes from
        run to run; sort=False: the order inside a list is unspecified, lims and the sets are the same.
        max_results (default 1 << 26, < 2**31): a total above it raises ValueError naming the true total — nothing is
        returned, no list is ever cut, and the index stays usable.  Float32 vectors, d <= 128; not for a list-sharded
        index.  The vectors of removed rows stay in HBM, as for knn_brute: allowed= with the mask of the surviving
        rows is the truth after remove()."""
        qn, radius, restrict = self._radius_args("radius_search", qn, radius, allowed, exclude, group, tags, tags_mode,
                                                 between)
        max_results = (1 << 26) if max_results is None else int(max_results)
        if not 0 <= max_results < 2**31:
            raise ValueError(f"max_results: in [0, 2**31), got {max_results}")
        nq = len(qn)
        lims = np.zeros(nq + 1, dtype=np.int64)
        total = np.zeros(1, dtype=np.int64)
        lib = _lib.lib()
        rc = lib.tk_index_radius_brute(
            self._h, _lib.ptr(qn, _lib._f32p), nq, _lib.ptr(radius, _lib._f32p), *self._host_pointers(restrict),
            int(bool(sort)), 0, max_results, _lib.ptr(lims, _lib._i64p), _lib.ptr(total, _lib._i64p))
        if rc == -1 and int(total[0]) > max_results:
            raise ValueError(f"radius_search: {int(total[0])} rows lie within the radii, more than max_results = "
                             f"{max_results}; nothing is returned (raise max_results, or ask radius_count first)")
        _lib.check(rc)
        ids = np.empty(int(total[0]), dtype=np.int64)
        part = np.empty(int(total[0]), dtype=np.float32)
        _lib.check(lib.tk_index_radius_fetch(self._h, ids.ctypes.data, part.ctypes.data))
        return lims, ids, part

    def radius_count(self, qn, radius, *, allowed=None, exclude=None, group=None, tags=None, tags_mode="any",
                     between=None):
        """How many rows radius_brute would list per query: (nq,) int64, from the count pass alone (one pass over the
        rows instead of two and no sort).  No limit: the counts are summed in int64."""
        qn, radius, restrict = self._radius_args("radius_count", qn, radius, allowed, exclude, group, tags, tags_mode,
                                                 between)
        nq = len(qn)
        lims = np.zeros(nq + 1, dtype=np.int64)
        total = np.zeros(1, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_radius_brute(
            self._h, _lib.ptr(qn, _lib._f32p), nq, _lib.ptr(radius, _lib._f32p), *self._host_pointers(restrict),
            0, 1, 0, _lib.ptr(lims, _lib._i64p), _lib.ptr(total, _lib._i64p)))
        return np.diff(lims)

    # queries per tk_index_radius_probe call: a larger batch is cut here and its CSR parts joined (a part whose
    # candidate bitmap would not fit the workspace is halved again: TK_ERR_WORKSPACE)
    RADIUS_PROBE_CHUNK = 16384

    def radius_probe(self, qn, q_pq, radius, n_probes, *, allowed=None, exclude=None, group=None, tags=None,
                     tags_mode="any", between=None, sort=True, max_results=None):
        """Every row within a radius of each normalised query among the rows of the lists the query probes
        (tk_index_radius_probe): CSR (lims, ids, dist) — lims (nq + 1,) int64, query i's hits
        ids[lims[i]:lims[i + 1]] int64 with the rescoring's squared distances beside them, float32, float64 on float64
        vectors: the values query_batch(return_distances=True) and knn_group return, bit for bit.
        The probes are the index's own coarse stage for n_probes (query_batch(debug=True)["probes"]; they depend on
        n_probes alone).  The candidates are the labels in [0, N) stored in the distinct lists that row names — removed
        rows are never candidates, a row stored in several probed lists is one candidate — and a candidate is a hit iff
        it passes the restrictions (radius_brute's) and dist <= radius[i], inclusive (float64 vectors:
        dist <= float64(float32(r))).  Not radius_brute's `part`: the two round differently and agree exactly on
        integer data.  qn, q_pq: as query_batch takes them.  radius, sort, max_results: as radius_brute's; the limit
        holds for the whole call and is checked before any part of the result is fetched (join_radius_parts).  Every store, d <= 4096;
        not for a list-sharded index."""
        qn, radius, restrict = self._radius_args("radius_search", qn, radius, allowed, exclude, group, tags, tags_mode,
                                                 between)
        max_results = (1 << 26) if max_results is None else int(max_results)
        if not 0 <= max_results < 2**31:
            raise ValueError(f"max_results: in [0, 2**31), got {max_results}")
        q_pq, n_probes = self._probe_args(qn, q_pq, n_probes)
        return join_radius_parts(
            len(qn), self.RADIUS_PROBE_CHUNK, max_results,
            lambda o, e, limit: self._radius_probe_part(qn, q_pq, radius, n_probes, restrict, o, e, bool(sort), limit))

    def radius_probe_count(self, qn, q_pq, radius, n_probes, *, allowed=None, exclude=None, group=None, tags=None,
                           tags_mode="any", between=None):
        """How many rows radius_probe would list per query: (nq,) int64, from its count pass alone — no limit, no
        sort, nothing fetched."""
        qn, radius, restrict = self._radius_args("radius_count", qn, radius, allowed, exclude, group, tags, tags_mode,
                                                 between)
        q_pq, n_probes = self._probe_args(qn, q_pq, n_probes)
        lims, _, _ = join_radius_parts(
            len(qn), self.RADIUS_PROBE_CHUNK, None,
            lambda o, e, limit: self._radius_probe_part(qn, q_pq, radius, n_probes, restrict, o, e, False, None))
        return np.diff(lims)

    def _probe_args(self, qn, q_pq, n_probes):
        """the table-build queries as the C ABI takes them, and n_probes >= 1"""
        n_probes = int(n_probes)
        if n_probes < 1:
            raise ValueError(f"n_probes: at least 1, got {n_probes}")
        q_pq = np.ascontiguousarray(q_pq, dtype=np.float32 if q_pq.dtype == np.float32 else np.float64)
        assert q_pq.shape == (len(qn), self.dq)
        return q_pq, n_probes

    def _radius_probe_part(self, qn, q_pq, radius, n_probes, restrict, o, e, sort, limit):
        """Queries [o, e) through tk_index_radius_probe.  limit None: the count pass alone -> (lims, None);
        else (lims, fetch) with fetch() -> (ids, dist) of the result the index holds until its next radius call, or
        (lims, None) where the part's total is above the limit.  None where the part's bitmap does not fit."""
        mask, exclude, group, tags, mode, between = restrict
        part = (mask, None if exclude is None else exclude[o:e], None if group is None else group[o:e],
                None if tags is None else tags[o:e], mode, None if between is None else between[o:e])
        nq = e - o
        lims = np.zeros(nq + 1, dtype=np.int64)
        total = np.zeros(1, dtype=np.int64)
        lib = _lib.lib()
        qs, qp, rad = qn[o:e], q_pq[o:e], radius[o:e]
        rc = lib.tk_index_radius_probe(
            self._h, _lib.ptr(qs, _lib._f32p), qp.ctypes.data, int(qp.dtype == np.float64), nq, n_probes,
            _lib.ptr(rad, _lib._f32p), *self._host_pointers(part), int(sort), int(limit is None),
            0 if limit is None else limit, _lib.ptr(lims, _lib._i64p), _lib.ptr(total, _lib._i64p))
        if rc == -4:
            return None
        if rc == -1 and limit is not None and int(total[0]) > limit:
            return lims, None
        _lib.check(rc)
        if limit is None:
            return lims, None

        def fetch():
            ids = np.empty(int(total[0]), dtype=np.int64)
            dist = np.empty(int(total[0]), dtype=np.float64 if self._f64 else np.float32)
            _lib.check(lib.tk_index_radius_probe_fetch(self._h, ids.ctypes.data, dist.ctypes.data))
            return ids, dist
        return lims, fetch

    def _radius_args(self, call, qn, radius, allowed, exclude, group, tags, tags_mode, between):
        """the prepared queries, the (nq,) float32 radii and the restrictions of a radius call"""
        qn = np.ascontiguousarray(qn, dtype=np.float32)
        assert qn.ndim == 2 and qn.shape[1] == self.d
        restrict = self._brute_restrictions(call, len(qn), allowed, exclude, group, tags, tags_mode, between)
        return qn, query_radius(radius, len(qn)), restrict

    def knn_group(self, qn, k, group, *, allowed=None, exclude=None, tags=None, tags_mode="any", between=None,
                  return_distances=False):
        """The exact k nearest STORED rows inside each query's own group (tk_index_knn_group) for
        normalised queries: (nq, k) int64 ids ascending by (distance, row id), ending in -1 where fewer than k rows
        pass; with return_distances (ids, dists), the rescoring's exact squared distances — what query_batch(
        return_distances=True) returns, bit for bit: float32, float64 on float64 vectors — +inf beside -1.
        group: an int for every query or one id >= 0 per query (required; -1 is refused: an unrestricted query is
        knn_brute's or query_batch's).  A query reads the rows of its group and no other, so the cost follows the
        group's size; one workgroup walks a group, so for large groups knn_brute(group=) is the call.  Rows taken out
        by remove() never come back.  allowed / exclude / tags, tags_mode / between: as knn_brute's; an AllowSet is
        refused (TypeError).  Every vector store.  Not for a list-sharded index."""
        if isinstance(allowed, AllowSet):
            raise TypeError("knn_group: allowed= takes a bool mask of length N or row ids; an AllowSet is laid out by "
                            "list position")
        if _dev_is_sharded(self) or self._source is not None:
            raise RuntimeError("knn_group is not supported on a list-sharded index")
        qn = np.ascontiguousarray(qn, dtype=np.float32)
        assert qn.ndim == 2 and qn.shape[1] == self.d
        nq = qn.shape[0]
        group = query_groups(group, nq)
        if len(group) and int(group.min()) < 0:
            raise AssertionError("knn_group: group= needs a group id >= 0 for every query (-1, any group, is "
                                 "knn_brute's or query_batch's to answer)")
        mask = None if allowed is None else AllowSet.mask_of(allowed, self.N)
        exclude = None if exclude is None else self._exclude_of(exclude, nq)
        tags, mode = (None, 0) if tags is None else (query_tags(tags, nq), tag_mode_of(tags_mode))
        between = None if between is None else np.ascontiguousarray(self._ranges_of(between, nq))
        out = np.full((nq, k), -1, dtype=np.int64)
        dist = np.full((nq, k), np.inf, dtype=np.float64 if self._f64 else np.float32) if return_distances else None

        def host(a):
            return None if a is None else a.ctypes.data

        _lib.check(_lib.lib().tk_index_knn_group(
            self._h, _lib.ptr(qn, _lib._f32p), nq, int(k), host(group), host(mask), host(exclude), host(tags), mode,
            host(between), _lib.ptr(out, _lib._i64p), host(dist)))
        return (out, dist) if return_distances else out

    def group_sizes(self, g):
        """The number of rows that carry each group id of g (an int or a 1-d integer array; tk_index_group_sizes):
        int64, 0 for an id no row carries.  Counted over all N rows: the rows remove() took out are still counted."""
        g = np.ascontiguousarray(np.atleast_1d(np.asarray(g)))
        if g.ndim != 1 or not np.issubdtype(g.dtype, np.integer):
            raise TypeError("group_sizes: an int or a 1-d integer array of group ids")
        if len(g) and (int(g.min()) < -(2 ** 31) or int(g.max()) >= 2 ** 31):
            raise ValueError("group_sizes: group ids must fit int32")
        g = np.ascontiguousarray(g, dtype=np.int32)
        out = np.zeros(len(g), dtype=np.int64)
        _lib.check(_lib.lib().tk_index_group_sizes(self._h, g.ctypes.data, len(g), _lib.ptr(out, _lib._i64p)))
        return out

    def group_rows(self):
        """The rows gathered by group behind knn_group (tk_index_group_rows): dict(built, bytes, builds, groups)."""
        o = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_group_rows(self._h, _lib.ptr(o, _lib._i64p)))
        return {"built": bool(o[0]), "bytes": int(o[1]), "builds": int(o[2]), "groups": int(o[3])}

    def knn_between(self, qn, k, between, *, allowed=None, exclude=None, group=None, tags=None, tags_mode="any",
                    return_distances=False):
        """The exact k nearest STORED rows inside each query's value range (tk_index_knn_between) for
        normalised queries: outputs as knn_group's — (nq, k) int64 ids ascending by (distance, row id), ending in -1
        where fewer than k rows pass; with return_distances (ids, dists), the rescoring's exact squared distances,
        +inf beside -1.  between: (lo, hi) as query_batch's (required); every query must bound at least one column
        (ValueError naming the first that does not: an unrestricted query is knn_brute's or query_batch's).  A query
        walks the rows that ONE column of its range admits — the column that admits the fewest (range_sizes) — in
        value order and tests every condition on them, so the cost follows that number; one workgroup walks a span, so
        for wide ranges knn_brute(between=) is the call.  Rows taken out by remove() never come back.  allowed /
        exclude / group (-1: any) / tags, tags_mode: as knn_brute's; an AllowSet is refused (TypeError).  Every vector
        store.  Not for a list-sharded index."""
        if isinstance(allowed, AllowSet):
            raise TypeError("knn_between: allowed= takes a bool mask of length N or row ids; an AllowSet is laid out by "
                            "list position")
        if _dev_is_sharded(self) or self._source is not None:
            raise RuntimeError("knn_between is not supported on a list-sharded index")
        qn = np.ascontiguousarray(qn, dtype=np.float32)
        assert qn.ndim == 2 and qn.shape[1] == self.d
        nq = qn.shape[0]
        if between is None:
            raise TypeError("knn_between: between= is required: a pair (lo, hi)")
        between = np.ascontiguousarray(self._ranges_of(between, nq))
        free = np.flatnonzero(unbounded_queries(between))
        if len(free):
            raise ValueError(f"knn_between: query {int(free[0])} bounds no column (an unrestricted query is knn_brute's "
                             "or query_batch's to answer)")
        mask = None if allowed is None else AllowSet.mask_of(allowed, self.N)
        exclude = None if exclude is None else self._exclude_of(exclude, nq)
        group = None if group is None else query_groups(group, nq)
        tags, mode = (None, 0) if tags is None else (query_tags(tags, nq), tag_mode_of(tags_mode))
        out = np.full((nq, k), -1, dtype=np.int64)
        dist = np.full((nq, k), np.inf, dtype=np.float64 if self._f64 else np.float32) if return_distances else None

        def host(a):
            return None if a is None else a.ctypes.data

        _lib.check(_lib.lib().tk_index_knn_between(
            self._h, _lib.ptr(qn, _lib._f32p), nq, int(k), host(between), host(mask), host(exclude), host(group),
            host(tags), mode, _lib.ptr(out, _lib._i64p), host(dist)))
        return (out, dist) if return_distances else out

    def range_sizes(self, between, nq=None):
        """(len, col) per query of a `between=` argument (tk_index_range_sizes): the number of rows of the span
        knn_between would walk for it — the rows that the column admitting the fewest admits — and that column; (N, -1)
        for a query that bounds no column, length 0 for an empty interval.  int64 / int32.  Counted over all N rows, the
        rows remove() took out too: what the walk costs, and an upper bound on the rows that pass.  nq: the number
        of queries where the argument does not say (scalars for every query); default: the length of its arrays, or 1."""
        if nq is None:
            nq = ranges_length(between, self._value_cols or 1)
        keys = np.ascontiguousarray(self._ranges_of(between, int(nq)))
        length = np.zeros(len(keys), dtype=np.int64)
        col = np.zeros(len(keys), dtype=np.int32)
        _lib.check(_lib.lib().tk_index_range_sizes(self._h, keys.ctypes.data, len(keys), _lib.ptr(length, _lib._i64p),
                                                   _lib.ptr(col, _lib._i32p)))
        return length, col

    def value_rows(self):
        """The rows in value order behind knn_between (tk_index_value_rows): dict(built, bytes, builds, columns)."""
        o = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_value_rows(self._h, _lib.ptr(o, _lib._i64p)))
        return {"built": bool(o[0]), "bytes": int(o[1]), "builds": int(o[2]), "columns": int(o[3])}

    def query_batch_dev(self, qn_ptr, qpq_ptr, qpq_is_f64, nq, k, n_probes, out_ptr,
                        pass_1=None, stream=0, done_event=None, *, allowed=None, dist_ptr=None, exclude_ptr=None,
                        group_ptr=None, tags_ptr=None, tags_mode="any", between_ptr=None, per_group_ptr=None):
        """Device pointers in, device pointer out, enqueued on `stream` (no sync).
        done_event: a hipEvent_t (integer handle) recorded behind the batch's last kernel, on
        whichever internal stream that runs (tk_index_query_batch_dev_ex).
        With set_pipeline(depth > 1) the kernels of a call run up to three calls later, and with
        set_coalesce(2) they read the queries from, and write the ids to, these very buffers (no
        staging copy): all three buffers belong to the library until join() — or the call's
        done_event — as include/tinyknn_hip.h says for tk_index_set_pipeline.
        allowed: None or an AllowSet of this index (allow()), which must stay open until the call has run
        (tk_index_query_batch_dev_allow).
        dist_ptr: None, or a device buffer of nq * k distances (float32; float64 for float64 vectors) that receives
        the rescoring's exact squared distances beside the ids, complete when out_ptr's ids are
        (tk_index_query_batch_dev_dist).
        exclude_ptr: None, or a device buffer of nq int64: the row each query may not return, anything outside [0, N)
        for none; the library's until join() or done_event, like the others.
        group_ptr: None, or a device buffer of nq int32: the group each query is restricted to, any entry < 0 for an
        unrestricted query; the caller's again after join() or done_event.
        tags_ptr: None, or a device buffer of nq uint64: the tag mask each query is restricted by under tags_mode
        ("any" / "all"), an entry of 0 for an unrestricted query; the caller's again after join() or done_event.
        between_ptr: None, or a device buffer of nq x C x 2 int64 keys (query_ranges' array): the interval each query
        is restricted to per value column, INT64_MIN / INT64_MAX for an unbounded end; the caller's again after
        join() or done_event.
        A call with any of these four takes the library's one restricted entry point (tk_index_query_batch_dev_ex5,
        NULL for the ones not given).
        per_group_ptr: None, or a device buffer of nq int32: the most rows of any one group each query returns, an
        entry <= 0 for no cap; the caller's again after join() or done_event.  A call with it takes
        tk_index_query_batch_dev_ex6."""
        if allowed is not None:
            if not isinstance(allowed, AllowSet):
                raise TypeError("query_batch_dev: allowed= takes a prepared set (DeviceIndex.allow / IVF.allow)")
            allowed = self._allow_of(allowed)[0].handle
        L, ev = _lib.lib(), None if done_event is None else C.c_void_p(int(done_event))
        if per_group_ptr is not None:
            mode = tag_mode_of(tags_mode) if tags_ptr is not None else 0
            rc = L.tk_index_query_batch_dev_ex6(
                self._h, allowed, exclude_ptr, group_ptr, tags_ptr, mode, between_ptr, per_group_ptr, qn_ptr, qpq_ptr,
                int(qpq_is_f64), nq, int(k), int(n_probes), int(pass_1 or 0), out_ptr, dist_ptr, ev, stream)
        elif exclude_ptr is not None or group_ptr is not None or tags_ptr is not None or between_ptr is not None:
            mode = tag_mode_of(tags_mode) if tags_ptr is not None else 0
            rc = L.tk_index_query_batch_dev_ex5(
                self._h, allowed, exclude_ptr, group_ptr, tags_ptr, mode, between_ptr, qn_ptr, qpq_ptr, int(qpq_is_f64),
                nq, int(k), int(n_probes), int(pass_1 or 0), out_ptr, dist_ptr, ev, stream)
        elif dist_ptr is not None:
            rc = L.tk_index_query_batch_dev_dist(
                self._h, allowed, qn_ptr, qpq_ptr, int(qpq_is_f64), nq, int(k), int(n_probes), int(pass_1 or 0),
                out_ptr, dist_ptr, ev, stream)
        elif allowed is not None:
            rc = L.tk_index_query_batch_dev_allow(
                self._h, allowed, qn_ptr, qpq_ptr, int(qpq_is_f64), nq, int(k), int(n_probes), int(pass_1 or 0),
                out_ptr, None, ev, stream)
        else:       # (NULL pinned buffer; with a NULL event this is the library's plain _dev call)
            rc = L.tk_index_query_batch_dev_ex(
                self._h, qn_ptr, qpq_ptr, int(qpq_is_f64), nq, int(k), int(n_probes), int(pass_1 or 0),
                out_ptr, None, ev, stream)
        _lib.check(rc)

    def shard_coarse_dev(self, slot, qn_ptr, qpq_ptr, qpq_is_f64, nq, k, n_probes, pass_1,
                         probes_home_ptr, stream=0):
        """Tables for all queries + the coarse stage of this rank's home queries
        (tk_index_shard_coarse_dev); the caller all-gathers the probe lists."""
        _lib.check(_lib.lib().tk_index_shard_coarse_dev(
            self._h, int(slot), qn_ptr, qpq_ptr, int(qpq_is_f64), nq, int(k), int(n_probes),
            int(pass_1 or 0), probes_home_ptr, stream))

    def shard_scan_dev(self, slot, qn_ptr, qpq_ptr, qpq_is_f64, nq, k, n_probes, pass_1, capacity,
                       send_ptr, flag_ptr, stream=0, probes_all_ptr=None):
        """Scan of the owned segments into the send buffer (tk_index_shard_scan_dev);
        probes_all_ptr None: the replicated coarse stage runs inside this call."""
        _lib.check(_lib.lib().tk_index_shard_scan_dev(
            self._h, int(slot), qn_ptr, qpq_ptr, int(qpq_is_f64), nq, int(k), int(n_probes),
            int(pass_1 or 0), probes_all_ptr, int(capacity), send_ptr, flag_ptr, stream))

    def shard_finish_dev(self, slot, qn_ptr, nq, k, n_probes, pass_1, capacity, recv_ptr, out_ptr,
                         stream=0, flag_ptr=None):
        """Second half, after the all-to-all (tk_index_shard_finish_dev).  flag_ptr: the batch's flag
        word — required behind shard_scan_plain_dev (bit 4: a home query failed the plain path's check)."""
        _lib.check(_lib.lib().tk_index_shard_finish_dev(
            self._h, int(slot), qn_ptr, nq, int(k), int(n_probes), int(pass_1 or 0),
            int(capacity), recv_ptr, out_ptr, flag_ptr, stream))

    def shard_scan_plain_dev(self, slot, qn_ptr, qpq_ptr, qpq_is_f64, nq, k, n_probes, pass_1, capacity,
                             send_ptr, flag_ptr, stream=0, probes_all_ptr=None, bound_ptr=None):
        """The owned segments in ONE phase as the unsharded pipeline scores them: heads exactly, the rest
        as plain sums on the matrix cores, checked by the home rank's replay
        (tk_index_shard_scan_plain_dev; falls back to shard_scan_dev's kernel where that does not apply).
        bound_ptr: the min-reduced bounds of shard_scan_head_dev — queries above their table's limit
        stay exact, the check at home cannot fail."""
        _lib.check(_lib.lib().tk_index_shard_scan_plain_dev(
            self._h, int(slot), qn_ptr, qpq_ptr, int(bool(qpq_is_f64)), nq, int(k), int(n_probes),
            int(pass_1 or 0), probes_all_ptr, int(capacity), send_ptr, flag_ptr, bound_ptr, stream))

    def shard_scan_head_dev(self, slot, qn_ptr, qpq_ptr, qpq_is_f64, nq, k, n_probes, pass_1, capacity,
                            send_ptr, flag_ptr, bound_ptr, stream=0, probes_all_ptr=None):
        """Heads of the first probed lists this rank owns, exactly, + the bound after them
        (tk_index_shard_scan_head_dev); the caller min-reduces the bytes, then shard_scan_plain_dev(bound_ptr)."""
        _lib.check(_lib.lib().tk_index_shard_scan_head_dev(
            self._h, int(slot), qn_ptr, qpq_ptr, int(bool(qpq_is_f64)), nq, int(k), int(n_probes),
            int(pass_1 or 0), probes_all_ptr, int(capacity), send_ptr, flag_ptr, bound_ptr, stream))

    def clone_shard(self, owner, rank, world):
        """Rank `rank`'s shard of this complete unsharded index as a NEW handle on the same device
        (tk_index_clone_shard): it borrows the replicated arrays — this index must outlive it — and owns
        the codes of its lists.  How several ranks of a list partition are played on one GPU."""
        own = np.ascontiguousarray(owner, dtype=np.int32)
        assert own.shape == (self.n_lists,)
        h = _lib.lib().tk_index_clone_shard(self._h, _lib.ptr(own, _lib._i32p), int(rank), int(world))
        if not h:
            raise _lib.TinyKnnHipError(_lib.lib().tk_last_error().decode() or "tk_index_clone_shard failed")
        c = DeviceIndex.__new__(DeviceIndex)
        c._new_state()
        c._h = h
        c._source = self            # keeps the lender alive
        c.dq, c.dpb, c.d, c.n_lists, c.N, c.angular = self.dq, self.dpb, self.d, self.n_lists, self.N, self.angular
        c._R, c._f64, c.list_sizes, c.code_bytes = self._R, self._f64, self.list_sizes, self.code_bytes
        c.rank, c.world = int(rank), int(world)
        self._clones.add(c)
        return c

    def shard_usage(self, slot):
        """Longest stream (uint4) of the slot's last shard_scan_dev (tk_index_shard_usage; syncs)."""
        v = C.c_int64(0)
        _lib.check(_lib.lib().tk_index_shard_usage(self._h, int(slot), C.byref(v)))
        return int(v.value)

    def shard_bound_dev(self, slot, nq, k, n_probes, pass_1, capacity, scan_ptr, bound_ptr, stream=0):
        """Bound after the first probed list, for the queries whose first list this rank owns
        (tk_index_shard_bound_dev); the caller min-reduces the bytes over the ranks."""
        _lib.check(_lib.lib().tk_index_shard_bound_dev(
            self._h, int(slot), nq, int(k), int(n_probes), int(pass_1 or 0), int(capacity),
            scan_ptr, bound_ptr, stream))

    def shard_filter_dev(self, slot, nq, k, n_probes, pass_1, capacity, scan_ptr, bound_ptr,
                         counts_ptr, records_ptr, stream=0):
        """Blocks below the bound as records grouped by home rank, compact (tk_index_shard_filter_dev, region 0)."""
        _lib.check(_lib.lib().tk_index_shard_filter_dev(
            self._h, int(slot), nq, int(k), int(n_probes), int(pass_1 or 0), int(capacity),
            scan_ptr, bound_ptr, counts_ptr, records_ptr, 0, None, None, stream))

    def shard_finish_filtered_dev(self, slot, qn_ptr, nq, k, n_probes, pass_1, records_ptr,
                                  n_records, out_ptr, flag_ptr, stream=0):
        """Received compact records -> rows, replay, rescoring (tk_index_shard_finish_filtered_dev)."""
        _lib.check(_lib.lib().tk_index_shard_finish_filtered_dev(
            self._h, int(slot), qn_ptr, nq, int(k), int(n_probes), int(pass_1 or 0), records_ptr,
            int(n_records), None, 0, out_ptr, flag_ptr, stream))

    def shard_plain(self, k, n_probes, pass_1=None):
        """Does the two-phase scan with the matrix-core kernel apply (tk_index_shard_plain)?"""
        r = _lib.lib().tk_index_shard_plain(self._h, int(k), int(n_probes), int(pass_1 or 0))
        if r < 0:
            _lib.check(r)
        return bool(r)

    def shard_scan_first_dev(self, slot, qn_ptr, qpq_ptr, qpq_is_f64, nq, k, n_probes, pass_1, capacity,
                             send_ptr, flag_ptr, bound_ptr, stream=0, probes_all_ptr=None):
        """Phase 1 of the two-phase sharded scan: first slots exactly + their bound
        (tk_index_shard_scan_first_dev); the caller min-reduces the bound over the ranks."""
        _lib.check(_lib.lib().tk_index_shard_scan_first_dev(
            self._h, int(slot), qn_ptr, qpq_ptr, int(bool(qpq_is_f64)), nq, int(k), int(n_probes),
            int(pass_1 or 0), probes_all_ptr, int(capacity), send_ptr, flag_ptr, bound_ptr, stream))

    def shard_scan_rest_dev(self, slot, nq, k, n_probes, pass_1, capacity, send_ptr, bound_ptr, stream=0):
        """Phase 2: the slots behind the first, on the plain kernel where the reduced bound allows
        (tk_index_shard_scan_rest_dev)."""
        _lib.check(_lib.lib().tk_index_shard_scan_rest_dev(
            self._h, int(slot), nq, int(k), int(n_probes), int(pass_1 or 0), int(capacity), send_ptr,
            bound_ptr, stream))

    def shard_plain_stats(self, slot=0):
        """What the slot's last two-phase scan did on this rank (tk_index_shard_plain_stats)."""
        o = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_shard_plain_stats(self._h, int(slot), _lib.ptr(o, _lib._i64p)))
        return dict(plain_pairs=int(o[0]), plain_tiles=int(o[1]), exact_pair_records_behind_first=int(o[2]),
                    plain_queries=int(o[3]))

    def shard_filter_regions_dev(self, slot, nq, k, n_probes, pass_1, capacity, scan_ptr, bound_ptr,
                                 counts_ptr, records_ptr, region, flag_ptr, acc_ptr=None, stream=0):
        """... into fixed regions of `region` records per home rank (tk_index_shard_filter_dev, region >= 1)."""
        _lib.check(_lib.lib().tk_index_shard_filter_dev(
            self._h, int(slot), nq, int(k), int(n_probes), int(pass_1 or 0), int(capacity),
            scan_ptr, bound_ptr, counts_ptr, records_ptr, int(region), flag_ptr, acc_ptr, stream))

    def shard_finish_regions_dev(self, slot, qn_ptr, nq, k, n_probes, pass_1, records_ptr,
                                 counts_recv_ptr, region, out_ptr, flag_ptr, stream=0):
        """Received regions + their counts on the device -> rows, replay, rescoring
        (tk_index_shard_finish_filtered_dev with the received counts)."""
        _lib.check(_lib.lib().tk_index_shard_finish_filtered_dev(
            self._h, int(slot), qn_ptr, nq, int(k), int(n_probes), int(pass_1 or 0), records_ptr,
            0, counts_recv_ptr, int(region), out_ptr, flag_ptr, stream))

    def replay_stats(self):
        """What the lane replays of the probed lists did since set_option(OPT_REPLAY_COUNT, 1) / the last call
        (tk_index_replay_stats; synchronises): insert rounds over all waves, the most one wave ran, waves,
        and under `segments` the refills of the per-lane rings, summed over the waves (the lane replay without a
        duplicate test; the forms with one: 16-block segments walked)."""
        o = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_replay_stats(self._h, _lib.ptr(o, _lib._i64p)))
        return dict(rounds=int(o[0]), max_rounds_of_a_wave=int(o[1]), waves=int(o[2]), segments=int(o[3]))

    def twin_table_width(self):
        """Other copies listed per stored row (tk_index_twin_table): 0 = no table (distinct labels, ...)."""
        w = np.zeros(1, np.int32)
        _lib.check(_lib.lib().tk_index_twin_table(self._h, None, _lib.ptr(w, _lib._i32p), None, None))
        return int(w[0])

    def twin_table(self):
        """(list, offset) of every stored row's other copies, two (rows, w) int32 arrays (tk_index_twin_table):
        what the lane replay decides `insert`'s duplicate test from where labels repeat (build n_probes >= 2).
        w = 0: no table."""
        rows, w = np.zeros(1, np.int64), np.zeros(1, np.int32)
        _lib.check(_lib.lib().tk_index_twin_table(self._h, _lib.ptr(rows, _lib._i64p), _lib.ptr(w, _lib._i32p), None, None))
        tl = np.zeros((int(rows[0]), int(w[0])), np.int32)
        to = np.zeros_like(tl)
        if tl.size:
            _lib.check(_lib.lib().tk_index_twin_table(self._h, None, None, _lib.ptr(tl, _lib._i32p), _lib.ptr(to, _lib._i32p)))
        return tl, to

    def reserve(self, nq, k, n_probes, pass_1=None):
        _lib.check(_lib.lib().tk_index_reserve(self._h, nq, int(k), int(n_probes), int(pass_1 or 0)))

    def set_pipeline(self, depth):
        """Number of batches in flight for query_batch_dev (see tinyknn_hip.h)."""
        _lib.check(_lib.lib().tk_index_set_pipeline(self._h, int(depth)))

    def set_option(self, option, value):
        """Per-index A/B and test options (tk_index_set_option): _lib.OPT_PAIR_NQ (batches of up to this many queries
        replay their heaps one query per wave, heap in registers: 8192 one batch at a time, at most 4096 per launch pipelined),
        _lib.OPT_LABELS24, _lib.OPT_SCAN_FORM, _lib.OPT_RESCORE_FORM, _lib.OPT_PLAIN_LIMIT, _lib.OPT_REPLAY_LAZY,
        _lib.OPT_REPLAY_COUNT, _lib.OPT_REPLAY_TWIN, _lib.OPT_TWIN_VOUCH (include/tinyknn_hip.h describes each)."""
        _lib.check(_lib.lib().tk_index_set_option(self._h, int(option), int(value)))

    def set_coalesce(self, n):
        """2: pairs of consecutive query_batch_dev calls run as one batch (tk_index_set_coalesce);
        the first call of a pair is held until the second arrives (join() launches it alone).  A
        held call has enqueued nothing: a `done_event` passed to it is recorded only once the partner
        call or join() has run — do not wait on it before (pending() > 0 says work is still owed)."""
        _lib.check(_lib.lib().tk_index_set_coalesce(self._h, int(n)))

    def join(self, stream=0):
        _lib.check(_lib.lib().tk_index_join(self._h, stream))

    def plain_stats(self):
        """What the plain (matrix-core) scan did for the last batch (tk_index_plain_stats)."""
        o = np.zeros(8, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_plain_stats(self._h, _lib.ptr(o, _lib._i64p)))
        return dict(plain_units=int(o[0]), plain_pairs=int(o[1]), exact_pair_records=int(o[2]),
                    head_pair_records=int(o[3]), flagged_queries=int(o[4]), plain_unit_chunk_pairs=int(o[5]),
                    state=("probe", "wait", "on", "paused")[int(o[6]) & 3], pause_left=int(o[7]))

    def last_replay(self):
        """Which heap replay the last batch took for its probed lists (tk_index_last_replay; nothing is waited for):
        form (_lib.REPLAY_*; -1 before the first batch) and its name, lane replay lazy, register heap on label24
        entries, twin table width used."""
        o = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.lib().tk_index_last_replay(self._h, _lib.ptr(o, _lib._i64p)))
        form = int(o[0])
        return dict(form=form, name=_lib.REPLAY_NAMES[form] if 0 <= form < len(_lib.REPLAY_NAMES) else None,
                    lazy=int(o[1]), labels24=int(o[2]), twin_w=int(o[3]))

    def quiesce(self):
        """Wait for everything enqueued and forget its completion events (before a stream
        capture of the pipelined mode: tinyknn_hip.h, tk_index_quiesce)."""
        _lib.check(_lib.lib().tk_index_quiesce(self._h))

    def set_heap_mode(self, mode):
        """0: automatic (small batches: one query per wave with the heap in registers — _lib.OPT_PAIR_NQ; else one
        query per lane), 1: general wave kernel, 2: packed wave kernel, 3: the register heap for every batch size
        (heaps of up to 513 entries)."""
        _lib.check(_lib.lib().tk_index_set_heap_mode(self._h, int(mode)))

    def set_scan_mode(self, mode):
        """0: automatic, 1: query-major scan, 2: list-major scan (see tinyknn_hip.h)."""
        _lib.check(_lib.lib().tk_index_set_scan_mode(self._h, int(mode)))

    def set_plain_scan(self, on):
        """Probed lists behind the first ones as plain sums on the int8 matrix cores where that
        is provably the same replay (tinyknn_hip.h: tk_index_set_plain_scan); True = automatic
        (default: the path has to prove itself on a probe batch, and is paused while more than
        1 % of the queries need the exact re-scan), False = the exact kernel for every list,
        "always" = no pausing (tests, A/B).  Identical results in every mode."""
        mode = 2 if on == "always" else (0 if on else 1)
        _lib.check(_lib.lib().tk_index_set_plain_scan(self._h, mode))

    def set_profiling(self, on):
        _lib.check(_lib.lib().tk_index_set_profiling(self._h, int(on)))

    def last_profile(self):
        ms = (C.c_float * 8)()
        b = C.c_double()
        n = C.c_int32()
        _lib.check(_lib.lib().tk_index_last_profile(self._h, ms, C.byref(b), C.byref(n)))
        names = ["tables", "coarse_scan", "coarse_heap", "coarse_rescore", "scan", "heap", "rescore"]
        self.last_plain_kernel_ms = float(ms[7])      # the plain kernel alone (0: no recorded batch ran it)
        return dict(zip(names, list(ms)[:7])), b.value, n.value


class IVF:
    """reference: ivf.py:8-163"""

    # (class-level: an IVF pickled before these existed still reads them)
    all_centers = None      # fit's coarse centres
    list_columns = None     # (n_lists, kp) members per (list, column of the build's nearest); None: not recorded
    _build_device = None    # did build() search on the GPU?  None: not built here (fast_pq.device_build decides)
    store = None            # how the device keeps the rescoring vectors: None / "float32" / "float16" (build's store=)
    groups = None           # set_groups' host copy: (N,) int32 group id per row; None (and no instance attribute): none
    tags = None             # set_tags' host copy: (N,) uint64 tag mask per row; None (and no instance attribute): none
    values = None           # set_values' host copy: (N,) or (N, C) in the caller's dtype; None (and no instance attribute): none

    def __init__(self, metric, n_clusters, pq=None):
        assert metric in ["euclidean", "angular"]
        self.metric = metric
        self.pq = FastPQ(dims_per_block=2) if pq is None else pq
        assert self.pq.centers is None, "PQ should not be pre-fitted"
        self.pq_transformed_points = [None] * n_clusters
        self.pq_transformed_centers = [None] * n_clusters
        self.n_clusters = n_clusters
        self.ids = [None] * n_clusters
        self._dev = None

    # device handles are not picklable (the reference pickles (pq, ivf), bench.py:88-103)
    def __getstate__(self):
        self._require_host_copy("pickle")
        st = dict(self.__dict__)
        st["_dev"] = None
        return st

    def _require_host_copy(self, what):
        """An index built in HBM (build_resident) keeps its lists, codes and vectors on the
        device only; what needs them on the host says so instead of failing on a None."""
        if getattr(self, "pq_transformed_points", 0) is None:
            raise RuntimeError(f"IVF.{what}: this index was built in HBM (build_resident): its lists, codes "
                               "and vectors live on the device only — device_index().export_lists() / "
                               "read_rows() fetch them")

    # ---- offline ---------------------------------------------------------
    def fit(self, X, verbose=False):
        """Coarse k-means centres + PQ codebook.  reference: ivf.py:19-51"""
        import sklearn.cluster
        n, d = X.shape
        assert n >= 1
        with timer(verbose, "Fitting IVF cluster centers..."):
            km = sklearn.cluster.KMeans(n_clusters=self.n_clusters, n_init=1, verbose=verbose)
            if self.metric == "angular":
                # spherical data: normalise the points, then the centres (ivf.py:38-45)
                X = X / np.linalg.norm(X, axis=1, keepdims=True)
                self.all_centers = km.fit(X).cluster_centers_
                self.all_centers /= np.linalg.norm(self.all_centers, axis=1, keepdims=True)
            else:
                self.all_centers = km.fit(X).cluster_centers_
        with timer(verbose, "Fitting PQ to data..."):
            self.pq.fit(X, verbose=verbose)
        return self

    def build(self, X, n_probes=2, verbose=False, device=None, store=None):
        """Assign every point to its n_probes nearest centres and encode the lists.
        store="float16": the DEVICE copy of the rescoring vectors is kept in IEEE half (summed in float32;
        INTEGRATION.md §2g) — IVF.data, the lists and the codes are what store=None gives.  ValueError, before
        anything changes, for float64 X or a value whose half is not finite.
        reference: ivf.py:53-104.  device=True (default: fast_pq.device_build): the two
        searches — nearest centres per point, nearest centroid per block — run on the GPU
        (build.hip) and give the lists and codes numpy gives; everything else (normalisation,
        the rotation GEMM, grouping, packing) is the same host code."""
        assert n_probes <= self.n_clusters, (
            f"Can't assign points to {n_probes} clusters, as index only has {self.n_clusters}")
        device = _fp.device_build if device is None else device
        check_store(store)
        if store == "float16" and np.asarray(X).dtype != np.float32:
            half_rows(X, "IVF.build")                   # (raises: float64 vectors)
        data = X.copy()
        if self.metric == "angular":
            data /= np.linalg.norm(data, axis=1, keepdims=True)
        if store == "float16":
            half_rows(data, "IVF.build")                # the refusals only: the rounding happens at upload
        self._dev = None
        self.data = data
        self.store = store
        self._forget_row_attrs()
        with timer(verbose, "Computing nearest clusters..."):
            if device:
                nearest = self._nearest_on_device(data, n_probes)
            else:
                nearest = knn_brute(data, self.all_centers, k=n_probes, metric=self.metric)
        self._build_device = bool(device)
        with timer(verbose, "PQ Transforming active centers..."):
            self.active_centers = np.ascontiguousarray(
                self.all_centers[np.unique(nearest)], dtype=np.float32)
            self.pq_transformed_centers = self.pq.transform(self.active_centers, device=device)
        with timer(verbose, "Transforming points..."):
            n_active = self.active_centers.shape[0]
            if device:
                self._encode_lists_on_device(data, nearest, n_active)
            else:
                groups, self.ids = group_data_by_indices(data, nearest, n_active)
                for i in range(n_active):
                    self.pq_transformed_points[i] = self.pq.transform(groups[i])
        # members per (list, column of nearest): where add() puts a new row inside a list
        self.list_columns = np.stack([np.bincount(nearest[:, j], minlength=n_active)
                                      for j in range(nearest.shape[1])], axis=1).astype(np.int64)
        return self

    def _nearest_on_device(self, data, n_probes):
        """knn_brute(data, all_centers, n_probes, metric) (utils.py:66-86): whole 100-row
        chunks on the GPU, the last partial chunk — a differently shaped GEMM — in numpy."""
        Y = np.asarray(self.all_centers)
        exact_ok = (data.dtype == np.float32 and n_probes <= 9 and n_probes < len(Y)
                    and data.shape[1] <= 384
                    and (self.metric != "angular" or data.shape[1] <= 128))
        if not exact_ok:
            return knn_brute(data, Y, k=n_probes, metric=self.metric)
        y64 = Y.dtype != np.float32
        Y = np.ascontiguousarray(Y, dtype=np.float64 if y64 else np.float32)
        if self.metric == "angular":
            Y = Y / np.linalg.norm(Y, axis=1, keepdims=True)          # utils.py:75
        ynorm2 = np.ascontiguousarray(np.einsum("ij,ij->i", Y, Y))    # utils.py:80
        n = data.shape[0]
        full = n - n % 100
        out = np.zeros((n, n_probes), dtype=np.int64)
        X = np.ascontiguousarray(data[:full])
        _lib.check(_lib.lib().tk_assign_lists(
            _lib.ptr(X, _lib._f32p), full, X.shape[1], int(self.metric == "angular"),
            Y.ctypes.data, int(y64), ynorm2.ctypes.data, Y.shape[0], int(n_probes),
            _lib.ptr(out, _lib._i64p)))
        if full < n:
            out[full:] = knn_brute(data[full:], self.all_centers, k=n_probes, metric=self.metric)
        if n_probes > 2 and full > 0 and not self._assign_order_holds(data, out, n_probes, full):
            # numpy's argpartition leaves the ORDER of the first k unspecified; the device writes them
            # ascending by (value, index), which is what this host's numpy was seen to return — but that
            # is an implementation detail of its argselect (x86-simd-sort on AVX-512; other on AVX2, ARM,
            # older numpy).  Column order decides list order (group_data_by_indices appends column by
            # column): where this host's numpy orders differently, numpy's answer is the reference's.
            warnings.warn("tinyknn_amd: numpy.argpartition on this host does not return the first k ascending "
                          "(k = %d); list assignment falls back to numpy's knn_brute" % n_probes)
            return knn_brute(data, self.all_centers, k=n_probes, metric=self.metric)
        return out

    def _assign_order_holds(self, data, nearest, n_probes, full, chunks=24):
        """Self-check of the k > 2 device assignment against THIS host's numpy: whole 100-row chunks of
        knn_brute (utils.py:81-85 works in chunks of 100), spread over the data."""
        n_chunks = full // 100
        if n_chunks == 0:
            return True
        pick = np.unique(np.linspace(0, n_chunks - 1, min(chunks, n_chunks)).astype(np.int64))
        for c in pick:
            rows = slice(100 * int(c), 100 * int(c) + 100)
            want = knn_brute(data[rows], self.all_centers, k=n_probes, metric=self.metric)
            if not np.array_equal(want, nearest[rows]):
                return False
        return True

    def _labels_of(self, data, device):
        """(n, M) uint8 PQ labels of rows: padded, rotated on the host as the reference does (slabs of
        rows), nearest centroid per block (on the GPU where `device`)."""
        pq = self.pq
        dpb = pq.dims_per_block
        n, d = data.shape
        pad = (-d) % (dpad * dpb)
        M = pq.centers.shape[1] // dpb
        labels = np.empty((n, M), dtype=np.uint8)
        slab = 1 << 20
        for o in range(0, n, slab):
            rows = data[o:o + slab]
            if pad:
                rows = np.concatenate([rows, np.zeros((len(rows), pad), rows.dtype)], axis=1)
            if pq.R is not None:
                rows = rows @ pq.R.T
            labels[o:o + slab] = pq.encode_labels(rows, device)
        return labels

    def _encode_lists_on_device(self, data, nearest, n_active):
        """ivf.py:98-102 with ONE pass over the points: a row's code does not depend on the
        list it lands in, so all rows are encoded once (slabs of rows: pad, rotate on the
        host as the reference does, nearest centroids on the GPU) and the per-list arrays
        are gathered from the labels; the rows that pad a list to a multiple of 16 carry the
        code of the zero vector, as pad2 + transform give them (fast_pq.py:165)."""
        pq = self.pq
        n, d = data.shape
        dq = pq.centers.shape[1]
        labels = self._labels_of(data, True)
        zero = pq.encode_labels(np.zeros((16, dq), dtype=np.float64 if pq.R is not None else data.dtype),
                                True)[0]
        # grouping as group_data_by_indices does (utils.py:95-162), without copying the vectors
        assert 0 <= nearest.min() and nearest.max() < n_active       # utils.py:128
        ids = [[] for _ in range(n_active)]
        for j in range(nearest.shape[1]):
            col = nearest[:, j]
            order = np.argsort(col)
            uniq, counts = np.unique(col[order], return_counts=True)
            start = 0
            for g, cnt in zip(uniq, counts):
                ids[g].append(order[start:start + cnt])
                start += cnt
        self.ids = [np.hstack(i) if i else np.empty(0) for i in ids]
        for i in range(n_active):
            sel = self.ids[i].astype(np.int64)
            if len(sel) == 0:
                self.pq_transformed_points[i] = np.empty((0, d))     # fast_pq.py:162-163
                continue
            self.pq_transformed_points[i] = _pack_labels(labels[sel], zero)

    # ---- persistence ---------------------------------------------------------
    # The reference pickles (pq, ivf) (examples/bench.py:88-103); that works here too
    # (__getstate__ drops the device handle).  save/load is the flat form the device upload
    # wants: CSR offsets + one array per component, no Python objects.
    def save(self, path):
        """Flat binary (.npz): PQ codebook (+ rotation), coarse centres and their codes, list
        sizes, packed codes and ids of all lists concatenated list-major, rescoring vectors."""
        self._require_host_copy("save")
        L = len(self.active_centers)
        M = self.pq.centers.shape[1] // self.pq.dims_per_block
        tds = [self.pq_transformed_points[i] for i in range(L)]
        sizes = np.array([_stored(t) for t in tds], dtype=np.int64)
        codes = [t.packed for t in tds if _stored(t)]
        ids = [np.asarray(self.ids[i], dtype=np.int64)[:sizes[i]] for i in range(L)]
        extra = {} if self.pq.R is None else {"R": self.pq.R}
        if self.all_centers is not None:
            extra["all_centers"] = self.all_centers
        if self.list_columns is not None:
            extra["list_columns"] = self.list_columns
        if self.store is not None:          # (the vectors are written unrounded: the upload rounds again, same bits)
            extra["store"] = self.store
        extra.update((at.name, getattr(self, at.name)) for at in ROW_ATTRS if getattr(self, at.name) is not None)
        path = self._npz_path(path)
        np.savez(path, format_version=1, metric=self.metric, n_clusters=self.n_clusters,
                 use_kmeans=int(self.pq.use_kmeans), rotate_dim=-1 if self.pq.rotate_dim is None else int(self.pq.rotate_dim),
                 dims_per_block=self.pq.dims_per_block, pq_centers=self.pq.centers,
                 pq_centers_f_order=int(not self.pq.centers.flags.c_contiguous),
                 sqrt_n_blocks=self.pq.sqrt_n_blocks, active_centers=self.active_centers,
                 center_size=self.pq_transformed_centers.size,
                 center_codes=self.pq_transformed_centers.packed, list_sizes=sizes,
                 list_codes=(np.concatenate(codes) if codes else np.zeros((0, M), np.uint64)),
                 ids=(np.concatenate(ids) if ids else np.zeros(0, np.int64)), data=self.data, **extra)

    @staticmethod
    def _npz_path(path):
        """np.savez appends '.npz' to a path without that suffix; save and load agree on it."""
        path = str(path)
        return path if path.endswith(".npz") else path + ".npz"

    @classmethod
    def load(cls, path, data=None):
        """Inverse of save.  `data`: the rescoring vectors if the file was written without them
        being wanted twice (pass the array to avoid keeping two copies)."""
        z = np.load(cls._npz_path(path), allow_pickle=False)
        assert int(z["format_version"]) == 1
        pq = FastPQ(int(z["dims_per_block"]),
                    use_kmeans=bool(int(z["use_kmeans"])) if "use_kmeans" in z else True,
                    rotate_dim=(None if int(z["rotate_dim"]) < 0 else int(z["rotate_dim"])) if "rotate_dim" in z else 64)
        ivf = cls(str(z["metric"]), int(z["n_clusters"]), pq)
        c = z["pq_centers"]
        ivf.pq.centers = np.asfortranarray(c) if int(z["pq_centers_f_order"]) else c
        ivf.pq.sqrt_n_blocks = float(z["sqrt_n_blocks"])
        ivf.pq.R = z["R"] if "R" in z else None
        if "all_centers" in z:
            ivf.all_centers = z["all_centers"]
        ivf.active_centers = z["active_centers"]
        ivf.pq_transformed_centers = TransformedData(int(z["center_size"]), z["center_codes"])
        ivf.pq_transformed_points, ivf.ids = _split_lists(z["list_sizes"], z["list_codes"], z["ids"],
                                                          ivf.active_centers.shape[1])
        ivf.data = z["data"] if data is None else data
        # (files written before add() existed have no list_columns: add() recovers them)
        ivf.list_columns = z["list_columns"] if "list_columns" in z else None
        ivf.store = check_store(str(z["store"])) if "store" in z else None     # (files written before store= existed)
        for at in ROW_ATTRS:
            if at.name in z:
                setattr(ivf, at.name, np.ascontiguousarray(z[at.name], dtype=at.dtype))
        return ivf

    def build_resident(self, N, d, seed, centres=None, sigma=1.0, verbose=False, n_probes=1, store=None):
        """IVF.build(X, n_probes=1 or 2) (ivf.py:53-104) for N synthetic float32 vectors that are
        generated IN HBM (seeded, devbuild.hip) and never visit the host — the way the
        100M x 128 configuration is assembled.  Needs all_centers and a
        fitted pq (fit()).  Everything runs on the device: nearest centre per row, PQ codes,
        grouping by list (rows of a list in ascending row order, where numpy's unstable
        argsort leaves their order unspecified), packing.  The rotation of a rotated PQ is
        the device front end's float64 FMA chain, not numpy's DGEMM, so a code can differ
        from IVF.build's where that flips a nearest centroid.  Afterwards: active_centers,
        pq_transformed_centers and list_sizes on the host; data / ids / codes stay in HBM
        (device_index().export_lists() / read_rows() fetch them for a checker).
        store="float16": after the build (which reads the float32 rows) the vectors are narrowed to half in
        HBM (DeviceIndex.narrow: ValueError for a value whose half is not finite)."""
        assert self.pq.centers is not None and self.all_centers is not None
        check_store(store)
        with timer(verbose, "Generating vectors in HBM..."):
            dev = DeviceIndex.resident(self, N, d)
            dev.synth_data(seed, centres, sigma)
        if n_probes > 2:
            # no host fallback here: refuse k > 2 unless this host's numpy orders argpartition's first k
            # the way the device does (see _nearest_on_device), checked on generated rows
            probe = IVF(self.metric, self.n_clusters, FastPQ(self.pq.dims_per_block))
            probe.all_centers = self.all_centers
            rows = dev.read_rows(np.arange(min(N - N % 100, 2400), dtype=np.int64))
            if self.metric == "angular":
                rows = rows / np.linalg.norm(rows, axis=1, keepdims=True)
            got = probe._nearest_on_device(np.ascontiguousarray(rows, dtype=np.float32), n_probes)
            if len(rows) and not np.array_equal(got, knn_brute(rows, self.all_centers, k=n_probes, metric=self.metric)):
                raise RuntimeError("build_resident(n_probes=%d): numpy.argpartition on this host does not return the "
                                   "first k ascending, which the device assignment assumes for k > 2; build with "
                                   "n_probes <= 2 or on the host (IVF.build)" % n_probes)
        with timer(verbose, "Building lists on the device..."):
            L = dev.build_dev(self.all_centers, n_probes)
        if store == "float16":
            dev.narrow()
        self.store = store
        self.active_centers, cc = dev.export_centers()
        self.pq_transformed_centers = TransformedData(L, cc)
        self.list_sizes = dev.list_sizes
        self.list_columns = dev.list_columns()
        self.data = ResidentData(dev)
        self.ids = self.pq_transformed_points = None
        self._forget_row_attrs()
        self._dev = dev
        return self

    # ---- growth ------------------------------------------------------------
    def add(self, X, verbose=False, groups=None, tags=None, values=None):
        """Append the rows of X with ids N .. N + n - 1 (returns self).  groups: the new rows' group ids, needed (and
        only taken) where the index has groups (set_groups): ValueError otherwise, before anything changes.  tags: the
        new rows' tag masks, by the same rule where the index has tags (set_tags); values: the new rows' values, (n,) or
        (n, C) as the index's, by the same rule where it has values (set_values).  The index afterwards is the one its own
        build would make over (old rows, X): new rows are prepared as the build prepared its rows (dtype of
        IVF.data, normalisation, padding, rotation, assignment, PQ codes); every list keeps its old members in
        place, and with n_probes = kp lists per row list l's column-j block becomes old_j ++ new_j (new_j: the
        new rows whose j-th nearest centre is l, ascending).  An index built by build_resident is then
        byte-identical to build_resident over all rows; against IVF.build the order inside a list is
        unspecified for kp = 1, as numpy's argsort leaves it.  Rows that activate centres past the active
        ones append lists (the centres stay a prefix, or AssertionError as in build).  The device index is
        updated in place: allowed sets made before fail afterwards.  A refused call changes nothing."""
        self._require_device_free()
        X = np.asarray(X)
        d = self.data.shape[1]
        if X.ndim != 2 or X.shape[1] != d:
            raise AssertionError(f"IVF.add: X must have shape (n, {d}), got {X.shape}")
        new = self._new_row_attrs("add", len(X), dict(groups=groups, tags=tags, values=values), needed=True)
        if self.all_centers is None:
            raise AssertionError("IVF.add: the index has no all_centers (fit, or a file written with them)")
        if len(X) == 0:
            return self
        if self.pq_transformed_points is None:
            self._add_resident(X, verbose)
        else:
            self._add_host(X, verbose)
        self._store_row_attrs(new, lambda old, rows: np.concatenate([old, rows]))
        return self

    # ---- the row attributes (ROW_ATTRS: groups, tags, values), one body for each thing done with all three ----
    def _host_rows(self, at, x, n, what, like=None):
        """The host copy of attribute `at` for n rows, from the caller's x: as the device takes it (at.rows), or where
        the host keeps something else (values: the caller's array, checked; host_values) that — like the index's own."""
        return at.rows(x, n, what) if at.host is None else at.host(x, n, what, like)

    def _set_rows(self, at, x):
        """set_groups / set_tags / set_values: x checked, handed to the device index where there is one, kept (a copy
        wherever it shares memory with x); None clears."""
        a = None if x is None else self._host_rows(at, x, len(self.data), f"IVF.set_{at.name}")
        if self._dev is not None:                # (a list-sharded index raises here, before the host copy changes)
            getattr(self._unsharded_device_index(), f"set_{at.name}")(a)
        if a is None:
            self.__dict__.pop(at.name, None)
        else:
            setattr(self, at.name, a.copy() if np.shares_memory(a, x) else a)
        return self

    def _forget_row_attrs(self):
        """(a build: attributes belong to the rows they were set for)"""
        for at in ROW_ATTRS:
            self.__dict__.pop(at.name, None)

    def _new_row_attrs(self, what, n, given, needed):
        """The first half of add / update, before anything changes: `given` {name: the n new rows' attribute, or None}
        against what the index has -> {name: host rows} of the ones given.  An attribute the index lacks is not taken;
        `needed`: one it has must be given."""
        new = {}
        for at in ROW_ATTRS:
            x, have = given[at.name], getattr(self, at.name)
            if have is None and x is not None:
                raise ValueError(f"IVF.{what}: {at.name}= on an index without {at.name} (set_{at.name} first)")
            if needed and have is not None and x is None:
                raise ValueError(f"IVF.{what}: this index has {at.name} (set_{at.name}): pass the new rows' with {at.name}=")
            if x is not None:
                new[at.name] = self._host_rows(at, x, n, f"IVF.{what}: {at.name}", like=have)
        return new

    def _store_row_attrs(self, new, merge):
        """The second half: merge(the host copy, the new rows) is the host copy, and the device's — which covers the
        old rows only — is set again for all."""
        for at in ROW_ATTRS:
            if at.name in new:
                setattr(self, at.name, merge(getattr(self, at.name), new[at.name]))
                if self._dev is not None:
                    getattr(self._dev, f"set_{at.name}")(getattr(self, at.name))

    def _require_device_free(self, what="add", doing="adding rows to"):
        if self._dev is not None and _dev_is_sharded(self._dev):
            raise NotImplementedError(f"IVF.{what}: this index has been list-sharded in place; {doing} a "
                                      "list-sharded index is not supported")

    def _add_resident(self, X, verbose):
        dev = self._dev
        cols = dev.list_columns()
        with timer(verbose, "Adding rows on the device..."):
            L = dev.add(np.ascontiguousarray(X, dtype=np.float32), cols.shape[1], normalise=self.metric == "angular",
                        all_centers=self.all_centers)
        self.active_centers, cc = dev.export_centers()
        self.pq_transformed_centers = TransformedData(L, cc)
        self.list_sizes = dev.list_sizes
        self.list_columns = dev.list_columns()
        self.data = ResidentData(dev)
        return self

    def _lists_per_row(self):
        if self.list_columns is not None:
            return self.list_columns.shape[1]
        stored = sum(_stored(t) for t in self.pq_transformed_points[:len(self.active_centers)])
        return max(1, stored // max(1, len(self.data)))

    def _list_columns_now(self, kp):
        """list_columns, recovered for a file written without them: the list sizes (kp = 1), or the build's own
        assignment over IVF.data (knn_brute, ivf.py:85) counted per column."""
        cols = self.list_columns
        if cols is None:
            L = len(self.active_centers)
            if kp == 1:
                cols = np.array([_stored(t) for t in self.pq_transformed_points[:L]], dtype=np.int64).reshape(L, 1)
            else:
                near = knn_brute(np.asarray(self.data), self.all_centers, k=kp, metric=self.metric)
                cols = np.stack([np.bincount(near[:, j], minlength=L) for j in range(kp)], axis=1).astype(np.int64)
            self.list_columns = cols
        return cols

    def _prepared_rows(self, X, what, row0, verbose):
        """New rows as the host build prepares its rows (ivf.py:77-102), for add and update on a host-built index ->
        (rows in IVF.data's dtype, normalised; nearest (n, kp); PQ labels (n, M); the members per (list, column)
        now; lists afterwards; the active centres and their codes afterwards — the index's own where no list is
        new).  A half store refuses a row whose half is not finite here, naming row0 + its row, before anything
        changes (the device rounds its copy)."""
        device = _fp.device_build if self._build_device is None else self._build_device
        kp = self._lists_per_row()
        L0 = len(self.active_centers)
        cols0 = self._list_columns_now(kp)
        new = np.array(X, dtype=self.data.dtype, copy=True)         # ivf.py:77-79: X's dtype, normalised
        if self.metric == "angular":
            new /= np.linalg.norm(new, axis=1, keepdims=True)
        if self.store == "float16":
            half_rows(new, f"IVF.{what}", row0=row0)
        with timer(verbose, "Computing nearest clusters..."):
            if device:
                nearest = self._nearest_on_device(new, kp)
            else:
                nearest = knn_brute(new, self.all_centers, k=kp, metric=self.metric)
            nearest = np.ascontiguousarray(nearest, dtype=np.int64).reshape(len(new), kp)
        used = np.union1d(np.arange(L0), np.unique(nearest))
        assert used.max() < len(used), ("a centre that received no row precedes one that did: the reference's "
                                        "group_data_by_indices asserts max(index) < n_active (utils.py:128)")
        L1 = len(used)
        with timer(verbose, "Transforming points..."):
            labels = self._labels_of(new, device)
        active, centers = self.active_centers, self.pq_transformed_centers
        if L1 > L0:
            active = np.ascontiguousarray(self.all_centers[:L1], dtype=np.float32)
            centers = self.pq.transform(active, device=device)
        return new, nearest, labels, cols0, L1, active, centers

    def _add_host(self, X, verbose):
        new, nearest, labels, cols0, L1, active, centers = self._prepared_rows(X, "add", len(self.data), verbose)
        kp, grown = nearest.shape[1], L1 > len(self.active_centers)

        def on_device(dev):
            dev.add(new, kp, nearest=nearest, labels=labels, list_columns=cols0,
                    all_centers=self.all_centers if grown else None,
                    center_codes=centers.packed if grown else None)
            return True

        self._change_lists("add", on_device, lambda: self._splice(new, nearest, labels, cols0, L1))
        self.active_centers, self.pq_transformed_centers = active, centers
        self.data = np.concatenate([self.data, new])
        return self

    def _change_lists(self, what, on_device, in_numpy):
        """The second half of add / remove on a host-built index.  With a device index the change is made there
        (on_device(dev) -> did the lists change?) and mirrored back; without one in_numpy() -> (codes per list, ids
        per list, list_columns).  Leaves the timings in last_<what>_ms and the lists in self."""
        dev, t0 = self._dev, time.perf_counter()
        if dev is not None:
            changed = on_device(dev)
            t1 = time.perf_counter()
            if changed:
                pts, idl = _split_lists(*dev.export_lists(), self.data.shape[1])
                cols = dev.list_columns()
            ms = {"device": 1e3 * (t1 - t0), "host": 1e3 * (time.perf_counter() - t1) if changed else 0.0}
        else:
            changed = True
            pts, idl, cols = in_numpy()
            ms = {"device": 0.0, "host": 1e3 * (time.perf_counter() - t0)}
        setattr(self, f"last_{what}_ms", ms)
        if changed:
            self._install_lists(pts, idl, cols)

    def _install_lists(self, pts, idl, cols):
        """The codes and ids of lists 0 .. len(pts) - 1 (lists past the old active ones are new) and the members per
        (list, column) become the index's."""
        self.pq_transformed_points = pts + list(self.pq_transformed_points[len(pts):])
        self.ids = idl + list(self.ids[len(idl):])
        self.list_columns = cols

    def _splice(self, new, nearest, labels, cols0, L1, old=None, new_ids=None):
        """The lists after add() in numpy: list l's column-j block = old_j ++ (new rows with nearest[:, j] == l,
        ascending); untouched lists are kept as they are.  old: (codes per list, ids per list) to splice into
        (None: the index's own); new_ids: the labels the new rows carry (None: N .. N + n - 1)."""
        kp = nearest.shape[1]
        L0 = len(cols0)
        old_pts, old_idl = (self.pq_transformed_points, self.ids) if old is None else old
        if new_ids is None:
            new_ids = len(self.data) + np.arange(len(new), dtype=np.int64)
        zero = self._zero_label()
        cols1 = np.zeros((L1, kp), dtype=np.int64)
        cols1[:L0] = cols0
        per = [[None] * kp for _ in range(L1)]
        for j in range(kp):
            order = np.argsort(nearest[:, j], kind="stable")
            cnt = np.bincount(nearest[:, j], minlength=L1)
            cols1[:, j] += cnt
            starts = np.concatenate([[0], np.cumsum(cnt)])
            for l in np.nonzero(cnt)[0]:
                per[l][j] = order[starts[l]:starts[l + 1]]
        pts, idl = [], []
        for l in range(L1):
            old_t = old_pts[l] if l < L0 else None
            old_ids = np.asarray(old_idl[l], dtype=np.int64) if l < L0 else np.zeros(0, np.int64)
            if all(p is None for p in per[l]):
                pts.append(old_t)
                idl.append(old_idl[l])
                continue
            old_n = len(old_ids)
            old_lab = (unpack(old_t.packed)[:old_n] if old_n else np.zeros((0, labels.shape[1]), np.uint8))
            lab_parts, id_parts, o = [], [], 0
            for j in range(kp):
                oc = int(cols0[l, j]) if l < L0 else 0
                lab_parts.append(old_lab[o:o + oc])
                id_parts.append(old_ids[o:o + oc])
                o += oc
                if per[l][j] is not None:
                    lab_parts.append(labels[per[l][j]])
                    id_parts.append(new_ids[per[l][j]])
            pts.append(_pack_labels(np.concatenate(lab_parts), zero))
            idl.append(np.concatenate(id_parts))
        return pts, idl, cols1

    # ---- replacement --------------------------------------------------------
    def update(self, ids, X, verbose=False, groups=None, tags=None, values=None):
        """Give the stored rows `ids` (n row ids in [0, N), pairwise distinct) the new vectors X (n, d), ids kept
        (returns self).  The index afterwards is the one that remove(ids) then add(X) gives on the same index, with
        two differences: the added row N + i carries the label ids[i] in every list, and its prepared vector sits in
        row ids[i] of IVF.data and of the device store, not behind the old rows — N, len(IVF.data) and the store's
        size do not change.  The rows are prepared exactly as add prepares them (dtype of IVF.data, normalisation,
        padding, rotation, assignment, PQ labels; a half store refuses a row whose half is not finite before anything
        changes).  List l's column-j block becomes (old_j minus the rows in ids, old order kept) ++ (the rows i whose
        j-th nearest centre is l, ascending i, labelled ids[i]): a row removed earlier is stored again, a row whose
        nearest list does not change moves to the end of its column block, a list that empties stays with its
        centre, rows that activate centres past the active ones append lists (the prefix rule and AssertionError of
        add); list_columns follows.  groups: new group ids for those rows, only taken where the index has groups;
        without it they keep their groups; tags: the same for tag masks (set_tags), values: for values (set_values).  A duplicate or out-of-range id raises
        ValueError.  The device index is
        updated in place (one pass over its codes, one scatter into its vectors): batches in flight finish on the
        old lists and vectors, allowed sets made before fail afterwards.  A refused call changes nothing."""
        self._require_device_free("update", "replacing rows of")
        ids = update_ids(ids, len(self.data))
        X = np.asarray(X)
        d = self.data.shape[1]
        if X.ndim != 2 or X.shape != (len(ids), d):
            raise AssertionError(f"IVF.update: X must have shape ({len(ids)}, {d}), got {X.shape}")
        new = self._new_row_attrs("update", len(X), dict(groups=groups, tags=tags, values=values), needed=False)
        if self.all_centers is None:
            raise AssertionError("IVF.update: the index has no all_centers (fit, or a file written with them)")
        if len(ids) == 0:
            return self
        if self.pq_transformed_points is None:
            self._update_resident(ids, X, verbose)
        else:
            self._update_host(ids, X, verbose)
        def put(old, rows):
            a = old.copy()
            a[ids] = rows
            return a

        self._store_row_attrs(new, put)
        return self

    def _update_resident(self, ids, X, verbose):
        dev = self._dev
        t0 = time.perf_counter()
        with timer(verbose, "Replacing rows on the device..."):
            L = dev.update(ids, np.ascontiguousarray(X, dtype=np.float32), dev.list_columns().shape[1],
                           normalise=self.metric == "angular", all_centers=self.all_centers)
        self.last_update_ms = {"device": 1e3 * (time.perf_counter() - t0), "host": 0.0}
        self.active_centers, cc = dev.export_centers()
        self.pq_transformed_centers = TransformedData(L, cc)
        self.list_sizes = dev.list_sizes
        self.list_columns = dev.list_columns()
        return self

    def _update_host(self, ids, X, verbose):
        new, nearest, labels, cols0, L1, active, centers = self._prepared_rows(X, "update", 0, verbose)
        kp, grown = nearest.shape[1], L1 > len(self.active_centers)
        if not self.data.flags.writeable:       # (before anything changes: the rows are overwritten in place below)
            self.data = self.data.copy()

        def on_device(dev):
            with timer(verbose, "Replacing rows on the device..."):
                dev.update(ids, new, kp, nearest=nearest, labels=labels, list_columns=cols0,
                           all_centers=self.all_centers if grown else None,
                           center_codes=centers.packed if grown else None)
            return True

        def in_numpy():
            dead = np.zeros(len(self.data), dtype=bool)
            dead[ids] = True
            pts, idl, cols = self._filter_lists(dead, cols0)
            return self._splice(new, nearest, labels, cols, L1, old=(pts, idl), new_ids=ids)

        self._change_lists("update", on_device, in_numpy)
        self.active_centers, self.pq_transformed_centers = active, centers
        self.data[ids] = new
        return self

    # ---- removal -----------------------------------------------------------
    def remove(self, ids_or_mask, verbose=False):
        """Delete every stored copy of the rows named by ids_or_mask (row ids, duplicates allowed, or a bool mask of
        length N) from the lists (returns self).  Ids are stable: IVF.data keeps every row (a removed row's vector
        stays as dead weight) and a later add() still appends ids N ..  Every list keeps its surviving members in
        their old order: list l's column-j block becomes old_j minus the removed rows (list_columns follows).  A
        list that empties stays, with its centre.  Ids in range but no longer stored are ignored; an id outside
        [0, N) raises and changes nothing.  The result is the index over the lists filtered so — not what
        allowed= the survivors gives on the old index (the reference's heap bound is taken per 16-row block, and
        compaction moves the blocks).  The device index is updated in place: allowed sets made before fail."""
        self._require_device_free("remove", "removing rows from")
        rows = removal_rows(ids_or_mask, len(self.data))
        if len(rows) == 0:
            return self
        if self.pq_transformed_points is None:
            return self._remove_resident(rows, verbose)
        return self._remove_host(rows, verbose)

    def _remove_resident(self, rows, verbose):
        dev = self._dev
        t0 = time.perf_counter()
        with timer(verbose, "Removing rows on the device..."):
            dev.remove(rows)
        self.last_remove_ms = {"device": 1e3 * (time.perf_counter() - t0), "host": 0.0}
        self.list_sizes = dev.list_sizes
        self.list_columns = dev.list_columns()
        return self

    def _remove_host(self, rows, verbose):
        kp = self._lists_per_row()
        cols0 = self._list_columns_now(kp)      # (before: their recovery from IVF.data assumes every row stored)
        dead = np.zeros(len(self.data), dtype=bool)
        dead[rows] = True

        def on_device(dev):
            with timer(verbose, "Removing rows on the device..."):
                return dev.remove(rows, list_columns=cols0) > 0     # (0: nothing stored was named, nothing changed)

        self._change_lists("remove", on_device, lambda: self._filter_lists(dead, cols0))
        return self

    def _filter_lists(self, dead, cols0):
        """The lists after remove() in numpy: every list's surviving entries in their old order (each column block
        shrinks in place), repacked with the zero vector's code in the padding rows; untouched lists are kept."""
        L, kp = cols0.shape
        d = self.data.shape[1]
        zero = self._zero_label()
        cols1 = np.array(cols0, dtype=np.int64, copy=True)
        pts, idl = [], []
        for l in range(L):
            t = self.pq_transformed_points[l]
            n_l = _stored(t)
            ids = np.asarray(self.ids[l])[:n_l]
            keep = ~dead[ids.astype(np.int64)]
            if keep.all():
                pts.append(t)
                idl.append(self.ids[l])
                continue
            cols1[l] = np.bincount(np.repeat(np.arange(kp), cols0[l])[keep], minlength=kp)
            n1 = int(keep.sum())
            idl.append(ids[keep])
            if n1 == 0:
                pts.append(np.empty((0, d)))      # as FastPQ.transform of no rows (fast_pq.py:162-163)
                continue
            pts.append(_pack_labels(unpack(t.packed)[:n_l][keep], zero))
        return pts, idl, cols1

    def _zero_label(self):
        """The zero vector's labels (the rows that pad a list to a multiple of 16, fast_pq.py:165)."""
        z = self.pq.transform(np.zeros((1, self.data.shape[1]), dtype=self.data.dtype), device=self._build_device)
        return unpack(z.packed)[1]

    # ---- queries (GPU) -----------------------------------------------------
    def device_index(self):
        if self._dev is None:
            dev = DeviceIndex(self)
            for at in ROW_ATTRS:
                if getattr(self, at.name) is not None:
                    getattr(dev, f"set_{at.name}")(getattr(self, at.name))
            self._dev = dev
        return self._dev

    def set_groups(self, groups):
        """One group id per row — tenant, language, category: a 1-d integer array of length N with ids in
        [0, 2**31 - 1) — for the `group=` argument of query / query_batch; None clears.  TypeError for
        another kind of value, ValueError for another length or an id outside.  IVF.groups is the host copy (int32);
        save / load and pickling carry it."""
        return self._set_rows(GROUPS, groups)

    def set_tags(self, tags):
        """One 64-bit tag mask per row — categories, ACL principals: a 1-d integer array of length N, uint64 or any
        integer dtype with every value in [0, 2**64), bit t set = the row carries tag t, 0 = no tag — for the `tags=`
        argument of query / query_batch; None clears.  TypeError for another kind of value, ValueError
        for another length or a value outside.  IVF.tags is the host copy (uint64); save / load and pickling carry it."""
        return self._set_rows(TAGS, tags)

    def set_values(self, values):
        """1 to 4 numeric columns per row — a timestamp, a price, a version: (N,) or (N, C) of ONE integer or floating
        dtype (float16 / 32 / 64) — for the `between=` argument of query / query_batch; None clears.
        TypeError for another kind of value, ValueError for another length, more than 4 columns, a NaN or a uint64
        above 2**63 - 1.  IVF.values is the host copy in the caller's dtype; save / load and pickling carry it."""
        return self._set_rows(VALUES, values)

    def _ranges(self, between, nq):
        """`between=` checked against IVF.values before anything runs (query_ranges): the keys the device takes"""
        if self.values is None:
            raise ValueError("between= on an index without values (set_values first)")
        return query_ranges(between, nq, 1 if self.values.ndim == 1 else self.values.shape[1],
                            value_kind(self.values.dtype))

    def _unsharded_device_index(self):
        dev = self.device_index()
        if _dev_is_sharded(dev):
            raise RuntimeError("this IVF's device index has been list-sharded in place (ListShardedIndex on an "
                               f"index built in HBM: rank {dev.rank} of {dev.world}); query it through the "
                               "ListShardedIndex")
        return dev

    def _prepare(self, qs):
        """Host side of ivf.py:125-128: float32, metric normalisation (numpy, in
        place for a contiguous float32 input as in the reference), padding and the
        optional float64 rotation of the table-build query."""
        pq = self.pq
        dq = pq.centers.shape[1]
        d = qs.shape[1]
        pad = (-d) % (dpad * pq.dims_per_block)
        R = pq.R
        if R is not None and (min(R.shape) < 2 or R.dtype != np.float64):
            # 1-row / 1-column products take other numpy code paths (dot, no BLAS)
            qn, qp = _front.numpy_prepare(qs, self.metric == "angular", R, pad)
        else:
            # the same two BLAS calls numpy makes per row, from a thread pool (_front.py)
            qn, qp = _front.prepare(qs, self.metric == "angular", R, pad)
        assert qp.shape[1] == dq
        return qn, qp

    def knn_brute(self, qs, k, *, allowed=None, exclude=None, group=None, tags=None, tags_mode="any", between=None,
                  return_distances=False):
        """The exact k nearest rows of IVF.data for raw queries, under the restrictions of query_batch (DeviceIndex.
        knn_brute on the prepared queries: an angular index ranks its normalised rows): (nq, k) int64 ids ascending
        by (part, row), ending in -1 where fewer than k rows pass; with return_distances (ids, part): also the float32
        `part` values (DeviceIndex.knn_brute_dist: numpy's knn_brute values, not the rescoring's distances), +inf beside -1.  The ground truth of
        restricted recall; allowed= with a mask of the surviving rows is the truth after remove().  allowed: a bool
        mask of length N or row ids, not an AllowSet.  Not for a list-sharded index."""
        if isinstance(allowed, AllowSet):
            raise TypeError("knn_brute: allowed= takes a bool mask of length N or row ids; an AllowSet is laid out by "
                            "list position")
        if between is not None:
            self._ranges(between, len(qs))
        if tags is not None:
            tag_mode_of(tags_mode)
        dev = self._unsharded_device_index()
        qn, _ = self._prepare(np.array(qs, dtype=np.float32, order="C", copy=True))
        call = dev.knn_brute_dist if return_distances else dev.knn_brute
        return call(qn, k, allowed=allowed, exclude=exclude, group=group, tags=tags, tags_mode=tags_mode, between=between)

    def radius_search(self, qs, radius, *, allowed=None, exclude=None, group=None, tags=None, tags_mode="any",
                      between=None, sort=True, max_results=None, n_probes=None):
        """Every row of IVF.data within a radius of each raw query, exactly, under the restrictions of query_batch
        (DeviceIndex.radius_brute on the prepared queries): CSR (lims, ids, part) — lims (nq + 1,)
        int64, query i's hits ids[lims[i]:lims[i + 1]] (int64) with their float32 `part` values, knn_brute's, beside
        them: part(i, j) <= radius[i], float32, inclusive, however many rows that is.  With sort=True (default) a list
        is ascending by (part, row) — knn_brute(k)'s ids are its first k entries at radius = the k-th part — and
        byte-identical from run to run; sort=False leaves the order inside a list unspecified.
        An angular index ranks its normalised rows, as knn_brute does: part = 2 - 2 cos, so radius = 2 - 2c asks for
        every row with cosine >= c.  radius: a scalar or (nq,), cast with np.float32; +inf: every passing row;
        negative: normally an empty list; NaN or a wrong length: ValueError.  max_results (default 1 << 26, < 2**31):
        a larger total raises ValueError with the true total, returns nothing and leaves the index usable — a list is
        never cut silently.  The vectors of removed rows stay in HBM: allowed= with a mask of the surviving rows is the
        truth after remove().  allowed: a bool mask of length N or row ids, not an AllowSet.  Float32 vectors,
        d <= 128; not for a list-sharded index.
        n_probes=P (an int >= 1; DESIGN §3.20, DeviceIndex.radius_probe): the rows of the P lists the query probes
        alone — FAISS's range_search on an IVF index — instead of all N: CSR (lims, ids, dist).  The probes are
        query_batch's for P; the candidates are the rows stored in the distinct probed lists, each once, so a row taken
        out by remove() is never listed (no allowed= needed, unlike the call over all rows); `dist` is the rescoring's
        squared distance — query_batch(return_distances=True)'s and knn_group's values bit for bit: float32, float64
        on float64 vectors — compared with float32(radius) inclusively.  It is not `part`: the two round differently
        and agree exactly on integer data, so a row on the boundary of one call may be outside the other's.  Every
        store (float32, float16, float64 vectors) and d <= 4096.  n_probes=None is the call over all rows, as it
        always was."""
        if n_probes is not None:
            qn, qp, dev = self._radius_front("radius_search", qs, radius, allowed, tags, tags_mode, between, n_probes)
            return dev.radius_probe(qn, qp, radius, n_probes, allowed=allowed, exclude=exclude, group=group, tags=tags,
                                    tags_mode=tags_mode, between=between, sort=sort, max_results=max_results)
        qn, dev = self._radius_front("radius_search", qs, radius, allowed, tags, tags_mode, between)
        return dev.radius_brute(qn, radius, allowed=allowed, exclude=exclude, group=group, tags=tags,
                                tags_mode=tags_mode, between=between, sort=sort, max_results=max_results)

    def radius_count(self, qs, radius, *, allowed=None, exclude=None, group=None, tags=None, tags_mode="any",
                     between=None, n_probes=None):
        """How many rows radius_search would list per raw query: (nq,) int64, from its count pass alone — no limit
        (the totals are summed in int64), half the work and no sort.  Arguments as radius_search's, n_probes=
        included (DeviceIndex.radius_probe_count)."""
        if n_probes is not None:
            qn, qp, dev = self._radius_front("radius_count", qs, radius, allowed, tags, tags_mode, between, n_probes)
            return dev.radius_probe_count(qn, qp, radius, n_probes, allowed=allowed, exclude=exclude, group=group,
                                          tags=tags, tags_mode=tags_mode, between=between)
        qn, dev = self._radius_front("radius_count", qs, radius, allowed, tags, tags_mode, between)
        return dev.radius_count(qn, radius, allowed=allowed, exclude=exclude, group=group, tags=tags,
                                tags_mode=tags_mode, between=between)

    def _radius_front(self, call, qs, radius, allowed, tags, tags_mode, between, n_probes=None):
        """knn_brute's early refusals in its order, then the radius', before any device call; the prepared queries
        (qn, dev) — with n_probes (qn, q_pq, dev)"""
        if isinstance(allowed, AllowSet):
            raise TypeError(f"{call}: allowed= takes a bool mask of length N or row ids; an AllowSet is laid out by "
                            "list position")
        if between is not None:
            self._ranges(between, len(qs))
        if tags is not None:
            tag_mode_of(tags_mode)
        query_radius(radius, len(qs))
        if n_probes is not None and int(n_probes) < 1:
            raise ValueError(f"n_probes: at least 1, got {int(n_probes)}")
        dev = self._unsharded_device_index()
        qn, qp = self._prepare(np.array(qs, dtype=np.float32, order="C", copy=True))
        return (qn, dev) if n_probes is None else (qn, qp, dev)

    def knn_group(self, qs, k, group, *, allowed=None, exclude=None, tags=None, tags_mode="any", between=None,
                  return_distances=False):
        """The exact k nearest stored rows inside each raw query's own group (DeviceIndex.knn_group on the prepared
        queries): (nq, k) int64 ids ascending by (distance, row id), ending in -1 where fewer than k
        rows pass; with return_distances (ids, dists), the distances of query_batch(return_distances=True), +inf
        beside -1.  group: an int or one id >= 0 per query.  The cost follows the group's size — the call for small
        groups, where the probed lists hold too few of a group's rows; knn_brute(group=) is the one for large groups,
        query_batch(group=, exact_below=) routes a batch by size.  The other restrictions as knn_brute's; allowed: a
        bool mask of length N or row ids, not an AllowSet.  Not for a list-sharded index."""
        if isinstance(allowed, AllowSet):
            raise TypeError("knn_group: allowed= takes a bool mask of length N or row ids; an AllowSet is laid out by "
                            "list position")
        if between is not None:
            self._ranges(between, len(qs))
        if tags is not None:
            tag_mode_of(tags_mode)
        group = query_groups(group, len(qs))
        if len(group) and int(group.min()) < 0:
            raise AssertionError("knn_group: group= needs a group id >= 0 for every query (-1, any group, is "
                                 "knn_brute's or query_batch's to answer)")
        dev = self._unsharded_device_index()
        qn, _ = self._prepare(np.array(qs, dtype=np.float32, order="C", copy=True))
        return dev.knn_group(qn, k, group, allowed=allowed, exclude=exclude, tags=tags, tags_mode=tags_mode,
                             between=between, return_distances=return_distances)

    def knn_between(self, qs, k, between, *, allowed=None, exclude=None, group=None, tags=None, tags_mode="any",
                    return_distances=False):
        """The exact k nearest stored rows inside each raw query's value range (DeviceIndex.knn_between on the
        prepared queries): (nq, k) int64 ids ascending by (distance, row id), ending in -1 where fewer
        than k rows pass; with return_distances (ids, dists), the distances of query_batch(return_distances=True),
        +inf beside -1.  between: (lo, hi) as query_batch's; every query must bound a column (ValueError).  The cost
        follows the number of rows the query's narrowest column admits — the call for narrow ranges, where the probed
        lists hold too few passing rows; knn_brute(between=) is the one for wide ranges, query_batch(between=,
        exact_below=) routes a batch by length.  The other restrictions as knn_brute's; allowed: a bool mask of length
        N or row ids, not an AllowSet.  Not for a list-sharded index."""
        if isinstance(allowed, AllowSet):
            raise TypeError("knn_between: allowed= takes a bool mask of length N or row ids; an AllowSet is laid out by "
                            "list position")
        if between is None:
            raise TypeError("knn_between: between= is required: a pair (lo, hi)")
        free = np.flatnonzero(unbounded_queries(self._ranges(between, len(qs))))
        if len(free):
            raise ValueError(f"knn_between: query {int(free[0])} bounds no column (an unrestricted query is knn_brute's "
                             "or query_batch's to answer)")
        if tags is not None:
            tag_mode_of(tags_mode)
        if group is not None:
            group = query_groups(group, len(qs))
        dev = self._unsharded_device_index()
        qn, _ = self._prepare(np.array(qs, dtype=np.float32, order="C", copy=True))
        return dev.knn_between(qn, k, between, allowed=allowed, exclude=exclude, group=group, tags=tags,
                               tags_mode=tags_mode, return_distances=return_distances)

    def allow(self, ids_or_mask):
        """Prepare an allowed set (a bool mask over the N rows, or row ids) for `allowed=`: made once on the
        device, reused across calls; .close() frees it, len() = allowed stored rows."""
        return self._unsharded_device_index().allow(ids_or_mask)

    def query(self, q, k, n_probes=1, pass_1=None, *, allowed=None, return_distances=False, exclude=None, group=None,
              tags=None, tags_mode="any", between=None, per_group=None):
        """Top-k ids for one query.  reference: ivf.py:106-163
        per_group: the most rows of any one group (set_groups) among the ids returned, 0 or None for no cap; fewer
        than k ids come back where the candidates run out of groups — raise pass_1 or n_probes then.
        between: (lo, hi), the inclusive interval of values (set_values) the query's rows must lie in: each end None
        (unbounded), a number, or one entry per column.
        tags: the 64-bit tag mask the query is restricted by under tags_mode — "any": rows that carry one of its tags
        (set_tags), "all": rows that carry every one; 0 or None for any row.
        group: the group of rows (set_groups) the query may return, -1 or None for any.
        exclude: a row id the query may not return, or None.
        allowed: the rows it may return (a bool mask of length N, row ids, or allow()'s set) — the reference's
        query with `insert` only for those labels.
        return_distances: (ids, dists) of the same length — the exact squared distance of each id to the
        (normalised) query, as the rescoring computed it."""
        if between is not None:
            if not isinstance(between, (tuple, list)) or len(between) != 2:
                raise TypeError("between: a pair (lo, hi), each None, a number or an array")
            between = tuple(b if b is None or np.ndim(b) == 0 else np.asarray(b).reshape(1, -1) for b in between)
            self._ranges(between, 1)                # (refused before anything runs)
        if per_group is not None:
            query_caps(np.asarray(per_group).reshape(-1), 1)
        q = np.ascontiguousarray(q, dtype=np.float32)
        assert self.data.shape[1] == q.shape[0]
        qn, qp = self._prepare(q[None, :])
        dev = self._unsharded_device_index()
        one = {w: None if x is None else np.asarray(x).reshape(1)
               for w, x in (("exclude", exclude), ("group", group), ("tags", tags), ("per_group", per_group))}
        got = dev.query_batch(qn, qp, k, n_probes, pass_1, allowed=allowed, return_distances=return_distances,
                              tags_mode=tags_mode, between=between, **one)
        out, dist = (got[0][0], got[1][0]) if return_distances else (got[0], None)
        keep = out != -1 if out[-1] == -1 else slice(None)
        return (out[keep], dist[keep]) if return_distances else out[keep]

    def query_rows(self, rows, k, n_probes=1, pass_1=None, *, exclude_self=True, allowed=None,
                   return_distances=False, per_group=None):
        """The neighbours of stored rows: (len(rows), k) ids padded with -1 — (ids, dists) with return_distances —
        of the queries float32(data[rows]), made on the device without a second normalisation.
        per_group: as query_batch's.
        exclude_self: a row's own copies are never inserted, so it is not among its neighbours; its twin with an equal
        vector is.  rows: ids in [0, N), duplicates allowed (ValueError outside).  A removed row is still a vector:
        it can be a query row, and nothing is masked for it."""
        if per_group is not None:
            per_group = query_caps(per_group, len(rows))
        return self._unsharded_device_index().query_rows(rows, k, n_probes, pass_1, exclude_self=exclude_self,
                                                         allowed=allowed, return_distances=return_distances,
                                                         per_group=per_group)

    def knn_graph(self, k, n_probes=1, pass_1=None, *, chunk=10000, return_distances=False):
        """query_rows over every row, itself left out: (N, k) ids — (ids, dists) with return_distances.  Chunks of
        `chunk` rows run through the pipelined device calls in pairs (set_pipeline(3), set_coalesce(2)): row ids are
        generated on the device, results copied back per group of chunks; the settings found are restored."""
        import torch
        dev = self._unsharded_device_index()
        N, d, dq = dev.N, dev.d, dev.dq
        chunk = int(max(1, min(chunk, dev.max_sub_batch(k, n_probes, pass_1), max(N, 1))))
        f64q, f64d = dev.rotated(), dev._f64
        ids = np.full((N, k), -1, dtype=np.int64)
        dist = np.full((N, k), np.inf, dtype=np.float64 if f64d else np.float32) if return_distances else None
        depth0, coalesce0 = dev.pipeline_settings()
        group = 8       # chunks in flight: their buffers are the library's until join()
        cuda = torch.device("cuda", torch.cuda.current_device())
        bufs = [dict(rows=torch.empty(chunk, dtype=torch.int64, device=cuda),
                     qn=torch.empty((chunk, d), dtype=torch.float32, device=cuda),
                     qp=torch.empty((chunk, dq), dtype=torch.float64 if f64q else torch.float32, device=cuda),
                     ids=torch.empty((chunk, k), dtype=torch.int64, device=cuda),
                     dist=torch.empty((chunk, k), dtype=torch.float64 if f64d else torch.float32, device=cuda)
                     if return_distances else None) for _ in range(min(group, -(-N // chunk)))]
        try:
            dev.set_pipeline(3)
            dev.set_coalesce(2)
            st = torch.cuda.current_stream().cuda_stream
            for g0 in range(0, N, group * chunk):
                spans = []
                for b in bufs:
                    o = g0 + len(spans) * chunk
                    if o >= N:
                        break
                    n = min(N, o + chunk) - o
                    torch.arange(o, o + n, out=b["rows"][:n])
                    dev.gather_queries_dev(b["rows"].data_ptr(), n, b["qn"].data_ptr(), b["qp"].data_ptr(), st)
                    dev.query_batch_dev(b["qn"].data_ptr(), b["qp"].data_ptr(), f64q, n, k, n_probes,
                                        b["ids"].data_ptr(), pass_1, st,
                                        dist_ptr=None if dist is None else b["dist"].data_ptr(),
                                        exclude_ptr=b["rows"].data_ptr())
                    spans.append((o, n))
                dev.join(st)
                torch.cuda.current_stream().synchronize()
                for b, (o, n) in zip(bufs, spans):
                    ids[o:o + n] = b["ids"][:n].cpu().numpy()
                    if dist is not None:
                        dist[o:o + n] = b["dist"][:n].cpu().numpy()
        finally:
            dev.join(0)
            dev.set_pipeline(depth0)
            dev.set_coalesce(coalesce0)
        return (ids, dist) if return_distances else ids

    def query_batch(self, qs, k, n_probes=1, pass_1=None, fast=False, *, allowed=None, return_distances=False,
                    exclude=None, group=None, tags=None, tags_mode="any", between=None, per_group=None,
                    exact_below=None):
        """(nq, d) queries -> (nq, k) int64 ids, rows padded with -1 when the
        reference would return fewer than k ids.  (The reference's README shows a
        2-d `ivf.query(queries, ...)` that its code does not support; this is that
        call.)  fast=True: normalisation, padding and rotation run on the device instead
        of numpy's per-query BLAS calls (35 ms per 10 000 queries on the host) — within
        4 float32 ulp of their normalised rows, so a rare id can differ from the
        reference's; the default is exact.
        return_distances: ((nq, k) ids, (nq, k) exact squared distances), INTEGRATION.md §2f.
        exclude: a 1-d integer array, the row each query may not return or -1; not with fast=True.
        group: an int for every query, or a 1-d integer array with one entry per query: the group of rows (set_groups)
        it may return, -1 for any; not with fast=True.
        tags: an int for every query, or a 1-d integer array with one 64-bit mask per query: the tags (set_tags) its
        rows must carry — one of them with tags_mode "any", every one with "all" — 0 for any row; not
        with fast=True.
        between: (lo, hi), the inclusive interval of values (set_values) each query's rows must lie in, per column:
        each end None (unbounded), a number for every query, (nq,) for one column, (nq, C), or (C,) where nq != C
        (DESIGN §3.14); not with fast=True.
        per_group: an int for every query, or a 1-d integer array with one entry per query: the most rows of any one
        group (set_groups) among a query's ids, 0 for no cap — "the k nearest documents, not chunks".  The rescoring's
        ranking is walked and a candidate kept while fewer than that many of its group have been kept; the candidates
        are the heap's pass_1 or (n_probes + 1) k + 1, so with a small cap a row can end in -1 before k ids: raise
        pass_1 or n_probes for a wider pool, nothing widens it by itself; not with fast=True.
        exact_below: None, or a number of rows T, with group=: the queries whose group carries fewer than T rows
        (group_sizes) are answered exactly by knn_group under the call's other restrictions — the probed lists hold
        too few rows of a small group — and all others, every query with group -1 among them, by this call without
        it; the rows come back in query order, both parts with the same kind of distance.  With
        between= and no group=: the queries that bound a column and whose range's span (range_sizes) is shorter than T
        rows are answered exactly by knn_between, all others by this call without it; with both, the
        routing is by group.  Not with per_group= (inside one group the cap would just cut k), an AllowSet or
        fast=True."""
        if exact_below is not None:
            if fast:
                raise NotImplementedError("IVF.query_batch: fast=True with exact_below= is not supported; "
                                          "use the exact default (fast=False)")
            return self._query_batch_exact_below(qs, k, n_probes, pass_1, exact_below, allowed, return_distances,
                                                 exclude, group, tags, tags_mode, between, per_group)
        # what fast=True does not take: the first of these that is asked for is the one refused
        asked = [word for word, given in (("per_group=", per_group is not None),
                                          ("between=", between is not None), ("tags=", tags is not None),
                                          ("group=", group is not None), ("exclude=", exclude is not None),
                                          ("return_distances=True", return_distances), ("allowed=", allowed is not None))
                 if given]
        if fast and asked:
            if asked == ["allowed="]:       # (the one refusal that comes behind a list-sharded index's own)
                self._unsharded_device_index()
            raise NotImplementedError(f"IVF.query_batch: fast=True with {asked[0]} is not supported; "
                                      "use the exact default (fast=False)")
        if between is not None:
            self._ranges(between, len(qs))
        if tags is not None:
            tag_mode_of(tags_mode)
        if per_group is not None:
            per_group = query_caps(per_group, len(qs))
        self._unsharded_device_index()
        if asked:
            qs = np.array(qs, dtype=np.float32, order="C", copy=True)
            if exclude is not None and np.ndim(exclude) == 1 and len(exclude) != len(qs):
                raise ValueError(f"exclude: one entry per query ({len(qs)}), got {len(exclude)}")
            if group is not None:
                group = query_groups(group, len(qs))
            if tags is not None:
                tags = query_tags(tags, len(qs))
            qn, qp = self._prepare(qs)
            return self.device_index().query_batch(qn, qp, k, n_probes, pass_1, allowed=allowed,
                                                   return_distances=return_distances, exclude=exclude, group=group,
                                                   tags=tags, tags_mode=tags_mode, between=between,
                                                   per_group=per_group)
        if fast:
            return self.device_index().query_batch_raw(qs, k, n_probes, pass_1)
        R = self.pq.R
        if _front.bind() and (R is None or (min(R.shape) >= 2 and R.dtype == np.float64)):
            # exact: chunks stream through preparation (numpy's BLAS on a thread pool),
            # pinned H2D, the kernels and D2H, overlapped
            return self.device_index().query_raw(qs, k, n_probes, pass_1)
        qs = np.array(qs, dtype=np.float32, order="C", copy=True)
        qn, qp = self._prepare(qs)
        return self.device_index().query_batch(qn, qp, k, n_probes, pass_1)

    def _query_batch_exact_below(self, qs, k, n_probes, pass_1, exact_below, allowed, return_distances, exclude, group,
                                 tags, tags_mode, between, per_group):
        """query_batch(group= / between=, exact_below=T): the refusals, the split — by group size where group= is given,
        else by the length of the range's span — the two calls on their subsets (an empty part runs nothing), the rows
        put back in query order"""
        if group is None and between is None:
            raise ValueError("exact_below= routes queries by the size of their group or the length of their range: it "
                             "needs group= or between=")
        if per_group is not None:
            raise ValueError("exact_below= with per_group= is not supported: inside one group the cap would just cut k")
        if isinstance(allowed, AllowSet):
            raise TypeError("exact_below=: allowed= takes a bool mask of length N or row ids here (knn_group's); an "
                            "AllowSet is laid out by list position")
        if isinstance(exact_below, (bool, np.bool_)) or not isinstance(exact_below, (int, np.integer)):
            raise TypeError("exact_below: None or an int, the number of rows below which a group is searched exactly")
        if exact_below < 0:
            raise ValueError("exact_below: a number of rows >= 0")
        nq = len(qs)
        by_group = group is not None
        if by_group:
            group = query_groups(group, nq)
        if between is not None:
            keys = self._ranges(between, nq)
            cols = 1 if self.values.ndim == 1 else self.values.shape[1]
            between = (_bound_array(between[0], "lo", nq, cols), _bound_array(between[1], "hi", nq, cols))
        if tags is not None:
            tag_mode_of(tags_mode)
            tags = query_tags(tags, nq)
        if exclude is not None and (np.ndim(exclude) != 1 or len(exclude) != nq):
            raise ValueError(f"exclude: a 1-d array with one entry per query ({nq})")
        dev = self._unsharded_device_index()
        qs = np.array(qs, dtype=np.float32, order="C", copy=True)
        sizes = np.zeros(nq, dtype=np.int64)
        if by_group:
            grouped = np.flatnonzero(group >= 0)
            if len(grouped):
                sizes[grouped] = dev.group_sizes(group[grouped])
            routed = (group >= 0) & (sizes < int(exact_below))
        else:       # by the span a range would walk; a query that bounds no column is the restricted call's
            bounded = np.flatnonzero(~unbounded_queries(keys))
            if len(bounded):
                sizes[bounded] = dev.range_sizes(tuple(None if b is None else b[bounded] for b in between),
                                                 len(bounded))[0]
            routed = ~unbounded_queries(keys) & (sizes < int(exact_below))
        parts = exact_below_parts(routed, between)

        def sub(x, rows):
            return None if x is None else np.asarray(x)[rows]

        ids = np.full((nq, k), -1, dtype=np.int64)
        dist = None
        for exact, rows, btw in parts:
            if exact and by_group:
                got = self.knn_group(qs[rows], k, group[rows], allowed=allowed, exclude=sub(exclude, rows),
                                     tags=sub(tags, rows), tags_mode=tags_mode, between=btw,
                                     return_distances=return_distances)
            elif exact:
                got = self.knn_between(qs[rows], k, btw, allowed=allowed, exclude=sub(exclude, rows),
                                       tags=sub(tags, rows), tags_mode=tags_mode, return_distances=return_distances)
            else:
                got = self.query_batch(qs[rows], k, n_probes, pass_1, allowed=allowed,
                                       return_distances=return_distances, exclude=sub(exclude, rows),
                                       group=sub(group, rows), tags=sub(tags, rows), tags_mode=tags_mode, between=btw)
            if return_distances:
                if dist is None:
                    dist = np.full((nq, k), np.inf, dtype=got[1].dtype)
                ids[rows], dist[rows] = got
            else:
                ids[rows] = got
        if return_distances and dist is None:       # (no query at all)
            dist = np.full((nq, k), np.inf, dtype=np.float64 if np.asarray(self.data).dtype == np.float64 else np.float32)
        return (ids, dist) if return_distances else ids
