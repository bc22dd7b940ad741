"""The shapes at which the build path (build.hip: list assignment, PQ encoding) is checked, and the inputs of
every case made from a seed, so that the CPU leg (oracle == numpy, tests/test_build_path.py) and the GPU leg
(device == oracle, tests/test_build_gpu.py) score the same rows against the same centres.

An assignment case names the kernel form tk_launch_assign picks for it (build.hip); the form is part of the
test id, so a failure says which kernel is wrong.  Shapes are the smallest at which a form can still go wrong:
every d branch (odd d, d < 8, d % 8, the 128/129 switch between the MFMA and the VALU form, the d <= 384
limit), L around the 32-column MFMA tile and the 512/1024-centre pass of the VALU forms, n around the rows
per workgroup (4, 8, 16, 128) — never a workload."""
import zlib
from collections import namedtuple

import numpy as np

# the forms of tk_launch_assign, and the centres each scores per pass (256 threads x C centres; the MFMA form
# walks 32-column tiles and is given the 512 of the C = 2 forms)
MFMA = "assign_mfma_kernel<1>"
F1, D1 = "assign_kernel<float,16,2,1>", "assign_kernel<double,16,2,1>"
F2, D2 = "assign_kernel<float,8,4,3>", "assign_kernel<double,8,4,3>"
F9, D9 = "assign_kernel<float,4,4,9>", "assign_kernel<double,4,2,9>"
PASS_WIDTH = {MFMA: 512, F1: 512, D1: 512, F2: 1024, D2: 1024, F9: 1024, D9: 512}


def form_of(y64, k, d):
    """The kernel tk_launch_assign runs (build.hip, the dispatch at its end)."""
    if not y64 and k == 1 and d <= 128:
        return MFMA
    if k == 1:
        return D1 if y64 else F1
    if k == 2:
        return D2 if y64 else F2
    return D9 if y64 else F9


# (form, float64 centres?, k, the two values of d of the L, n and tie sweeps: a small one, one past 128 where the form has it)
FORMS = [
    (MFMA, False, 1, (9, 128)),
    (F1, False, 1, (129, 384)),
    (D1, True, 1, (7, 130)),
    (F2, False, 2, (17, 257)),
    (D2, True, 2, (33, 129)),
    (F9, False, 3, (3, 130)),
    (F9, False, 9, (17, 257)),
    (D9, True, 3, (9, 129)),
    (D9, True, 9, (33, 384)),
]
D_ALL = (1, 2, 3, 7, 8, 9, 17, 33, 127, 128, 129, 130, 257, 384)
N_ALL = (1, 3, 15, 17, 31, 33, 127, 129, 333)

# metric: "euclidean"; "angular" (tk_assign_lists normalises the rows: normalise_rows_kernel, d <= 128);
# "unit": rows and centres the test normalised itself, scored as euclidean (angular past 128 dims)
# ties: None (random rows, tie-free for d >= 3) or one of TIE_KINDS (assign_inputs says what each places where)
# seed: from the case's own fields, so that a case keeps its data when the table around it changes
AssignCase = namedtuple("AssignCase", "form y64 k d L n metric ties seed")
TIE_KINDS = ("halfint", "dups", "zero_early", "zero_late", "ulp")


def _id(c):
    return "%s-k%d-d%d-L%d-n%d-%s-%s" % (c.form, c.k, c.d, c.L, c.n, c.metric, c.ties or "random")


def _valid_d(form, d):
    return (d <= 128) if form == MFMA else (d >= 129) if form == F1 else True


def assign_cases():
    out, seen = [], set()

    def add(form, y64, k, d, L, n, metric="euclidean", ties=None):
        assert form_of(y64, k, d) == form and L > k
        key = (form, k, d, L, n, metric, ties)
        if key not in seen:
            seen.add(key)
            out.append(AssignCase(form, y64, k, d, L, n, metric, ties, zlib.crc32(repr(key).encode()) & 0x7FFFFFFF))

    for form, y64, k, ds in FORMS:
        # every d, 33 centres (two MFMA tiles, the second one with one column), 37 rows (a partial workgroup
        # at 4, 8 and 16 rows; an MFMA wave of 5 rows)
        for d in D_ALL:
            if _valid_d(form, d):
                add(form, y64, k, d, 33, 37)
                add(form, y64, k, d, 33, 37, "angular" if d <= 128 else "unit")
        # L around the tile and the pass; the pass boundary +-1
        w = PASS_WIDTH[form]
        for L in (k + 1, 31, 32, 33, 257, w - 1, w, w + 1):
            for d in ds:
                add(form, y64, k, d, L, 37)
        # n around the rows per workgroup
        for n in N_ALL:
            add(form, y64, k, ds[0], 65, n)
        add(form, y64, k, ds[1], 65, 333, "angular" if ds[1] <= 128 else "unit")
        # ties inside a tile / pass (L = 40), across tiles (300), across the passes of the C = 2 forms (600) and
        # of the C = 4 forms (1100)
        for kind in TIE_KINDS:
            if kind.startswith("zero") and k != 2:          # (the branches of dumb_select's second pass)
                continue
            for L in (40, 300, 600, 1100):
                for d in ds:
                    add(form, y64, k, d, L, 129, "euclidean", kind)
        # centres one ulp apart under the device's own row normalisation: d < 8, d % 8 != 0, d % 8 == 0
        for d in (3, 7, 12, 33, 128):
            if _valid_d(form, d):
                add(form, y64, k, d, 40, 129, "angular", "ulp")
    return out


ASSIGN_CASES = assign_cases()
ASSIGN_IDS = [_id(c) for c in ASSIGN_CASES]


def _unit(A):
    return A / np.linalg.norm(A, axis=1, keepdims=True)


def assign_inputs(c, whole_chunks=False):
    """(X float32 (n, d), Y (L, d) float32 or float64) of a case.  whole_chunks: all the rows drawn (n rounded
    up to a multiple of 100, numpy's knn_brute chunk) — the first n of them are the rows without it."""
    rng = np.random.RandomState(c.seed)
    n_all = -(-c.n // 100) * 100
    ydt = np.float64 if c.y64 else np.float32
    X = rng.randn(n_all, c.d).astype(np.float32)
    Y = rng.randn(c.L, c.d).astype(ydt)
    if c.metric == "unit":
        X, Y = _unit(X), _unit(Y)
    L = c.L
    if c.ties:
        Y = Y.astype(np.float32).astype(ydt)                    # rows can lie exactly ON float64 centres too
    if c.ties == "halfint":
        # integer rows, half-integer centres: every product and sum is exact, equal distances are equal bits
        X = np.round(1.5 * X)
        Y = (np.round(2 * Y) / 2).astype(ydt)
    elif c.ties == "dups":
        # duplicated centres in one pass / tile and in different ones (centre 0 among them), rows ON centres
        for a, b in ((9, 3), (7, 0), (32, 3), (256, 0), (512, 1), (1024, 2), (L - 1, 0)):
            if a < L:
                Y[a] = Y[b]
        pick = np.concatenate([[0, 3, 7, 9, 1, 2, L - 1, 32 % L, 256 % L, 512 % L, 1024 % L],
                               rng.randint(L, size=n_all)])[:n_all]
        half = n_all // 2
        X[:half] = Y[pick[:half]].astype(np.float32)
        X[half:half + 20] = X[:20] + np.float32(0.25)           # near, not on, the duplicated centres
    elif c.ties == "ulp":
        # centres in pairs one ulp apart in one coordinate: which of a pair is nearer (or whether they tie) hangs
        # on the last bit of every operation — |x|^2, |y|^2, the FMA chain, the row norm — not on the data
        for i in range(0, L - 1, 2):
            Y[i + 1] = Y[i]
            j = rng.randint(c.d)
            Y[i + 1, j] = np.nextafter(Y[i, j], ydt(np.inf))
    elif c.ties in ("zero_early", "zero_late"):
        # dumb_select's second pass (k = 2) scans 1 .. m0-1, centre 0, m0+1 .. L-1.  Centre 0 and its duplicate
        # b sit next to centre a (half a unit away; every other centre is about sqrt(2 d) away):
        #   rows on centre a: the nearest is not 0, and centre 0 ties with the runner-up b — b wins when it comes
        #                     before a ("early"), 0 wins when b comes after a ("late", b in the last tile / pass)
        #   rows on centre 0: the nearest is 0 (first occurrence), the runner-up its duplicate
        #   rows on centre g: the nearest is not 0, neither is the tied pair of runners-up (g + 1, L - 3)
        a, g = 20, 11
        b = 5 if c.ties == "zero_early" else L - 2
        step = np.zeros(c.d, dtype=ydt)
        step[0] = 0.5
        Y[0] = Y[a] + step
        Y[b] = Y[0]
        Y[g + 1] = Y[g] - step
        Y[L - 3] = Y[g + 1]
        rows = [Y[a]] * 8 + [Y[0]] * 8 + [Y[g]] * 8
        for i, r in enumerate(rows):
            X[i] = r.astype(np.float32)
            X[i + len(rows)] = (r + (i % 4) * 0.125 * step).astype(np.float32)      # towards / past the neighbour
    X = np.ascontiguousarray(X, dtype=np.float32)
    Y = np.ascontiguousarray(Y, dtype=ydt)
    return (X if whole_chunks else np.ascontiguousarray(X[:c.n])), Y


def oracle_metric(c):
    """The metric the references (oracle.assign, knn_brute) are asked for: "unit" rows are scored as euclidean."""
    return "angular" if c.metric == "angular" else "euclidean"


# ---------------------------------------------------------------------------------------------------------------
# PQ encoding: encode_pq_kernel<T, DPB>, DPB in 1, 2, 4, 8 or 0 (the generic form: dims_per_block 16)
EncodeCase = namedtuple("EncodeCase", "dpb dq n f64 ties seed")
ENC_DQ = {1: (4, 12, 20, 36, 16, 32, 128),          # a strip is 16 elements: tails of 4 and 12, exact strips
          2: (8, 24, 40, 16, 32, 128),
          4: (20, 36, 16, 32, 128),
          8: (24, 40, 16, 32, 128),
          16: (16, 32, 64, 128)}
ENC_N = (1, 15, 17, 63, 65, 255, 257, 700)          # a wave is 64 rows, a workgroup 256
ENC_LDS_MAX_DQ = 336        # dims_per_block 1: 16*M*2*4 (codebook) + 4*64*17*8 (strips) + 4*64*M (labels) <= 160 KiB


def _enc_form(dpb, f64):
    return "encode_pq_kernel<%s,%d>" % ("double" if f64 else "float", 0 if dpb == 16 else dpb)


def _enc_id(c):
    return "%s-dpb%d-dq%d-n%d-%s" % (_enc_form(c.dpb, c.f64), c.dpb, c.dq, c.n, c.ties or "random")


def encode_cases():
    out = []

    def add(dpb, dq, n, f64, ties):
        out.append(EncodeCase(dpb, dq, n, f64, ties, zlib.crc32(repr((dpb, dq, n, f64, ties)).encode()) & 0x7FFFFFFF))

    for dpb, dqs in ENC_DQ.items():
        for f64 in (False, True):
            for dq in dqs:
                add(dpb, dq, 257, f64, None)
                add(dpb, dq, 65, f64, "ties")
                add(dpb, dq, 129, f64, "ulp")
            for n in ENC_N:
                if n != 257:
                    add(dpb, dqs[1], n, f64, "ties" if n in (15, 63, 700) else None)
    for f64 in (False, True):
        add(1, ENC_LDS_MAX_DQ, 257, f64, None)
    return out


ENCODE_CASES = encode_cases()
ENCODE_IDS = [_enc_id(c) for c in ENCODE_CASES]


def encode_inputs(c):
    """(centers (16, dq) float32, rows (n, dq) float32 or float64: padded, rotated rows as encode_labels takes them)"""
    rng = np.random.RandomState(c.seed)
    X = rng.randn(c.n, c.dq).astype(np.float64 if c.f64 else np.float32)
    centers = (rng.randn(16, c.dq) * 0.8).astype(np.float32)
    if c.n >= 3:
        X[c.n // 2] = 0                                     # a zero row (what pads a list)
    if c.ties == "ulp":
        # centroids in pairs one ulp apart in every coordinate: the label hangs on the last bit of every operation
        centers[1::2] = np.nextafter(centers[0::2], np.float32(np.inf))
    elif c.ties:
        # exact ties between centroids: integer rows, half-integer centroids, a duplicated centroid (the first
        # occurrence wins)
        X[: max(1, c.n // 2)] = np.round(X[: max(1, c.n // 2)])
        centers = (np.round(centers * 2) / 2).astype(np.float32)
        centers[5] = centers[3]
        centers[15] = centers[0]
    return centers, X
