"""CPU stand-in for the per-rank device engine of ListShardedIndex (test infrastructure:
built on the oracle).  `scan` scores the segments this rank owns with the oracle's
estimate_pq and packs them exactly where shard_positions_kernel would; `finish` checks
every received segment of the home queries against a local recomputation and answers them
with the oracle's full query — so a misplaced, missing or foreign byte in the exchange
fails the test.  Filtered exchange: `bound` replays the first probed list with the oracle's
query_pq from a fresh heap, `filter` packs the blocks below the reduced bound, and
`finish_filtered` checks that exactly the blocks the rule names arrived, byte for byte.

The plain scan: `scan_rest`, `scan_plain` and `finish` take `plain=`; with it they produce / accept,
for the queries and slots the device sends to the matrix-core kernel, clip(plain sum, -128, 127)
(`plain_segment`) where the rule of shard_count_rest_kernel / make_slots says so (`plain_queries`,
`table_limit`).  Without it (the default, what the gloo tests run) everything is scored exactly.
This module is the second statement of the wire contract of include/tinyknn_hip.h; tests/shard_wire.py
runs it in lock step with the HIP engine."""
import numpy as np

from tinyknn_amd.multi_gpu import shard_positions


def limits(T, avx):
    """(N_0, N_1, C) of a signed table T (M, 16): the negative mass of the reference's two saturating
    chains and the limit C = 127 - N_0 - N_1 of plain_scan.hip's lemma (tests/test_plain_scan_lemma.py)."""
    neg = np.maximum(0, -T.min(axis=1))
    chain = ((np.arange(len(T)) >> 1) & 1) if avx else np.zeros(len(T), int)
    n0, n1 = int(neg[chain == 0].sum()), int(neg[chain == 1].sum())
    return n0, n1, 127 - n0 - n1


def _signed(table):
    return np.ascontiguousarray(table).view(np.int8).reshape(-1, 16).astype(np.int64)


def table_limit(table, order="avx"):
    """C of a query's table ((M, 16) bytes as the oracle's debug output holds them), or None for "never"
    (a chain's negative mass above 128): table_limits_kernel / the table kernel's epilogue.  The AVX
    order reads M & ~3 blocks (api_index.hip: lim_m_used)."""
    avx = order in ("avx", 1)
    T = _signed(table)
    if avx:
        T = T[:len(T) & ~3]
    n0, n1, C = limits(T, avx)
    return C if n0 <= 128 and n1 <= 128 else None


class OracleShardEngine:
    device = "cpu"
    order = "avx"

    def __init__(self, O, ox, owner, rank, world):
        self.O, self.ox, self.owner, self.rank, self.world = O, ox, owner, rank, world
        self.chunks = np.diff(ox.list_chunk_off)
        T = int(ox.ids_off[-1])
        self.ids_unique = len(np.unique(ox.ids[:T])) == T

    def _front_all(self, qn, k, n_probes, pass_1):
        """One oracle query per row, once per batch: kept on the oracle index, so that the W engines of
        a simulated world share it.  The key is the batch's buffer, not id(qn): every Tensor.numpy()
        makes a new array object over the same memory (and the rows are compared on a hit, so a
        buffer that was written to or reused is not mistaken for the batch it held before)."""
        memo = self.ox.__dict__.setdefault("_shard_front", {})
        key = (qn.ctypes.data, qn.shape, k, n_probes, pass_1)
        f = memo.get(key)
        if f is not None and np.array_equal(f["qn"], qn):
            return f
        raw, tables, tables_raw = [], [], []
        for q in qn:
            _, dbg = self.ox.query(q, k, n_probes, pass_1, debug=True)
            raw.append(dbg["probes"].copy())        # unwrapped, as the coarse stage leaves them
            tables_raw.append(dbg["table"].copy())
            tables.append(self.O.transform_tables(dbg["table"]))
        raw = np.array(raw).reshape(len(qn), min(n_probes, self.ox.n_lists))
        probes = raw.copy()
        probes[probes < 0] += self.ox.n_lists       # ivf.py:141 list indexing from the end
        f = dict(qn=qn.copy(), raw=raw, probes=probes, tables=tables, tables_raw=tables_raw, plain_seg={})
        if len(memo) >= 8:
            memo.pop(next(iter(memo)))
        memo[key] = f
        return f

    def _front(self, qn, k, n_probes, pass_1):
        f = self._front_all(qn, k, n_probes, pass_1)
        return f["probes"], f["tables"]

    # ---- the plain scan's side of the contract
    def plain_segment(self, l, table):
        """clip(S, -128, 127) as bytes over list l's packed chunks, padding rows included; S = the plain
        integer sum of the signed table ((M, 16) bytes) over the rows' codes."""
        return np.clip(self.plain_sums(l, table), -128, 127).astype(np.int8).view(np.uint8)

    def plain_sums(self, l, table):
        off = self.ox.list_chunk_off
        if off[l + 1] == off[l]:
            return np.zeros(0, np.int64)
        codes = self.O.unpack(np.ascontiguousarray(self.ox.codes[off[l]:off[l + 1]])).astype(np.int64)
        T = _signed(table)
        return T[np.arange(len(T))[None, :], codes].sum(axis=1)

    def table_limit(self, table, order=None):
        return table_limit(table, self.order if order is None else order)

    def plain_queries(self, probes_unwrapped, tables, bound, capacity=None):
        """(nq,) bool, the rule of shard_count_rest_kernel: a query's lists behind the first go to the plain
        kernel iff its probe list did not wrap, its table has a limit C and the bound after its first list
        (order key -> distance byte) is at most C.  capacity: the call's — no query goes plain where
        world * capacity does not hold the longest list (the plain kernel scores an overflowed segment to
        the buffer's tail)."""
        b = (np.asarray(bound).astype(np.uint8) ^ 0x80).view(np.int8).astype(np.int64)
        out = np.zeros(len(tables), dtype=bool)
        if capacity is not None and self.world * capacity < int(self.chunks.max()):
            return out
        for i, t in enumerate(tables):
            C = self.table_limit(t)
            out[i] = not (probes_unwrapped[i] < 0).any() and C is not None and b[i] <= C
        return out

    def _plain_seg(self, f, i, s):
        key = (i, s)
        if key not in f["plain_seg"]:
            f["plain_seg"][key] = self.plain_segment(f["probes"][i, s], f["tables_raw"][i])
        return f["plain_seg"][key]

    def head_chunks(self, k, n_probes, pass_1):
        """chunks of a first probed list that the one-phase forms keep on the exact kernel: two heap sizes
        of rows, four where labels repeat (api_index.hip: head_rows)"""
        return ((2 if self.ids_unique else 4) * self._heap_size(k, n_probes, pass_1) + 15) // 16

    def one_phase_exact(self, f, k, n_probes, pass_1, bound=None):
        """-> (nq, S + 1) int: [i, s] = leading chunks of slot s that stay exact in the one-phase scan, the rest
        of the slot being plain sums (make_slots: slot_exact / head mode); [i, S] = 1 where the query has plain
        blocks at all.  bound: the min-reduced head bounds (queries above their limit stay exact)."""
        nq, S = f["probes"].shape
        rows = (2 if self.ids_unique else 4) * self._heap_size(k, n_probes, pass_1)
        E = (rows + 15) // 16
        out = np.zeros((nq, S + 1), dtype=np.int64)
        ch = self.chunks[f["probes"]]
        b = None if bound is None else (np.asarray(bound).astype(np.uint8) ^ 0x80).view(np.int8)
        for i in range(nq):
            C = self.table_limit(f["tables_raw"][i])
            ok = not (f["raw"][i] < 0).any() and C is not None and (b is None or int(b[i]) <= C)
            seen = np.cumsum(self.ox.list_n[f["probes"][i]])
            e = int(np.argmax(seen >= rows)) + 1 if (seen >= rows).any() else S
            if not ok:
                out[i, :S] = ch[i]
            elif e == 1 and ch[i, 0] > E:
                out[i, 0] = E
                out[i, S] = 1
            else:
                out[i, :e] = ch[i, :e]
                out[i, S] = int(e < S)
        return out

    def _segment(self, l, table):
        # (kept per (list, table object) on the oracle index: a batch's stages ask for the same segments
        #  many times; the entry holds the table, so its id cannot pass to another array meanwhile)
        memo = self.ox.__dict__.setdefault("_shard_segments", {})
        hit = memo.get((int(l), id(table)))
        if hit is not None and hit[0] is table:
            return hit[1]
        off = self.ox.list_chunk_off
        codes = np.ascontiguousarray(self.ox.codes[off[l]:off[l + 1]])
        out = np.zeros(2 * len(codes), dtype=np.uint64)
        if len(codes):
            self.O.estimate_pq(codes, table, out, True)
        if len(memo) >= 1 << 15:
            memo.clear()
        memo[(int(l), id(table))] = (table, out.view(np.uint8))
        return out.view(np.uint8)

    def coarse(self, slot, qn, qp, k, n_probes, pass_1, probes_home):
        """Probe lists of this rank's home queries only (rows past nq: 0)."""
        qn = qn.numpy()
        qh = -(-len(qn) // self.world)
        out = probes_home.numpy().reshape(qh, -1)
        out[:] = 0
        lo, hi = self.rank * qh, min(len(qn), (self.rank + 1) * qh)
        if hi > lo:
            out[:hi - lo] = self._front_all(qn, k, n_probes, pass_1)["raw"][lo:hi]     # unwrapped, as the coarse stage leaves them
        self.coarse_calls = getattr(self, "coarse_calls", 0) + 1

    def scan(self, slot, qn, qp, k, n_probes, pass_1, capacity, send, flag, probes_all=None):
        qn = qn.numpy()
        self.last_capacity = capacity
        probes, tables = self._front(qn, k, n_probes, pass_1)
        if probes_all is not None:
            # the gathered probe lists must be what every rank would have derived itself
            got = probes_all.numpy().reshape(-1, probes.shape[1])[:len(qn)].copy()
            got[got < 0] += self.ox.n_lists
            np.testing.assert_array_equal(got, probes)
        src, pos = shard_positions(probes, self.chunks, self.owner, self.world, capacity)
        _, free = shard_positions(probes, self.chunks, self.owner, self.world, 10 ** 12)
        qh = -(-len(qn) // self.world)
        # the streams this rank sends or receives (the callers max-reduce over the ranks)
        mine = (src == self.rank) | ((np.arange(len(qn)) // qh)[:, None] == self.rank)
        self.last_usage = int((free + self.chunks[probes])[mine].max()) if mine.any() else 0
        buf = send.numpy().reshape(self.world, capacity * 16)
        buf[:] = 0xAB                               # stale bytes must never be consumed
        for i in range(len(qn)):
            for s in range(probes.shape[1]):
                if src[i, s] != self.rank:
                    continue
                if pos[i, s] < 0:
                    flag[0] = 1
                    continue
                seg = self._segment(probes[i, s], tables[i])
                buf[i // qh, pos[i, s] * 16: pos[i, s] * 16 + len(seg)] = seg

    # ---- the scan in two phases (tk_index_shard_scan_first_dev / _rest_dev).  This engine has no
    # second kernel: phase 1 scores everything and computes the bound, phase 2 checks that the
    # bound it is handed is the min-reduced one every rank must hold.
    def plain_ok(self, k, n_probes, pass_1):
        return n_probes >= 2

    def scan_first(self, slot, qn, qp, k, n_probes, pass_1, capacity, send, flag, bound, probes_all=None):
        self.scan(slot, qn, qp, k, n_probes, pass_1, capacity, send, flag, probes_all=probes_all)
        self.bound(slot, qn, k, n_probes, pass_1, capacity, send, bound)
        self.first_bound = bound.numpy().copy()

    def scan_rest(self, slot, qn, k, n_probes, pass_1, capacity, send, bound, plain=False):
        b = bound.numpy()
        mine = self.first_bound != 255
        np.testing.assert_array_equal(b[mine], self.first_bound[mine])      # my queries: my value survived the MIN
        qn_ = qn.numpy()
        probes, _ = self._front(qn_, k, n_probes, pass_1)
        owned_elsewhere = (self.owner[probes[:, 0]] != self.rank)
        assert (self.first_bound[owned_elsewhere] == 255).all()
        self.rest_calls = getattr(self, "rest_calls", 0) + 1
        if not plain:
            return
        # plain=True: the lists behind the first of the queries the rule names become plain sums
        f = self._front_all(qn_, k, n_probes, pass_1)
        self.last_plain = self.plain_queries(f["raw"], f["tables_raw"], b, capacity)
        self.last_plain_pairs = 0       # owned (query, slot >= 1) pairs of those queries, fitted or not
        src, pos = shard_positions(probes, self.chunks, self.owner, self.world, capacity)
        buf = send.numpy().reshape(self.world, capacity * 16)
        qh = -(-len(qn_) // self.world)
        for i in np.flatnonzero(self.last_plain):
            for s in range(1, probes.shape[1]):
                if src[i, s] != self.rank:
                    continue
                self.last_plain_pairs += 1
                if pos[i, s] >= 0:
                    seg = self._plain_seg(f, i, s)
                    buf[i // qh, pos[i, s] * 16: pos[i, s] * 16 + len(seg)] = seg

    # ---- the scan in ONE phase (tk_index_shard_scan_plain_dev).  This engine has no second kernel: it
    # scores every segment exactly (bytes that trivially satisfy the lemma); `fail_plain` makes the
    # home replay of the next `fail_plain` such batches report a query that failed the check, which
    # is how the tests drive the bit-4 protocol (flag travels with the ids, the batch is repeated
    # in the two-phase form).
    fail_plain = 0

    def scan_plain(self, slot, qn, qp, k, n_probes, pass_1, capacity, send, flag, probes_all=None, bound=None,
                   plain=False):
        if bound is not None:       # behind scan_head: the bytes are the min-reduced head bounds every rank must hold
            b = bound.numpy()
            mine = self.head_bound != 255
            np.testing.assert_array_equal(b[mine], self.head_bound[mine])
            self.head_calls = getattr(self, "head_calls", 0) + 1
        else:
            self.scan(slot, qn, qp, k, n_probes, pass_1, capacity, send, flag, probes_all=probes_all)
            self.plain_calls = getattr(self, "plain_calls", 0) + 1
        if not plain:
            return
        # plain=True: everything behind the exact chunks make_slots keeps becomes plain sums (where the form
        # applies as far as this model knows: two probed lists, the longest list fits the buffer's tail)
        qn_ = qn.numpy()
        f = self._front_all(qn_, k, n_probes, pass_1)
        probes = f["probes"]
        if probes.shape[1] < 2 or self.world * capacity < int(self.chunks.max()):
            return
        keep = self.one_phase_exact(f, k, n_probes, pass_1, None if bound is None else bound.numpy())
        src, pos = shard_positions(probes, self.chunks, self.owner, self.world, capacity)
        buf = send.numpy().reshape(self.world, capacity * 16)
        qh = -(-len(qn_) // self.world)
        for i in range(len(qn_)):
            for s in range(probes.shape[1]):
                n = int(self.chunks[probes[i, s]])
                if src[i, s] != self.rank or pos[i, s] < 0 or keep[i, s] >= n:
                    continue
                seg = self._plain_seg(f, i, s)
                a = pos[i, s] * 16
                buf[i // qh, a + 16 * keep[i, s]: a + len(seg)] = seg[16 * keep[i, s]:]

    def scan_head(self, slot, qn, qp, k, n_probes, pass_1, capacity, send, flag, bound, probes_all=None):
        """tk_index_shard_scan_head_dev: (this engine scores everything at once) + the bound after the HEAD
        of the first probed list — its first ceil(2 R / 16) chunks, ceil(4 R / 16) where labels repeat — for
        the queries whose first list is mine."""
        self.scan(slot, qn, qp, k, n_probes, pass_1, capacity, send, flag, probes_all=probes_all)
        qn_ = qn.numpy()
        probes, tables = self._front(qn_, k, n_probes, pass_1)
        R = self._heap_size(k, n_probes, pass_1)
        E = self.head_chunks(k, n_probes, pass_1)
        out = bound.numpy()
        out[:] = 255
        off = self.ox.list_chunk_off
        for i in range(len(qn_)):
            l = probes[i, 0]
            if self.owner[l] != self.rank:
                continue
            idx = np.zeros(R, dtype=np.int64)
            val = np.zeros(R, dtype=np.int32)
            self.O.init_heap(idx, val, True)
            codes = np.ascontiguousarray(self.ox.codes[off[l]:off[l + 1]][:E])
            if len(codes):
                self.O.query_pq(codes, min(int(self.ox.list_n[l]), 16 * len(codes)), tables[i], idx, val, True)
            out[i] = (int(val[0]) & 0xff) ^ 0x80
        self.head_bound = out.copy()

    def finish(self, slot, qn, k, n_probes, pass_1, capacity, recv, out_home, flag=None, plain=None):
        """plain: None — every received byte is the exact one; a (nq,) bool array — the two-phase rule: the
        slots behind the first of those queries hold plain sums, all else exact; "blocks" — the one-phase
        contract: the head of the first list exact, every other 16-byte block exact or plain."""
        if flag is not None and self.fail_plain > 0:
            self.fail_plain -= 1
            flag.numpy()[0] |= 4
        qn = qn.numpy()
        probes, tables = self._front(qn, k, n_probes, pass_1)
        f = self._front_all(qn, k, n_probes, pass_1)
        E = self.head_chunks(k, n_probes, pass_1)
        src, pos = shard_positions(probes, self.chunks, self.owner, self.world, capacity)
        buf = recv.numpy().reshape(self.world, capacity * 16)
        qh = -(-len(qn) // self.world)
        out = out_home.numpy().reshape(qh, k)
        out[:] = -1
        for i in range(self.rank * qh, min(len(qn), (self.rank + 1) * qh)):
            for s in range(probes.shape[1]):
                if pos[i, s] < 0:
                    continue                        # overflowed: the batch is repeated
                seg = self._segment(probes[i, s], tables[i])
                got = buf[src[i, s], pos[i, s] * 16: pos[i, s] * 16 + len(seg)]
                if isinstance(plain, str):
                    assert plain == "blocks"
                    head = 16 * min(E, len(seg) // 16) if s == 0 else 0
                    np.testing.assert_array_equal(got[:head], seg[:head])
                    ps = self._plain_seg(f, i, s)
                    ok = ((got.reshape(-1, 16) == seg.reshape(-1, 16)).all(axis=1) |
                          (got.reshape(-1, 16) == ps.reshape(-1, 16)).all(axis=1))
                    assert ok.all(), ("neither the exact nor the plain block", i, s, np.flatnonzero(~ok)[:4])
                    continue
                if plain is not None and s >= 1 and plain[i]:
                    seg = self._plain_seg(f, i, s)
                np.testing.assert_array_equal(got, seg, err_msg=f"query {i} slot {s}")
            out[i - self.rank * qh] = self.ox.query_batch(qn[i:i + 1], k, n_probes, pass_1)[0]

    def usage(self, slot):
        """longest stream of the last scan, fitted or not (tk_index_shard_usage)"""
        return self.last_usage

    # ---- filtered exchange: same three calls as the HIP engine
    def _heap_size(self, k, n_probes, pass_1):
        return int(pass_1) if pass_1 else (n_probes + 1) * k + 1        # ivf.py:135-136

    def bound(self, slot, qn, k, n_probes, pass_1, capacity, scan_buf, bound):
        qn = qn.numpy()
        probes, tables = self._front(qn, k, n_probes, pass_1)
        out = bound.numpy()
        out[:] = 255
        off = self.ox.list_chunk_off
        for i in range(len(qn)):
            l = probes[i, 0]
            if self.owner[l] != self.rank:
                continue
            idx = np.zeros(self._heap_size(k, n_probes, pass_1), dtype=np.int64)
            val = np.zeros(len(idx), dtype=np.int32)
            self.O.init_heap(idx, val, True)
            codes = np.ascontiguousarray(self.ox.codes[off[l]:off[l + 1]])
            if len(codes):
                self.O.query_pq(codes, int(self.ox.list_n[l]), tables[i], idx, val, True)
            out[i] = (int(val[0]) & 0xff) ^ 0x80

    def _passing(self, seg, slot, b):
        """chunk indices of a segment that travel under bound key b"""
        m = seg.view(np.int8).reshape(-1, 16).min(axis=1).astype(np.int64) + 128
        return np.arange(len(m)) if slot == 0 else np.flatnonzero(m < int(b))

    def filter(self, slot, qn, k, n_probes, pass_1, capacity, scan_buf, bound, counts, records):
        qn = qn.numpy()
        probes, tables = self._front(qn, k, n_probes, pass_1)
        src, pos = shard_positions(probes, self.chunks, self.owner, self.world, capacity)
        buf = scan_buf.numpy().reshape(self.world, capacity * 16)
        b = bound.numpy()
        qh = -(-len(qn) // self.world)
        cap = probes.shape[1] * int(self.chunks.max())                  # Plan.cap (api_index.hip make_plan)
        prefix = np.concatenate([np.zeros((len(qn), 1), np.int64),
                                 np.cumsum(self.chunks[probes], axis=1)], axis=1)
        per_home = [[] for _ in range(self.world)]
        dense = np.zeros(self.world, dtype=np.int64)
        for i in range(len(qn)):
            h = i // qh
            for s in range(probes.shape[1]):
                if src[i, s] != self.rank or pos[i, s] < 0:
                    continue
                n = int(self.chunks[probes[i, s]])
                seg = buf[h, pos[i, s] * 16:(pos[i, s] + n) * 16]
                dense[h] += n
                for c in self._passing(seg, s, b[i]):
                    rec = np.empty(5, dtype=np.int32)
                    rec[0] = (i - h * qh) * cap + prefix[i, s] + c
                    rec[1:] = seg[16 * c:16 * c + 16].view(np.int32)
                    per_home[h].append(rec)
        cnt = counts.numpy()
        cnt[:] = 0
        cnt[:self.world] = [len(x) for x in per_home]
        cnt[2 * self.world:] = dense
        flat = [r for x in per_home for r in x]
        if flat:
            records.numpy()[:len(flat)] = np.array(flat)

    def finish_filtered(self, slot, qn, k, n_probes, pass_1, records, n_records, out_home, flag):
        qn = qn.numpy()
        probes, tables = self._front(qn, k, n_probes, pass_1)
        qh = -(-len(qn) // self.world)
        cap = probes.shape[1] * int(self.chunks.max())
        _, pos = shard_positions(probes, self.chunks, self.owner, self.world, self.last_capacity)
        rec = records.numpy()[:n_records]
        got = {int(r[0]): r[1:].tobytes() for r in rec}
        assert len(got) == n_records, "a block arrived twice"
        out = out_home.numpy().reshape(qh, k)
        out[:] = -1
        want = 0
        # the bound every rank must have used: after the first list, from a fresh heap
        for i in range(self.rank * qh, min(len(qn), (self.rank + 1) * qh)):
            idx = np.zeros(self._heap_size(k, n_probes, pass_1), dtype=np.int64)
            val = np.zeros(len(idx), dtype=np.int32)
            self.O.init_heap(idx, val, True)
            l0 = probes[i, 0]
            off = self.ox.list_chunk_off
            codes = np.ascontiguousarray(self.ox.codes[off[l0]:off[l0 + 1]])
            if len(codes):
                self.O.query_pq(codes, int(self.ox.list_n[l0]), tables[i], idx, val, True)
            b = (int(val[0]) & 0xff) ^ 0x80
            f0 = 0
            for s in range(probes.shape[1]):
                seg = self._segment(probes[i, s], tables[i])
                for c in (self._passing(seg, s, b) if pos[i, s] >= 0 else []):   # overflowed: repeated
                    key = (i - self.rank * qh) * cap + f0 + int(c)
                    assert got.get(key) == seg[16 * c:16 * c + 16].tobytes(), (i, s, c)
                    want += 1
                f0 += int(self.chunks[probes[i, s]])
            out[i - self.rank * qh] = self.ox.query_batch(qn[i:i + 1], k, n_probes, pass_1)[0]
        assert want == n_records, "blocks that should not have travelled"

    # ---- the same without the host synchronisation: fixed regions, counts read "on the device"
    def filter_regions(self, slot, qn, k, n_probes, pass_1, capacity, scan_buf, bound, counts, records,
                       region, flag, acc=None):
        import torch
        W = self.world
        compact = torch.zeros((W * capacity, 5), dtype=torch.int32)
        self.filter(slot, qn, k, n_probes, pass_1, capacity, scan_buf, bound, counts, compact)
        cnt = counts.numpy()[:W]
        if acc is not None:                             # the caller's books (atomics on the device)
            a = acc.numpy()
            a[0] = max(int(a[0]), int(cnt.max()))
            a[1] += int(cnt.sum())
            a[2] += int(counts.numpy()[2 * W:].sum())
        rec = records.numpy().reshape(W, region, 5)
        rec[:] = -9                                     # (stale bytes must never be read as records)
        o = 0
        for h in range(W):
            n = int(cnt[h])
            rec[h, :min(n, region)] = compact.numpy()[o:o + min(n, region)]
            if n > region:
                flag.numpy()[0] |= 1
            o += n

    def finish_regions(self, slot, qn, k, n_probes, pass_1, records, counts_recv, region, out_home, flag):
        import torch
        W = self.world
        cnt = counts_recv.numpy()[:W]
        if (cnt > region).any():                        # a sender overflowed (its flag says so): the
            out_home.numpy()[:] = -1                    # batch is repeated, nothing to check here
            return
        rec = records.numpy().reshape(W, region, 5)
        got = np.concatenate([rec[s_, :int(cnt[s_])] for s_ in range(W)]) if cnt.sum() else np.zeros((0, 5), np.int32)
        self.finish_filtered(slot, qn, k, n_probes, pass_1, torch.from_numpy(np.ascontiguousarray(got)),
                             len(got), out_home, flag)

