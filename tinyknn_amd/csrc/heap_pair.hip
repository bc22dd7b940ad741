// heap_pair.hip — heap_replay_pair_kernel: one query per wave with the heap in registers, two nodes per lane and group
// (heap.hip's head has the overview of all replays).
#include <stdlib.h>

#include <type_traits>

#include "heap_common.h"

// Wave-per-query replay with the heap in REGISTERS, two nodes per lane: heaps of up to 129 entries (IVF.query at the
// reference's bench settings: (n_probes + 1) k + 1 = 111; its coarse `top`: 2 n_probes + 10 = 30).  This is the kernel
// of ONE query per call (examples/bench.py:118-137 times exactly that) and of small batches, where the lane kernel's
// round of ~2 000 cycles serves a single lane: ~760 dependent inserts of one query were 0.47 of the call's 0.54 ms.
//
// Layout (tests/test_pair_heap_lemma.py restates it in numpy and checks it against the reference's loop): the root is
// wave-uniform; lane L holds the two CHILDREN of node L — node 2L+1 in slot 0, node 2L+2 in slot 1.  "Which child of
// node L is larger" (the left one on ties: `vl > v`, then `vr > nxt_val`, _fast_pq.pyx:297-300) is a comparison inside
// the lane; one ballot B of it describes the whole max-child path, which `insert`'s sift follows whatever v is: node t
// is on it iff every ancestor chose the child on the chain down to t — ((B ^ bits) & mask) == 0 with a per-lane constant
// pair.  Values never rise along the path, so with CE[L] = the entry of node L's larger child
//     root                                           <- CE[0]  if CE[0].v > v   else (label, v)
//     larger child c of an on-path node L, CE[L].v > v <- CE[c]  if c < 64 and CE[c].v > v   else (label, v)
// B, the path, CE and the cross-lane fetch of CE[c] (one ds_bpermute per register of an entry) are prepared BEHIND an
// insert, before the next candidate is known; a compare and two selects per lane remain on the candidate's own chain.
// Nodes >= R hold a value no candidate is below and are never taken.
// Entries: POSITIONS (value8 << 24 | flat position24, one register per slot) where no label can repeat among a query's
// lists; (value, label64) — three registers per slot — with the reference's duplicate test (`if i == indices[j]:
// return`, :284-287, one ballot) where labels repeat (IVF.build(n_probes >= 2)) or a probe list names a list twice.
#define TK_PAIR_LOW (-(1 << 20))

struct PairLane {      // constants of lane L = node L: its ancestors (as lanes, all < 32) and the child each must choose
    uint32_t anc_mask, anc_bits;
};
__device__ __forceinline__ PairLane pair_lane(int lane)
{
    PairLane K;
    K.anc_mask = K.anc_bits = 0;
    for (int t = lane; t > 0;) {
        const int par = (t - 1) >> 1;
        K.anc_mask |= 1u << par;
        K.anc_bits |= (uint32_t)((t - 1) & 1) << par;
        t = par;
    }
    return K;
}

// ---- position entries
template <bool SIGNED>
struct PairHeapPos {
    uint32_t e0, e1, er;            // er: wave-uniform
    // prepared behind every change
    bool right, onp;
    uint32_t ce, fe, ce0;
    int cev, fev;
    __device__ __forceinline__ void init(int lane, int R)
    {
        const uint32_t fresh = SIGNED ? 0x7fffffffu : 0xffffffffu;
        const uint32_t lowest = SIGNED ? 0x80ffffffu : 0x00ffffffu;
        er = fresh;
        e0 = 2 * lane + 1 < R ? fresh : lowest;
        e1 = 2 * lane + 2 < R ? fresh : lowest;
    }
    __device__ __forceinline__ void prepare(int lane, const PairLane &K)
    {
        const uint32_t lowest = SIGNED ? 0x80ffffffu : 0x00ffffffu;
        const int v0 = entry_val<SIGNED>(e0), v1 = entry_val<SIGNED>(e1);
        right = v1 > v0;
        const uint32_t ball = (uint32_t)__builtin_amdgcn_ballot_w64(right);
        onp = ((ball ^ K.anc_bits) & K.anc_mask) == 0;
        ce = right ? e1 : e0;
        cev = right ? v1 : v0;
        const int c = 2 * lane + 1 + (int)right;
        const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute((c & 63) << 2, (int)ce);
        fe = c < 64 ? got : lowest;
        fev = entry_val<SIGNED>(fe);
        ce0 = __builtin_amdgcn_readlane(ce, 0);
    }
    __device__ __forceinline__ uint32_t bound() const { return er >> 24; }
    // entries value8 << 24 | label24 (labels below 0xffffff): `if i == indices[j]: return` (:284-287) on the low 24 bits —
    // fresh nodes and nodes >= R hold 0xffffff, which no row carries
    __device__ __forceinline__ bool holds24(uint32_t l24) const
    {
        const bool here = (((e0 ^ l24) & 0x00ffffffu) == 0) | (((e1 ^ l24) & 0x00ffffffu) == 0);
        return __builtin_amdgcn_ballot_w64(here) != 0 || ((er ^ l24) & 0x00ffffffu) == 0;
    }
    __device__ __forceinline__ void insert(uint32_t e, int v, int lane, const PairLane &K)
    {
        const bool upd = onp && cev > v;
        const uint32_t ne = fev > v ? fe : e;
        e0 = (upd && !right) ? ne : e0;
        e1 = (upd && right) ? ne : e1;
        er = entry_val<SIGNED>(ce0) > v ? ce0 : e;
        prepare(lane, K);
    }
};

// ---- (value, label) entries with the duplicate test
template <bool SIGNED>
struct PairHeapLab {
    int v0, v1, vr;
    uint32_t lo0, lo1, lor, hi0, hi1, hir;
    bool right, onp;
    int cev, fev, cev0;
    uint32_t clo, chi, flo, fhi, clo0, chi0;
    __device__ __forceinline__ void init(int lane, int R)
    {
        const int fresh = SIGNED ? 127 : 255;
        vr = fresh;
        v0 = 2 * lane + 1 < R ? fresh : TK_PAIR_LOW;
        v1 = 2 * lane + 2 < R ? fresh : TK_PAIR_LOW;
        lo0 = lo1 = lor = hi0 = hi1 = hir = 0xffffffffu;       // label -1
    }
    __device__ __forceinline__ void prepare(int lane, const PairLane &K)
    {
        right = v1 > v0;
        const uint32_t ball = (uint32_t)__builtin_amdgcn_ballot_w64(right);
        onp = ((ball ^ K.anc_bits) & K.anc_mask) == 0;
        cev = right ? v1 : v0;
        clo = right ? lo1 : lo0;
        chi = right ? hi1 : hi0;
        const int c = 2 * lane + 1 + (int)right;
        const int a = (c & 63) << 2;
        const int gv = __builtin_amdgcn_ds_bpermute(a, cev);
        const uint32_t gl = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)clo);
        const uint32_t gh = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)chi);
        fev = c < 64 ? gv : TK_PAIR_LOW;
        flo = gl;
        fhi = gh;
        cev0 = __builtin_amdgcn_readlane(cev, 0);
        clo0 = __builtin_amdgcn_readlane(clo, 0);
        chi0 = __builtin_amdgcn_readlane(chi, 0);
    }
    __device__ __forceinline__ uint32_t bound() const { return (uint32_t)vr & 0xffu; }
    // `if i == indices[j]: return` (:284-287): nodes >= R and fresh nodes hold -1, which no row carries
    __device__ __forceinline__ bool holds(uint32_t llo, uint32_t lhi) const
    {
        const bool here = ((lo0 == llo) & (hi0 == lhi)) | ((lo1 == llo) & (hi1 == lhi));
        return __builtin_amdgcn_ballot_w64(here) != 0 || (lor == llo && hir == lhi);
    }
    __device__ __forceinline__ void insert(uint32_t llo, uint32_t lhi, int v, int lane, const PairLane &K)
    {
        const bool upd = onp && cev > v;
        const bool deeper = fev > v;
        const int nv = deeper ? fev : v;
        const uint32_t nl = deeper ? flo : llo, nh = deeper ? fhi : lhi;
        const bool u0 = upd && !right, u1 = upd && right;
        v0 = u0 ? nv : v0; lo0 = u0 ? nl : lo0; hi0 = u0 ? nh : hi0;
        v1 = u1 ? nv : v1; lo1 = u1 ? nl : lo1; hi1 = u1 ? nh : hi1;
        const bool rt = cev0 > v;
        vr = rt ? cev0 : v; lor = rt ? clo0 : llo; hir = rt ? chi0 : lhi;
        prepare(lane, K);
    }
};

// ---- G groups of node pairs per lane: heaps of up to 128 G + 1 entries (G = 2: 257 — n_probes <= 24 at k = 10; G = 4: 513 —
// n_probes <= 50).  Lane L, group g holds the children of node t = 64 g + L.  One ballot per group describes the path; the
// ancestors of an internal node are all below 32 G (the lower half of the groups), so a node's on-path test is a mask test
// against the ballots of those groups with per-lane constants; the chosen child c = 2 t + 1 + right of a node of group g
// has its own pair in lane c & 63 of group c >> 6 in {2g, 2g+1, 2g+2} (c < 64 G), else it is a leaf.  Formulation checked
// on the CPU for G = 1, 2, 4 (tests/test_pair_heap_lemma.py: GroupHeap).  G = 1 keeps the structs above (same arithmetic,
// written out: the kernel of the smallest heaps is the one that matters most).
template <int G>
struct GroupLane {
    static constexpr int GA = G >= 2 ? G / 2 : 1;      // groups that hold ancestors
    uint32_t m_lo[G][GA], m_hi[G][GA], b_lo[G][GA], b_hi[G][GA];
};
template <int G>
__device__ __forceinline__ GroupLane<G> group_lane(int lane)
{
    GroupLane<G> K;
#pragma unroll
    for (int g = 0; g < G; g++) {
#pragma unroll
        for (int a = 0; a < GroupLane<G>::GA; a++) K.m_lo[g][a] = K.m_hi[g][a] = K.b_lo[g][a] = K.b_hi[g][a] = 0;
        for (int t = 64 * g + lane; t > 0;) {
            const int par = (t - 1) >> 1;
            const uint32_t bit = (uint32_t)((t - 1) & 1);
            const int a = par >> 6, l = par & 63;       // a < GA by construction
#pragma unroll
            for (int aa = 0; aa < GroupLane<G>::GA; aa++)
                if (aa == a) {
                    if (l < 32) { K.m_lo[g][aa] |= 1u << l; K.b_lo[g][aa] |= bit << l; }
                    else { K.m_hi[g][aa] |= 1u << (l - 32); K.b_hi[g][aa] |= bit << (l - 32); }
                }
            t = par;
        }
    }
    return K;
}

template <bool SIGNED, int G>
struct GroupHeapPos {
    static constexpr int GROUPS = G;
    uint32_t e0[G], e1[G], er;
    bool right[G], onp[G];
    uint32_t ce[G], fe[G], ce0;
    __device__ __forceinline__ void init(int lane, int R)
    {
        const uint32_t fresh = SIGNED ? 0x7fffffffu : 0xffffffffu;
        const uint32_t lowest = SIGNED ? 0x80ffffffu : 0x00ffffffu;
        er = fresh;
#pragma unroll
        for (int g = 0; g < G; g++) {
            e0[g] = 2 * (64 * g + lane) + 1 < R ? fresh : lowest;
            e1[g] = 2 * (64 * g + lane) + 2 < R ? fresh : lowest;
        }
    }
    __device__ __forceinline__ void prepare(int lane, const GroupLane<G> &K)
    {
        const uint32_t lowest = SIGNED ? 0x80ffffffu : 0x00ffffffu;
        uint64_t B[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            right[g] = entry_val<SIGNED>(e1[g]) > entry_val<SIGNED>(e0[g]);
            B[g] = __builtin_amdgcn_ballot_w64(right[g]);
            ce[g] = right[g] ? e1[g] : e0[g];
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            uint32_t bad = 0;
#pragma unroll
            for (int a = 0; a < GroupLane<G>::GA; a++)
                bad |= (((uint32_t)B[a] ^ K.b_lo[g][a]) & K.m_lo[g][a]) | (((uint32_t)(B[a] >> 32) ^ K.b_hi[g][a]) & K.m_hi[g][a]);
            onp[g] = bad == 0;
            const int c = 2 * (64 * g + lane) + 1 + (int)right[g];
            const int a4 = (c & 63) << 2;
            uint32_t f = lowest;
#pragma unroll
            for (int sg = 2 * g; sg <= 2 * g + 2; sg++)
                if (sg < G) {
                    const uint32_t got = (uint32_t)__builtin_amdgcn_ds_bpermute(a4, (int)ce[sg]);
                    f = (c >> 6) == sg ? got : f;
                }
            fe[g] = f;
        }
        ce0 = __builtin_amdgcn_readlane(ce[0], 0);
    }
    __device__ __forceinline__ uint32_t bound() const { return er >> 24; }
    __device__ __forceinline__ bool holds24(uint32_t l24) const
    {
        bool here = false;
#pragma unroll
        for (int g = 0; g < G; g++) here |= (((e0[g] ^ l24) & 0x00ffffffu) == 0) | (((e1[g] ^ l24) & 0x00ffffffu) == 0);
        return __builtin_amdgcn_ballot_w64(here) != 0 || ((er ^ l24) & 0x00ffffffu) == 0;
    }
    __device__ __forceinline__ void insert(uint32_t e, int v, int lane, const GroupLane<G> &K)
    {
#pragma unroll
        for (int g = 0; g < G; g++) {
            const bool upd = onp[g] && entry_val<SIGNED>(ce[g]) > v;
            const uint32_t ne = entry_val<SIGNED>(fe[g]) > v ? fe[g] : e;
            e0[g] = (upd && !right[g]) ? ne : e0[g];
            e1[g] = (upd && right[g]) ? ne : e1[g];
        }
        er = entry_val<SIGNED>(ce0) > v ? ce0 : e;
        prepare(lane, K);
    }
    __device__ __forceinline__ uint32_t slot_entry(int g, int slot) const { return slot ? e1[g] : e0[g]; }
};

template <bool SIGNED, int G>
struct GroupHeapLab {
    static constexpr int GROUPS = G;
    int v0[G], v1[G], vr;
    uint32_t lo0[G], lo1[G], hi0[G], hi1[G], lor, hir;
    bool right[G], onp[G];
    int cev[G], fev[G], cev0;
    uint32_t clo[G], chi[G], flo[G], fhi[G], clo0, chi0;
    __device__ __forceinline__ void init(int lane, int R)
    {
        const int fresh = SIGNED ? 127 : 255;
        vr = fresh;
        lor = hir = 0xffffffffu;
#pragma unroll
        for (int g = 0; g < G; g++) {
            v0[g] = 2 * (64 * g + lane) + 1 < R ? fresh : TK_PAIR_LOW;
            v1[g] = 2 * (64 * g + lane) + 2 < R ? fresh : TK_PAIR_LOW;
            lo0[g] = lo1[g] = hi0[g] = hi1[g] = 0xffffffffu;       // label -1
        }
    }
    __device__ __forceinline__ void prepare(int lane, const GroupLane<G> &K)
    {
        uint64_t B[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            right[g] = v1[g] > v0[g];
            B[g] = __builtin_amdgcn_ballot_w64(right[g]);
            cev[g] = right[g] ? v1[g] : v0[g];
            clo[g] = right[g] ? lo1[g] : lo0[g];
            chi[g] = right[g] ? hi1[g] : hi0[g];
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            uint32_t bad = 0;
#pragma unroll
            for (int a = 0; a < GroupLane<G>::GA; a++)
                bad |= (((uint32_t)B[a] ^ K.b_lo[g][a]) & K.m_lo[g][a]) | (((uint32_t)(B[a] >> 32) ^ K.b_hi[g][a]) & K.m_hi[g][a]);
            onp[g] = bad == 0;
            const int c = 2 * (64 * g + lane) + 1 + (int)right[g];
            const int a4 = (c & 63) << 2;
            int fv = TK_PAIR_LOW;
            uint32_t fl = 0xffffffffu, fh = 0xffffffffu;
#pragma unroll
            for (int sg = 2 * g; sg <= 2 * g + 2; sg++)
                if (sg < G) {
                    const int gv = __builtin_amdgcn_ds_bpermute(a4, cev[sg]);
                    const uint32_t gl = (uint32_t)__builtin_amdgcn_ds_bpermute(a4, (int)clo[sg]);
                    const uint32_t gh = (uint32_t)__builtin_amdgcn_ds_bpermute(a4, (int)chi[sg]);
                    const bool here = (c >> 6) == sg;
                    fv = here ? gv : fv; fl = here ? gl : fl; fh = here ? gh : fh;
                }
            fev[g] = fv; flo[g] = fl; fhi[g] = fh;
        }
        cev0 = __builtin_amdgcn_readlane(cev[0], 0);
        clo0 = __builtin_amdgcn_readlane(clo[0], 0);
        chi0 = __builtin_amdgcn_readlane(chi[0], 0);
    }
    __device__ __forceinline__ uint32_t bound() const { return (uint32_t)vr & 0xffu; }
    __device__ __forceinline__ bool holds(uint32_t llo, uint32_t lhi) const
    {
        bool here = false;
#pragma unroll
        for (int g = 0; g < G; g++)
            here |= ((lo0[g] == llo) & (hi0[g] == lhi)) | ((lo1[g] == llo) & (hi1[g] == lhi));
        return __builtin_amdgcn_ballot_w64(here) != 0 || (lor == llo && hir == lhi);
    }
    __device__ __forceinline__ void insert(uint32_t llo, uint32_t lhi, int v, int lane, const GroupLane<G> &K)
    {
#pragma unroll
        for (int g = 0; g < G; g++) {
            const bool upd = onp[g] && cev[g] > v;
            const bool deeper = fev[g] > v;
            const int nv = deeper ? fev[g] : v;
            const uint32_t nl = deeper ? flo[g] : llo, nh = deeper ? fhi[g] : lhi;
            const bool u0 = upd && !right[g], u1 = upd && right[g];
            v0[g] = u0 ? nv : v0[g]; lo0[g] = u0 ? nl : lo0[g]; hi0[g] = u0 ? nh : hi0[g];
            v1[g] = u1 ? nv : v1[g]; lo1[g] = u1 ? nl : lo1[g]; hi1[g] = u1 ? nh : hi1[g];
        }
        const bool rt = cev0 > v;
        vr = rt ? cev0 : v; lor = rt ? clo0 : llo; hir = rt ? chi0 : lhi;
        prepare(lane, K);
    }
};

// The replay of one query by one wave: LABELS = the duplicate test on (value, label) entries, else position entries.
// (Two instantiations called from one wave-uniform branch: as ONE loop with a run-time switch the compiler merged
//  both heaps' registers and masks through every iteration — ~30 scalar moves per insert.)
// KIND 0: position entries (no label can repeat among the query's lists); 1: (value, label64) entries with the duplicate
// test; 2: the duplicate test on value8 << 24 | label24 entries (every label of the index below 0xffffff: one register per
// slot as with positions — the reference's default build, IVF.build(n_probes=2), of anything up to 16.7 M rows)
template <bool SIGNED, int KIND, int G>
__device__ __forceinline__ void pair_replay_body(const uint4 *__restrict__ drow, const uint8_t *__restrict__ mrow,
                                                 const int *__restrict__ prefix, const int *__restrict__ ns,
                                                 const int64_t *__restrict__ loffs, int S,
                                                 const int64_t *__restrict__ labels, int64_t *__restrict__ oi,
                                                 int32_t *__restrict__ ov, int R, int lane, int plain0, uint32_t &b_plain)
{
    // G = 1 (heaps <= 129): the written-out structs; G = 2 / 4: the same arithmetic over G groups of pairs per lane
    typename std::conditional<G == 1, PairLane, GroupLane<G>>::type K;
    if constexpr (G == 1) K = pair_lane(lane); else K = group_lane<G>(lane);
    const int total = S > 0 ? prefix[S] : 0;
    const uint4 never = never16<SIGNED>();
    constexpr bool LABELS = KIND == 1;          // three registers per slot
    constexpr bool NEEDS_LABELS = KIND != 0;    // the candidate rows' labels are loaded
    typename std::conditional<G == 1,
                              typename std::conditional<LABELS, PairHeapLab<SIGNED>, PairHeapPos<SIGNED>>::type,
                              typename std::conditional<LABELS, GroupHeapLab<SIGNED, G>, GroupHeapPos<SIGNED, G>>::type>::type H;
    H.init(lane, R);
    H.prepare(lane, K);
    uint32_t bound = SIGNED ? 0x7fu : 0xffu;
    // slot cursor (wave-uniform): flat blocks [c0, c1) belong to slot s, a list of n_s rows with its labels at loff_s
    int s = 0, c0 = 0, c1 = S > 0 ? prefix[1] : 0;
    int n_s = S > 0 ? ns[0] : 0;
    int64_t loff_s = S > 0 ? loffs[0] : -1;
    // 64 blocks per step, each lane one block and its minimum; the next step's are requested before this one is replayed
    uint4 nd = never;
    uint32_t nm = SIGNED ? 0x7fu : 0xffu;
    if (lane < total) { nd = drow[lane]; nm = mrow[lane]; }
    for (int base = 0; base < total; base += 64) {
        const uint4 dd = nd;
        const uint32_t mn = nm;
        nd = never;
        nm = SIGNED ? 0x7fu : 0xffu;
        if (base + 64 + lane < total) { nd = drow[base + 64 + lane]; nm = mrow[base + 64 + lane]; }
        // blocks whose minimum is below the bound of now: a superset of what the reference enters (the bound only falls)
        uint64_t mask = __builtin_amdgcn_ballot_w64(byte_lt<SIGNED>(mn, bound));
        // The labels of a voted block — lanes 0..15, one vector load — are requested one voted block ahead (two ahead was
        // measured: no gain).  The slot's row count and label offset live in registers and change only where the cursor
        // steps into the next list: read through `ns[s]` / `loffs[s]` per voted block they were a scalar load each in
        // front of every block's cmp_mask — the build(n_probes=2) index (labels: three such loads per voted block) spent
        // 0.28 ms in this replay against 0.09 for distinct labels.
        // (a macro, not a lambda: a closure over c0 / n_s / loff_s by reference whose body selects between them and
        //  freshly loaded values went to scratch — 12 bytes per lane, tests/test_kernel_resources.py)
#define TK_LOAD_LABELS(out_, f2_)                                                          \
        {                                                                                  \
            const int f2__ = (f2_);                                                        \
            int a0__ = c0, n2__ = n_s;                                                     \
            int64_t loff2__ = loff_s;                                                      \
            if (f2__ >= c1) {       /* (rare: the next voted block lies in a later list) */ \
                int s2__ = s, a1__ = c1;                                                   \
                while (f2__ >= a1__) { s2__++; a0__ = a1__; a1__ = prefix[s2__ + 1]; }     \
                n2__ = ns[s2__];                                                           \
                loff2__ = loffs[s2__];                                                     \
            }                                                                              \
            const int64_t inl2__ = 16 * (int64_t)(f2__ - a0__) + lane;                     \
            (out_) = -2;                                                                   \
            if (lane < 16 && inl2__ < n2__) (out_) = loff2__ < 0 ? inl2__ : labels[loff2__ + inl2__]; \
        }
        int j_pref = -1;
        int64_t lab_pref = -2;
        while (mask) {
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int f = base + j;
            while (f >= c1) {            // (empty lists: several steps)
                s++;
                c0 = c1;
                c1 = prefix[s + 1];
                n_s = ns[s];
                loff_s = loffs[s];
            }
            const int rows = n_s - 16 * (f - c0);           // `pos < n`, _fast_pq_256.pyx:111
            int64_t lab_cur = -2;
            if (NEEDS_LABELS) {
                if (j == j_pref) lab_cur = lab_pref;
                else TK_LOAD_LABELS(lab_cur, f)
                // The labels of THIS block are taken into use here, in front of the next request: the compiler waits
                // for a load with `s_waitcnt vmcnt(0)` at its first use (it cannot count loads across the loop's back
                // edge); with that first use behind the next request the "prefetch" would be waited for at once.
                // (Worth 3 % on the build(n_probes=2) index, 0.254 -> 0.245 ms per query: its replay is 2.7 x the one
                // over distinct labels because the lists are twice as long and every near row is met twice — ~1 240
                // candidates and ~800 inserts against 620 — not because of the labels' trip to memory.)
                uint32_t cur_lo = (uint32_t)lab_cur, cur_hi = (uint32_t)((uint64_t)lab_cur >> 32);
                asm volatile("" : "+v"(cur_lo), "+v"(cur_hi));
                __builtin_amdgcn_sched_barrier(0);
                lab_cur = (int64_t)(((uint64_t)cur_hi << 32) | cur_lo);
                j_pref = -1;
                if (mask) {                                 // the next voted block of this step (a superset: the bound may fall)
                    j_pref = __builtin_ctzll(mask);
                    TK_LOAD_LABELS(lab_pref, base + j_pref)
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            const uint32_t d0 = __builtin_amdgcn_readlane(dd.x, j);
            const uint32_t d1 = __builtin_amdgcn_readlane(dd.y, j);
            const uint32_t d2 = __builtin_amdgcn_readlane(dd.z, j);
            const uint32_t d3 = __builtin_amdgcn_readlane(dd.w, j);
            // the reference's cmp_mask of this block against the bound captured at its start: row r in lane r
            // (block_byte(d0, d1, d2, d3, lane), written out: through the call the <true, 4> form parks one SGPR more)
            const uint32_t w = lane < 4 ? d0 : lane < 8 ? d1 : lane < 12 ? d2 : d3;
            const uint32_t by = (w >> (8 * (lane & 3))) & 0xffu;
            uint32_t bits = (uint32_t)__builtin_amdgcn_ballot_w64(lane < 16 && lane < rows && byte_lt<SIGNED>(by, bound));
            if (!bits) continue;
            const uint32_t pos0 = (uint32_t)(16 * f);
            while (bits) {               // every passing row goes in, in row order, without a second look (:113-118)
                const int r = __builtin_ctz(bits);
                bits &= bits - 1;
                const uint32_t byr = __builtin_amdgcn_readlane(by, r);
                const int v = SIGNED ? (int)(int8_t)byr : (int)byr;
                if constexpr (LABELS) {
                    const uint32_t llo = __builtin_amdgcn_readlane((uint32_t)lab_cur, r);
                    const uint32_t lhi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)lab_cur >> 32), r);
                    if (H.holds(llo, lhi)) continue;
                    H.insert(llo, lhi, v, lane, K);
                } else if constexpr (KIND == 2) {
                    const uint32_t l24 = __builtin_amdgcn_readlane((uint32_t)lab_cur, r) & 0x00ffffffu;
                    if (H.holds24(l24)) continue;
                    H.insert((byr << 24) | l24, v, lane, K);
                } else {
                    H.insert((byr << 24) | (pos0 + (uint32_t)r), v, lane, K);
                }
            }
            bound = H.bound();                                              // refresh behind the block, :123
            b_plain = f < plain0 ? bound : b_plain;                         // (plain_scan.hip's lemma: the bound at the first plain block)
            if (mask) mask &= __builtin_amdgcn_ballot_w64(byte_lt<SIGNED>(mn, bound));
        }
    }
#undef TK_LOAD_LABELS
    // heap arrays out, in the reference's layout: node 0 = the root, node 2 t + 1 + slot = the slot of lane L, group g (t = 64 g + L)
    auto resolve = [&](uint32_t e) -> int64_t {      // a flat position back to (list, row): its label (KIND 2: the label itself)
        const uint32_t pos = e & 0x00ffffffu;
        if (KIND == 2) return pos == 0x00ffffffu ? -1 : (int64_t)pos;
        return resolve_position(pos, prefix, loffs, S, labels);
    };
    if constexpr (G == 1 && LABELS) {
        if (lane == 0) { oi[0] = (int64_t)(((uint64_t)H.hir << 32) | H.lor); ov[0] = H.vr; }
        if (2 * lane + 1 < R) { oi[2 * lane + 1] = (int64_t)(((uint64_t)H.hi0 << 32) | H.lo0); ov[2 * lane + 1] = H.v0; }
        if (2 * lane + 2 < R) { oi[2 * lane + 2] = (int64_t)(((uint64_t)H.hi1 << 32) | H.lo1); ov[2 * lane + 2] = H.v1; }
    } else if constexpr (G == 1) {
        if (lane == 0) { oi[0] = resolve(H.er); ov[0] = entry_val<SIGNED>(H.er); }
        if (2 * lane + 1 < R) { oi[2 * lane + 1] = resolve(H.e0); ov[2 * lane + 1] = entry_val<SIGNED>(H.e0); }
        if (2 * lane + 2 < R) { oi[2 * lane + 2] = resolve(H.e1); ov[2 * lane + 2] = entry_val<SIGNED>(H.e1); }
    } else if constexpr (LABELS) {
        if (lane == 0) { oi[0] = (int64_t)(((uint64_t)H.hir << 32) | H.lor); ov[0] = H.vr; }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int t0 = 2 * (64 * g + lane) + 1;
            if (t0 < R) { oi[t0] = (int64_t)(((uint64_t)H.hi0[g] << 32) | H.lo0[g]); ov[t0] = H.v0[g]; }
            if (t0 + 1 < R) { oi[t0 + 1] = (int64_t)(((uint64_t)H.hi1[g] << 32) | H.lo1[g]); ov[t0 + 1] = H.v1[g]; }
        }
    } else {
        if (lane == 0) { oi[0] = resolve(H.er); ov[0] = entry_val<SIGNED>(H.er); }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int t0 = 2 * (64 * g + lane) + 1;
            if (t0 < R) { oi[t0] = resolve(H.e0[g]); ov[t0] = entry_val<SIGNED>(H.e0[g]); }
            if (t0 + 1 < R) { oi[t0 + 1] = resolve(H.e1[g]); ov[t0 + 1] = entry_val<SIGNED>(H.e1[g]); }
        }
    }
}

// One wave per query.  dist / mins / slot tables as heap_replay_packed_kernel; `flags`: queries that need the duplicate
// test although labels are distinct (a probe list that names a list twice); dedupe_all: labels repeat in the index.
// plain0_arr / qlim / flag_list (plain_scan.hip: the blocks from flat chunk plain0_arr[q] on carry clamp(plain sums)): the
// replay checks the lemma's condition per query as the lane kernel does — bound at the first plain block <= qlim[q] —
// and lists the queries that fail it, and those flagged beforehand, for the exact re-scan behind it (flags[q] = 2).
template <bool SIGNED, int G>
__global__ __launch_bounds__(64) void heap_replay_pair_kernel(
    const uint4 *__restrict__ dist, int64_t cap, const uint8_t *__restrict__ mins, int64_t cap_min,
    const int *__restrict__ slot_prefix, const int *__restrict__ slot_n, const int64_t *__restrict__ slot_label_off,
    int S, const int64_t *__restrict__ labels, int64_t *__restrict__ heap_idx, int32_t *__restrict__ heap_val, int R,
    int slots_uniform, unsigned char *__restrict__ flags, int dedupe_all, int64_t nq,
    const int *__restrict__ plain0_arr, const int *__restrict__ qlim, int *__restrict__ flag_list, int only_flagged,
    const int *__restrict__ count_src, volatile int *host_count)
{
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    // (the count of the flagged queries to the page-locked word the host polls: plain_scan's state machine)
    if (host_count && count_src && q == 0 && lane == 0) *host_count = count_src[0];
    if (q >= nq) return;
    const bool flagged = flags && flags[q];
    if (only_flagged && !flagged) return;      // the tail behind a lane replay: the queries it left (re-scanned exactly)
    __builtin_amdgcn_s_setprio(3);
    const int64_t qs = slots_uniform ? 0 : q;
    if (plain0_arr && flagged) {       // (its rows hold plain sums: left, with the queries that fail the check, to the kernels behind)
        if (lane == 0 && flag_list) flag_list[1 + atomicAdd(&flag_list[0], 1)] = (int)q;
        return;
    }
    const int plain0 = plain0_arr ? plain0_arr[q] : 0x7fffffff;
    uint32_t b_plain = SIGNED ? 0x7fu : 0xffu;
    const int *prefix = slot_prefix + qs * (S + 1);
    // dedupe_all: bit 0 = every query takes the duplicate test (labels repeat in the index), bit 1 = every label is below 0xffffff
    const uint4 *drow = dist + q * cap;
    const uint8_t *mrow = mins + q * cap_min;
    const int *ns = slot_n + qs * S;
    const int64_t *loffs = slot_label_off + qs * S;
    int64_t *oi = heap_idx + q * R;
    int32_t *ov = heap_val + q * R;
    if (!((dedupe_all & 1) || flagged))
        pair_replay_body<SIGNED, 0, G>(drow, mrow, prefix, ns, loffs, S, labels, oi, ov, R, lane, plain0, b_plain);
    else if (dedupe_all & 2)
        pair_replay_body<SIGNED, 2, G>(drow, mrow, prefix, ns, loffs, S, labels, oi, ov, R, lane, plain0, b_plain);
    else
        pair_replay_body<SIGNED, 1, G>(drow, mrow, prefix, ns, loffs, S, labels, oi, ov, R, lane, plain0, b_plain);
    if (SIGNED && plain0_arr && S > 0 && plain0 < prefix[S] && (int)(int8_t)b_plain > qlim[q] && lane == 0) {
        flags[q] = 2;
        if (flag_list) flag_list[1 + atomicAdd(&flag_list[0], 1)] = (int)q;
    }
}

// tk_positions_fit(cap) (position entries) is the caller's to check where labels are distinct.  The check needs flags and
// signed tables (otherwise none is made); its flag_list (the failing queries listed for a re-scan) has its count zeroed
// here, on the stream, in front of the kernel.  only_flagged: the tail behind a lane replay — queries it flagged,
// re-scanned exactly meanwhile; count_src / host_count: the flagged count the host polls.
int tk_launch_heap_replay_pair(const TkReplayJob &j, unsigned char *flags, int dedupe_all, hipStream_t s,
                               const TkPlainCheck &check, bool only_flagged, const int *count_src, int *host_count)
{
    if (j.nq == 0 || j.R == 0) return 0;
    TkPlainCheck c = check;
    if (!c.plain0 || !c.qlim || !flags || !j.signd) c = TkPlainCheck();
    if (c.flag_list && hipMemsetAsync(c.flag_list, 0, 4, s) != hipSuccess) return -1;
    // two nodes per lane up to 129 entries, four up to 257 (n_probes <= 24 at k = 10), eight up to 513 (n_probes <= 50)
    const int R = j.R, signd = j.signd;
    if (R > TK_PAIR_MAX_R) return -1;
    const auto kernel = R <= 129 ? (signd ? heap_replay_pair_kernel<true, 1> : heap_replay_pair_kernel<false, 1>)
                      : R <= 257 ? (signd ? heap_replay_pair_kernel<true, 2> : heap_replay_pair_kernel<false, 2>)
                                 : (signd ? heap_replay_pair_kernel<true, 4> : heap_replay_pair_kernel<false, 4>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)j.nq), dim3(64), 0, s, j.dist, j.cap, j.mins, j.cap_min, j.slot_prefix,
                       j.slot_n, j.slot_label_off, j.S, j.labels, j.heap_idx, j.heap_val, j.R, j.slots_uniform, flags,
                       dedupe_all, j.nq, c.plain0, c.qlim, c.flag_list, (int)only_flagged, count_src, host_count);
    return 0;
}
