// heap_common.h — what the heap replays share (heap.hip, heap_wave.hip, heap_flat.hip, heap_pair.hip): the LDS
// address-space types, the byte compares of a 16-row distance block against a bound, and the way from a packed
// entry's flat position back to its label.
#pragma once

#include "kernels.h"

// Heap state shared by the lanes of a wave lives in LDS and is accessed through
// address-space-3 volatile pointers: volatile keeps every access in program order
// (one lane stores, all lanes load), and the explicit address space keeps them
// ds_read/ds_write — a volatile access through a generic pointer compiles to
// flat_load/flat_store sc0 sc1 with a vmcnt(0) wait each, ~10x slower.
typedef __attribute__((address_space(3))) volatile uint32_t lds_vu32;
typedef __attribute__((address_space(3))) volatile int32_t lds_vi32;
typedef __attribute__((address_space(3))) volatile int64_t lds_vi64;
#define LDS_PTR(T, p) ((T *)(__attribute__((address_space(3))) unsigned char *)(p))

template <bool SIGNED>
__device__ __forceinline__ bool byte_lt(uint32_t d, uint32_t bound8)
{
    if (SIGNED) return (int)(int8_t)d < (int)(int8_t)bound8;
    return d < bound8;
}

template <bool SIGNED>
__device__ __forceinline__ bool any_lt16(const uint4 v, uint32_t bound8)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    bool any = false;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int b = 0; b < 4; b++) any |= byte_lt<SIGNED>((w[i] >> (8 * b)) & 0xffu, bound8);
    return any;
}

// a block no row of which is ever below a bound
template <bool SIGNED>
__device__ __forceinline__ uint4 never16()
{
    return SIGNED ? make_uint4(0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu)
                  : make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
}

// byte r (row r's distance) of a 16-byte block held in four dwords
__device__ __forceinline__ uint32_t block_byte(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, int r)
{
    const uint32_t w = r < 4 ? d0 : r < 8 ? d1 : r < 12 ? d2 : d3;
    return (w >> (8 * (r & 3))) & 0xffu;
}
__device__ __forceinline__ uint32_t block_byte(const uint4 dd, int r) { return block_byte(dd.x, dd.y, dd.z, dd.w, r); }

// packed entries: value8 << 24 | flat position24 (or slot24)
template <bool SIGNED>
__device__ __forceinline__ int entry_val(uint32_t e)
{
    return SIGNED ? ((int32_t)e >> 24) : (int)(e >> 24);
}

// The 16-bit mask "row r < bound" of a block by byte-parallel arithmetic (22 VALU instead of ~75: the lane replay is a
// dependent-issue chain on a wave that has its SIMD to itself, so its time IS its instruction
// count).  Per dword: bytes as unsigned (signed: top bits flipped), x < b per byte from
// t = (x | H) - (b & ~H) — no borrow crosses a byte — as  (~x7 & b7) | (~(x7 ^ b7) & ~t7)  in bit 7
// of every byte; v_dot4_u32_u8 with weights 1,2,4,8 / 16,..,128 gathers the four 0x80 flags of a
// dword into a nibble.  `bb`: the bound's byte (biased for SIGNED) in all four bytes.
template <bool SIGNED>
__device__ __forceinline__ uint32_t bound_bytes(uint32_t bound8)
{
    const uint32_t b = SIGNED ? (bound8 ^ 0x80u) : bound8;
    return __builtin_amdgcn_perm(b, b, 0u);       // byte 0 in every byte
}

template <bool SIGNED>
__device__ __forceinline__ uint32_t lt4(uint32_t x, uint32_t bb, uint32_t bl)
{
    const uint32_t H = 0x80808080u;
    const uint32_t xu = SIGNED ? (x ^ H) : x;
    const uint32_t t = (xu | H) - bl;
    return ((~xu & bb) | (~(xu ^ bb) & ~t)) & H;
}

template <bool SIGNED>
__device__ __forceinline__ uint32_t mask_lt16_swar(const uint4 v, uint32_t bb)
{
    const uint32_t bl = bb & 0x7f7f7f7fu;
    uint32_t lo = __builtin_amdgcn_udot4(lt4<SIGNED>(v.x, bb, bl), 0x08040201u, 0u, false);
    lo = __builtin_amdgcn_udot4(lt4<SIGNED>(v.y, bb, bl), 0x80402010u, lo, false);
    uint32_t hi = __builtin_amdgcn_udot4(lt4<SIGNED>(v.z, bb, bl), 0x08040201u, 0u, false);
    hi = __builtin_amdgcn_udot4(lt4<SIGNED>(v.w, bb, bl), 0x80402010u, hi, false);
    return (lo >> 7) | (hi << 1);
}

// The label behind the low 24 bits of a position entry: flat position `pos` of the query's rows lies in the slot s
// with prefix[s] <= pos / 16 < prefix[s + 1]; its label is labels[loffs[s] + row in the list], or the row itself
// where the slot has no labels (loffs[s] < 0).  0xffffff is the fresh entry: no row, label -1.
__device__ __forceinline__ int64_t resolve_position(uint32_t pos, const int *prefix, const int64_t *loffs, int S,
                                                    const int64_t *labels)
{
    if (pos == 0x00ffffffu) return -1;
    const int f = (int)(pos >> 4);
    int lo = 0, hi = S;  // prefix[lo] <= f < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= f) lo = mid; else hi = mid;
    }
    const int64_t inlist = (int64_t)pos - 16 * (int64_t)prefix[lo];
    const int64_t loff = loffs[lo];
    return loff < 0 ? inlist : labels[loff + inlist];
}
