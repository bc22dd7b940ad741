// chunk_mask.h — the masking body the restricting passes share (allow.hip: one set per call; groups.hip: one group
// per query).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// keep: bit r set = row r of the chunk stays.  A chunk whose 16 bits are all set is not touched; one with none set is
// written without being read; else the bytes of the rows that leave take the heap's empty value (127 signed, 255
// unsigned) and the chunk's minimum byte is recomputed (the replays' LAZY form and the block-minimum skips read it).
template <bool SIGNED>
__device__ __forceinline__ void tk_mask_chunk(uint4 *__restrict__ d, uint8_t *__restrict__ m, uint32_t keep16)
{
    const uint32_t fill = SIGNED ? 0x7f7f7f7fu : 0xffffffffu;
    const uint32_t b = keep16;
    if (b == 0xffffu) return;
    if (b == 0) {
        *d = make_uint4(fill, fill, fill, fill);
        *m = (uint8_t)fill;
        return;
    }
    const uint4 v = *d;
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
    int mn = SIGNED ? 127 : 255;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        // nibble j of the row bits -> 0xff in the bytes of the rows that stay
        const uint32_t keep = (((b >> (4 * j)) & 0xfu) * 0x00204081u & 0x01010101u) * 0xffu;
        w[j] = (w[j] & keep) | (fill & ~keep);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t y = (w[j] >> (8 * t)) & 0xffu;
            const int x = SIGNED ? (int)(int8_t)y : (int)y;
            mn = x < mn ? x : mn;
        }
    }
    *d = make_uint4(w[0], w[1], w[2], w[3]);
    *m = (uint8_t)mn;
}
