// wave_crc.h -- the CRC-32 of a payload one wavefront has just written, shared by the device inflaters (bgzf_read.hip, gz_read.hip).
#pragma once
#include "common.h"
#include "gzfmt.h"

namespace sfgpu {

// CRC-32 of out[0 .. n): lane slices in order, then a tree of combinations (crc of A || B from crc A, crc B and |B|); all lanes
// return it
static __device__ __noinline__ uint32_t wave_crc32(const uint8_t* out, uint32_t n, uint32_t lane, const uint32_t* crc_table) {
    const uint32_t per = (n + 63u) / 64u;
    const uint32_t a = lane * per < n ? lane * per : n, b = a + per < n ? a + per : n;
    uint32_t crc = crc32_slice(0u, crc_table, [&](uint32_t i) -> uint32_t { return out[a + i]; }, b - a);
    uint32_t len = b - a;
#pragma unroll 1
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t crc_hi = __shfl_down(crc, o), len_hi = __shfl_down(len, o);
        crc = crc32_combine(crc, crc_hi, len_hi);
        len += len_hi;
    }
    return __shfl(crc, 0);
}

}  // namespace sfgpu
