// textlines.h -- what the device text readers (eqtext.hip: eq_classes.txt, readtext.hip: FASTA / FASTQ) share: a text lies on the
// device as 16-byte groups, the '\n' bytes of every group are counted (each reader's own count kernel: eqtext.hip counts tabs in
// the same pass, readtext.hip counts a range of groups), and an exclusive scan of the counts gives every group its line index.
// genemap.hip and samtext.hip cut their masks to the text's length (eq_mask, range_mask) and find the end of the whole lines of a
// device text with k_last_nl.
#pragma once
#include "common.h"

namespace sfgpu {
namespace textlines {

constexpr int kBlock = 256;

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// bit i = byte i of the group is c
__device__ inline uint32_t eq_mask(const uint4 v, unsigned char c) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) m |= (uint32_t)(((w[i >> 2] >> (8 * (i & 3))) & 0xffu) == c) << i;
    return m;
}

// bit i = byte p0 + i lies in [s, e)
__device__ inline uint32_t range_mask(uint64_t p0, uint64_t s, uint64_t e) {
    if (p0 >= e || p0 + 16 <= s) return 0;
    const uint32_t lo = s > p0 ? (uint32_t)(s - p0) : 0, hi = e - p0 >= 16 ? 16u : (uint32_t)(e - p0);
    return ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// bit i = byte i of the group is '\n'
__device__ inline uint32_t nl_mask(const uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) m |= (uint32_t)(((w[i >> 2] >> (8 * (i & 3))) & 0xffu) == '\n') << i;
    return m;
}

// line_end[j] = the byte at which line j ends; nl_scan[g] = the '\n' bytes before group g
[[maybe_unused]] static __global__ void k_line_ends(const uint4* __restrict__ buf, uint64_t n_groups, const uint32_t* __restrict__ nl_scan,
                                   uint32_t* __restrict__ line_end) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    uint32_t nl = nl_mask(buf[g]);
    uint32_t at = nl_scan[g];
    while (nl) {
        const int i = __ffs(nl) - 1;
        nl &= nl - 1;
        line_end[at++] = (uint32_t)(g * 16 + i);
    }
}

// *last (zeroed by the caller) = the byte behind the last '\n' below n (0: none): where the whole lines of a device text end
[[maybe_unused]] static __global__ void k_last_nl(const unsigned char* __restrict__ bytes, uint64_t n, unsigned long long* __restrict__ last) {
    const uint64_t p0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16u;
    unsigned long long best = 0;
    for (uint64_t p = p0; p < n && p < p0 + 16u; ++p)
        if (bytes[p] == '\n') best = p + 1;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && best) atomicMax(last, best);
}

}  // namespace textlines
}  // namespace sfgpu
