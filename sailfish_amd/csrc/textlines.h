// textlines.h -- what the device text readers (eqtext.hip: eq_classes.txt, readtext.hip: FASTA / FASTQ) share: a text lies on the
// device as 16-byte groups, the '\n' bytes of every group are counted (each reader's own count kernel: eqtext.hip counts tabs in
// the same pass, readtext.hip counts a range of groups), and an exclusive scan of the counts gives every group its line index.
#pragma once
#include "common.h"

namespace sfgpu {
namespace textlines {

constexpr int kBlock = 256;

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// bit i = byte i of the group is '\n'
__device__ inline uint32_t nl_mask(const uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) m |= (uint32_t)(((w[i >> 2] >> (8 * (i & 3))) & 0xffu) == '\n') << i;
    return m;
}

// line_end[j] = the byte at which line j ends; nl_scan[g] = the '\n' bytes before group g
static __global__ void k_line_ends(const uint4* __restrict__ buf, uint64_t n_groups, const uint32_t* __restrict__ nl_scan,
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

}  // namespace textlines
}  // namespace sfgpu
