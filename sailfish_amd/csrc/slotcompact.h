// slotcompact.h -- the last device step of the slot writers (slotpipe.h; gzwrite.hip's blocks, bgzf_write.hip's members): every
// workgroup has left its bytes in a slot of kSlotBytes at a 16-byte boundary, a scan of the lengths gives the byte offsets, and
// this kernel moves the slots there.  Blocks and members end on byte boundaries, so no bit is touched.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sfgpu {

// slot b (16-byte aligned, blk_off[b + 1] - blk_off[b] bytes) to out + blk_off[b]: aligned dwords of the destination from two
// aligned dwords of the slot, the ragged ends byte by byte
template <uint32_t kSlotBytes>
__global__ void __launch_bounds__(256)
k_slot_compact(const uint8_t* __restrict__ slots, const uint64_t* __restrict__ blk_off, uint8_t* __restrict__ out) {
    const uint8_t* src = slots + (uint64_t)blockIdx.x * kSlotBytes;
    const uint64_t o0 = blk_off[blockIdx.x];
    const uint32_t len = (uint32_t)(blk_off[blockIdx.x + 1] - o0);
    uint8_t* dst = out + o0;
    uint32_t head = (uint32_t)((4u - (o0 & 3u)) & 3u);
    if (head > len) head = len;
    const uint32_t n_dw = (len - head) / 4u, tail0 = head + 4u * n_dw;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    if (threadIdx.x < len - tail0) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    const uint32_t sh = 8u * head;                      // the slot is aligned: source byte head + 4 k sits `head` bytes into dword k
    for (uint32_t k = threadIdx.x; k < n_dw; k += blockDim.x)
        dw[k] = head ? (sw[k] >> sh) | (sw[k + 1] << (32u - sh)) : sw[k];
}

}  // namespace sfgpu
