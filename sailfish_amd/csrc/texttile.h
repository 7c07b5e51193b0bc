// texttile.h -- the device side of textchunks.h's tiles: what every formatter (eqtext_write.hip, rowtext.h, samtext_write.hip)
// does with the kTileBytes of output its block owns.  The image is the kernel's own `__shared__ uint4 tile4[kBlock]`; a Tile
// zeroes it, knows which bytes of the text it holds, takes bytes clipped to it and stores it, one aligned 16-byte group a lane.
// No barrier is issued here: the kernel synchronises after the constructor (with whatever else it set up) and before store().
#pragma once
#include "textchunks.h"

namespace sfgpu {
namespace textchunks {

// the last i in [0, n) with start[i] <= x, for starts that never decrease and start[0] <= x: the line (row, unit, read) that holds
// byte x of a text whose lines are not empty -- or whose empty lines are to be skipped
template <typename T, typename X>
__device__ __forceinline__ uint64_t holder_of(const T* __restrict__ start, uint64_t n, X x) {
    uint64_t lo = 0, hi = n;                              // start[lo] <= x < start[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

struct Tile {
    char* bytes;                                          // the LDS image
    uint64_t n_bytes, index, base;                        // tile `index` of the text of n_bytes holds its bytes [base, end): fewer than
                                                          // kTileBytes only at the text's end (base < n_bytes: the grid ends with the chunk)
    __device__ __forceinline__ Tile(uint4* tile4, uint64_t first_tile, uint64_t n_bytes)
        : bytes(reinterpret_cast<char*>(tile4)), n_bytes(n_bytes), index(first_tile + blockIdx.x), base(index << kTileShift) {
        tile4[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);  // (the bytes behind the end of the text)
    }
    __device__ __forceinline__ uint64_t end() const { return base + kTileBytes < n_bytes ? base + kTileBytes : n_bytes; }
    // tile offset p, which may lie before or behind the tile
    __device__ __forceinline__ void put(int64_t p, char ch) const {
        if (p >= 0 && p < (int64_t)kTileBytes) bytes[p] = ch;
    }
    // `out` is the chunk buffer, whose byte 0 is text byte out_base (a multiple of kTileBytes)
    __device__ __forceinline__ void store(uint64_t out_base, uint4* __restrict__ out) const {
        const uint64_t g = base + 16ull * threadIdx.x;
        if (g < n_bytes) out[(g - out_base) >> 4] = reinterpret_cast<const uint4*>(bytes)[threadIdx.x];
    }
};

}  // namespace textchunks
}  // namespace sfgpu
