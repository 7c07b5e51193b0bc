// deflate_wg.h -- the stages of a DEFLATE-encoding workgroup that do not depend on its parse (device only), shared by k_gz_encode
// (gzwrite.hip) and k_bgzw_encode (bgzf_write.hip).  One lane owns one 64-byte slice of the workgroup's block of kThreads x 64
// bytes.  The arithmetic is gzfmt.h's; the LDS state lives in sub-structs that each kernel's EncodeLds embeds.
// COLLECTIVE functions hold barriers or shuffles: every lane of the workgroup must call them.
#pragma once
#include "common.h"
#include "gzfmt.h"

namespace sfgpu {

constexpr uint32_t kWgSlice = 64;                       // bytes of the block per lane
constexpr uint32_t kInStride = 17;                      // dwords per slice in LDS

// dword d of the block at `in` (any alignment); bytes at or behind n read as 0
__device__ inline uint32_t load_dword(const uint8_t* __restrict__ in, uint32_t d, uint32_t n) {
    const uint32_t b = 4u * d;
    if (b >= n) return 0u;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(in) + b;
    const uint32_t a = (uint32_t)(addr & 3u);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(addr - a);
    uint32_t v = w[0];
    if (a) {
        v >>= 8u * a;
        if (b + (4u - a) < n) v |= w[1] << (32u - 8u * a);          // the next dword holds bytes of the block
    }
    const uint32_t left = n - b;
    return left >= 4u ? v : v & ((1u << (8u * left)) - 1u);
}

// the first n bytes from `in`, zeros behind them, into lds_in at 17 dwords per slice (lanes walking their slices hit different
// banks).  Called by every lane; a barrier comes before the first read.
template <int kThreads>
__device__ __forceinline__ void wg_stage_input(uint32_t* lds_in, const uint8_t* __restrict__ in, uint32_t n, uint32_t tid) {
    for (uint32_t k = 0; k < kWgSlice / 4; ++k) {
        const uint32_t d = tid + k * kThreads;
        lds_in[(d >> 4) * kInStride + (d & 15u)] = load_dword(in, d, n);
    }
}

struct CrcLds {
    uint32_t table[256];
    uint32_t xp[12];                                    // x^(8 x 64 x 2^k) mod P
    uint32_t full, part;                                // the full slices, weighted and summed; the last, partial slice
};

// COLLECTIVE (shuffles).  Folds in `crc`, the CRC-32 of the lane's slice (`len` bytes of a block of n).  Full slices are weighted
// by x^(8 x 64 x slices behind them), log2(kThreads) factors at most; wg_crc_member applies the partial slice's factor to their sum.
template <int kThreads>
__device__ __forceinline__ void wg_crc_fold(CrcLds& c, uint32_t crc, uint32_t tid, uint32_t lane, uint32_t n, uint32_t len) {
    static_assert(kThreads > 320 && kThreads <= 4096, "lane 320 exists; xp[12] reaches every slice");
    const uint32_t full = n / kWgSlice;
    uint32_t p = 0u;
    if (tid < full) {
        p = crc;
        const uint32_t behind = full - tid - 1u;
        for (int k = 0; (1 << k) < kThreads; ++k) if ((behind >> k) & 1u) p = crc32_mulmod(c.xp[k], p);
    } else if (tid == full && len) {
        c.part = crc;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) p ^= __shfl_xor(p, o);
    if (lane == 0 && p) atomicXor(&c.full, p);
}

// CRC-32 of the block's n bytes, behind a barrier that follows wg_crc_fold
__device__ __forceinline__ uint32_t wg_crc_member(const CrcLds& c, uint32_t n) {
    const uint32_t r = n % kWgSlice;
    return r ? crc32_mulmod(crc32_xpow8(r), c.full) ^ c.part : c.full;
}

struct LitCodeLds {
    uint32_t hist[288];
    uint32_t node_freq[2 * kGzLitSyms];
    uint32_t count[kGzMaxBits + 1], first[kGzMaxBits + 1];
    uint32_t n_used;
    uint16_t order[288], parent[2 * kGzLitSyms], codes[288];
    uint8_t lens[288];
};

// the CRC table [one lane per entry], the powers [lane 320] and an empty histogram.  Called by every lane; a barrier comes before
// wg_crc_fold and before the first count.
__device__ __forceinline__ void wg_init(CrcLds& c, LitCodeLds& L, uint32_t tid) {
    if (tid < 256) c.table[tid] = crc32_table_entry(tid);
    if (tid < 288) { L.hist[tid] = 0u; L.lens[tid] = 0; L.codes[tid] = 0; }
    if (tid <= (uint32_t)kGzMaxBits) L.count[tid] = 0u;
    if (tid == 320) {
        uint32_t p = 0x00800000u;                       // x^8
        for (int k = 0; k < 6; ++k) p = crc32_mulmod(p, p);        // x^(8 x 64)
        for (int k = 0; k < 12; ++k) { c.xp[k] = p; p = crc32_mulmod(p, p); }
        c.full = 0u; c.part = 0u;
    }
}

// COLLECTIVE (five barriers, the last one at the end).  From the complete L.hist (>= 2 used symbols) behind a barrier: L.lens and
// L.codes as huff_lengths_serial and huff_code_rev give them, by rank [lane per symbol], merge [one lane], depths [lane per leaf],
// Kraft repair [one lane], lengths and codes [lane per symbol].  aside() runs beside the merge; it holds no barrier of its own.
template <typename Aside>
__device__ __forceinline__ void wg_lit_code_build(LitCodeLds& L, uint32_t tid, Aside aside) {
    if (tid < (uint32_t)kGzLitSyms && L.hist[tid]) {
        int u;
        const int r = huff_rank(L.hist, kGzLitSyms, (int)tid, &u);
        L.order[r] = (uint16_t)tid;
        if (tid == (uint32_t)kGzEob) L.n_used = (uint32_t)u;
    }
    __syncthreads();
    const int n_used = (int)L.n_used;
    if (tid == 0) huff_merge(L.hist, L.order, n_used, L.node_freq, L.parent);
    aside();
    __syncthreads();
    if (tid < (uint32_t)n_used) {
        const int d = huff_depth(L.parent, (int)tid, 2 * n_used - 2);
        atomicAdd(&L.count[d < kGzMaxBits ? d : kGzMaxBits], 1u);
    }
    __syncthreads();
    if (tid == 0) { huff_limit(L.count, kGzMaxBits); huff_first_codes(L.count, kGzMaxBits, L.first); }
    __syncthreads();
    if (tid < (uint32_t)n_used) L.lens[L.order[tid]] = (uint8_t)huff_len_of_rank(L.count, (int)tid, kGzMaxBits);
    __syncthreads();
    if (tid < (uint32_t)kGzLitSyms && L.lens[tid]) {
        const int l = L.lens[tid];
        uint32_t code = L.first[l];
        for (uint32_t s = 0; s < tid; ++s) code += L.lens[s] == l;
        L.codes[tid] = (uint16_t)gz_rev_bits(code, l);
    }
    __syncthreads();
}

struct WgBits { uint32_t before, body; };               // bits of the lanes in front of this one; bits of all lanes

// COLLECTIVE (shuffles and one barrier).  wave_sum: kThreads / kWave words of LDS.
template <int kThreads>
__device__ __forceinline__ WgBits wg_scan_bits(uint32_t* wave_sum, uint32_t my_bits, uint32_t lane, uint32_t wave) {
    uint32_t incl = my_bits;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t other = __shfl_up(incl, o);
        if ((int)lane >= o) incl += other;
    }
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    WgBits r{incl - my_bits, 0u};
    for (uint32_t w = 0; w < (uint32_t)(kThreads / kWave); ++w) { const uint32_t s = wave_sum[w]; if (w < wave) r.before += s; r.body += s; }
    return r;
}

// the image's first out_len bytes, rounded up to 16, to the slot.  Called by every lane behind the image's last barrier.
template <int kThreads>
__device__ __forceinline__ void wg_store_image(const uint32_t* img, uint32_t out_len, uint4* __restrict__ slot, uint32_t tid) {
    const uint4* img4 = reinterpret_cast<const uint4*>(img);
    for (uint32_t i = tid; i < (out_len + 15u) / 16u; i += kThreads) slot[i] = img4[i];
}

}  // namespace sfgpu
