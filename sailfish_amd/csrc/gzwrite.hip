// gzwrite.hip -- aux/bootstrap/bootstraps.gz written from the device (GZipWriter::writeBootstrap<T>, src/GZipWriter.cpp:249-285:
// every sample appended as raw little-endian binary to one gzip stream): sfgpu_gz_open / sfgpu_gz_write_device / sfgpu_gz_close.
//
// The arithmetic (CRC-32, the run-match parse, code lengths, canonical codes, the block header, framing) is gzfmt.h, which the
// CPU tests drive serially; this file is the parallel driver.  A write is cut into independent blocks of 64 KB, one workgroup of
// 1024 lanes each (k_gz_encode); lane l owns the 64-byte slice l of the block:
//   load    the block into LDS, 17 dwords per slice (a lane walking its slice and its neighbours walking theirs hit different banks)
//   mask    bit i = "byte i equals byte i - 1", one 64-bit word per lane; the CRC-32 of the slice by table, weighted by
//           x^(8 x bytes behind the slice) and XOR-reduced over the block; a max-scan gives every lane the last clear bit before it
//   parse   gz_chunk_tokens: the tokens of the greedy parse that start in the slice, found from the mask alone; histogram in LDS
//   codes   rank of every used symbol by (frequency, symbol) [one lane per symbol], two-queue merge [one lane], leaf depths
//           [one lane per leaf], Kraft repair of the depth counts [one lane], lengths by rank and canonical codes [one lane per symbol]
//   header  the code lengths in run-length form, their 7-bit code, the header bits into the image [one lane]
//   pack    bits per slice, a block scan for the bit offsets, the codes ORed into the LDS image (LDS atomics: OR commutes, the
//           image does not depend on their order); a block that would not be shorter than its stored form is laid out stored
//   store   the image to the block's slot, 16 bytes per lane
// A block ends on a byte boundary (gzfmt.h), so k_gz_compact moves the slots to their scanned byte offsets without touching bits.
// LDS: 69 632 B input + 65 568 B image + 8 KB mask + ~8 KB tables = 152 KB of the CU's 160 KB: one workgroup = 16 waves per CU,
// 4 per SIMD.
// The compressed bytes of a batch (<= 1024 blocks) are copied through two pinned buffers in pieces of <= chunk_bytes and handed
// to the sink; batch b + 1 is encoded, and piece p + 1 copied, while the sink holds piece p.
#include "common.h"
#include "gzfmt.h"
#include "primitives.h"

#include <cstring>
#include <new>

namespace sfgpu {
namespace {

constexpr int kThreads = 1024;                          // = kGzBlockBytes / kSlice
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kSlice = 64;
constexpr uint32_t kInStride = 17;                      // dwords per slice in LDS
constexpr uint32_t kImgWords = 16392;                   // gz_stored_bytes(65536) = 65546 -> 16-byte groups, + room for the second word of an OR
constexpr uint32_t kSlotBytes = kImgWords * 4;
constexpr uint32_t kBatchBlocks = 1024;                 // 64 MiB of payload per launch
constexpr uint64_t kDefaultChunk = 32ull << 20;
constexpr uint64_t kMaxChunk = 1ull << 30;
static_assert(kThreads * kSlice == kGzBlockBytes, "one lane per slice");
static_assert(kSlotBytes % 16 == 0 && kSlotBytes >= 65546 + 8, "a slot holds the stored form");

struct alignas(16) EncodeLds {
    uint32_t img[kImgWords];
    uint32_t in[kThreads * kInStride];
    uint64_t eq[kThreads + 8];
    uint32_t crc_table[256];
    uint32_t hist[288];
    uint32_t node_freq[2 * kGzLitSyms];
    uint32_t count[kGzMaxBits + 1], first[kGzMaxBits + 1];
    uint32_t wave_sum[kWaves];
    int32_t wave_z[kWaves];
    uint32_t xp[12];                                    // x^(8 x 64 x 2^k) mod P
    uint32_t n_used, hdr_bits, crc_full, crc_part;
    uint16_t order[288], parent[2 * kGzLitSyms], codes[288];
    uint8_t lens[288];
    GzClWork clw;
};

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

__global__ void __launch_bounds__(kThreads)
k_gz_encode(const uint8_t* __restrict__ src, uint64_t n_bytes, uint4* __restrict__ slots, uint32_t* __restrict__ blk_len,
            uint32_t* __restrict__ blk_crc, uint32_t* __restrict__ blk_stored) {
    __shared__ EncodeLds S;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint64_t base = (uint64_t)blockIdx.x * kGzBlockBytes;
    const uint32_t n = n_bytes - base < kGzBlockBytes ? (uint32_t)(n_bytes - base) : kGzBlockBytes;
    const uint8_t* in = src + base;

    // ---- load
    for (uint32_t i = tid; i < kImgWords; i += kThreads) S.img[i] = 0u;
    if (tid < 288) { S.hist[tid] = 0u; S.lens[tid] = 0; S.codes[tid] = 0; }
    if (tid < 256) S.crc_table[tid] = crc32_table_entry(tid);
    if (tid < 8) S.eq[kThreads + tid] = 0ull;
    if (tid <= (uint32_t)kGzMaxBits) S.count[tid] = 0u;
    if (tid == 320) {
        uint32_t p = 0x00800000u;                       // x^8
        for (int k = 0; k < 6; ++k) p = crc32_mulmod(p, p);        // x^(8 x 64)
        for (int k = 0; k < 12; ++k) { S.xp[k] = p; p = crc32_mulmod(p, p); }
        S.crc_full = 0u; S.crc_part = 0u;
    }
    for (uint32_t k = 0; k < kGzBlockBytes / 4 / kThreads; ++k) {
        const uint32_t d = tid + k * kThreads;
        S.in[(d >> 4) * kInStride + (d & 15u)] = load_dword(in, d, n);
    }
    __syncthreads();

    // ---- mask, CRC of the slice, last clear bit
    const uint32_t c0 = tid * kSlice;
    const uint32_t len = c0 < n ? (n - c0 < kSlice ? n - c0 : kSlice) : 0u;
    auto byte_at = [&](uint32_t i) -> uint32_t { return (S.in[(i >> 6) * kInStride + ((i & 63u) >> 2)] >> (8u * (i & 3u))) & 0xffu; };
    uint64_t mask = 0;
    uint32_t crc = 0xffffffffu;
    {
        uint32_t prev = tid ? S.in[(tid - 1) * kInStride + 15] >> 24 : 0x100u;
        for (uint32_t w = 0; w < 16; ++w) {
            const uint32_t v = S.in[tid * kInStride + w];
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t j = 4u * w + b, byte = (v >> (8u * b)) & 0xffu;
                if (j < len) {
                    if (byte == prev) mask |= 1ull << j;
                    crc = S.crc_table[(crc ^ byte) & 0xffu] ^ (crc >> 8);
                }
                prev = byte;
            }
        }
        crc = ~crc;
    }
    S.eq[tid] = mask;
    {
        // slices in front of the last (partial) one are weighted by x^(8 x 64 x slices behind them); the factor of the partial
        // slice's bytes is applied once to their sum
        const uint32_t full = n / kSlice;
        uint32_t p = 0u;
        if (tid < full) {
            p = crc;
            const uint32_t behind = full - tid - 1u;
            for (int k = 0; k < 10; ++k) if ((behind >> k) & 1u) p = crc32_mulmod(S.xp[k], p);
        } else if (tid == full && len) {
            S.crc_part = crc;
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) p ^= __shfl_xor(p, o);
        if (lane == 0 && p) atomicXor(&S.crc_full, p);
    }
    int32_t z_incl;
    {
        const uint64_t clear = ~mask;
        z_incl = clear ? (int32_t)(c0 + 63u - (uint32_t)gz_clz64(clear)) : -1;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int32_t other = __shfl_up(z_incl, o);
            if ((int)lane >= o && other > z_incl) z_incl = other;
        }
        if (lane == kWave - 1) S.wave_z[wave] = z_incl;
    }
    __syncthreads();
    int32_t z_in = __shfl_up(z_incl, 1);
    if (lane == 0) z_in = -1;
    for (uint32_t w = 0; w < wave; ++w) { const int32_t o = S.wave_z[w]; if (o > z_in) z_in = o; }

    // ---- parse: the histogram
    auto eqw = [&](uint32_t w) -> uint64_t { return S.eq[w]; };
    gz_chunk_tokens(eqw, c0, c0 + kSlice, n, z_in, [&](uint32_t pos, uint32_t l) {
        atomicAdd(&S.hist[gz_token_symbol(byte_at(pos), l)], 1u);
    });
    if (tid == 0) atomicAdd(&S.hist[kGzEob], 1u);
    __syncthreads();

    // ---- code lengths and codes of the literal/length alphabet (huff_lengths_serial, one lane per item where items are independent)
    if (tid < (uint32_t)kGzLitSyms && S.hist[tid]) {
        int u;
        const int r = huff_rank(S.hist, kGzLitSyms, (int)tid, &u);
        S.order[r] = (uint16_t)tid;
        if (tid == (uint32_t)kGzEob) S.n_used = (uint32_t)u;
    }
    __syncthreads();
    const int n_used = (int)S.n_used;                   // >= 2: a byte and the end-of-block symbol
    if (tid == 0) huff_merge(S.hist, S.order, n_used, S.node_freq, S.parent);
    __syncthreads();
    if (tid < (uint32_t)n_used) {
        const int d = huff_depth(S.parent, (int)tid, 2 * n_used - 2);
        atomicAdd(&S.count[d < kGzMaxBits ? d : kGzMaxBits], 1u);
    }
    __syncthreads();
    if (tid == 0) { huff_limit(S.count, kGzMaxBits); huff_first_codes(S.count, kGzMaxBits, S.first); }
    __syncthreads();
    if (tid < (uint32_t)n_used) S.lens[S.order[tid]] = (uint8_t)huff_len_of_rank(S.count, (int)tid, kGzMaxBits);
    __syncthreads();
    if (tid < (uint32_t)kGzLitSyms && S.lens[tid]) {
        const int l = S.lens[tid];
        uint32_t code = S.first[l];
        for (uint32_t s = 0; s < tid; ++s) code += S.lens[s] == l;
        S.codes[tid] = (uint16_t)gz_rev_bits(code, l);
    }
    __syncthreads();

    // ---- the header (one lane) and the bits of every slice
    if (tid == 0) S.hdr_bits = gz_write_block_header(S.lens, &S.clw, [&](uint32_t w, uint32_t bits) { S.img[w] |= bits; });
    uint32_t my_bits = 0;
    gz_chunk_tokens(eqw, c0, c0 + kSlice, n, z_in, [&](uint32_t pos, uint32_t l) { my_bits += gz_token_bits(S.lens, byte_at(pos), l); });
    uint32_t incl = my_bits;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t other = __shfl_up(incl, o);
        if ((int)lane >= o) incl += other;
    }
    if (lane == kWave - 1) S.wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = incl - my_bits, body = 0;
    for (uint32_t w = 0; w < (uint32_t)kWaves; ++w) { const uint32_t s = S.wave_sum[w]; if (w < wave) before += s; body += s; }
    const uint32_t hdr = S.hdr_bits;
    const uint32_t coded = gz_coded_bytes(hdr + body + S.lens[kGzEob]), raw = gz_stored_bytes(n);
    const bool use_coded = coded < raw;                 // the same for every lane

    // ---- pack
    if (use_coded) {
        auto or32 = [&](uint32_t w, uint32_t bits) { atomicOr(&S.img[w], bits); };
        uint64_t pos = (uint64_t)hdr + before;
        gz_chunk_tokens(eqw, c0, c0 + kSlice, n, z_in, [&](uint32_t at, uint32_t l) {
            int nb;
            const uint32_t c = gz_token_code(S.lens, S.codes, byte_at(at), l, &nb);
            gz_put_bits(or32, pos, c, nb);
            pos += (uint32_t)nb;
        });
        if (tid == 0) {
            gz_put_bits(or32, (uint64_t)hdr + body, S.codes[kGzEob], S.lens[kGzEob]);
            for (uint32_t b = coded - 2u; b < coded; ++b) atomicOr(&S.img[b >> 2], 0xffu << (8u * (b & 3u)));      // NLEN of the empty stored block
        }
    } else {
        uint8_t* img8 = reinterpret_cast<uint8_t*>(S.img);
        if (tid == 0) for (uint32_t at = 0; at < n; at += kGzStoredMax) gz_stored_header(at, n, [&](uint32_t o, uint8_t b) { img8[o] = b; });
        for (uint32_t j = 0; j < len; ++j) img8[gz_stored_pos(c0 + j)] = (uint8_t)byte_at(c0 + j);
    }
    __syncthreads();

    // ---- store
    const uint32_t out_len = use_coded ? coded : raw;
    uint4* slot = slots + (uint64_t)blockIdx.x * (kSlotBytes / 16);
    const uint4* img4 = reinterpret_cast<const uint4*>(S.img);
    for (uint32_t i = tid; i < (out_len + 15u) / 16u; i += kThreads) slot[i] = img4[i];
    if (tid == 0) {
        const uint32_t r = n % kSlice;
        blk_crc[blockIdx.x] = r ? crc32_mulmod(crc32_xpow8(r), S.crc_full) ^ S.crc_part : S.crc_full;
        blk_len[blockIdx.x] = out_len;
        blk_stored[blockIdx.x] = use_coded ? 0u : 1u;
    }
}

// slot b (16-byte aligned, blk_off[b + 1] - blk_off[b] bytes) to out + blk_off[b]: aligned dwords of the destination from two
// aligned dwords of the slot, the ragged ends byte by byte
__global__ void __launch_bounds__(256)
k_gz_compact(const uint8_t* __restrict__ slots, const uint64_t* __restrict__ blk_off, uint8_t* __restrict__ out) {
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

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

struct sfgpu_gz {
    sfgpu_text_sink sink = nullptr;
    void* user = nullptr;
    uint64_t chunk_bytes = 0;
    bool broken = false;                                // a write failed: the stream cannot be continued
    uint32_t crc = 0;
    sfgpu_gz_result res{};
    hipStream_t st = nullptr, cs = nullptr;
    hipEvent_t ev_in = nullptr, ev_e0 = nullptr, ev_e1 = nullptr, ev_c0[2] = {nullptr, nullptr}, ev_c1[2] = {nullptr, nullptr};
    char* pinned[2] = {nullptr, nullptr};
    uint64_t pinned_cap = 0;
    uint32_t* h_meta = nullptr;                         // crc[kBatchBlocks], stored[kBatchBlocks] of the batch just encoded
    uint64_t* h_total = nullptr;
    DevBuf<uint4> slots;
    DevBuf<uint32_t> blk_len, blk_meta;
    DevBuf<uint64_t> blk_off;
    DevBuf<uint8_t> out[2];
    CallScope scope;                                    // streams, events, h_meta, h_total; last, so that it drains before the DevBufs go
    ~sfgpu_gz() {
        scope.drain();
        for (char* p : pinned) if (p) pinned_free(p);   // the staging buffers grow between writes: not the scope's
    }
};

namespace {

int gz_sink(sfgpu_gz* z, const char* bytes, uint64_t n, const char* who) {
    const auto t0 = std::chrono::steady_clock::now();
    const int stop = z->sink(bytes, n, z->user);
    z->res.sink_ms += ms_since(t0);
    z->res.n_chunks++;
    if (stop) {
        z->broken = true;
        set_error("%s: the sink refused a chunk", who);
        return SFGPU_ERR_IO;
    }
    z->res.n_bytes_out += n;
    return SFGPU_OK;
}

int gz_open_impl(sfgpu_gz* z) {
    SF_HIP(z->scope.acquire(&z->st));
    SF_HIP(z->scope.acquire(&z->cs));
    SF_HIP(z->scope.event(&z->ev_in, hipEventDisableTiming));
    for (hipEvent_t* e : {&z->ev_e0, &z->ev_e1, &z->ev_c0[0], &z->ev_c1[0], &z->ev_c0[1], &z->ev_c1[1]}) SF_HIP(z->scope.event(e));
    SF_HIP(z->scope.pinned_block(&z->h_meta, 2 * kBatchBlocks * sizeof(uint32_t)));
    SF_HIP(z->scope.pinned_block(&z->h_total, sizeof(uint64_t)));
    uint8_t head[kGzHeaderBytes];
    gz_header(head);
    return gz_sink(z, reinterpret_cast<const char*>(head), kGzHeaderBytes, "sfgpu_gz_open");
}

int gz_write_impl(sfgpu_gz* z, const uint8_t* d_src, uint64_t n_bytes, sfgpu_stream stream) {
    hipStream_t st = z->st, cs = z->cs;
    SF_HIP(hipEventRecord(z->ev_in, as_stream(stream)));       // behind whatever the caller has queued on `stream`
    SF_HIP(hipStreamWaitEvent(st, z->ev_in, 0));
    const uint64_t n_blocks = (n_bytes + kGzBlockBytes - 1) / kGzBlockBytes;
    const uint64_t n_batches = (n_blocks + kBatchBlocks - 1) / kBatchBlocks;
    const uint64_t max_nb = n_blocks < kBatchBlocks ? n_blocks : kBatchBlocks;
    // staging: as large as a piece of this write can get, at most chunk_bytes (nothing is in flight between writes)
    const uint64_t stage = z->chunk_bytes < max_nb * kSlotBytes ? z->chunk_bytes : max_nb * kSlotBytes;
    if (stage > z->pinned_cap) {
        for (int b = 0; b < 2; ++b) {
            if (z->pinned[b]) { pinned_free(z->pinned[b]); z->pinned[b] = nullptr; }
            z->pinned_cap = 0;
            SF_HIP(pinned_malloc(&z->pinned[b], stage));
        }
        z->pinned_cap = stage;
    }
    if (int rc = z->slots.reserve(max_nb * (kSlotBytes / 16), st, false)) return rc;
    if (int rc = z->blk_len.reserve(max_nb + 1, st, false)) return rc;
    if (int rc = z->blk_off.reserve(max_nb + 1, st, false)) return rc;
    if (int rc = z->blk_meta.reserve(2 * kBatchBlocks, st, false)) return rc;
    for (int b = 0; b < 2 && (uint64_t)b < n_batches; ++b) if (int rc = z->out[b].reserve(max_nb * kSlotBytes, st, false)) return rc;

    auto batch_blocks = [&](uint64_t i) -> uint32_t {
        return (uint32_t)(n_blocks - i * kBatchBlocks < kBatchBlocks ? n_blocks - i * kBatchBlocks : kBatchBlocks);
    };
    // encode + scan + compact of batch i on st into out[i & 1]; every copy that read this buffer has been waited for, and the
    // sizes of the batch before have been read
    auto enqueue = [&](uint64_t i) -> int {
        const uint32_t nb = batch_blocks(i);
        const uint64_t b0 = i * kBatchBlocks * (uint64_t)kGzBlockBytes;
        const uint64_t bytes = n_bytes - b0 < (uint64_t)nb * kGzBlockBytes ? n_bytes - b0 : (uint64_t)nb * kGzBlockBytes;
        uint32_t* d_crc = z->blk_meta.p;
        uint32_t* d_stored = d_crc + kBatchBlocks;
        SF_HIP(hipEventRecord(z->ev_e0, st));
        hipLaunchKernelGGL(k_gz_encode, dim3(nb), dim3(kThreads), 0, st, d_src + b0, bytes, z->slots.p, z->blk_len.p, d_crc, d_stored);
        SF_HIP(hipGetLastError());
        if (int rc = exclusive_scan_u32(z->blk_len.p, z->blk_off.p, nb, st, false)) return rc;
        hipLaunchKernelGGL(k_gz_compact, dim3(nb), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(z->slots.p), z->blk_off.p, z->out[i & 1].p);
        SF_HIP(hipGetLastError());
        SF_HIP(hipEventRecord(z->ev_e1, st));
        SF_HIP(hipMemcpyAsync(z->h_total, z->blk_off.p + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(z->h_meta, d_crc, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(z->h_meta + kBatchBlocks, d_stored, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        return SFGPU_OK;
    };
    const uint32_t x_block = crc32_xpow8(kGzBlockBytes);
    int pb = 0;                                         // pinned buffer of the next piece
    auto copy_piece = [&](int p, const uint8_t* d, uint64_t len) -> int {
        SF_HIP(hipEventRecord(z->ev_c0[p], cs));
        SF_HIP(hipMemcpyAsync(z->pinned[p], d, len, hipMemcpyDeviceToHost, cs));
        SF_HIP(hipEventRecord(z->ev_c1[p], cs));
        return SFGPU_OK;
    };
    if (int rc = enqueue(0)) return rc;
    for (uint64_t i = 0; i < n_batches; ++i) {
        const uint32_t nb = batch_blocks(i);
        SF_HIP(hipStreamSynchronize(st));               // batch i is encoded, its sizes and CRCs are here
        add_elapsed(&z->res.encode_ms, z->ev_e0, z->ev_e1);
        const uint64_t total = *z->h_total;
        for (uint32_t b = 0; b < nb; ++b) {
            const uint64_t at = (i * kBatchBlocks + b) * (uint64_t)kGzBlockBytes;
            const uint64_t blen = n_bytes - at < kGzBlockBytes ? n_bytes - at : kGzBlockBytes;
            z->crc = crc32_mulmod(blen == kGzBlockBytes ? x_block : crc32_xpow8(blen), z->crc) ^ z->h_meta[b];
            z->res.n_stored_blocks += z->h_meta[kBatchBlocks + b];
        }
        z->res.n_blocks += nb;
        if (i + 1 < n_batches) if (int rc = enqueue(i + 1)) return rc;
        const uint8_t* d_out = z->out[i & 1].p;
        const uint64_t chunk = z->pinned_cap < z->chunk_bytes ? z->pinned_cap : z->chunk_bytes;
        if (int rc = copy_piece(pb, d_out, total < chunk ? total : chunk)) return rc;
        for (uint64_t off = 0; off < total;) {
            const uint64_t len = total - off < chunk ? total - off : chunk, next = off + len;
            if (next < total) if (int rc = copy_piece(pb ^ 1, d_out + next, total - next < chunk ? total - next : chunk)) return rc;
            SF_HIP(hipEventSynchronize(z->ev_c1[pb]));
            add_elapsed(&z->res.d2h_ms, z->ev_c0[pb], z->ev_c1[pb]);
            if (int rc = gz_sink(z, z->pinned[pb], len, "sfgpu_gz_write_device")) return rc;
            off = next; pb ^= 1;
        }
    }
    z->res.n_bytes_in += n_bytes;
    return SFGPU_OK;
}

}  // namespace

extern "C" int sfgpu_gz_open(sfgpu_gz** out, sfgpu_text_sink sink, void* user, uint64_t chunk_bytes) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_gz_open: null handle pointer");
    *out = nullptr;
    SF_REQUIRE(sink, SFGPU_ERR_INVALID, "sfgpu_gz_open: null sink");
    if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
    SF_REQUIRE(chunk_bytes >= 16 && chunk_bytes <= kMaxChunk, SFGPU_ERR_INVALID, "sfgpu_gz_open: chunk_bytes must lie in [16, 2^30] (0 = default)");
    sfgpu_gz* z = new (std::nothrow) sfgpu_gz;
    SF_REQUIRE(z, SFGPU_ERR_HIP, "sfgpu_gz_open: out of host memory");
    z->sink = sink; z->user = user; z->chunk_bytes = chunk_bytes;
    const int rc = gz_open_impl(z);
    if (rc != SFGPU_OK) { delete z; return rc; }
    *out = z;
    return SFGPU_OK;
}

extern "C" int sfgpu_gz_write_device(sfgpu_gz* z, const void* d_src, uint64_t n_bytes, sfgpu_stream stream) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_gz_write_device: null handle");
    SF_REQUIRE(!z->broken, SFGPU_ERR_STATE, "sfgpu_gz_write_device: an earlier write failed; close the stream");
    if (n_bytes == 0) return SFGPU_OK;
    SF_REQUIRE(d_src, SFGPU_ERR_INVALID, "sfgpu_gz_write_device: null source");
    const int rc = gz_write_impl(z, static_cast<const uint8_t*>(d_src), n_bytes, stream);
    if (rc != SFGPU_OK) {
        z->broken = true;                               // nothing may stay in flight behind a failed write
        z->scope.drain();
    }
    return rc;
}

extern "C" int sfgpu_gz_close(sfgpu_gz* z, sfgpu_gz_result* res) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_gz_close: null handle");
    int rc = SFGPU_OK;
    if (!z->broken) {
        uint8_t tail[kGzFinalBlockBytes + kGzTrailerBytes];
        gz_trailer(z->crc, z->res.n_bytes_in, tail);
        rc = gz_sink(z, reinterpret_cast<const char*>(tail), sizeof(tail), "sfgpu_gz_close");
    }
    if (res) *res = z->res;
    delete z;
    return rc;
}
