// gzwrite.hip -- aux/bootstrap/bootstraps.gz written from the device (GZipWriter::writeBootstrap<T>, src/GZipWriter.cpp:249-285:
// every sample appended as raw little-endian binary to one gzip stream): sfgpu_gz_open / sfgpu_gz_write_device / sfgpu_gz_close.
//
// The arithmetic is gzfmt.h, which the CPU tests drive serially.  A write is cut into independent blocks of 64 KB, one workgroup
// of 1024 lanes each (k_gz_encode); lane l owns the 64-byte slice l.  The stages that do not depend on the parse are
// deflate_wg.h's, the host driver is slotpipe.h's, both shared with bgzf_write.hip.  This kernel's own:
//   mask    bit i = "byte i equals byte i - 1", one 64-bit word per lane, the slice's CRC-32 by table in the same pass; a max-scan
//           gives every lane the last clear bit before it
//   parse   gz_chunk_tokens: the greedy tokens that start in the slice, found from the mask alone; histogram in LDS
//   pack    the header by one lane; the codes ORed into the LDS image at the scanned bit offsets (OR commutes); a block that
//           would not be shorter than its stored form is laid out stored, with a 5-byte header every 65 535 bytes
// LDS: 69 632 B input + 65 568 B image + 8 KB mask + ~8 KB tables = 152 KB of the CU's 160 KB: one workgroup per CU.
// The host side adds the stream's running CRC-32 from the per-block CRCs, the stored flags, and the gzip header and trailer.
#include "common.h"
#include "deflate_wg.h"
#include "gzfmt.h"
#include "slotpipe.h"

#include <memory>
#include <new>

namespace sfgpu {
namespace {

constexpr int kThreads = 1024;                          // = kGzBlockBytes / kSlice
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kSlice = kWgSlice;
constexpr uint32_t kImgWords = 16392;                   // gz_stored_bytes(65536) = 65546 -> 16-byte groups, + room for the second word of an OR
constexpr uint32_t kSlotBytes = kImgWords * 4;
constexpr uint32_t kBatchBlocks = 1024;                 // 64 MiB of payload per launch
static_assert(kThreads * kSlice == kGzBlockBytes, "one lane per slice");
static_assert(kSlotBytes % 16 == 0 && kSlotBytes >= 65546 + 8, "a slot holds the stored form");

struct alignas(16) EncodeLds {
    uint32_t img[kImgWords];
    uint32_t in[kThreads * kInStride];
    uint64_t eq[kThreads + 8];
    CrcLds crc;
    LitCodeLds lit;
    uint32_t wave_sum[kWaves];
    int32_t wave_z[kWaves];
    uint32_t hdr_bits;
    GzClWork clw;
};
static_assert(sizeof(EncodeLds) == 151296, "one workgroup per CU; the struct does not grow");

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
    if (tid < 8) S.eq[kThreads + tid] = 0ull;
    wg_init(S.crc, S.lit, tid);
    wg_stage_input<kThreads>(S.in, in, n, tid);
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
                    crc = S.crc.table[(crc ^ byte) & 0xffu] ^ (crc >> 8);
                }
                prev = byte;
            }
        }
        crc = ~crc;
    }
    S.eq[tid] = mask;
    wg_crc_fold<kThreads>(S.crc, crc, tid, lane, n, len);
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
        atomicAdd(&S.lit.hist[gz_token_symbol(byte_at(pos), l)], 1u);
    });
    if (tid == 0) atomicAdd(&S.lit.hist[kGzEob], 1u);
    __syncthreads();

    // ---- code lengths and codes of the literal/length alphabet (>= 2 used symbols: a byte and the end-of-block symbol)
    wg_lit_code_build(S.lit, tid, [] {});

    // ---- the header (one lane) and the bits of every slice
    if (tid == 0) S.hdr_bits = gz_write_block_header(S.lit.lens, &S.clw, [&](uint32_t w, uint32_t bits) { S.img[w] |= bits; });
    uint32_t my_bits = 0;
    gz_chunk_tokens(eqw, c0, c0 + kSlice, n, z_in, [&](uint32_t pos, uint32_t l) { my_bits += gz_token_bits(S.lit.lens, byte_at(pos), l); });
    const auto [before, body] = wg_scan_bits<kThreads>(S.wave_sum, my_bits, lane, wave);
    const uint32_t hdr = S.hdr_bits;
    const uint32_t coded = gz_coded_bytes(hdr + body + S.lit.lens[kGzEob]), raw = gz_stored_bytes(n);
    const bool use_coded = coded < raw;                 // the same for every lane

    // ---- pack
    if (use_coded) {
        auto or32 = [&](uint32_t w, uint32_t bits) { atomicOr(&S.img[w], bits); };
        uint64_t pos = (uint64_t)hdr + before;
        gz_chunk_tokens(eqw, c0, c0 + kSlice, n, z_in, [&](uint32_t at, uint32_t l) {
            int nb;
            const uint32_t c = gz_token_code(S.lit.lens, S.lit.codes, byte_at(at), l, &nb);
            gz_put_bits(or32, pos, c, nb);
            pos += (uint32_t)nb;
        });
        if (tid == 0) {
            gz_put_bits(or32, (uint64_t)hdr + body, S.lit.codes[kGzEob], S.lit.lens[kGzEob]);
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
    wg_store_image<kThreads>(S.img, out_len, slots + (uint64_t)blockIdx.x * (kSlotBytes / 16), tid);
    if (tid == 0) {
        blk_crc[blockIdx.x] = wg_crc_member(S.crc, n);
        blk_len[blockIdx.x] = out_len;
        blk_stored[blockIdx.x] = use_coded ? 0u : 1u;
    }
}

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

struct sfgpu_gz {
    uint32_t crc = 0;                                   // of the payload so far
    sfgpu_gz_result res{};                              // n_blocks, n_stored_blocks
    uint32_t* h_meta = nullptr;                         // crc[kBatchBlocks], stored[kBatchBlocks] of the batch just encoded; the pipe's scope owns it
    DevBuf<uint32_t> blk_meta;                          // the same on the device
    SlotPipe pipe;                                      // last, so that it drains before blk_meta goes
};

extern "C" int sfgpu_gz_open(sfgpu_gz** out, sfgpu_text_sink sink, void* user, uint64_t chunk_bytes) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_gz_open: null handle pointer");
    *out = nullptr;
    std::unique_ptr<sfgpu_gz> z(new (std::nothrow) sfgpu_gz);
    SF_REQUIRE(z, SFGPU_ERR_HIP, "sfgpu_gz_open: out of host memory");
    if (int rc = z->pipe.open("sfgpu_gz_open", sink, user, chunk_bytes)) return rc;
    SF_HIP(z->pipe.scope.pinned_block(&z->h_meta, 2 * kBatchBlocks * sizeof(uint32_t)));
    if (int rc = z->blk_meta.reserve(2 * kBatchBlocks, z->pipe.st, false)) return rc;
    uint8_t head[kGzHeaderBytes];
    gz_header(head);
    if (int rc = z->pipe.sink(reinterpret_cast<const char*>(head), kGzHeaderBytes, "sfgpu_gz_open")) return rc;
    *out = z.release();
    return SFGPU_OK;
}

extern "C" int sfgpu_gz_write_device(sfgpu_gz* z, const void* d_src, uint64_t n_bytes, sfgpu_stream stream) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_gz_write_device: null handle");
    SF_REQUIRE(!z->pipe.broken, SFGPU_ERR_STATE, "sfgpu_gz_write_device: an earlier write failed; close the stream");
    if (n_bytes == 0) return SFGPU_OK;
    SF_REQUIRE(d_src, SFGPU_ERR_INVALID, "sfgpu_gz_write_device: null source");
    hipStream_t st = z->pipe.st;
    uint32_t* d_crc = z->blk_meta.p;
    uint32_t* d_stored = d_crc + kBatchBlocks;
    const uint32_t x_block = crc32_xpow8(kGzBlockBytes);
    return z->pipe.write<kGzBlockBytes, kSlotBytes, kBatchBlocks>(
        static_cast<const uint8_t*>(d_src), n_bytes, stream, "sfgpu_gz_write_device",
        [&](const uint8_t* src, uint64_t bytes, uint32_t nb, uint4* slots, uint32_t* blk_len) {
            hipLaunchKernelGGL(k_gz_encode, dim3(nb), dim3(kThreads), 0, st, src, bytes, slots, blk_len, d_crc, d_stored);
        },
        [&](uint32_t nb) -> int {
            SF_HIP(hipMemcpyAsync(z->h_meta, d_crc, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            SF_HIP(hipMemcpyAsync(z->h_meta + kBatchBlocks, d_stored, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            return SFGPU_OK;
        },
        [&](uint64_t first, uint32_t nb) {              // the stream's CRC from the blocks' CRCs
            for (uint32_t b = 0; b < nb; ++b) {
                const uint64_t at = (first + b) * (uint64_t)kGzBlockBytes;
                const uint64_t blen = n_bytes - at < kGzBlockBytes ? n_bytes - at : kGzBlockBytes;
                z->crc = crc32_mulmod(blen == kGzBlockBytes ? x_block : crc32_xpow8(blen), z->crc) ^ z->h_meta[b];
                z->res.n_stored_blocks += z->h_meta[kBatchBlocks + b];
            }
            z->res.n_blocks += nb;
        });
}

extern "C" int sfgpu_gz_close(sfgpu_gz* z, sfgpu_gz_result* res) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_gz_close: null handle");
    uint8_t tail[kGzFinalBlockBytes + kGzTrailerBytes];
    gz_trailer(z->crc, z->pipe.n_bytes_in, tail);
    const int rc = z->pipe.broken ? SFGPU_OK : z->pipe.sink(reinterpret_cast<const char*>(tail), sizeof(tail), "sfgpu_gz_close");
    if (res) z->pipe.report(res, z->res);
    delete z;
    return rc;
}
