// bgzf_write.hip -- blocked gzip (BGZF: what samtools, IGV and htslib read, and the container of BAM) written from device memory:
// sfgpu_bgzw_open / sfgpu_bgzw_write_device / sfgpu_bgzw_close.  The DEFLATE blocks carry real (length, distance) matches.
//
// What a member says is bgzwfmt.h, which the CPU tests drive serially.  A write is cut into members of 32 KB of payload, one
// workgroup of 512 lanes each (k_bgzw_encode); lane l owns the 64-byte slice l.  The stages that do not depend on the parse are
// deflate_wg.h's, the host driver is slotpipe.h's, both shared with gzwrite.hip.  This kernel's own:
//   candidates  128 steps of 256 positions: a lane hashes the four bytes at its position, reads the table (the greatest position
//               of the steps before, per bucket) into the position's token slot, and after a barrier enters its own position with
//               atomicMax, which commutes: the table after a step does not depend on the order of the lanes
//   parse       CRC-32 of the slice by table, then bgzw_slice_tokens (distance 1, the slice's previous distance and the candidate,
//               extended byte by byte from LDS to the slice's end at most), which leaves the tokens where the candidates were
//               (length at the token's first position, distance - 1 at its second) and counts the two histograms in LDS
//   codes       the distance code (30 symbols) by lane 64, while lane 0 of another wavefront merges the literal/length code
//   pack        the block header by one lane behind the 18 header bytes; the codes ORed into the LDS image at the scanned bit
//               offsets; a member not shorter than its stored form is laid out stored.  Then the BGZF header, BSIZE and trailer
// No workgroup waits for another one; every loop is bounded (a match extension by the slice, the candidates by three).
// LDS: 34 880 B input + 67 584 B candidates / tokens + 32 816 B image (the candidate table lives in the same bytes: it is dead
// when the first bit is packed) + ~9 KB tables = 141 KB of the CU's 160 KB: one workgroup per CU (DESIGN 4.22 weighs a 16 KB member).
// The host side adds the three counters the kernel sums and the EOF member.
#include "common.h"
#include "bgzwfmt.h"
#include "deflate_wg.h"
#include "slotpipe.h"

#include <memory>
#include <new>

namespace sfgpu {
namespace {

constexpr int kThreads = kBgzwPayload / kBgzwSlice;     // 512: one lane per slice
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kInWords = kThreads * kInStride + 16;        // the four bytes at the last positions reach into the next dword
constexpr uint32_t kTokStride = 66;                     // 16-bit slots per slice: 33 dwords, so that lanes walking their slices hit different banks
constexpr uint32_t kTableWords = 1u << kBgzwHashBits;
constexpr uint32_t kImgWords = 8204;                    // kBgzwMaxMember = 32 799 -> 2050 16-byte groups, + room for the second word of an OR
constexpr uint32_t kSlotBytes = kImgWords * 4;
constexpr uint32_t kBatchMembers = 2048;                // 64 MiB of payload per launch
constexpr uint64_t kBitPos0 = 8ull * kBgzwHeaderBytes;  // the DEFLATE stream begins behind the 18 header bytes
static_assert(kThreads <= 1024 && kThreads % kWave == 0 && (uint32_t)kThreads >= kBgzwStep, "one lane per position of a step");
static_assert(kBgzwSlice == kWgSlice, "the parse restarts where deflate_wg.h cuts the lanes' slices");
static_assert(kSlotBytes % 16 == 0 && kSlotBytes >= kBgzwMaxMember + 8 && kImgWords >= kTableWords, "a slot holds the stored form; the image holds the table");

struct alignas(16) EncodeLds {
    uint32_t img[kImgWords];                            // first the candidate table, then the member's bytes
    uint32_t in[kInWords];
    uint16_t tok[kThreads * kTokStride];                // candidate position + 1 of every position, then the tokens
    CrcLds crc;
    LitCodeLds lit;
    uint32_t dhist[32], dnode_freq[2 * kBgzwDistSyms], dcount[kGzMaxBits + 1];
    uint32_t wave_sum[kWaves];
    uint32_t hdr_bits, n_matches, n_literals;
    uint16_t dorder[32], dparent[2 * kBgzwDistSyms], dcodes[32];
    uint8_t dlens[32];
    GzClWork clw;
};
static_assert(sizeof(EncodeLds) == 143744 && sizeof(EncodeLds) <= 150 * 1024, "one workgroup per CU; the struct does not grow");

// stats: members stored, matches, literals (of the coded members), summed over all launches of a handle
__global__ void __launch_bounds__(kThreads)
k_bgzw_encode(const uint8_t* __restrict__ src, uint64_t n_bytes, uint4* __restrict__ slots, uint32_t* __restrict__ mem_len,
              unsigned long long* __restrict__ stats) {
    __shared__ EncodeLds S;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint64_t base = (uint64_t)blockIdx.x * kBgzwPayload;
    const uint32_t n = n_bytes - base < kBgzwPayload ? (uint32_t)(n_bytes - base) : kBgzwPayload;
    const uint8_t* in = src + base;
    auto in_word = [&](uint32_t d) -> uint32_t { return S.in[(d >> 4) * kInStride + (d & 15u)]; };
    auto byte_at = [&](uint32_t i) -> uint32_t { return (in_word(i >> 2) >> (8u * (i & 3u))) & 0xffu; };
    auto tok_at = [&](uint32_t i) -> uint16_t& { return S.tok[(i >> 6) * kTokStride + (i & 63u)]; };

    // ---- load
    for (uint32_t i = tid; i < kTableWords; i += kThreads) S.img[i] = 0u;
    if (tid < 32) S.dhist[tid] = 0u;
    if (tid < 16) S.in[kThreads * kInStride + tid] = 0u;
    if (tid == 320) { S.n_matches = 0u; S.n_literals = 0u; }
    wg_init(S.crc, S.lit, tid);
    wg_stage_input<kThreads>(S.in, in, n, tid);
    __syncthreads();

    // ---- candidates (bgzw_candidates): look the step's positions up, barrier, enter them
    for (uint32_t s = 0; s < n; s += kBgzwStep) {
        const uint32_t i = s + tid;
        const bool in_step = tid < kBgzwStep && i < n, hashed = in_step && i + 4u <= n;
        uint32_t h = 0;
        if (hashed) {
            const uint32_t sh = 8u * (i & 3u), lo = in_word(i >> 2);
            h = bgzw_hash(sh ? (lo >> sh) | (in_word((i >> 2) + 1u) << (32u - sh)) : lo);
        }
        if (in_step) tok_at(i) = hashed ? (uint16_t)S.img[h] : (uint16_t)0;
        __syncthreads();
        if (hashed) atomicMax(&S.img[h], i + 1u);
        __syncthreads();
    }
    for (uint32_t i = tid; i < kImgWords; i += kThreads) S.img[i] = 0u;        // the table is dead: the image begins empty

    // ---- CRC of the slice, parse of the slice
    const uint32_t c0 = tid * kBgzwSlice;
    const uint32_t len = c0 < n ? (n - c0 < kBgzwSlice ? n - c0 : kBgzwSlice) : 0u;
    const uint32_t c1 = c0 + len;
    {
        uint32_t crc = 0xffffffffu;
        for (uint32_t j = 0; j < len; ++j) crc = S.crc.table[(crc ^ byte_at(c0 + j)) & 0xffu] ^ (crc >> 8);
        wg_crc_fold<kThreads>(S.crc, ~crc, tid, lane, n, len);
    }
    {
        uint32_t n_m = 0, n_l = 0;
        bgzw_slice_tokens(byte_at, [&](uint32_t i) -> uint32_t { return tok_at(i); }, c0, c1, [&](uint32_t pos, uint32_t l, uint32_t dist) {
            tok_at(pos) = (uint16_t)l;
            atomicAdd(&S.lit.hist[gz_token_symbol(byte_at(pos), l)], 1u);
            if (l > 1u) {
                int eb; uint32_t ev;
                tok_at(pos + 1u) = (uint16_t)(dist - 1u);
                atomicAdd(&S.dhist[bgzw_dist_symbol(dist, &eb, &ev)], 1u);
                ++n_m;
            } else {
                ++n_l;
            }
        });
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) { n_m += __shfl_xor(n_m, o); n_l += __shfl_xor(n_l, o); }
        if (lane == 0) { atomicAdd(&S.n_matches, n_m); atomicAdd(&S.n_literals, n_l); }
    }
    if (tid == 0) atomicAdd(&S.lit.hist[kGzEob], 1u);
    __syncthreads();
    // the tokens of the slice again: f(position, length, distance)
    auto tokens = [&](auto f) {
        for (uint32_t i = c0; i < c1;) {
            const uint32_t l = tok_at(i);
            f(i, l, l > 1u ? (uint32_t)tok_at(i + 1u) + 1u : 0u);
            i += l;
        }
    };

    // ---- the two codes (>= 2 literal/length symbols: the member's first byte is a literal, and the end-of-block symbol); the
    // distance code serially (huff_lengths_serial) by lane 64 while lane 0 merges
    wg_lit_code_build(S.lit, tid, [&] {
        if (tid == 64) {
            huff_lengths_serial(S.dhist, kBgzwDistSyms, kGzMaxBits, S.dlens, S.dorder, S.dparent, S.dnode_freq, S.dcount);
            for (int s = 0; s < kBgzwDistSyms; ++s) S.dcodes[s] = (uint16_t)huff_code_rev(S.dlens, kBgzwDistSyms, s);
        }
    });

    // ---- the block header (one lane) and the bits of every slice
    if (tid == 0) S.hdr_bits = bgzw_write_block_header(S.lit.lens, S.dlens, &S.clw, kBitPos0, [&](uint32_t w, uint32_t bits) { S.img[w] |= bits; });
    uint32_t my_bits = 0;
    tokens([&](uint32_t pos, uint32_t l, uint32_t dist) { my_bits += bgzw_token_bits(S.lit.lens, S.dlens, byte_at(pos), l, dist); });
    const auto [before, body] = wg_scan_bits<kThreads>(S.wave_sum, my_bits, lane, wave);
    const uint32_t hdr = S.hdr_bits;
    const uint32_t coded = bgzw_coded_bytes(hdr + body + S.lit.lens[kGzEob]), raw = bgzw_stored_bytes(n);
    const bool use_coded = coded < raw;                 // the same for every lane
    const uint32_t out_len = use_coded ? coded : raw;
    uint8_t* img8 = reinterpret_cast<uint8_t*>(S.img);

    // ---- pack
    if (use_coded) {
        auto or32 = [&](uint32_t w, uint32_t bits) { atomicOr(&S.img[w], bits); };
        uint64_t pos = kBitPos0 + hdr + before;
        tokens([&](uint32_t at, uint32_t l, uint32_t dist) {
            pos += bgzw_put_token(or32, pos, S.lit.lens, S.lit.codes, S.dlens, S.dcodes, byte_at(at), l, dist);
        });
        if (tid == 0) gz_put_bits(or32, kBitPos0 + hdr + body, S.lit.codes[kGzEob], S.lit.lens[kGzEob]);
    } else {
        for (uint32_t i = tid; i < kImgWords; i += kThreads) S.img[i] = 0u;    // the block header that lane 0 wrote
        __syncthreads();
        for (uint32_t j = 0; j < len; ++j) img8[kBgzwHeaderBytes + 5u + c0 + j] = (uint8_t)byte_at(c0 + j);
    }
    __syncthreads();
    if (tid == 0) {                                     // every bit is in place: plain byte stores
        bgzw_member_header(out_len, img8);
        if (!use_coded) bgzw_stored_header(n, img8 + kBgzwHeaderBytes);
        bgzw_member_trailer(wg_crc_member(S.crc, n), n, img8 + out_len - kBgzwTrailerBytes);
    }
    __syncthreads();

    // ---- store
    wg_store_image<kThreads>(S.img, out_len, slots + (uint64_t)blockIdx.x * (kSlotBytes / 16), tid);
    if (tid == 0) {
        mem_len[blockIdx.x] = out_len;
        if (use_coded) { atomicAdd(&stats[1], (unsigned long long)S.n_matches); atomicAdd(&stats[2], (unsigned long long)S.n_literals); }
        else atomicAdd(&stats[0], 1ull);
    }
}

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

struct sfgpu_bgzw {
    sfgpu_bgzw_result stats{};                          // n_members, and the three counters as last copied
    uint64_t* h_stats = nullptr;                        // stored members, matches, literals so far; the pipe's scope owns it
    DevBuf<unsigned long long> d_stats;                 // the same on the device, summed by the kernel over all launches
    bool track = false;                                 // sfgpu_bgzw_track_members: every batch's mem_len is kept in d_sizes
    DevBuf<uint32_t> d_sizes;                           // compressed bytes of the members written since, in file order
    uint64_t n_sizes = 0;
    SlotPipe pipe;                                      // last, so that it drains before d_stats goes
};

extern "C" int sfgpu_bgzw_open(sfgpu_bgzw** out, sfgpu_text_sink sink, void* user, uint64_t chunk_bytes) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_bgzw_open: null handle pointer");
    *out = nullptr;
    std::unique_ptr<sfgpu_bgzw> z(new (std::nothrow) sfgpu_bgzw);
    SF_REQUIRE(z, SFGPU_ERR_HIP, "sfgpu_bgzw_open: out of host memory");
    if (int rc = z->pipe.open("sfgpu_bgzw_open", sink, user, chunk_bytes)) return rc;
    SF_HIP(z->pipe.scope.pinned_block(&z->h_stats, 3 * sizeof(uint64_t)));
    if (int rc = z->d_stats.reserve(3, z->pipe.st, false)) return rc;
    SF_HIP(hipMemsetAsync(z->d_stats.p, 0, 3 * sizeof(unsigned long long), z->pipe.st));
    SF_HIP(hipStreamSynchronize(z->pipe.st));
    *out = z.release();
    return SFGPU_OK;
}

extern "C" int sfgpu_bgzw_write_device(sfgpu_bgzw* z, const void* d_src, uint64_t n_bytes, sfgpu_stream stream) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_bgzw_write_device: null handle");
    SF_REQUIRE(!z->pipe.broken, SFGPU_ERR_STATE, "sfgpu_bgzw_write_device: an earlier write failed; close the file");
    if (n_bytes == 0) return SFGPU_OK;
    SF_REQUIRE(d_src, SFGPU_ERR_INVALID, "sfgpu_bgzw_write_device: null source");
    hipStream_t st = z->pipe.st;
    return z->pipe.write<kBgzwPayload, kSlotBytes, kBatchMembers>(
        static_cast<const uint8_t*>(d_src), n_bytes, stream, "sfgpu_bgzw_write_device",
        [&](const uint8_t* src, uint64_t bytes, uint32_t nm, uint4* slots, uint32_t* mem_len) {
            hipLaunchKernelGGL(k_bgzw_encode, dim3(nm), dim3(kThreads), 0, st, src, bytes, slots, mem_len, z->d_stats.p);
        },
        [&](uint32_t nm) -> int {
            SF_HIP(hipMemcpyAsync(z->h_stats, z->d_stats.p, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            if (z->track) {                             // behind the batch on st: the sizes stay on the device
                if (int rc = z->d_sizes.reserve(z->n_sizes + nm, st, true, z->n_sizes)) return rc;
                SF_HIP(hipMemcpyAsync(z->d_sizes.p + z->n_sizes, z->pipe.len.p, nm * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
                z->n_sizes += nm;
            }
            return SFGPU_OK;
        },
        [&](uint64_t, uint32_t nm) {
            z->stats.n_stored_members = z->h_stats[0]; z->stats.n_matches = z->h_stats[1]; z->stats.n_literals = z->h_stats[2];
            z->stats.n_members += nm;
        });
}

extern "C" int sfgpu_bgzw_track_members(sfgpu_bgzw* z) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_bgzw_track_members: null handle");
    z->track = true;
    return SFGPU_OK;
}

extern "C" int sfgpu_bgzw_member_sizes(sfgpu_bgzw* z, const uint32_t** d_sizes, uint64_t* n_members) {
    SF_REQUIRE(z && d_sizes && n_members, SFGPU_ERR_INVALID, "sfgpu_bgzw_member_sizes: null argument");
    SF_REQUIRE(z->track, SFGPU_ERR_STATE, "sfgpu_bgzw_member_sizes: the handle does not track its members");
    *d_sizes = z->d_sizes.p; *n_members = z->n_sizes;
    return SFGPU_OK;
}

extern "C" int sfgpu_bgzw_close(sfgpu_bgzw* z, sfgpu_bgzw_result* res) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_bgzw_close: null handle");
    uint8_t tail[kBgzwEofBytes];
    bgzw_eof_member(tail);
    const int rc = z->pipe.broken ? SFGPU_OK : z->pipe.sink(reinterpret_cast<const char*>(tail), sizeof(tail), "sfgpu_bgzw_close");
    if (res) z->pipe.report(res, z->stats);
    delete z;
    return rc;
}
