// bgzf_write.hip -- blocked gzip (BGZF: what samtools, IGV and htslib read, and the container of BAM) written from device memory:
// sfgpu_bgzw_open / sfgpu_bgzw_write_device / sfgpu_bgzw_close.  The DEFLATE blocks carry real (length, distance) matches.
//
// What a member says (layout, the parse, the two codes, the header) is bgzwfmt.h, which the CPU tests drive serially; this file
// is the parallel driver.  A write is cut into members of 32 KB of payload, one workgroup of 512 lanes each (k_bgzw_encode):
//   load        the member into LDS, 17 dwords per 64-byte slice; the candidate table is cleared
//   candidates  128 steps of 256 positions: a lane hashes the four bytes at its position, reads the table (the greatest position
//               of the steps before, per bucket) into the position's token slot, and after a barrier enters its own position with
//               atomicMax, which commutes: the table after a step does not depend on the order of the lanes
//   parse       lane l owns slice l: CRC-32 of the slice by table (weighted by x^(8 x bytes behind it), XOR-reduced over the
//               member), then bgzw_slice_tokens -- distance 1, the slice's previous distance and the candidate are verified and
//               extended byte by byte from LDS, at most to the slice's end -- which leaves the tokens where the candidates were
//               (length at the token's first position, distance - 1 at its second) and counts the two histograms in LDS
//   codes       literal/length code as in gzwrite.hip (rank per symbol, two-queue merge by one lane, depth per leaf, Kraft repair,
//               lengths by rank, canonical codes per symbol); the distance code (30 symbols) by one lane of another wavefront
//               at the same time
//   header      the code lengths of both codes in run-length form and their 7-bit code, by one lane, behind the 18 header bytes
//   pack        bits per slice, a block scan for the bit offsets, the codes ORed into the LDS image (OR commutes); a member that
//               would not be shorter than its stored form is laid out stored.  Then the BGZF header with BSIZE and the trailer
//   store       the image to the member's slot, 16 bytes per lane
// k_slot_compact (slotcompact.h) moves the slots to their scanned byte offsets.  No workgroup waits for another one; every loop is
// bounded (a match extension by the slice, 64 bytes; the candidates by three).
// LDS: 34 880 B input + 67 584 B candidates / tokens + 32 816 B image (the candidate table, 32 KB, lives in the same bytes: it is
// dead when the first bit is packed) + ~9 KB tables = 141 KB of the CU's 160 KB: one workgroup = 8 waves per CU, 2 per SIMD.  Two
// workgroups per CU would need a 16 KB member, with half the window and 100-odd header bytes per member.  Whether that costs more
// than the occupancy would return has NOT been measured: it is reasoning from the code (the long phases, candidates and parse,
// are latency chains of LDS reads, which a second workgroup would hide, while the candidate steps keep 256 of the 512 lanes idle).
// The compressed bytes of a batch (<= 2048 members) are copied through two pinned buffers in pieces of <= chunk_bytes and handed
// to the sink; batch b + 1 is encoded, and piece p + 1 copied, while the sink holds piece p.
#include "common.h"
#include "bgzwfmt.h"
#include "primitives.h"
#include "slotcompact.h"

#include <cstring>
#include <new>

namespace sfgpu {
namespace {

constexpr int kThreads = kBgzwPayload / kBgzwSlice;     // 512: one lane per slice
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kInStride = 17;                      // dwords per slice in LDS
constexpr uint32_t kInWords = kThreads * kInStride + 16;        // the four bytes at the last positions reach into the next dword
constexpr uint32_t kTokStride = 66;                     // 16-bit slots per slice: 33 dwords, so that lanes walking their slices hit different banks
constexpr uint32_t kTableWords = 1u << kBgzwHashBits;
constexpr uint32_t kImgWords = 8204;                    // kBgzwMaxMember = 32 799 -> 2050 16-byte groups, + room for the second word of an OR
constexpr uint32_t kSlotBytes = kImgWords * 4;
constexpr uint32_t kBatchMembers = 2048;                // 64 MiB of payload per launch
constexpr uint64_t kDefaultChunk = 32ull << 20;
constexpr uint64_t kMaxChunk = 1ull << 30;
constexpr uint64_t kBitPos0 = 8ull * kBgzwHeaderBytes;  // the DEFLATE stream begins behind the 18 header bytes
static_assert(kThreads <= 1024 && kThreads % kWave == 0 && (uint32_t)kThreads >= kBgzwStep, "one lane per position of a step");
static_assert(kSlotBytes % 16 == 0 && kSlotBytes >= kBgzwMaxMember + 8 && kImgWords >= kTableWords, "a slot holds the stored form; the image holds the table");

struct alignas(16) EncodeLds {
    uint32_t img[kImgWords];                            // first the candidate table, then the member's bytes
    uint32_t in[kInWords];
    uint16_t tok[kThreads * kTokStride];                // candidate position + 1 of every position, then the tokens
    uint32_t crc_table[256];
    uint32_t hist[288], dhist[32];
    uint32_t node_freq[2 * kGzLitSyms], dnode_freq[2 * kBgzwDistSyms];
    uint32_t count[kGzMaxBits + 1], first[kGzMaxBits + 1], dcount[kGzMaxBits + 1];
    uint32_t wave_sum[kWaves];
    uint32_t xp[12];                                    // x^(8 x 64 x 2^k) mod P
    uint32_t n_used, hdr_bits, crc_full, crc_part, n_matches, n_literals;
    uint16_t order[288], parent[2 * kGzLitSyms], codes[288], dorder[32], dparent[2 * kBgzwDistSyms], dcodes[32];
    uint8_t lens[288], dlens[32];
    GzClWork clw;
};
static_assert(sizeof(EncodeLds) <= 150 * 1024, "one workgroup per CU");

// dword d of the member at `in` (any alignment); bytes at or behind n read as 0
__device__ inline uint32_t load_dword(const uint8_t* __restrict__ in, uint32_t d, uint32_t n) {
    const uint32_t b = 4u * d;
    if (b >= n) return 0u;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(in) + b;
    const uint32_t a = (uint32_t)(addr & 3u);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(addr - a);
    uint32_t v = w[0];
    if (a) {
        v >>= 8u * a;
        if (b + (4u - a) < n) v |= w[1] << (32u - 8u * a);          // the next dword holds bytes of the member
    }
    const uint32_t left = n - b;
    return left >= 4u ? v : v & ((1u << (8u * left)) - 1u);
}

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
    if (tid < 288) { S.hist[tid] = 0u; S.lens[tid] = 0; S.codes[tid] = 0; }
    if (tid < 32) S.dhist[tid] = 0u;
    if (tid < 256) S.crc_table[tid] = crc32_table_entry(tid);
    if (tid < 16) S.in[kThreads * kInStride + tid] = 0u;
    if (tid <= (uint32_t)kGzMaxBits) S.count[tid] = 0u;
    if (tid == 320) {
        uint32_t p = 0x00800000u;                       // x^8
        for (int k = 0; k < 6; ++k) p = crc32_mulmod(p, p);        // x^(8 x 64)
        for (int k = 0; k < 12; ++k) { S.xp[k] = p; p = crc32_mulmod(p, p); }
        S.crc_full = 0u; S.crc_part = 0u; S.n_matches = 0u; S.n_literals = 0u;
    }
    for (uint32_t k = 0; k < kBgzwPayload / 4 / kThreads; ++k) {
        const uint32_t d = tid + k * kThreads;
        S.in[(d >> 4) * kInStride + (d & 15u)] = load_dword(in, d, n);
    }
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
        for (uint32_t j = 0; j < len; ++j) crc = S.crc_table[(crc ^ byte_at(c0 + j)) & 0xffu] ^ (crc >> 8);
        crc = ~crc;
        // slices in front of the last (partial) one are weighted by x^(8 x 64 x slices behind them); the factor of the partial
        // slice's bytes is applied once to their sum
        const uint32_t full = n / kBgzwSlice;
        uint32_t p = 0u;
        if (tid < full) {
            p = crc;
            const uint32_t behind = full - tid - 1u;
            for (int k = 0; k < 9; ++k) if ((behind >> k) & 1u) p = crc32_mulmod(S.xp[k], p);
        } else if (tid == full && len) {
            S.crc_part = crc;
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) p ^= __shfl_xor(p, o);
        if (lane == 0 && p) atomicXor(&S.crc_full, p);
    }
    {
        uint32_t n_m = 0, n_l = 0;
        bgzw_slice_tokens(byte_at, [&](uint32_t i) -> uint32_t { return tok_at(i); }, c0, c1, [&](uint32_t pos, uint32_t l, uint32_t dist) {
            tok_at(pos) = (uint16_t)l;
            atomicAdd(&S.hist[gz_token_symbol(byte_at(pos), l)], 1u);
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
    if (tid == 0) atomicAdd(&S.hist[kGzEob], 1u);
    __syncthreads();
    // the tokens of the slice again: f(position, length, distance)
    auto tokens = [&](auto f) {
        for (uint32_t i = c0; i < c1;) {
            const uint32_t l = tok_at(i);
            f(i, l, l > 1u ? (uint32_t)tok_at(i + 1u) + 1u : 0u);
            i += l;
        }
    };

    // ---- the two codes (huff_lengths_serial, one lane per item where items are independent; the distance code by lane 64)
    if (tid < (uint32_t)kGzLitSyms && S.hist[tid]) {
        int u;
        const int r = huff_rank(S.hist, kGzLitSyms, (int)tid, &u);
        S.order[r] = (uint16_t)tid;
        if (tid == (uint32_t)kGzEob) S.n_used = (uint32_t)u;
    }
    __syncthreads();
    const int n_used = (int)S.n_used;                   // >= 2: the member's first byte is a literal, and the end-of-block symbol
    if (tid == 0) huff_merge(S.hist, S.order, n_used, S.node_freq, S.parent);
    if (tid == 64) {
        huff_lengths_serial(S.dhist, kBgzwDistSyms, kGzMaxBits, S.dlens, S.dorder, S.dparent, S.dnode_freq, S.dcount);
        for (int s = 0; s < kBgzwDistSyms; ++s) S.dcodes[s] = (uint16_t)huff_code_rev(S.dlens, kBgzwDistSyms, s);
    }
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

    // ---- the block header (one lane) and the bits of every slice
    if (tid == 0) S.hdr_bits = bgzw_write_block_header(S.lens, S.dlens, &S.clw, kBitPos0, [&](uint32_t w, uint32_t bits) { S.img[w] |= bits; });
    uint32_t my_bits = 0;
    tokens([&](uint32_t pos, uint32_t l, uint32_t dist) { my_bits += bgzw_token_bits(S.lens, S.dlens, byte_at(pos), l, dist); });
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
    const uint32_t coded = bgzw_coded_bytes(hdr + body + S.lens[kGzEob]), raw = bgzw_stored_bytes(n);
    const bool use_coded = coded < raw;                 // the same for every lane
    const uint32_t out_len = use_coded ? coded : raw;
    uint8_t* img8 = reinterpret_cast<uint8_t*>(S.img);

    // ---- pack
    if (use_coded) {
        auto or32 = [&](uint32_t w, uint32_t bits) { atomicOr(&S.img[w], bits); };
        uint64_t pos = kBitPos0 + hdr + before;
        tokens([&](uint32_t at, uint32_t l, uint32_t dist) {
            pos += bgzw_put_token(or32, pos, S.lens, S.codes, S.dlens, S.dcodes, byte_at(at), l, dist);
        });
        if (tid == 0) gz_put_bits(or32, kBitPos0 + hdr + body, S.codes[kGzEob], S.lens[kGzEob]);
    } else {
        for (uint32_t i = tid; i < kImgWords; i += kThreads) S.img[i] = 0u;    // the block header that lane 0 wrote
        __syncthreads();
        for (uint32_t j = 0; j < len; ++j) img8[kBgzwHeaderBytes + 5u + c0 + j] = (uint8_t)byte_at(c0 + j);
    }
    __syncthreads();
    if (tid == 0) {                                     // every bit is in place: plain byte stores
        const uint32_t r = n % kBgzwSlice;
        const uint32_t crc = r ? crc32_mulmod(crc32_xpow8(r), S.crc_full) ^ S.crc_part : S.crc_full;
        bgzw_member_header(out_len, img8);
        if (!use_coded) bgzw_stored_header(n, img8 + kBgzwHeaderBytes);
        bgzw_member_trailer(crc, n, img8 + out_len - kBgzwTrailerBytes);
    }
    __syncthreads();

    // ---- store
    uint4* slot = slots + (uint64_t)blockIdx.x * (kSlotBytes / 16);
    const uint4* img4 = reinterpret_cast<const uint4*>(S.img);
    for (uint32_t i = tid; i < (out_len + 15u) / 16u; i += kThreads) slot[i] = img4[i];
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
    sfgpu_text_sink sink = nullptr;
    void* user = nullptr;
    uint64_t chunk_bytes = 0;
    bool broken = false;                                // a write failed: the file cannot be continued
    sfgpu_bgzw_result res{};
    hipStream_t st = nullptr, cs = nullptr;
    hipEvent_t ev_in = nullptr, ev_e0 = nullptr, ev_e1 = nullptr, ev_c0[2] = {nullptr, nullptr}, ev_c1[2] = {nullptr, nullptr};
    char* pinned[2] = {nullptr, nullptr};
    uint64_t pinned_cap = 0;
    uint64_t* h_meta = nullptr;                         // total bytes of the batch just encoded; stored members, matches, literals so far
    DevBuf<uint4> slots;
    DevBuf<uint32_t> mem_len;
    DevBuf<uint64_t> mem_off;
    DevBuf<unsigned long long> stats;
    DevBuf<uint8_t> out[2];
    CallScope scope;                                    // streams, events, h_meta; last, so that it drains before the DevBufs go
    ~sfgpu_bgzw() {
        scope.drain();
        for (char* p : pinned) if (p) pinned_free(p);   // the staging buffers grow between writes: not the scope's
    }
};

namespace {

int bgzw_sink(sfgpu_bgzw* z, const char* bytes, uint64_t n, const char* who) {
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

int bgzw_open_impl(sfgpu_bgzw* z) {
    SF_HIP(z->scope.acquire(&z->st));
    SF_HIP(z->scope.acquire(&z->cs));
    SF_HIP(z->scope.event(&z->ev_in, hipEventDisableTiming));
    for (hipEvent_t* e : {&z->ev_e0, &z->ev_e1, &z->ev_c0[0], &z->ev_c1[0], &z->ev_c0[1], &z->ev_c1[1]}) SF_HIP(z->scope.event(e));
    SF_HIP(z->scope.pinned_block(&z->h_meta, 4 * sizeof(uint64_t)));
    if (int rc = z->stats.reserve(3, z->st, false)) return rc;
    SF_HIP(hipMemsetAsync(z->stats.p, 0, 3 * sizeof(unsigned long long), z->st));
    SF_HIP(hipStreamSynchronize(z->st));
    return SFGPU_OK;
}

int bgzw_write_impl(sfgpu_bgzw* z, const uint8_t* d_src, uint64_t n_bytes, sfgpu_stream stream) {
    hipStream_t st = z->st, cs = z->cs;
    SF_HIP(hipEventRecord(z->ev_in, as_stream(stream)));       // behind whatever the caller has queued on `stream`
    SF_HIP(hipStreamWaitEvent(st, z->ev_in, 0));
    const uint64_t n_members = (n_bytes + kBgzwPayload - 1) / kBgzwPayload;
    const uint64_t n_batches = (n_members + kBatchMembers - 1) / kBatchMembers;
    const uint64_t max_nm = n_members < kBatchMembers ? n_members : kBatchMembers;
    // staging: as large as a piece of this write can get, at most chunk_bytes (nothing is in flight between writes)
    const uint64_t stage = z->chunk_bytes < max_nm * kSlotBytes ? z->chunk_bytes : max_nm * kSlotBytes;
    if (stage > z->pinned_cap) {
        for (int b = 0; b < 2; ++b) {
            if (z->pinned[b]) { pinned_free(z->pinned[b]); z->pinned[b] = nullptr; }
            z->pinned_cap = 0;
            SF_HIP(pinned_malloc(&z->pinned[b], stage));
        }
        z->pinned_cap = stage;
    }
    if (int rc = z->slots.reserve(max_nm * (kSlotBytes / 16), st, false)) return rc;
    if (int rc = z->mem_len.reserve(max_nm + 1, st, false)) return rc;
    if (int rc = z->mem_off.reserve(max_nm + 1, st, false)) return rc;
    for (int b = 0; b < 2 && (uint64_t)b < n_batches; ++b) if (int rc = z->out[b].reserve(max_nm * kSlotBytes, st, false)) return rc;

    auto batch_members = [&](uint64_t i) -> uint32_t {
        return (uint32_t)(n_members - i * kBatchMembers < kBatchMembers ? n_members - i * kBatchMembers : kBatchMembers);
    };
    // encode + scan + compact of batch i on st into out[i & 1]; every copy that read this buffer has been waited for, and the
    // sizes of the batch before have been read
    auto enqueue = [&](uint64_t i) -> int {
        const uint32_t nm = batch_members(i);
        const uint64_t b0 = i * kBatchMembers * (uint64_t)kBgzwPayload;
        const uint64_t bytes = n_bytes - b0 < (uint64_t)nm * kBgzwPayload ? n_bytes - b0 : (uint64_t)nm * kBgzwPayload;
        SF_HIP(hipEventRecord(z->ev_e0, st));
        hipLaunchKernelGGL(k_bgzw_encode, dim3(nm), dim3(kThreads), 0, st, d_src + b0, bytes, z->slots.p, z->mem_len.p, z->stats.p);
        SF_HIP(hipGetLastError());
        if (int rc = exclusive_scan_u32(z->mem_len.p, z->mem_off.p, nm, st, false)) return rc;
        hipLaunchKernelGGL(k_slot_compact<kSlotBytes>, dim3(nm), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(z->slots.p), z->mem_off.p,
                           z->out[i & 1].p);
        SF_HIP(hipGetLastError());
        SF_HIP(hipEventRecord(z->ev_e1, st));
        SF_HIP(hipMemcpyAsync(z->h_meta, z->mem_off.p + nm, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(z->h_meta + 1, z->stats.p, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        return SFGPU_OK;
    };
    int pb = 0;                                         // pinned buffer of the next piece
    auto copy_piece = [&](int p, const uint8_t* d, uint64_t len) -> int {
        SF_HIP(hipEventRecord(z->ev_c0[p], cs));
        SF_HIP(hipMemcpyAsync(z->pinned[p], d, len, hipMemcpyDeviceToHost, cs));
        SF_HIP(hipEventRecord(z->ev_c1[p], cs));
        return SFGPU_OK;
    };
    if (int rc = enqueue(0)) return rc;
    for (uint64_t i = 0; i < n_batches; ++i) {
        SF_HIP(hipStreamSynchronize(st));               // batch i is encoded, its size and the counters are here
        add_elapsed(&z->res.encode_ms, z->ev_e0, z->ev_e1);
        const uint64_t total = z->h_meta[0];
        z->res.n_stored_members = z->h_meta[1]; z->res.n_matches = z->h_meta[2]; z->res.n_literals = z->h_meta[3];
        z->res.n_members += batch_members(i);
        if (i + 1 < n_batches) if (int rc = enqueue(i + 1)) return rc;
        const uint8_t* d_out = z->out[i & 1].p;
        const uint64_t chunk = z->pinned_cap < z->chunk_bytes ? z->pinned_cap : z->chunk_bytes;
        if (int rc = copy_piece(pb, d_out, total < chunk ? total : chunk)) return rc;
        for (uint64_t off = 0; off < total;) {
            const uint64_t len = total - off < chunk ? total - off : chunk, next = off + len;
            if (next < total) if (int rc = copy_piece(pb ^ 1, d_out + next, total - next < chunk ? total - next : chunk)) return rc;
            SF_HIP(hipEventSynchronize(z->ev_c1[pb]));
            add_elapsed(&z->res.d2h_ms, z->ev_c0[pb], z->ev_c1[pb]);
            if (int rc = bgzw_sink(z, z->pinned[pb], len, "sfgpu_bgzw_write_device")) return rc;
            off = next; pb ^= 1;
        }
    }
    z->res.n_bytes_in += n_bytes;
    return SFGPU_OK;
}

}  // namespace

extern "C" int sfgpu_bgzw_open(sfgpu_bgzw** out, sfgpu_text_sink sink, void* user, uint64_t chunk_bytes) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_bgzw_open: null handle pointer");
    *out = nullptr;
    SF_REQUIRE(sink, SFGPU_ERR_INVALID, "sfgpu_bgzw_open: null sink");
    if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
    SF_REQUIRE(chunk_bytes >= 16 && chunk_bytes <= kMaxChunk, SFGPU_ERR_INVALID, "sfgpu_bgzw_open: chunk_bytes must lie in [16, 2^30] (0 = default)");
    sfgpu_bgzw* z = new (std::nothrow) sfgpu_bgzw;
    SF_REQUIRE(z, SFGPU_ERR_HIP, "sfgpu_bgzw_open: out of host memory");
    z->sink = sink; z->user = user; z->chunk_bytes = chunk_bytes;
    const int rc = bgzw_open_impl(z);
    if (rc != SFGPU_OK) { delete z; return rc; }
    *out = z;
    return SFGPU_OK;
}

extern "C" int sfgpu_bgzw_write_device(sfgpu_bgzw* z, const void* d_src, uint64_t n_bytes, sfgpu_stream stream) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_bgzw_write_device: null handle");
    SF_REQUIRE(!z->broken, SFGPU_ERR_STATE, "sfgpu_bgzw_write_device: an earlier write failed; close the file");
    if (n_bytes == 0) return SFGPU_OK;
    SF_REQUIRE(d_src, SFGPU_ERR_INVALID, "sfgpu_bgzw_write_device: null source");
    const int rc = bgzw_write_impl(z, static_cast<const uint8_t*>(d_src), n_bytes, stream);
    if (rc != SFGPU_OK) {
        z->broken = true;                               // nothing may stay in flight behind a failed write
        z->scope.drain();
    }
    return rc;
}

extern "C" int sfgpu_bgzw_close(sfgpu_bgzw* z, sfgpu_bgzw_result* res) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_bgzw_close: null handle");
    int rc = SFGPU_OK;
    if (!z->broken) {
        uint8_t tail[kBgzwEofBytes];
        bgzw_eof_member(tail);
        rc = bgzw_sink(z, reinterpret_cast<const char*>(tail), sizeof(tail), "sfgpu_bgzw_close");
    }
    if (res) *res = z->res;
    delete z;
    return rc;
}
