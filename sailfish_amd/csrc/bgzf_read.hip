// bgzf_read.hip -- blocked gzip (BGZF) inflated on the device: sfgpu_bgzf_inflate_host.  What a member is and how it inflates is
// decided by bgzfmt.h (the same functions run serially in tests/bgzf_harness.cpp); this file is the wave-level IO policy under
// bgz_inflate_body, the kernel around it and the staging.
//
// Host: bgz_scan hops from member to member over the BC sizes (headers and trailers only) and builds the directory
// (in_off, out_off, in_len, isize).  The compressed bytes go through two pinned buffers in sub-chunks of kSubBytes; the copy of
// sub-chunk c + 1 runs on the copy stream while members that have arrived are inflated -- kLaunchMembers of them at a time, or
// what is left behind the last copy: a launch lasts as long as its slowest member, so small launches would add up to many such
// latencies on a mostly empty device.
//
// Kernel: one wavefront per member, kWaves members per workgroup.  The decode is one serial bit stream per member, so all 64
// lanes run bgz_inflate_body's statements on the same values (wave-uniform: no divergence, reads of one LDS address broadcast);
// the lanes part only where there is something to spread:
//   - the compressed bytes are seen through a kStageBytes window in LDS that all lanes refill with 16-byte loads,
//   - the decode tables (BgzTables, 4 KB) are in LDS; one lane builds them,
//   - the payload goes straight to its place in d_dst: literals are collected one per lane and stored 64 at a time, match and
//     stored copies are spread over the lanes (a match with distance < length reads the last `distance` bytes periodically, so it needs no order either),
//   - the CRC-32 is taken by lane slices of the payload and combined with gzfmt.h's x^(8n) mod P.
// The window onto the payload lives in global memory, not in LDS: ~6 KB of LDS per wave keep 24 waves on a CU where a 64 KB
// window per wave would keep two.  A wave reads back only bytes that it stored itself, in program order.
#include <vector>

#include "common.h"
#include "bgzfmt.h"
#include "wave_crc.h"

namespace sfgpu {
namespace {

constexpr int kWaves = 4;                                // members per workgroup
constexpr uint32_t kStageBytes = 2048;                   // LDS window onto the compressed bytes: 64 lanes x 2 x 16 bytes
constexpr uint32_t kSrcPad = kStageBytes + 32;           // readable bytes behind the compressed bytes in device memory
constexpr uint64_t kSubBytes = 4ull << 20;               // staged sub-chunk
constexpr uint64_t kLaunchMembers = 4096;                // members that wait for a launch before the last copy
constexpr uint64_t kMaxBytes = 1ull << 30;
constexpr unsigned long long kNoError = ~0ull;

struct WaveLds {
    BgzTables T;
    uint4 in[kStageBytes / 16];
};

struct WaveIO {
    const uint4* frame;       // the 16-byte group of device memory in which the member begins
    uint8_t* out;             // the member's payload
    uint4* in;                // LDS window: bytes [base, base + kStageBytes) of the frame
    uint32_t base;
    uint32_t lane;
    uint32_t pend_n, pend_o, mine;      // literals not stored yet: lane k holds the k-th of them, they go to out[pend_o ..)

    __device__ void load(uint32_t p) {
        base = p & ~15u;
        const uint4* g = frame + (base >> 4);
        in[lane] = g[lane];
        in[lane + 64u] = g[lane + 64u];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    __device__ uint32_t word(uint32_t p) {
        if (p - base >= kStageBytes) load(p);              // p never falls below base: the reader only moves on
        return uniform(reinterpret_cast<const uint32_t*>(in)[(p - base) >> 2]);
    }
    // Every lane decodes the same stream, but the compiler cannot know that of a value read from LDS: without this the bit
    // reader lives in vector registers and every `if` of the decode becomes an exec-mask sequence (~1000 cycles per symbol).
    // With it the reader's state is scalar and the branches are scalar branches.
    __device__ uint32_t uniform(uint32_t v) const { return __builtin_amdgcn_readfirstlane(v); }
    template <typename F>
    __device__ void single(F f) {
        if (lane == 0u) f();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    __device__ bool status(const BgzTables* T) const { return uniform((uint32_t)*reinterpret_cast<const volatile int32_t*>(&T->status)) != 0u; }
    __device__ void store_len(BgzTables* T, uint32_t i, uint32_t v) const { if (lane == 0u) T->lens[i] = (uint8_t)v; }
    // A byte store per literal makes every literal a partial write of one cache line, and those queue up behind one another:
    // literals are collected one per lane and leave as one store of up to 64 consecutive bytes.
    __device__ void flush() {
        if (lane < pend_n) out[pend_o + lane] = (uint8_t)mine;
        pend_n = 0;
    }
    __device__ void put(uint32_t o, uint32_t b) {
        if (pend_n == 0u) pend_o = o;
        if (lane == pend_n) mine = b;
        if (++pend_n == 64u) flush();
    }
    __device__ void copy(uint32_t o, uint32_t dist, uint32_t len) {
        flush();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint8_t* from = out + o - dist;              // every source byte lies below o, every destination at or above it
        if (dist >= len) {
            for (uint32_t i = lane; i < len; i += 64u) out[o + i] = from[i];
        } else if (dist == 1u) {
            const uint8_t b = from[0];
            for (uint32_t i = lane; i < len; i += 64u) out[o + i] = b;
        } else {
            for (uint32_t i = lane; i < len; i += 64u) out[o + i] = from[i % dist];
        }
    }
    __device__ void stored(uint32_t o, uint32_t p, uint32_t len) {
        flush();
        const uint8_t* from = reinterpret_cast<const uint8_t*>(frame) + p;
        for (uint32_t i = lane; i < len; i += 64u) out[o + i] = from[i];
    }
};

// res[0] = min over the bad members of (member << 8 | kind), res[1 .. 4) += blocks by type
__global__ void __launch_bounds__(kWaves * kWave) k_bgzf_inflate(const uint8_t* __restrict__ src, const BgzDirEntry* __restrict__ dir, uint32_t m0,
                                                                 uint32_t m1, uint8_t* dst, unsigned long long* __restrict__ res) {
    __shared__ WaveLds lds[kWaves];
    __shared__ uint32_t crc_table[256];
    for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) crc_table[i] = crc32_table_entry(i);
    __syncthreads();
    // (the wave's number is the same in all its lanes; said so that the member, and with it the decode state, is scalar)
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const uint64_t m = (uint64_t)m0 + (uint64_t)blockIdx.x * kWaves + wave;
    if (m >= m1) return;
    const BgzDirEntry e = dir[m];
    const uint8_t* member = src + e.in_off;
    auto byte = [&](uint64_t p) -> uint32_t { return member[p]; };

    // the header again, against what the directory says
    BgzHeader h;
    int kind = bgz_parse_header(byte, e.in_len, &h);
    if (kind != SFGPU_BGZF_OK || h.total != e.in_len) kind = SFGPU_BGZF_BAD_HEADER;
    BgzCounts cnt;
    cnt.n_out = 0; cnt.blocks[0] = cnt.blocks[1] = cnt.blocks[2] = 0;
    if (kind == SFGPU_BGZF_OK) {
        const uint32_t end_pos = h.total - kBgzTrailer;
        const uint32_t crc_stored = bgz_le32(byte, end_pos), isize = bgz_le32(byte, end_pos + 4u);
        if (isize != e.isize || isize > kBgzMaxPayload) {
            kind = SFGPU_BGZF_BAD_HEADER;
        } else {
            const uint32_t skew = (uint32_t)(e.in_off & 15u);
            WaveIO io;
            io.frame = reinterpret_cast<const uint4*>(member - skew);
            io.out = dst + e.out_off;
            io.in = lds[wave].in;
            io.lane = lane;
            io.pend_n = 0; io.pend_o = 0; io.mine = 0;
            io.load(skew + h.hdr_len);
            uint32_t stream_end = 0;
            const int body = bgz_inflate_body(io, &lds[wave].T, skew + h.hdr_len, skew + end_pos, isize, &cnt, &stream_end);
            io.flush();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const uint32_t n = cnt.n_out;
            const uint32_t crc = wave_crc32(io.out, n, lane, crc_table);
            kind = bgz_finish(body, stream_end, skew + end_pos, n, isize, crc, crc_stored);
        }
    }
    if (lane == 0u) {
        if (kind != SFGPU_BGZF_OK) atomicMin(&res[0], ((unsigned long long)m << 8) | (unsigned long long)kind);
        for (int t = 0; t < 3; ++t) if (cnt.blocks[t]) atomicAdd(&res[1 + t], (unsigned long long)cnt.blocks[t]);
    }
}

const char* kind_text(int kind) {
    switch (kind) {
        case SFGPU_BGZF_BAD_HEADER: return "not a BGZF member header (gzip magic, BC subfield, BSIZE, ISIZE <= 65536)";
        case SFGPU_BGZF_TRUNCATED: return "the member ends before its last block does";
        case SFGPU_BGZF_BAD_BLOCK_TYPE: return "block type 3";
        case SFGPU_BGZF_STORED_LEN: return "a stored block's LEN and NLEN disagree";
        case SFGPU_BGZF_BAD_CODE_LENGTHS: return "invalid code lengths";
        case SFGPU_BGZF_BAD_SYMBOL: return "invalid literal/length or distance code";
        case SFGPU_BGZF_DISTANCE_TOO_FAR: return "a match reaches before the member's first byte";
        case SFGPU_BGZF_SIZE_MISMATCH: return "the payload is not ISIZE bytes";
        case SFGPU_BGZF_CRC_MISMATCH: return "CRC-32 mismatch";
        default: return "malformed";
    }
}

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_bgzf_inflate_host(const void* h_src, uint64_t n_bytes, int final, uint8_t* d_dst, uint64_t cap_bytes,
                                       sfgpu_bgzf_result* out, sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_bgzf_inflate_host: null result");
    memset(out, 0, sizeof(*out));
    out->error_member = ~0ull;
    SF_REQUIRE(n_bytes <= kMaxBytes, SFGPU_ERR_RANGE, "sfgpu_bgzf_inflate_host: more than 2^30 bytes in one call");
    SF_REQUIRE(n_bytes == 0 || h_src, SFGPU_ERR_INVALID, "sfgpu_bgzf_inflate_host: null input");
    const uint8_t* src = static_cast<const uint8_t*>(h_src);
    hipStream_t st = as_stream(stream);

    // ---- the directory
    std::vector<BgzDirEntry> dir;
    const bool sizing = d_dst == nullptr;
    const BgzScan scan = bgz_scan(src, n_bytes, final ? 1 : 0, cap_bytes, [&](const BgzDirEntry& e) { if (!sizing) dir.push_back(e); });
    out->n_members = scan.n_members; out->consumed = scan.consumed; out->n_bytes_out = scan.n_bytes_out;
    unsigned long long err = scan.error_kind != SFGPU_BGZF_OK ? ((unsigned long long)scan.error_member << 8) | (unsigned long long)scan.error_kind
                                                              : kNoError;
    auto finish = [&]() -> int {
        if (err == kNoError) return SFGPU_OK;
        out->error_member = err >> 8; out->error_kind = (int32_t)(err & 0xff);
        set_error("bgzf: member %llu of this input: %s", (unsigned long long)out->error_member, kind_text(out->error_kind));
        return SFGPU_ERR_FORMAT;
    };
    if (sizing || dir.empty()) {
        if (!sizing) SF_HIP(hipStreamSynchronize(st));
        return finish();
    }

    // ---- staging
    const uint64_t n_copy = scan.consumed, n_sub = (n_copy + kSubBytes - 1) / kSubBytes, M = dir.size();
    DevBuf<uint4> comp;
    DevBuf<BgzDirEntry> ddir;
    DevBuf<unsigned long long> res;
    CallScope scope;        // after the DevBufs: it drains both streams before their blocks go back to the pool
    hipStream_t cs = nullptr;
    uint8_t* pinned[2] = {nullptr, nullptr};
    BgzDirEntry* h_dir = nullptr;
    unsigned long long* h_res = nullptr;
    hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr}, ev_c0[2] = {nullptr, nullptr}, ev_c1[2] = {nullptr, nullptr};
    hipEvent_t ev_ready = nullptr;
    bool in_flight[2] = {false, false};
    auto collect = [&](int slot) {
        if (!in_flight[slot]) return;
        (void)hipEventSynchronize(ev_c1[slot]);
        add_elapsed(&out->ms_copy, ev_h2d[slot], ev_copied[slot]);
        add_elapsed(&out->ms_kernels, ev_c0[slot], ev_c1[slot]);
        in_flight[slot] = false;
    };
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.acquire(&cs));
    for (int b = 0; b < 2 && (uint64_t)b < n_sub; ++b) {
        SF_HIP(scope.pinned_block(&pinned[b], n_copy < kSubBytes ? n_copy : kSubBytes));
        for (hipEvent_t* e : {&ev_h2d[b], &ev_copied[b], &ev_c0[b], &ev_c1[b]}) SF_HIP(scope.event(e));
    }
    SF_HIP(scope.event(&ev_ready));
    SF_HIP(scope.pinned_block(&h_dir, M * sizeof(BgzDirEntry)));
    SF_HIP(scope.pinned_block(&h_res, 4 * sizeof(unsigned long long)));
    if (int r = comp.reserve((n_copy + kSrcPad + 15) / 16, st, false)) return r;
    if (int r = ddir.reserve(M, st, false)) return r;
    if (int r = res.reserve(4, st, false)) return r;
    memcpy(h_dir, dir.data(), M * sizeof(BgzDirEntry));
    SF_HIP(hipMemcpyAsync(ddir.p, h_dir, M * sizeof(BgzDirEntry), hipMemcpyHostToDevice, st));
    SF_HIP(hipMemsetAsync(res.p, 0xff, 8, st));
    SF_HIP(hipMemsetAsync(res.p + 1, 0, 24, st));
    SF_HIP(hipEventRecord(ev_ready, st));
    SF_HIP(hipStreamWaitEvent(cs, ev_ready, 0));         // the copies stay behind whatever `stream` held and behind the reservations

    uint64_t m_done = 0;                                 // members [0, m_done) are launched
    for (uint64_t c = 0; c < n_sub; ++c) {
        const int slot = (int)(c & 1);
        collect(slot);                                   // its previous copy has left the pinned buffer
        const uint64_t p = c * kSubBytes, q = (c + 1 == n_sub) ? n_copy : p + kSubBytes;
        memcpy(pinned[slot], src + p, q - p);
        SF_HIP(hipEventRecord(ev_h2d[slot], cs));
        SF_HIP(hipMemcpyAsync(reinterpret_cast<uint8_t*>(comp.p) + p, pinned[slot], q - p, hipMemcpyHostToDevice, cs));
        SF_HIP(hipEventRecord(ev_copied[slot], cs));
        uint64_t m_end = m_done;                         // the members that end within the bytes copied so far
        while (m_end < M && dir[m_end].in_off + dir[m_end].in_len <= q) ++m_end;
        SF_HIP(hipStreamWaitEvent(st, ev_copied[slot], 0));
        SF_HIP(hipEventRecord(ev_c0[slot], st));
        if (m_end > m_done && (c + 1 == n_sub || m_end - m_done >= kLaunchMembers)) {
            hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)((m_end - m_done + kWaves - 1) / kWaves)), dim3(kWaves * kWave), 0, st,
                               reinterpret_cast<const uint8_t*>(comp.p), ddir.p, (uint32_t)m_done, (uint32_t)m_end, d_dst, res.p);
            SF_HIP(hipGetLastError());
            m_done = m_end;
        }
        SF_HIP(hipEventRecord(ev_c1[slot], st));
        in_flight[slot] = true;
    }
    SF_HIP(hipMemcpyAsync(h_res, res.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    collect(0); collect(1);
    if (h_res[0] < err) err = h_res[0];
    out->n_stored_blocks = h_res[1]; out->n_fixed_blocks = h_res[2]; out->n_dynamic_blocks = h_res[3];
    return finish();
}
