// gz_read.hip -- ordinary gzip inflated on the device, chunk by chunk: sfgpu_gzrd_open / _plan_host / _emit / _close.  What a
// candidate, a chunk, the chain and the propagation are is decided by gzrdfmt.h (the same functions run serially in
// tests/gzrd_harness.cpp); this file is the wave-level IO policies under gzr_decode_chunk, the four kernels and the staging.
//
//   k_gzrd_find        one wavefront per span.  The lanes take 64 consecutive bit offsets for the cheap test (ALU on four words
//                      per lane); the survivors of a ballot get the full header check one at a time, wave-uniform, with the
//                      decoder's own table code in LDS.
//   k_gzrd_pass_a      one wavefront per candidate (and one for the known start): gzr_decode_chunk into the chunk's ring of
//                      32768 sixteen-bit symbols in global memory (64 KB per span, from the pool).
//   k_gzrd_propagate   one workgroup walks the chain: the previous resolved window is in LDS (32 KB), each thread resolves 32
//                      entries of the next one, keeps them in registers over the barrier and writes them to LDS and to memory.
//   k_gzrd_pass_b      one wavefront per chain chunk: gzr_decode_chunk again, bytes to the chunk's exact offset in d_dst, copies
//                      that reach before the chunk read the resolved window; then the chunk's CRC-32.
// Pass A and pass B are bgzf_read.hip's form: every lane runs the decoder's statements on the same values, the state is scalar
// via readfirstlane, tables and a 2 KB window onto the input are in LDS (~6 KB per wave: 24 waves per CU), literals are collected
// one per lane and stored 64 at a time, copies are spread over the lanes.  Every value stored to memory leaves through ordinary
// vector stores.
//
// Host: the member header, the chain (gzr_chain, on the records pass A wrote: 40 bytes per span) and the CRC combination run on
// the host; the compressed bytes go through two pinned buffers in sub-chunks of kSubBytes.
#include <vector>

#include "common.h"
#include "gzrdfmt.h"
#include "wave_crc.h"

namespace sfgpu {
namespace {

constexpr int kWaves = 4;                                // chunks (spans) per workgroup
constexpr uint32_t kStageBytes = 2048;                   // LDS window onto the compressed bytes: 64 lanes x 2 x 16 bytes
constexpr uint32_t kSrcPad = kStageBytes + 64;           // readable bytes behind the compressed bytes in device memory
constexpr uint64_t kSubBytes = 4ull << 20;               // staged sub-chunk
constexpr uint64_t kMaxBytes = 1ull << 30;
constexpr uint64_t kMaxSpans = 65536;                    // per call: 1 GiB at the default chunk_bytes; bounds the rings at 4 GiB
constexpr int kPropThreads = 1024;

struct WaveLds {
    BgzTables T;
    uint4 in[kStageBytes / 16];
};

// the reading half of the policy: bgzf_read.hip's WaveIO
struct WaveIn {
    const uint4* frame;       // the call's compressed bytes (16-byte aligned, kSrcPad readable bytes behind them)
    uint4* in;                // LDS window: bytes [base, base + kStageBytes) of the frame
    uint32_t base;
    uint32_t lane;

    __device__ void load(uint32_t p) {
        base = p & ~15u;
        const uint4* g = frame + (base >> 4);
        in[lane] = g[lane];
        in[lane + 64u] = g[lane + 64u];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    __device__ uint32_t word(uint32_t p) {
        if (p - base >= kStageBytes) load(p);              // (also when the finder steps back: the difference wraps)
        return uniform(reinterpret_cast<const uint32_t*>(in)[(p - base) >> 2]);
    }
    __device__ uint32_t uniform(uint32_t v) const { return __builtin_amdgcn_readfirstlane(v); }
    template <typename F>
    __device__ void single(F f) {
        if (lane == 0u) f();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    __device__ bool status(const BgzTables* T) const { return uniform((uint32_t)*reinterpret_cast<const volatile int32_t*>(&T->status)) != 0u; }
    __device__ void store_len(BgzTables* T, uint32_t i, uint32_t v) const { if (lane == 0u) T->lens[i] = (uint8_t)v; }
};

// pass A: symbols into the ring
struct RingIO : WaveIn {
    uint16_t* ring;
    uint32_t pend_n, pend_o, mine;      // literals not stored yet: lane k holds the k-th of them, they go to ring[pend_o + k]

    __device__ void flush() {
        if (lane < pend_n) ring[(pend_o + lane) & kGzrMask] = (uint16_t)mine;
        pend_n = 0;
    }
    __device__ void put(uint64_t o, uint32_t b) {
        if (pend_n == 0u) pend_o = (uint32_t)o;
        if (lane == pend_n) mine = b;
        if (++pend_n == 64u) flush();
    }
    // Sources lie in [o - dist, o), destinations in [o, o + len): as ring slots they can only meet when dist > 32768 - len, and
    // then a slot is read (by the lane whose store depends on that load) before the lane that owns it stores to it.
    __device__ void copy(uint64_t o, uint32_t dist, uint32_t len) {
        flush();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t to = (uint32_t)o, from = to - dist;
        if (dist >= len) {
            for (uint32_t i = lane; i < len; i += 64u) ring[(to + i) & kGzrMask] = ring[(from + i) & kGzrMask];
        } else {
            for (uint32_t i = lane; i < len; i += 64u) ring[(to + i) & kGzrMask] = ring[(from + i % dist) & kGzrMask];
        }
    }
    __device__ void stored(uint64_t o, uint32_t p, uint32_t len) {
        flush();
        const uint8_t* from = reinterpret_cast<const uint8_t*>(frame) + p;
        for (uint32_t i = lane; i < len; i += 64u) ring[((uint32_t)o + i) & kGzrMask] = from[i];
    }
};

// pass B: bytes to out[0 .. limit), the resolved window win[0 .. 32768) in front of out[0]
struct ByteIO : WaveIn {
    uint8_t* out;
    const uint8_t* win;
    uint32_t limit;           // what pass A counted: nothing is stored at or behind it
    uint32_t pend_n, pend_o, mine;

    __device__ void flush() {
        if (lane < pend_n && pend_o + lane < limit) out[pend_o + lane] = (uint8_t)mine;
        pend_n = 0;
    }
    __device__ void put(uint64_t o, uint32_t b) {
        if (pend_n == 0u) pend_o = (uint32_t)o;
        if (lane == pend_n) mine = b;
        if (++pend_n == 64u) flush();
    }
    __device__ void copy(uint64_t o64, uint32_t dist, uint32_t len) {
        flush();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t o = (uint32_t)o64;
        if (o64 + len > limit) return;
        if (dist <= o) {                                   // bgzf_read.hip's copy: all of it is the chunk's own output
            const uint8_t* from = out + o - dist;
            if (dist >= len) {
                for (uint32_t i = lane; i < len; i += 64u) out[o + i] = from[i];
            } else if (dist == 1u) {
                const uint8_t b = from[0];
                for (uint32_t i = lane; i < len; i += 64u) out[o + i] = b;
            } else {
                for (uint32_t i = lane; i < len; i += 64u) out[o + i] = from[i % dist];
            }
        } else {                                           // split at the window boundary (dist <= o + valid <= o + 32768)
            const uint32_t back = dist - o;                // source byte j < back is win[32768 - back + j], the others out[j - back]
            for (uint32_t i = lane; i < len; i += 64u) {
                const uint32_t j = dist >= len ? i : i % dist;
                out[o + i] = j < back ? win[kGzrWindow - back + j] : out[j - back];
            }
        }
    }
    __device__ void stored(uint64_t o64, uint32_t p, uint32_t len) {
        flush();
        if (o64 + len > limit) return;
        const uint32_t o = (uint32_t)o64;
        const uint8_t* from = reinterpret_cast<const uint8_t*>(frame) + p;
        for (uint32_t i = lane; i < len; i += 64u) out[o + i] = from[i];
    }
};

// cand[s] = the candidate of span s (kGzrNone: none; s = 0 has none)
__global__ void __launch_bounds__(kWaves * kWave) k_gzrd_find(const uint4* __restrict__ src, uint32_t n_bytes, uint64_t start_byte, uint32_t chunk_bytes,
                                                              uint32_t n_spans, uint64_t* __restrict__ cand) {
    __shared__ WaveLds lds[kWaves];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const uint32_t s = blockIdx.x * kWaves + wave;
    if (s >= n_spans) return;
    uint64_t found = kGzrNone;
    if (s) {
        const uint64_t n_bits = (uint64_t)n_bytes * 8u, q0 = (start_byte + (uint64_t)s * chunk_bytes) * 8u;
        const uint64_t q1 = q0 + (uint64_t)chunk_bytes * 8u < n_bits ? q0 + (uint64_t)chunk_bytes * 8u : n_bits;
        const uint32_t* words = reinterpret_cast<const uint32_t*>(src);
        WaveIn io;
        io.frame = src; io.in = lds[wave].in; io.lane = lane;
        io.load((uint32_t)(q0 >> 3));
        for (uint64_t base = q0; base < q1 && found == kGzrNone; base += 64u) {
            const uint64_t q = base + lane;
            const bool ok = q < q1 && gzr_cheap_test([&](uint32_t p) -> uint32_t { return words[p >> 2]; }, q, n_bits);
            unsigned long long mask = __ballot(ok);
            while (mask) {
                const uint64_t at = base + (uint64_t)__builtin_ctzll(mask);
                mask &= mask - 1ull;
                if (gzr_header_at(io, &lds[wave].T, at, n_bytes)) { found = at; break; }
            }
        }
    }
    if (lane == 0u) cand[s] = found;
}

// rec[s] = what the chunk that starts at the candidate of span s (s = 0: at start_bit) found; status -1 where there is no chunk
__global__ void __launch_bounds__(kWaves * kWave) k_gzrd_pass_a(const uint4* __restrict__ src, uint32_t n_bytes, uint64_t start_bit, uint32_t chunk_bytes,
                                                                uint32_t n_spans, const uint64_t* __restrict__ cand, uint16_t* __restrict__ rings,
                                                                GzrChunkRec* __restrict__ recs) {
    __shared__ WaveLds lds[kWaves];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const uint32_t s = blockIdx.x * kWaves + wave;
    if (s >= n_spans) return;
    const uint64_t at = s ? cand[s] : start_bit;
    GzrChunkRec rec;
    rec.end_bit = at; rec.n_out = 0; rec.blocks[0] = rec.blocks[1] = rec.blocks[2] = 0; rec.status = -1; rec.kind = 0; rec.pad_ = 0;
    if (at != kGzrNone) {
        RingIO io;
        io.frame = src; io.in = lds[wave].in; io.lane = lane;
        io.ring = rings + (uint64_t)s * kGzrWindow;
        io.pend_n = 0; io.pend_o = 0; io.mine = 0;
        uint32_t* ring2 = reinterpret_cast<uint32_t*>(io.ring);          // the identity, two entries per store
        for (uint32_t i = lane; i < kGzrWindow / 2u; i += 64u) ring2[i] = (kGzrMarker | (2u * i)) | ((kGzrMarker | (2u * i + 1u)) << 16);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        io.load((uint32_t)(at >> 3));
        const uint64_t start_byte = start_bit >> 3;
        gzr_decode_chunk(io, &lds[wave].T, at, n_bytes, kGzrWindow,
                         [&](uint64_t b) -> bool { return gzr_is_candidate(cand, n_spans, b, start_byte, chunk_bytes); }, &rec);
        io.flush();
    }
    if (lane == 0u) recs[s] = rec;
}

// chain[0 .. K) = spans, chain[K .. 2K) = n_out: resolved[k] = the window behind chain chunk k, k = 0 .. K - 2
__global__ void __launch_bounds__(kPropThreads) k_gzrd_propagate(const uint16_t* __restrict__ rings, const uint64_t* __restrict__ chain, uint32_t K,
                                                                 const uint8_t* __restrict__ win0, uint8_t* __restrict__ resolved) {
    __shared__ uint32_t prev[kGzrWindow / 4];
    const uint32_t t = threadIdx.x;
    constexpr uint32_t kPer = kGzrWindow / 4 / kPropThreads;            // words per thread
    for (uint32_t r = 0; r < kPer; ++r) prev[r * kPropThreads + t] = reinterpret_cast<const uint32_t*>(win0)[r * kPropThreads + t];
    __syncthreads();
    const uint8_t* prev_bytes = reinterpret_cast<const uint8_t*>(prev);
    for (uint32_t k = 0; k + 1 < K; ++k) {
        const uint16_t* ring = rings + chain[k] * kGzrWindow;
        const uint64_t n_out = chain[K + k];
        uint32_t w[kPer];
#pragma unroll
        for (uint32_t r = 0; r < kPer; ++r) {
            const uint32_t j = (r * kPropThreads + t) * 4u;
            uint32_t v = 0;
            for (uint32_t e = 0; e < 4u; ++e)
                v |= gzr_resolve([&](uint32_t i) -> uint32_t { return ring[i]; }, [&](uint32_t i) -> uint32_t { return prev_bytes[i]; }, n_out, j + e) << (8u * e);
            w[r] = v;
        }
        __syncthreads();
        uint32_t* out = reinterpret_cast<uint32_t*>(resolved + (uint64_t)k * kGzrWindow);
#pragma unroll
        for (uint32_t r = 0; r < kPer; ++r) { prev[r * kPropThreads + t] = w[r]; out[r * kPropThreads + t] = w[r]; }
        __syncthreads();
    }
}

// chain[2K ..) = start bits, [3K ..) = end bits, [4K ..) = output offsets, [5K ..) = valid window lengths;
// emit[2k] = the chunk's CRC-32, emit[2k + 1] = its kind
__global__ void __launch_bounds__(kWaves * kWave) k_gzrd_pass_b(const uint4* __restrict__ src, uint32_t n_bytes, const uint64_t* __restrict__ chain, uint32_t K,
                                                                const uint8_t* __restrict__ win0, const uint8_t* __restrict__ resolved, uint8_t* dst,
                                                                uint32_t* __restrict__ emit) {
    __shared__ WaveLds lds[kWaves];
    __shared__ uint32_t crc_table[256];
    for (uint32_t i = threadIdx.x; i < 256u; i += blockDim.x) crc_table[i] = crc32_table_entry(i);
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
    const uint32_t k = blockIdx.x * kWaves + wave;
    if (k >= K) return;
    const uint64_t n_out = chain[K + k], at = chain[2ull * K + k], end_bit = chain[3ull * K + k], out_off = chain[4ull * K + k];
    const uint32_t valid = (uint32_t)chain[5ull * K + k];
    ByteIO io;
    io.frame = src; io.in = lds[wave].in; io.lane = lane;
    io.out = dst + out_off;
    io.win = k ? resolved + (uint64_t)(k - 1u) * kGzrWindow : win0;
    io.limit = (uint32_t)n_out;
    io.pend_n = 0; io.pend_o = 0; io.mine = 0;
    io.load((uint32_t)(at >> 3));
    GzrChunkRec rec;
    gzr_decode_chunk(io, &lds[wave].T, at, n_bytes, valid, [&](uint64_t b) -> bool { return b == end_bit; }, &rec);
    io.flush();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const uint32_t crc = wave_crc32(io.out, (uint32_t)n_out, lane, crc_table);
    if (lane == 0u) {
        emit[2u * k] = crc;
        emit[2u * k + 1u] = rec.status == kGzrStopError ? (uint32_t)rec.kind : (rec.n_out == n_out && rec.end_bit == end_bit ? 0u : (uint32_t)SFGPU_BGZF_SIZE_MISMATCH);
    }
}

// the window the next call starts from
__global__ void k_gzrd_carry(const uint8_t* __restrict__ old_win, const uint8_t* __restrict__ dst, uint64_t n_out, uint8_t* __restrict__ new_win) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= kGzrWindow) return;
    new_win[j] = (uint8_t)gzr_carry([&](uint32_t i) -> uint32_t { return old_win[i]; }, [&](uint64_t i) -> uint32_t { return dst[i]; }, n_out, j);
}

const char* kind_text(int kind) {
    switch (kind) {
        case SFGPU_BGZF_BAD_HEADER: return "not a gzip member header (magic, CM = 8, reserved flags)";
        case SFGPU_BGZF_TRUNCATED: return "the file ends inside a member";
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

struct sfgpu_gzrd {
    uint32_t chunk_bytes = kGzrDefaultChunk;
    GzrState st{};
    DevBuf<uint8_t> win[2];               // the carried window: win[cur]
    int cur = 0;
    // the plan, and the device scratch it leaves for the emit
    bool planned = false;
    uint64_t n_bytes = 0;
    GzrStart start{};
    GzrChain chain;
    std::vector<uint64_t> cand;
    std::vector<GzrChunkRec> rec;
    uint32_t crc_stored = 0, isize = 0;
    sfgpu_gzrd_result res{};
    DevBuf<uint4> comp;
    DevBuf<uint64_t> d_cand, d_chain;
    DevBuf<GzrChunkRec> d_rec;
    DevBuf<uint16_t> rings;
    DevBuf<uint8_t> resolved;
    DevBuf<uint32_t> d_emit;
};

static int result_rc(const sfgpu_gzrd_result* res, const char* who) {
    if (res->error_kind == SFGPU_BGZF_OK) return SFGPU_OK;
    set_error("%s: byte %llu of this input: %s", who, (unsigned long long)res->error_offset, kind_text(res->error_kind));
    return SFGPU_ERR_FORMAT;
}

extern "C" int sfgpu_gzrd_open(sfgpu_gzrd** out, uint32_t chunk_bytes) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_gzrd_open: null handle");
    SF_REQUIRE(chunk_bytes == 0 || chunk_bytes >= 64, SFGPU_ERR_RANGE, "sfgpu_gzrd_open: chunk_bytes below 64");
    sfgpu_gzrd* z = new sfgpu_gzrd;
    if (chunk_bytes) z->chunk_bytes = chunk_bytes;
    for (auto& w : z->win) {
        if (int r = w.reserve(kGzrWindow, nullptr, false)) { delete z; return r; }
        if (hipMemsetAsync(w.p, 0, kGzrWindow, nullptr) != hipSuccess) { delete z; set_error("sfgpu_gzrd_open: hipMemsetAsync failed"); return SFGPU_ERR_HIP; }
    }
    if (hipStreamSynchronize(nullptr) != hipSuccess) { delete z; set_error("sfgpu_gzrd_open: no device"); return SFGPU_ERR_HIP; }
    *out = z;
    return SFGPU_OK;
}

extern "C" int sfgpu_gzrd_close(sfgpu_gzrd* z) {
    if (!z) return SFGPU_OK;
    (void)hipDeviceSynchronize();
    delete z;
    return SFGPU_OK;
}

extern "C" int sfgpu_gzrd_plan_host(sfgpu_gzrd* z, const void* h_src, uint64_t n_bytes, int final, uint64_t cap_bytes, sfgpu_gzrd_result* res,
                                    sfgpu_stream stream) {
    SF_REQUIRE(z && res, SFGPU_ERR_INVALID, "sfgpu_gzrd_plan_host: null handle or result");
    memset(res, 0, sizeof(*res));
    res->error_offset = ~0ull;
    SF_REQUIRE(n_bytes <= kMaxBytes, SFGPU_ERR_RANGE, "sfgpu_gzrd_plan_host: more than 2^30 bytes in one call");
    SF_REQUIRE(n_bytes == 0 || h_src, SFGPU_ERR_INVALID, "sfgpu_gzrd_plan_host: null input");
    const uint8_t* src = static_cast<const uint8_t*>(h_src);
    hipStream_t st = as_stream(stream);
    z->planned = false;                                  // a plan that leaves early (range, allocation, HIP) is no plan
    z->chain = GzrChain();
    z->n_bytes = n_bytes;
    z->start = gzr_call_start(z->st, src, n_bytes, final ? 1 : 0);
    auto leave = [&]() -> int { z->res = *res; z->planned = true; return result_rc(res, "gzip"); };
    if (z->start.kind != SFGPU_BGZF_OK) { res->error_kind = z->start.kind; res->error_offset = z->start.at; return leave(); }
    res->consumed = z->start.at;
    if (!z->start.decode) return leave();

    const uint64_t start_bit = z->start.start_bit, start_byte = start_bit >> 3;
    const uint64_t n_spans = n_bytes > start_byte ? (n_bytes - start_byte + z->chunk_bytes - 1) / z->chunk_bytes : 1;
    SF_REQUIRE(n_spans <= kMaxSpans, SFGPU_ERR_RANGE, "sfgpu_gzrd_plan_host: more than 65536 spans of chunk_bytes in one call");
    const uint64_t n_sub = (n_bytes + kSubBytes - 1) / kSubBytes;
    CallScope scope;        // the handle owns the device scratch: the scope drains both streams before this call returns
    hipStream_t cs = nullptr;
    uint8_t* pinned[2] = {nullptr, nullptr};
    uint8_t* h_back = nullptr;
    uint64_t* h_chain = nullptr;
    hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
    hipEvent_t ev_ready = nullptr, ev_f0 = nullptr, ev_f1 = nullptr, ev_a1 = nullptr, ev_p0 = nullptr, ev_p1 = nullptr;
    bool in_flight[2] = {false, false};
    auto collect = [&](int slot) {
        if (!in_flight[slot]) return;
        (void)hipEventSynchronize(ev_copied[slot]);
        add_elapsed(&res->ms_copy, ev_h2d[slot], ev_copied[slot]);
        in_flight[slot] = false;
    };
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.acquire(&cs));
    for (int b = 0; b < 2 && (uint64_t)b < n_sub; ++b) {
        SF_HIP(scope.pinned_block(&pinned[b], n_bytes < kSubBytes ? n_bytes : kSubBytes));
        SF_HIP(scope.event(&ev_h2d[b]));
        SF_HIP(scope.event(&ev_copied[b]));
    }
    for (hipEvent_t* e : {&ev_ready, &ev_f0, &ev_f1, &ev_a1, &ev_p0, &ev_p1}) SF_HIP(scope.event(e));
    const uint64_t back_bytes = n_spans * (sizeof(uint64_t) + sizeof(GzrChunkRec));
    SF_HIP(scope.pinned_block(&h_back, back_bytes));
    if (int r = z->comp.reserve((n_bytes + kSrcPad + 15) / 16, st, false)) return r;
    if (int r = z->d_cand.reserve(n_spans, st, false)) return r;
    if (int r = z->d_rec.reserve(n_spans, st, false)) return r;
    if (int r = z->rings.reserve(n_spans * kGzrWindow, st, false)) return r;
    uint8_t* comp = reinterpret_cast<uint8_t*>(z->comp.p);
    SF_HIP(hipMemsetAsync(comp + (n_bytes & ~15ull), 0, ((n_bytes + kSrcPad + 15) / 16) * 16 - (n_bytes & ~15ull), st));
    SF_HIP(hipEventRecord(ev_ready, st));
    SF_HIP(hipStreamWaitEvent(cs, ev_ready, 0));         // the copies stay behind whatever `stream` held and behind the reservations
    for (uint64_t c = 0; c < n_sub; ++c) {
        const int slot = (int)(c & 1);
        collect(slot);                                   // its previous copy has left the pinned buffer
        const uint64_t p = c * kSubBytes, q = (c + 1 == n_sub) ? n_bytes : p + kSubBytes;
        memcpy(pinned[slot], src + p, q - p);
        SF_HIP(hipEventRecord(ev_h2d[slot], cs));
        SF_HIP(hipMemcpyAsync(comp + p, pinned[slot], q - p, hipMemcpyHostToDevice, cs));
        SF_HIP(hipEventRecord(ev_copied[slot], cs));
        in_flight[slot] = true;
        if (c + 1 == n_sub) SF_HIP(hipStreamWaitEvent(st, ev_copied[slot], 0));
    }

    // ---- the finder and pass A
    const dim3 grid((unsigned)((n_spans + kWaves - 1) / kWaves)), block(kWaves * kWave);
    SF_HIP(hipEventRecord(ev_f0, st));
    hipLaunchKernelGGL(k_gzrd_find, grid, block, 0, st, z->comp.p, (uint32_t)n_bytes, start_byte, z->chunk_bytes, (uint32_t)n_spans, z->d_cand.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipEventRecord(ev_f1, st));
    hipLaunchKernelGGL(k_gzrd_pass_a, grid, block, 0, st, z->comp.p, (uint32_t)n_bytes, start_bit, z->chunk_bytes, (uint32_t)n_spans, z->d_cand.p,
                       z->rings.p, z->d_rec.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipEventRecord(ev_a1, st));
    SF_HIP(hipMemcpyAsync(h_back, z->d_cand.p, n_spans * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(h_back + n_spans * sizeof(uint64_t), z->d_rec.p, n_spans * sizeof(GzrChunkRec), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    collect(0); collect(1);
    add_elapsed(&res->ms_find, ev_f0, ev_f1);
    add_elapsed(&res->ms_decode, ev_f1, ev_a1);
    z->cand.assign(reinterpret_cast<const uint64_t*>(h_back), reinterpret_cast<const uint64_t*>(h_back) + n_spans);
    z->rec.assign(reinterpret_cast<const GzrChunkRec*>(h_back + n_spans * sizeof(uint64_t)),
                  reinterpret_cast<const GzrChunkRec*>(h_back + n_spans * sizeof(uint64_t)) + n_spans);
    for (uint64_t s = 1; s < n_spans; ++s) res->n_candidates += z->cand[s] != kGzrNone;

    // ---- the chain
    z->chain = gzr_chain(z->cand.data(), z->rec.data(), n_spans, start_bit, z->chunk_bytes, final ? 1 : 0, cap_bytes);
    const GzrChain& c = z->chain;
    const uint64_t K = c.span.size();
    res->consumed = gzr_consumed(z->start, c);
    res->n_bytes_out = c.n_out; res->n_chunks = K; res->n_false_starts = c.n_false;
    res->n_stored_blocks = c.blocks[0]; res->n_fixed_blocks = c.blocks[1]; res->n_dynamic_blocks = c.blocks[2];
    res->need_cap = c.need_cap; res->member_end = c.member_end;
    if (c.error_kind != SFGPU_BGZF_OK) { res->error_kind = c.error_kind; res->error_offset = c.error_bit >> 3; }
    if (c.member_end) {
        auto byte = [&](uint64_t p) -> uint32_t { return src[p]; };
        z->crc_stored = bgz_le32(byte, c.end_bit >> 3); z->isize = bgz_le32(byte, (c.end_bit >> 3) + 4);
    }

    // ---- what the kernels behind the chain read, and the propagation
    if (K) {
        SF_HIP(scope.pinned_block(&h_chain, 6 * K * sizeof(uint64_t)));
        if (int r = z->d_chain.reserve(6 * K, st, false)) return r;
        if (int r = z->resolved.reserve((K > 1 ? K - 1 : 1) * kGzrWindow, st, false)) return r;
        const uint64_t valid0 = z->start.begins_member ? 0u : z->st.valid;
        for (uint64_t k = 0; k < K; ++k) {
            const GzrChunkRec& r = z->rec[c.span[k]];
            h_chain[k] = c.span[k]; h_chain[K + k] = r.n_out;
            h_chain[2 * K + k] = k ? z->cand[c.span[k]] : start_bit; h_chain[3 * K + k] = r.end_bit;
            h_chain[4 * K + k] = c.out_off[k];
            h_chain[5 * K + k] = valid0 + c.out_off[k] < kGzrWindow ? valid0 + c.out_off[k] : kGzrWindow;
        }
        SF_HIP(hipMemcpyAsync(z->d_chain.p, h_chain, 6 * K * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        SF_HIP(hipEventRecord(ev_p0, st));
        if (K > 1) {
            hipLaunchKernelGGL(k_gzrd_propagate, dim3(1), dim3(kPropThreads), 0, st, z->rings.p, z->d_chain.p, (uint32_t)K, z->win[z->cur].p, z->resolved.p);
            SF_HIP(hipGetLastError());
        }
        SF_HIP(hipEventRecord(ev_p1, st));
        SF_HIP(hipStreamSynchronize(st));
        add_elapsed(&res->ms_propagate, ev_p0, ev_p1);
    }
    return leave();
}

extern "C" int sfgpu_gzrd_emit(sfgpu_gzrd* z, uint8_t* d_dst, sfgpu_gzrd_result* res, sfgpu_stream stream) {
    SF_REQUIRE(z && res, SFGPU_ERR_INVALID, "sfgpu_gzrd_emit: null handle or result");
    SF_REQUIRE(z->planned, SFGPU_ERR_STATE, "sfgpu_gzrd_emit: no plan");
    z->planned = false;
    *res = z->res;
    const GzrChain& c = z->chain;
    const uint64_t K = c.span.size();
    if (K == 0) return result_rc(res, "gzip");
    SF_REQUIRE(d_dst || c.n_out == 0, SFGPU_ERR_INVALID, "sfgpu_gzrd_emit: null output");
    hipStream_t st = as_stream(stream);
    CallScope scope;
    uint32_t* h_emit = nullptr;
    hipEvent_t ev_b0 = nullptr, ev_b1 = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_b0));
    SF_HIP(scope.event(&ev_b1));
    SF_HIP(scope.pinned_block(&h_emit, 2 * K * sizeof(uint32_t)));
    if (int r = z->d_emit.reserve(2 * K, st, false)) return r;
    SF_HIP(hipEventRecord(ev_b0, st));
    hipLaunchKernelGGL(k_gzrd_pass_b, dim3((unsigned)((K + kWaves - 1) / kWaves)), dim3(kWaves * kWave), 0, st, z->comp.p, (uint32_t)z->n_bytes,
                       z->d_chain.p, (uint32_t)K, z->win[z->cur].p, z->resolved.p, d_dst, z->d_emit.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipEventRecord(ev_b1, st));
    hipLaunchKernelGGL(k_gzrd_carry, dim3(kGzrWindow / 256), dim3(256), 0, st, z->win[z->cur].p, d_dst, c.n_out, z->win[1 - z->cur].p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(h_emit, z->d_emit.p, 2 * K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_emit, ev_b0, ev_b1);
    std::vector<uint32_t> crcs(K);
    for (uint64_t k = 0; k < K; ++k) {
        crcs[k] = h_emit[2 * k];
        if (h_emit[2 * k + 1] != 0u) {                   // the first chunk in stream order that pass B could not decode
            res->error_kind = (int32_t)h_emit[2 * k + 1];
            res->error_offset = (k ? z->cand[c.span[k]] : z->start.start_bit) >> 3;
            return result_rc(res, "gzip");
        }
    }
    z->cur = 1 - z->cur;
    const int kind = gzr_finish_call(&z->st, z->start, c, z->rec.data(), crcs.data(), z->crc_stored, z->isize);
    if (kind != SFGPU_BGZF_OK) {
        res->error_kind = kind;
        res->error_offset = (K > 1 ? z->cand[c.span[K - 1]] : z->start.start_bit) >> 3;
    }
    return result_rc(res, "gzip");
}
