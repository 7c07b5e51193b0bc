// bamfront.h -- the front end the BAM readers share (bamtext.hip: name-grouped files; samcollate.hip: the collated reading): from
// the inflated record stream on the device to the record starts of a call, in order, and "one SamLine per record", kept packed.
// What the stream says is bamfmt.h's.
//
// A record's start is known only from the block_size of the record in front of it.  That chain is resolved exactly, from the known
// start behind the header, and in parallel: nobody guesses what looks like a record, and no lane follows more dependent links than
// the few bounds below allow, however many records the call holds.  The text is taken in spans of at most 2^26 bytes; per span:
//   k_bam_tile      one workgroup per tile of kTile bytes: the tile (+ 3 bytes) in LDS, nxt[p] for EVERY byte position p (most
//                   of them are no record start; that is not known yet), bam_tile_rounds pointer doublings between two LDS
//                   arrays, exit[p] -- where the chain that begins at p leaves the tile -- written as one uint32 per text byte
//   k_bam_super     per supertile of kSuper tiles and per entry offset into its first tile: at most kSuper hops through exit[]
//   k_bam_walk      one lane: the supertiles of the span in order, one lookup each (span bytes / (kSuper kTile) dependent loads);
//                   a record longer than a tile that crosses a supertile's edge enters behind its first tile and costs that
//                   supertile at most kSuper hops more.  The value it ends with is the entry of the next span.
//   k_bam_entries   one lane per supertile: the entry of each of its tiles, kSuper hops
//   k_bam_enum      per tile, from its entry: its record starts (at most kTile / 36 hops in LDS), their count
//   scan, k_bam_compact   rec_off[]: the record starts of the call in order.  The chain's last value says how it ended.
// No workgroup waits for another: every stage is a launch of its own.  Then
//   k_bam_records   one lane per record: bam_parse_record (FLAG, pos, the CIGAR words, ref_tid[refID], the lengths); the lowest
//                   malformed record is a 64-bit min, the key of k_sam_lines
#pragma once
#include "bamfmt.h"
#include "common.h"
#include "primitives.h"
#include "samback.h"

namespace sfgpu {
namespace bamfront {

using namespace samback;

constexpr uint32_t kTile = 4096;                         // bytes: text 4 KB + two pointer arrays 32 KB of LDS, four workgroups per CU
constexpr uint32_t kSuper = 64;                          // tiles per supertile
constexpr uint32_t kSuperBytes = kSuper * kTile;
constexpr uint64_t kSpanBytes = 1ull << 26;              // the exit table: 4 bytes per text byte, 256 MB
constexpr uint32_t kTileRecs = bam_tile_records<kTile>();
constexpr uint32_t kNoEntry = 0xffffffffu;               // (a chain value that has ended)
constexpr int kEnumBlock = 64;
constexpr uint64_t kMaxBytes = 1ull << 30;               // one parse call
constexpr unsigned long long kNoBad = ~0ull;
static_assert(kTile % 16 == 0 && kSpanBytes % kSuperBytes == 0 && kTile % kBlock == 0, "tiles are whole 16-byte groups, spans whole supertiles");

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

struct Bytes {
    const unsigned char* p;
    __device__ unsigned char operator()(uint32_t i) const { return p[i]; }
};
// the tile [base, base + kTile + 16) of the text in LDS
struct TileBytes {
    const unsigned char* lds;
    uint32_t base;
    __device__ unsigned char operator()(uint32_t i) const { return lds[i - base]; }
};
struct ExitTable {
    const uint32_t* exit;         // exit[p - span0]
    uint32_t span0;
    __device__ uint32_t operator()(uint32_t p) const { return exit[p - span0]; }
};

// the 16-byte groups of the tile at `base` (a multiple of 16; the text's buffer holds whole groups) that begin below n, and zeros
template <int kThreads>
__device__ inline void load_tile(const unsigned char* __restrict__ bytes, uint32_t base, uint32_t n, unsigned char* lds) {
    for (uint32_t g = threadIdx.x; g < kTile / 16 + 1; g += kThreads) {
        const uint64_t p = (uint64_t)base + 16ull * g;
        reinterpret_cast<uint4*>(lds)[g] = p < n ? *reinterpret_cast<const uint4*>(bytes + p) : make_uint4(0, 0, 0, 0);
    }
}

// ---- the chain ------------------------------------------------------------------------------------------------------------

[[maybe_unused]] static __global__ void __launch_bounds__(kBlock) k_bam_tile(const unsigned char* __restrict__ bytes, uint32_t span0, uint32_t n, uint32_t* __restrict__ exit_tab) {
    __shared__ __attribute__((aligned(16))) unsigned char text[kTile + 16];
    __shared__ uint32_t ptr[2][kTile];
    const uint32_t base = span0 + blockIdx.x * kTile;
    load_tile<kBlock>(bytes, base, n, text);
    __syncthreads();
    const TileBytes get{text, base};
    for (uint32_t i = threadIdx.x; i < kTile; i += kBlock) ptr[0][i] = bam_tile_nxt<kTile>(get, base, i, n);
    __syncthreads();
    int cur = 0;
    for (uint32_t r = 0; r < bam_tile_rounds<kTile>(); ++r, cur ^= 1) {
        for (uint32_t i = threadIdx.x; i < kTile; i += kBlock) ptr[cur ^ 1][i] = bam_tile_double<kTile>(ptr[cur], base, i);
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < kTile && base + i < n; i += kBlock) exit_tab[base - span0 + i] = ptr[cur][i];
}

// super_exit[s * kTile + o] = where the chain that begins at offset o of supertile s leaves it (grid: kTile / kBlock x supertiles)
[[maybe_unused]] static __global__ void __launch_bounds__(kBlock) k_bam_super(ExitTable exit_at, uint32_t span_end, uint32_t n, uint32_t* __restrict__ super_exit) {
    const uint32_t s = blockIdx.y, o = blockIdx.x * kBlock + threadIdx.x;
    const uint64_t sbase = (uint64_t)exit_at.span0 + (uint64_t)s * kSuperBytes;
    if (sbase + o >= span_end) return;
    const uint32_t send = sbase + kSuperBytes < span_end ? (uint32_t)(sbase + kSuperBytes) : span_end;
    super_exit[(uint64_t)s * kTile + o] = bam_follow(exit_at, (uint32_t)(sbase + o), send, n);
}

// One lane.  chain[0]: the value that enters the span, then the one that leaves it; super_entry[s] = the value that enters supertile s.
[[maybe_unused]] static __global__ void k_bam_walk(ExitTable exit_at, uint32_t span_end, uint32_t n, uint32_t n_super, const uint32_t* __restrict__ super_exit,
                           uint32_t* __restrict__ super_entry, uint32_t* __restrict__ chain) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t v = chain[0];
    for (uint32_t s = 0; s < n_super; ++s) {
        const uint64_t sbase = (uint64_t)exit_at.span0 + (uint64_t)s * kSuperBytes;
        const uint32_t send = sbase + kSuperBytes < span_end ? (uint32_t)(sbase + kSuperBytes) : span_end;
        super_entry[s] = v;
        if (bam_ended(v) || v >= send) continue;
        v = v - sbase < kTile ? super_exit[(uint64_t)s * kTile + (v - (uint32_t)sbase)] : bam_follow(exit_at, v, send, n);
    }
    chain[0] = v;
}

// one lane per supertile: tile_entry[t] = the chain value that enters tile t, or kNoEntry when the chain has no position in it
[[maybe_unused]] static __global__ void __launch_bounds__(kBlock) k_bam_entries(ExitTable exit_at, uint32_t span_end, uint32_t n_super, uint32_t n_tiles,
                                                        const uint32_t* __restrict__ super_entry, uint32_t* __restrict__ tile_entry) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_super) return;
    uint32_t v = super_entry[s];
    for (uint32_t t = s * kSuper; t < (s + 1) * kSuper && t < n_tiles; ++t) {
        const uint64_t tbase = (uint64_t)exit_at.span0 + (uint64_t)t * kTile;
        const bool in = !bam_ended(v) && v >= tbase && v < tbase + kTile && v < span_end;
        tile_entry[t] = in ? v : kNoEntry;
        if (in) v = exit_at(v);
    }
}

// starts[t * kTileRecs + i] = record start i of tile t, count[t] of them
[[maybe_unused]] static __global__ void __launch_bounds__(kEnumBlock) k_bam_enum(const unsigned char* __restrict__ bytes, uint32_t span0, uint32_t n,
                                                         const uint32_t* __restrict__ tile_entry, uint32_t* __restrict__ starts,
                                                         uint32_t* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) unsigned char text[kTile + 16];
    __shared__ uint32_t list[kTileRecs];
    __shared__ uint32_t n_list;
    const uint32_t t = blockIdx.x, base = span0 + t * kTile, entry = tile_entry[t];
    if (entry == kNoEntry) {                              // (the same for every lane)
        if (threadIdx.x == 0) count[t] = 0;
        return;
    }
    load_tile<kEnumBlock>(bytes, base, n, text);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t leave;
        n_list = bam_tile_starts<kTile>(TileBytes{text, base}, base, entry, n, list, &leave);
        count[t] = n_list;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_list; i += kEnumBlock) starts[(uint64_t)t * kTileRecs + i] = list[i];
}

[[maybe_unused]] static __global__ void __launch_bounds__(kEnumBlock) k_bam_compact(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ count,
                                                            const uint32_t* __restrict__ count_scan, uint32_t* __restrict__ rec_off) {
    const uint32_t t = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < count[t]; i += kEnumBlock) rec_off[count_scan[t] + i] = starts[(uint64_t)t * kTileRecs + i];
}

// ---- the records ----------------------------------------------------------------------------------------------------------

// One lane per record.  No lane leaves before the shuffles.
[[maybe_unused]] static __global__ void __launch_bounds__(kBlock) k_bam_records(const unsigned char* __restrict__ bytes, uint32_t K, const uint32_t* __restrict__ rec_off, int paired,
                                                        uint32_t n_ref, const uint32_t* __restrict__ ref_tid, uint32_t* __restrict__ info,
                                                        uint32_t* __restrict__ tid, int32_t* __restrict__ pos, uint32_t* __restrict__ name_len,
                                                        uint32_t* __restrict__ rec_line, unsigned long long* __restrict__ first_bad) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = kNoBad;
    if (k < K) {
        const SamLine l = bam_parse_record(Bytes{bytes}, rec_off[k], paired != 0, n_ref, [&](uint32_t r) { return ref_tid[r]; });
        info[k] = pack_line(l); tid[k] = l.tid; pos[k] = l.pos; name_len[k] = l.q_len; rec_line[k] = k;
        if (l.bad) key = ((unsigned long long)k << 8) | l.bad;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other < key ? other : key;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && key != kNoBad) atomicMin(first_bad, key);
}

// the scratch of the chain, and what it leaves: rec_off
struct Chain {
    DevBuf<uint32_t> exit_tab, super_exit, super_entry, tile_entry, starts, count, count_scan, chain, rec_off;
};

}  // namespace bamfront
}  // namespace sfgpu

// the handle of sfgpu_bam_open
struct sfgpu_bam {
    sfgpu_sam* names = nullptr;                   // the transcript names' table
    uint32_t n_ref = 0;
    uint64_t header_bytes = 0, stream_pos = 0;    // stream_pos: the sum of the `consumed` values returned so far
    sfgpu::DevBuf<uint32_t> ref_tid;
};

namespace sfgpu {
namespace bamfront {

// The record starts of bytes[skip, n) in order: S.rec_off[0 .. *K); *last = the chain value behind them (n: the chain ended well).
// h32: 8 pinned words.
inline int resolve_chain(Chain& S, const unsigned char* bytes, uint32_t skip, uint32_t n, uint32_t* K, uint32_t* last, hipStream_t st, uint32_t* h32) {
    *K = 0; *last = skip;
    if (skip >= n) return SFGPU_OK;
    const uint64_t first_span = skip / kSpanBytes * kSpanBytes;
    const uint64_t max_span = n - first_span < kSpanBytes ? n - first_span : kSpanBytes;
    const uint64_t max_tiles = (max_span + kTile - 1) / kTile, max_super = (max_tiles + kSuper - 1) / kSuper;
    if (int r = S.exit_tab.reserve(max_span, st, false)) return r;
    if (int r = S.super_exit.reserve(max_super * kTile, st, false)) return r;
    if (int r = S.super_entry.reserve(max_super, st, false)) return r;
    for (DevBuf<uint32_t>* b : {&S.tile_entry, &S.count, &S.count_scan}) if (int r = b->reserve(max_tiles + 2, st, false)) return r;
    if (int r = S.starts.reserve(max_tiles * kTileRecs, st, false)) return r;
    if (int r = S.chain.reserve(1, st, false)) return r;
    if (int r = S.rec_off.reserve((uint64_t)(n - skip) / kBamMin + 2, st, false)) return r;
    h32[4] = skip;
    SF_HIP(hipMemcpyAsync(S.chain.p, &h32[4], 4, hipMemcpyHostToDevice, st));
    for (uint64_t span0 = first_span; span0 < n && !bam_ended(*last); span0 += kSpanBytes) {
        const uint32_t span_end = (uint32_t)(span0 + kSpanBytes < n ? span0 + kSpanBytes : n);
        if (*last >= span_end) continue;                  // (a record longer than a span)
        const uint32_t n_tiles = (uint32_t)((span_end - span0 + kTile - 1) / kTile), n_super = (n_tiles + kSuper - 1) / kSuper;
        const ExitTable exit_at{S.exit_tab.p, (uint32_t)span0};
        hipLaunchKernelGGL(k_bam_tile, dim3(n_tiles), dim3(kBlock), 0, st, bytes, (uint32_t)span0, n, S.exit_tab.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_bam_super, dim3(kTile / kBlock, n_super), dim3(kBlock), 0, st, exit_at, span_end, n, S.super_exit.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_bam_walk, dim3(1), dim3(kWave), 0, st, exit_at, span_end, n, n_super, S.super_exit.p, S.super_entry.p, S.chain.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_bam_entries, dim3(grid_of(n_super)), dim3(kBlock), 0, st, exit_at, span_end, n_super, n_tiles, S.super_entry.p, S.tile_entry.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_bam_enum, dim3(n_tiles), dim3(kEnumBlock), 0, st, bytes, (uint32_t)span0, n, S.tile_entry.p, S.starts.p, S.count.p);
        SF_CHECK_LAUNCH();
        if (int r = exclusive_scan_u32_u32(S.count.p, S.count_scan.p, n_tiles, st)) return r;
        hipLaunchKernelGGL(k_bam_compact, dim3(n_tiles), dim3(kEnumBlock), 0, st, S.starts.p, S.count.p, S.count_scan.p, S.rec_off.p + *K);
        SF_CHECK_LAUNCH();
        SF_HIP(hipMemcpyAsync(&h32[0], S.count_scan.p + n_tiles, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(&h32[1], S.chain.p, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        *K += h32[0];
        *last = h32[1];
    }
    return SFGPU_OK;
}

}  // namespace bamfront
}  // namespace sfgpu
