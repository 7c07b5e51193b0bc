// bamtext.hip -- a mapper's BAM record stream (the bytes behind the BGZF inflate) turned into sfgpu_hit records and read offsets on
// the device: sfgpu_bam_*.  What the stream says is bamfmt.h; the back end (pairs, survivors, the stable sort, the records) is
// samback.h, the kernels samtext.hip runs.  This file is the front end: where the records begin.
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
//   k_bam_heads     record k begins a group when its name differs from record k - 1's
// and samback.h, with rec_line = the identity.
#include "bamfmt.h"
#include "common.h"
#include "primitives.h"
#include "samback.h"

namespace sfgpu {
namespace {

using namespace samback;

constexpr uint32_t kTile = 4096;                         // bytes: text 4 KB + two pointer arrays 32 KB of LDS, four workgroups per CU
constexpr uint32_t kSuper = 64;                          // tiles per supertile
constexpr uint32_t kSuperBytes = kSuper * kTile;
constexpr uint64_t kSpanBytes = 1ull << 26;              // the exit table: 4 bytes per text byte, 256 MB
constexpr uint32_t kTileRecs = bam_tile_records<kTile>();
constexpr uint32_t kNoEntry = 0xffffffffu;               // (a chain value that has ended)
constexpr int kEnumBlock = 64;
constexpr uint64_t kSubBytes = 4ull << 20;               // staged sub-chunk (a multiple of 16)
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

__global__ void __launch_bounds__(kBlock) k_bam_tile(const unsigned char* __restrict__ bytes, uint32_t span0, uint32_t n, uint32_t* __restrict__ exit_tab) {
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
__global__ void __launch_bounds__(kBlock) k_bam_super(ExitTable exit_at, uint32_t span_end, uint32_t n, uint32_t* __restrict__ super_exit) {
    const uint32_t s = blockIdx.y, o = blockIdx.x * kBlock + threadIdx.x;
    const uint64_t sbase = (uint64_t)exit_at.span0 + (uint64_t)s * kSuperBytes;
    if (sbase + o >= span_end) return;
    const uint32_t send = sbase + kSuperBytes < span_end ? (uint32_t)(sbase + kSuperBytes) : span_end;
    super_exit[(uint64_t)s * kTile + o] = bam_follow(exit_at, (uint32_t)(sbase + o), send, n);
}

// One lane.  chain[0]: the value that enters the span, then the one that leaves it; super_entry[s] = the value that enters supertile s.
__global__ void k_bam_walk(ExitTable exit_at, uint32_t span_end, uint32_t n, uint32_t n_super, const uint32_t* __restrict__ super_exit,
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
__global__ void __launch_bounds__(kBlock) k_bam_entries(ExitTable exit_at, uint32_t span_end, uint32_t n_super, uint32_t n_tiles,
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
__global__ void __launch_bounds__(kEnumBlock) k_bam_enum(const unsigned char* __restrict__ bytes, uint32_t span0, uint32_t n,
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

__global__ void __launch_bounds__(kEnumBlock) k_bam_compact(const uint32_t* __restrict__ starts, const uint32_t* __restrict__ count,
                                                            const uint32_t* __restrict__ count_scan, uint32_t* __restrict__ rec_off) {
    const uint32_t t = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < count[t]; i += kEnumBlock) rec_off[count_scan[t] + i] = starts[(uint64_t)t * kTileRecs + i];
}

// ---- the records ----------------------------------------------------------------------------------------------------------

// ref_tid[r] = the transcript that reference r names, kSamNone when none does
__global__ void k_bam_refs(const unsigned char* __restrict__ ref_blob, const uint64_t* __restrict__ ref_off, uint32_t n_ref, NameTable T,
                           uint32_t* __restrict__ ref_tid, uint32_t* __restrict__ flag) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_ref) return;
    if (ref_off[r + 1] < ref_off[r] || ref_off[r + 1] - ref_off[r] > 0xfffffffeull) { atomicOr(flag, 2u); ref_tid[r] = kSamNone; return; }
    ref_tid[r] = T.find(ref_blob + ref_off[r], (uint32_t)(ref_off[r + 1] - ref_off[r]));
}

// One lane per record.  No lane leaves before the shuffles.
__global__ void __launch_bounds__(kBlock) k_bam_records(const unsigned char* __restrict__ bytes, uint32_t K, const uint32_t* __restrict__ rec_off, int paired,
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

// head[k] = record k's name differs from record k - 1's
__global__ void k_bam_heads(const unsigned char* __restrict__ bytes, uint32_t K, const uint32_t* __restrict__ rec_off, const uint32_t* __restrict__ name_len,
                            uint32_t* __restrict__ head) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    if (k == 0) { head[0] = 1; return; }
    const uint32_t n = name_len[k], a = rec_off[k] + kBamMin, b = rec_off[k - 1] + kBamMin;
    bool same = name_len[k - 1] == n;
    for (uint32_t i = 0; same && i < n; ++i) same = bytes[a + i] == bytes[b + i];
    head[k] = same ? 0u : 1u;
}

// the last head: cut[0] = its record, cut[1] = where that record begins
__global__ void k_bam_cut(uint32_t K, const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_scan, const uint32_t* __restrict__ rec_off,
                          uint32_t* __restrict__ cut) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K || !head[k] || head_scan[k] + 1 != head_scan[K]) return;
    cut[0] = k; cut[1] = rec_off[k];
}

struct Scratch {
    DevBuf<uint4> text;
    DevBuf<uint32_t> exit_tab, super_exit, super_entry, tile_entry, starts, count, count_scan, chain, rec_off, info, tid, name_len, rec_line, head,
        head_scan, pair_head, has_pair, surv, surv_scan, val, val2, cut;
    DevBuf<int32_t> pos;
    DevBuf<uint64_t> key, key2;
    DevBuf<unsigned long long> word;              // [0] the lowest malformed record, [1] the pairs
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

struct sfgpu_bam {
    sfgpu_sam* names = nullptr;                   // the transcript names' table
    uint32_t n_ref = 0;
    uint64_t header_bytes = 0, stream_pos = 0;    // stream_pos: the sum of the `consumed` values returned so far
    DevBuf<uint32_t> ref_tid;
};

namespace {

// The record starts of bytes[skip, n) in order: S.rec_off[0 .. *K); *last = the chain value behind them (n: the chain ended well).
// h32: 8 pinned words.
int resolve_chain(Scratch& S, const unsigned char* bytes, uint32_t skip, uint32_t n, uint32_t* K, uint32_t* last, hipStream_t st, uint32_t* h32) {
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

// The text on the device: bytes[0, n) in a buffer of whole 16-byte groups.  h: 8 pinned 64-bit words.
int parse_device_text(sfgpu_bam* m, Scratch& S, const unsigned char* bytes, uint64_t n, bool final, sfgpu_hit* d_hits, uint64_t cap_hits, uint32_t* d_off,
                      uint64_t cap_reads, sfgpu_sam_result* res, hipStream_t st, uint64_t* h) {
    uint32_t* h32 = reinterpret_cast<uint32_t*>(h);
    const uint64_t skip = m->header_bytes > m->stream_pos ? m->header_bytes - m->stream_pos : 0;
    if (skip > n) {                                       // the header goes on: present more
        if (final) { res->consumed = n; m->stream_pos += n; }
        return SFGPU_OK;
    }
    uint32_t K = 0, last = 0;
    if (int r = resolve_chain(S, bytes, (uint32_t)skip, (uint32_t)n, &K, &last, st, h32)) return r;
    const bool chain_bad = bam_ended(last) && (bam_broken(last) || final);     // BAD_FIELDS at record K

    // ---- the records
    if (int r = S.word.reserve(2, st, false)) return r;
    if (int r = S.cut.reserve(4, st, false)) return r;
    for (DevBuf<uint32_t>* b : {&S.info, &S.tid, &S.name_len, &S.rec_line, &S.head, &S.head_scan, &S.pair_head, &S.has_pair, &S.surv, &S.surv_scan})
        if (int r = b->reserve((uint64_t)K + 2, st, false)) return r;
    if (int r = S.pos.reserve((uint64_t)K + 2, st, false)) return r;
    h[1] = kNoBad;
    if (K) {
        SF_HIP(hipMemsetAsync(S.word.p, 0xff, 8, st));
        SF_HIP(hipMemsetAsync(S.word.p + 1, 0, 8, st));
        hipLaunchKernelGGL(k_bam_records, dim3(grid_of(K)), dim3(kBlock), 0, st, bytes, K, S.rec_off.p, m->names->paired ? 1 : 0, m->n_ref, m->ref_tid.p,
                           S.info.p, S.tid.p, S.pos.p, S.name_len.p, S.rec_line.p, S.word.p);
        SF_CHECK_LAUNCH();
        SF_HIP(hipMemcpyAsync(&h[1], S.word.p, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
    }
    if (h[1] != kNoBad || chain_bad) {
        res->bad = h[1] != kNoBad ? (uint32_t)(h[1] & 0xffu) : (uint32_t)SFGPU_SAM_BAD_FIELDS;
        res->bad_line = h[1] != kNoBad ? h[1] >> 8 : K;
        set_error("sfgpu_bam_parse: record %llu of the text is malformed (SFGPU_SAM_BAD_* %u)", (unsigned long long)res->bad_line, res->bad);
        return SFGPU_ERR_FORMAT;
    }
    if (K == 0) {
        if (final) { res->consumed = n; m->stream_pos += n; }
        return SFGPU_OK;
    }

    // ---- the groups
    hipLaunchKernelGGL(k_bam_heads, dim3(grid_of(K)), dim3(kBlock), 0, st, bytes, K, S.rec_off.p, S.name_len.p, S.head.p);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(S.head.p, S.head_scan.p, K, st)) return r;
    hipLaunchKernelGGL(k_bam_cut, dim3(grid_of(K)), dim3(kBlock), 0, st, K, S.head.p, S.head_scan.p, S.rec_off.p, S.cut.p);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(&h32[0], S.head_scan.p + K, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h32[1], S.cut.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t n_groups_seen = h32[0];
    const uint32_t Kc = final ? K : h32[1], n_reads = final ? n_groups_seen : n_groups_seen - 1;
    const uint64_t consumed = final ? n : h32[2];
    if (n_reads == 0) return SFGPU_OK;                    // one group, held back: present more

    // ---- the records of the groups: samback.h
    const Lines lines{S.info.p, S.tid.p, S.pos.p};
    SF_HIP(hipMemsetAsync(S.has_pair.p, 0, (uint64_t)n_reads * 4, st));
    if (m->names->paired) {
        hipLaunchKernelGGL(k_sam_pairs, dim3(grid_of(Kc)), dim3(kBlock), 0, st, Kc, S.rec_line.p, S.head.p, S.head_scan.p, lines, S.pair_head.p,
                           S.has_pair.p);
        SF_CHECK_LAUNCH();
    } else {
        SF_HIP(hipMemsetAsync(S.pair_head.p, 0, (uint64_t)Kc * 4, st));
    }
    hipLaunchKernelGGL(k_sam_survive, dim3(grid_of(K)), dim3(kBlock), 0, st, K, Kc, S.rec_line.p, S.head.p, S.head_scan.p, lines, S.pair_head.p,
                       S.has_pair.p, S.surv.p, S.word.p + 1);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(S.surv.p, S.surv_scan.p, K, st)) return r;
    SF_HIP(hipMemcpyAsync(&h32[0], S.surv_scan.p + K, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h[1], S.word.p + 1, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t n_hits = h32[0];
    if (n_hits > cap_hits || n_reads > cap_reads) {
        res->need_hits = n_hits; res->need_reads = n_reads;
        set_error("sfgpu_bam_parse: %u records in %u reads do not fit cap_hits = %llu, cap_reads = %llu", n_hits, n_reads,
                  (unsigned long long)cap_hits, (unsigned long long)cap_reads);
        return SFGPU_ERR_CAPACITY;
    }
    for (DevBuf<uint64_t>* b : {&S.key, &S.key2}) if (int r = b->reserve((uint64_t)n_hits + 2, st, false)) return r;
    for (DevBuf<uint32_t>* b : {&S.val, &S.val2}) if (int r = b->reserve((uint64_t)n_hits + 2, st, false)) return r;
    hipLaunchKernelGGL(k_sam_keys, dim3(grid_of(Kc)), dim3(kBlock), 0, st, Kc, S.rec_line.p, S.head.p, S.head_scan.p, lines, S.surv.p, S.surv_scan.p, d_off,
                       S.key.p, S.val.p);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(d_off + n_reads, S.surv_scan.p + K, 4, hipMemcpyDeviceToDevice, st));
    if (n_hits) {
        int group_bits = 1;
        while (group_bits < 31 && (1u << group_bits) < n_reads) ++group_bits;
        if (int r = sort_pairs_u64_u32(S.key.p, S.key2.p, S.val.p, S.val2.p, n_hits, st, 33 + group_bits, false)) return r;
        hipLaunchKernelGGL(k_sam_write, dim3(grid_of(n_hits)), dim3(kBlock), 0, st, n_hits, S.val2.p, S.rec_line.p, S.pair_head.p, lines, d_hits);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipStreamSynchronize(st));
    res->n_lines = Kc; res->n_reads = n_reads; res->n_hits = n_hits; res->n_pairs = h[1];
    res->consumed = consumed;
    m->stream_pos += consumed;
    return SFGPU_OK;
}

int check_parse_args(const char* who, sfgpu_bam* m, const void* text, uint64_t n_bytes, sfgpu_hit* d_hits, uint64_t cap_hits, uint32_t* d_off,
                     sfgpu_sam_result* res) {
    if (!m || !res) { set_error("%s: null handle or result", who); return SFGPU_ERR_INVALID; }
    memset(res, 0, sizeof(*res));
    if (n_bytes > kMaxBytes) { set_error("%s: more than 2^30 bytes in one call", who); return SFGPU_ERR_RANGE; }
    if ((n_bytes && !text) || !d_off || (cap_hits && !d_hits)) { set_error("%s: null array", who); return SFGPU_ERR_INVALID; }
    return SFGPU_OK;
}

}  // namespace

extern "C" int sfgpu_bam_close(sfgpu_bam* m) {
    if (!m) return SFGPU_OK;
    (void)sfgpu_sam_close(m->names);                      // (synchronises the device)
    delete m;
    return SFGPU_OK;
}

extern "C" int sfgpu_bam_open(sfgpu_bam** out, const char* d_names, const uint64_t* d_name_off, uint64_t M, const char* d_ref_names,
                              const uint64_t* d_ref_off, uint64_t n_ref, uint64_t header_bytes, int paired, sfgpu_stream stream) {
    SF_REQUIRE(out && d_ref_off, SFGPU_ERR_INVALID, "sfgpu_bam_open: null handle or reference offsets");
    SF_REQUIRE(n_ref < 0x7fffffffull, SFGPU_ERR_RANGE, "sfgpu_bam_open: 2^31 - 1 references or more");
    hipStream_t st = as_stream(stream);
    sfgpu_bam* m = new sfgpu_bam;
    m->n_ref = (uint32_t)n_ref;
    m->header_bytes = header_bytes;
    DevBuf<uint32_t> flag;
    auto build = [&]() -> int {
        if (int r = sfgpu_sam_open(&m->names, d_names, d_name_off, M, paired, stream)) return r;
        CallScope scope;
        uint32_t* h32 = nullptr;
        SF_HIP(scope.adopt(st));
        SF_HIP(scope.pinned_block(&h32, 4 * sizeof(uint32_t)));
        if (int r = m->ref_tid.reserve(n_ref + 1, st, false)) return r;
        if (int r = flag.reserve(1, st, false)) return r;
        SF_HIP(hipMemsetAsync(flag.p, 0, 4, st));
        if (n_ref) {
            SF_REQUIRE(d_ref_names != nullptr, SFGPU_ERR_INVALID, "sfgpu_bam_open: null reference names");
            const NameTable T{m->names->blob.p, m->names->off.p, m->names->slot.p, m->names->mask};
            hipLaunchKernelGGL(k_bam_refs, dim3(grid_of(n_ref)), dim3(kBlock), 0, st, reinterpret_cast<const unsigned char*>(d_ref_names), d_ref_off,
                               (uint32_t)n_ref, T, m->ref_tid.p, flag.p);
            SF_CHECK_LAUNCH();
        }
        SF_HIP(hipMemcpyAsync(h32, flag.p, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        SF_REQUIRE(!(h32[0] & 2u), SFGPU_ERR_INVALID, "sfgpu_bam_open: the reference offsets decrease");
        return SFGPU_OK;
    };
    const int rc = build();
    if (rc != SFGPU_OK) { (void)hipStreamSynchronize(st); (void)sfgpu_bam_close(m); return rc; }
    *out = m;
    return SFGPU_OK;
}

extern "C" int sfgpu_bam_parse_host(sfgpu_bam* m, const char* h_text, uint64_t n_bytes, int final, sfgpu_hit* d_hits, uint64_t cap_hits,
                                    uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream) {
    if (int r = check_parse_args("sfgpu_bam_parse_host", m, h_text, n_bytes, d_hits, cap_hits, d_off, res)) return r;
    hipStream_t st = as_stream(stream);
    SF_HIP(hipMemsetAsync(d_off, 0, 4, st));
    if (n_bytes == 0) { SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }
    const uint64_t n_groups = (n_bytes + 15) / 16, n_sub = (n_bytes + kSubBytes - 1) / kSubBytes;

    Scratch S;
    CallScope scope;        // after S: it drains both streams before S's blocks go back to the pool
    hipStream_t cs = nullptr;
    char* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev_slot[2] = {nullptr, nullptr}, ev_c0 = nullptr, ev_c1 = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;
    uint64_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.acquire(&cs));
    for (int b = 0; b < 2 && (uint64_t)b < n_sub; ++b) {
        SF_HIP(scope.pinned_block(&pinned[b], (n_bytes < kSubBytes ? n_bytes : kSubBytes) + 48));
        SF_HIP(scope.event(&ev_slot[b]));
    }
    for (hipEvent_t* e : {&ev_c0, &ev_c1, &ev_k0, &ev_k1}) SF_HIP(scope.event(e));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint64_t)));
    if (int r = S.text.reserve(n_groups + 1, st, false)) return r;
    SF_HIP(hipEventRecord(ev_k0, st));
    SF_HIP(hipStreamWaitEvent(cs, ev_k0, 0));                // the copies stay behind whatever `stream` held and behind the reservation
    SF_HIP(hipEventRecord(ev_c0, cs));
    for (uint64_t c = 0; c < n_sub; ++c) {
        const int slot = (int)(c & 1);
        if (c >= 2) SF_HIP(hipEventSynchronize(ev_slot[slot]));      // its previous copy has left the pinned buffer
        const uint64_t p = c * kSubBytes, q = (c + 1 == n_sub) ? n_bytes : p + kSubBytes;
        uint64_t n = q - p;
        memcpy(pinned[slot], h_text + p, n);
        if (c + 1 == n_sub) {
            const uint64_t padded = (n + 15) & ~15ull;
            memset(pinned[slot] + n, 0, padded - n);
            n = padded;
        }
        SF_HIP(hipMemcpyAsync(reinterpret_cast<char*>(S.text.p) + p, pinned[slot], n, hipMemcpyHostToDevice, cs));
        SF_HIP(hipEventRecord(ev_slot[slot], cs));
    }
    SF_HIP(hipEventRecord(ev_c1, cs));
    SF_HIP(hipStreamWaitEvent(st, ev_c1, 0));
    SF_HIP(hipEventRecord(ev_k0, st));
    const int rc = parse_device_text(m, S, reinterpret_cast<const unsigned char*>(S.text.p), n_bytes, final != 0, d_hits, cap_hits, d_off, cap_reads, res, st, h);
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_copy, ev_c0, ev_c1);
    add_elapsed(&res->ms_kernels, ev_k0, ev_k1);
    return rc;
}

extern "C" int sfgpu_bam_parse_device(sfgpu_bam* m, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, sfgpu_hit* d_hits,
                                      uint64_t cap_hits, uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream) {
    if (int r = check_parse_args("sfgpu_bam_parse_device", m, d_text, n_bytes, d_hits, cap_hits, d_off, res)) return r;
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_bam_parse_device: d_text must be 16-byte aligned");
    SF_REQUIRE(n_bytes == 0 || cap_text >= ((n_bytes + 1 + 15) & ~15ull) + 16, SFGPU_ERR_INVALID,
               "sfgpu_bam_parse_device: cap_text must hold the text, one byte more, the rest of that 16-byte group and one group more");
    hipStream_t st = as_stream(stream);
    SF_HIP(hipMemsetAsync(d_off, 0, 4, st));
    if (n_bytes == 0) { SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }
    Scratch S;
    CallScope scope;        // after the scratch, as in sfgpu_bam_parse_host
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;
    uint64_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_k0));
    SF_HIP(scope.event(&ev_k1));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint64_t)));
    SF_HIP(hipEventRecord(ev_k0, st));
    const int rc = parse_device_text(m, S, d_text, n_bytes, final != 0, d_hits, cap_hits, d_off, cap_reads, res, st, h);
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_kernels, ev_k0, ev_k1);
    return rc;
}
