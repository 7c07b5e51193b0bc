// eqtext_write.hip -- the class section of an eq_classes.txt file (GZipWriter::writeEquivCounts, src/GZipWriter.cpp:77-88)
// formatted on the device from a CSR class table: sfgpu_eqvec_write_text, the mirror of eqtext.hip.
//
// Tokens in file order are k, the ids, the count of every class: class c starts at token rowptr[c] + 2 c and token t of the
// table is followed by '\t', the count by '\n'.  All work is per token, so a label of 100 000 ids is as parallel as 100 000
// one-id labels.
//   sizing  k_tok_size: one lane per token finds its class (the class keys of a block's 256 tokens are staged in LDS) and
//           writes digits + 1; an exclusive scan (primitives.h) gives every token its byte start, 64-bit over the table.
//           k_tok_place: the start of every line, and for every 4 KB tile of the OUTPUT the token that holds its first byte.
//           textchunks.h: the longest line, and the greedy chunk ends by binary search of the line starts.
//   format  k_format: one block per 4 KB tile of the output.  The tokens that overlap the tile are formatted into an LDS image
//           of the tile (decfmt.h; a token is clipped to the tile), then every lane stores one aligned 16-byte group: global
//           memory sees only full-width coalesced stores.  Tiles are aligned in the TABLE's byte offsets, so the per-tile
//           token index is made once whatever the chunk size; a chunk's buffer starts at the tile that holds its first byte.
// The longest line, the chunk plan and the loop that hands the chunks to the sink (chunk c + 1 is produced and copied to its pinned
// buffer while the sink consumes chunk c) are textchunks.h, shared with quant_write.hip.
#include "common.h"
#include "decfmt.h"
#include "primitives.h"
#include "texttile.h"

#include <cstring>

namespace sfgpu {
namespace {

using textchunks::kBlock;
using textchunks::kTileBytes;
using textchunks::kTileShift;
using textchunks::kDefaultChunk;
using textchunks::kMaxChunk;
using textchunks::grid_of;
constexpr uint64_t kMaxClasses = 0xffffffffull;           // a token's class index is kept in 32 bits
constexpr int kMaxTokBytes = 21;                          // 20 digits and the separator

__device__ inline uint64_t class_key(const uint32_t* __restrict__ rowptr, uint64_t c) { return (uint64_t)rowptr[c] + 2 * c; }

// the value of token t of class c: 0 -> k, 1 .. k -> the ids, k + 1 -> the count (is_count)
__device__ inline uint64_t token_value(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ ids,
                                       const uint64_t* __restrict__ counts, uint64_t t, uint32_t c, bool* is_count) {
    const uint32_t r0 = rowptr[c], k = rowptr[c + 1] - r0;
    const uint64_t j = t - ((uint64_t)r0 + 2ull * c);
    *is_count = j == (uint64_t)k + 1;
    if (j == 0) return k;
    if (*is_count) return counts[c];
    return ids[t - 2ull * c - 1];
}

// misc[0] |= 1 where rowptr decreases (the token layout would leave the arrays)
__global__ void k_check_rowptr(const uint32_t* __restrict__ rowptr, uint64_t n_classes, unsigned long long* __restrict__ misc) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_classes && rowptr[c] > rowptr[c + 1]) atomicOr(&misc[0], 1ull);
}

__global__ void __launch_bounds__(kBlock)
k_tok_size(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ ids, const uint64_t* __restrict__ counts,
           uint64_t n_classes, uint64_t n_tok, uint32_t* __restrict__ tok_len, uint32_t* __restrict__ tok_class) {
    __shared__ uint64_t keys[kBlock];
    const uint64_t t0 = (uint64_t)blockIdx.x * kBlock, t = t0 + threadIdx.x;
    // the class of the block's first token (the same search in every lane: its loads are uniform)
    uint64_t lo = 0, hi = n_classes;                      // key(lo) <= t0 < key(hi), key(n_classes) = n_tok
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (class_key(rowptr, mid) <= t0) lo = mid; else hi = mid;
    }
    // a class holds >= 2 tokens: at most 128 classes begin behind t0 inside the block
    const uint64_t cc = lo + threadIdx.x;
    keys[threadIdx.x] = cc <= n_classes ? class_key(rowptr, cc) : ~0ull;
    __syncthreads();
    if (t >= n_tok) return;
    uint32_t a = 0, b = kBlock;                           // keys[a] <= t < keys[b] (keys[kBlock] = infinity)
    while (b - a > 1) {
        const uint32_t mid = (a + b) / 2;
        if (keys[mid] <= t) a = mid; else b = mid;
    }
    const uint32_t c = (uint32_t)(lo + a);
    bool is_count;
    const uint64_t v = token_value(rowptr, ids, counts, t, c, &is_count);
    tok_len[t] = (uint32_t)dec_len_u64(v) + 1u;
    tok_class[t] = c;
}

// line_start[c] = byte start of class c's first token (line_start[n_classes] = the total); tile_first[i] = the token that holds
// byte i * kTileBytes (tile_first[number of tiles] = n_tok).  A token is shorter than a tile: it crosses at most one tile edge.
__global__ void k_tok_place(const uint32_t* __restrict__ rowptr, uint64_t n_classes, uint64_t n_tok, const uint64_t* __restrict__ tok_start,
                            const uint32_t* __restrict__ tok_class, uint64_t* __restrict__ line_start, uint64_t* __restrict__ tile_first) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tok) return;
    const uint64_t s = tok_start[t], e = tok_start[t + 1];
    const uint64_t ta = s >> kTileShift, tb = (e - 1) >> kTileShift;
    if ((s & (kTileBytes - 1)) == 0) tile_first[ta] = t;
    if (tb > ta) tile_first[tb] = t;
    const uint32_t c = tok_class[t];
    if (t == class_key(rowptr, c)) line_start[c] = s;
    if (t == n_tok - 1) {
        line_start[n_classes] = e;
        tile_first[(e + kTileBytes - 1) >> kTileShift] = n_tok;
    }
}

// one block per tile of the output; `out` is the chunk buffer, whose byte 0 is table byte out_base (a multiple of kTileBytes)
__global__ void __launch_bounds__(kBlock)
k_format(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ ids, const uint64_t* __restrict__ counts,
         const uint64_t* __restrict__ tok_start, const uint32_t* __restrict__ tok_class, const uint64_t* __restrict__ tile_first,
         uint64_t n_tok, uint64_t n_bytes, uint64_t first_tile, uint64_t out_base, uint4* __restrict__ out) {
    __shared__ uint4 tile4[kBlock];
    const textchunks::Tile tile(tile4, first_tile, n_bytes);
    __syncthreads();
    // tokens [t_lo, t_hi]: t_hi holds the first byte of the next tile (it may begin there: then nothing of it is in this tile)
    const uint64_t t_lo = tile_first[tile.index];
    uint64_t t_hi = tile_first[tile.index + 1];
    if (t_hi >= n_tok) t_hi = n_tok - 1;
    for (uint64_t t = t_lo + threadIdx.x; t <= t_hi; t += kBlock) {
        const uint64_t s = tok_start[t];
        const int nd = (int)(tok_start[t + 1] - s) - 1;
        bool is_count;
        const uint64_t v = token_value(rowptr, ids, counts, t, tok_class[t], &is_count);
        const int64_t last = (int64_t)(s - tile.base) + nd - 1;     // tile offset of the last digit (may lie before or behind the tile)
        auto put = [&](int i, char ch) { tile.put(last - i, ch); };
        if (v <= 0xffffffffull) dec_put_fixed_u32((uint32_t)v, nd, 0, put);
        else dec_put_u64(v, put);
        tile.put(last + 1, is_count ? '\n' : '\t');
    }
    __syncthreads();
    tile.store(out_base, out);
}

struct WriteScratch {
    DevBuf<uint32_t> tok_len, tok_class;
    DevBuf<uint64_t> tok_start, line_start, tile_first;
    DevBuf<unsigned long long> misc;        // [0] rowptr not monotone, [1] longest line
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_eqvec_write_text(const uint32_t* d_rowptr, const uint32_t* d_ids, const uint64_t* d_counts, uint64_t n_classes,
                                      uint64_t chunk_bytes, sfgpu_text_sink sink, void* user, sfgpu_eqtext_write_result* out,
                                      sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_eqvec_write_text: null result");
    memset(out, 0, sizeof(*out));
    if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
    SF_REQUIRE(chunk_bytes >= 16 && chunk_bytes <= kMaxChunk, SFGPU_ERR_INVALID,
               "sfgpu_eqvec_write_text: chunk_bytes must lie in [16, 2^30] (0 = default)");
    if (n_classes == 0) return SFGPU_OK;
    SF_REQUIRE(d_rowptr && d_counts, SFGPU_ERR_INVALID, "sfgpu_eqvec_write_text: null table");
    SF_REQUIRE(n_classes < kMaxClasses, SFGPU_ERR_RANGE, "sfgpu_eqvec_write_text: n_classes must be below 2^32 - 1");

    WriteScratch S;
    CallScope scope;        // after S: it drains the stream before S's blocks go back to the pool
    hipStream_t st = nullptr;
    hipEvent_t ev_in = nullptr, ev_s[2] = {nullptr, nullptr};
    unsigned long long* h_misc = nullptr;     // [0 .. 1] misc, [3] total bytes, [4] rowptr[0] and rowptr[n_classes]
    SF_HIP(scope.acquire(&st));
    SF_HIP(scope.event(&ev_in, hipEventDisableTiming));
    for (auto& e : ev_s) SF_HIP(scope.event(&e));
    SF_HIP(scope.pinned_block(&h_misc, 8 * sizeof(unsigned long long)));
    // behind whatever the caller has queued on `stream`
    SF_HIP(hipEventRecord(ev_in, as_stream(stream)));
    SF_HIP(hipStreamWaitEvent(st, ev_in, 0));

    if (int rc = S.misc.reserve(4, st, false)) return rc;
    SF_HIP(hipMemsetAsync(S.misc.p, 0, 4 * sizeof(unsigned long long), st));
    uint32_t* h_ends = reinterpret_cast<uint32_t*>(&h_misc[4]);
    SF_HIP(hipMemcpyAsync(&h_ends[0], d_rowptr, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_ends[1], d_rowptr + n_classes, 4, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_check_rowptr, dim3(grid_of(n_classes)), dim3(kBlock), 0, st, d_rowptr, n_classes, S.misc.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    SF_REQUIRE(h_ends[0] == 0 && h_misc[0] == 0, SFGPU_ERR_INVALID, "sfgpu_eqvec_write_text: rowptr must start at 0 and never decrease");
    const uint64_t nnz = h_ends[1];
    SF_REQUIRE(!nnz || d_ids, SFGPU_ERR_INVALID, "sfgpu_eqvec_write_text: null ids");
    const uint64_t n_tok = nnz + 2 * n_classes;
    const uint64_t tile_cap = (n_tok * kMaxTokBytes >> kTileShift) + 2;

    // ---- sizing: token lengths, byte starts, line starts, the tile index, the longest line
    if (int rc = S.tok_len.reserve(n_tok + 1, st, false)) return rc;
    if (int rc = S.tok_class.reserve(n_tok, st, false)) return rc;
    if (int rc = S.tok_start.reserve(n_tok + 1, st, false)) return rc;
    if (int rc = S.line_start.reserve(n_classes + 1, st, false)) return rc;
    if (int rc = S.tile_first.reserve(tile_cap, st, false)) return rc;
    SF_HIP(hipEventRecord(ev_s[0], st));
    hipLaunchKernelGGL(k_tok_size, dim3(grid_of(n_tok)), dim3(kBlock), 0, st, d_rowptr, d_ids, d_counts, n_classes, n_tok,
                       S.tok_len.p, S.tok_class.p);
    SF_HIP(hipGetLastError());
    if (int rc = exclusive_scan_u32(S.tok_len.p, S.tok_start.p, n_tok, st, false)) return rc;
    hipLaunchKernelGGL(k_tok_place, dim3(grid_of(n_tok)), dim3(kBlock), 0, st, d_rowptr, n_classes, n_tok, S.tok_start.p,
                       S.tok_class.p, S.line_start.p, S.tile_first.p);
    SF_HIP(hipGetLastError());
    if (int rc = textchunks::line_max(S.line_start.p, n_classes, S.misc.p + 1, st)) return rc;
    SF_HIP(hipEventRecord(ev_s[1], st));
    SF_HIP(hipMemcpyAsync(&h_misc[1], S.misc.p + 1, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_misc[3], S.tok_start.p + n_tok, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&out->format_ms, ev_s[0], ev_s[1]);
    const uint64_t total = h_misc[3];
    out->n_bytes = total; out->n_lines = n_classes; out->n_ids = nnz; out->max_line_bytes = h_misc[1];
    if (!sink) return SFGPU_OK;
    SF_REQUIRE(out->max_line_bytes <= chunk_bytes, SFGPU_ERR_RANGE, "sfgpu_eqvec_write_text: a line is longer than chunk_bytes");

    // ---- the chunk plan and the format + copy + sink loop (textchunks.h), with this table's tiles
    textchunks::Stats ts;
    const int rc = textchunks::deliver("sfgpu_eqvec_write_text", S.line_start.p, n_classes, total, chunk_bytes, sink, user, st, &ts,
                                       [&](uint64_t first_tile, uint64_t last_tile, uint64_t out_base, uint4* buf, hipStream_t s) -> int {
        hipLaunchKernelGGL(k_format, dim3((unsigned)(last_tile - first_tile + 1)), dim3(kBlock), 0, s, d_rowptr, d_ids, d_counts,
                           S.tok_start.p, S.tok_class.p, S.tile_first.p, n_tok, total, first_tile, out_base, buf);
        SF_HIP(hipGetLastError());
        return SFGPU_OK;
    });
    out->format_ms += ts.format_ms; out->d2h_ms = ts.d2h_ms; out->sink_ms = ts.sink_ms; out->n_chunks = ts.n_chunks;
    return rc;
}
