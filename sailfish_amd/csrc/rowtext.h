// rowtext.h -- the device row writer that quant_write.hip (quant.sf) and genes.hip (quant.genes.sf) instantiate: a table of
// named rows whose numeric cells are decimal integers or %g doubles, formatted into 4 KB tiles of the output.
//   kGene = false   row r is  names[r] \t first[r] in decimal \t %g(c0) \t %g(c1) \t %g(c2) \n           (first = Length, u32)
//   kGene = true    row r is  names[first[r]] \t %g(c0) \t %g(c1) \t %g(c2) \t %g(c3) \n                 (first = the row's name index)
// with %g as printf prints a double with six significant digits (gfmt.h: exact, ties to even on the binary value).
//   sizing  k_decode: one lane per double cell -> the 4-byte record of gfmt.h (digits, exponent, sign), kept for the format
//           pass, so the wide arithmetic runs once per cell; k_decode_slow fills in the cells outside the 128-bit window.
//           k_row_size: one lane per row -> its bytes; an exclusive scan (primitives.h) gives every row its 64-bit byte
//           start.  textchunks.h: the longest row and the greedy chunk ends.
//   format  k_format: one block per 4 KB tile of the output.  The rows that overlap the tile are found by binary search of the
//           row starts (a row may span many tiles: names are of any length).  One lane per row writes the numeric tail and a
//           short name into an LDS image of the tile, clipped to the tile; names longer than kShortName bytes are copied by all
//           lanes of the block, a byte per lane and step.  Then every lane stores one aligned 16-byte group: global memory sees
//           only full-width coalesced stores.  Name bytes are copied, never inspected.
// The chunks are planned and handed to the sink by textchunks.h, the loop eqtext_write.hip uses.
#pragma once
#include "common.h"
#include "decfmt.h"
#include "gfmt.h"
#include "primitives.h"
#include "texttile.h"

#include <cstring>

namespace sfgpu {
namespace rowtext {

using textchunks::kBlock;
using textchunks::kTileBytes;
using textchunks::kDefaultChunk;
using textchunks::kMaxChunk;
using textchunks::grid_of;

constexpr uint64_t kMaxRows = 0xffffffffull;
template <bool kGene> constexpr int n_cols() { return kGene ? 4 : 3; }
// separators, [Length,] the tokens: 54 bytes (quant.sf), 57 bytes (quant.genes.sf)
template <bool kGene> constexpr uint32_t tail_max() { return 5 + (kGene ? 0 : 10) + n_cols<kGene>() * kGfmtMaxLen; }
template <bool kGene> constexpr uint64_t max_name() { return 0xffffffffull - tail_max<kGene>(); }      // a row's length is scanned in 32 bits
constexpr uint32_t kShortName = 48;                       // longer names are copied by the whole block
constexpr int kLongCap = kTileBytes / kShortName + 3;     // rows with a long name that can touch one tile

struct Cols {                                             // the double columns: three (kGene = false) or four
    const double* c[4];
};

// misc[0] |= 1 where name_off decreases, |= 2 where a name is longer than max_name()
template <bool kGene>
__global__ void k_check_off(const uint64_t* __restrict__ name_off, uint64_t n_names, unsigned long long* __restrict__ misc) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_names) return;
    const uint64_t a = name_off[r], b = name_off[r + 1];
    if (a > b) atomicOr(&misc[0], 1ull);
    else if (b - a > max_name<kGene>()) atomicOr(&misc[0], 2ull);
}

// misc[0] |= 4 where a row names an entry the name table does not have
static __global__ void k_check_name_index(const uint32_t* __restrict__ first, uint64_t n_rows, uint64_t n_names,
                                          unsigned long long* __restrict__ misc) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rows && first[r] >= n_names) atomicOr(&misc[0], 4ull);
}

// rec[col * n_rows + r] = the record of column col, row r, by the 128-bit path: registers only.  Cells outside its window are
// left as kGfmtPending and counted in misc[3]
static __global__ void __launch_bounds__(kBlock)
k_decode(Cols cols, uint64_t n_rows, uint32_t* __restrict__ rec, unsigned long long* __restrict__ misc) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double* __restrict__ col = blockIdx.y == 0 ? cols.c[0] : blockIdx.y == 1 ? cols.c[1] : blockIdx.y == 2 ? cols.c[2] : cols.c[3];
    uint32_t g = 0;
    if (r < n_rows) rec[(uint64_t)blockIdx.y * n_rows + r] = g = gfmt_decode_fast(col[r]);
    const unsigned long long m = __ballot(g == kGfmtPending);
    if (m && (threadIdx.x & (kWave - 1)) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(&misc[3], (unsigned long long)__popcll(m));
}

// the pending cells in multi-word integers (private arrays: scratch memory), in a kernel of their own so that k_decode pays for
// none of it; launched over all cells, most lanes leave at once
static __global__ void __launch_bounds__(kBlock)
k_decode_slow(Cols cols, uint64_t n_rows, uint32_t* __restrict__ rec) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t i = (uint64_t)blockIdx.y * n_rows + r;
    if (rec[i] != kGfmtPending) return;
    const double* __restrict__ col = blockIdx.y == 0 ? cols.c[0] : blockIdx.y == 1 ? cols.c[1] : blockIdx.y == 2 ? cols.c[2] : cols.c[3];
    rec[i] = gfmt_decode_slow(col[r]);
}

// the index of row r's name in the name table
template <bool kGene>
__device__ __forceinline__ uint64_t name_of(const uint32_t* __restrict__ first, uint64_t r) {
    return kGene ? (uint64_t)first[r] : r;
}

template <bool kGene>
__global__ void k_row_size(const uint64_t* __restrict__ name_off, const uint32_t* __restrict__ first, const uint32_t* __restrict__ rec,
                           uint64_t n_rows, uint32_t* __restrict__ row_len) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t ni = name_of<kGene>(first, r);
    uint32_t len = (uint32_t)(name_off[ni + 1] - name_off[ni]) + 5u;
    if (!kGene) len += (uint32_t)dec_len_u32(first[r]);
#pragma unroll
    for (int c = 0; c < n_cols<kGene>(); ++c) len += (uint32_t)gfmt_len(rec[(uint64_t)c * n_rows + r]);
    row_len[r] = len;
}

// one block per tile of the output; `out` is the chunk buffer, whose byte 0 is text byte out_base (a multiple of kTileBytes)
template <bool kGene>
__global__ void __launch_bounds__(kBlock)
k_format(const char* __restrict__ names, const uint64_t* __restrict__ name_off, const uint32_t* __restrict__ first,
         const uint32_t* __restrict__ rec, const uint64_t* __restrict__ row_start, uint64_t n_rows, uint64_t n_bytes,
         uint64_t first_tile, uint64_t out_base, uint4* __restrict__ out) {
    __shared__ uint4 tile4[kBlock];
    __shared__ uint32_t long_rows[kLongCap];
    __shared__ uint32_t n_long;
    const textchunks::Tile tile(tile4, first_tile, n_bytes);
    if (threadIdx.x == 0) n_long = 0;
    __syncthreads();
    // rows are never empty, so their starts increase strictly
    const uint64_t r_lo = textchunks::holder_of(row_start, n_rows, tile.base), r_hi = textchunks::holder_of(row_start, n_rows, tile.end() - 1);
    for (uint64_t r = r_lo + threadIdx.x; r <= r_hi; r += kBlock) {
        const uint64_t ni = name_of<kGene>(first, r);
        const uint64_t s = row_start[r], no = name_off[ni];
        const uint32_t nl = (uint32_t)(name_off[ni + 1] - no);
        const int64_t p0 = (int64_t)(s - tile.base);      // tile offset of the row's first byte (may lie before the tile)
        if (nl > kShortName) {
            const uint32_t k = atomicAdd(&n_long, 1u);
            if (k < (uint32_t)kLongCap) long_rows[k] = (uint32_t)(r - r_lo);
        } else {
            for (uint32_t i = 0; i < nl; ++i) tile.put(p0 + i, names[no + i]);
        }
        int64_t p = p0 + nl;                              // the tail: \t [Length \t] the doubles, \t between them, \n
        if (p + (int64_t)tail_max<kGene>() <= 0 || p >= (int64_t)kTileBytes) continue;
        auto sep = [&](char ch) { tile.put(p++, ch); };
        if (!kGene) {
            sep('\t');
            const uint32_t v = first[r];
            const int nd = dec_len_u32(v);
            const int64_t last = p + nd - 1;
            dec_put_fixed_u32(v, nd, 0, [&](int i, char ch) { tile.put(last - i, ch); });
            p += nd;
        }
#pragma unroll
        for (int c = 0; c < n_cols<kGene>(); ++c) {
            sep('\t');
            const uint32_t g = rec[(uint64_t)c * n_rows + r];
            const int64_t last = p + gfmt_len(g) - 1;
            p += gfmt_put(g, [&](int i, char ch) { tile.put(last - i, ch); });
        }
        sep('\n');
    }
    __syncthreads();
    // long names: all lanes copy the part of the name that lies in the tile
    const uint32_t nl_rows = n_long < (uint32_t)kLongCap ? n_long : (uint32_t)kLongCap;
    for (uint32_t k = 0; k < nl_rows; ++k) {
        const uint64_t r = r_lo + long_rows[k];
        const uint64_t ni = name_of<kGene>(first, r);
        const uint64_t s = row_start[r], no = name_off[ni], e = s + (name_off[ni + 1] - no);
        const uint64_t a = s > tile.base ? s : tile.base, b = e < tile.end() ? e : tile.end();
        for (uint64_t x = a + threadIdx.x; x < b; x += kBlock) tile.bytes[x - tile.base] = names[no + (x - s)];
    }
    __syncthreads();
    tile.store(out_base, out);
}

struct Scratch {
    DevBuf<uint32_t> rec, row_len;
    DevBuf<uint64_t> row_start;
    DevBuf<unsigned long long> misc;        // [0] name table flags, [1] longest row, [3] slow cells
};

// The body of sfgpu_quant_write_text (kGene = false: n_names = n_rows, `first` = Length) and sfgpu_genes_write_text (kGene =
// true: `first` = each row's index into the n_names names); the contract is in sfgpu.h.  `who` names the entry in messages.
template <bool kGene>
int write_rows(const char* who, const char* d_names, const uint64_t* d_name_off, uint64_t n_names, const uint32_t* d_first, Cols cols,
               uint64_t n_rows, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user, sfgpu_quant_write_result* out, sfgpu_stream stream) {
    Scratch S;
    CallScope scope;        // after S: it drains the stream before S's blocks go back to the pool
    hipStream_t st = nullptr;
    hipEvent_t ev_in = nullptr, ev_s[2] = {nullptr, nullptr};
    unsigned long long* h_misc = nullptr;     // [0 .. 3] misc, [4] total bytes, [5] name_off[0], [6] name_off[n_names]
    constexpr int kCols = n_cols<kGene>();
    auto fail = [&](int code, const char* what) -> int { set_error("%s: %s", who, what); return code; };
    SF_HIP(scope.acquire(&st));
    SF_HIP(scope.event(&ev_in, hipEventDisableTiming));
    for (auto& e : ev_s) SF_HIP(scope.event(&e));
    SF_HIP(scope.pinned_block(&h_misc, 8 * sizeof(unsigned long long)));
    // behind whatever the caller has queued on `stream`
    SF_HIP(hipEventRecord(ev_in, as_stream(stream)));
    SF_HIP(hipStreamWaitEvent(st, ev_in, 0));

    if (int rc = S.misc.reserve(4, st, false)) return rc;
    SF_HIP(hipMemsetAsync(S.misc.p, 0, 4 * sizeof(unsigned long long), st));
    SF_HIP(hipMemcpyAsync(&h_misc[5], d_name_off, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_misc[6], d_name_off + n_names, 8, hipMemcpyDeviceToHost, st));
    if (n_names) {
        hipLaunchKernelGGL(k_check_off<kGene>, dim3(grid_of(n_names)), dim3(kBlock), 0, st, d_name_off, n_names, S.misc.p);
        SF_HIP(hipGetLastError());
    }
    if (kGene) {
        hipLaunchKernelGGL(k_check_name_index, dim3(grid_of(n_rows)), dim3(kBlock), 0, st, d_first, n_rows, n_names, S.misc.p);
        SF_HIP(hipGetLastError());
    }
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h_misc[5] != 0 || (h_misc[0] & 1)) return fail(SFGPU_ERR_INVALID, "name_off must start at 0 and never decrease");
    if (h_misc[0] & 2) return fail(SFGPU_ERR_RANGE, "a name is longer than 2^32 - 60 bytes");
    if (h_misc[0] & 4) return fail(SFGPU_ERR_INVALID, "a row's name index is not below the number of names");
    if (h_misc[6] && !d_names) return fail(SFGPU_ERR_INVALID, "null names");

    // ---- sizing: the decoded cells, row lengths, row starts, the longest row
    if (int rc = S.rec.reserve(kCols * n_rows, st, false)) return rc;
    if (int rc = S.row_len.reserve(n_rows + 1, st, false)) return rc;
    if (int rc = S.row_start.reserve(n_rows + 1, st, false)) return rc;
    SF_HIP(hipEventRecord(ev_s[0], st));
    hipLaunchKernelGGL(k_decode, dim3(grid_of(n_rows), kCols), dim3(kBlock), 0, st, cols, n_rows, S.rec.p, S.misc.p);
    SF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_decode_slow, dim3(grid_of(n_rows), kCols), dim3(kBlock), 0, st, cols, n_rows, S.rec.p);
    SF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_row_size<kGene>, dim3(grid_of(n_rows)), dim3(kBlock), 0, st, d_name_off, d_first, S.rec.p, n_rows, S.row_len.p);
    SF_HIP(hipGetLastError());
    if (int rc = exclusive_scan_u32(S.row_len.p, S.row_start.p, n_rows, st, false)) return rc;
    if (int rc = textchunks::line_max(S.row_start.p, n_rows, S.misc.p + 1, st)) return rc;
    SF_HIP(hipEventRecord(ev_s[1], st));
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_misc[4], S.row_start.p + n_rows, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&out->format_ms, ev_s[0], ev_s[1]);
    const uint64_t total = h_misc[4];
    out->n_bytes = total; out->n_rows = n_rows; out->max_row_bytes = h_misc[1]; out->n_slow = h_misc[3];
    if (!sink) return SFGPU_OK;
    if (out->max_row_bytes > chunk_bytes) return fail(SFGPU_ERR_RANGE, "a row is longer than chunk_bytes");

    // ---- the chunk plan and the format + copy + sink loop (textchunks.h), with this table's tiles
    textchunks::Stats ts;
    const int rc = textchunks::deliver(who, S.row_start.p, n_rows, total, chunk_bytes, sink, user, st, &ts,
                                       [&](uint64_t first_tile, uint64_t last_tile, uint64_t out_base, uint4* buf, hipStream_t s) -> int {
        hipLaunchKernelGGL(k_format<kGene>, dim3((unsigned)(last_tile - first_tile + 1)), dim3(kBlock), 0, s, d_names, d_name_off, d_first,
                           S.rec.p, S.row_start.p, n_rows, total, first_tile, out_base, buf);
        SF_HIP(hipGetLastError());
        return SFGPU_OK;
    });
    out->format_ms += ts.format_ms; out->d2h_ms = ts.d2h_ms; out->sink_ms = ts.sink_ms; out->n_chunks = ts.n_chunks;
    return rc;
}

}  // namespace rowtext
}  // namespace sfgpu
