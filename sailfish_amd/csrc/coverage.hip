// coverage.hip -- sfgpu_cov_*: posterior-weighted coverage of the transcripts accumulated over a run's batches, its runs and summary
// columns, and the bedGraph file.  WHAT a line covers, what a record weighs, what a run, a row and a column are is csrc/coverfmt.h,
// stated once and run here unchanged; this file is only the way the work is laid out.
//
//   k_cov_len1      a lane per transcript: len + 1, scanned into the transcripts' bases (open)
//   k_cov_check     a fixed grid strides over the records: the lowest record whose tid is no transcript and the lowest whose p is
//                   refused (atomicMin), and the batch's lines, before anything is added
//   k_cov_add       a fixed grid strides over the line slots (two a record): a lane takes a line, walks its words where there is an
//                   alignment and adds +q / -q at the ends of every interval with 64-bit integer atomics whose result is not
//                   returned.  Integer addition commutes: the order the lanes arrive in changes no bit.  The counters leave as one
//                   atomic a wavefront.
//   finish          the inclusive scan (primitives.h); then the runs by count -> scan -> write: a block takes a tile of 2048 slots, a
//                   lane 8 consecutive ones and the slot before them.  A slot opens a run iff its sum is not 0 and differs from the
//                   slot before it -- every transcript's last slot reads 0, so no run crosses into the next transcript and the test
//                   needs no transcript.  k_cov_run_count leaves the tile's count, the scan of the counts places the tiles, and
//                   k_cov_run_write ranks the lanes by a block scan and writes (tid, start, sum) where a run opens and the end where
//                   one closes: the run that closes at a slot is the last one opened before it.  The transcript is found by binary
//                   search of the bases, once a run.
//   k_cov_summary   a wavefront per transcript strides over its bases: covered, the 128-bit sum as two words with the carry, the
//                   maximum; a butterfly folds the lanes (integer sums: any tree gives the same bits) and lane 0 writes the columns.
//   write           cov_write, over a run table (covwrite.h: the genome coverage calls it too): k_cov_decode / k_cov_decode_slow: the
//                   six-digit record of every run's depth; k_cov_row_size: a lane per run sizes its row; a scan places the rows;
//                   k_cov_format: a block per 4 KB tile of the output formats the rows that touch it in LDS (texttile.h; long names
//                   by the whole block) and every lane stores 16 bytes.  The chunks are planned and delivered by textchunks.h, to
//                   the sink or on the device to the BGZF encoder.
#include "common.h"
#include "coverfmt.h"
#include "covwrite.h"
#include "hitgroup.h"
#include "primitives.h"
#include "texttile.h"

#include <cstring>

namespace sfgpu {
namespace {

using textchunks::kBlock;
using textchunks::kTileBytes;
using textchunks::kDefaultChunk;
using textchunks::kMaxChunk;
using textchunks::grid_of;

constexpr unsigned kCovGridMax = 4096;                     // the fixed grids of the check and add passes
constexpr int kCovPerLane = 8;                             // slots a lane takes in the run passes
constexpr uint64_t kCovTile = (uint64_t)kBlock * kCovPerLane;
enum { kCovBadTid = 0, kCovBadP, kCovLines, kCovIntervals, kCovEmpty, kCovBases, kCovCounters };
enum { kCovCovered = 0, kCovResidue, kCovFinishCounters };

inline unsigned cov_grid(uint64_t n) { return n ? (grid_of(n) < kCovGridMax ? grid_of(n) : kCovGridMax) : 1u; }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void k_cov_len1(const uint32_t* __restrict__ ref_len, uint64_t M, uint32_t* __restrict__ len1, unsigned long long* __restrict__ flag) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    const uint32_t l = ref_len[t];
    if (l == 0xffffffffu) atomicOr(flag, 1ull);
    len1[t] = l + 1u;
}

__global__ void __launch_bounds__(kBlock)
k_cov_check(const sfgpu_hit* __restrict__ hits, uint64_t n_rec, uint64_t M, const double* __restrict__ p, unsigned long long* __restrict__ ctr) {
    unsigned long long lines = 0;
    for (uint64_t h = (uint64_t)blockIdx.x * kBlock + threadIdx.x; h < n_rec; h += (uint64_t)gridDim.x * kBlock) {
        const sfgpu_hit hit = hits[h];
        if (hit.tid >= M) atomicMin(&ctr[kCovBadTid], (unsigned long long)h);
        if (p && cov_p_bad(p[h])) atomicMin(&ctr[kCovBadP], (unsigned long long)h);
        lines += cov_record_lines(hit);
    }
    lines = wave_sum(lines);
    if ((threadIdx.x & (kWave - 1)) == 0 && lines) atomicAdd(&ctr[kCovLines], lines);
}

// every tid is below M here (k_cov_check), so a line's slots base[tid] + [0, len] lie inside the array
__global__ void __launch_bounds__(kBlock)
k_cov_add(const sfgpu_hit* __restrict__ hits, const uint32_t* __restrict__ hit_off, uint64_t n_reads, uint64_t n_rec, const double* __restrict__ p,
          const int32_t* __restrict__ aln_pos, const uint64_t* __restrict__ aln_op_off, const uint32_t* __restrict__ aln_ops,
          const uint64_t* __restrict__ base, unsigned long long* __restrict__ slot, unsigned long long* __restrict__ ctr) {
    CovCount sum = {0, 0, 0};
    for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < 2 * n_rec; s += (uint64_t)gridDim.x * kBlock) {
        const uint64_t h = s >> 1;
        const uint32_t w = (uint32_t)(s & 1);
        const sfgpu_hit hit = hits[h];
        if (w >= cov_record_lines(hit)) continue;
        uint64_t q;
        if (p) q = cov_weight(p[h]);
        else {
            const uint64_t r = textchunks::holder_of(hit_off, n_reads, (uint32_t)h);
            const uint64_t n = (uint64_t)hit_off[r + 1] - hit_off[r];
            q = cov_weight_uniform(n ? n : 1);
        }
        const uint64_t at = base[hit.tid], len_t = base[hit.tid + 1] - at - 1;
        const uint64_t o0 = aln_pos ? aln_op_off[s] : 0, n_ops = aln_pos ? aln_op_off[s + 1] - o0 : 0;
        const CovCount c = cov_line(cov_line_pos(hit, w), cov_line_len(hit, w), len_t, aln_pos != nullptr, aln_ops + o0, n_ops, aln_pos ? (int64_t)aln_pos[s] : 0,
                                    [&](uint64_t lo, uint64_t hi) {
                                        atomicAdd(&slot[at + lo], (unsigned long long)q);
                                        atomicAdd(&slot[at + hi], (unsigned long long)(0ull - q));
                                    });
        sum.intervals += c.intervals; sum.empty += c.empty; sum.bases += c.bases;
    }
    const unsigned long long a = wave_sum(sum.intervals), b = wave_sum(sum.empty), c = wave_sum(sum.bases);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (a) atomicAdd(&ctr[kCovIntervals], a);
        if (b) atomicAdd(&ctr[kCovEmpty], b);
        if (c) atomicAdd(&ctr[kCovBases], c);
    }
}

// a lane's kCovPerLane slots from i0 on and the one before them (0 before the array and behind it)
__device__ __forceinline__ void cov_load(const uint64_t* __restrict__ slot, uint64_t N, uint64_t i0, uint64_t (&v)[kCovPerLane + 1]) {
    v[0] = (i0 > 0 && i0 <= N) ? slot[i0 - 1] : 0;
#pragma unroll
    for (int j = 0; j < kCovPerLane; ++j) v[j + 1] = i0 + j < N ? slot[i0 + j] : 0;
}
__device__ __forceinline__ uint32_t cov_opens(const uint64_t (&v)[kCovPerLane + 1]) {
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < kCovPerLane; ++j) n += (v[j + 1] != 0 && v[j + 1] != v[j]) ? 1u : 0u;
    return n;
}

// the exclusive scan of one value a lane over the block, *total in every lane; s_wave: kBlock / kWave words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += u; }
    if (lane == kWave - 1) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kBlock / kWave; ++k) { const uint32_t t = s_wave[k]; if ((uint32_t)k < wave) before += t; all += t; }
    *total = all;
    return before + inc - v;
}

__global__ void __launch_bounds__(kBlock)
k_cov_run_count(const uint64_t* __restrict__ slot, uint64_t N, uint32_t* __restrict__ tile_runs) {
    __shared__ uint32_t s_wave[kBlock / kWave];
    uint64_t v[kCovPerLane + 1];
    cov_load(slot, N, ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kCovPerLane, v);
    uint32_t total;
    block_excl_scan(cov_opens(v), s_wave, &total);
    if (threadIdx.x == 0) tile_runs[blockIdx.x] = total;
}

// tile_start[b]: the runs opened before tile b; the arrays have room for all n_runs = tile_start[gridDim.x]
__global__ void __launch_bounds__(kBlock)
k_cov_run_write(const uint64_t* __restrict__ slot, uint64_t N, const uint64_t* __restrict__ base, uint64_t M, const uint64_t* __restrict__ tile_start,
                uint64_t n_runs, uint32_t* __restrict__ r_tid, uint32_t* __restrict__ r_start, uint32_t* __restrict__ r_end, uint64_t* __restrict__ r_sum) {
    __shared__ uint32_t s_wave[kBlock / kWave];
    uint64_t v[kCovPerLane + 1];
    const uint64_t i0 = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kCovPerLane;
    cov_load(slot, N, i0, v);
    uint32_t total;
    uint64_t k = tile_start[blockIdx.x] + block_excl_scan(cov_opens(v), s_wave, &total);        // runs opened before slot i0
#pragma unroll
    for (int j = 0; j < kCovPerLane; ++j) {
        const uint64_t i = i0 + j;
        if (i >= N || v[j + 1] == v[j]) continue;
        if (v[j] != 0 && k >= 1 && k <= n_runs) {          // the run whose last base is slot i - 1 closes
            const uint64_t t = textchunks::holder_of(base, M, i - 1);
            r_end[k - 1] = (uint32_t)(i - base[t]);
        }
        if (v[j + 1] != 0) {
            if (k < n_runs) {
                const uint64_t t = textchunks::holder_of(base, M, i);
                r_tid[k] = (uint32_t)t; r_start[k] = (uint32_t)(i - base[t]); r_sum[k] = v[j + 1];
            }
            ++k;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
k_cov_summary(const uint64_t* __restrict__ slot, const uint64_t* __restrict__ base, uint64_t M, double* __restrict__ frac, double* __restrict__ mean,
              double* __restrict__ maxd, unsigned long long* __restrict__ ctr) {
    const uint64_t t = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (t >= M) return;                                    // (a whole wavefront)
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t at = base[t], len = base[t + 1] - at - 1;
    unsigned long long cov = 0, lo = 0, hi = 0, mx = 0;
    for (uint64_t i = lane; i < len; i += kWave) {
        const unsigned long long v = slot[at + i];
        cov += v != 0;
        lo += v; hi += lo < v;
        mx = v > mx ? v : mx;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long lo2 = __shfl_xor(lo, o), hi2 = __shfl_xor(hi, o), mx2 = __shfl_xor(mx, o);
        cov += __shfl_xor(cov, o);
        lo += lo2; hi += hi2 + (lo < lo2);
        mx = mx2 > mx ? mx2 : mx;
    }
    if (lane) return;
    cov_summary((uint32_t)len, cov, hi, lo, mx, &frac[t], &mean[t], &maxd[t]);
    if (cov) atomicAdd(&ctr[kCovCovered], cov);
    if (slot[at + len] != 0) atomicAdd(&ctr[kCovResidue], 1ull);
}

// ---- the file ----------------------------------------------------------------------------------------------------------------------
constexpr uint64_t kMaxRows = 0xffffffffull;
constexpr uint64_t kMaxName = 0xffffffffull - kCovRowTail;  // a row's length is scanned in 32 bits
constexpr uint32_t kShortName = 48;                        // longer names are copied by the whole block
constexpr int kLongCap = kTileBytes / kShortName + 3;      // rows with a long name that can touch one tile

// misc[0] |= 1 where name_off decreases, |= 2 where a name is longer than kMaxName
__global__ void k_cov_check_names(const uint64_t* __restrict__ name_off, uint64_t M, unsigned long long* __restrict__ misc) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    const uint64_t a = name_off[t], b = name_off[t + 1];
    if (a > b) atomicOr(&misc[0], 1ull);
    else if (b - a > kMaxName) atomicOr(&misc[0], 2ull);
}

// rec[r] = the record of run r's depth; the ones outside the 128-bit window are left pending for k_cov_decode_slow
__global__ void __launch_bounds__(kBlock)
k_cov_decode(const uint64_t* __restrict__ r_sum, uint64_t n_runs, uint32_t* __restrict__ rec) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r < n_runs) rec[r] = gfmt_decode_fast(cov_depth(r_sum[r]));
}
__global__ void __launch_bounds__(kBlock)
k_cov_decode_slow(const uint64_t* __restrict__ r_sum, uint64_t n_runs, uint32_t* __restrict__ rec) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_runs || rec[r] != kGfmtPending) return;
    rec[r] = gfmt_decode_slow(cov_depth(r_sum[r]));
}

__global__ void __launch_bounds__(kBlock)
k_cov_row_size(const uint64_t* __restrict__ name_off, const uint32_t* __restrict__ r_tid, const uint32_t* __restrict__ r_start, const uint32_t* __restrict__ r_end,
               const uint32_t* __restrict__ rec, uint64_t n_runs, uint32_t* __restrict__ row_len) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_runs) return;
    const uint64_t t = r_tid[r];
    row_len[r] = (uint32_t)(name_off[t + 1] - name_off[t]) + cov_row_tail_len(r_start[r], r_end[r], rec[r]);
}

// one block per tile of the output; `out` is the chunk buffer, whose byte 0 is text byte out_base (a multiple of kTileBytes)
__global__ void __launch_bounds__(kBlock)
k_cov_format(const char* __restrict__ names, const uint64_t* __restrict__ name_off, const uint32_t* __restrict__ r_tid, const uint32_t* __restrict__ r_start,
             const uint32_t* __restrict__ r_end, const uint32_t* __restrict__ rec, const uint64_t* __restrict__ row_start, uint64_t n_rows, uint64_t n_bytes,
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
        const uint64_t t = r_tid[r], no = name_off[t];
        const uint32_t nl = (uint32_t)(name_off[t + 1] - no);
        const int64_t p0 = (int64_t)(row_start[r] - tile.base);      // tile offset of the row's first byte (may lie before the tile)
        if (nl > kShortName) {
            const uint32_t k = atomicAdd(&n_long, 1u);
            if (k < (uint32_t)kLongCap) long_rows[k] = (uint32_t)(r - r_lo);
        } else {
            for (uint32_t i = 0; i < nl; ++i) tile.put(p0 + i, names[no + i]);
        }
        const int64_t p = p0 + nl;
        if (p + (int64_t)kCovRowTail <= 0 || p >= (int64_t)kTileBytes) continue;
        cov_row_tail(r_start[r], r_end[r], rec[r], [&](int i, char ch) { tile.put(p + i, ch); });
    }
    __syncthreads();
    // long names: all lanes copy the part of the name that lies in the tile
    const uint32_t nl_rows = n_long < (uint32_t)kLongCap ? n_long : (uint32_t)kLongCap;
    for (uint32_t k = 0; k < nl_rows; ++k) {
        const uint64_t r = r_lo + long_rows[k];
        const uint64_t t = r_tid[r];
        const uint64_t s = row_start[r], no = name_off[t], e = s + (name_off[t + 1] - no);
        const uint64_t a = s > tile.base ? s : tile.base, b = e < tile.end() ? e : tile.end();
        for (uint64_t x = a + threadIdx.x; x < b; x += kBlock) tile.bytes[x - tile.base] = names[no + (x - s)];
    }
    __syncthreads();
    tile.store(out_base, out);
}

struct WriteScratch {
    DevBuf<uint32_t> rec, row_len;
    DevBuf<uint64_t> row_start;
    DevBuf<unsigned long long> misc;                       // [0] name table flags, [1] the longest row
};

}  // namespace

// `out` starts zeroed; the caller has checked its handle and copies the figures into its own result
int cov_write(const char* who, const CovRunTable& T, const char* d_names, const uint64_t* d_name_off, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
              sfgpu_bgzw* z, CovWriteStats* out, sfgpu_stream stream) {
    auto fail = [&](int code, const char* what) -> int { set_error("%s: %s", who, what); return code; };
    *out = CovWriteStats{};
    if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
    if (!(chunk_bytes >= 16 && chunk_bytes <= kMaxChunk)) return fail(SFGPU_ERR_INVALID, "chunk_bytes must lie in [16, 2^30] (0 = default)");
    const uint64_t n_rows = T.n_rows, M = T.n_names;
    if (n_rows == 0) return SFGPU_OK;
    if (!d_name_off) return fail(SFGPU_ERR_INVALID, "null name offsets");
    if (!(n_rows < kMaxRows)) return fail(SFGPU_ERR_RANGE, "the runs must be fewer than 2^32 - 1");

    WriteScratch S;
    CallScope scope;        // after S: it drains the stream before S's blocks go back to the pool
    hipStream_t st = nullptr;
    hipEvent_t ev_in = nullptr, ev_s[2] = {nullptr, nullptr};
    unsigned long long* h_misc = nullptr;     // [0 .. 1] misc, [2] total bytes, [3] name_off[0], [4] name_off[M]
    SF_HIP(scope.acquire(&st));
    SF_HIP(scope.event(&ev_in, hipEventDisableTiming));
    for (auto& e : ev_s) SF_HIP(scope.event(&e));
    SF_HIP(scope.pinned_block(&h_misc, 8 * sizeof(unsigned long long)));
    // behind whatever the caller has queued on `stream`
    SF_HIP(hipEventRecord(ev_in, as_stream(stream)));
    SF_HIP(hipStreamWaitEvent(st, ev_in, 0));

    if (int rc = S.misc.reserve(4, st, false)) return rc;
    SF_HIP(hipMemsetAsync(S.misc.p, 0, 4 * sizeof(unsigned long long), st));
    SF_HIP(hipMemcpyAsync(&h_misc[3], d_name_off, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_misc[4], d_name_off + M, 8, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_cov_check_names, dim3(grid_of(M)), dim3(kBlock), 0, st, d_name_off, M, S.misc.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h_misc[3] != 0 || (h_misc[0] & 1)) return fail(SFGPU_ERR_INVALID, "name_off must start at 0 and never decrease");
    if (h_misc[0] & 2) return fail(SFGPU_ERR_RANGE, "a name is longer than 2^32 - 38 bytes");
    if (h_misc[4] && !d_names) return fail(SFGPU_ERR_INVALID, "null names");

    // ---- sizing: the depth records, row lengths, row starts, the longest row
    if (int rc = S.rec.reserve(n_rows, st, false)) return rc;
    if (int rc = S.row_len.reserve(n_rows + 1, st, false)) return rc;
    if (int rc = S.row_start.reserve(n_rows + 1, st, false)) return rc;
    SF_HIP(hipEventRecord(ev_s[0], st));
    hipLaunchKernelGGL(k_cov_decode, dim3(grid_of(n_rows)), dim3(kBlock), 0, st, T.sum, n_rows, S.rec.p);
    SF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cov_decode_slow, dim3(grid_of(n_rows)), dim3(kBlock), 0, st, T.sum, n_rows, S.rec.p);
    SF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cov_row_size, dim3(grid_of(n_rows)), dim3(kBlock), 0, st, d_name_off, T.id, T.start,
                       T.end, (const uint32_t*)S.rec.p, n_rows, S.row_len.p);
    SF_HIP(hipGetLastError());
    if (int rc = exclusive_scan_u32(S.row_len.p, S.row_start.p, n_rows, st, false)) return rc;
    if (int rc = textchunks::line_max(S.row_start.p, n_rows, S.misc.p + 1, st)) return rc;
    SF_HIP(hipEventRecord(ev_s[1], st));
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_misc[2], S.row_start.p + n_rows, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&out->format_ms, ev_s[0], ev_s[1]);
    const uint64_t total = h_misc[2];
    out->n_bytes = total; out->max_row_bytes = h_misc[1];
    if (!sink && !z) return SFGPU_OK;
    if (out->max_row_bytes > chunk_bytes) return fail(SFGPU_ERR_RANGE, "a row is longer than chunk_bytes");

    // ---- the chunk plan and the format + copy + sink loop (textchunks.h), with this text's tiles
    textchunks::Stats ts;
    auto format_tiles = [&](uint64_t first_tile, uint64_t last_tile, uint64_t out_base, uint4* buf, hipStream_t s) -> int {
        hipLaunchKernelGGL(k_cov_format, dim3((unsigned)(last_tile - first_tile + 1)), dim3(kBlock), 0, s, d_names, d_name_off, T.id,
                           T.start, T.end, (const uint32_t*)S.rec.p, (const uint64_t*)S.row_start.p, n_rows, total,
                           first_tile, out_base, buf);
        SF_HIP(hipGetLastError());
        return SFGPU_OK;
    };
    // compressed: the chunk's device bytes go to the BGZF encoder, which copies and sinks what IT writes
    const int rc = z ? textchunks::deliver_device(who, S.row_start.p, n_rows, total, chunk_bytes, st, &ts,
                                                  [&](const uint8_t* d_bytes, uint64_t n, hipStream_t ready) -> int {
                                                      return sfgpu_bgzw_write_device(z, d_bytes, n, reinterpret_cast<sfgpu_stream>(ready));
                                                  }, format_tiles)
                     : textchunks::deliver(who, S.row_start.p, n_rows, total, chunk_bytes, sink, user, st, &ts, format_tiles);
    out->format_ms += ts.format_ms; out->d2h_ms = ts.d2h_ms; out->sink_ms = ts.sink_ms; out->n_chunks = ts.n_chunks;
    return rc;
}

}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_cov_open(sfgpu_cov** out, const uint32_t* d_ref_len, uint64_t M, sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_cov_open: null handle pointer");
    *out = nullptr;
    SF_REQUIRE(d_ref_len || M == 0, SFGPU_ERR_INVALID, "sfgpu_cov_open: null transcript lengths");
    SF_REQUIRE(M < 0xffffffffull, SFGPU_ERR_RANGE, "sfgpu_cov_open: the transcripts must be fewer than 2^32 - 1");
    hipStream_t st = as_stream(stream);
    sfgpu_cov* c = new sfgpu_cov;
    struct Guard { sfgpu_cov* c; ~Guard() { delete c; } } guard{c};
    DevBuf<uint32_t> len1; DevBuf<unsigned long long> flag;
    StreamSyncOnExit sync_first{st};          // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    int rc;
    if ((rc = len1.reserve(M + 1, st, false)) || (rc = flag.reserve(1, st, false)) || (rc = c->base.reserve(M + 1, st, false))) return rc;
    SF_HIP(hipMemsetAsync(flag.p, 0, 8, st));
    SF_HIP(hipMemsetAsync(len1.p, 0, (M + 1) * 4, st));
    if (M) {
        hipLaunchKernelGGL(k_cov_len1, dim3(grid_of(M)), dim3(kBlock), 0, st, d_ref_len, M, len1.p, flag.p);
        SF_CHECK_LAUNCH();
    }
    if ((rc = exclusive_scan_u32(len1.p, c->base.p, M, st, false))) return rc;
    unsigned long long h[2] = {0, 0};
    SF_HIP(hipMemcpyAsync(&h[0], flag.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h[1], c->base.p + M, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    SF_REQUIRE(!h[0], SFGPU_ERR_RANGE, "sfgpu_cov_open: a transcript of 2^32 - 1 bases");
    c->M = M; c->N = h[1];
    if ((rc = c->slot.reserve(c->N ? c->N : 1, st, false))) return rc;
    SF_HIP(hipMemsetAsync(c->slot.p, 0, (c->N ? c->N : 1) * 8, st));
    SF_HIP(hipStreamSynchronize(st));
    guard.c = nullptr;
    *out = c;
    return SFGPU_OK;
}

extern "C" int sfgpu_cov_close(sfgpu_cov* c) {
    if (!c) return SFGPU_OK;
    (void)hipDeviceSynchronize();
    delete c;
    return SFGPU_OK;
}

extern "C" int sfgpu_cov_add(sfgpu_cov* c, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, const double* d_p,
                             const int32_t* d_aln_pos, const uint64_t* d_aln_op_off, const uint32_t* d_aln_ops, sfgpu_cov_stats* stats,
                             sfgpu_stream stream) {
    const char* who = "sfgpu_cov_add";
    SF_REQUIRE(c && stats && (d_hit_offsets || n_reads == 0), SFGPU_ERR_INVALID, "sfgpu_cov_add: null pointer");
    SF_REQUIRE(!c->finished, SFGPU_ERR_INVALID, "sfgpu_cov_add: called after sfgpu_cov_finish");
    SF_REQUIRE((d_aln_pos != nullptr) == (d_aln_op_off != nullptr) && (d_aln_pos || !d_aln_ops), SFGPU_ERR_INVALID,
               "sfgpu_cov_add: the alignment's pos, op_off and ops come together or not at all");
    hipStream_t st = as_stream(stream);
    uint64_t n_rec = 0;
    if (int rc = hit_n_rec(d_hit_offsets, n_reads, st, &n_rec)) return rc;
    SF_REQUIRE(n_rec == 0 || d_hits, SFGPU_ERR_INVALID, "sfgpu_cov_add: null records");
    DevBuf<unsigned long long> ctr;
    StreamSyncOnExit sync_first{st};          // (declared after the buffer: an early return waits for the kernels before scratch goes back)
    unsigned long long h_ctr[kCovCounters + 1] = {~0ull, ~0ull, 0, 0, 0, 0, 0};      // [kCovCounters]: the alignment's words
    if (int rc = ctr.reserve(kCovCounters, st, false)) return rc;
    SF_HIP(hipMemcpyAsync(ctr.p, h_ctr, kCovCounters * sizeof h_ctr[0], hipMemcpyHostToDevice, st));
    if (n_rec) {
        hipLaunchKernelGGL(k_cov_check, dim3(cov_grid(n_rec)), dim3(kBlock), 0, st, d_hits, n_rec, c->M, d_p, ctr.p);
        SF_CHECK_LAUNCH();
        if (d_aln_pos) SF_HIP(hipMemcpyAsync(&h_ctr[kCovCounters], d_aln_op_off + 2 * n_rec, 8, hipMemcpyDeviceToHost, st));
    }
    SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, 3 * sizeof h_ctr[0], hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h_ctr[kCovBadTid] != ~0ull) {
        set_error("%s: record %llu names transcript >= %llu", who, h_ctr[kCovBadTid], (unsigned long long)c->M);
        return SFGPU_ERR_RANGE;
    }
    if (h_ctr[kCovBadP] != ~0ull) {
        set_error("%s: the posterior of record %llu is NaN, negative or above 1", who, h_ctr[kCovBadP]);
        return SFGPU_ERR_INVALID;
    }
    if (c->stats.lines + h_ctr[kCovLines] > kCovMaxLines) {
        set_error("%s: %llu lines more would bring the total to 2^32 or beyond", who, h_ctr[kCovLines]);
        return SFGPU_ERR_RANGE;
    }
    SF_REQUIRE(!h_ctr[kCovCounters] || d_aln_ops, SFGPU_ERR_INVALID, "sfgpu_cov_add: the alignment has operations but no ops array");
    if (n_rec) {
        hipLaunchKernelGGL(k_cov_add, dim3(cov_grid(2 * n_rec)), dim3(kBlock), 0, st, d_hits, d_hit_offsets, (uint64_t)n_reads, n_rec, d_p, d_aln_pos, d_aln_op_off,
                           d_aln_ops, (const uint64_t*)c->base.p, reinterpret_cast<unsigned long long*>(c->slot.p), ctr.p);
        SF_CHECK_LAUNCH();
        SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, kCovCounters * sizeof h_ctr[0], hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
    }
    sfgpu_cov_stats& t = c->stats;
    t.reads += n_reads; t.records += n_rec; t.lines += h_ctr[kCovLines];
    t.intervals += h_ctr[kCovIntervals]; t.empty_intervals += h_ctr[kCovEmpty]; t.bases_added += h_ctr[kCovBases];
    stats->reads += n_reads; stats->records += n_rec; stats->lines += h_ctr[kCovLines];
    stats->intervals += h_ctr[kCovIntervals]; stats->empty_intervals += h_ctr[kCovEmpty]; stats->bases_added += h_ctr[kCovBases];
    return SFGPU_OK;
}

extern "C" int sfgpu_cov_finish(sfgpu_cov* c, sfgpu_cov_result* out, sfgpu_stream stream) {
    SF_REQUIRE(c && out, SFGPU_ERR_INVALID, "sfgpu_cov_finish: null pointer");
    if (c->finished) { *out = c->res; return SFGPU_OK; }
    hipStream_t st = as_stream(stream);
    const uint64_t N = c->N, M = c->M, n_tiles = (N + kCovTile - 1) / kCovTile;
    DevBuf<uint32_t> tile_runs; DevBuf<uint64_t> tile_start; DevBuf<unsigned long long> ctr;
    StreamSyncOnExit sync_first{st};          // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Events { hipEvent_t* e; ~Events() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } events{ev};
    for (auto& e : ev) SF_HIP(hipEventCreate(&e));
    int rc;
    if ((rc = tile_runs.reserve(n_tiles + 1, st, false)) || (rc = tile_start.reserve(n_tiles + 1, st, false)) || (rc = ctr.reserve(kCovFinishCounters, st, false)) ||
        (rc = c->col.reserve(3 * M + 1, st, false)))
        return rc;
    SF_HIP(hipEventRecord(ev[0], st));
    SF_HIP(hipMemsetAsync(ctr.p, 0, kCovFinishCounters * sizeof(unsigned long long), st));
    SF_HIP(hipMemsetAsync(tile_runs.p, 0, (n_tiles + 1) * 4, st));
    if ((rc = inclusive_scan_u64(c->slot.p, N, st))) return rc;
    c->finished = true;                                    // the slots hold sums from here on: nothing may be added
    if (n_tiles) {
        hipLaunchKernelGGL(k_cov_run_count, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, (const uint64_t*)c->slot.p, N, tile_runs.p);
        SF_CHECK_LAUNCH();
    }
    if ((rc = exclusive_scan_u32(tile_runs.p, tile_start.p, n_tiles, st, false))) return rc;
    unsigned long long n_runs = 0;
    SF_HIP(hipMemcpyAsync(&n_runs, tile_start.p + n_tiles, 8, hipMemcpyDeviceToHost, st));
    if (M) {
        hipLaunchKernelGGL(k_cov_summary, dim3((unsigned)((M + kBlock / kWave - 1) / (kBlock / kWave))), dim3(kBlock), 0, st, (const uint64_t*)c->slot.p,
                           (const uint64_t*)c->base.p, M, c->col.p, c->col.p + M, c->col.p + 2 * M, ctr.p);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipStreamSynchronize(st));
    SF_REQUIRE(n_runs <= N, SFGPU_ERR_HIP, "sfgpu_cov_finish: the run count lost its way");
    const uint64_t room = n_runs ? n_runs : 1;
    if ((rc = c->r_tid.reserve(room, st, false)) || (rc = c->r_start.reserve(room, st, false)) || (rc = c->r_end.reserve(room, st, false)) ||
        (rc = c->r_sum.reserve(room, st, false)))
        return rc;
    if (n_runs) {
        SF_HIP(hipMemsetAsync(c->r_end.p, 0, n_runs * 4, st));
        hipLaunchKernelGGL(k_cov_run_write, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, (const uint64_t*)c->slot.p, N, (const uint64_t*)c->base.p, M,
                           (const uint64_t*)tile_start.p, (uint64_t)n_runs, c->r_tid.p, c->r_start.p, c->r_end.p, c->r_sum.p);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipEventRecord(ev[1], st));
    unsigned long long h_ctr[kCovFinishCounters] = {0, 0};
    SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    c->res = sfgpu_cov_result{};
    c->res.n_runs = n_runs; c->res.bases_covered = h_ctr[kCovCovered]; c->res.bases_total = N - M; c->res.residue = h_ctr[kCovResidue];
    c->res.state_bytes = c->state_bytes();
    add_elapsed(&c->res.finish_ms, ev[0], ev[1]);
    *out = c->res;
    return SFGPU_OK;
}

extern "C" int sfgpu_cov_runs(sfgpu_cov* c, uint32_t* d_tid, uint32_t* d_start, uint32_t* d_end, uint64_t* d_sum) {
    SF_REQUIRE(c, SFGPU_ERR_INVALID, "sfgpu_cov_runs: null handle");
    SF_REQUIRE(c->finished, SFGPU_ERR_STATE, "sfgpu_cov_runs: called before sfgpu_cov_finish");
    const uint64_t n = c->res.n_runs;
    if (!n) return SFGPU_OK;
    if (d_tid) SF_HIP(hipMemcpy(d_tid, c->r_tid.p, n * 4, hipMemcpyDeviceToDevice));
    if (d_start) SF_HIP(hipMemcpy(d_start, c->r_start.p, n * 4, hipMemcpyDeviceToDevice));
    if (d_end) SF_HIP(hipMemcpy(d_end, c->r_end.p, n * 4, hipMemcpyDeviceToDevice));
    if (d_sum) SF_HIP(hipMemcpy(d_sum, c->r_sum.p, n * 8, hipMemcpyDeviceToDevice));
    SF_HIP(hipDeviceSynchronize());
    return SFGPU_OK;
}

extern "C" int sfgpu_cov_summary(sfgpu_cov* c, double* d_covered_fraction, double* d_mean, double* d_max) {
    SF_REQUIRE(c, SFGPU_ERR_INVALID, "sfgpu_cov_summary: null handle");
    SF_REQUIRE(c->finished, SFGPU_ERR_STATE, "sfgpu_cov_summary: called before sfgpu_cov_finish");
    const uint64_t M = c->M;
    if (!M) return SFGPU_OK;
    if (d_covered_fraction) SF_HIP(hipMemcpy(d_covered_fraction, c->col.p, M * 8, hipMemcpyDeviceToDevice));
    if (d_mean) SF_HIP(hipMemcpy(d_mean, c->col.p + M, M * 8, hipMemcpyDeviceToDevice));
    if (d_max) SF_HIP(hipMemcpy(d_max, c->col.p + 2 * M, M * 8, hipMemcpyDeviceToDevice));
    SF_HIP(hipDeviceSynchronize());
    return SFGPU_OK;
}

// the checks of the handle and the result's fields around covwrite.h's cov_write
static int cov_write_handle(const char* who, sfgpu_cov* c, const char* d_names, const uint64_t* d_name_off, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
                            sfgpu_bgzw* z, sfgpu_cov_result* out, sfgpu_stream stream) {
    auto fail = [&](int code, const char* what) -> int { set_error("%s: %s", who, what); return code; };
    if (!c || !out) return fail(SFGPU_ERR_INVALID, "null handle or result");
    if (!c->finished) return fail(SFGPU_ERR_STATE, "called before sfgpu_cov_finish");
    *out = c->res;
    const CovRunTable T = {c->r_tid.p, c->r_start.p, c->r_end.p, c->r_sum.p, c->res.n_runs, c->M};
    CovWriteStats w;
    const int rc = cov_write(who, T, d_names, d_name_off, chunk_bytes, sink, user, z, &w, stream);
    out->n_bytes = w.n_bytes; out->n_chunks = w.n_chunks; out->max_row_bytes = w.max_row_bytes;
    out->format_ms = w.format_ms; out->d2h_ms = w.d2h_ms; out->sink_ms = w.sink_ms;
    return rc;
}

extern "C" int sfgpu_cov_write_text(sfgpu_cov* c, const char* d_names, const uint64_t* d_name_off, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
                                    sfgpu_cov_result* out, sfgpu_stream stream) {
    return cov_write_handle("sfgpu_cov_write_text", c, d_names, d_name_off, chunk_bytes, sink, user, nullptr, out, stream);
}

extern "C" int sfgpu_cov_write_bgzf(sfgpu_cov* c, const char* d_names, const uint64_t* d_name_off, uint64_t chunk_bytes, sfgpu_bgzw* z, sfgpu_cov_result* out,
                                    sfgpu_stream stream) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_cov_write_bgzf: null BGZF handle");
    return cov_write_handle("sfgpu_cov_write_bgzf", c, d_names, d_name_off, chunk_bytes, nullptr, nullptr, z, out, stream);
}
