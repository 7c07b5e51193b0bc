// coverage_genome.hip -- sfgpu_covg_*: a finished transcript coverage (coverage.hip) projected through the exon blocks onto the
// chromosomes, summed per genomic base, its runs and the bedGraph file.  WHAT a piece, an event, a sum, a run and a row are is
// csrc/covgfmt.h, stated once and run here unchanged; this file is only the way the work is laid out.
//
//   open            k_covg_check_off: a lane per transcript, the offsets start at 0 and never decrease; the model is copied onto the
//                   handle and the block lengths are scanned into 64-bit prefix sums (block e of transcript t lies at prefix[e] -
//                   prefix[exon_off[t]]); k_covg_check_model: a lane per transcript and per block runs covg_block_ok.  The lowest
//                   offending transcript leaves by atomicMin.
//   k_covg_count    a lane per transcript run: the blocks holding its first and its last base by binary search of the prefix sums.
//                   Blocks are never empty, so the pieces are the blocks from the first to the last: no walk.  The counters leave as
//                   one integer atomic a wavefront.
//   k_covg_emit     after the scan of the counts, a lane per run writes the two events of each of its pieces to their places; a run of
//                   more than kCovgShort pieces goes on a list instead, at the place a scan of the "long" flags gives it, and
//                   k_covg_emit_long gives each of those a wavefront, a lane a piece.
//   sort            sort_pairs_u64_u32 over the keys' used bits with the event index as payload; k_covg_gather brings the deltas
//                   into key order and inclusive_scan_u64 sums them.  After a key's LAST event the scan reads the sum that holds from
//                   that key on, whatever order the key's events came in: the fold of equal keys is the difference of the scan across
//                   them, and no sum is ever added with an atomic.
//   runs            k_covg_tail_flag marks the last event of every key; scan; k_covg_tail_compact leaves (key, sum) per distinct key.
//                   A key whose sum equals the one before it had delta 0 and does nothing.  k_covg_open_flag marks the keys that open a
//                   run (sum != 0 and != the sum before); scan; k_covg_run_write writes (chrom, start, sum) where a run opens and the
//                   end where one closes: the run that closes at a key is the last one opened before it.  A chromosome's deltas sum
//                   to 0, so its last key closes its last run.
//   write           covwrite.h's cov_write over the run table, the chromosomes' names naming the rows.
#include "common.h"
#include "covgfmt.h"
#include "covwrite.h"
#include "primitives.h"
#include "texttile.h"

struct sfgpu_covg {
    uint64_t M = 0, E = 0;
    uint32_t n_chrom = 0;
    uint64_t cap = sfgpu::kCovgMaxEvents;                  // projections refuse this many events or more
    sfgpu::DevBuf<uint8_t> status;
    sfgpu::DevBuf<int32_t> chrom;
    sfgpu::DevBuf<int8_t> strand;
    sfgpu::DevBuf<uint64_t> exon_off, prefix;              // exon_off[M + 1], prefix[E + 1]
    sfgpu::DevBuf<uint32_t> exon_start, exon_len;          // [E], [E + 1]
    bool projected = false;
    sfgpu_covg_result res{};
    sfgpu::DevBuf<uint32_t> r_chrom, r_start, r_end;       // the runs
    sfgpu::DevBuf<uint64_t> r_sum;
    uint64_t state_bytes() const {
        return status.cap + strand.cap + 4 * (chrom.cap + exon_start.cap + exon_len.cap + r_chrom.cap + r_start.cap + r_end.cap) +
               8 * (exon_off.cap + prefix.cap + r_sum.cap);
    }
};

namespace sfgpu {
namespace {

using textchunks::kBlock;
using textchunks::grid_of;

constexpr uint32_t kCovgShort = 8;                         // runs of more pieces are emitted by a wavefront
enum { kCgPieces = 0, kCgRunsUnplaced, kCgBasesUnplaced, kCgOffModel, kCgLong, kCgPlaced, kCgMismatch, kCgKeys, kCgCovered, kCgCounters };

__device__ __forceinline__ unsigned long long covg_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ void covg_count_out(unsigned long long v, unsigned long long* __restrict__ at) {
    v = covg_wave_sum(v);
    if ((threadIdx.x & (kWave - 1)) == 0 && v) atomicAdd(at, v);
}

__global__ void __launch_bounds__(kBlock)
k_covg_check_off(const uint64_t* __restrict__ exon_off, uint64_t M, unsigned long long* __restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= M) return;
    if (exon_off[t] > exon_off[t + 1] || (t == 0 && exon_off[0] != 0)) atomicMin(bad, (unsigned long long)t);
}

// lane i checks transcript i (i < M) and block i (i < E); the offsets are known to ascend from 0 to E
__global__ void __launch_bounds__(kBlock)
k_covg_check_model(const uint8_t* __restrict__ status, const int32_t* __restrict__ chrom, const int8_t* __restrict__ strand, const uint64_t* __restrict__ exon_off,
                   const uint32_t* __restrict__ exon_start, const uint32_t* __restrict__ exon_len, uint64_t M, uint64_t E, uint32_t n_chrom,
                   unsigned long long* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < M && status[i] == 0) {
        const int32_t c = chrom[i];
        const int s = strand[i];
        if (c < 0 || (uint32_t)c >= n_chrom || (s != 1 && s != -1)) atomicMin(bad, (unsigned long long)i);
    }
    if (i >= E) return;
    const uint64_t t = textchunks::holder_of(exon_off, M, i);          // the last transcript whose blocks start at or before i: the one that holds it
    const bool placed = status[t] == 0, next = placed && i + 1 < exon_off[t + 1];
    if (!covg_block_ok(exon_start[i], exon_len[i], next, next ? exon_start[i + 1] : 0, next ? exon_len[i + 1] : 0, placed ? (int)strand[t] : 1))
        atomicMin(bad, (unsigned long long)t);
}

// base[t + 1] - base[t] - 1 is transcript t's length (coverage.hip's slots)
__global__ void __launch_bounds__(kBlock)
k_covg_transcripts(const uint8_t* __restrict__ status, const uint64_t* __restrict__ exon_off, const uint64_t* __restrict__ prefix, const uint64_t* __restrict__ base,
                   uint64_t M, unsigned long long* __restrict__ ctr) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long placed = 0, mism = 0;
    if (t < M && status[t] == 0) {
        placed = 1;
        mism = prefix[exon_off[t + 1]] - prefix[exon_off[t]] != base[t + 1] - base[t] - 1;
    }
    covg_count_out(placed, &ctr[kCgPlaced]);
    covg_count_out(mism, &ctr[kCgMismatch]);
}

// every r_tid is below M (sfgpu_cov_finish wrote it, and the two handles' M agree)
__global__ void __launch_bounds__(kBlock)
k_covg_count(const uint32_t* __restrict__ r_tid, const uint32_t* __restrict__ r_start, const uint32_t* __restrict__ r_end, uint64_t n_runs,
             const uint8_t* __restrict__ status, const uint64_t* __restrict__ exon_off, const uint64_t* __restrict__ prefix, uint32_t* __restrict__ first,
             uint32_t* __restrict__ n_pieces, uint32_t* __restrict__ long_flag, unsigned long long* __restrict__ ctr) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    CovgCount c = {0, 0, 0, 0};
    unsigned long long is_long = 0;
    if (r < n_runs) {
        const uint64_t t = r_tid[r], a = r_start[r];
        uint64_t b = r_end[r];
        uint32_t np = 0, i0 = 0;
        if (status[t] != 0) { c.runs_unplaced = 1; c.bases_unplaced = b - a; }
        else {
            const uint64_t e0 = exon_off[t], n = exon_off[t + 1] - e0, p0 = prefix[e0], L = prefix[e0 + n] - p0;
            if (b > L) { c.bases_off_model = b - (a > L ? a : L); b = L; }
            if (a < b) {                                   // then L > 0 and n >= 1
                const uint64_t f = textchunks::holder_of(prefix + e0, n, p0 + a), l = textchunks::holder_of(prefix + e0, n, p0 + b - 1);
                i0 = (uint32_t)(e0 + f);
                np = (uint32_t)(l - f + 1);
            }
        }
        c.pieces = np; is_long = np > kCovgShort;
        first[r] = i0; n_pieces[r] = np; long_flag[r] = (uint32_t)is_long;
    }
    covg_count_out(c.pieces, &ctr[kCgPieces]);
    covg_count_out(c.runs_unplaced, &ctr[kCgRunsUnplaced]);
    covg_count_out(c.bases_unplaced, &ctr[kCgBasesUnplaced]);
    covg_count_out(c.bases_off_model, &ctr[kCgOffModel]);
    covg_count_out(is_long, &ctr[kCgLong]);
}

struct CovgEmit {                                          // what the two emit kernels read and write
    const uint32_t *r_tid, *r_start, *r_end;
    const uint64_t* r_sum;
    const int32_t* chrom;
    const int8_t* strand;
    const uint64_t *exon_off, *prefix;
    const uint32_t *exon_start, *exon_len, *first, *n_pieces;
    const uint64_t* piece_start;
    uint64_t* key;
    uint64_t* delta;
    uint32_t* idx;
    uint64_t n_events;
};

// piece j of run r: the two events at 2 (piece_start[r] + j)
__device__ __forceinline__ void covg_emit_piece(const CovgEmit& E, uint64_t r, uint32_t j) {
    const uint64_t t = E.r_tid[r], e0 = E.exon_off[t], p0 = E.prefix[e0], L = E.prefix[E.exon_off[t + 1]] - p0;
    const uint64_t a = E.r_start[r], b = E.r_end[r] < L ? E.r_end[r] : L, s = E.r_sum[r];
    const uint64_t e = (uint64_t)E.first[r] + j, at = 2 * (E.piece_start[r] + j);
    if (at + 1 >= E.n_events) return;                      // (never: the places were counted from the same figures)
    uint64_t lo, hi;
    covg_piece(a, b, E.prefix[e] - p0, E.exon_start[e], E.exon_len[e], E.strand[t], &lo, &hi);
    const uint32_t c = (uint32_t)E.chrom[t];
    E.key[at] = covg_key(c, lo); E.delta[at] = s; E.idx[at] = (uint32_t)at;
    E.key[at + 1] = covg_key(c, hi); E.delta[at + 1] = 0ull - s; E.idx[at + 1] = (uint32_t)(at + 1);
}

__global__ void __launch_bounds__(kBlock)
k_covg_emit(CovgEmit E, uint64_t n_runs, const uint32_t* __restrict__ long_pos, uint32_t* __restrict__ long_list, uint64_t n_long) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_runs) return;
    const uint32_t np = E.n_pieces[r];
    if (np > kCovgShort) {
        const uint32_t k = long_pos[r];                    // the long runs before this one
        if (k < n_long) long_list[k] = (uint32_t)r;
        return;
    }
    for (uint32_t j = 0; j < np; ++j) covg_emit_piece(E, r, j);
}

__global__ void __launch_bounds__(kBlock)
k_covg_emit_long(CovgEmit E, const uint32_t* __restrict__ long_list, uint64_t n_long) {
    const uint64_t w = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (w >= n_long) return;                               // (a whole wavefront)
    const uint64_t r = long_list[w];
    const uint32_t np = E.n_pieces[r];
    for (uint32_t j = threadIdx.x & (kWave - 1); j < np; j += kWave) covg_emit_piece(E, r, j);
}

__global__ void __launch_bounds__(kBlock)
k_covg_gather(const uint32_t* __restrict__ idx, const uint64_t* __restrict__ delta, uint64_t n, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = idx[i] < n ? delta[idx[i]] : 0;
}

__global__ void __launch_bounds__(kBlock)
k_covg_tail_flag(const uint64_t* __restrict__ key, uint64_t n, uint32_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) flag[i] = (i + 1 == n || key[i + 1] != key[i]) ? 1u : 0u;
}

__global__ void __launch_bounds__(kBlock)
k_covg_tail_compact(const uint64_t* __restrict__ key, const uint64_t* __restrict__ sum, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint64_t n,
                    uint64_t n_keys, uint64_t* __restrict__ K, uint64_t* __restrict__ V) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !flag[i] || pos[i] >= n_keys) return;
    K[pos[i]] = key[i]; V[pos[i]] = sum[i];
}

__global__ void __launch_bounds__(kBlock)
k_covg_open_flag(const uint64_t* __restrict__ V, uint64_t n, uint32_t* __restrict__ flag, unsigned long long* __restrict__ ctr) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long changes = 0;
    if (j < n) {
        const uint64_t prev = j ? V[j - 1] : 0;
        changes = V[j] != prev;
        flag[j] = (changes && V[j] != 0) ? 1u : 0u;
    }
    covg_count_out(changes, &ctr[kCgKeys]);
}

__global__ void __launch_bounds__(kBlock)
k_covg_run_write(const uint64_t* __restrict__ K, const uint64_t* __restrict__ V, const uint32_t* __restrict__ pos, uint64_t n, uint64_t n_runs,
                 uint32_t* __restrict__ r_chrom, uint32_t* __restrict__ r_start, uint32_t* __restrict__ r_end, uint64_t* __restrict__ r_sum) {
    const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const uint64_t prev = j ? V[j - 1] : 0;
    if (V[j] == prev) return;
    const uint64_t k = pos[j];                             // runs opened before key j
    if (prev != 0 && k >= 1 && k <= n_runs) r_end[k - 1] = (uint32_t)K[j];
    if (V[j] != 0 && k < n_runs) { r_chrom[k] = (uint32_t)(K[j] >> 32); r_start[k] = (uint32_t)K[j]; r_sum[k] = V[j]; }
}

__global__ void __launch_bounds__(kBlock)
k_covg_bases(const uint32_t* __restrict__ r_start, const uint32_t* __restrict__ r_end, uint64_t n_runs, unsigned long long* __restrict__ ctr) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    covg_count_out(r < n_runs ? (unsigned long long)(r_end[r] - r_start[r]) : 0ull, &ctr[kCgCovered]);
}

template <typename T>
void take(DevBuf<T>& into, DevBuf<T>& from) {
    T* p = into.p; const uint64_t cap = into.cap;
    into.p = from.p; into.cap = from.cap;
    from.p = p; from.cap = cap;
}

int covg_write(const char* who, sfgpu_covg* g, const char* d_names, const uint64_t* d_name_off, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
               sfgpu_bgzw* z, sfgpu_covg_result* out, sfgpu_stream stream) {
    auto fail = [&](int code, const char* what) -> int { set_error("%s: %s", who, what); return code; };
    if (!g || !out) return fail(SFGPU_ERR_INVALID, "null handle or result");
    if (!g->projected) return fail(SFGPU_ERR_STATE, "called before sfgpu_covg_project");
    *out = g->res;
    const CovRunTable T = {g->r_chrom.p, g->r_start.p, g->r_end.p, g->r_sum.p, g->res.n_runs, g->n_chrom};
    CovWriteStats w;
    const int rc = cov_write(who, T, d_names, d_name_off, chunk_bytes, sink, user, z, &w, stream);
    out->n_bytes = w.n_bytes; out->n_chunks = w.n_chunks; out->max_row_bytes = w.max_row_bytes;
    out->format_ms = w.format_ms; out->d2h_ms = w.d2h_ms; out->sink_ms = w.sink_ms;
    return rc;
}

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_covg_open(sfgpu_covg** out, const uint8_t* d_status, const int32_t* d_chrom, const int8_t* d_strand, const uint64_t* d_exon_off,
                               const uint32_t* d_exon_start, const uint32_t* d_exon_len, uint64_t M, uint32_t n_chrom, sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_covg_open: null handle pointer");
    *out = nullptr;
    SF_REQUIRE(d_exon_off && ((d_status && d_chrom && d_strand) || M == 0), SFGPU_ERR_INVALID, "sfgpu_covg_open: null model array");
    SF_REQUIRE(M < 0xffffffffull, SFGPU_ERR_RANGE, "sfgpu_covg_open: the transcripts must be fewer than 2^32 - 1");
    hipStream_t st = as_stream(stream);
    sfgpu_covg* g = new sfgpu_covg;
    struct Guard { sfgpu_covg* g; ~Guard() { delete g; } } guard{g};
    DevBuf<unsigned long long> bad;
    StreamSyncOnExit sync_first{st};          // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    int rc;
    if ((rc = bad.reserve(1, st, false))) return rc;
    unsigned long long h_bad = ~0ull, h_E = 0;
    SF_HIP(hipMemcpyAsync(bad.p, &h_bad, 8, hipMemcpyHostToDevice, st));
    if (M) {
        hipLaunchKernelGGL(k_covg_check_off, dim3(grid_of(M)), dim3(kBlock), 0, st, d_exon_off, M, bad.p);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipMemcpyAsync(&h_bad, bad.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_E, d_exon_off + M, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h_bad != ~0ull) {
        set_error("sfgpu_covg_open: the block offsets of transcript %llu decrease or do not start at 0", h_bad);
        return SFGPU_ERR_INVALID;
    }
    SF_REQUIRE(M || h_E == 0, SFGPU_ERR_INVALID, "sfgpu_covg_open: blocks without a transcript");
    SF_REQUIRE(h_E < 0xffffffffull, SFGPU_ERR_RANGE, "sfgpu_covg_open: the blocks must be fewer than 2^32 - 1");
    const uint64_t E = h_E;
    SF_REQUIRE(E == 0 || (d_exon_start && d_exon_len), SFGPU_ERR_INVALID, "sfgpu_covg_open: null block array");
    if ((rc = g->status.reserve(M + 1, st, false)) || (rc = g->chrom.reserve(M + 1, st, false)) || (rc = g->strand.reserve(M + 1, st, false)) ||
        (rc = g->exon_off.reserve(M + 1, st, false)) || (rc = g->exon_start.reserve(E + 1, st, false)) || (rc = g->exon_len.reserve(E + 1, st, false)) ||
        (rc = g->prefix.reserve(E + 1, st, false)))
        return rc;
    if (M) {
        SF_HIP(hipMemcpyAsync(g->status.p, d_status, M, hipMemcpyDeviceToDevice, st));
        SF_HIP(hipMemcpyAsync(g->chrom.p, d_chrom, M * 4, hipMemcpyDeviceToDevice, st));
        SF_HIP(hipMemcpyAsync(g->strand.p, d_strand, M, hipMemcpyDeviceToDevice, st));
    }
    SF_HIP(hipMemcpyAsync(g->exon_off.p, d_exon_off, (M + 1) * 8, hipMemcpyDeviceToDevice, st));
    SF_HIP(hipMemsetAsync(g->exon_len.p, 0, (E + 1) * 4, st));
    if (E) {
        SF_HIP(hipMemcpyAsync(g->exon_start.p, d_exon_start, E * 4, hipMemcpyDeviceToDevice, st));
        SF_HIP(hipMemcpyAsync(g->exon_len.p, d_exon_len, E * 4, hipMemcpyDeviceToDevice, st));
    }
    if ((rc = exclusive_scan_u32(g->exon_len.p, g->prefix.p, E, st, false))) return rc;
    const uint64_t lanes = M > E ? M : E;
    if (lanes) {
        hipLaunchKernelGGL(k_covg_check_model, dim3(grid_of(lanes)), dim3(kBlock), 0, st, (const uint8_t*)g->status.p, (const int32_t*)g->chrom.p,
                           (const int8_t*)g->strand.p, (const uint64_t*)g->exon_off.p, (const uint32_t*)g->exon_start.p, (const uint32_t*)g->exon_len.p, M, E, n_chrom,
                           bad.p);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipMemcpyAsync(&h_bad, bad.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h_bad != ~0ull) {
        set_error("sfgpu_covg_open: the model of transcript %llu is refused (a chromosome that is none of the %u, a strand that is neither +1 nor -1, an "
                  "empty block, a block beyond 2^32 - 1, or blocks that overlap or run against the strand)", h_bad, n_chrom);
        return SFGPU_ERR_INVALID;
    }
    g->M = M; g->E = E; g->n_chrom = n_chrom;
    guard.g = nullptr;
    *out = g;
    return SFGPU_OK;
}

extern "C" int sfgpu_covg_close(sfgpu_covg* g) {
    if (!g) return SFGPU_OK;
    (void)hipDeviceSynchronize();
    delete g;
    return SFGPU_OK;
}

extern "C" int sfgpu_covg_event_cap(sfgpu_covg* g, uint64_t cap) {
    SF_REQUIRE(g, SFGPU_ERR_INVALID, "sfgpu_covg_event_cap: null handle");
    g->cap = cap && cap < kCovgMaxEvents ? cap : kCovgMaxEvents;
    return SFGPU_OK;
}

extern "C" int sfgpu_covg_project(sfgpu_covg* g, sfgpu_cov* c, sfgpu_covg_result* out, sfgpu_stream stream) {
    SF_REQUIRE(g && c && out, SFGPU_ERR_INVALID, "sfgpu_covg_project: null pointer");
    SF_REQUIRE(c->finished, SFGPU_ERR_STATE, "sfgpu_covg_project: called before sfgpu_cov_finish");
    if (c->M != g->M) {
        set_error("sfgpu_covg_project: the coverage has %llu transcripts, the model %llu", (unsigned long long)c->M, (unsigned long long)g->M);
        return SFGPU_ERR_INVALID;
    }
    hipStream_t st = as_stream(stream);
    const uint64_t M = g->M, R = c->res.n_runs;
    DevBuf<uint32_t> first, n_pieces, long_flag, long_pos, idx_a, idx_b, long_list, n_chrom_runs, n_start, n_end;
    DevBuf<uint64_t> piece_start, key_a, key_b, delta, sum, n_sum;
    DevBuf<unsigned long long> ctr;
    CallScope scope;                          // (declared after the buffers: it drains the stream before scratch goes back)
    SF_HIP(scope.adopt(st));
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // start; events emitted; sorted; summed; runs written
    for (auto& e : ev) SF_HIP(scope.event(&e));
    int rc;
    if ((rc = ctr.reserve(kCgCounters, st, false)) || (rc = first.reserve(R + 1, st, false)) || (rc = n_pieces.reserve(R + 1, st, false)) ||
        (rc = long_flag.reserve(R + 1, st, false)) || (rc = long_pos.reserve(R + 1, st, false)) || (rc = piece_start.reserve(R + 1, st, false)))
        return rc;
    SF_HIP(hipEventRecord(ev[0], st));
    SF_HIP(hipMemsetAsync(ctr.p, 0, kCgCounters * sizeof(unsigned long long), st));
    SF_HIP(hipMemsetAsync(n_pieces.p, 0, (R + 1) * 4, st));
    SF_HIP(hipMemsetAsync(long_flag.p, 0, (R + 1) * 4, st));
    if (M) {
        hipLaunchKernelGGL(k_covg_transcripts, dim3(grid_of(M)), dim3(kBlock), 0, st, (const uint8_t*)g->status.p, (const uint64_t*)g->exon_off.p,
                           (const uint64_t*)g->prefix.p, (const uint64_t*)c->base.p, M, ctr.p);
        SF_CHECK_LAUNCH();
    }
    if (R) {
        hipLaunchKernelGGL(k_covg_count, dim3(grid_of(R)), dim3(kBlock), 0, st, (const uint32_t*)c->r_tid.p, (const uint32_t*)c->r_start.p, (const uint32_t*)c->r_end.p, R,
                           (const uint8_t*)g->status.p, (const uint64_t*)g->exon_off.p, (const uint64_t*)g->prefix.p, first.p, n_pieces.p, long_flag.p, ctr.p);
        SF_CHECK_LAUNCH();
    }
    if ((rc = exclusive_scan_u32(n_pieces.p, piece_start.p, R, st, false))) return rc;
    if ((rc = exclusive_scan_u32_u32(long_flag.p, long_pos.p, R, st))) return rc;
    unsigned long long h[kCgCounters] = {0}, h_pieces = 0;
    SF_HIP(hipMemcpyAsync(h, ctr.p, sizeof h, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_pieces, piece_start.p + R, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    SF_REQUIRE(h_pieces == h[kCgPieces], SFGPU_ERR_HIP, "sfgpu_covg_project: the piece count lost its way");
    if (!(h_pieces < g->cap / 2 + (g->cap & 1))) {         // 2 pieces < cap
        set_error("sfgpu_covg_project: %llu events, which must stay below %llu", 2 * h_pieces, (unsigned long long)g->cap);
        return SFGPU_ERR_RANGE;
    }
    const uint64_t Ne = 2 * h_pieces, n_long = h[kCgLong];
    if ((rc = key_a.reserve(Ne + 1, st, false)) || (rc = key_b.reserve(Ne + 1, st, false)) || (rc = idx_a.reserve(Ne + 1, st, false)) ||
        (rc = idx_b.reserve(Ne + 1, st, false)) || (rc = delta.reserve(Ne + 1, st, false)) || (rc = sum.reserve(Ne + 1, st, false)) ||
        (rc = long_list.reserve(n_long + 1, st, false)))
        return rc;
    uint64_t peak = g->state_bytes() + 8 * (ctr.cap + piece_start.cap + key_a.cap + key_b.cap + delta.cap + sum.cap) +
                    4 * (first.cap + n_pieces.cap + long_flag.cap + long_pos.cap + idx_a.cap + idx_b.cap + long_list.cap);
    uint64_t Nd = 0, n_runs = 0;
    if (Ne) {
        const CovgEmit E = {c->r_tid.p, c->r_start.p, c->r_end.p, c->r_sum.p, g->chrom.p, g->strand.p, g->exon_off.p, g->prefix.p, g->exon_start.p, g->exon_len.p,
                            first.p, n_pieces.p, piece_start.p, key_a.p, delta.p, idx_a.p, Ne};
        hipLaunchKernelGGL(k_covg_emit, dim3(grid_of(R)), dim3(kBlock), 0, st, E, R, (const uint32_t*)long_pos.p, long_list.p, n_long);
        SF_CHECK_LAUNCH();
        if (n_long) {
            hipLaunchKernelGGL(k_covg_emit_long, dim3((unsigned)((n_long + kBlock / kWave - 1) / (kBlock / kWave))), dim3(kBlock), 0, st, E,
                               (const uint32_t*)long_list.p, n_long);
            SF_CHECK_LAUNCH();
        }
        SF_HIP(hipEventRecord(ev[1], st));
        int end_bit = 33;
        while (end_bit < 64 && (1ull << (end_bit - 32)) < (uint64_t)g->n_chrom) ++end_bit;
        if ((rc = sort_pairs_u64_u32(key_a.p, key_b.p, idx_a.p, idx_b.p, Ne, st, end_bit, false))) return rc;
        SF_HIP(hipEventRecord(ev[2], st));
        hipLaunchKernelGGL(k_covg_gather, dim3(grid_of(Ne)), dim3(kBlock), 0, st, (const uint32_t*)idx_b.p, (const uint64_t*)delta.p, Ne, sum.p);
        SF_CHECK_LAUNCH();
        if ((rc = inclusive_scan_u64(sum.p, Ne, st))) return rc;
        SF_HIP(hipEventRecord(ev[3], st));
        // the last event of every key -> (K, V) = (key_a, delta), both free by now; the flags in idx_a, their places in idx_b
        SF_HIP(hipMemsetAsync(idx_a.p, 0, (Ne + 1) * 4, st));
        hipLaunchKernelGGL(k_covg_tail_flag, dim3(grid_of(Ne)), dim3(kBlock), 0, st, (const uint64_t*)key_b.p, Ne, idx_a.p);
        SF_CHECK_LAUNCH();
        if ((rc = exclusive_scan_u32_u32(idx_a.p, idx_b.p, Ne, st))) return rc;
        uint32_t h_nd = 0;
        SF_HIP(hipMemcpyAsync(&h_nd, idx_b.p + Ne, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        Nd = h_nd;
        SF_REQUIRE(Nd >= 1 && Nd <= Ne, SFGPU_ERR_HIP, "sfgpu_covg_project: the key count lost its way");
        hipLaunchKernelGGL(k_covg_tail_compact, dim3(grid_of(Ne)), dim3(kBlock), 0, st, (const uint64_t*)key_b.p, (const uint64_t*)sum.p, (const uint32_t*)idx_a.p,
                           (const uint32_t*)idx_b.p, Ne, Nd, key_a.p, delta.p);
        SF_CHECK_LAUNCH();
        // the keys that open a run, and their places
        SF_HIP(hipMemsetAsync(idx_a.p, 0, (Nd + 1) * 4, st));
        hipLaunchKernelGGL(k_covg_open_flag, dim3(grid_of(Nd)), dim3(kBlock), 0, st, (const uint64_t*)delta.p, Nd, idx_a.p, ctr.p);
        SF_CHECK_LAUNCH();
        if ((rc = exclusive_scan_u32_u32(idx_a.p, idx_b.p, Nd, st))) return rc;
        uint32_t h_nr = 0;
        SF_HIP(hipMemcpyAsync(&h_nr, idx_b.p + Nd, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        n_runs = h_nr;
        SF_REQUIRE(n_runs <= Nd, SFGPU_ERR_HIP, "sfgpu_covg_project: the run count lost its way");
    }
    const uint64_t room = n_runs ? n_runs : 1;
    if ((rc = n_chrom_runs.reserve(room, st, false)) || (rc = n_start.reserve(room, st, false)) || (rc = n_end.reserve(room, st, false)) ||
        (rc = n_sum.reserve(room, st, false)))
        return rc;
    peak += 4 * (n_chrom_runs.cap + n_start.cap + n_end.cap) + 8 * n_sum.cap;
    if (n_runs) {
        SF_HIP(hipMemsetAsync(n_end.p, 0, n_runs * 4, st));
        hipLaunchKernelGGL(k_covg_run_write, dim3(grid_of(Nd)), dim3(kBlock), 0, st, (const uint64_t*)key_a.p, (const uint64_t*)delta.p, (const uint32_t*)idx_b.p, Nd,
                           n_runs, n_chrom_runs.p, n_start.p, n_end.p, n_sum.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_covg_bases, dim3(grid_of(n_runs)), dim3(kBlock), 0, st, (const uint32_t*)n_start.p, (const uint32_t*)n_end.p, n_runs, ctr.p);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipEventRecord(ev[4], st));
    SF_HIP(hipMemcpyAsync(h, ctr.p, sizeof h, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    // nothing was refused: the handle takes the new runs, the old ones go back with the scratch
    take(g->r_chrom, n_chrom_runs); take(g->r_start, n_start); take(g->r_end, n_end); take(g->r_sum, n_sum);
    sfgpu_covg_result& r = g->res;
    r = sfgpu_covg_result{};
    r.n_pieces = h_pieces; r.n_events = Ne; r.n_keys = h[kCgKeys]; r.n_runs = n_runs; r.bases_covered = h[kCgCovered];
    r.runs_unplaced = h[kCgRunsUnplaced]; r.bases_unplaced = h[kCgBasesUnplaced]; r.bases_off_model = h[kCgOffModel];
    r.transcripts_placed = h[kCgPlaced]; r.transcripts_length_mismatch = h[kCgMismatch];
    r.state_bytes = peak;
    add_elapsed(&r.project_ms, ev[0], ev[4]);
    if (Ne) {
        add_elapsed(&r.emit_ms, ev[0], ev[1]); add_elapsed(&r.sort_ms, ev[1], ev[2]);
        add_elapsed(&r.sum_ms, ev[2], ev[3]); add_elapsed(&r.runs_ms, ev[3], ev[4]);
    }
    g->projected = true;
    *out = r;
    return SFGPU_OK;
}

extern "C" int sfgpu_covg_runs(sfgpu_covg* g, uint32_t* d_chrom, uint32_t* d_start, uint32_t* d_end, uint64_t* d_sum) {
    SF_REQUIRE(g, SFGPU_ERR_INVALID, "sfgpu_covg_runs: null handle");
    SF_REQUIRE(g->projected, SFGPU_ERR_STATE, "sfgpu_covg_runs: called before sfgpu_covg_project");
    const uint64_t n = g->res.n_runs;
    if (!n) return SFGPU_OK;
    if (d_chrom) SF_HIP(hipMemcpy(d_chrom, g->r_chrom.p, n * 4, hipMemcpyDeviceToDevice));
    if (d_start) SF_HIP(hipMemcpy(d_start, g->r_start.p, n * 4, hipMemcpyDeviceToDevice));
    if (d_end) SF_HIP(hipMemcpy(d_end, g->r_end.p, n * 4, hipMemcpyDeviceToDevice));
    if (d_sum) SF_HIP(hipMemcpy(d_sum, g->r_sum.p, n * 8, hipMemcpyDeviceToDevice));
    SF_HIP(hipDeviceSynchronize());
    return SFGPU_OK;
}

extern "C" int sfgpu_covg_write_text(sfgpu_covg* g, const char* d_chrom_names, const uint64_t* d_chrom_name_off, uint64_t chunk_bytes, sfgpu_text_sink sink,
                                     void* user, sfgpu_covg_result* out, sfgpu_stream stream) {
    return covg_write("sfgpu_covg_write_text", g, d_chrom_names, d_chrom_name_off, chunk_bytes, sink, user, nullptr, out, stream);
}

extern "C" int sfgpu_covg_write_bgzf(sfgpu_covg* g, const char* d_chrom_names, const uint64_t* d_chrom_name_off, uint64_t chunk_bytes, sfgpu_bgzw* z,
                                     sfgpu_covg_result* out, sfgpu_stream stream) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_covg_write_bgzf: null BGZF handle");
    return covg_write("sfgpu_covg_write_bgzf", g, d_chrom_names, d_chrom_name_off, chunk_bytes, nullptr, nullptr, z, out, stream);
}
