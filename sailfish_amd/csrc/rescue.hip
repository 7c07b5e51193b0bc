// rescue.hip -- sfgpu_hits_rescue_mates: the missing mates of orphan-only reads, searched for on the orphans' transcripts (DESIGN
// 4.35).  WHICH reads are searched, where, what a placement is and what a rescued read's records are is csrc/rescuefmt.h, stated
// once and run here unchanged; this file is only the way the work is laid out, with the hit passes' toolkit (csrc/hitgroup.h).
//
// Only a few percent of a batch's reads are orphan-only, and one job is (window - lb) candidates times lb columns, so the work is
// laid out over JOBS and, within a job, over CANDIDATES:
//   k_rescue_flag    a lane per read: eligible?  -> jobs per read (its records, or 0); names the lowest record with tid >= M
//   scan             -> the job list's offsets; the call fails here, before anything is emitted, where a tid was bad
//   k_rescue_jobs    a lane per eligible read writes its records into the job list: no wavefront idles over mapped pairs
//   k_rescue_search  a wavefront per job (a block is one wavefront, so the LDS tile needs no wider barrier).  The missing mate is
//                    staged once in LDS, packed two bits a base beside a "no base" plane (rs_mate_word), the transcript tile by tile
//                    the same way (rs_seg_word: kRsTile candidates, one clipped 16-byte load a word).  Lane l of round k scores
//                    candidate lo + 64 k + l (rs_count_packed: per 16 columns two funnel shifts, an XOR, a popcount) and stops
//                    above the budget; one minimum of mism << 32 | x over the wavefront ends the round and tightens the budget
//                    (rs_round_done).  A mate of more than kRsMateMax bases is scored from global memory (rs_count_windows).
//   k_rescue_count   a lane per read: records out (the placed ones, or all), the read's counters
//   scan             -> the output's offsets
//   k_rescue_fill    a lane per read: pass-through, or the placed records ranked by (tid, fwd) by counting within the read
#include "common.h"
#include "mapidx.h"
#include "primitives.h"
#include "hitgroup.h"
#include "rescuefmt.h"

namespace sfgpu {

enum { kRsEligible = kHitFirstCounter, kRsOrphan, kRsWithCand, kRsCandidates, kRsReadsRescued, kRsRecRescued, kRsDropped, kRsSumMism, kRsCounters };
constexpr uint32_t kRsMaxGrid = 1u << 22;            // blocks of the search: jobs beyond are taken in a stride

__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
#pragma unroll
    for (int o = kRsLanes / 2; o > 0; o >>= 1) { const uint64_t u = __shfl_xor((unsigned long long)v, o, kRsLanes); v = u < v ? u : v; }
    return v;
}

__global__ void __launch_bounds__(kHitBlock)
k_rescue_flag(const sfgpu_hit* __restrict__ hits, uint64_t M, uint64_t n_reads, const uint32_t* __restrict__ hit_off, uint64_t n_rec,
              uint32_t* __restrict__ jobs /* [n_reads + 1] */, unsigned long long* ctr) {
    __shared__ unsigned long long s_ctr[kRsCounters];
    hit_ctr_zero(s_ctr);
    const uint64_t r = (uint64_t)blockIdx.x * kHitBlock + threadIdx.x;
    if (r == n_reads) jobs[r] = 0;
    if (r < n_reads) {
        uint64_t b, e;
        hit_range(hit_off, r, n_rec, &b, &e);
        bool eligible = e > b;
        for (uint64_t i = b; i < e; ++i) {
            if (hits[i].tid >= M) atomicMin(&ctr[kHitBadTid], (unsigned long long)i);
            eligible = eligible && rs_is_orphan(hits[i]);
        }
        jobs[r] = eligible ? (uint32_t)(e - b) : 0u;
        if (eligible) { atomicAdd(&s_ctr[kRsEligible], 1ull); atomicAdd(&s_ctr[kRsOrphan], (unsigned long long)(e - b)); }
    }
    hit_ctr_flush(s_ctr, ctr);
}

__global__ void __launch_bounds__(kHitBlock)
k_rescue_jobs(uint64_t n_reads, const uint32_t* __restrict__ hit_off, uint64_t n_rec, const uint32_t* __restrict__ jobs, const uint64_t* __restrict__ job_off,
              uint32_t* __restrict__ job_rec, uint32_t* __restrict__ job_read) {
    const uint64_t r = (uint64_t)blockIdx.x * kHitBlock + threadIdx.x;
    if (r >= n_reads || !jobs[r]) return;
    uint64_t b, e;
    hit_range(hit_off, r, n_rec, &b, &e);
    const uint64_t o = job_off[r];
    for (uint64_t i = b; i < e; ++i) { job_rec[o + (i - b)] = (uint32_t)i; job_read[o + (i - b)] = (uint32_t)r; }
}

// a job's two mates: the anchor's length, the missing mate's bases and length
struct RsMates { const char* m; uint64_t la, lb; };
__device__ __forceinline__ RsMates rs_mates_dev(const HitBatchDev& B, const sfgpu_hit& h, uint64_t r) {
    const uint64_t b1 = B.off1[r], b2 = B.off2[r], len1 = B.off1[r + 1] - b1, len2 = B.off2[r + 1] - b2;
    if (h.mate_status == 2) return RsMates{B.seq1 + b1, len2, len1};
    return RsMates{B.seq2 + b2, len1, len2};
}

__global__ void __launch_bounds__(kRsLanes)
k_rescue_search(const HitBatchDev B, uint64_t n_jobs, const uint32_t* __restrict__ job_rec, const uint32_t* __restrict__ job_read, uint32_t permille,
                uint32_t window, uint64_t* __restrict__ place /* [n_rec]: mism << 32 | x, or kRsNone */, unsigned long long* ctr) {
    __shared__ uint32_t s_mc[kRsMateWords], s_mi[kRsMateWords], s_tc[kRsSegWords], s_ti[kRsSegWords];
    const uint32_t lane = threadIdx.x;
    for (uint64_t job = blockIdx.x; job < n_jobs; job += gridDim.x) {                // (everything below is the same in every lane but `lane`)
        const uint64_t i = job_rec[job], r = job_read[job];
        const sfgpu_hit h = B.hits[i];
        const RsMates mt = rs_mates_dev(B, h, r);
        const char* t = B.tseq + B.tseq_off[h.tid];
        const uint64_t tlen = B.tlen[h.tid], lb = mt.lb;
        const bool f = h.fwd != 0, mfwd = !f;
        const RsWindow w = rs_window((int64_t)h.pos, mt.la, lb, tlen, f, window);
        uint64_t best = kRsNone;
        if (w.hi >= w.lo) {
            int64_t budget = rs_budget(lb, permille);
            const bool packed = lb <= kRsMateMax;
            const uint64_t tile = packed ? (uint64_t)kRsTile : rs_n_candidates(w);
            if (packed) for (uint32_t k = lane; k < kRsMateWords; k += kRsLanes) rs_mate_word(mt.m, lb, mfwd, k, &s_mc[k], &s_mi[k]);
            for (int64_t x0 = w.lo; x0 <= w.hi && budget >= 0; x0 += (int64_t)tile) {
                const uint64_t left = (uint64_t)(w.hi - x0) + 1ull, ncand = left < tile ? left : tile;
                if (packed) {
                    __syncthreads();                                                 // (the last tile's readers are done)
                    const uint32_t words = (uint32_t)((ncand + lb + 14u) / 16u) + 1u;      // bases 0 .. ncand + lb - 2, and one word for the shift
                    for (uint32_t q = lane; q < words; q += kRsLanes) rs_seg_word(t, tlen, x0, q, &s_tc[q], &s_ti[q]);
                    __syncthreads();
                }
                for (uint64_t c0 = 0; c0 < ncand && budget >= 0; c0 += kRsLanes) {
                    const uint64_t c = c0 + lane;
                    uint64_t key = kRsNone;
                    if (c < ncand) {
                        const int64_t x = x0 + (int64_t)c;
                        const uint64_t cnt = packed ? (uint64_t)rs_count_packed(s_tc, s_ti, (uint32_t)c, s_mc, s_mi, (uint32_t)lb, budget)
                                                    : rs_count_windows(mt.m, lb, mfwd, t, tlen, x, budget);
                        key = rs_lane_key(cnt, x, budget);
                    }
                    rs_round_done(wave_min64(key), &best, &budget);
                }
            }
            if (lane == 0) { atomicAdd(&ctr[kRsWithCand], 1ull); atomicAdd(&ctr[kRsCandidates], (unsigned long long)rs_n_candidates(w)); }
        }
        if (lane == 0) place[i] = best;
        __syncthreads();                                                             // (the next job restages the mate)
    }
}

__global__ void __launch_bounds__(kHitBlock)
k_rescue_count(uint64_t n_reads, const uint32_t* __restrict__ hit_off, uint64_t n_rec, const uint32_t* __restrict__ jobs, const uint64_t* __restrict__ place,
               uint32_t* __restrict__ cnt /* [n_reads + 1] */, unsigned long long* ctr) {
    __shared__ unsigned long long s_ctr[kRsCounters];
    hit_ctr_zero(s_ctr);
    const uint64_t r = (uint64_t)blockIdx.x * kHitBlock + threadIdx.x;
    if (r == n_reads) cnt[r] = 0;
    if (r < n_reads) {
        uint64_t b, e;
        hit_range(hit_off, r, n_rec, &b, &e);
        uint64_t placed = 0, sum = 0;
        if (jobs[r]) for (uint64_t i = b; i < e; ++i) { const uint64_t p = place[i]; if (p != kRsNone) { ++placed; sum += p >> 32; } }
        cnt[r] = (uint32_t)(placed ? placed : e - b);
        if (placed) {
            atomicAdd(&s_ctr[kRsReadsRescued], 1ull); atomicAdd(&s_ctr[kRsRecRescued], (unsigned long long)placed);
            if (e - b > placed) atomicAdd(&s_ctr[kRsDropped], (unsigned long long)(e - b - placed));
            if (sum) atomicAdd(&s_ctr[kRsSumMism], (unsigned long long)sum);
        }
    }
    hit_ctr_flush(s_ctr, ctr);
}

__global__ void __launch_bounds__(kHitBlock)
k_rescue_fill(const HitBatchDev B, uint64_t n_reads, const uint32_t* __restrict__ hit_off, uint64_t n_rec, const uint32_t* __restrict__ jobs,
              const uint64_t* __restrict__ place, const uint64_t* __restrict__ out_off, sfgpu_hit* __restrict__ hits_out, uint32_t* __restrict__ offsets_out,
              uint16_t* __restrict__ mism_out) {
    const uint64_t r = (uint64_t)blockIdx.x * kHitBlock + threadIdx.x;
    if (r > n_reads) return;
    const uint64_t o = out_off[r];
    offsets_out[r] = (uint32_t)o;
    if (r == n_reads) return;
    uint64_t b, e;
    hit_range(hit_off, r, n_rec, &b, &e);
    const bool rescued = jobs[r] && out_off[r + 1] - o < e - b;                      // fewer records go out than came in
    bool any = rescued;
    if (jobs[r] && !rescued) for (uint64_t i = b; i < e && !any; ++i) any = place[i] != kRsNone;      // ... or as many, every one placed
    if (!any) {
        for (uint64_t i = b; i < e; ++i) { hits_out[o + (i - b)] = B.hits[i]; if (mism_out) mism_out[o + (i - b)] = 0; }
        return;
    }
    for (uint64_t i = b; i < e; ++i) {
        const uint64_t p = place[i];
        if (p == kRsNone) continue;
        const sfgpu_hit h = B.hits[i];
        const uint64_t key = rs_order_key(h);
        uint64_t rank = 0;
        for (uint64_t j = b; j < e; ++j) {
            if (j == i || place[j] == kRsNone) continue;
            const uint64_t kj = rs_order_key(B.hits[j]);
            rank += kj < key || (kj == key && j < i);
        }
        const RsMates mt = rs_mates_dev(B, h, r);
        hits_out[o + rank] = rs_record(h, (int64_t)(p & 0xFFFFFFFFull), mt.la, mt.lb);
        if (mism_out) mism_out[o + rank] = vf_sat16(p >> 32);
    }
}

}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_hits_rescue_mates(const sfgpu_index* x, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                       uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_rescue_opts* opts,
                                       sfgpu_hit* d_hits_out, uint32_t* d_offsets_out, uint16_t* d_mism_out, uint64_t* n_out,
                                       sfgpu_rescue_stats* stats, sfgpu_stream stream) {
    static const char* kEntry = "sfgpu_hits_rescue_mates";
#define RS_REQUIRE(cond, what) do { if (!(cond)) { set_error("%s: %s", kEntry, what); return SFGPU_ERR_INVALID; } } while (0)
    RS_REQUIRE(x && opts && n_out && stats && d_offsets_out, "null pointer");
    RS_REQUIRE(opts->min_identity_permille <= 1000u, "min_identity_permille is 0 .. 1000");
    RS_REQUIRE(opts->window >= 1u && opts->window <= kRsMaxWindow, "window is 1 .. 2^20");
    RS_REQUIRE(d_seq2 && d_off2, "a single-end batch has no mates to rescue");
    RS_REQUIRE(n_reads == 0 || (d_seq1 && d_off1 && d_hit_offsets), "null reads");
    hipStream_t st = as_stream(stream);
    if (n_reads == 0) {
        SF_HIP(hipMemsetAsync(d_offsets_out, 0, 4, st)); SF_HIP(hipStreamSynchronize(st));
        *n_out = 0; *stats = sfgpu_rescue_stats{};
        return SFGPU_OK;
    }
    int rc;
    uint64_t n_rec = 0;
    if ((rc = hit_n_rec(d_hit_offsets, n_reads, st, &n_rec))) return rc;
    RS_REQUIRE(n_rec == 0 || (d_hits && d_hits_out), "null records");
#undef RS_REQUIRE
    DevBuf<uint32_t> jobs, cnt, job_rec, job_read; DevBuf<uint64_t> job_off, out_off, place; DevBuf<unsigned long long> ctr;
    StreamSyncOnExit sync_first{st};         // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    if ((rc = jobs.reserve((uint64_t)n_reads + 1, st, false)) || (rc = cnt.reserve((uint64_t)n_reads + 1, st, false)) || (rc = job_off.reserve((uint64_t)n_reads + 2, st, false)) ||
        (rc = out_off.reserve((uint64_t)n_reads + 2, st, false)) || (rc = place.reserve(n_rec + 1, st, false)) || (rc = ctr.reserve(kRsCounters, st, false))) return rc;
    unsigned long long h_ctr[kRsCounters] = {~0ull, ~0ull};
    SF_HIP(hipMemcpyAsync(ctr.p, h_ctr, sizeof h_ctr, hipMemcpyHostToDevice, st));
    const HitBatchDev B(x, d_seq1, d_off1, d_seq2, d_off2, d_hits);
    const dim3 per_read((unsigned)(((uint64_t)n_reads + 1 + kHitBlock - 1) / kHitBlock));
    hipLaunchKernelGGL(k_rescue_flag, per_read, dim3(kHitBlock), 0, st, d_hits, B.M, (uint64_t)n_reads, d_hit_offsets, n_rec, jobs.p, ctr.p);
    SF_CHECK_LAUNCH();
    if ((rc = exclusive_scan_u32(jobs.p, job_off.p, n_reads, st, false))) return rc;
    uint64_t n_jobs = 0, total = 0;
    SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&n_jobs, job_off.p + n_reads, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if ((rc = hit_report_bad(kEntry, h_ctr, x->M))) return rc;
    if (n_jobs) {
        if ((rc = job_rec.reserve(n_jobs, st, false)) || (rc = job_read.reserve(n_jobs, st, false))) return rc;
        hipLaunchKernelGGL(k_rescue_jobs, per_read, dim3(kHitBlock), 0, st, (uint64_t)n_reads, d_hit_offsets, n_rec, jobs.p, job_off.p, job_rec.p, job_read.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_rescue_search, dim3((unsigned)(n_jobs < kRsMaxGrid ? n_jobs : kRsMaxGrid)), dim3(kRsLanes), 0, st, B, n_jobs, job_rec.p, job_read.p,
                           opts->min_identity_permille, opts->window, place.p, ctr.p);
        SF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_rescue_count, per_read, dim3(kHitBlock), 0, st, (uint64_t)n_reads, d_hit_offsets, n_rec, jobs.p, place.p, cnt.p, ctr.p);
    SF_CHECK_LAUNCH();
    if ((rc = exclusive_scan_u32(cnt.p, out_off.p, n_reads, st, false))) return rc;
    hipLaunchKernelGGL(k_rescue_fill, per_read, dim3(kHitBlock), 0, st, B, (uint64_t)n_reads, d_hit_offsets, n_rec, jobs.p, place.p, out_off.p, d_hits_out, d_offsets_out,
                       d_mism_out);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&total, out_off.p + n_reads, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    *n_out = total;
    stats->reads_eligible = h_ctr[kRsEligible]; stats->records_orphan = h_ctr[kRsOrphan];
    stats->jobs_with_candidates = h_ctr[kRsWithCand]; stats->candidates = h_ctr[kRsCandidates];
    stats->reads_rescued = h_ctr[kRsReadsRescued]; stats->records_rescued = h_ctr[kRsRecRescued];
    stats->records_dropped = h_ctr[kRsDropped]; stats->sum_mism = h_ctr[kRsSumMism];
    return SFGPU_OK;
}
