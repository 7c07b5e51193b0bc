// verify_gapped.hip -- sfgpu_hits_verify_gapped: the mapper's hit records against the transcripts' bases, scored with gaps (DESIGN
// 4.28).  WHAT a job's edits are and which records survive is csrc/verifygfmt.h, stated once and run here unchanged; this file is only
// the way the work is laid out.
//
// count -> scan -> fill, as verify.hip:
//   k_verifyg_score<W>  a group of W lanes per READ walks the read's records (W = 16 for max_indel <= 7, four reads a wavefront; 32 up
//                       to 15).  Per job the group first counts ungapped (vf_job_lane + a group sum: the score's `ungapped`, and what
//                       `rescued` is decided by); a count of 0 means 0 edits and the job is done.  Otherwise lanes are DIAGONALS: lane
//                       l holds D[.][l - k].  A row is one shuffle for the upper neighbour's cell, vg_lane_v, and an inclusive prefix
//                       minimum in log2 W shuffle steps.  Every 16 rows each lane refills its transcript window on its own diagonal
//                       and the mate's window (clipped 16-byte loads, the reverse strand read downwards), classifies the 16 pairs
//                       into a bit mask, and the group takes the band's minimum: above vg_max_edits the job, and with it the record,
//                       has failed and stops.  Lane 0 decides (vg_record) and keeps score, flags and the read's survivor count in
//                       scratch; counters go through LDS.  A read's records are together in one group: keep_best needs no further pass.
//   scan                survivors per read -> output offsets
//   k_verifyg_fill      a lane per read copies its surviving records and scores to their places
// Errors are found by the scoring pass, which writes scratch only: the call fails before anything is emitted.
#include "common.h"
#include "mapidx.h"
#include "primitives.h"
#include "verifygfmt.h"

namespace sfgpu {

constexpr int kVgBlock = 256;
enum { kVgBadTid = 0, kVgBadMate, kVgFailed, kVgNotBest, kVgSumEdits, kVgRescued, kVgReadsIn, kVgReadsOut, kVgCounters };
constexpr uint64_t kVgPassBit = 1ull << 63, kVgRescuedBit = 1ull << 62;

template <int W> __device__ __forceinline__ uint64_t vg_group_sum(uint64_t v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor((unsigned long long)v, o, W);
    return v;
}
template <int W> __device__ __forceinline__ uint32_t vg_group_min(uint32_t v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(v, o, W); v = u < v ? u : v; }
    return v;
}

// the banded recurrence of one job over the group's lanes -> edits, or kVgFail (the same in every lane of the group)
template <int W> __device__ __forceinline__ uint64_t vg_job_dev(const char* r, uint64_t len, bool fwd, const char* t, uint64_t tl, int64_t pos, uint32_t k,
                                                                uint32_t lane, uint64_t max_edits) {
    uint32_t D = vg_lane_start(lane, k), m = 0;
    for (uint64_t i0 = 0; i0 < len; i0 += kVfStep) {
        const uint32_t mask = vg_lane_submask(vf_mate_window(r, (int64_t)len, fwd, (int64_t)i0), t, tl, pos, i0, lane, k, fwd);
        const uint32_t n = len - i0 < kVfStep ? (uint32_t)(len - i0) : kVfStep;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t up = __shfl_down(D, 1, W);                // (lane W - 1 gets its own: it is never in the band)
            uint32_t key = vg_key(vg_lane_v(D, up, (mask >> j) & 1u), lane, W);
#pragma unroll
            for (int o = 1; o < W; o <<= 1) key = vg_scan_step(key, __shfl_up(key, o, W), lane, (uint32_t)o);
            D = vg_lane_d(key, lane, W, k);
        }
        m = vg_group_min<W>(D);
        if (m > max_edits) return kVgFail;
    }
    return m;
}

template <int W> __global__ void __launch_bounds__(kVgBlock)
k_verifyg_score(const char* __restrict__ tseq, const uint64_t* __restrict__ tseq_off, const uint32_t* __restrict__ tlen, uint64_t M,
                const char* __restrict__ seq1, const uint64_t* __restrict__ off1, const char* __restrict__ seq2, const uint64_t* __restrict__ off2,
                uint64_t n_reads, const sfgpu_hit* __restrict__ hits, const uint32_t* __restrict__ hit_off, uint64_t n_rec, uint32_t permille, int keep_best, uint32_t k,
                uint64_t* __restrict__ cost /* [n_rec]: cost | rescued << 62 | pass << 63 */, sfgpu_hit_gscore* __restrict__ score, uint8_t* __restrict__ keep,
                uint32_t* __restrict__ cnt /* [n_reads + 1] */, unsigned long long* ctr /* [kVgCounters] */) {
    constexpr uint32_t kReadsPerBlock = kVgBlock / W;
    __shared__ unsigned long long s_ctr[kVgCounters];
    if (threadIdx.x < kVgCounters) s_ctr[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * kReadsPerBlock + threadIdx.x / W;
    const uint32_t lane = threadIdx.x % W;
    if (r == n_reads && lane == 0) cnt[r] = 0;
    if (r < n_reads) {
        uint64_t e = hit_off[r + 1], b = hit_off[r];
        e = e < n_rec ? e : n_rec; b = b < e ? b : e;
        uint64_t best = ~0ull, failed = 0, sum_edits = 0, rescued = 0;
        uint32_t kept = 0;
        for (uint64_t i = b; i < e; ++i) {
            const sfgpu_hit h = hits[i];
            if (h.tid >= M) { if (lane == 0) { atomicMin(&ctr[kVgBadTid], (unsigned long long)i); cost[i] = 0; keep[i] = 0; } continue; }
            const uint32_t nj = vf_n_jobs(h);
            if ((h.mate_status == 2 || nj > 1) && !seq2) { if (lane == 0) { atomicMin(&ctr[kVgBadMate], (unsigned long long)i); cost[i] = 0; keep[i] = 0; } continue; }
            const char* t = tseq + tseq_off[h.tid];
            const uint64_t tl = tlen[h.tid];
            VgJob job[2] = {{0, 0, true}, {0, 0, true}}; uint64_t len[2] = {0, 0};
            bool alive = true;                                       // (the same in every lane of the group)
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j) {                      // (unrolled: job[] and len[] stay in registers)
                if (j >= nj || !alive) break;
                const VfJob jb = vf_job(h, j);
                const uint64_t* off = jb.mate ? off2 : off1;
                const uint64_t mb = off[r];
                len[j] = off[r + 1] - mb;
                const char* m = (jb.mate ? seq2 : seq1) + mb;
                const VfCount c = vf_job_lane(m, len[j], jb.fwd, t, tl, (int64_t)jb.pos, lane, W);
                const uint64_t mism = vg_group_sum<W>(c.mism), over = vg_group_sum<W>(c.over);
                job[j].ungapped = mism + over;
                job[j].ungapped_pass = vf_passes(len[j], mism, over, permille);
                const uint64_t max_edits = vg_max_edits(len[j], permille);
                job[j].edits = job[j].ungapped == 0 ? 0ull : vg_job_dev<W>(m, len[j], jb.fwd, t, tl, (int64_t)jb.pos, k, lane, max_edits);
                alive = job[j].edits != kVgFail && job[j].edits <= max_edits;
                if (!alive) job[j].edits = kVgFail;
            }
            if (lane == 0) {
                const VgRecord v = vg_record(h, job, len, permille);
                cost[i] = v.cost | (v.pass ? kVgPassBit : 0ull) | (v.rescued ? kVgRescuedBit : 0ull);
                score[i] = v.score;
                if (v.pass && v.cost < best) best = v.cost;
                failed += !v.pass;
                if (!keep_best) { keep[i] = v.pass; kept += v.pass; if (v.pass) { sum_edits += v.cost; rescued += v.rescued; } }
            }
        }
        if (lane == 0) {
            uint64_t not_best = 0;
            if (keep_best) {                                         // (lane 0 reads back what it wrote itself)
                for (uint64_t i = b; i < e; ++i) {
                    const uint64_t c = cost[i], cv = c & ~(kVgPassBit | kVgRescuedBit);
                    const bool pass = (c & kVgPassBit) != 0, kp = pass && cv == best;
                    keep[i] = kp; kept += kp; not_best += pass && !kp;
                    if (kp) { sum_edits += cv; rescued += (c & kVgRescuedBit) != 0; }
                }
            }
            cnt[r] = kept;
            if (failed) atomicAdd(&s_ctr[kVgFailed], (unsigned long long)failed);
            if (not_best) atomicAdd(&s_ctr[kVgNotBest], (unsigned long long)not_best);
            if (sum_edits) atomicAdd(&s_ctr[kVgSumEdits], (unsigned long long)sum_edits);
            if (rescued) atomicAdd(&s_ctr[kVgRescued], (unsigned long long)rescued);
            if (e > b) atomicAdd(&s_ctr[kVgReadsIn], 1ull);
            if (kept) atomicAdd(&s_ctr[kVgReadsOut], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x >= kVgFailed && threadIdx.x < kVgCounters && s_ctr[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], s_ctr[threadIdx.x]);
}

__global__ void __launch_bounds__(kVgBlock)
k_verifyg_fill(uint64_t n_reads, const sfgpu_hit* __restrict__ hits, const uint32_t* __restrict__ hit_off, uint64_t n_rec, const uint8_t* __restrict__ keep,
               const sfgpu_hit_gscore* __restrict__ score, const uint64_t* __restrict__ out_off, sfgpu_hit* __restrict__ hits_out,
               uint32_t* __restrict__ offsets_out, sfgpu_hit_gscore* __restrict__ scores_out) {
    const uint64_t r = (uint64_t)blockIdx.x * kVgBlock + threadIdx.x;
    if (r > n_reads) return;
    uint64_t o = out_off[r];
    offsets_out[r] = (uint32_t)o;
    if (r == n_reads) return;
    uint64_t e = hit_off[r + 1], b = hit_off[r];
    e = e < n_rec ? e : n_rec; b = b < e ? b : e;
    for (uint64_t i = b; i < e; ++i) {
        if (!keep[i]) continue;
        hits_out[o] = hits[i];
        if (scores_out) scores_out[o] = score[i];
        ++o;
    }
}

}  // namespace sfgpu

using namespace sfgpu;

struct VerifyGSyncOnExit { hipStream_t s; ~VerifyGSyncOnExit() { (void)hipStreamSynchronize(s); } };

extern "C" int sfgpu_hits_verify_gapped(const sfgpu_index* x, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                        uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_verify_gopts* opts,
                                        sfgpu_hit* d_hits_out, uint32_t* d_offsets_out, sfgpu_hit_gscore* d_scores_out, uint64_t* n_out,
                                        sfgpu_verify_gstats* stats, sfgpu_stream stream) {
    SF_REQUIRE(x && opts && n_out && stats && d_offsets_out, SFGPU_ERR_INVALID, "sfgpu_hits_verify_gapped: null pointer");
    SF_REQUIRE(opts->min_identity_permille <= 1000u, SFGPU_ERR_INVALID, "sfgpu_hits_verify_gapped: min_identity_permille is 0 .. 1000");
    SF_REQUIRE(opts->max_indel >= 1u && opts->max_indel <= kVgMaxIndel, SFGPU_ERR_INVALID, "sfgpu_hits_verify_gapped: max_indel is 1 .. 15");
    SF_REQUIRE(n_reads == 0 || (d_seq1 && d_off1 && d_hit_offsets && (!d_seq2 || d_off2)), SFGPU_ERR_INVALID, "sfgpu_hits_verify_gapped: null reads");
    hipStream_t st = as_stream(stream);
    if (n_reads == 0) {
        SF_HIP(hipMemsetAsync(d_offsets_out, 0, 4, st)); SF_HIP(hipStreamSynchronize(st));
        *n_out = 0; *stats = sfgpu_verify_gstats{};
        return SFGPU_OK;
    }
    uint32_t n_rec32 = 0;
    SF_HIP(hipMemcpyAsync(&n_rec32, d_hit_offsets + n_reads, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint64_t n_rec = n_rec32;
    SF_REQUIRE(n_rec == 0 || (d_hits && d_hits_out), SFGPU_ERR_INVALID, "sfgpu_hits_verify_gapped: null records");
    int rc;
    DevBuf<uint64_t> cost, out_off; DevBuf<sfgpu_hit_gscore> score; DevBuf<uint8_t> keep; DevBuf<uint32_t> cnt; DevBuf<unsigned long long> ctr;
    VerifyGSyncOnExit sync_first{st};        // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    if ((rc = cost.reserve(n_rec + 1, st, false)) || (rc = score.reserve(n_rec + 1, st, false)) || (rc = keep.reserve(n_rec + 1, st, false)) ||
        (rc = cnt.reserve((uint64_t)n_reads + 1, st, false)) || (rc = out_off.reserve((uint64_t)n_reads + 2, st, false)) || (rc = ctr.reserve(kVgCounters, st, false))) return rc;
    unsigned long long h_ctr[kVgCounters] = {~0ull, ~0ull, 0, 0, 0, 0, 0, 0};
    SF_HIP(hipMemcpyAsync(ctr.p, h_ctr, sizeof h_ctr, hipMemcpyHostToDevice, st));
    const uint32_t W = vg_width(opts->max_indel), per_block = kVgBlock / W;
    const unsigned grid = (unsigned)(((uint64_t)n_reads + 1 + per_block - 1) / per_block);
    auto score_kernel = W == 16u ? k_verifyg_score<16> : k_verifyg_score<32>;
    hipLaunchKernelGGL(score_kernel, dim3(grid), dim3(kVgBlock), 0, st, x->tseq.p, x->tseq_off.p, x->tlen.p, x->M, d_seq1, d_off1, d_seq2, d_off2,
                       (uint64_t)n_reads, d_hits, d_hit_offsets, n_rec, opts->min_identity_permille, (int)(opts->keep_best != 0), opts->max_indel, cost.p, score.p, keep.p,
                       cnt.p, ctr.p);
    SF_CHECK_LAUNCH();
    if ((rc = exclusive_scan_u32(cnt.p, out_off.p, n_reads, st, false))) return rc;
    uint64_t total = 0;
    SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&total, out_off.p + n_reads, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h_ctr[kVgBadTid] != ~0ull) {
        set_error("sfgpu_hits_verify_gapped: record %llu names transcript >= %llu", h_ctr[kVgBadTid], (unsigned long long)x->M);
        return SFGPU_ERR_RANGE;
    }
    if (h_ctr[kVgBadMate] != ~0ull) {
        set_error("sfgpu_hits_verify_gapped: record %llu names mate 2 of a single-end batch", h_ctr[kVgBadMate]);
        return SFGPU_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_verifyg_fill, dim3((unsigned)(((uint64_t)n_reads + 1 + kVgBlock - 1) / kVgBlock)), dim3(kVgBlock), 0, st, (uint64_t)n_reads, d_hits, d_hit_offsets,
                       n_rec, keep.p, score.p, out_off.p, d_hits_out, d_offsets_out, d_scores_out);
    SF_CHECK_LAUNCH();
    SF_HIP(hipStreamSynchronize(st));
    *n_out = total;
    stats->records_in = n_rec; stats->records_out = total;
    stats->reads_in = h_ctr[kVgReadsIn]; stats->reads_out = h_ctr[kVgReadsOut];
    stats->failed_identity = h_ctr[kVgFailed]; stats->dropped_not_best = h_ctr[kVgNotBest]; stats->sum_edits = h_ctr[kVgSumEdits]; stats->rescued = h_ctr[kVgRescued];
    return SFGPU_OK;
}
