// verify.hip -- sfgpu_hits_verify and sfgpu_hits_verify_gapped: the mapper's hit records against the transcripts' bases, on the
// recorded diagonal or scored with gaps (4.28).  WHAT a record's score is and which records survive is
// csrc/verifyfmt.h and csrc/verifygfmt.h, stated once and run here unchanged; this file is only the way the work is laid out, and
// what the hit passes share of that is csrc/hitgroup.h.
//
// count -> scan -> fill, as the mapper does:
//   k_verify_score<GAPPED, W>  a group of W lanes per READ walks the read's records (ungapped: W = 16, four reads a wavefront;
//                   gapped: 16 for max_indel <= 7, 32 up to 15).  For each job every lane takes 16 oriented bases of the mate and
//                   the 16 transcript bases under them per step (vf_job_lane: one unaligned 16-byte load from each text, pulled
//                   inside the text at its ends; the reverse strand reads the mate downwards from its end), classifies them in
//                   registers, and the group adds its counts up with shuffles: a mate of up to 16 W bases is one step.  Ungapped,
//                   that is the job.  Gapped, it is the score's `ungapped` and what `rescued` is decided by; a count of 0 means 0
//                   edits, otherwise the band runs (hit_band_dev<W, false>: lanes are DIAGONALS; above vg_max_edits the job, and
//                   with it the record, has failed and stops).  Lane 0 decides (vf_record / vg_record), keeps the score, the keep
//                   flag and the read's survivor count in scratch; the counters go through LDS, one global atomic per counter and
//                   block.  The read's records are together in one group, so keep_best needs no further pass.
//   scan            survivors per read -> output offsets
//   k_hits_fill     a lane per read copies its surviving records and scores to their places
// A record with tid >= M (or one that names mate 2 of a single-end batch) is found by the scoring pass, which writes scratch only:
// the call fails before anything is emitted.
#include "common.h"
#include "mapidx.h"
#include "primitives.h"
#include "hitgroup.h"

namespace sfgpu {

enum { kVfFailed = kHitFirstCounter, kVfNotBest, kVfSum /* mism, or edits */, kVfReadsIn, kVfReadsOut, kVfRescued /* gapped only */, kVfCounters };
constexpr uint64_t kVfPassBit = 1ull << 63, kVfRescuedBit = 1ull << 62;    // of a cost word; the second is the gapped pass's

// what the two passes do not share: their types, their name, and the counters they have (the rest is `if constexpr (GAPPED)` below)
template <bool GAPPED> struct VerifyKind;
template <> struct VerifyKind<false> {
    using Job = VfCount; using Score = sfgpu_hit_score; using Opts = sfgpu_verify_opts; using Stats = sfgpu_verify_stats;
    static constexpr int kCounters = kVfRescued;
    static constexpr const char* kEntry = "sfgpu_hits_verify";
};
template <> struct VerifyKind<true> {
    using Job = VgJob; using Score = sfgpu_hit_gscore; using Opts = sfgpu_verify_gopts; using Stats = sfgpu_verify_gstats;
    static constexpr int kCounters = kVfCounters;
    static constexpr const char* kEntry = "sfgpu_hits_verify_gapped";
};

__device__ __forceinline__ VfRecord verify_record(const sfgpu_hit& h, const VfCount* job, const uint64_t* len, uint32_t permille) { return vf_record(h, job, len, permille); }
__device__ __forceinline__ VgRecord verify_record(const sfgpu_hit& h, const VgJob* job, const uint64_t* len, uint32_t permille) { return vg_record(h, job, len, permille); }

template <bool GAPPED, int W> __global__ void __launch_bounds__(kHitBlock)
k_verify_score(const HitBatchDev B, uint64_t n_reads, const uint32_t* __restrict__ hit_off, uint64_t n_rec, uint32_t permille, int keep_best,
               [[maybe_unused]] uint32_t k /* GAPPED */, uint64_t* __restrict__ cost /* [n_rec]: cost | rescued << 62 | pass << 63 */,
               [[maybe_unused]] uint64_t* __restrict__ mism /* !GAPPED: unsaturated */, typename VerifyKind<GAPPED>::Score* __restrict__ score,
               uint8_t* __restrict__ keep, uint32_t* __restrict__ cnt /* [n_reads + 1] */, unsigned long long* ctr /* [kCounters] */) {
    using Kind = VerifyKind<GAPPED>;
    constexpr uint32_t kReadsPerBlock = kHitBlock / W;
    __shared__ unsigned long long s_ctr[Kind::kCounters];
    hit_ctr_zero(s_ctr);
    const uint64_t r = (uint64_t)blockIdx.x * kReadsPerBlock + threadIdx.x / W;
    const uint32_t lane = threadIdx.x % W;
    if (r == n_reads && lane == 0) cnt[r] = 0;
    if (r < n_reads) {
        uint64_t b, e;
        hit_range(hit_off, r, n_rec, &b, &e);
        uint64_t best = ~0ull, failed = 0, sum = 0;
        [[maybe_unused]] uint64_t rescued = 0;
        uint32_t kept = 0;
        for (uint64_t i = b; i < e; ++i) {
            const sfgpu_hit h = B.hits[i];
            const int bad = hit_bad_record(h, B.M, B.seq2);
            if (bad >= 0) { if (lane == 0) { atomicMin(&ctr[bad], (unsigned long long)i); cost[i] = 0; keep[i] = 0; } continue; }
            const uint32_t nj = vf_n_jobs(h);
            typename Kind::Job job[2] = {}; uint64_t len[2] = {0, 0};
            if constexpr (GAPPED) job[0].ungapped_pass = job[1].ungapped_pass = true;
            bool alive = true;                                       // (the same in every lane of the group; ungapped: both jobs are counted)
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j) {                      // (unrolled: job[] and len[] stay in registers)
                if (j >= nj || !alive) break;
                const HitJobDev jb = hit_job_dev(B, h, j, r);
                len[j] = jb.len;
                const VfCount c = vf_job_lane(jb.m, jb.len, jb.fwd, jb.t, jb.tl, jb.pos, lane, W);
                const uint64_t mm = group_sum<W>(c.mism), over = group_sum<W>(c.over);
                if constexpr (!GAPPED) job[j] = VfCount{mm, over};
                else {
                    job[j].ungapped = mm + over;
                    job[j].ungapped_pass = vf_passes(jb.len, mm, over, permille);
                    const uint64_t max_edits = vg_max_edits(jb.len, permille);
                    job[j].edits = job[j].ungapped == 0 ? 0ull : hit_band_dev<W, false>(jb, k, lane, max_edits, nullptr);
                    alive = job[j].edits != kVgFail && job[j].edits <= max_edits;
                    if (!alive) job[j].edits = kVgFail;
                }
            }
            if (lane == 0) {
                const auto v = verify_record(h, job, len, permille);
                uint64_t word = v.cost | (v.pass ? kVfPassBit : 0ull), add;
                if constexpr (GAPPED) { word |= v.rescued ? kVfRescuedBit : 0ull; add = v.cost; }
                else { mism[i] = v.mism; add = v.mism; }
                cost[i] = word;
                score[i] = v.score;
                if (v.pass && v.cost < best) best = v.cost;
                failed += !v.pass;
                if (!keep_best) {
                    keep[i] = v.pass; kept += v.pass;
                    if (v.pass) { sum += add; if constexpr (GAPPED) rescued += v.rescued; }
                }
            }
        }
        if (lane == 0) {
            uint64_t not_best = 0;
            if (keep_best) {                                         // (lane 0 reads back what it wrote itself)
                for (uint64_t i = b; i < e; ++i) {
                    const uint64_t c = cost[i], cv = c & ~(kVfPassBit | kVfRescuedBit);
                    const bool pass = (c & kVfPassBit) != 0, kp = pass && cv == best;
                    keep[i] = kp; kept += kp; not_best += pass && !kp;
                    if constexpr (GAPPED) { if (kp) { sum += cv; rescued += (c & kVfRescuedBit) != 0; } }
                    else if (kp) sum += mism[i];
                }
            }
            cnt[r] = kept;
            if (failed) atomicAdd(&s_ctr[kVfFailed], (unsigned long long)failed);
            if (not_best) atomicAdd(&s_ctr[kVfNotBest], (unsigned long long)not_best);
            if (sum) atomicAdd(&s_ctr[kVfSum], (unsigned long long)sum);
            if constexpr (GAPPED) if (rescued) atomicAdd(&s_ctr[kVfRescued], (unsigned long long)rescued);
            if (e > b) atomicAdd(&s_ctr[kVfReadsIn], 1ull);
            if (kept) atomicAdd(&s_ctr[kVfReadsOut], 1ull);
        }
    }
    hit_ctr_flush(s_ctr, ctr);
}

// both entries: `opts` is the entry's own struct, max_indel read from it where it has one
template <bool GAPPED>
static int hits_verify(const sfgpu_index* x, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2, uint32_t n_reads,
                       const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const typename VerifyKind<GAPPED>::Opts* opts, sfgpu_hit* d_hits_out,
                       uint32_t* d_offsets_out, typename VerifyKind<GAPPED>::Score* d_scores_out, uint64_t* n_out, typename VerifyKind<GAPPED>::Stats* stats,
                       sfgpu_stream stream) {
    using Kind = VerifyKind<GAPPED>;
#define VF_REQUIRE(cond, what) do { if (!(cond)) { set_error("%s: %s", Kind::kEntry, what); return SFGPU_ERR_INVALID; } } while (0)
    VF_REQUIRE(x && opts && n_out && stats && d_offsets_out, "null pointer");
    VF_REQUIRE(opts->min_identity_permille <= 1000u, "min_identity_permille is 0 .. 1000");
    uint32_t k = 0, W = 16;
    if constexpr (GAPPED) {
        k = opts->max_indel;
        VF_REQUIRE(k >= 1u && k <= kVgMaxIndel, "max_indel is 1 .. 15");
        W = vg_width(k);
    }
    VF_REQUIRE(n_reads == 0 || (d_seq1 && d_off1 && d_hit_offsets && (!d_seq2 || d_off2)), "null reads");
    hipStream_t st = as_stream(stream);
    if (n_reads == 0) {
        SF_HIP(hipMemsetAsync(d_offsets_out, 0, 4, st)); SF_HIP(hipStreamSynchronize(st));
        *n_out = 0; *stats = typename Kind::Stats{};
        return SFGPU_OK;
    }
    int rc;
    uint64_t n_rec = 0;
    if ((rc = hit_n_rec(d_hit_offsets, n_reads, st, &n_rec))) return rc;
    VF_REQUIRE(n_rec == 0 || (d_hits && d_hits_out), "null records");
#undef VF_REQUIRE
    DevBuf<uint64_t> cost, mism, out_off; DevBuf<typename Kind::Score> score; DevBuf<uint8_t> keep; DevBuf<uint32_t> cnt; DevBuf<unsigned long long> ctr;
    StreamSyncOnExit sync_first{st};         // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    if ((rc = cost.reserve(n_rec + 1, st, false)) || (!GAPPED && (rc = mism.reserve(n_rec + 1, st, false))) || (rc = score.reserve(n_rec + 1, st, false)) ||
        (rc = keep.reserve(n_rec + 1, st, false)) || (rc = cnt.reserve((uint64_t)n_reads + 1, st, false)) || (rc = out_off.reserve((uint64_t)n_reads + 2, st, false)) ||
        (rc = ctr.reserve(Kind::kCounters, st, false))) return rc;
    unsigned long long h_ctr[Kind::kCounters] = {~0ull, ~0ull};
    SF_HIP(hipMemcpyAsync(ctr.p, h_ctr, sizeof h_ctr, hipMemcpyHostToDevice, st));
    const uint32_t per_block = kHitBlock / W;
    const unsigned grid = (unsigned)(((uint64_t)n_reads + 1 + per_block - 1) / per_block);
    auto score_kernel = k_verify_score<GAPPED, 16>;
    if constexpr (GAPPED) if (W == 32u) score_kernel = k_verify_score<GAPPED, 32>;
    hipLaunchKernelGGL(score_kernel, dim3(grid), dim3(kHitBlock), 0, st, HitBatchDev(x, d_seq1, d_off1, d_seq2, d_off2, d_hits), (uint64_t)n_reads, d_hit_offsets, n_rec,
                       opts->min_identity_permille, (int)(opts->keep_best != 0), k, cost.p, mism.p, score.p, keep.p, cnt.p, ctr.p);
    SF_CHECK_LAUNCH();
    if ((rc = exclusive_scan_u32(cnt.p, out_off.p, n_reads, st, false))) return rc;
    uint64_t total = 0;
    SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&total, out_off.p + n_reads, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if ((rc = hit_report_bad(Kind::kEntry, h_ctr, x->M))) return rc;
    hipLaunchKernelGGL(k_hits_fill<typename Kind::Score>, dim3((unsigned)(((uint64_t)n_reads + 1 + kHitBlock - 1) / kHitBlock)), dim3(kHitBlock), 0, st, (uint64_t)n_reads,
                       d_hits, d_hit_offsets, n_rec, keep.p, score.p, out_off.p, d_hits_out, d_offsets_out, d_scores_out);
    SF_CHECK_LAUNCH();
    SF_HIP(hipStreamSynchronize(st));
    *n_out = total;
    stats->records_in = n_rec; stats->records_out = total;
    stats->reads_in = h_ctr[kVfReadsIn]; stats->reads_out = h_ctr[kVfReadsOut];
    stats->failed_identity = h_ctr[kVfFailed]; stats->dropped_not_best = h_ctr[kVfNotBest];
    if constexpr (GAPPED) { stats->sum_edits = h_ctr[kVfSum]; stats->rescued = h_ctr[kVfRescued]; }
    else stats->sum_mism = h_ctr[kVfSum];
    return SFGPU_OK;
}

}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_hits_verify(const sfgpu_index* x, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                 uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_verify_opts* opts,
                                 sfgpu_hit* d_hits_out, uint32_t* d_offsets_out, sfgpu_hit_score* d_scores_out, uint64_t* n_out,
                                 sfgpu_verify_stats* stats, sfgpu_stream stream) {
    return hits_verify<false>(x, d_seq1, d_off1, d_seq2, d_off2, n_reads, d_hits, d_hit_offsets, opts, d_hits_out, d_offsets_out, d_scores_out, n_out, stats, stream);
}

extern "C" int sfgpu_hits_verify_gapped(const sfgpu_index* x, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                        uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_verify_gopts* opts,
                                        sfgpu_hit* d_hits_out, uint32_t* d_offsets_out, sfgpu_hit_gscore* d_scores_out, uint64_t* n_out,
                                        sfgpu_verify_gstats* stats, sfgpu_stream stream) {
    return hits_verify<true>(x, d_seq1, d_off1, d_seq2, d_off2, n_reads, d_hits, d_hit_offsets, opts, d_hits_out, d_offsets_out, d_scores_out, n_out, stats, stream);
}
