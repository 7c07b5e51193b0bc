// verify.hip -- sfgpu_hits_verify: the mapper's hit records against the transcripts' bases.  WHAT a record's score is and
// which records survive is csrc/verifyfmt.h, stated once and run here unchanged; this file is only the way the work is laid out.
//
// count -> scan -> fill, as the mapper does:
//   k_verify_score  a group of kVfLanes = 16 lanes per READ (four reads a wavefront) walks the read's records; for each job every lane
//                   takes 16 oriented bases of the mate and the 16 transcript bases under them per step (vf_job_lane: one unaligned
//                   16-byte load from each text, pulled inside the text at its ends; the reverse strand reads the mate downwards
//                   from its end), classifies them in registers, and the group adds its counts up with shuffles: a mate of up to
//                   256 bases is one step.  Lane 0 decides (vf_record), keeps the score, the keep flag and the read's survivor count
//                   in scratch; the counters go through LDS, one global atomic per counter and block.  The read's records are
//                   together in one group, so keep_best needs no further pass.
//   scan            survivors per read -> output offsets
//   k_verify_fill   a lane per read copies its surviving records and scores to their places
// A record with tid >= M (or one that names mate 2 of a single-end batch) is found by the scoring pass, which writes scratch only:
// the call fails before anything is emitted.
#include "common.h"
#include "mapidx.h"
#include "primitives.h"
#include "verifyfmt.h"

namespace sfgpu {

constexpr int kVfBlock = 256;
constexpr uint32_t kVfLanes = 16;                                    // lanes per read
constexpr uint32_t kVfReadsPerBlock = kVfBlock / kVfLanes;
enum { kVfBadTid = 0, kVfBadMate, kVfFailed, kVfNotBest, kVfSumMism, kVfReadsIn, kVfReadsOut, kVfCounters };

__device__ __forceinline__ uint64_t group_sum(uint64_t v) {
#pragma unroll
    for (int o = kVfLanes / 2; o > 0; o >>= 1) v += __shfl_xor((unsigned long long)v, o, kVfLanes);
    return v;
}

__global__ void __launch_bounds__(kVfBlock)
k_verify_score(const char* __restrict__ tseq, const uint64_t* __restrict__ tseq_off, const uint32_t* __restrict__ tlen, uint64_t M,
               const char* __restrict__ seq1, const uint64_t* __restrict__ off1, const char* __restrict__ seq2, const uint64_t* __restrict__ off2,
               uint64_t n_reads, const sfgpu_hit* __restrict__ hits, const uint32_t* __restrict__ hit_off, uint64_t n_rec, uint32_t permille, int keep_best,
               uint64_t* __restrict__ cost /* [n_rec]: cost | pass << 63 */, uint64_t* __restrict__ mism /* unsaturated */, sfgpu_hit_score* __restrict__ score, uint8_t* __restrict__ keep,
               uint32_t* __restrict__ cnt /* [n_reads + 1] */, unsigned long long* ctr /* [kVfCounters] */) {
    __shared__ unsigned long long s_ctr[kVfCounters];
    if (threadIdx.x < kVfCounters) s_ctr[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * kVfReadsPerBlock + threadIdx.x / kVfLanes;
    const uint32_t lane = threadIdx.x % kVfLanes;
    if (r == n_reads && lane == 0) cnt[r] = 0;
    if (r < n_reads) {
        uint64_t e = hit_off[r + 1], b = hit_off[r];
        e = e < n_rec ? e : n_rec; b = b < e ? b : e;
        constexpr uint64_t kPass = 1ull << 63;
        uint64_t best = ~0ull, failed = 0, sum_mism = 0;
        uint32_t kept = 0;
        for (uint64_t i = b; i < e; ++i) {
            const sfgpu_hit h = hits[i];
            if (h.tid >= M) { if (lane == 0) { atomicMin(&ctr[kVfBadTid], (unsigned long long)i); cost[i] = 0; keep[i] = 0; } continue; }
            const uint32_t nj = vf_n_jobs(h);
            if ((h.mate_status == 2 || nj > 1) && !seq2) { if (lane == 0) { atomicMin(&ctr[kVfBadMate], (unsigned long long)i); cost[i] = 0; keep[i] = 0; } continue; }
            const char* t = tseq + tseq_off[h.tid];
            const uint64_t tl = tlen[h.tid];
            VfCount job[2] = {{0, 0}, {0, 0}}; uint64_t len[2] = {0, 0};
#pragma unroll
            for (uint32_t j = 0; j < 2u; ++j) {                      // (unrolled: job[] and len[] stay in registers)
                if (j >= nj) break;
                const VfJob jb = vf_job(h, j);
                const uint64_t* off = jb.mate ? off2 : off1;
                const uint64_t mb = off[r];
                len[j] = off[r + 1] - mb;
                const VfCount c = vf_job_lane((jb.mate ? seq2 : seq1) + mb, len[j], jb.fwd, t, tl, (int64_t)jb.pos, lane, kVfLanes);
                job[j].mism = group_sum(c.mism); job[j].over = group_sum(c.over);
            }
            if (lane == 0) {
                const VfRecord v = vf_record(h, job, len, permille);
                cost[i] = v.cost | (v.pass ? kPass : 0ull);
                mism[i] = v.mism;
                score[i] = v.score;
                if (v.pass && v.cost < best) best = v.cost;
                failed += !v.pass;
                if (!keep_best) { keep[i] = v.pass; kept += v.pass; if (v.pass) sum_mism += v.mism; }
            }
        }
        if (lane == 0) {
            uint64_t not_best = 0;
            if (keep_best) {                                         // (lane 0 reads back what it wrote itself)
                for (uint64_t i = b; i < e; ++i) {
                    const uint64_t c = cost[i];
                    const bool pass = (c & kPass) != 0, k = pass && (c & ~kPass) == best;
                    keep[i] = k; kept += k; not_best += pass && !k;
                    if (k) sum_mism += mism[i];
                }
            }
            cnt[r] = kept;
            if (failed) atomicAdd(&s_ctr[kVfFailed], (unsigned long long)failed);
            if (not_best) atomicAdd(&s_ctr[kVfNotBest], (unsigned long long)not_best);
            if (sum_mism) atomicAdd(&s_ctr[kVfSumMism], (unsigned long long)sum_mism);
            if (e > b) atomicAdd(&s_ctr[kVfReadsIn], 1ull);
            if (kept) atomicAdd(&s_ctr[kVfReadsOut], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x >= kVfFailed && threadIdx.x < kVfCounters && s_ctr[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], s_ctr[threadIdx.x]);
}

__global__ void __launch_bounds__(kVfBlock)
k_verify_fill(uint64_t n_reads, const sfgpu_hit* __restrict__ hits, const uint32_t* __restrict__ hit_off, uint64_t n_rec, const uint8_t* __restrict__ keep,
              const sfgpu_hit_score* __restrict__ score, const uint64_t* __restrict__ out_off, sfgpu_hit* __restrict__ hits_out,
              uint32_t* __restrict__ offsets_out, sfgpu_hit_score* __restrict__ scores_out) {
    const uint64_t r = (uint64_t)blockIdx.x * kVfBlock + threadIdx.x;
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

struct VerifySyncOnExit { hipStream_t s; ~VerifySyncOnExit() { (void)hipStreamSynchronize(s); } };

extern "C" int sfgpu_hits_verify(const sfgpu_index* x, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                 uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_verify_opts* opts,
                                 sfgpu_hit* d_hits_out, uint32_t* d_offsets_out, sfgpu_hit_score* d_scores_out, uint64_t* n_out,
                                 sfgpu_verify_stats* stats, sfgpu_stream stream) {
    SF_REQUIRE(x && opts && n_out && stats && d_offsets_out, SFGPU_ERR_INVALID, "sfgpu_hits_verify: null pointer");
    SF_REQUIRE(opts->min_identity_permille <= 1000u, SFGPU_ERR_INVALID, "sfgpu_hits_verify: min_identity_permille is 0 .. 1000");
    SF_REQUIRE(n_reads == 0 || (d_seq1 && d_off1 && d_hit_offsets && (!d_seq2 || d_off2)), SFGPU_ERR_INVALID, "sfgpu_hits_verify: null reads");
    hipStream_t st = as_stream(stream);
    if (n_reads == 0) {
        SF_HIP(hipMemsetAsync(d_offsets_out, 0, 4, st)); SF_HIP(hipStreamSynchronize(st));
        *n_out = 0; *stats = sfgpu_verify_stats{};
        return SFGPU_OK;
    }
    uint32_t n_rec32 = 0;
    SF_HIP(hipMemcpyAsync(&n_rec32, d_hit_offsets + n_reads, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint64_t n_rec = n_rec32;
    SF_REQUIRE(n_rec == 0 || (d_hits && d_hits_out), SFGPU_ERR_INVALID, "sfgpu_hits_verify: null records");
    int rc;
    DevBuf<uint64_t> cost, mism, out_off; DevBuf<sfgpu_hit_score> score; DevBuf<uint8_t> keep; DevBuf<uint32_t> cnt; DevBuf<unsigned long long> ctr;
    VerifySyncOnExit sync_first{st};         // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    if ((rc = cost.reserve(n_rec + 1, st, false)) || (rc = mism.reserve(n_rec + 1, st, false)) || (rc = score.reserve(n_rec + 1, st, false)) || (rc = keep.reserve(n_rec + 1, st, false)) ||
        (rc = cnt.reserve((uint64_t)n_reads + 1, st, false)) || (rc = out_off.reserve((uint64_t)n_reads + 2, st, false)) || (rc = ctr.reserve(kVfCounters, st, false))) return rc;
    unsigned long long h_ctr[kVfCounters] = {~0ull, ~0ull, 0, 0, 0, 0, 0};
    SF_HIP(hipMemcpyAsync(ctr.p, h_ctr, sizeof h_ctr, hipMemcpyHostToDevice, st));
    const unsigned grid = (unsigned)(((uint64_t)n_reads + 1 + kVfReadsPerBlock - 1) / kVfReadsPerBlock);
    hipLaunchKernelGGL(k_verify_score, dim3(grid), dim3(kVfBlock), 0, st, x->tseq.p, x->tseq_off.p, x->tlen.p, x->M, d_seq1, d_off1, d_seq2, d_off2,
                       (uint64_t)n_reads, d_hits, d_hit_offsets, n_rec, opts->min_identity_permille, (int)(opts->keep_best != 0), cost.p, mism.p, score.p, keep.p, cnt.p, ctr.p);
    SF_CHECK_LAUNCH();
    if ((rc = exclusive_scan_u32(cnt.p, out_off.p, n_reads, st, false))) return rc;
    uint64_t total = 0;
    SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&total, out_off.p + n_reads, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h_ctr[kVfBadTid] != ~0ull) {
        set_error("sfgpu_hits_verify: record %llu names transcript >= %llu", h_ctr[kVfBadTid], (unsigned long long)x->M);
        return SFGPU_ERR_RANGE;
    }
    if (h_ctr[kVfBadMate] != ~0ull) {
        set_error("sfgpu_hits_verify: record %llu names mate 2 of a single-end batch", h_ctr[kVfBadMate]);
        return SFGPU_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_verify_fill, dim3((unsigned)(((uint64_t)n_reads + 1 + kVfBlock - 1) / kVfBlock)), dim3(kVfBlock), 0, st, (uint64_t)n_reads, d_hits, d_hit_offsets,
                       n_rec, keep.p, score.p, out_off.p, d_hits_out, d_offsets_out, d_scores_out);
    SF_CHECK_LAUNCH();
    SF_HIP(hipStreamSynchronize(st));
    *n_out = total;
    stats->records_in = n_rec; stats->records_out = total;
    stats->reads_in = h_ctr[kVfReadsIn]; stats->reads_out = h_ctr[kVfReadsOut];
    stats->failed_identity = h_ctr[kVfFailed]; stats->dropped_not_best = h_ctr[kVfNotBest]; stats->sum_mism = h_ctr[kVfSumMism];
    return SFGPU_OK;
}
