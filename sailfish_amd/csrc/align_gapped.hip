// align_gapped.hip -- sfgpu_hits_align_gapped: the gapped alignment of the records that survive sfgpu_hits_verify_gapped, as a
// position and BAM CIGAR words per job.  WHAT the alignment of a job is -- candidates, end cell, walk, trim -- is
// csrc/aligngfmt.h, stated once and run here unchanged; this file is only the way the work is laid out, and what the hit passes
// share of that -- the batch, the job decode, the group tools, the band, the slot pass's host side (HitSlotPass) -- is csrc/hitgroup.h.
//
// Two slots per record (slot 2 h + j is job j of record h); count -> scan -> fill, twice:
//   k_hits_rec_read     (hitgroup.h) a lane per read names the read of each of its records
//   k_aligng_size<W>    a group of W lanes per slot (W = 16 for max_indel <= 7, 32 up to 15) counts the job's ungapped mismatches
//                       (vf_job_lane + a group sum) and with them its kind -- no job, no bases, all bases match, traced -- and the
//                       steps of scratch it needs (ceil(len / 16) for a traced job, else none); errors are found here
//   scan                steps -> the scratch's CSR; the host cuts the slots into slices whose scratch fits the cap (k_aligng_cut)
//   k_aligng_trace<W, false>  per slice, a group per slot.  Forward (hit_band_dev<W, true>): lanes are DIAGONALS, the row is the
//                       scoring pass's plus one exchange for the lower neighbour's new cell; every 16 rows a lane stores the 4 bits of its 16 cells as one
//                       64-bit word, the group W consecutive words (128 or 256 bytes).  Backward: ag_walk over those words, a lane
//                       loading its own word of a step once and the group taking the current lane's by shuffle; this pass counts
//                       the operations only.
//   scan                operations -> the outputs' CSR; too many for the caller's room: SFGPU_ERR_RANGE, nothing written
//   k_aligng_trace<W, true>   the same walk again, writing each run where it belongs, and pos, nm, op_off and the counters.  With one
//                       slice the scratch still holds the cells and the forward pass is not repeated.
#include "common.h"
#include "mapidx.h"
#include "primitives.h"
#include "hitgroup.h"

#include <vector>

namespace sfgpu {

constexpr int kAgBlock = kHitBlock;
constexpr uint64_t kAgDefaultCap = 256ull << 20;
enum { kAgJobs = kHitFirstCounter, kAgTraced, kAgUnalignable, kAgSumNm, kAgCounters };
enum : uint8_t { kAgNoJob = 0, kAgNoBases, kAgAllMatch, kAgTracedJob };

template <int W> __global__ void __launch_bounds__(kAgBlock)
k_aligng_size(const HitBatchDev B, uint32_t* __restrict__ steps /* [n_slots] */, uint8_t* __restrict__ kind /* [n_slots] */, unsigned long long* ctr) {
    const uint64_t s = (uint64_t)blockIdx.x * (kAgBlock / W) + threadIdx.x / W;
    const uint32_t lane = threadIdx.x % W;
    if (s >= B.n_slots) return;                                      // (a whole group)
    const sfgpu_hit h = B.hits[s >> 1];
    const uint32_t j = (uint32_t)(s & 1u), r = B.rec_read[s >> 1];
    uint32_t need = 0; uint8_t kd = kAgNoJob;
    const int bad = hit_bad_record(h, B.M, B.seq2);
    if (bad >= 0) { if (lane == 0) atomicMin(&ctr[bad], (unsigned long long)(s >> 1)); }
    else if (j < vf_n_jobs(h) && r != ~0u) {
        const HitJobDev jb = hit_job_dev(B, h, j, r);
        const VfCount c = vf_job_lane(jb.m, jb.len, jb.fwd, jb.t, jb.tl, jb.pos, lane, W);
        const uint64_t ungapped = group_sum<W>(c.mism + c.over);
        kd = jb.len == 0 ? kAgNoBases : ungapped == 0 ? kAgAllMatch : kAgTracedJob;
        need = kd == kAgTracedJob ? (uint32_t)ag_steps(jb.len) : 0u;
    }
    if (lane == 0) { steps[s] = need; kind[s] = kd; }
}

// the largest b in (a, n_slots] whose slots a .. b - 1 need at most cap_steps of scratch; a + 1 where slot a alone needs more
__global__ void k_aligng_cut(const uint64_t* __restrict__ prefix, uint64_t n_slots, uint64_t a, uint64_t cap_steps, uint64_t* __restrict__ out /* [2]: b, steps */) {
    if (threadIdx.x || blockIdx.x) return;
    uint64_t lo = a + 1, hi = n_slots;                               // prefix[lo] - prefix[a] may exceed the cap: slot a then runs alone
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (prefix[mid] - prefix[a] <= cap_steps) lo = mid; else hi = mid - 1;
    }
    out[0] = lo; out[1] = prefix[lo] - prefix[a];
}

// ag_walk's fetch: a lane keeps its own word of the step the walk is in; the group takes the current lane's by shuffle
template <int W> struct AgFetchDev {
    const uint64_t* cells; uint32_t lane; uint64_t q_have; uint64_t word;
    __device__ __forceinline__ uint64_t operator()(uint64_t q, uint32_t l) {
        if (q != q_have) { word = cells[q * W + lane]; q_have = q; }
        return (uint64_t)__shfl((unsigned long long)word, (int)l, W);
    }
};

template <int W, bool WRITE> __global__ void __launch_bounds__(kAgBlock)
k_aligng_trace(const HitBatchDev B, const uint8_t* __restrict__ kind, const uint64_t* __restrict__ prefix, uint64_t a, uint64_t b, uint32_t k, int do_forward,
               uint64_t* cells /* the slice's */, uint8_t* lane_end /* [n_slots] */,
               uint32_t* __restrict__ n_ops /* [n_slots], !WRITE */, const uint64_t* __restrict__ woff /* [n_slots + 1], WRITE */, int32_t* __restrict__ pos_out,
               uint32_t* __restrict__ nm_out, uint64_t* __restrict__ op_off_out, uint32_t* __restrict__ ops_out, unsigned long long* ctr) {
    __shared__ unsigned long long s_ctr[kAgCounters];
    if (WRITE) hit_ctr_zero(s_ctr);
    const uint64_t s = a + (uint64_t)blockIdx.x * (kAgBlock / W) + threadIdx.x / W;
    const uint32_t lane = threadIdx.x % W;
    if (s < b) {                                                     // (a whole group)
        const uint8_t kd = kind[s];
        const int64_t lo = WRITE ? (int64_t)woff[s] : 0, hi = WRITE ? (int64_t)woff[s + 1] : 0;
        uint32_t* ops = (WRITE && lane == 0) ? ops_out : nullptr;
        AgTrace w{};
        if (kd >= kAgAllMatch) {
            const HitJobDev jb = hit_job_dev(B, B.hits[s >> 1], (uint32_t)(s & 1u), B.rec_read[s >> 1]);
            if (kd == kAgAllMatch) w = ag_all_match(jb.len, jb.pos, ops, lo, hi);
            else {
                uint64_t* mine = cells + (prefix[s] - prefix[a]) * W;
                uint32_t le;
                if (do_forward) { le = (uint32_t)hit_band_dev<W, true>(jb, k, lane, 0, mine); if (lane == 0) lane_end[s] = (uint8_t)le; }
                else le = lane_end[s];
                AgFetchDev<W> fetch{mine, lane, ~0ull, 0ull};
                w = ag_walk(jb.len, jb.pos, jb.tl, k, le, fetch, ops, lo, hi);
            }
        }
        if (lane == 0) {
            if (!WRITE) n_ops[s] = ag_n_ops(w);
            else {
                pos_out[s] = (int32_t)w.x0; nm_out[s] = w.nm; op_off_out[s] = (uint64_t)lo;
                if (s + 1 == B.n_slots) op_off_out[B.n_slots] = (uint64_t)hi;
                if (kd != kAgNoJob) atomicAdd(&s_ctr[kAgJobs], 1ull);
                if (kd == kAgTracedJob) atomicAdd(&s_ctr[kAgTraced], 1ull);
                if (kd != kAgNoJob && !w.started) atomicAdd(&s_ctr[kAgUnalignable], 1ull);
                if (w.nm) atomicAdd(&s_ctr[kAgSumNm], (unsigned long long)w.nm);
            }
        }
    }
    if (WRITE) hit_ctr_flush(s_ctr, ctr);
}

}  // namespace sfgpu

using namespace sfgpu;

struct AgSlice { uint64_t a, b, steps; };

extern "C" int sfgpu_hits_align_gapped(const sfgpu_index* x, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                       uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const sfgpu_align_gopts* opts,
                                       int32_t* d_pos, uint32_t* d_nm, uint64_t* d_op_off, uint32_t* d_ops, uint64_t cap_ops, uint64_t* n_ops,
                                       sfgpu_align_gstats* stats, sfgpu_stream stream) {
    SF_REQUIRE(x && opts && n_ops && stats && d_op_off, SFGPU_ERR_INVALID, "sfgpu_hits_align_gapped: null pointer");
    SF_REQUIRE(opts->max_indel >= 1u && opts->max_indel <= kVgMaxIndel, SFGPU_ERR_INVALID, "sfgpu_hits_align_gapped: max_indel is 1 .. 15");
    hipStream_t st = as_stream(stream);
    HitSlotPass sp("sfgpu_hits_align_gapped", x, d_seq1, d_off1, d_seq2, d_off2, n_reads, d_hits, d_hit_offsets, kAgCounters, st);
    int rc;
    if ((rc = sp.null_reads())) return rc;
    SF_REQUIRE(cap_ops == 0 || d_ops, SFGPU_ERR_INVALID, "sfgpu_hits_align_gapped: null operations");
    if ((rc = sp.count_records())) return rc;
    if (sp.n_rec == 0) {
        *n_ops = 0; *stats = sfgpu_align_gstats{};
        return sp.empty(d_op_off);
    }
    SF_REQUIRE(d_hits && d_pos && d_nm, SFGPU_ERR_INVALID, "sfgpu_hits_align_gapped: null records");
    const uint64_t n_slots = 2 * sp.n_rec;
    const uint32_t k = opts->max_indel, W = vg_width(k), per_block = kAgBlock / W;
    // (steps and cnt: n_slots + 1 entries, exclusive_scan_u32 reads one past the last)
    DevBuf<uint32_t> steps, cnt; DevBuf<uint8_t> kind, lane_end; DevBuf<uint64_t> prefix, woff, cells, cut;
    StreamSyncOnExit sync_first{st};          // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    if ((rc = steps.reserve(n_slots + 1, st, false)) || (rc = cnt.reserve(n_slots + 1, st, false)) || (rc = kind.reserve(n_slots, st, false)) ||
        (rc = lane_end.reserve(n_slots, st, false)) || (rc = prefix.reserve(n_slots + 1, st, false)) || (rc = woff.reserve(n_slots + 1, st, false)) ||
        (rc = cut.reserve(2, st, false)) || (rc = sp.start())) return rc;
    hipLaunchKernelGGL(W == 16u ? k_aligng_size<16> : k_aligng_size<32>, sp.grid(n_slots, per_block), dim3(kAgBlock), 0, st, sp.B, steps.p, kind.p, sp.ctr.p);
    SF_CHECK_LAUNCH();
    uint64_t total_steps = 0;
    if ((rc = sp.scan(steps.p, prefix.p, &total_steps, true))) return rc;
    // the slices
    const uint64_t cap_bytes = opts->scratch_cap_bytes ? opts->scratch_cap_bytes : kAgDefaultCap;
    const uint64_t cap_steps = cap_bytes / (8ull * W) ? cap_bytes / (8ull * W) : 1ull;
    std::vector<AgSlice> slices;
    uint64_t peak_steps = 0;
    if (total_steps <= cap_steps) { slices.push_back(AgSlice{0, n_slots, total_steps}); peak_steps = total_steps; }
    else {
        for (uint64_t a = 0; a < n_slots;) {
            uint64_t h_cut[2] = {0, 0};
            hipLaunchKernelGGL(k_aligng_cut, dim3(1), dim3(1), 0, st, prefix.p, n_slots, a, cap_steps, cut.p);
            SF_CHECK_LAUNCH();
            SF_HIP(hipMemcpyAsync(h_cut, cut.p, 16, hipMemcpyDeviceToHost, st));
            SF_HIP(hipStreamSynchronize(st));
            SF_REQUIRE(h_cut[0] > a && h_cut[0] <= n_slots, SFGPU_ERR_STATE, "sfgpu_hits_align_gapped: a slice without slots");
            slices.push_back(AgSlice{a, h_cut[0], h_cut[1]});
            peak_steps = h_cut[1] > peak_steps ? h_cut[1] : peak_steps;
            a = h_cut[0];
        }
    }
    if ((rc = cells.reserve(peak_steps * W, st, false))) return rc;
    auto count_kernel = W == 16u ? k_aligng_trace<16, false> : k_aligng_trace<32, false>;
    auto write_kernel = W == 16u ? k_aligng_trace<16, true> : k_aligng_trace<32, true>;
    for (const AgSlice& sl : slices) {
        hipLaunchKernelGGL(count_kernel, sp.grid(sl.b - sl.a, per_block), dim3(kAgBlock), 0, st, sp.B, kind.p, prefix.p, sl.a, sl.b, k, 1, cells.p, lane_end.p, cnt.p,
                           (const uint64_t*)nullptr, (int32_t*)nullptr, (uint32_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, sp.ctr.p);
        SF_CHECK_LAUNCH();
    }
    uint64_t total = 0;
    if ((rc = sp.scan(cnt.p, woff.p, &total, false))) return rc;
    *n_ops = total;
    if ((rc = sp.room(total, cap_ops, "operations"))) return rc;
    for (const AgSlice& sl : slices) {
        hipLaunchKernelGGL(write_kernel, sp.grid(sl.b - sl.a, per_block), dim3(kAgBlock), 0, st, sp.B, kind.p, prefix.p, sl.a, sl.b, k, (int)(slices.size() > 1), cells.p,
                           lane_end.p, (uint32_t*)nullptr, (const uint64_t*)woff.p, d_pos, d_nm, d_op_off, d_ops, sp.ctr.p);
        SF_CHECK_LAUNCH();
    }
    if ((rc = sp.finish())) return rc;
    stats->jobs = sp.h_ctr[kAgJobs]; stats->jobs_traced = sp.h_ctr[kAgTraced]; stats->unalignable = sp.h_ctr[kAgUnalignable]; stats->sum_nm = sp.h_ctr[kAgSumNm];
    stats->words = total; stats->scratch_bytes = peak_steps * W * 8ull;
    return SFGPU_OK;
}
