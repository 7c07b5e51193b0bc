// posterior.hip -- sfgpu_hits_posteriors: the posterior probability of every record of a batch under a weight per transcript, with
// the record and the float a mappings file's ZW:f: tag holds for it.  WHAT a record's value is -- the weight read, the fixed order of
// the sum, the flush, the six digits -- is csrc/postfmt.h, stated once and run here unchanged; this file is only the way the work is
// laid out.
//
//   k_post_weights  a lane per transcript: the lowest weight the rule refuses (atomicMin)
//   k_post_tids     a lane per record: the lowest record whose tid is no transcript (atomicMin), and the record's tid to a dense
//                   array -- of a 24-byte record only these 4 bytes are needed, and they are read out of the records once
//   k_post_reads    a lane per read (256 a block).  A read of 1 .. 4 records is done by its lane: the tree over 4 leaves in
//                   registers.  A longer read is queued in LDS by its width class and taken, behind a barrier, by a lane group of
//                   8 (5 .. 8 records) or 16 (9 .. 16) lanes, or by a whole wavefront (17 and more): a lane holds the accumulator
//                   a_lane -- the read's records lane, lane + 64, ... in ascending order -- and the group adds them with
//                   __shfl_xor butterflies of k = W/2 .. 1, which is postfmt.h's tree over W leaves.  Every lane of the group then
//                   divides, decodes and stores its own records.  A read of 1000 records costs its wavefront 16 steps.
// The errors are found before k_post_reads runs, so the outputs stay untouched.
#include "common.h"
#include "hitgroup.h"
#include "postfmt.h"

namespace sfgpu {

constexpr int kPostBlock = kHitBlock;
// (the first two: the lowest bad record, the lowest bad weight)
enum { kPostMapped = kHitFirstCounter, kPostMulti, kPostFlat, kPostZero, kPostMax, kPostCounters };
static_assert(kPostCounters <= kHitMaxCounters, "the counters of a hit pass");

__global__ void __launch_bounds__(kPostBlock)
k_post_weights(const double* __restrict__ w, uint64_t n_refs, unsigned long long* ctr) {
    const uint64_t t = (uint64_t)blockIdx.x * kPostBlock + threadIdx.x;
    if (t < n_refs && post_weight_bad(w[t])) atomicMin(&ctr[1], (unsigned long long)t);
}

__global__ void __launch_bounds__(kPostBlock)
k_post_tids(const sfgpu_hit* __restrict__ hits, uint64_t n_rec, uint64_t n_refs, uint32_t* __restrict__ tid, unsigned long long* ctr) {
    const uint64_t h = (uint64_t)blockIdx.x * kPostBlock + threadIdx.x;
    if (h >= n_rec) return;
    const uint32_t t = hits[h].tid;
    tid[h] = t;
    if (t >= n_refs) atomicMin(&ctr[0], (unsigned long long)h);
}

__device__ __forceinline__ uint32_t post_store(double x, double S, uint64_t n, uint64_t at, double* __restrict__ p, uint32_t* __restrict__ rec, float* __restrict__ f32) {
    const PostValue v = post_value(x, S, n);
    p[at] = v.p; rec[at] = v.rec; f32[at] = v.f32;
    return v.p == 0.0 ? 1u : 0u;
}

// records [b, b + n) of one read by a group of W lanes (n <= W unless W is the wavefront) -> the records this lane wrote as 0; *flat in every lane
template <int W>
__device__ __forceinline__ uint32_t post_group(uint64_t b, uint64_t n, uint32_t lane, const uint32_t* __restrict__ tid, const double* __restrict__ w,
                                               double* __restrict__ p, uint32_t* __restrict__ rec, float* __restrict__ f32, bool* flat) {
    double a = 0.0, mine = 0.0;
    for (uint64_t i = lane; i < n; i += W) { mine = post_weight(w[tid[b + i]]); a = a + mine; }
#pragma unroll
    for (int k = W / 2; k > 0; k >>= 1) a = a + __shfl_xor(a, k, W);
    *flat = !(a > 0.0);
    uint32_t zero = 0;
    if (n <= (uint64_t)W) { if (lane < n) zero = post_store(mine, a, n, b + lane, p, rec, f32); }
    else for (uint64_t i = lane; i < n; i += W) zero += post_store(post_weight(w[tid[b + i]]), a, n, b + i, p, rec, f32);
    return zero;
}

template <int W>
__device__ __forceinline__ void post_queue(const uint32_t* queue, uint32_t n_queued, const uint32_t* __restrict__ hit_off, uint64_t n_rec, const uint32_t* __restrict__ tid,
                                           const double* __restrict__ w, double* __restrict__ p, uint32_t* __restrict__ rec, float* __restrict__ f32,
                                           unsigned long long* s_ctr) {
    const uint32_t lane = threadIdx.x % W;
    for (uint32_t i = threadIdx.x / W; i < n_queued; i += kPostBlock / W) {          // (a whole group)
        uint64_t b, e;
        hit_range(hit_off, queue[i], n_rec, &b, &e);
        bool flat;
        const uint32_t zero = post_group<W>(b, e - b, lane, tid, w, p, rec, f32, &flat);
        if (zero) atomicAdd(&s_ctr[kPostZero], (unsigned long long)zero);
        if (flat && lane == 0) atomicAdd(&s_ctr[kPostFlat], 1ull);
    }
}

__global__ void __launch_bounds__(kPostBlock)
k_post_reads(uint64_t n_reads, const uint32_t* __restrict__ hit_off, uint64_t n_rec, const uint32_t* __restrict__ tid, const double* __restrict__ w,
             double* __restrict__ p, uint32_t* __restrict__ rec, float* __restrict__ f32, unsigned long long* ctr) {
    __shared__ unsigned long long s_ctr[kPostCounters];
    __shared__ uint32_t s_queue[3][kPostBlock];
    __shared__ uint32_t s_queued[3];
    if (threadIdx.x < 3) s_queued[threadIdx.x] = 0u;
    hit_ctr_zero(s_ctr);
    const uint64_t r = (uint64_t)blockIdx.x * kPostBlock + threadIdx.x;
    if (r < n_reads) {
        uint64_t b, e;
        hit_range(hit_off, r, n_rec, &b, &e);
        const uint64_t n = e - b;
        if (n) {
            atomicAdd(&s_ctr[kPostMapped], 1ull);
            if (n >= 2) atomicAdd(&s_ctr[kPostMulti], 1ull);
            atomicMax(&s_ctr[kPostMax], (unsigned long long)n);
        }
        if (n > 4) {
            const int cls = n <= 8 ? 0 : n <= 16 ? 1 : 2;
            s_queue[cls][atomicAdd(&s_queued[cls], 1u)] = (uint32_t)r;
        } else if (n) {
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = (uint64_t)i < n ? post_weight(w[tid[b + i]]) : 0.0;
            const double S = post_sum4(x[0], x[1], x[2], x[3]);
            uint32_t zero = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) if ((uint64_t)i < n) zero += post_store(x[i], S, n, b + i, p, rec, f32);
            if (zero) atomicAdd(&s_ctr[kPostZero], (unsigned long long)zero);
            if (!(S > 0.0)) atomicAdd(&s_ctr[kPostFlat], 1ull);
        }
    }
    __syncthreads();
    post_queue<8>(s_queue[0], s_queued[0], hit_off, n_rec, tid, w, p, rec, f32, s_ctr);
    post_queue<16>(s_queue[1], s_queued[1], hit_off, n_rec, tid, w, p, rec, f32, s_ctr);
    post_queue<kWave>(s_queue[2], s_queued[2], hit_off, n_rec, tid, w, p, rec, f32, s_ctr);
    hit_ctr_flush<kPostCounters, kPostMax>(s_ctr, ctr);
}

}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_hits_posteriors(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, const double* d_weights, uint64_t n_refs,
                                     double* d_p, uint32_t* d_rec, float* d_f32, sfgpu_posterior_stats* stats, sfgpu_stream stream) {
    const char* who = "sfgpu_hits_posteriors";
    SF_REQUIRE(stats && (d_weights || n_refs == 0) && (d_hit_offsets || n_reads == 0), SFGPU_ERR_INVALID, "sfgpu_hits_posteriors: null pointer");
    hipStream_t st = as_stream(stream);
    uint64_t n_rec = 0;
    if (int rc = hit_n_rec(d_hit_offsets, n_reads, st, &n_rec)) return rc;
    SF_REQUIRE(n_rec == 0 || (d_hits && d_p && d_rec && d_f32), SFGPU_ERR_INVALID, "sfgpu_hits_posteriors: null records");
    DevBuf<uint32_t> tid; DevBuf<unsigned long long> ctr;
    StreamSyncOnExit sync_first{st};          // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    unsigned long long h_ctr[kPostCounters] = {~0ull, ~0ull};
    int rc;
    if ((rc = ctr.reserve(kPostCounters, st, false)) || (rc = tid.reserve(n_rec ? n_rec : 1, st, false))) return rc;
    SF_HIP(hipMemcpyAsync(ctr.p, h_ctr, sizeof h_ctr, hipMemcpyHostToDevice, st));
    auto grid = [](uint64_t n) { return dim3((unsigned)((n + kPostBlock - 1) / kPostBlock)); };
    if (n_refs) {
        hipLaunchKernelGGL(k_post_weights, grid(n_refs), dim3(kPostBlock), 0, st, d_weights, n_refs, ctr.p);
        SF_CHECK_LAUNCH();
    }
    if (n_rec) {
        hipLaunchKernelGGL(k_post_tids, grid(n_rec), dim3(kPostBlock), 0, st, d_hits, n_rec, n_refs, tid.p, ctr.p);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, 2 * sizeof h_ctr[0], hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h_ctr[1] != ~0ull) {
        set_error("%s: the weight of transcript %llu is negative, not finite or above 2^960", who, h_ctr[1]);
        return SFGPU_ERR_INVALID;
    }
    if (h_ctr[0] != ~0ull) {
        set_error("%s: record %llu names transcript >= %llu", who, h_ctr[0], (unsigned long long)n_refs);
        return SFGPU_ERR_RANGE;
    }
    if (n_rec) {
        hipLaunchKernelGGL(k_post_reads, grid(n_reads), dim3(kPostBlock), 0, st, (uint64_t)n_reads, d_hit_offsets, n_rec, (const uint32_t*)tid.p, d_weights, d_p, d_rec,
                           d_f32, ctr.p);
        SF_CHECK_LAUNCH();
        SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
    }
    *stats = sfgpu_posterior_stats{};
    stats->reads = n_reads; stats->records = n_rec;
    stats->reads_mapped = h_ctr[kPostMapped]; stats->reads_multi = h_ctr[kPostMulti]; stats->reads_flat = h_ctr[kPostFlat];
    stats->records_zero = h_ctr[kPostZero]; stats->max_records = h_ctr[kPostMax];
    return SFGPU_OK;
}
