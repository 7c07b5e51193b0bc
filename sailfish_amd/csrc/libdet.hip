// libdet.hip -- sfgpu_hits_library_kinds: the tally of the library formats a batch's records show, behind lib_format "A" and
// aux/lib_format_counts.json.  WHAT a record's kind is, what a read adds and who votes is csrc/libdetfmt.h, stated once and run here
// unchanged; this file is only the way the work is laid out.
//
//   k_libdet_reads  a lane per read (256 a block), shaped like the filter's count pass: a block's reads own one contiguous range of
//                   records, which is copied to LDS with coalesced 8-byte loads (a lane walking 24-byte records in global memory makes
//                   every load touch 64 lines); a block whose range exceeds the stage walks global memory.  A lane ORs its records'
//                   kinds into a mask.  Nearly every read has records of one kind, so nothing is counted per record: per wavefront,
//                   one ballot per kind finds the reads of that kind and, where there are any, one shuffle sum adds their record
//                   counts -- an LDS histogram fed per record would put 64 lanes on one address, step after step.  Only a mixed read
//                   walks its records a second time and adds them to the block's LDS counters one by one.  The block's totals leave
//                   as one atomic per non-zero counter into one of 64 striped copies (same-address atomics serialise).
//                   The lane also writes the read's vote: a byte, its kind or 0xFF (and the flag the scan takes).
//   scan            primitives.h ranks the voters, only while the budget lasts
//   k_libdet_votes  a lane per read: the voters of rank < budget, by ballots per kind, to the same striped copies
#include "common.h"
#include "libdetfmt.h"
#include "primitives.h"

namespace sfgpu {

constexpr int kLdBlock = 256;
constexpr uint32_t kLdStage = 1536;                          // records: 36 KB, four blocks per CU
constexpr int kLdCopies = 64;
enum { kLdMapped = 0, kLdOver, kLdMixed, kLdCompat, kLdRecKind, kLdReadKind = kLdRecKind + kLdKinds, kLdVoteKind = kLdReadKind + kLdKinds,
       kLdCounters = kLdVoteKind + kLdKinds };
static_assert(kLdVoteKind <= kLdBlock, "a thread per block counter");

__device__ __forceinline__ unsigned long long ld_wave_sum(unsigned long long x) {
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) x += __shfl_xor(x, s, kWave);
    return x;
}

// P: const sfgpu_hit* in LDS or in global memory (two instantiations: the loads keep their address space)
template <typename P> __device__ __forceinline__ uint32_t ld_walk_mask(P h, uint32_t n, bool dovetail) {
    uint32_t mask = 0;
    for (uint32_t i = 0; i < n; ++i) mask |= 1u << ld_kind(h[i], dovetail);
    return mask;
}
template <typename P> __device__ __forceinline__ void ld_walk_count(P h, uint32_t n, bool dovetail, unsigned long long* s_ctr) {
    for (uint32_t i = 0; i < n; ++i) atomicAdd(&s_ctr[kLdRecKind + ld_kind(h[i], dovetail)], 1ull);
}

__global__ void __launch_bounds__(kLdBlock)
k_libdet_reads(const sfgpu_hit* __restrict__ hits, const uint32_t* __restrict__ off, uint32_t n_reads, uint32_t n_rec, sfgpu_libdet_opts o,
               uint32_t compat, uint8_t* __restrict__ vote, uint32_t* __restrict__ voter, unsigned long long* __restrict__ ctr) {
    __shared__ __attribute__((aligned(8))) sfgpu_hit s_hits[kLdStage];
    __shared__ unsigned long long s_ctr[kLdVoteKind];
    if (threadIdx.x < kLdVoteKind) s_ctr[threadIdx.x] = 0ull;
    // every record index is clamped to the batch's n_rec, and a staged read's to the block's range: offsets that are not what the
    // contract says give wrong counts, never a load outside the records
    const uint32_t r0 = blockIdx.x * kLdBlock;               // (the grid has no block past the reads)
    const uint32_t r1 = r0 + kLdBlock < n_reads ? r0 + kLdBlock : n_reads;
    uint32_t lo = off[r0], hi = off[r1];
    lo = lo < n_rec ? lo : n_rec; hi = hi < n_rec ? hi : n_rec;
    const bool staged = hi >= lo && hi - lo <= kLdStage;     // uniform
    if (staged) {
        const uint2* src = reinterpret_cast<const uint2*>(hits + lo);           // records are 24 bytes: 8-byte aligned
        uint2* dst = reinterpret_cast<uint2*>(s_hits);
        const uint32_t n8 = (hi - lo) * 3;
        for (uint32_t i = threadIdx.x; i < n8; i += kLdBlock) dst[i] = src[i];
    }
    __syncthreads();

    const bool dovetail = o.can_dovetail != 0;
    const uint32_t r = r0 + threadIdx.x;
    uint32_t mask = 0, n = 0, b = 0;
    bool mapped = false, over = false;
    if (r < n_reads) {
        uint32_t e = off[r + 1];
        b = off[r];
        b = b < n_rec ? b : n_rec; e = e < n_rec ? e : n_rec;
        if (staged) { b = b < lo ? lo : (b > hi ? hi : b); e = e > hi ? hi : e; }
        if (e < b) e = b;
        n = e - b;
        over = n > o.max_read_occs;
        mapped = n > 0 && !over;
        if (mapped) mask = staged ? ld_walk_mask(s_hits + (b - lo), n, dovetail) : ld_walk_mask(hits + b, n, dovetail);
    }
    const bool single = mapped && (mask & (mask - 1)) == 0;
    const uint32_t kind = single ? (uint32_t)__ffs(mask) - 1u : (uint32_t)kLdKinds;
    const bool lead = (threadIdx.x & (kWave - 1)) == 0;
    const unsigned long long b_mapped = __ballot(mapped), b_over = __ballot(over), b_mixed = __ballot(mapped && !single),
                             b_compat = __ballot(mapped && (mask & compat) != 0);
    if (lead) {
        if (b_mapped) atomicAdd(&s_ctr[kLdMapped], (unsigned long long)__popcll(b_mapped));
        if (b_over) atomicAdd(&s_ctr[kLdOver], (unsigned long long)__popcll(b_over));
        if (b_mixed) atomicAdd(&s_ctr[kLdMixed], (unsigned long long)__popcll(b_mixed));
        if (b_compat) atomicAdd(&s_ctr[kLdCompat], (unsigned long long)__popcll(b_compat));
    }
    for (uint32_t k = 0; k < kLdKinds; ++k) {
        const unsigned long long of_kind = __ballot(kind == k);
        if (!of_kind) continue;                              // uniform over the wavefront
        const unsigned long long recs = ld_wave_sum(kind == k ? n : 0u);
        if (lead) {
            atomicAdd(&s_ctr[kLdReadKind + k], (unsigned long long)__popcll(of_kind));
            atomicAdd(&s_ctr[kLdRecKind + k], recs);
        }
    }
    if (mapped && !single) {
        if (staged) ld_walk_count(s_hits + (b - lo), n, dovetail, s_ctr);
        else ld_walk_count(hits + b, n, dovetail, s_ctr);
    }
    if (vote && r < n_reads) {
        const uint32_t v = mapped ? ld_vote(mask, o.paired_library != 0) : kLdNoVote;
        vote[r] = (uint8_t)v;
        voter[r] = v != kLdNoVote;
    }
    __syncthreads();
    if (threadIdx.x < kLdVoteKind && s_ctr[threadIdx.x])
        atomicAdd(&ctr[(blockIdx.x % kLdCopies) * kLdCounters + threadIdx.x], s_ctr[threadIdx.x]);
}

__global__ void __launch_bounds__(kLdBlock)
k_libdet_votes(uint32_t n_reads, const uint8_t* __restrict__ vote, const uint64_t* __restrict__ rank, uint64_t budget,
               unsigned long long* __restrict__ ctr) {
    __shared__ unsigned int s_votes[kLdKinds];
    if (threadIdx.x < kLdKinds) s_votes[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t r = blockIdx.x * kLdBlock + threadIdx.x;
    uint32_t v = kLdNoVote;
    if (r < n_reads) { v = vote[r]; if (v != kLdNoVote && rank[r] >= budget) v = kLdNoVote; }
    const bool lead = (threadIdx.x & (kWave - 1)) == 0;
    for (uint32_t k = 0; k < kLdKinds; ++k) {
        const unsigned long long of_kind = __ballot(v == k);
        if (of_kind && lead) atomicAdd(&s_votes[k], (unsigned int)__popcll(of_kind));
    }
    __syncthreads();
    if (threadIdx.x < kLdKinds && s_votes[threadIdx.x])
        atomicAdd(&ctr[(blockIdx.x % kLdCopies) * kLdCounters + kLdVoteKind + threadIdx.x], (unsigned long long)s_votes[threadIdx.x]);
}

}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_hits_library_kinds(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, const sfgpu_libdet_opts* opts,
                                        int64_t* remaining_votes, sfgpu_libdet_stats* stats, sfgpu_stream stream) {
    SF_REQUIRE(opts && remaining_votes && stats && (d_hit_offsets || n_reads == 0), SFGPU_ERR_INVALID, "sfgpu_hits_library_kinds: null pointer");
    SF_REQUIRE(n_reads < 0x7FFFFFFFu, SFGPU_ERR_RANGE, "sfgpu_hits_library_kinds: a batch holds < 2^31 reads");
    if (n_reads == 0) return SFGPU_OK;
    hipStream_t st = as_stream(stream);
    uint32_t n_rec = 0;
    SF_HIP(hipMemcpyAsync(&n_rec, d_hit_offsets + n_reads, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    SF_REQUIRE(n_rec == 0 || d_hits, SFGPU_ERR_INVALID, "sfgpu_hits_library_kinds: null records");
    const bool want_votes = *remaining_votes > 0;
    const uint64_t budget = want_votes ? (uint64_t)*remaining_votes : 0;
    DevBuf<unsigned long long> ctr; DevBuf<uint8_t> vote; DevBuf<uint32_t> voter; DevBuf<uint64_t> rank;
    StreamSyncOnExit sync_first{st};          // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    int rc;
    if ((rc = ctr.reserve(kLdCopies * kLdCounters, st, false))) return rc;
    if (want_votes && ((rc = vote.reserve(n_reads, st, false)) || (rc = voter.reserve((uint64_t)n_reads + 1, st, false)) ||
                       (rc = rank.reserve((uint64_t)n_reads + 2, st, false)))) return rc;
    SF_HIP(hipMemsetAsync(ctr.p, 0, kLdCopies * kLdCounters * sizeof(unsigned long long), st));
    const dim3 grid((n_reads + kLdBlock - 1) / kLdBlock);
    const uint32_t compat = opts->has_expected ? ld_compat_mask(opts->expected) : 0u;
    hipLaunchKernelGGL(k_libdet_reads, grid, dim3(kLdBlock), 0, st, d_hits, d_hit_offsets, n_reads, n_rec, *opts, compat, vote.p, voter.p, ctr.p);
    SF_CHECK_LAUNCH();
    uint64_t h_voters = 0;
    if (want_votes) {
        SF_HIP(hipMemsetAsync(voter.p + n_reads, 0, 4, st));                    // (the scan's sentinel)
        if ((rc = exclusive_scan_u32(voter.p, rank.p, n_reads, st, false))) return rc;
        hipLaunchKernelGGL(k_libdet_votes, grid, dim3(kLdBlock), 0, st, n_reads, (const uint8_t*)vote.p, (const uint64_t*)rank.p, budget, ctr.p);
        SF_CHECK_LAUNCH();
        SF_HIP(hipMemcpyAsync(&h_voters, rank.p + n_reads, 8, hipMemcpyDeviceToHost, st));
    }
    static_assert(sizeof(unsigned long long) == 8, "the counters are 64 bits");
    unsigned long long h_copies[kLdCopies * kLdCounters];
    SF_HIP(hipMemcpyAsync(h_copies, ctr.p, sizeof h_copies, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    unsigned long long t[kLdCounters] = {};
    for (int c = 0; c < kLdCopies; ++c)
        for (int q = 0; q < kLdCounters; ++q) t[q] += h_copies[c * kLdCounters + q];
    const uint64_t taken = h_voters < budget ? h_voters : budget;
    *remaining_votes -= (int64_t)taken;
    stats->reads += n_reads; stats->reads_mapped += t[kLdMapped]; stats->reads_over_occs += t[kLdOver]; stats->reads_mixed += t[kLdMixed];
    stats->reads_compatible += t[kLdCompat]; stats->votes += taken;
    for (uint32_t k = 0; k < kLdKinds; ++k) {
        stats->records_kind[k] += t[kLdRecKind + k]; stats->reads_kind[k] += t[kLdReadKind + k]; stats->votes_kind[k] += t[kLdVoteKind + k];
    }
    return SFGPU_OK;
}
