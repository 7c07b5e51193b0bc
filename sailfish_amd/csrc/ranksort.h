// ranksort.h -- the exact string sort on the device that the gene map (genemap.hip) and the collated alignment reader
// (samcollate.hip) share: rank refinement in rounds of 8 bytes.  The key of a round is the next 8 bytes of each string, big-endian
// and zero-padded; two stable sort_pairs_u64_u32 passes, by key and then by the current run, order the strings by (run, key), and a
// new run starts wherever either changes.  The rounds end when no run of several strings holds one with bytes behind the round: the
// strings of a run are then equal in every byte.  The first order is item order and every pass is stable, so inside a run of equal
// strings the items stay in item order.
//
// `Names` says what the strings are:
//   __device__ uint64_t key(uint32_t item, uint32_t round) const    bytes [8 round, 8 round + 8) of the item's string, the first byte
//                                                                   in the top bits, zeros behind its end
//   __device__ uint64_t bytes(uint32_t item) const                  its length
// Zero padding tells "a" from "a\0" only if the strings say so themselves: genemap.hip's names hold no NUL (a prefix then sorts
// first), samcollate.hip's begin with their length.
#pragma once
#include "common.h"
#include "primitives.h"

namespace sfgpu {
namespace ranksort {

constexpr int kBlock = 256;
inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

[[maybe_unused]] static __global__ void k_rank_init(uint32_t n, uint32_t* __restrict__ perm, uint32_t* __restrict__ run, uint32_t* __restrict__ iota) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    perm[j] = j; run[j] = 0; iota[j] = j;
}

template <typename Names>
__global__ void k_rank_keys(Names nm, uint32_t n, const uint32_t* __restrict__ perm, uint32_t round, uint64_t* __restrict__ key) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    key[j] = nm.key(perm[j], round);
}

[[maybe_unused]] static __global__ void k_rank_runs_of(uint32_t n, const uint32_t* __restrict__ run, const uint32_t* __restrict__ idx2, uint64_t* __restrict__ rk) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) rk[j] = run[idx2[j]];
}

// the new order: position j holds what stood at idx2[idx3[j]]; a run begins where the old run or the key changes
[[maybe_unused]] static __global__ void k_rank_apply(uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ idx2, const uint32_t* __restrict__ idx3,
                                                     const uint64_t* __restrict__ key2, const uint64_t* __restrict__ rk2, uint32_t* __restrict__ perm_out,
                                                     uint32_t* __restrict__ head) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    perm_out[j] = perm[idx2[idx3[j]]];
    head[j] = (j == 0 || rk2[j] != rk2[j - 1] || key2[idx3[j]] != key2[idx3[j - 1]]) ? 1u : 0u;
}

// run[j] from the scan of the heads; *more = 1 when a run of several strings holds one with bytes behind this round
template <typename Names>
__global__ void k_rank_runs(Names nm, uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ head_scan, uint32_t round,
                            uint32_t* __restrict__ run, uint32_t* __restrict__ more) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t mine = head_scan[j + 1] - 1;
    run[j] = mine;
    const bool shared = (j > 0 && head_scan[j] - 1 == mine) || (j + 1 < n && head_scan[j + 2] - 1 == mine);
    if (!shared) return;
    if (nm.bytes(perm[j]) > 8ull * (round + 1)) *more = 1;
}

struct RankScratch {
    DevBuf<uint64_t> key, key2, rk, rk2;
    DevBuf<uint32_t> iota, idx2, idx3, perm2, head, head_scan, more;
};

// perm[j] = the item at sorted position j (bytewise, equal strings in item order); run[j] = the number of distinct strings in front of
// position j's; *n_runs distinct strings.  h_pair: two pinned words.
template <typename Names>
int rank_strings(Names nm, uint32_t n, RankScratch& R, DevBuf<uint32_t>& perm, DevBuf<uint32_t>& run, uint32_t* n_runs, uint32_t* rounds,
                 uint32_t* h_pair, hipStream_t st) {
    *n_runs = 0;
    if (n == 0) return SFGPU_OK;
    for (DevBuf<uint64_t>* b : {&R.key, &R.key2, &R.rk, &R.rk2}) if (int r = b->reserve((uint64_t)n + 2, st, false)) return r;
    for (DevBuf<uint32_t>* b : {&R.iota, &R.idx2, &R.idx3, &R.perm2, &R.head, &R.head_scan, &perm, &run})
        if (int r = b->reserve((uint64_t)n + 3, st, false)) return r;
    if (int r = R.more.reserve(2, st, false)) return r;
    hipLaunchKernelGGL(k_rank_init, dim3(grid_of(n)), dim3(kBlock), 0, st, n, perm.p, run.p, R.iota.p);
    SF_CHECK_LAUNCH();
    for (uint32_t round = 0;; ++round) {
        hipLaunchKernelGGL(k_rank_keys<Names>, dim3(grid_of(n)), dim3(kBlock), 0, st, nm, n, perm.p, round, R.key.p);
        SF_CHECK_LAUNCH();
        if (int r = sort_pairs_u64_u32(R.key.p, R.key2.p, R.iota.p, R.idx2.p, n, st, 64, false)) return r;
        hipLaunchKernelGGL(k_rank_runs_of, dim3(grid_of(n)), dim3(kBlock), 0, st, n, run.p, R.idx2.p, R.rk.p);
        SF_CHECK_LAUNCH();
        if (int r = sort_pairs_u64_u32(R.rk.p, R.rk2.p, R.iota.p, R.idx3.p, n, st, 32, false)) return r;
        hipLaunchKernelGGL(k_rank_apply, dim3(grid_of(n)), dim3(kBlock), 0, st, n, perm.p, R.idx2.p, R.idx3.p, R.key2.p, R.rk2.p, R.perm2.p, R.head.p);
        SF_CHECK_LAUNCH();
        if (int r = exclusive_scan_u32_u32(R.head.p, R.head_scan.p, n, st)) return r;
        SF_HIP(hipMemsetAsync(R.more.p, 0, 4, st));
        hipLaunchKernelGGL(k_rank_runs<Names>, dim3(grid_of(n)), dim3(kBlock), 0, st, nm, n, R.perm2.p, R.head_scan.p, round, run.p, R.more.p);
        SF_CHECK_LAUNCH();
        SF_HIP(hipMemcpyAsync(perm.p, R.perm2.p, (uint64_t)n * 4, hipMemcpyDeviceToDevice, st));
        SF_HIP(hipMemcpyAsync(&h_pair[0], R.more.p, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(&h_pair[1], R.head_scan.p + n, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        if (rounds) ++*rounds;
        if (!h_pair[0]) break;
    }
    *n_runs = h_pair[1];
    return SFGPU_OK;
}

}  // namespace ranksort
}  // namespace sfgpu
