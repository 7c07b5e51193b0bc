// hitgroup.h -- the device toolkit of the passes over the mapper's hit records (verify.hip, align_gapped.hip): what a
// group of W lanes (16 or 32, lanes of one wavefront) does that is the same in every pass, stated once.  The rules are the format
// headers' (verifyfmt.h, verifygfmt.h, aligngfmt.h); this file is only the way the work is laid out.
//   group_sum / group_min   over the W lanes of a group, the result in every lane
//   hit_job_dev             a record's job j of read r: its mate, its transcript, strand and position
//   hit_range               a read's records, clamped to the batch's record count
//   hit_bad_record          the two errors a record can carry; the first two counters of every pass name the lowest such record
//   hit_band_dev<W, CELLS>  the band's forward pass (verifygfmt.h's row; lanes are DIAGONALS) -- the ONE device statement of it
//   k_hits_fill<Score>      survivors and their scores to their places, a lane per read
//   hit_n_rec, hit_report_bad   the host side the entry functions share
#pragma once
#include "common.h"
#include "aligngfmt.h"

namespace sfgpu {

constexpr int kHitBlock = 256;
enum { kHitBadTid = 0, kHitBadMate, kHitFirstCounter };              // ctr[0 .. 1] of every pass: atomicMin of the record's index

template <int W> __device__ __forceinline__ uint64_t group_sum(uint64_t v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor((unsigned long long)v, o, W);
    return v;
}
template <int W> __device__ __forceinline__ uint32_t group_min(uint32_t v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(v, o, W); v = u < v ? u : v; }
    return v;
}

struct HitJobDev { const char* m; const char* t; uint64_t len, tl; int64_t pos; bool fwd; };
__device__ __forceinline__ HitJobDev hit_job_dev(const sfgpu_hit& h, uint32_t j, uint64_t r, const char* tseq, const uint64_t* tseq_off, const uint32_t* tlen,
                                                 const char* seq1, const uint64_t* off1, const char* seq2, const uint64_t* off2) {
    const VfJob jb = vf_job(h, j);
    const uint64_t* off = jb.mate ? off2 : off1;
    const uint64_t mb = off[r];
    return HitJobDev{(jb.mate ? seq2 : seq1) + mb, tseq + tseq_off[h.tid], off[r + 1] - mb, tlen[h.tid], (int64_t)jb.pos, jb.fwd};
}

// records [b, e) of read r
__device__ __forceinline__ void hit_range(const uint32_t* hit_off, uint64_t r, uint64_t n_rec, uint64_t* b, uint64_t* e) {
    const uint64_t hi = hit_off[r + 1], lo = hit_off[r];
    *e = hi < n_rec ? hi : n_rec; *b = lo < *e ? lo : *e;
}

// -> kHitBadTid (tid >= M), kHitBadMate (mate 2 of a single-end batch), or -1
__device__ __forceinline__ int hit_bad_record(const sfgpu_hit& h, uint64_t M, const char* seq2) {
    if (h.tid >= M) return kHitBadTid;
    return ((h.mate_status == 2 || vf_n_jobs(h) > 1) && !seq2) ? kHitBadMate : -1;
}

// the banded recurrence of one job over the group's lanes (the same result in every lane of the group).
// CELLS == false -> the job's edits, or kVgFail once the band's minimum exceeds max_edits: no lower-neighbour exchange, no stores.
// CELLS == true  -> the end lane; every kVfStep rows a lane stores the 4 bits of its 16 cells as one word, the group W consecutive
//                   words of `cells`; never stops early (max_edits is not read).
template <int W, bool CELLS>
__device__ __forceinline__ uint64_t hit_band_dev(const HitJobDev& jb, uint32_t k, uint32_t lane, uint64_t max_edits, uint64_t* __restrict__ cells) {
    uint32_t D = vg_lane_start(lane, k), m = 0;
    for (uint64_t i0 = 0; i0 < jb.len; i0 += kVfStep) {
        const uint32_t mask = vg_lane_submask(vf_mate_window(jb.m, (int64_t)jb.len, jb.fwd, (int64_t)i0), jb.t, jb.tl, jb.pos, i0, lane, k, jb.fwd);
        const uint32_t n = jb.len - i0 < kVfStep ? (uint32_t)(jb.len - i0) : kVfStep;
        [[maybe_unused]] uint64_t word = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t up = __shfl_down(D, 1, W), sub = (mask >> j) & 1u;      // (lane W - 1 gets its own: it is never in the band)
            uint32_t key = vg_key(vg_lane_v(D, up, sub), lane, W);
#pragma unroll
            for (int o = 1; o < W; o <<= 1) key = vg_scan_step(key, __shfl_up(key, o, W), lane, (uint32_t)o);
            const uint32_t nd = vg_lane_d(key, lane, W, k);
            if constexpr (CELLS) word |= (uint64_t)ag_lane_cand(D, up, sub, nd, __shfl_up(nd, 1, W), lane, k) << (4u * j);
            D = nd;
        }
        if constexpr (CELLS) cells[(i0 / kVfStep) * W + lane] = word;              // (the group: W consecutive words)
        else { m = group_min<W>(D); if (m > max_edits) return kVgFail; }
    }
    if constexpr (CELLS) { m = group_min<W>(D); return ag_rank_lane(group_min<W>(ag_end_rank(D, m, lane, k)), k); }
    else return m;
}

template <typename Score> __global__ void __launch_bounds__(kHitBlock)
k_hits_fill(uint64_t n_reads, const sfgpu_hit* __restrict__ hits, const uint32_t* __restrict__ hit_off, uint64_t n_rec, const uint8_t* __restrict__ keep,
            const Score* __restrict__ score, const uint64_t* __restrict__ out_off, sfgpu_hit* __restrict__ hits_out, uint32_t* __restrict__ offsets_out,
            Score* __restrict__ scores_out) {
    const uint64_t r = (uint64_t)blockIdx.x * kHitBlock + threadIdx.x;
    if (r > n_reads) return;
    uint64_t o = out_off[r];
    offsets_out[r] = (uint32_t)o;
    if (r == n_reads) return;
    uint64_t b, e;
    hit_range(hit_off, r, n_rec, &b, &e);
    for (uint64_t i = b; i < e; ++i) {
        if (!keep[i]) continue;
        hits_out[o] = hits[i];
        if (scores_out) scores_out[o] = score[i];
        ++o;
    }
}

// ---- the host side of an entry function -----------------------------------------------------------------------------------------
// the batch's record count, from the end of the offsets (the stream is waited for)
inline int hit_n_rec(const uint32_t* d_hit_offsets, uint32_t n_reads, hipStream_t st, uint64_t* n_rec) {
    uint32_t n = 0;
    if (n_reads) {
        SF_HIP(hipMemcpyAsync(&n, d_hit_offsets + n_reads, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
    }
    *n_rec = n;
    return SFGPU_OK;
}
// what the first two counters found, as the error of `entry` -> SFGPU_OK where they found nothing
inline int hit_report_bad(const char* entry, const unsigned long long* h_ctr, uint64_t M) {
    if (h_ctr[kHitBadTid] != ~0ull) {
        set_error("%s: record %llu names transcript >= %llu", entry, h_ctr[kHitBadTid], (unsigned long long)M);
        return SFGPU_ERR_RANGE;
    }
    if (h_ctr[kHitBadMate] != ~0ull) {
        set_error("%s: record %llu names mate 2 of a single-end batch", entry, h_ctr[kHitBadMate]);
        return SFGPU_ERR_INVALID;
    }
    return SFGPU_OK;
}

}  // namespace sfgpu
