// hitgroup.h -- the toolkit of the passes over the mapper's hit records (verify.hip, align_gapped.hip, mdtag.hip):
// what a group of W lanes (16 or 32, lanes of one wavefront) does that is the same in every pass, and what the entry functions of
// the slot passes do alike on the host, stated once.  The rules are the format headers' (verifyfmt.h, verifygfmt.h, aligngfmt.h,
// mdfmt.h); this file is only the way the work is laid out.
//   group_sum / group_min   over the W lanes of a group, the result in every lane
//   HitBatchDev             the batch as the kernels take it, by value: transcripts, reads, records (and a slot pass's rec_read, n_slots)
//   hit_job_dev             a record's job j of read r: its mate, its transcript, strand and position
//   hit_range               a read's records, clamped to the batch's record count
//   hit_bad_record          the two errors a record can carry; the first two counters of every pass name the lowest such record
//   hit_ctr_zero / hit_ctr_flush   a block's counters in LDS: zeroed, then one global atomic per counter and block (one may be a maximum)
//   hit_band_dev<W, CELLS>  the band's forward pass (verifygfmt.h's row; lanes are DIAGONALS) -- the ONE device statement of it
//   k_hits_fill<Score>      survivors and their scores to their places, a lane per read
//   k_hits_rec_read         a lane per read names the read of each of its records (two slots per record: slot 2 h + j)
//   hit_n_rec, hit_report_bad   the host side the entry functions share
//   HitSlotPass             the host side of a slot pass (count -> scan -> write): record count, rec_read, counters, scan and refusal
#pragma once
#include "common.h"
#include "aligngfmt.h"
#include "mapidx.h"
#include "primitives.h"

namespace sfgpu {

constexpr int kHitBlock = 256, kHitMaxCounters = 8;
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

struct HitBatchDev {
    const char* tseq; const uint64_t* tseq_off; const uint32_t* tlen; uint64_t M;
    const char* seq1; const uint64_t* off1; const char* seq2; const uint64_t* off2;
    const sfgpu_hit* hits;
    const uint32_t* rec_read = nullptr; uint64_t n_slots = 0;       // a slot pass's: HitSlotPass::start fills them
    HitBatchDev(const sfgpu_index* x, const char* s1, const uint64_t* o1, const char* s2, const uint64_t* o2, const sfgpu_hit* h)
        : tseq(x->tseq.p), tseq_off(x->tseq_off.p), tlen(x->tlen.p), M(x->M), seq1(s1), off1(o1), seq2(s2), off2(o2), hits(h) {}
};

struct HitJobDev { const char* m; const char* t; uint64_t len, tl; int64_t pos; bool fwd; };
__device__ __forceinline__ HitJobDev hit_job_dev(const HitBatchDev& B, const sfgpu_hit& h, uint32_t j, uint64_t r) {
    const VfJob jb = vf_job(h, j);
    const uint64_t* off = jb.mate ? B.off2 : B.off1;
    const uint64_t mb = off[r];
    return HitJobDev{(jb.mate ? B.seq2 : B.seq1) + mb, B.tseq + B.tseq_off[h.tid], off[r + 1] - mb, B.tlen[h.tid], (int64_t)jb.pos, jb.fwd};
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

// a block's counters [kHitFirstCounter, N) in LDS (every thread of the block calls both); MAX: the counter that is a maximum, not a sum
template <int N> __device__ __forceinline__ void hit_ctr_zero(unsigned long long (&s_ctr)[N]) {
    if (threadIdx.x < N) s_ctr[threadIdx.x] = 0ull;
    __syncthreads();
}
template <int N, int MAX = -1> __device__ __forceinline__ void hit_ctr_flush(const unsigned long long (&s_ctr)[N], unsigned long long* ctr) {
    __syncthreads();
    if (threadIdx.x < kHitFirstCounter || threadIdx.x >= N || !s_ctr[threadIdx.x]) return;
    if ((int)threadIdx.x == MAX) atomicMax(&ctr[threadIdx.x], s_ctr[threadIdx.x]);
    else atomicAdd(&ctr[threadIdx.x], s_ctr[threadIdx.x]);
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

template <int BLOCK = kHitBlock> __global__ void __launch_bounds__(BLOCK)     // (a template only so that the files that include this may each hold it)
k_hits_rec_read(uint64_t n_reads, const uint32_t* __restrict__ hit_off, uint64_t n_rec, uint32_t* __restrict__ rec_read) {
    const uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_reads) return;
    uint64_t b, e;
    hit_range(hit_off, r, n_rec, &b, &e);
    for (uint64_t i = b; i < e; ++i) rec_read[i] = (uint32_t)r;
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

// A slot pass (align_gapped.hip, mdtag.hip): two slots per record, count -> scan -> write.  The entry declares it BEFORE its own
// DevBufs and its StreamSyncOnExit after them all, so that an early return waits for the kernels before any scratch goes back.
struct HitSlotPass {
    const char* entry; hipStream_t st; uint32_t n_reads; const uint32_t* hit_off; int n_ctr; HitBatchDev B; uint64_t n_rec = 0;
    DevBuf<uint32_t> rec_read; DevBuf<unsigned long long> ctr; unsigned long long h_ctr[kHitMaxCounters] = {~0ull, ~0ull};
    HitSlotPass(const char* entry_, const sfgpu_index* x, const char* s1, const uint64_t* o1, const char* s2, const uint64_t* o2, uint32_t n_reads_,
                const sfgpu_hit* hits, const uint32_t* hit_off_, int n_ctr_, hipStream_t st_)
        : entry(entry_), st(st_), n_reads(n_reads_), hit_off(hit_off_), n_ctr(n_ctr_), B(x, s1, o1, s2, o2, hits) {}
    int null_reads() const {
        if (n_reads == 0 || (B.seq1 && B.off1 && hit_off && (!B.seq2 || B.off2))) return SFGPU_OK;
        set_error("%s: null reads", entry);
        return SFGPU_ERR_INVALID;
    }
    int count_records() { return hit_n_rec(hit_off, n_reads, st, &n_rec); }
    // no records: the output's offsets are one 0
    int empty(uint64_t* d_off) { SF_HIP(hipMemsetAsync(d_off, 0, 8, st)); SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }
    // rec_read and the counters {~0, ~0, 0 ...}; B is complete from here on
    int start() {
        int rc = rec_read.reserve(n_rec, st, false);
        if (rc || (rc = ctr.reserve(n_ctr, st, false))) return rc;
        SF_HIP(hipMemcpyAsync(ctr.p, h_ctr, n_ctr * sizeof h_ctr[0], hipMemcpyHostToDevice, st));
        SF_HIP(hipMemsetAsync(rec_read.p, 0xFF, n_rec * 4, st));
        hipLaunchKernelGGL(k_hits_rec_read<>, dim3((unsigned)(((uint64_t)n_reads + kHitBlock - 1) / kHitBlock)), dim3(kHitBlock), 0, st, (uint64_t)n_reads, hit_off, n_rec, rec_read.p);
        SF_CHECK_LAUNCH();
        B.rec_read = rec_read.p; B.n_slots = 2 * n_rec;
        return SFGPU_OK;
    }
    dim3 grid(uint64_t slots, uint32_t per_block) const { return dim3((unsigned)((slots + per_block - 1) / per_block)); }
    // a count pass's cnt[n_slots + 1] -> its CSR off[n_slots + 1] and *total, one wait; errors: the counters come back too, and what the first two found fails the entry
    int scan(const uint32_t* cnt, uint64_t* off, uint64_t* total, bool errors) {
        if (int rc = exclusive_scan_u32(cnt, off, B.n_slots, st, false)) return rc;
        if (errors) SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, n_ctr * sizeof h_ctr[0], hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(total, off + B.n_slots, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        return errors ? hit_report_bad(entry, h_ctr, B.M) : SFGPU_OK;
    }
    // more than the caller has room for: refused before anything is written
    int room(uint64_t total, uint64_t cap, const char* what) const {
        if (total <= cap) return SFGPU_OK;
        set_error("%s: %llu %s, room for %llu", entry, (unsigned long long)total, what, (unsigned long long)cap);
        return SFGPU_ERR_RANGE;
    }
    // after the write pass: the counters, in h_ctr
    int finish() { SF_HIP(hipMemcpyAsync(h_ctr, ctr.p, n_ctr * sizeof h_ctr[0], hipMemcpyDeviceToHost, st)); SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }
};

}  // namespace sfgpu
