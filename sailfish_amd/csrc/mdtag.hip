// mdtag.hip -- sfgpu_hits_md_tags: the NM and MD tags of the lines a mappings file holds for a batch of hit records.  WHAT a
// slot's tags are -- the CIGAR walked, what a mismatch is, the reference character -- is csrc/mdfmt.h, stated once and run here
// unchanged; this file is only the way the work is laid out, and what the hit passes share of that -- the batch, the job decode,
// the block's counters, the slot pass's host side (HitSlotPass) -- is csrc/hitgroup.h.
//
// Two slots per record (slot 2 h + which is line `which` of record h); count -> scan -> write:
//   k_hits_rec_read     (hitgroup.h) a lane per read names the read of each of its records
//   k_mdtag_walk<false> a group of 16 lanes per slot walks the slot's CIGAR.  Along an M run a lane takes 16 columns per step
//                       (vf_window's clipped 16-byte loads, md_mask16: a 16-bit mismatch mask in registers), so the group 256; the
//                       matches behind a lane's last mismatch reach the next lane's first token through a segmented shuffle scan
//                       (md_seg_join), a lane sums dec_len + 1 over its own tokens, and the group adds the lanes' bytes.  A
//                       deletion is <run>^ and one reference character a lane and step.  This pass only counts: bytes per slot.
//                       Errors are found here.
//   scan                bytes -> the MD's CSR; too many for the caller's room: SFGPU_ERR_RANGE, nothing written
//   k_mdtag_walk<true>  the same walk again: every lane places its tokens from the exclusive prefix of the lanes' bytes, lane 0
//                       the numbers in front of a deletion and at the end; nm, md_off and the counters are written here.
// A step whose masks are all 0 -- on real data nearly every one -- runs neither token loop nor the byte scan: a load pair, the
// segment scan, and <len> at the slot's end.  Stores are plain byte stores from vector registers.
#include "common.h"
#include "mapidx.h"
#include "primitives.h"
#include "hitgroup.h"
#include "mdfmt.h"

namespace sfgpu {

constexpr int kMdBlock = kHitBlock;
constexpr int kMdW = 16;
enum { kMdSlots = kHitFirstCounter, kMdSumNm, kMdMax, kMdPlain, kMdCounters };

// the lane's bytes of a number at out[at ..]
__device__ __forceinline__ uint32_t md_put_number_dev(uint8_t* out, uint64_t at, uint32_t v) {
    const int nd = dec_len_u32(v);
    dec_put_fixed_u32(v, nd, 0, [&](int i, char ch) { out[at + (uint64_t)(nd - 1 - i)] = (uint8_t)ch; });
    return (uint32_t)nd;
}

// One slot by its group (the same `at`, `run` and return value in every lane).  WRITE: the bytes go to out[0 ..); else out is not
// touched.  -> the MD's bytes; *nm_out the slot's nm
template <bool WRITE>
__device__ __forceinline__ uint64_t md_slot_dev(const MdCigar& c, const HitJobDev& jb, uint32_t lane, uint8_t* out, uint32_t* nm_out) {
    uint64_t q = 0, at = 0;
    int64_t x = c.x0;
    uint32_t run = 0, nm = 0, mine = 0;           // mine: this lane's mismatches, summed over the group at the end
    for (uint32_t i = 0; i < c.n_ops; ++i) {
        const uint32_t w = md_op(c, i), n = w >> 4, op = w & 15u;
        if (op == 4u) q += n;
        else if (op == 1u) { q += n; nm += n; }
        else if (md_is_del_op(op)) {
            const uint32_t nd = (uint32_t)dec_len_u32(run);
            if (WRITE) {
                if (lane == 0) { md_put_number_dev(out, at, run); out[at + nd] = (uint8_t)'^'; }
                for (uint32_t j = lane; j < n; j += kMdW) out[at + nd + 1u + j] = md_ref_at(jb.t, jb.tl, x + (int64_t)j);
            }
            at += (uint64_t)nd + 1u + n; run = 0; nm += n; x += n;
        } else if (md_is_match_op(op)) {
            for (uint64_t c0 = 0; c0 < n; c0 += (uint64_t)kMdW * kVfStep) {
                const uint64_t c1 = c0 + (uint64_t)lane * kVfStep;
                const uint32_t cols = c1 >= n ? 0u : (n - c1 < kVfStep ? (uint32_t)(n - c1) : kVfStep);
                uint32_t mask = 0;
                VfWin tw{0, 0};
                if (cols) {
                    tw = vf_window(jb.t, (int64_t)jb.tl, x + (int64_t)c1);
                    mask = md_mask16(vf_mate_window(jb.m, (int64_t)jb.len, jb.fwd, (int64_t)(q + c1)), tw, jb.fwd) & ((1u << cols) - 1u);
                }
                uint32_t seg = md_seg(mask, cols);                   // inclusive scan of the segments over the group
#pragma unroll
                for (int o = 1; o < kMdW; o <<= 1) {
                    const uint32_t left = __shfl_up(seg, o, kMdW);
                    if (lane >= (uint32_t)o) seg = md_seg_join(left, seg);
                }
                const uint32_t all = __shfl(seg, kMdW - 1, kMdW);
                if (all & kMdCut) {                                  // (the group's decision) a mismatch somewhere in the step
                    uint32_t left = __shfl_up(seg, 1, kMdW);
                    if (lane == 0) left = 0u;
                    const uint32_t carry = md_seg_run(left, run);
                    uint32_t bytes = 0;
                    md_lane_tokens(mask, carry, tw, [&](uint32_t v, uint8_t) { bytes += md_token_len(v); });
                    uint32_t incl = bytes;                           // prefix sum of the lanes' bytes
#pragma unroll
                    for (int o = 1; o < kMdW; o <<= 1) {
                        const uint32_t up = __shfl_up(incl, o, kMdW);
                        if (lane >= (uint32_t)o) incl += up;
                    }
                    if (WRITE) {
                        uint64_t place = at + (incl - bytes);
                        md_lane_tokens(mask, carry, tw, [&](uint32_t v, uint8_t ch) {
                            const uint32_t nd = md_put_number_dev(out, place, v);
                            out[place + nd] = ch;
                            place += nd + 1u;
                        });
                    }
                    at += __shfl(incl, kMdW - 1, kMdW);
                    mine += vf_popc(mask);
                }
                run = md_seg_run(all, run);
            }
            q += n; x += n;
        }
    }
    if (WRITE && lane == 0) md_put_number_dev(out, at, run);
    at += (uint32_t)dec_len_u32(run);
    *nm_out = nm + (uint32_t)group_sum<kMdW>((uint64_t)mine);
    return at;
}

template <bool WRITE> __global__ void __launch_bounds__(kMdBlock)
k_mdtag_walk(const HitBatchDev B, const int32_t* __restrict__ aln_pos, const uint64_t* __restrict__ aln_op_off, const uint32_t* __restrict__ aln_ops, uint32_t* __restrict__ bytes /* [n_slots], !WRITE */,
             const uint64_t* __restrict__ woff /* [n_slots + 1], WRITE */, uint32_t* __restrict__ nm_out, uint64_t* __restrict__ md_off_out,
             uint8_t* __restrict__ md_out, unsigned long long* ctr) {
    __shared__ unsigned long long s_ctr[kMdCounters];
    if (WRITE) hit_ctr_zero(s_ctr);
    const uint64_t s = (uint64_t)blockIdx.x * (kMdBlock / kMdW) + threadIdx.x / kMdW;
    const uint32_t lane = threadIdx.x % kMdW;
    if (s < B.n_slots) {                                             // (a whole group)
        const sfgpu_hit h = B.hits[s >> 1];
        const uint32_t which = (uint32_t)(s & 1u), r = B.rec_read[s >> 1];
        const int bad = WRITE ? -1 : hit_bad_record(h, B.M, B.seq2);    // (the write pass runs only after a count pass without errors)
        bool is_line = false, plain = false;
        uint64_t n = 0;
        uint32_t nm = 0;
        if (bad >= 0) { if (lane == 0) atomicMin(&ctr[bad], (unsigned long long)(s >> 1)); }
        else if (which < vf_n_jobs(h) && r != ~0u) {
            const HitJobDev jb = hit_job_dev(B, h, which, r);
            const MdCigar c = md_slot_cigar(h, which, s, aln_pos, aln_op_off, aln_ops);
            n = md_slot_dev<WRITE>(c, jb, lane, WRITE ? md_out + woff[s] : nullptr, &nm);
            is_line = true; plain = md_plain(c, nm);
        }
        if (lane == 0) {
            if (!WRITE) bytes[s] = (uint32_t)n;
            else {
                nm_out[s] = nm; md_off_out[s] = woff[s];
                if (s + 1 == B.n_slots) md_off_out[B.n_slots] = woff[B.n_slots];
                if (is_line) atomicAdd(&s_ctr[kMdSlots], 1ull);
                if (nm) atomicAdd(&s_ctr[kMdSumNm], (unsigned long long)nm);
                if (is_line) atomicMax(&s_ctr[kMdMax], (unsigned long long)n);
                if (plain) atomicAdd(&s_ctr[kMdPlain], 1ull);
            }
        }
    }
    if (WRITE) hit_ctr_flush<kMdCounters, kMdMax>(s_ctr, ctr);
}

}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_hits_md_tags(const sfgpu_index* x, const char* d_seq1, const uint64_t* d_off1, const char* d_seq2, const uint64_t* d_off2,
                                  uint32_t n_reads, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, const int32_t* d_aln_pos,
                                  const uint64_t* d_aln_op_off, const uint32_t* d_aln_ops, uint32_t* d_nm, uint64_t* d_md_off, uint8_t* d_md,
                                  uint64_t cap_md, uint64_t* n_md, sfgpu_mdtag_stats* stats, sfgpu_stream stream) {
    SF_REQUIRE(x && n_md && stats && d_md_off, SFGPU_ERR_INVALID, "sfgpu_hits_md_tags: null pointer");
    hipStream_t st = as_stream(stream);
    HitSlotPass sp("sfgpu_hits_md_tags", x, d_seq1, d_off1, d_seq2, d_off2, n_reads, d_hits, d_hit_offsets, kMdCounters, st);
    int rc;
    if ((rc = sp.null_reads())) return rc;
    SF_REQUIRE((d_aln_pos && d_aln_op_off && d_aln_ops) || (!d_aln_pos && !d_aln_op_off && !d_aln_ops), SFGPU_ERR_INVALID,
               "sfgpu_hits_md_tags: an alignment is d_aln_pos, d_aln_op_off and d_aln_ops, or none of them");
    SF_REQUIRE(cap_md == 0 || d_md, SFGPU_ERR_INVALID, "sfgpu_hits_md_tags: null MD bytes");
    if ((rc = sp.count_records())) return rc;
    if (sp.n_rec == 0) {
        *n_md = 0; *stats = sfgpu_mdtag_stats{};
        return sp.empty(d_md_off);
    }
    SF_REQUIRE(d_hits && d_nm, SFGPU_ERR_INVALID, "sfgpu_hits_md_tags: null records");
    const uint64_t n_slots = 2 * sp.n_rec;
    // (cnt: n_slots + 1 entries, exclusive_scan_u32 reads one past the last)
    DevBuf<uint32_t> cnt; DevBuf<uint64_t> woff;
    StreamSyncOnExit sync_first{st};          // (declared after the buffers: an early return waits for the kernels before scratch goes back)
    if ((rc = cnt.reserve(n_slots + 1, st, false)) || (rc = woff.reserve(n_slots + 1, st, false)) || (rc = sp.start())) return rc;
    const dim3 grid = sp.grid(n_slots, kMdBlock / kMdW);
    hipLaunchKernelGGL(k_mdtag_walk<false>, grid, dim3(kMdBlock), 0, st, sp.B, d_aln_pos, d_aln_op_off, d_aln_ops, cnt.p, (const uint64_t*)nullptr, (uint32_t*)nullptr,
                       (uint64_t*)nullptr, (uint8_t*)nullptr, sp.ctr.p);
    SF_CHECK_LAUNCH();
    uint64_t total = 0;
    if ((rc = sp.scan(cnt.p, woff.p, &total, true))) return rc;
    *n_md = total;
    if ((rc = sp.room(total, cap_md, "MD bytes"))) return rc;
    hipLaunchKernelGGL(k_mdtag_walk<true>, grid, dim3(kMdBlock), 0, st, sp.B, d_aln_pos, d_aln_op_off, d_aln_ops, (uint32_t*)nullptr, (const uint64_t*)woff.p, d_nm, d_md_off,
                       d_md, sp.ctr.p);
    SF_CHECK_LAUNCH();
    if ((rc = sp.finish())) return rc;
    stats->slots = sp.h_ctr[kMdSlots]; stats->sum_nm = sp.h_ctr[kMdSumNm]; stats->md_bytes = total; stats->max_md_bytes = sp.h_ctr[kMdMax]; stats->slots_plain = sp.h_ctr[kMdPlain];
    return SFGPU_OK;
}
