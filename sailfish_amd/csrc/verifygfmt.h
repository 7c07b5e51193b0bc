// verifygfmt.h -- gapped hit verification: a job's banded edit distance, stated once.  Plain C++, host and device.  Jobs, base codes,
// orientation and the record -> jobs mapping are verifyfmt.h's (vf_job, vf_code, vf_oriented); hitgroup.h runs the lane functions
// below inside the kernels of verify.hip and align_gapped.hip (hit_band_dev), tests/verifyg_harness.cpp runs them alone (vg_serial_verify), and hits.gapped_edits_host /
// hits.verify_hits_gapped_host are the Python statement both are judged by.
//
// A job of len oriented bases a[0 .. len) at recorded position pos on a transcript of tlen bases, band k = max_indel (1 .. 15):
// COLUMN   b(x) = vf_code(t[x]) for 0 <= x < tlen, else OFF.
// COST     sub(i, x) = 0 iff a[i] <= 3 and b(x) == a[i], else 1: N matches nothing, OFF matches nothing.
// CELLS    D[i][d], rows i = -1 .. len - 1, diagonals d = -k .. k; cell (i, d) aligns read base i to x = pos + i + d.
// START    D[-1][d] = 0 for every d: the start diagonal is free (the mapper's seed may lie behind an indel).
// ROW      V[d] = min(D[i-1][d] + sub(i, pos + i + d), D[i-1][d+1] + 1) (the second term for d < k: read base i unaligned), then
//          D[i][d] = min over d' <= d of V[d'] + (d - d') (transcript bases skipped at 1 each).
// EDITS    min over d of D[len-1][d]; 0 for len == 0.  With k = 0 this is mism + over of the ungapped pass; for any k it is <= that.
// PASS     a job passes iff 1000 * (len - edits) >= permille * len (64-bit integers), i.e. edits <= vg_max_edits; a record passes iff
//          all its jobs pass.
// BEST     keep_best: of a read's passing records those of least cost -- edits summed over the record's jobs, unsaturated.
// SCORE    per survivor {edits, ungapped, mate_edits, mate_ungapped}, 16 bits each, saturating at 65 535; ungapped = mism + over on the
//          recorded diagonal; the mate fields are 0 unless the status is 3.
// STATS    verifyfmt.h's with sum_edits for sum_mism, plus `rescued`: the survivors with a job that fails vf_passes(len, mism, over).
// ORDER / ERRORS  as verifyfmt.h.
//
// Lanes are DIAGONALS: lane l of a group of `width` (16 for k <= 7, 32 for k <= 15) holds d = l - k; the lanes above 2 k hold
// kVgInf, so the lane above the band's top supplies the missing second term by itself.  A row is: the upper neighbour's D (one
// exchange), vg_lane_v, then an inclusive prefix minimum of V + (width - l) over the lanes (log2 width exchanges of vg_scan_step).
// Every kVfStep rows a lane refills its transcript window on its own diagonal and the mate's window, classifies the sixteen pairs at
// once (vg_submask) and the group takes the band's minimum: row minima never fall, so a job whose minimum exceeds vg_max_edits has
// failed (kVgFail) and stops.  vg_band_group runs these functions for all lanes of a group in lockstep on the host -- the ONE host
// statement of the band's row, for this pass and, with `cells`, for aligngfmt.h's forward pass.  The cells are 32 bits: mates shorter
// than kVgInf bases.
#pragma once
#include "verifyfmt.h"

namespace sfgpu {

constexpr uint32_t kVgMaxIndel = 15;
constexpr uint32_t kVgMaxWidth = 32;
constexpr uint32_t kVgInf = 0x3FFFFFFFu;          // a cell outside the band
constexpr uint64_t kVgFail = ~0ull;               // a job known to fail: its edits are not computed to the end

VF_HD uint32_t vg_width(uint32_t k) { return k <= 7u ? 16u : 32u; }
VF_HD uint64_t vg_max_edits(uint64_t len, uint32_t permille) { return (uint64_t)(1000u - permille) * len / 1000ull; }   // the most edits that pass
VF_HD bool vg_passes(uint64_t len, uint64_t edits, uint32_t permille) { return 1000ull * (len - edits) >= (uint64_t)permille * len; }

// ---- the recurrence in plain loops ----------------------------------------------------------------------------------------------
VF_HD uint64_t vg_job_serial(const char* r, uint64_t len, bool fwd, const char* t, uint64_t tlen, int64_t pos, uint32_t k) {
    uint64_t D[2 * kVgMaxIndel + 1], V[2 * kVgMaxIndel + 1];
    const uint32_t n = 2u * k + 1u;
    if (len == 0) return 0;
    for (uint32_t l = 0; l < n; ++l) D[l] = 0;
    for (uint64_t i = 0; i < len; ++i) {
        const uint32_t a = vf_oriented(vf_code((unsigned char)(fwd ? r[i] : r[len - 1 - i])), fwd);
        for (uint32_t l = 0; l < n; ++l) {
            const int64_t x = pos + (int64_t)i + (int64_t)l - (int64_t)k;
            const bool on = x >= 0 && x < (int64_t)tlen;
            const uint64_t sub = (on && a <= 3u && vf_code((unsigned char)t[x]) == a) ? 0u : 1u;
            uint64_t v = D[l] + sub;
            if (l + 1u < n && D[l + 1u] + 1u < v) v = D[l + 1u] + 1u;
            V[l] = v;
        }
        for (uint32_t l = 0; l < n; ++l) D[l] = (l > 0 && D[l - 1u] + 1u < V[l]) ? D[l - 1u] + 1u : V[l];
    }
    uint64_t e = D[0];
    for (uint32_t l = 1; l < n; ++l) e = D[l] < e ? D[l] : e;
    return e;
}

// ---- what a lane does -----------------------------------------------------------------------------------------------------------
// 0x80 in bytes 0 .. 3 -> bits 0 .. 3
VF_HD uint32_t vg_gather4(uint32_t m) { return (((m >> 7) * 0x01020408u) >> 24) & 0xFu; }
// bit j: oriented mate base j of the window does NOT match the transcript byte under it (vf_differ4: N, a byte off the transcript,
// which vf_window reads as 0, and unequal bases all differ)
VF_HD uint32_t vg_submask(VfWin m, VfWin t, bool fwd) {
    const uint32_t cx = fwd ? 0u : 0x15151515u, cm = fwd ? 0u : 0x11u;
    return vg_gather4(vf_differ4((uint32_t)m.lo, (uint32_t)t.lo, cx, cm)) | vg_gather4(vf_differ4((uint32_t)(m.lo >> 32), (uint32_t)(t.lo >> 32), cx, cm)) << 4 |
           vg_gather4(vf_differ4((uint32_t)m.hi, (uint32_t)t.hi, cx, cm)) << 8 | vg_gather4(vf_differ4((uint32_t)(m.hi >> 32), (uint32_t)(t.hi >> 32), cx, cm)) << 12;
}
// the sixteen rows from i0 on the diagonal of lane `lane`
VF_HD uint32_t vg_lane_submask(VfWin mate, const char* t, uint64_t tlen, int64_t pos, uint64_t i0, uint32_t lane, uint32_t k, bool fwd) {
    return vg_submask(mate, vf_window(t, (int64_t)tlen, pos + (int64_t)i0 + (int64_t)lane - (int64_t)k), fwd);
}
VF_HD uint32_t vg_lane_start(uint32_t lane, uint32_t k) { return lane <= 2u * k ? 0u : kVgInf; }
// V of a row: d = this lane's D[i-1], up = the next lane's (the last lane of a group is never in the band and is handed its own)
VF_HD uint32_t vg_lane_v(uint32_t d, uint32_t up, uint32_t sub) { const uint32_t a = d + sub, b = up + 1u; return a < b ? a : b; }
VF_HD uint32_t vg_key(uint32_t v, uint32_t lane, uint32_t width) { return v + (width - lane); }
// one step of the inclusive prefix minimum: `below` is the key of lane - o (any value where lane < o)
VF_HD uint32_t vg_scan_step(uint32_t key, uint32_t below, uint32_t lane, uint32_t o) { return (lane >= o && below < key) ? below : key; }
VF_HD uint32_t vg_lane_d(uint32_t key, uint32_t lane, uint32_t width, uint32_t k) { return lane <= 2u * k ? key - (width - lane) : kVgInf; }

// aligngfmt.h's view of a row (its CANDIDATES and END), here because the one band function below stores it: the 4 bits of this
// lane's cell -- d_prev = its D[i-1], up = the next lane's D[i-1], d_new = its D[i], below = the lane before's D[i]
constexpr uint32_t kAgDiag = 1u, kAgIns = 2u, kAgDel = 4u;                  // candidate bits of a cell; bit 3 is sub on its diagonal
constexpr uint32_t kAgNoEnd = 0xFFFFu;
VF_HD uint32_t ag_lane_cand(uint32_t d_prev, uint32_t up, uint32_t sub, uint32_t d_new, uint32_t below, uint32_t lane, uint32_t k) {
    if (lane > 2u * k) return 0u;
    return (d_prev + sub == d_new ? kAgDiag : 0u) | ((lane < 2u * k && up + 1u == d_new) ? kAgIns : 0u) |
           ((lane > 0u && below + 1u == d_new) ? kAgDel : 0u) | sub << 3;
}
// END: the least rank over the lanes names the end diagonal
VF_HD uint32_t ag_end_rank(uint32_t d_last, uint32_t edits, uint32_t lane, uint32_t k) {
    if (lane > 2u * k || d_last != edits) return kAgNoEnd;
    return lane >= k ? 2u * (lane - k) + (lane > k ? 1u : 0u) : 2u * (k - lane);
}
VF_HD uint32_t ag_rank_lane(uint32_t rank, uint32_t k) { return (rank & 1u) ? k + (rank >> 1) : k - (rank >> 1); }

// a group of `width` lanes in lockstep on the host: the forward pass of one job.  cells == nullptr -> the job's edits, or kVgFail
// once they are known to exceed max_edits.  With cells (width words a step of kVfStep rows) every row's candidate bits are stored,
// the pass never stops early, and *lane_end is the END lane.
VF_HD uint64_t vg_band_group(const char* r, uint64_t len, bool fwd, const char* t, uint64_t tlen, int64_t pos, uint32_t k, uint32_t width, uint64_t max_edits,
                             uint64_t* cells, uint32_t* lane_end) {
    uint32_t D[kVgMaxWidth], key[kVgMaxWidth], nxt[kVgMaxWidth], mask[kVgMaxWidth];
    uint64_t word[kVgMaxWidth];
    for (uint32_t l = 0; l < width; ++l) D[l] = vg_lane_start(l, k);
    uint32_t m = 0;
    for (uint64_t i0 = 0; i0 < len; i0 += kVfStep) {
        const VfWin mate = vf_mate_window(r, (int64_t)len, fwd, (int64_t)i0);
        for (uint32_t l = 0; l < width; ++l) { mask[l] = vg_lane_submask(mate, t, tlen, pos, i0, l, k, fwd); word[l] = 0; }
        const uint32_t n = len - i0 < kVfStep ? (uint32_t)(len - i0) : kVfStep;
        for (uint32_t j = 0; j < n; ++j) {
            for (uint32_t l = 0; l < width; ++l) key[l] = vg_key(vg_lane_v(D[l], D[l + 1u < width ? l + 1u : l], (mask[l] >> j) & 1u), l, width);
            for (uint32_t o = 1; o < width; o <<= 1) {
                for (uint32_t l = 0; l < width; ++l) nxt[l] = vg_scan_step(key[l], key[l >= o ? l - o : l], l, o);
                for (uint32_t l = 0; l < width; ++l) key[l] = nxt[l];
            }
            for (uint32_t l = 0; l < width; ++l) nxt[l] = vg_lane_d(key[l], l, width, k);
            for (uint32_t l = 0; cells && l < width; ++l)
                word[l] |= (uint64_t)ag_lane_cand(D[l], D[l + 1u < width ? l + 1u : l], (mask[l] >> j) & 1u, nxt[l], nxt[l > 0 ? l - 1u : l], l, k) << (4u * j);
            for (uint32_t l = 0; l < width; ++l) D[l] = nxt[l];
        }
        for (uint32_t l = 0; cells && l < width; ++l) cells[(i0 / kVfStep) * width + l] = word[l];
        m = D[0];
        for (uint32_t l = 1; l < width; ++l) m = D[l] < m ? D[l] : m;
        if (!cells && m > max_edits) return kVgFail;
    }
    if (cells) {
        uint32_t rank = kAgNoEnd;
        for (uint32_t l = 0; l < width; ++l) { const uint32_t q = ag_end_rank(D[l], m, l, k); rank = q < rank ? q : rank; }
        *lane_end = ag_rank_lane(rank, k);
    }
    return m;
}

// ---- a record -------------------------------------------------------------------------------------------------------------------
struct VgJob { uint64_t edits, ungapped; bool ungapped_pass; };                  // edits: kVgFail allowed where the job fails
struct VgRecord { sfgpu_hit_gscore score; uint64_t cost; bool pass, rescued; };   // cost and score: of a passing record only
VF_HD VgRecord vg_record(const sfgpu_hit& h, const VgJob* job /* [vf_n_jobs] */, const uint64_t* len /* [vf_n_jobs] */, uint32_t permille) {
    VgRecord out;
    const uint32_t nj = vf_n_jobs(h);
    out.pass = true; out.rescued = false; out.cost = 0;
    for (uint32_t j = 0; j < nj; ++j) {
        out.pass = out.pass && job[j].edits != kVgFail && vg_passes(len[j], job[j].edits, permille);
        if (!out.pass) break;
        out.cost += job[j].edits;
        out.rescued = out.rescued || !job[j].ungapped_pass;
    }
    if (!out.pass) { out.rescued = false; out.cost = 0; out.score = sfgpu_hit_gscore{0, 0, 0, 0}; return out; }
    out.score.edits = vf_sat16(job[0].edits); out.score.ungapped = vf_sat16(job[0].ungapped);
    out.score.mate_edits = nj > 1 ? vf_sat16(job[1].edits) : (uint16_t)0; out.score.mate_ungapped = nj > 1 ? vf_sat16(job[1].ungapped) : (uint16_t)0;
    return out;
}

#if !defined(__HIPCC__)
// the whole pass, serially (lanes = false: vg_job_serial; true: as a group of vg_width(k) lanes runs it, with its early stop).
// -> 0, or 1 + the lowest record with tid >= M (nothing is emitted then)
inline uint64_t vg_serial_verify(const char* tseq, const uint64_t* tseq_off, const uint32_t* tlen, uint64_t M, const char* seq1, const uint64_t* off1,
                                 const char* seq2, const uint64_t* off2, uint32_t n_reads, const sfgpu_hit* hits, const uint32_t* hit_off,
                                 uint32_t permille, bool keep_best, uint32_t k, bool lanes, std::vector<sfgpu_hit>* out_hits,
                                 std::vector<uint32_t>* out_off, std::vector<sfgpu_hit_gscore>* out_scores, sfgpu_verify_gstats* stats) {
    const VfBatch b{tseq, tseq_off, tlen, M, seq1, off1, seq2, off2, n_reads, hits, hit_off};
    if (const uint64_t bad = vf_bad_tid(b)) return bad;
    std::vector<VgRecord> rec(b.n_rec());
    VgJob job[2]; uint64_t len[2];
    vf_each_job(b, [&](uint32_t, uint32_t i, uint32_t j, const char* mate, uint64_t n, const char* tx, uint64_t tl, bool fwd, int64_t pos) {
        if (j == 0) { job[0] = job[1] = VgJob{0, 0, true}; len[0] = len[1] = 0; }
        len[j] = n;
        const VfCount c = lanes ? vf_job_windows(mate, n, fwd, tx, tl, pos, 16) : vf_job_serial(mate, n, fwd, tx, tl, pos);
        job[j].ungapped = c.mism + c.over;
        job[j].ungapped_pass = vf_passes(n, c.mism, c.over, permille);
        job[j].edits = lanes ? vg_band_group(mate, n, fwd, tx, tl, pos, k, vg_width(k), vg_max_edits(n, permille), nullptr, nullptr)
                             : vg_job_serial(mate, n, fwd, tx, tl, pos, k);
        if (j + 1u == vf_n_jobs(b.hits[i])) rec[i] = vg_record(b.hits[i], job, len, permille);
    });
    vf_select(b, rec, keep_best, out_hits, out_off, out_scores, stats,
              [](const VgRecord& v, sfgpu_verify_gstats* st) { st->sum_edits += v.cost; st->rescued += v.rescued; });
    return 0;
}
#endif

}  // namespace sfgpu
