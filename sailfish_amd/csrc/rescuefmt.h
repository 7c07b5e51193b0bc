// rescuefmt.h -- what it means to rescue an orphan's missing mate, stated once.  Plain C++, host and device, serial: rescue.hip runs
// the same functions inside its kernels, tests/rescue_harness.cpp runs them alone (rs_serial_rescue below), and
// hits.rescue_mates_host is the Python statement both are judged by.
//
// READS       a read is ELIGIBLE iff it has at least one record and every record has mate_status 1 or 2.  Every other read (no
//             records, any status 3, any status 0) keeps its records unchanged and in order.
// JOB         one orphan record h of an eligible read.  The ANCHOR is the mate the record places -- mate 1 for status 1, mate 2 for
//             status 2 -- at p = h.pos on strand f = (h.fwd != 0); its length la comes from the reads' offsets (NOT the 16-bit
//             fields).  The MISSING mate is the other one: lb bases, oriented on strand 1 - f (vf_code / vf_oriented; 4 stays 4).
// CANDIDATES  integers x with 0 <= x <= tlen - lb (the missing mate lies wholly on the transcript) and, with W = window,
//             f == 1: x >= p and x + lb <= p + W;   f == 0: x + lb <= p + la and x >= p + la - W   (inward facing, no dovetail).
//             lb == 0, lb > tlen, lb > 65 535 and la > 65 535 give no candidates.  A negative p or an anchor that hangs over the
//             transcript's end changes nothing but the clipping.
// SCORE       mism(x) = the columns j < lb where either code is 4 or the codes differ, against transcript base x + j.  A candidate
//             passes iff vf_passes(lb, mism, 0, permille); the job's PLACEMENT is the passing candidate of least mism, the lowest x
//             on a tie; none passes: no placement.
// RECORD      a placed job yields a status-3 record in the mapper's form (mate 1 in pos / fwd / read_len, mate 2 in mate_pos /
//             mate_fwd / mate_len):   status 1 -> {tid, p, x, frag, len1, len2, f, 1 - f, 3, 0}
//                                     status 2 -> {tid, x, p, frag, len1, len2, 1 - f, f, 3, 0}
//             frag = max(ends) - min(starts), as the mapper computes it for its own pairs.
// READ        at least one job of an eligible read placed: the read's records become the placed records ONLY (the mapper's own
//             rule: a read with pairs yields only its pairs), ordered by (tid, fwd) ascending and by input order on equal keys.
//             No job placed: the read keeps its orphans unchanged.
// OUTPUT      CSR over the same reads, never more records than came in; per output record one uint16 with the placed mate's mism,
//             saturated (0 for records that passed through).
// STATS       reads_eligible, records_orphan (the jobs), jobs_with_candidates, candidates (sum of the window sizes), reads_rescued,
//             records_rescued, records_dropped (orphans of rescued reads that found no mate), sum_mism (unsaturated).
// ERRORS      a record with tid >= M fails the whole call (the lowest such record is named); nothing is emitted.
//
// The kernel does not score a candidate byte by byte.  A wavefront of kRsLanes lanes takes a job; the lanes are CANDIDATES, round
// after round of kRsLanes consecutive x.  A mate of at most kRsMateMax bases is staged PACKED, 16 bases a word: two bits a base
// and, in a second word, bit 2 j set where base j is no base.  The transcript is staged the same way, a TILE of kRsTile candidates
// (kRsTile + kRsMateMax bases, one word more for the shift) at a time; a candidate at base s of the tile is then, per 16 columns,
// one funnel shift of either plane, an XOR and a popcount (rs_count_packed).  Longer mates are counted from the texts themselves,
// sixteen bases a step (rs_count_windows: vf_window / vf_classify).  Either count stops as soon as it exceeds the budget -- the
// largest mism that passes -- and after every round the budget drops to the round's best mism - 1: later candidates lie higher,
// so only a strictly smaller count can still win and the tie rule stays exact.  rs_job_serial and rs_job_lanes state both ways;
// the harness holds them against each other and against the Python statement.
#pragma once
#include "verifyfmt.h"

namespace sfgpu {

constexpr uint32_t kRsMaxWindow = 1u << 20;          // opts.window is 1 .. kRsMaxWindow
constexpr uint64_t kRsMaxLen = 65535;                // of either mate of a job
constexpr uint32_t kRsLanes = 64;                    // candidates a round
constexpr uint32_t kRsTile = 1024;                   // candidates a staged tile
constexpr uint32_t kRsMateMax = 512;                 // bases of a mate the packed form holds
constexpr uint32_t kRsMateWords = kRsMateMax / 16, kRsSegWords = (kRsTile + kRsMateMax) / 16 + 1;
constexpr uint64_t kRsNone = ~0ull;                  // no placement (else mism << 32 | x)

VF_HD bool rs_is_orphan(const sfgpu_hit& h) { return h.mate_status == 1 || h.mate_status == 2; }

// candidates lo .. hi of a job; none when hi < lo (at most `window` of them)
struct RsWindow { int64_t lo, hi; };
VF_HD uint64_t rs_n_candidates(RsWindow w) { return w.hi < w.lo ? 0ull : (uint64_t)(w.hi - w.lo) + 1ull; }
VF_HD RsWindow rs_window(int64_t p, uint64_t la, uint64_t lb, uint64_t tlen, bool f, uint32_t window) {
    if (lb == 0 || lb > tlen || lb > kRsMaxLen || la > kRsMaxLen) return RsWindow{0, -1};
    int64_t lo = f ? p : p + (int64_t)la - (int64_t)window;
    int64_t hi = (f ? p + (int64_t)window : p + (int64_t)la) - (int64_t)lb;
    const int64_t last = (int64_t)tlen - (int64_t)lb;
    if (lo < 0) lo = 0;
    if (hi > last) hi = last;
    return RsWindow{lo, hi};
}
// the largest mism with vf_passes(lb, mism, 0, permille)
VF_HD int64_t rs_budget(uint64_t lb, uint32_t permille) { return (int64_t)(((uint64_t)(1000u - permille) * lb) / 1000ull); }

// the record a placed job yields: h the orphan, x the missing mate's position, la / lb the anchor's and the missing mate's lengths
VF_HD sfgpu_hit rs_record(const sfgpu_hit& h, int64_t x, uint64_t la, uint64_t lb) {
    const int64_t p = h.pos, ea = p + (int64_t)la, eb = x + (int64_t)lb;
    const uint32_t frag = (uint32_t)((ea > eb ? ea : eb) - (p < x ? p : x));
    const uint8_t f = h.fwd != 0, g = (uint8_t)(1u - f);
    if (h.mate_status == 1) return sfgpu_hit{h.tid, h.pos, (int32_t)x, frag, (uint16_t)la, (uint16_t)lb, f, g, 3, 0};
    return sfgpu_hit{h.tid, (int32_t)x, h.pos, frag, (uint16_t)lb, (uint16_t)la, g, f, 3, 0};
}
// what a read's placed records are ordered by: (tid, the output record's fwd)
VF_HD uint64_t rs_order_key(const sfgpu_hit& h) { return 2ull * h.tid + ((h.mate_status == 1) == (h.fwd != 0) ? 1ull : 0ull); }

// ---- byte by byte ---------------------------------------------------------------------------------------------------------------
// m: the missing mate, lb bases, oriented on strand mfwd; t: the transcript.  -> mism << 32 | x of the placement, or kRsNone
VF_HD uint64_t rs_job_serial(const char* m, uint64_t lb, bool mfwd, const char* t, uint64_t tlen, RsWindow w, uint32_t permille) {
    uint64_t best = kRsNone;
    for (int64_t x = w.lo; x <= w.hi; ++x) {
        const VfCount c = vf_job_serial(m, lb, mfwd, t, tlen, x);
        if (!vf_passes(lb, c.mism, c.over, permille)) continue;
        const uint64_t key = c.mism << 32 | (uint64_t)x;
        if (key < best) best = key;
    }
    return best;
}

// ---- as the kernel counts -------------------------------------------------------------------------------------------------------
// sixteen oriented bytes -> their codes, two bits a base, and bit 2 j of `inval` where byte j is no base (a byte outside its text
// reads as 0: no base)
VF_HD void rs_pack16(VfWin w, bool fwd, uint32_t* codes, uint32_t* inval) {
    uint32_t c = 0, n = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 16; ++j) {
        const unsigned char b = (unsigned char)((j < 8 ? w.lo >> (8 * j) : w.hi >> (8 * (j - 8))) & 0xFFu);
        const uint32_t code = vf_oriented(vf_code(b), fwd);
        c |= (code & 3u) << (2 * j);
        n |= (code > 3u ? 1u : 0u) << (2 * j);
    }
    *codes = c; *inval = n;
}
// word k of the staged mate: oriented bases 16 k .. 16 k + 15
VF_HD void rs_mate_word(const char* m, uint64_t lb, bool mfwd, uint32_t k, uint32_t* codes, uint32_t* inval) {
    rs_pack16(vf_mate_window(m, (int64_t)lb, mfwd, 16 * (int64_t)k), mfwd, codes, inval);
}
// word q of the staged tile that begins at transcript base x0: bases x0 + 16 q .. + 15
VF_HD void rs_seg_word(const char* t, uint64_t tlen, int64_t x0, uint32_t q, uint32_t* codes, uint32_t* inval) {
    rs_pack16(vf_window(t, (int64_t)tlen, x0 + 16 * (int64_t)q), true, codes, inval);
}
// bits sh .. sh + 31 of hi:lo, sh = 0 .. 31
VF_HD uint32_t rs_funnel(uint32_t lo, uint32_t hi, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __funnelshift_r(lo, hi, sh);
#else
    return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
#endif
}
// mism of the candidate whose first column is base s of the staged tile (tc / ti: the tile's planes, words s / 16 .. s / 16 +
// ceil(lb / 16) are read; mc / mi: the mate's).  Stops with a count above `budget` as soon as it has one.
VF_HD uint32_t rs_count_packed(const uint32_t* tc, const uint32_t* ti, uint32_t s, const uint32_t* mc, const uint32_t* mi, uint32_t lb, int64_t budget) {
    const uint32_t w = s >> 4, sh = 2u * (s & 15u), nw = (lb + 15u) >> 4;
    uint32_t cnt = 0, c0 = tc[w], i0 = ti[w];
    for (uint32_t k = 0; k < nw; ++k) {
        const uint32_t c1 = tc[w + k + 1u], i1 = ti[w + k + 1u];
        const uint32_t x = rs_funnel(c0, c1, sh) ^ mc[k];
        uint32_t d = (x | (x >> 1) | rs_funnel(i0, i1, sh) | mi[k]) & 0x55555555u;
        if (k + 1u == nw && (lb & 15u)) d &= (1u << (2u * (lb & 15u))) - 1u;
        cnt += vf_popc(d);
        if ((int64_t)cnt > budget) return cnt;
        c0 = c1; i0 = i1;
    }
    return cnt;
}
// the same count from the texts themselves, sixteen bases a step; the candidate lies wholly on the transcript
VF_HD uint64_t rs_count_windows(const char* m, uint64_t lb, bool mfwd, const char* t, uint64_t tlen, int64_t x, int64_t budget) {
    uint64_t cnt = 0;
    for (uint64_t j0 = 0; j0 < lb; j0 += kVfStep) {
        const VfWin a = vf_mate_window(m, (int64_t)lb, mfwd, (int64_t)j0);
        const VfWin b = vf_window(t, (int64_t)tlen, x + (int64_t)j0);
        cnt += vf_classify(a, b, mfwd, (int64_t)j0, (int64_t)lb, x, (int64_t)tlen).mism;
        if ((int64_t)cnt > budget) return cnt;
    }
    return cnt;
}
// what a round makes of its lanes' keys: the least of them is the job's best so far, and only a strictly smaller count can still win
VF_HD void rs_round_done(uint64_t round_best, uint64_t* best, int64_t* budget) {
    if (round_best == kRsNone) return;
    *best = round_best; *budget = (int64_t)(round_best >> 32) - 1;
}
// a lane's key for its candidate x with count cnt under the round's budget
VF_HD uint64_t rs_lane_key(uint64_t cnt, int64_t x, int64_t budget) { return (int64_t)cnt <= budget ? cnt << 32 | (uint64_t)x : kRsNone; }

#if !defined(__HIPCC__)
// the job as a wavefront of kRsLanes lanes runs it, lane after lane
inline uint64_t rs_job_lanes(const char* m, uint64_t lb, bool mfwd, const char* t, uint64_t tlen, RsWindow w, uint32_t permille) {
    uint64_t best = kRsNone;
    int64_t budget = rs_budget(lb, permille);
    if (w.hi < w.lo) return best;
    const bool packed = lb <= kRsMateMax;
    const uint64_t tile = packed ? kRsTile : rs_n_candidates(w);
    std::vector<uint32_t> mc(kRsMateWords), mi(kRsMateWords), tc(kRsSegWords), ti(kRsSegWords);
    if (packed) for (uint32_t k = 0; k < kRsMateWords; ++k) rs_mate_word(m, lb, mfwd, k, &mc[k], &mi[k]);
    for (int64_t x0 = w.lo; x0 <= w.hi && budget >= 0; x0 += (int64_t)tile) {
        const uint64_t left = (uint64_t)(w.hi - x0) + 1ull, ncand = left < tile ? left : tile;
        if (packed) for (uint32_t q = 0; q < kRsSegWords; ++q) rs_seg_word(t, tlen, x0, q, &tc[q], &ti[q]);
        for (uint64_t c0 = 0; c0 < ncand && budget >= 0; c0 += kRsLanes) {
            uint64_t round_best = kRsNone;
            for (uint64_t c = c0; c < c0 + kRsLanes && c < ncand; ++c) {
                const int64_t x = x0 + (int64_t)c;
                const uint64_t cnt = packed ? rs_count_packed(tc.data(), ti.data(), (uint32_t)c, mc.data(), mi.data(), (uint32_t)lb, budget)
                                            : rs_count_windows(m, lb, mfwd, t, tlen, x, budget);
                const uint64_t key = rs_lane_key(cnt, x, budget);
                if (key < round_best) round_best = key;
            }
            rs_round_done(round_best, &best, &budget);
        }
    }
    return best;
}

// the whole pass, serially (lanes = false: byte by byte; true: as the kernel counts).  -> 0, or 1 + the lowest record with
// tid >= M (nothing is emitted then).  Every text is handed over in a block of exactly its length.
inline uint64_t rs_serial_rescue(const VfBatch& b, uint32_t permille, uint32_t window, bool lanes, std::vector<sfgpu_hit>* out_hits,
                                 std::vector<uint32_t>* out_off, std::vector<uint16_t>* out_mism, sfgpu_rescue_stats* stats) {
    if (const uint64_t bad = vf_bad_tid(b)) return bad;
    *stats = sfgpu_rescue_stats{};
    out_hits->clear(); out_mism->clear(); out_off->assign(1, 0u);
    for (uint32_t r = 0; r < b.n_reads; ++r) {
        const uint32_t lo = b.hit_off[r], hi = b.hit_off[r + 1];
        bool eligible = hi > lo;
        for (uint32_t i = lo; i < hi; ++i) eligible = eligible && rs_is_orphan(b.hits[i]);
        std::vector<sfgpu_hit> placed; std::vector<uint64_t> mism;
        if (eligible) {
            ++stats->reads_eligible;
            stats->records_orphan += hi - lo;
            for (uint32_t i = lo; i < hi; ++i) {
                const sfgpu_hit& h = b.hits[i];
                const bool second = h.mate_status == 2, f = h.fwd != 0;              // the anchor is mate 2; the missing one mate 1
                const uint64_t len1 = b.off1[r + 1] - b.off1[r], len2 = b.off2[r + 1] - b.off2[r];
                const uint64_t la = second ? len2 : len1, lb = second ? len1 : len2;
                const char* mp = second ? b.seq1 + b.off1[r] : b.seq2 + b.off2[r];
                const std::vector<char> mate(mp, mp + lb), tx(b.tseq + b.tseq_off[h.tid], b.tseq + b.tseq_off[h.tid] + b.tlen[h.tid]);
                const RsWindow w = rs_window(h.pos, la, lb, tx.size(), f, window);
                stats->jobs_with_candidates += w.hi >= w.lo;
                stats->candidates += rs_n_candidates(w);
                const uint64_t key = lanes ? rs_job_lanes(mate.data(), lb, !f, tx.data(), tx.size(), w, permille)
                                           : rs_job_serial(mate.data(), lb, !f, tx.data(), tx.size(), w, permille);
                if (key == kRsNone) continue;
                placed.push_back(rs_record(h, (int64_t)(key & 0xFFFFFFFFull), la, lb));
                mism.push_back(key >> 32);
            }
        }
        if (placed.empty()) {
            for (uint32_t i = lo; i < hi; ++i) { out_hits->push_back(b.hits[i]); out_mism->push_back(0); }
        } else {
            ++stats->reads_rescued;
            stats->records_rescued += placed.size();
            stats->records_dropped += (hi - lo) - placed.size();
            const size_t base = out_hits->size(), n = placed.size();
            out_hits->resize(base + n); out_mism->resize(base + n);
            for (size_t i = 0; i < n; ++i) {                                         // rank by counting within the read
                size_t rank = 0;
                const uint64_t ki = 2ull * placed[i].tid + placed[i].fwd;
                for (size_t j = 0; j < n; ++j) {
                    const uint64_t kj = 2ull * placed[j].tid + placed[j].fwd;
                    rank += kj < ki || (kj == ki && j < i);
                }
                (*out_hits)[base + rank] = placed[i]; (*out_mism)[base + rank] = vf_sat16(mism[i]);
                stats->sum_mism += mism[i];
            }
        }
        out_off->push_back((uint32_t)out_hits->size());
    }
    return 0;
}
#endif

}  // namespace sfgpu
