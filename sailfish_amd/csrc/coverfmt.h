// coverfmt.h -- posterior-weighted coverage of the transcripts by the mappings, and the bedGraph rows and summary columns written of
// it, stated once.  Plain C++, host and device: coverage.hip runs the functions below inside its kernels, tests/coverage_harness.cpp
// runs them alone (cov_serial), and hits.coverage_host is the Python statement both are judged by.
//
// SLOTS    transcript t of length len_t owns len_t + 1 slots of ONE uint64 array; its base is off_t + t (off_t the bases before it),
//          the array has sum(len) + M slots, and all arithmetic is modulo 2^64.
// LINES    the writer's (samwfmt.h): line 0 of a record is (pos, read_len); a mate_status == 3 record has line 1, (mate_pos, mate_len).
// INTERVAL without an alignment the one interval [max(pos, 0), min(pos + len, len_t)).  With the alignment slot 2 h + which
//          (sfgpu_hits_align_gapped's pos / op_off / ops) the words are walked from pos[slot]: M, = and X cover [x, x + n) clipped to
//          [0, len_t) and advance x; D and N advance x; I, S, H and P do neither.  A slot without operations has no interval.  An
//          empty interval adds nothing and is counted.  Overlapping mates count twice.
// WEIGHT   q = trunc(p 2^32) as uint64 for 0 <= p <= 1 (a scaling by a power of two: exact); both lines of a pair carry the record's
//          q.  Without posteriors q = floor(2^32 / n), n the read's record count.
// ADD      slot[base + a] += q, slot[base + b] -= q for an interval [a, b).
// FINISH   one inclusive scan over the whole array turns it into sums; a transcript's last slot then reads 0 (`residue` counts the
//          ones that do not), which is why the scan need not be segmented.
// DEPTH    (double)sum 2^-32: the conversion rounds to nearest even, the scaling is exact.
// RUNS     maximal stretches of one transcript's bases with the same sum; those of sum 0 are dropped; by transcript, then start.
// ROW      name \t start \t end \t %g(depth) \n, 0-based, half open.
// SUMMARY  covered = bases with sum > 0; S = the sum of sum over the bases, in 128 bits; max = the largest sum.
//          CoveredFraction = (double)covered / (double)len, MeanDepth = (double)floor(S / len) 2^-32, MaxDepth = (double)max 2^-32;
//          all 0 for len == 0.
// Every step is integer arithmetic: any order of the adds and any reduction tree give the same bits.
#pragma once
#include <cstdint>

#include "../../include/sfgpu.h"
#include "decfmt.h"
#include "gfmt.h"

#if defined(__HIPCC__)
#define COV_HD __host__ __device__ __forceinline__
#else
#define COV_HD inline
#include <string>
#include <vector>
#endif

namespace sfgpu {

constexpr uint64_t kCovOne = 1ull << 32;                   // the weight of p = 1
constexpr uint64_t kCovMaxLines = 0xffffffffull;           // a handle's lines stay below 2^32: (2^32 - 1) 2^32 < 2^64, no depth wraps
constexpr uint32_t kCovRowTail = 4 + 10 + 10 + kGfmtMaxLen; // the separators, start, end and the token of a row: 37 bytes

COV_HD uint32_t cov_record_lines(const sfgpu_hit& h) { return h.mate_status == 3 ? 2u : 1u; }
COV_HD int64_t cov_line_pos(const sfgpu_hit& h, uint32_t which) { return which ? h.mate_pos : h.pos; }
COV_HD uint32_t cov_line_len(const sfgpu_hit& h, uint32_t which) { return which ? h.mate_len : h.read_len; }

COV_HD bool cov_p_bad(double p) { return !(p >= 0.0 && p <= 1.0); }
COV_HD uint64_t cov_weight(double p) { return (uint64_t)(p * 4294967296.0); }
COV_HD uint64_t cov_weight_uniform(uint64_t n) { return kCovOne / n; }

// [a, b) clipped to [0, len_t) -> whether anything is left
COV_HD bool cov_clip(int64_t a, int64_t b, uint64_t len_t, uint64_t* lo, uint64_t* hi) {
    if (a < 0) a = 0;
    if (b > (int64_t)len_t) b = (int64_t)len_t;
    if (a >= b) return false;
    *lo = (uint64_t)a; *hi = (uint64_t)b;
    return true;
}

struct CovCount { uint64_t intervals, empty, bases; };     // of one line: intervals added, empty ones, the bases of the added

// the intervals of one line: add(lo, hi) for every one that is not empty.  aligned == false: the recorded diagonal (pos, len); else
// the n_ops words from aln_pos
template <typename Add>
COV_HD CovCount cov_line(int64_t pos, uint32_t len, uint64_t len_t, bool aligned, const uint32_t* ops, uint64_t n_ops, int64_t aln_pos, Add add) {
    CovCount c = {0, 0, 0};
    uint64_t lo, hi;
    if (!aligned) {
        if (cov_clip(pos, pos + (int64_t)len, len_t, &lo, &hi)) { add(lo, hi); c.intervals++; c.bases += hi - lo; }
        else c.empty++;
        return c;
    }
    int64_t x = aln_pos;
    for (uint64_t i = 0; i < n_ops; ++i) {
        const uint32_t n = ops[i] >> 4, op = ops[i] & 15u;
        if (op == 0u || op == 7u || op == 8u) {            // M = X
            if (cov_clip(x, x + (int64_t)n, len_t, &lo, &hi)) { add(lo, hi); c.intervals++; c.bases += hi - lo; }
            else c.empty++;
            x += n;
        } else if (op == 2u || op == 3u) {                 // D N
            x += n;
        }
    }
    return c;
}

COV_HD double cov_depth(uint64_t sum) { return (double)sum * (1.0 / 4294967296.0); }

// floor((hi 2^64 + lo) / d) for d > 0 and hi < d (the quotient fits 64 bits): long division by 32-bit limbs
COV_HD uint64_t cov_div128(uint64_t hi, uint64_t lo, uint32_t d) {
    uint64_t rem = hi % d, q = 0;
    const uint32_t limb[2] = {(uint32_t)(lo >> 32), (uint32_t)lo};
    for (int i = 0; i < 2; ++i) {
        const uint64_t cur = rem << 32 | limb[i];
        q = q << 32 | cur / d;
        rem = cur % d;
    }
    return q;
}

// the three columns of a transcript
COV_HD void cov_summary(uint32_t len, uint64_t covered, uint64_t s_hi, uint64_t s_lo, uint64_t max, double* frac, double* mean, double* maxd) {
    if (len == 0) { *frac = *mean = *maxd = 0.0; return; }
    *frac = (double)covered / (double)len;
    *mean = cov_depth(cov_div128(s_hi, s_lo, len));
    *maxd = cov_depth(max);
}

// the bytes of a run's row behind its name
COV_HD uint32_t cov_row_tail_len(uint32_t start, uint32_t end, uint32_t rec) {
    return 4u + (uint32_t)dec_len_u32(start) + (uint32_t)dec_len_u32(end) + (uint32_t)gfmt_len(rec);
}
// ... written through put(i, ch), i counted from the first byte behind the name
template <typename Put>
COV_HD void cov_row_tail(uint32_t start, uint32_t end, uint32_t rec, Put put) {
    int p = 0;
    put(p++, '\t');
    int nd = dec_len_u32(start);
    dec_put_fixed_u32(start, nd, 0, [&](int i, char ch) { put(p + nd - 1 - i, ch); });
    p += nd;
    put(p++, '\t');
    nd = dec_len_u32(end);
    dec_put_fixed_u32(end, nd, 0, [&](int i, char ch) { put(p + nd - 1 - i, ch); });
    p += nd;
    put(p++, '\t');
    nd = gfmt_len(rec);
    gfmt_put(rec, [&](int i, char ch) { put(p + nd - 1 - i, ch); });
    p += nd;
    put(p, '\n');
}

#if !defined(__HIPCC__)
// The whole of it, serially (host only): the state a handle keeps, add() per batch, finish() once.
struct CovSerial {
    std::vector<uint32_t> len;
    std::vector<uint64_t> base, slot;                      // base[M + 1]
    sfgpu_cov_stats stats{};
    bool finished = false;
    std::vector<uint32_t> r_tid, r_start, r_end;           // the runs
    std::vector<uint64_t> r_sum;
    std::vector<double> frac, mean, maxd;                  // the summary
    uint64_t covered = 0, residue = 0;

    CovSerial(const uint32_t* ref_len, uint64_t M) : len(ref_len, ref_len + M), base(M + 1, 0) {
        for (uint64_t t = 0; t < M; ++t) base[t + 1] = base[t] + len[t] + 1ull;
        slot.assign(base[M], 0);
    }
    // -> 0; -(1 + the lowest record whose tid is no transcript); 1 + the lowest record whose p is refused; INT64_MIN: too many lines;
    // INT64_MIN + 1: after finish.  On an error nothing is added.
    int64_t add(const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t n_reads, const double* p, const int32_t* aln_pos, const uint64_t* aln_op_off,
                const uint32_t* aln_ops) {
        if (finished) return INT64_MIN + 1;
        const uint64_t n_rec = n_reads ? hit_off[n_reads] : 0, M = len.size();
        uint64_t lines = 0;
        for (uint64_t h = 0; h < n_rec; ++h) { if (hits[h].tid >= M) return -(int64_t)(1 + h); lines += cov_record_lines(hits[h]); }
        for (uint64_t h = 0; p && h < n_rec; ++h) if (cov_p_bad(p[h])) return (int64_t)(1 + h);
        if (stats.lines + lines > kCovMaxLines) return INT64_MIN;
        stats.reads += n_reads; stats.records += n_rec; stats.lines += lines;
        for (uint64_t r = 0; r < n_reads; ++r) {
            const uint64_t b = hit_off[r], e = hit_off[r + 1];
            for (uint64_t h = b; h < e; ++h) {
                const uint64_t q = p ? cov_weight(p[h]) : cov_weight_uniform(e - b), at = base[hits[h].tid];
                for (uint32_t w = 0; w < cov_record_lines(hits[h]); ++w) {
                    const uint64_t s = 2 * h + w;
                    const CovCount c = cov_line(cov_line_pos(hits[h], w), cov_line_len(hits[h], w), len[hits[h].tid], aln_pos != nullptr,
                                                aln_pos ? aln_ops + aln_op_off[s] : nullptr, aln_pos ? aln_op_off[s + 1] - aln_op_off[s] : 0, aln_pos ? aln_pos[s] : 0,
                                                [&](uint64_t lo, uint64_t hi) { slot[at + lo] += q; slot[at + hi] -= q; });
                    stats.intervals += c.intervals; stats.empty_intervals += c.empty; stats.bases_added += c.bases;
                }
            }
        }
        return 0;
    }
    void finish() {
        if (finished) return;
        finished = true;
        uint64_t acc = 0;
        for (auto& v : slot) { acc += v; v = acc; }
        const uint64_t M = len.size();
        frac.assign(M, 0.0); mean.assign(M, 0.0); maxd.assign(M, 0.0);
        for (uint64_t t = 0; t < M; ++t) {
            const uint64_t* s = slot.data() + base[t];
            uint64_t cov = 0, hi = 0, lo = 0, mx = 0;
            for (uint32_t i = 0; i < len[t]; ++i) {
                if (s[i]) {
                    if (i == 0 || s[i] != s[i - 1]) { r_tid.push_back((uint32_t)t); r_start.push_back(i); r_end.push_back(i + 1); r_sum.push_back(s[i]); }
                    else r_end.back() = i + 1;
                    ++cov;
                }
                lo += s[i]; hi += lo < s[i];
                if (s[i] > mx) mx = s[i];
            }
            if (s[len[t]]) ++residue;
            covered += cov;
            cov_summary(len[t], cov, hi, lo, mx, &frac[t], &mean[t], &maxd[t]);
        }
    }
    // the file: names[name_off[t] .. name_off[t + 1]) is transcript t's
    std::string text(const char* names, const uint64_t* name_off) const {
        std::string out;
        for (size_t r = 0; r < r_tid.size(); ++r) {
            out.append(names + name_off[r_tid[r]], names + name_off[r_tid[r] + 1]);
            bool slow;
            const uint32_t rec = gfmt_decode(cov_depth(r_sum[r]), &slow);
            const size_t at = out.size();
            out.resize(at + cov_row_tail_len(r_start[r], r_end[r], rec));
            cov_row_tail(r_start[r], r_end[r], rec, [&](int i, char ch) { out[at + (size_t)i] = ch; });
        }
        return out;
    }
};
#endif

}  // namespace sfgpu
