// galnfmt.h -- a batch of hit records and their alignment slots rewritten from transcript into GENOME terms through the exon blocks,
// stated once.  Plain C++, host and device: genomealn.hip runs the functions below inside its kernels, tests/galn_harness.cpp runs
// them alone (GalnSerial), and hits.project_alignments_host is the Python statement both are judged by.  The writers (samwfmt.h,
// bamwfmt.h, baifmt.h) are handed the result as they are handed any batch: RNAME from tid over the chromosomes' names, POS and CIGAR
// from the alignment slots, N counted in the reference span.
//
// MODEL    covgfmt.h's: a status per transcript (0 = placed), a chromosome id, a strand, exon blocks (gs_i, len_i) in TRANSCRIPT order
//          with toff_i = sum of len_j for j < i, L = sum of len_i; covg_block_ok is the rule a model is refused by.  A placed transcript
//          without a block has no place either: it counts as not placed.
// LINES    record h has line 0, and line 1 iff mate_status == 3; line `which` lies in slot 2 h + which.  A line's transcript CIGAR is
//          the one the writer would write: the slot's words (len << 4 | op, MIDNSHP=X) at x0 = aln_pos[slot] where an alignment is
//          given, else samw_aligned's <clip>S<match>M at x0 = max(pos, 0) from pos / read_len (mate_pos / mate_len on line 1), and no
//          word at all where no base lies on the transcript.
// KEEP     a record is kept iff its transcript is placed (else records_unplaced), every line has a reference column -- an M = X D N
//          word of length > 0; a line without a word has none -- (else records_unalignable), and every line is in range (else
//          records_off_range): x0 >= 0, its projected interval [lo, hi) has 0 <= lo and hi <= 2^31 - 1 (hit.pos, aln_pos and BAM's
//          pos are int32), and no N it needs is 2^28 bases or longer (an operation's length has 28 bits).  The first failing test
//          counts; a pair stands or falls as a whole.
// COLUMNS  the words are walked from x = x0.  Reference column x < L lies in the block b with toff_b <= x < toff_b + len_b, at
//          g(x) = gs_b + (x - toff_b) on +, gs_b + len_b - 1 - (x - toff_b) on -.  A column at x >= L continues the LAST block past
//          its end by the same formula (columns_beyond_model; on - it can fall below 0, which is off_range).  No column is added,
//          removed or retyped: nm is unchanged, and the MD changes only by orientation.
// SPLICE   between block i and i + 1 lies the gap (gs_{i+1} - gs_i - len_i on +, gs_i - gs_{i+1} - len_{i+1} on -); the boundary is
//          a junction iff the gap is > 0.  An M = X D N word whose columns lie on both sides of a junction is cut there and <gap>N is
//          put between the pieces.  The N is put in front of the first reference column beyond the junction, not behind the last one
//          before it: a word that ends exactly at a block's end is not cut and the N follows only if a reference column follows, and
//          I / S / H / P words that sit on the junction stay upstream of the N.  Touching blocks cut nothing.  Words of length 0 and
//          words that are not M = X D N are copied.
// ORIENT   on a - transcript the words are written in reverse order (leading and trailing S swap), fwd and mate_fwd are inverted,
//          and the line's interval is [g(last column), g(first column) + 1); on + it is [g(first), g(last) + 1).  POS - 1 = lo.
// RECORD   tid = the chromosome id; pos = line 0's lo; of a pair mate_pos = line 1's lo and frag_len = max(hi_0, hi_1) - min(lo_0,
//          lo_1) (N included); every other field, mate_pos and frag_len of a record that is no pair among them, unchanged.  Kept
//          records keep their order inside the read, a read with none left becomes a read without records (the writer's 77 / 141 / 4
//          lines), and src_record[new] names the old record: per-record values (ZW) are gathered, never recomputed.  The slot of a
//          line that does not exist has position 0, nm 0, no word and no MD byte.
// MD       on + the bytes are copied.  On - the tokens num (letter | ^letters) num ... are written in reverse order: a number as it
//          is, a letter complemented (A<->T, C<->G, every other byte as it is), a deletion as ^ and its letters reversed and
//          complemented: 5^AC0T3 becomes 3A0^GT5.  The length is unchanged.
// Everything is integers and bytes: any layout of the work gives the same arrays.
#pragma once
#include <cstdint>

#include "../../include/sfgpu.h"
#include "covgfmt.h"
#include "samwfmt.h"

#if !defined(__HIPCC__)
#include <string>
#include <vector>
#endif

namespace sfgpu {

constexpr int64_t kGalnMaxEnd = 0x7fffffffll;              // hi <= 2^31 - 1
constexpr uint64_t kGalnMaxOpLen = 1ull << 28;             // an operation is shorter
enum { GALN_KEPT = 0, GALN_UNPLACED = 1, GALN_UNALIGNABLE = 2, GALN_OFF_RANGE = 3 };
// the counters, in the order of hits.GENOME_ALN_STATS and of sfgpu_galn_stats
enum { kGaRecordsIn = 0, kGaRecordsOut, kGaUnplaced, kGaUnalignable, kGaOffRange, kGaReadsEmptied, kGaLines, kGaLinesSpliced, kGaNOps, kGaLinesReversed,
       kGaBeyond, kGaWordsIn, kGaWordsOut, kGaCounters };

COV_HD bool galn_ref_op(uint32_t op) { return op == 0u || op == 2u || op == 3u || op == 7u || op == 8u; }      // M D N = X

// a line's transcript CIGAR: n words at ops, or (ops == nullptr) the up to two words of the ungapped form; x0 = POS - 1
struct GalnWords {
    const uint32_t* ops;
    uint32_t n, own[2];
    int64_t x0;
};
COV_HD uint32_t galn_word(const GalnWords& w, uint32_t i) { return w.ops ? w.ops[i] : w.own[i]; }

COV_HD GalnWords galn_line_words(const sfgpu_hit& h, uint32_t which, uint64_t slot, const int32_t* aln_pos, const uint64_t* aln_op_off, const uint32_t* aln_ops) {
    GalnWords w;
    w.own[0] = w.own[1] = 0;
    if (aln_pos) {
        w.ops = aln_ops + aln_op_off[slot];
        w.n = (uint32_t)(aln_op_off[slot + 1] - aln_op_off[slot]);
        w.x0 = aln_pos[slot];
        return w;
    }
    const int32_t pos = which ? h.mate_pos : h.pos;
    const uint32_t len = which ? h.mate_len : h.read_len;
    w.ops = nullptr; w.n = 0; w.x0 = 0;
    if (!samw_pos_ok(pos, len)) return w;
    uint32_t p, clip, match;
    samw_aligned(pos, len, &p, &clip, &match);
    w.x0 = (int64_t)p - 1;
    if (clip) w.own[w.n++] = clip << 4 | 4u;
    w.own[w.n++] = match << 4;
    return w;
}

// the reference columns of the words
COV_HD uint64_t galn_ref_span(const GalnWords& w) {
    uint64_t span = 0;
    for (uint32_t i = 0; i < w.n; ++i) {
        const uint32_t v = galn_word(w, i);
        if (galn_ref_op(v & 15u)) span += v >> 4;
    }
    return span;
}

// a placed transcript's blocks: toff[i] is block i's transcript offset plus toff0 (toff has nb + 1 entries), gs / len its place
struct GalnBlocks {
    const uint64_t* toff;
    const uint32_t *gs, *len;
    uint64_t nb, toff0;
    int strand;
};
COV_HD int64_t galn_g(const GalnBlocks& B, uint64_t b, int64_t x) {
    const int64_t d = x - (int64_t)(B.toff[b] - B.toff0);
    return B.strand > 0 ? (int64_t)B.gs[b] + d : (int64_t)B.gs[b] + (int64_t)B.len[b] - 1 - d;
}
COV_HD uint64_t galn_gap(const GalnBlocks& B, uint64_t b) {                // between block b and b + 1
    return B.strand > 0 ? (uint64_t)B.gs[b + 1] - ((uint64_t)B.gs[b] + B.len[b]) : (uint64_t)B.gs[b] - ((uint64_t)B.gs[b + 1] + B.len[b + 1]);
}
// the block that holds x >= 0; the last one for x >= L
COV_HD uint64_t galn_block_of(const GalnBlocks& B, int64_t x) {
    uint64_t lo = 0, hi = B.nb;                            // toff[lo] <= x + toff0 < toff[hi], or lo the last
    const uint64_t key = (uint64_t)x + B.toff0;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (B.toff[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

struct GalnLine {
    uint32_t n_out, n_N;         // the words written, the N among them
    uint64_t beyond;             // reference columns at x >= L
    int64_t lo, hi;              // the interval on the chromosome
    bool too_long;               // an N of 2^28 bases or more
};

// One line with a reference column at x0 >= 0 over a transcript of nb >= 1 blocks.  put(k, word): word k of the line in TRANSCRIPT
// order (the caller turns the order on -).
template <typename Put>
COV_HD GalnLine galn_walk(const GalnWords& w, const GalnBlocks& B, Put put) {
    GalnLine out;
    out.n_out = 0; out.n_N = 0; out.beyond = 0; out.too_long = false;
    const uint64_t L = B.toff[B.nb] - B.toff0;
    int64_t x = w.x0, g_first = 0, g_last = 0;
    uint64_t b = galn_block_of(B, x);
    bool any = false;
    for (uint32_t i = 0; i < w.n; ++i) {
        const uint32_t v = galn_word(w, i), op = v & 15u;
        uint64_t rem = v >> 4, cur = 0;
        if (!galn_ref_op(op) || rem == 0) { put(out.n_out++, v); continue; }
        while (rem) {
            const int64_t end_b = (int64_t)(B.toff[b + 1] - B.toff0);
            if (b + 1 < B.nb && x >= end_b) {              // the next column lies in the next block
                const uint64_t gap = galn_gap(B, b);
                ++b;
                if (gap) {
                    if (cur) { put(out.n_out++, (uint32_t)(cur << 4) | op); cur = 0; }
                    put(out.n_out++, (uint32_t)(gap << 4) | 3u);
                    ++out.n_N;
                    if (gap >= kGalnMaxOpLen) out.too_long = true;
                }
                continue;
            }
            const uint64_t take = b + 1 < B.nb && (uint64_t)(end_b - x) < rem ? (uint64_t)(end_b - x) : rem;
            if (!any) { g_first = galn_g(B, b, x); any = true; }
            g_last = galn_g(B, b, x + (int64_t)take - 1);
            if ((uint64_t)x + take > L) out.beyond += (uint64_t)x + take - ((uint64_t)x > L ? (uint64_t)x : L);
            cur += take; x += (int64_t)take; rem -= take;
        }
        put(out.n_out++, (uint32_t)(cur << 4) | op);
    }
    if (B.strand > 0) { out.lo = g_first; out.hi = g_last + 1; }
    else { out.lo = g_last; out.hi = g_first + 1; }
    return out;
}

// what becomes of one line: GALN_KEPT (then *line is its walk, counted with put), GALN_UNALIGNABLE or GALN_OFF_RANGE
template <typename Put>
COV_HD int galn_line(const GalnWords& w, const GalnBlocks& B, GalnLine* line, Put put) {
    if (galn_ref_span(w) == 0) return GALN_UNALIGNABLE;
    if (w.x0 < 0) return GALN_OFF_RANGE;
    *line = galn_walk(w, B, put);
    return line->lo < 0 || line->hi > kGalnMaxEnd || line->too_long ? GALN_OFF_RANGE : GALN_KEPT;
}

// a record's fate from its lines': the first failing test in the order unplaced, unalignable, off_range
COV_HD int galn_merge(int k0, bool two, int k1) {
    if (!two) return k0;
    if (k0 == GALN_UNALIGNABLE || k1 == GALN_UNALIGNABLE) return GALN_UNALIGNABLE;
    return k0 != GALN_KEPT ? k0 : k1;
}

// the record written for h: its lines' intervals are [lo0, hi0) and, of a pair, [lo1, hi1)
COV_HD sfgpu_hit galn_record(const sfgpu_hit& h, uint32_t chrom, int strand, int64_t lo0, int64_t hi0, int64_t lo1, int64_t hi1) {
    sfgpu_hit o = h;
    o.tid = chrom;
    o.pos = (int32_t)lo0;
    if (h.mate_status == 3) {
        o.mate_pos = (int32_t)lo1;
        o.frag_len = (uint32_t)((hi0 > hi1 ? hi0 : hi1) - (lo0 < lo1 ? lo0 : lo1));
    }
    if (strand < 0) { o.fwd = h.fwd ? 0 : 1; o.mate_fwd = h.mate_fwd ? 0 : 1; }
    return o;
}

COV_HD uint8_t galn_md_comp(uint8_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }
COV_HD bool galn_md_digit(uint8_t c) { return c >= '0' && c <= '9'; }
// the MD of a line on a - transcript: out[0 .. n) from in[0 .. n)
COV_HD void galn_md_reverse(const uint8_t* in, uint64_t n, uint8_t* out) {
    for (uint64_t a = 0; a < n;) {
        uint64_t b = a + 1;
        if (galn_md_digit(in[a])) {
            while (b < n && galn_md_digit(in[b])) ++b;
            for (uint64_t i = a; i < b; ++i) out[n - b + (i - a)] = in[i];
        } else if (in[a] == '^') {
            while (b < n && !galn_md_digit(in[b]) && in[b] != '^') ++b;
            out[n - b] = '^';
            for (uint64_t i = a + 1; i < b; ++i) out[n - b + (b - i)] = galn_md_comp(in[i]);
        } else {
            out[n - b] = galn_md_comp(in[a]);
        }
        a = b;
    }
}

#if !defined(__HIPCC__)
// The whole of it, serially (host only).  The model's arrays are the ones sfgpu_galn_open takes; the batch's the ones of
// sfgpu_galn_batch, each optional group nullptr when not given.
struct GalnSerial {
    std::vector<sfgpu_hit> hits;
    std::vector<uint32_t> hit_off, nm, tag_nm, ops, src_record;
    std::vector<int32_t> pos;
    std::vector<uint64_t> op_off, md_off;
    std::vector<uint8_t> md;
    uint64_t count[kGaCounters] = {0};

    // -> -1, or the lowest record whose tid is no transcript of the M (nothing is written then)
    int64_t project(const uint8_t* status, const int32_t* chrom, const int8_t* strand, const uint64_t* exon_off, const uint32_t* exon_start, const uint32_t* exon_len,
                    uint64_t M, const sfgpu_hit* in, const uint32_t* in_off, uint32_t n_reads, const int32_t* aln_pos, const uint64_t* aln_op_off,
                    const uint32_t* aln_ops, const uint32_t* aln_nm, const uint32_t* t_nm, const uint64_t* t_md_off, const uint8_t* t_md) {
        const uint64_t n = n_reads ? in_off[n_reads] : 0;
        for (uint64_t i = 0; i < n; ++i) if (in[i].tid >= M) return (int64_t)i;
        std::vector<uint64_t> prefix(exon_off[M] + 1, 0);
        for (uint64_t e = 0; e < exon_off[M]; ++e) prefix[e + 1] = prefix[e] + exon_len[e];
        hit_off.assign(1, 0); op_off.assign(1, 0); md_off.assign(1, 0);
        for (uint32_t r = 0; r < n_reads; ++r) {
            for (uint64_t i = in_off[r]; i < in_off[r + 1]; ++i) {
                const sfgpu_hit& h = in[i];
                const uint64_t t = h.tid, e0 = exon_off[t], nb = exon_off[t + 1] - e0;
                const bool two = h.mate_status == 3;
                ++count[kGaRecordsIn];
                if (status[t] != 0 || nb == 0) { ++count[kGaUnplaced]; continue; }
                const GalnBlocks B = {prefix.data() + e0, exon_start + e0, exon_len + e0, nb, prefix[e0], strand[t]};
                std::vector<uint32_t> words[2];
                GalnLine line[2] = {};
                GalnWords w[2];
                int kind[2] = {GALN_KEPT, GALN_KEPT};
                for (uint32_t j = 0; j < (two ? 2u : 1u); ++j) {
                    w[j] = galn_line_words(h, j, 2 * i + j, aln_pos, aln_op_off, aln_ops);
                    kind[j] = galn_line(w[j], B, &line[j], [&](uint32_t, uint32_t v) { words[j].push_back(v); });
                }
                const int fate = galn_merge(kind[0], two, kind[1]);
                if (fate != GALN_KEPT) { ++count[fate == GALN_UNALIGNABLE ? kGaUnalignable : kGaOffRange]; continue; }
                ++count[kGaRecordsOut];
                hits.push_back(galn_record(h, (uint32_t)chrom[t], strand[t], line[0].lo, line[0].hi, line[1].lo, line[1].hi));
                src_record.push_back((uint32_t)i);
                for (uint32_t j = 0; j < 2; ++j) {
                    const uint64_t s = 2 * i + j;
                    if (j == 1 && !two) {
                        pos.push_back(0); nm.push_back(0); tag_nm.push_back(0);
                        op_off.push_back(ops.size()); md_off.push_back(md.size());
                        continue;
                    }
                    ++count[kGaLines];
                    count[kGaLinesSpliced] += line[j].n_N != 0; count[kGaNOps] += line[j].n_N; count[kGaLinesReversed] += strand[t] < 0;
                    count[kGaBeyond] += line[j].beyond; count[kGaWordsIn] += w[j].n; count[kGaWordsOut] += line[j].n_out;
                    pos.push_back((int32_t)line[j].lo);
                    nm.push_back(aln_nm ? aln_nm[s] : 0);
                    tag_nm.push_back(t_nm ? t_nm[s] : 0);
                    if (strand[t] > 0) ops.insert(ops.end(), words[j].begin(), words[j].end());
                    else ops.insert(ops.end(), words[j].rbegin(), words[j].rend());
                    op_off.push_back(ops.size());
                    if (t_md_off) {
                        const uint64_t a = t_md_off[s], len = t_md_off[s + 1] - a, at = md.size();
                        md.resize(at + len);
                        if (strand[t] > 0) for (uint64_t q = 0; q < len; ++q) md[at + q] = t_md[a + q];
                        else galn_md_reverse(t_md + a, len, md.data() + at);
                    }
                    md_off.push_back(md.size());
                }
            }
            count[kGaReadsEmptied] += in_off[r + 1] > in_off[r] && hits.size() == hit_off.back();
            hit_off.push_back((uint32_t)hits.size());
        }
        return -1;
    }
};
#endif

}  // namespace sfgpu
