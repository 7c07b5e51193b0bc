// samwfmt.h -- the SAM lines this library writes for its hit records, stated once: the alignment lines of samfile._sam_text (the
// text samfile.write_sam writes), byte for byte, for `paired` given explicitly.  Plain C++, host and device, serial:
// samtext_write.hip runs the same functions inside its kernels (WHERE a line lies in the output and which lines a tile holds is
// found in parallel there; WHAT a line says is decided here), and tests/samwrite_harness.cpp runs them alone (samw_serial below).
//
// A line is   QNAME \t FLAG \t RNAME \t POS \t 255 \t CIGAR \t RNEXT \t PNEXT \t TLEN \t SEQ \t QUAL \n
// and a UNIT is what one hit record or one read without records produces; units follow each other in read order, a read's
// records in their order.
//   pair record (mate_status 3): two lines.  FLAG 0x1|0x2|0x40|sec|(fwd ? 0 : 0x10)|(mate_fwd ? 0 : 0x20), then the mirrored 0x80
//          line (0x10 from mate_fwd, 0x20 from fwd); RNEXT '='; PNEXT the other line's POS; TLEN +frag_len on the first line iff
//          pos <= mate_pos, negated on the second; SEQ of mate 1, then of mate 2.
//   orphan (any other nonzero mate_status): one line.  FLAG 0x1|0x8|0x40 (status 1, SEQ of mate 1) or 0x1|0x8|0x80 (SEQ of
//          mate 2), |sec|(fwd ? 0 : 0x10); RNEXT '*', PNEXT 0, TLEN 0.
//   single-end record (mate_status 0): one line.  FLAG sec|(fwd ? 0 : 0x10); RNEXT '*', PNEXT 0, TLEN 0; SEQ of mate 1.
//   sec = 0x100 from the read's second record on.
//   read without a record: paired, the lines 77 and 141 (SEQ of mate 1, of mate 2); single end, one line 4.  RNAME '*', POS 0,
//          CIGAR '*', RNEXT '*', PNEXT 0, TLEN 0.
//   POS and CIGAR of a read of len bases at pos: pos >= 0 gives pos + 1 and <len>M; pos < 0 gives 1 and <-pos>S<len + pos>M, and
//          -pos >= len is an error (no base lies on the transcript: SAM cannot say that), as is tid >= n_refs.
//   MAPQ is 255.  QNAME is the caller's bytes, or r<global read index> when none are given; SEQ is the caller's bytes, or '*' when
//   none are given; RNAME is the transcript's name.  Names are copied, never inspected.
//   QUAL is '*' unless the mate's qualities are given (qual1 / qual2: bytes back to back that share the mate's base offsets, so
//          they can only be given with the bases): then it is those bytes, on every line that carries the mate's SEQ (0x100 lines and
//          the 77 / 141 / 4 lines too); a read of 0 bases has an empty QUAL as it has an empty SEQ.  Every quality byte must lie in
//          '!' .. '~' (a tab or a newline would break the text; BAM stores byte - 33): a read that holds another one fails the batch
//          as (read, record 0) of kind SAMW_BAD_QUAL, merged with the other kinds by lowest (read, record), then lowest kind.  One
//          quality byte '*' of a 1-base read reads as "no qualities": the format's ambiguity, written as it is.
//   Orientation: with `oriented` == 0 SEQ and QUAL are written as given on every line (the reader, samfmt.h, takes only SEQ's
//          length).  With `oriented` != 0 a line whose FLAG has 0x10 stores them on the reference's strand, as the SAM
//          specification has it: SEQ reverse-complemented (samw_comp, byte by byte), QUAL reversed.  Lines without 0x10 -- every
//          line of a read without records among them -- are as given.
//   Alignments: with aln_pos / aln_op_off / aln_ops given (sfgpu_hits_align_gapped's outputs for the same records: two slots per
//          record, slot 2 h + which is line `which` of record h) a mapped line takes POS = aln_pos[slot] + 1 and its CIGAR from the
//          slot's words len << 4 | op (MIDNSHP=X), PNEXT is the other line's POS written this way; FLAG and TLEN stay.  The position
//          rule is then the slot's: a line whose slot has no operation has no base on the transcript (SAMW_BAD_POS), and the record's
//          own pos is not consulted.  Without them every byte is what it is above.
//   Tags: with tag_nm / tag_md_off / tag_md given (sfgpu_hits_md_tags' outputs for the same records and the same alignment, two
//          slots per record as above; csrc/mdfmt.h) a mapped line ends ... QUAL \t NM:i:<nm> \t MD:Z:<md> \t NH:i:<nh> \n, nh being the
//          read's record count hit_off[r + 1] - hit_off[r].  The lines of a read without records carry no tags.  Without them every
//          byte is what it is above.
//   Posteriors: with tag_zw_rec / tag_zw_f32 given (sfgpu_hits_posteriors' d_rec and d_f32 for the same records: one entry per
//          record, slot >> 1) a mapped line ends, behind the tags above where they are given, \t ZW:f:<token>, the token being the
//          "%g" of the record's posterior probability, placed from its six-digit record (gfmt_len / gfmt_put: no arithmetic on
//          the value happens here).  Both lines of a pair carry the record's value; the lines of a read without records carry
//          nothing.  tag_zw_f32 is what bamwfmt.h stores.  Without them every byte is what it is above.
#pragma once
#include <cstdint>

#include "../../include/sfgpu.h"
#include "decfmt.h"
#include "gfmt.h"

#if defined(__HIPCC__)
#define SAMW_HD __host__ __device__ __forceinline__
#else
#define SAMW_HD inline
#endif

namespace sfgpu {

constexpr uint32_t kSamwTail = 2;                 // \t and \n around QUAL
// (the head \t FLAG \t is at most 5 bytes: the largest FLAG is 0x1b3 = 435; the middle \t POS \t 255 \t CIGAR \t RNEXT \t PNEXT \t TLEN \t
// at most 54 without an alignment: 65535S65535M, -4294967295; with one the CIGAR is as long as its operations make it)
enum { SAMW_OK = 0, SAMW_BAD_POS = 1, SAMW_BAD_TID = 2, SAMW_BAD_QUAL = 6 };     // (3 .. 5 are bamwfmt.h's)

// the complement of a base: A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H, in either case (kept); S, W, N and every other byte as it is
SAMW_HD uint8_t samw_comp(uint8_t c) {
    const uint8_t low = (c >= 'a' && c <= 'z') ? 0x20 : 0;
    uint8_t v;
    switch ((uint8_t)(c - low)) {
        case 'A': v = 'T'; break;  case 'T': v = 'A'; break;  case 'U': v = 'A'; break;
        case 'C': v = 'G'; break;  case 'G': v = 'C'; break;
        case 'R': v = 'Y'; break;  case 'Y': v = 'R'; break;
        case 'K': v = 'M'; break;  case 'M': v = 'K'; break;
        case 'B': v = 'V'; break;  case 'V': v = 'B'; break;
        case 'D': v = 'H'; break;  case 'H': v = 'D'; break;
        default: return c;
    }
    return (uint8_t)(v + low);
}
SAMW_HD bool samw_qual_ok(uint8_t q) { return q >= 33 && q <= 126; }

// what one line says, names and SEQ apart
struct SamwLine {
    int64_t tlen;
    uint32_t flag, pos, pnext;
    uint32_t clip, match;        // CIGAR <clip>S<match>M (clip = 0: <match>M); unmapped: '*'
    const uint32_t* ops;         // an alignment is given: the CIGAR is these n_ops words (clip and match are then 0), else nullptr
    uint32_t n_ops;
    uint32_t ref_span, query;    // the transcript bases the CIGAR covers (M + D) and the read bases it names (S + M + I)
    uint8_t mapped;              // RNAME is the name of the record's tid; else '*'
    uint8_t rnext;               // '=' or '*'
    uint8_t mate2;               // SEQ is mate 2's
    uint64_t slot;               // of a record's line: 2 * (the record's index) + which, where its alignment and its tags lie
};

SAMW_HD uint32_t samw_record_lines(const sfgpu_hit& h) { return h.mate_status == 3 ? 2u : 1u; }
SAMW_HD uint32_t samw_empty_lines(bool paired) { return paired ? 2u : 1u; }

// _aligned's rule for one mate
SAMW_HD bool samw_pos_ok(int32_t pos, uint32_t len) { return pos >= 0 || -(int64_t)pos < (int64_t)len; }

// 0, or the first rule the record breaks (the position rule before the transcript id, as _sam_text meets them)
SAMW_HD int samw_check(const sfgpu_hit& h, uint32_t n_refs) {
    if (!samw_pos_ok(h.pos, h.read_len)) return SAMW_BAD_POS;
    if (h.mate_status == 3 && !samw_pos_ok(h.mate_pos, h.mate_len)) return SAMW_BAD_POS;
    if (h.tid >= n_refs) return SAMW_BAD_TID;
    return SAMW_OK;
}

SAMW_HD void samw_aligned(int32_t pos, uint32_t len, uint32_t* p, uint32_t* clip, uint32_t* match) {
    if (pos >= 0) { *p = (uint32_t)pos + 1u; *clip = 0; *match = len; }
    else { *p = 1; *clip = (uint32_t)(-(int64_t)pos); *match = (uint32_t)((int64_t)len + pos); }
}

// line `which` (0, or 1 for the second line of a pair record) of a checked record that is number `rank` among its read's
SAMW_HD SamwLine samw_record_line(const sfgpu_hit& h, uint64_t rank, uint32_t which) {
    SamwLine l;
    const uint32_t sec = rank ? 0x100u : 0u, st = h.mate_status;
    uint32_t p1, c1, m1;
    samw_aligned(h.pos, h.read_len, &p1, &c1, &m1);
    l.mapped = 1; l.ops = nullptr; l.n_ops = 0; l.slot = 0;
    if (st == 3) {
        uint32_t p2, c2, m2;
        samw_aligned(h.mate_pos, h.mate_len, &p2, &c2, &m2);
        const int64_t tlen = h.pos <= h.mate_pos ? (int64_t)h.frag_len : -(int64_t)h.frag_len;
        const uint32_t r1 = h.fwd ? 0u : 1u, r2 = h.mate_fwd ? 0u : 1u;
        l.rnext = '=';
        if (which == 0) {
            l.flag = 0x1u | 0x2u | 0x40u | sec | (r1 ? 0x10u : 0u) | (r2 ? 0x20u : 0u);
            l.pos = p1; l.clip = c1; l.match = m1; l.pnext = p2; l.tlen = tlen; l.mate2 = 0;
            l.ref_span = m1; l.query = c1 + m1;
        } else {
            l.flag = 0x1u | 0x2u | 0x80u | sec | (r2 ? 0x10u : 0u) | (r1 ? 0x20u : 0u);
            l.pos = p2; l.clip = c2; l.match = m2; l.pnext = p1; l.tlen = -tlen; l.mate2 = 1;
            l.ref_span = m2; l.query = c2 + m2;
        }
        return l;
    }
    l.pos = p1; l.clip = c1; l.match = m1; l.rnext = '*'; l.pnext = 0; l.tlen = 0;
    l.ref_span = m1; l.query = c1 + m1;
    l.flag = sec | (h.fwd ? 0u : 0x10u);
    l.mate2 = 0;
    if (st) {
        l.flag |= 0x1u | 0x8u | (st == 1 ? 0x40u : 0x80u);
        l.mate2 = st != 1;
    }
    return l;
}

// line `which` of a read without records
SAMW_HD SamwLine samw_empty_line(bool paired, uint32_t which) {
    SamwLine l;
    l.flag = paired ? (which ? 141u : 77u) : 4u;
    l.pos = 0; l.clip = 0; l.match = 0; l.pnext = 0; l.tlen = 0;
    l.ops = nullptr; l.n_ops = 0; l.ref_span = 0; l.query = 0; l.slot = 0;
    l.mapped = 0; l.rnext = '*'; l.mate2 = (uint8_t)(paired && which);
    return l;
}

// QNAME when the caller gives none: r<index>
SAMW_HD uint32_t samw_default_qname_len(uint64_t index) { return 1u + (uint32_t)dec_len_u64(index); }
template <typename Put>
SAMW_HD void samw_put_default_qname(uint64_t index, Put put) {          // put(i, ch): byte i of the name
    const int nd = dec_len_u64(index);
    put(0, 'r');
    dec_put_u64(index, [&](int i, char ch) { put(nd - i, ch); });
}

// the head: \t FLAG \t, between QNAME and RNAME
SAMW_HD uint32_t samw_head_len(const SamwLine& l) { return 2u + (uint32_t)dec_len_u32(l.flag); }
template <typename Put>
SAMW_HD void samw_put_head(const SamwLine& l, Put put) {
    const int nd = dec_len_u32(l.flag);
    put(0, '\t');
    dec_put_fixed_u32(l.flag, nd, 0, [&](int i, char ch) { put(nd - i, ch); });
    put(nd + 1, '\t');
}

SAMW_HD uint32_t samw_cigar_len(const SamwLine& l) {
    if (!l.mapped) return 1;
    if (l.ops) {
        uint32_t n = 0;
        for (uint32_t i = 0; i < l.n_ops; ++i) n += (uint32_t)dec_len_u32(l.ops[i] >> 4) + 1u;
        return n;
    }
    return (l.clip ? (uint32_t)dec_len_u32(l.clip) + 1u : 0u) + (uint32_t)dec_len_u32(l.match) + 1u;
}

// the middle: \t POS \t 255 \t CIGAR \t RNEXT \t PNEXT \t TLEN \t, between RNAME and SEQ
SAMW_HD uint32_t samw_mid_len(const SamwLine& l) {
    const uint32_t t = (uint32_t)(l.tlen < 0 ? -l.tlen : l.tlen);        // |TLEN| is a frag_len: it fits 32 bits
    return 1u + (uint32_t)dec_len_u32(l.pos) + 5u + samw_cigar_len(l) + 3u + (uint32_t)dec_len_u32(l.pnext) + 1u + (l.tlen < 0 ? 1u : 0u) +
           (uint32_t)dec_len_u32(t) + 1u;
}
template <typename Put>
SAMW_HD void samw_put_mid(const SamwLine& l, Put put) {
    int p = 0;
    auto num = [&](uint32_t v) {                  // the digits of v at p .. p + nd - 1
        const int nd = dec_len_u32(v), last = p + nd - 1;
        dec_put_fixed_u32(v, nd, 0, [&](int i, char ch) { put(last - i, ch); });
        p += nd;
    };
    put(p++, '\t'); num(l.pos);
    put(p++, '\t'); put(p++, '2'); put(p++, '5'); put(p++, '5'); put(p++, '\t');
    if (!l.mapped) put(p++, '*');
    else if (l.ops) for (uint32_t i = 0; i < l.n_ops; ++i) { num(l.ops[i] >> 4); put(p++, "MIDNSHP=X???????"[l.ops[i] & 15u]); }
    else {
        if (l.clip) { num(l.clip); put(p++, 'S'); }
        num(l.match); put(p++, 'M');
    }
    put(p++, '\t'); put(p++, (char)l.rnext); put(p++, '\t'); num(l.pnext); put(p++, '\t');
    if (l.tlen < 0) put(p++, '-');
    num((uint32_t)(l.tlen < 0 ? -l.tlen : l.tlen));
    put(p++, '\t');
}

// ---- the arrays of one write call, and the serial statement over them ---------------------------------------------------------
// The batch of the writer entries, sfgpu_samw_batch (include/sfgpu.h, where each field group is described): names and SEQ as
// bytes back to back with n + 1 offsets, the qualities, the alignment, the tags and the posteriors, each group nullptr when not
// given.  C++ callers brace-initialise the leading fields they give (tests/*_harness.cpp) and leave the rest to the language's
// zeroing, which is what "not given" means for every group; the C struct has no default member initialisers to say so, so the
// -Wextra warning about exactly those omitted fields is off for the files that include this one.
using SamwArgs = sfgpu_samw_batch;
#pragma GCC diagnostic ignored "-Wmissing-field-initializers"

// The lines of a record WITH the batch's alignment, where one is given.  `hidx` is the record's index in a.hits: its slots are
// 2 * hidx and 2 * hidx + 1 (h itself may be a copy of the record, as in the kernels).
SAMW_HD SamwLine samw_line(const SamwArgs& a, const sfgpu_hit& h, uint64_t rank, uint32_t which, uint64_t hidx) {
    SamwLine l = samw_record_line(h, rank, which);
    const uint64_t slot = 2 * hidx + which;
    l.slot = slot;
    if (!a.aln_pos) return l;
    l.pos = (uint32_t)a.aln_pos[slot] + 1u;
    if (h.mate_status == 3) l.pnext = (uint32_t)a.aln_pos[slot ^ 1ull] + 1u;
    l.clip = 0; l.match = 0; l.ref_span = 0; l.query = 0;
    l.ops = a.aln_ops + a.aln_op_off[slot];
    l.n_ops = (uint32_t)(a.aln_op_off[slot + 1] - a.aln_op_off[slot]);
    for (uint32_t i = 0; i < l.n_ops; ++i) {
        const uint32_t n = l.ops[i] >> 4, op = l.ops[i] & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) l.ref_span += n;      // M D N = X
        if (op == 0u || op == 1u || op == 4u || op == 7u || op == 8u) l.query += n;         // M I S = X
    }
    return l;
}
// samw_check with the position rule taken from the alignment where one is given
SAMW_HD int samw_check_a(const SamwArgs& a, const sfgpu_hit& h, uint64_t hidx) {
    if (!a.aln_pos) return samw_check(h, a.n_refs);
    const uint64_t slot = 2 * hidx;
    for (uint32_t w = 0; w < samw_record_lines(h); ++w) if (a.aln_op_off[slot + w + 1] == a.aln_op_off[slot + w]) return SAMW_BAD_POS;
    if (h.tid >= a.n_refs) return SAMW_BAD_TID;
    return SAMW_OK;
}

SAMW_HD uint64_t samw_qname_len(const SamwArgs& a, uint64_t r) {
    return a.qname_off ? a.qname_off[r + 1] - a.qname_off[r] : (uint64_t)samw_default_qname_len(a.read_index_base + r);
}
SAMW_HD uint64_t samw_rname_len(const SamwArgs& a, const SamwLine& l, uint32_t tid) {
    return l.mapped ? a.ref_name_off[tid + 1] - a.ref_name_off[tid] : 1u;
}
// SEQ of the line of read r: false and 1 byte for '*', else the bases (a null pointer only with *len == 0)
SAMW_HD bool samw_seq(const SamwArgs& a, const SamwLine& l, uint64_t r, const uint8_t** seq, uint64_t* len) {
    const uint8_t* s = l.mate2 ? a.seq2 : a.seq1;
    const int64_t* o = l.mate2 ? a.seq2_off : a.seq1_off;
    *seq = nullptr; *len = 1;
    if (!o) return false;
    *len = (uint64_t)(o[r + 1] - o[r]);
    if (*len) *seq = s + o[r];
    return true;
}
// QUAL of the line of read r: false and 1 byte for '*', else the qualities, as many as the bases
SAMW_HD bool samw_qual(const SamwArgs& a, const SamwLine& l, uint64_t r, const uint8_t** qual, uint64_t* len) {
    const uint8_t* q = l.mate2 ? a.qual2 : a.qual1;
    const int64_t* o = l.mate2 ? a.seq2_off : a.seq1_off;
    *qual = nullptr; *len = 1;
    if (!q || !o) return false;
    *len = (uint64_t)(o[r + 1] - o[r]);
    *qual = q + o[r];
    return true;
}
// SEQ and QUAL of the line go on the reference's strand
SAMW_HD bool samw_reversed(const SamwArgs& a, const SamwLine& l) { return a.oriented != 0 && (l.flag & 0x10u) != 0; }
// the tags of the line of read r: whether it carries any, and NM, NH and the MD's bytes
struct SamwTags { uint32_t nm, nh; const uint8_t* md; uint64_t md_len; };
SAMW_HD bool samw_tags(const SamwArgs& a, const SamwLine& l, uint64_t r, SamwTags* t) {
    if (!a.tag_nm || !l.mapped) return false;
    t->nm = a.tag_nm[l.slot]; t->nh = a.hit_off[r + 1] - a.hit_off[r];
    t->md_len = a.tag_md_off[l.slot + 1] - a.tag_md_off[l.slot];
    t->md = a.tag_md + a.tag_md_off[l.slot];
    return true;
}
constexpr uint32_t kSamwTagLead = 6;              // \t NM:i:   \t MD:Z:   \t NH:i:
// the bytes between QUAL and the line's \n
SAMW_HD uint64_t samw_tags_len(const SamwArgs& a, const SamwLine& l, uint64_t r) {
    SamwTags t;
    if (!samw_tags(a, l, r, &t)) return 0;
    return 3ull * kSamwTagLead + (uint64_t)dec_len_u32(t.nm) + t.md_len + (uint64_t)dec_len_u32(t.nh);
}
// \t <tag> :i: <v> through put(i, ch) -> its bytes
template <typename Put>
SAMW_HD uint32_t samw_put_int_tag(char t0, char t1, uint32_t v, Put put) {
    put(0, '\t'); put(1, t0); put(2, t1); put(3, ':'); put(4, 'i'); put(5, ':');
    const int nd = dec_len_u32(v);
    dec_put_fixed_u32(v, nd, 0, [&](int i, char ch) { put((int)kSamwTagLead + nd - 1 - i, ch); });
    return kSamwTagLead + (uint32_t)nd;
}
template <typename Put>
SAMW_HD void samw_put_md_lead(Put put) { put(0, '\t'); put(1, 'M'); put(2, 'D'); put(3, ':'); put(4, 'Z'); put(5, ':'); }
// the posterior of the line: whether it carries one, and the record of its token
SAMW_HD bool samw_zw(const SamwArgs& a, const SamwLine& l, uint32_t* rec) {
    if (!a.tag_zw_rec || !l.mapped) return false;
    *rec = a.tag_zw_rec[l.slot >> 1];
    return true;
}
// \t ZW:f:<token>, behind the other tags
SAMW_HD uint64_t samw_zw_len(const SamwArgs& a, const SamwLine& l) {
    uint32_t rec;
    return samw_zw(a, l, &rec) ? (uint64_t)kSamwTagLead + (uint64_t)gfmt_len(rec) : 0ull;
}
template <typename Put>
SAMW_HD uint32_t samw_put_zw(uint32_t rec, Put put) {
    put(0, '\t'); put(1, 'Z'); put(2, 'W'); put(3, ':'); put(4, 'f'); put(5, ':');
    const int n = gfmt_len(rec);
    gfmt_put(rec, [&](int i, char ch) { put((int)kSamwTagLead + n - 1 - i, ch); });
    return kSamwTagLead + (uint32_t)n;
}
SAMW_HD uint64_t samw_line_len(const SamwArgs& a, const SamwLine& l, uint64_t r, uint32_t tid) {
    const uint8_t* p;
    uint64_t sl, ql;
    (void)samw_seq(a, l, r, &p, &sl);
    (void)samw_qual(a, l, r, &p, &ql);
    return samw_qname_len(a, r) + samw_head_len(l) + samw_rname_len(a, l, tid) + samw_mid_len(l) + sl + ql + kSamwTail + samw_tags_len(a, l, r) + samw_zw_len(a, l);
}
// the bytes of unit (read r, record h of rank `rank` and index hidx in a.hits; h == nullptr: the read has no record)
SAMW_HD uint64_t samw_unit_len(const SamwArgs& a, uint64_t r, const sfgpu_hit* h, uint64_t rank, uint64_t hidx) {
    const uint32_t n = h ? samw_record_lines(*h) : samw_empty_lines(a.paired != 0);
    uint64_t len = 0;
    for (uint32_t w = 0; w < n; ++w) len += samw_line_len(a, h ? samw_line(a, *h, rank, w, hidx) : samw_empty_line(a.paired != 0, w), r, h ? h->tid : 0);
    return len;
}
// the same where h is nullptr or points INTO a.hits (never at a copy): the index is the pointer's
SAMW_HD uint64_t samw_unit_len(const SamwArgs& a, uint64_t r, const sfgpu_hit* h, uint64_t rank) {
    return samw_unit_len(a, r, h, rank, h ? (uint64_t)(h - a.hits) : 0ull);
}

#if !defined(__HIPCC__)
// The whole text, serially (host only; the judge of the kernels is still _sam_text).  Pass 1 sizes and checks: returns 0 and the
// sizes, or the kind of the lowest (read, record) that breaks a rule.  Pass 2 (out != nullptr, room for *n_bytes) writes.
struct SamwSerial {
    uint64_t n_bytes = 0, n_lines = 0, n_units = 0, max_unit_bytes = 0, error_read = 0, error_record = 0;
    int error_kind = 0;
};

// the lowest read with a quality byte outside '!' .. '~' (one flat pass over each mate's bytes; every read is written at least
// once), or n_reads
inline uint64_t samw_bad_qual_read(const SamwArgs& a) {
    uint64_t worst = a.n_reads;
    for (int m = 0; m < 2; ++m) {
        const uint8_t* q = m ? a.qual2 : a.qual1;
        const int64_t* o = m ? a.seq2_off : a.seq1_off;
        if (!q || !o) continue;
        for (int64_t i = o[0]; i < o[a.n_reads]; ++i)
            if (!samw_qual_ok(q[i])) {
                uint64_t r = 0;
                while (o[r + 1] <= i) ++r;
                if (r < worst) worst = r;
                break;
            }
    }
    return worst;
}
// the error of the records (kind 0: none) merged with the quality rule: lowest (read, record), then lowest kind
inline int samw_merge_qual(const SamwArgs& a, SamwSerial* res) {
    const uint64_t r = samw_bad_qual_read(a);
    if (r < a.n_reads && (!res->error_kind || r < res->error_read || (r == res->error_read && res->error_record > 0))) {
        res->error_read = r; res->error_record = 0; res->error_kind = SAMW_BAD_QUAL;
    }
    return res->error_kind;
}

inline int samw_serial(const SamwArgs& a, char* out, SamwSerial* res) {
    *res = SamwSerial();
    for (uint64_t r = 0; r < a.n_reads && !res->error_kind; ++r)
        for (uint64_t h = a.hit_off[r]; h < a.hit_off[r + 1]; ++h)
            if (int kind = samw_check_a(a, a.hits[h], h)) {
                res->error_read = r; res->error_record = h - a.hit_off[r]; res->error_kind = kind;
                break;
            }
    if (int kind = samw_merge_qual(a, res)) return kind;
    uint64_t at = 0;
    auto line = [&](const SamwLine& l, uint64_t r, uint32_t tid) {
        const uint64_t len = samw_line_len(a, l, r, tid);
        if (out) {
            char* p = out + at;
            if (a.qname_off) for (uint64_t i = a.qname_off[r]; i < a.qname_off[r + 1]; ++i) *p++ = a.qnames[i];
            else { samw_put_default_qname(a.read_index_base + r, [&](int i, char ch) { p[i] = ch; }); p += samw_default_qname_len(a.read_index_base + r); }
            samw_put_head(l, [&](int i, char ch) { p[i] = ch; }); p += samw_head_len(l);
            if (l.mapped) for (uint64_t i = a.ref_name_off[tid]; i < a.ref_name_off[tid + 1]; ++i) *p++ = a.ref_names[i];
            else *p++ = '*';
            samw_put_mid(l, [&](int i, char ch) { p[i] = ch; }); p += samw_mid_len(l);
            const uint8_t* s;
            uint64_t sl;
            const bool rev = samw_reversed(a, l);
            if (samw_seq(a, l, r, &s, &sl)) for (uint64_t i = 0; i < sl; ++i) *p++ = (char)(rev ? samw_comp(s[sl - 1 - i]) : s[i]);
            else *p++ = '*';
            *p++ = '\t';
            if (samw_qual(a, l, r, &s, &sl)) for (uint64_t i = 0; i < sl; ++i) *p++ = (char)(rev ? s[sl - 1 - i] : s[i]);
            else *p++ = '*';
            SamwTags t;
            if (samw_tags(a, l, r, &t)) {
                p += samw_put_int_tag('N', 'M', t.nm, [&](int i, char ch) { p[i] = ch; });
                samw_put_md_lead([&](int i, char ch) { p[i] = ch; }); p += kSamwTagLead;
                for (uint64_t i = 0; i < t.md_len; ++i) *p++ = (char)t.md[i];
                p += samw_put_int_tag('N', 'H', t.nh, [&](int i, char ch) { p[i] = ch; });
            }
            uint32_t zw;
            if (samw_zw(a, l, &zw)) p += samw_put_zw(zw, [&](int i, char ch) { p[i] = ch; });
            *p++ = '\n';
        }
        at += len;
        res->n_lines++;
    };
    auto unit = [&](uint64_t r, const sfgpu_hit* h, uint64_t rank) {
        const uint64_t before = at;
        const uint32_t n = h ? samw_record_lines(*h) : samw_empty_lines(a.paired != 0);
        for (uint32_t w = 0; w < n; ++w) line(h ? samw_line(a, *h, rank, w, (uint64_t)(h - a.hits)) : samw_empty_line(a.paired != 0, w), r, h ? h->tid : 0);
        res->n_units++;
        if (at - before > res->max_unit_bytes) res->max_unit_bytes = at - before;
    };
    for (uint64_t r = 0; r < a.n_reads; ++r) {
        const uint64_t h0 = a.hit_off[r], h1 = a.hit_off[r + 1];
        if (h0 == h1) unit(r, nullptr, 0);
        for (uint64_t u = h0; u < h1; ++u) unit(r, a.hits + u, u - h0);
    }
    res->n_bytes = at;
    return 0;
}
#endif

}  // namespace sfgpu
