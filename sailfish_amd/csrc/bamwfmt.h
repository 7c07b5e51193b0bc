// bamwfmt.h -- the BAM records this library writes for its hit records, stated once: the records of
// samfile.sam_to_bam(samfile._sam_text(...)) (what samfile.write_bam writes), byte for byte from the first record on.  Plain C++,
// host and device, serial: samtext_write.hip runs the same functions inside its kernels, tests/bamwrite_harness.cpp runs them
// alone (bamw_serial below).  WHICH lines a batch gives and what FLAG, POS, clip / match, PNEXT, TLEN and mate say is samwfmt.h's
// SamwLine and is not stated again here; this file says how one SamwLine reads as a record.
//
// A record is, little-endian,
//   int32 block_size (the bytes behind it)   int32 refID (tid, or -1)   int32 pos (POS - 1: -1 when unmapped)
//   uint8 l_read_name (QNAME and its NUL)    uint8 mapq 255             uint16 bin     uint16 n_cigar_op   uint16 flag
//   uint32 l_seq                             int32 next_refID (own tid for '=', else -1)   int32 next_pos (PNEXT - 1)   int32 tlen
//   QNAME NUL | n_cigar_op words len << 4 | op (S = 4 then M = 0; a line without clip has the M word alone, an unmapped line none)
//   | SEQ, 4 bits a base, the high nibble first, through =ACMGRSVTWYHKDBN after upper-casing, anything else 15
//   | QUAL, l_seq bytes: 0xff without qualities, else the quality bytes - 33.
// A record is what sam_to_bam makes of samwfmt.h's line: on a line that samwfmt.h puts on the reference's strand (samw_reversed) the
// bases are taken from the last to the first and complemented (samw_comp) before they are packed, the qualities are reversed.
// bin is the specification's reg2bin(pos, pos + max(match, 1)), 4680 when pos < 0.  SEQ '*' (no bases given) is l_seq 0.  TLEN is
// a frag_len below 2^31 (a larger one is written modulo 2^32; sam_to_bam cannot pack it at all).
// What BAM cannot say fails the batch like samwfmt.h's kinds 1 and 2, after them where one record breaks several:
//   3  QNAME not 1 .. 254 bytes
//   4  bases given whose number differs from the line's read length (clip + match; an unmapped line has none to differ from), or
//      more than 65 535 bases
//   5  the alignment ends beyond 2^29: pos + match > 2^29
// With tags given (samwfmt.h: samw_tags) a mapped line's record ends, behind QUAL, NM <t> <nm> | MD Z <md> NUL | NH <t> <nh>, <t>
// being the first of c C s S i I that holds the value (what sam_to_bam picks), and block_size counts them.
// With posteriors given (samwfmt.h: samw_zw) the record then ends Z W f and the four bytes of tag_zw_f32's float: what sam_to_bam
// makes of the text's ZW:f:<token>; block_size counts those seven bytes.
// With an alignment given (samwfmt.h: samw_line) the CIGAR words are the slot's; bin and rule 5 take the reference span (M + D) for
// `match`, rule 4 compares the bases with the read bases the CIGAR names (S + M + I) and also covers more than 65 535 operations.
#pragma once
#include "samwfmt.h"

namespace sfgpu {

enum { BAMW_BAD_QNAME = 3, BAMW_BAD_SEQ = 4, BAMW_BAD_END = 5 };
constexpr uint32_t kBamwFixed = 36;               // block_size .. tlen
constexpr uint32_t kBamwMaxSeq = 65535;
constexpr uint32_t kBamwUnmappedBin = 4680;

// the specification's bin of the zero-based half-open interval [beg, end)
SAMW_HD uint32_t bamw_reg2bin(uint32_t beg, uint32_t end) {
    --end;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0;
}

// the 4-bit code of a base
SAMW_HD uint32_t bamw_base_code(uint8_t c) {
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 'a' + 'A');
    switch (c) {
        case '=': return 0;  case 'A': return 1;  case 'C': return 2;  case 'M': return 3;
        case 'G': return 4;  case 'R': return 5;  case 'S': return 6;  case 'V': return 7;
        case 'T': return 8;  case 'W': return 9;  case 'Y': return 10; case 'H': return 11;
        case 'K': return 12; case 'D': return 13; case 'B': return 14;
        default: return 15;
    }
}
// byte i of the packed SEQ of n bases
SAMW_HD uint8_t bamw_packed_byte(const uint8_t* seq, uint64_t n, uint64_t i) {
    const uint32_t hi = bamw_base_code(seq[2 * i]), lo = 2 * i + 1 < n ? bamw_base_code(seq[2 * i + 1]) : 0u;
    return (uint8_t)(hi << 4 | lo);
}

// byte i of the packed SEQ of the reverse complement of n bases: bases n - 1 - 2i and n - 2 - 2i, low nibble 0 past the start
SAMW_HD uint8_t bamw_packed_byte_rev(const uint8_t* seq, uint64_t n, uint64_t i) {
    const uint32_t hi = bamw_base_code(samw_comp(seq[n - 1 - 2 * i])), lo = 2 * i + 1 < n ? bamw_base_code(samw_comp(seq[n - 2 - 2 * i])) : 0u;
    return (uint8_t)(hi << 4 | lo);
}

SAMW_HD uint32_t bamw_cigar_ops(const SamwLine& l) { return !l.mapped ? 0u : l.ops ? l.n_ops : (l.clip ? 2u : 1u); }
// l_seq of the line of read r
SAMW_HD uint64_t bamw_l_seq(const SamwArgs& a, const SamwLine& l, uint64_t r, const uint8_t** seq) {
    uint64_t n;
    return samw_seq(a, l, r, seq, &n) ? n : 0;
}

// 0, or the first rule of this file the line breaks
SAMW_HD int bamw_check_line(const SamwArgs& a, const SamwLine& l, uint64_t r) {
    const uint64_t qn = samw_qname_len(a, r);
    if (qn < 1 || qn > 254) return BAMW_BAD_QNAME;
    const uint8_t* seq;
    uint64_t n;
    if (samw_seq(a, l, r, &seq, &n) && (n > kBamwMaxSeq || (l.mapped && n != (uint64_t)l.query))) return BAMW_BAD_SEQ;
    if (l.mapped && l.n_ops > 65535u) return BAMW_BAD_SEQ;
    if (l.mapped && (uint64_t)(l.pos - 1u) + l.ref_span > (1ull << 29)) return BAMW_BAD_END;
    return 0;
}
// 0, or the first rule the unit breaks, samwfmt.h's rules first (h == nullptr: the read has no record; hidx: h's index in a.hits)
SAMW_HD int bamw_check(const SamwArgs& a, uint64_t r, const sfgpu_hit* h, uint64_t rank, uint64_t hidx) {
    if (h) if (const int kind = samw_check_a(a, *h, hidx)) return kind;
    const uint32_t n = h ? samw_record_lines(*h) : samw_empty_lines(a.paired != 0);
    int worst = 0;
    for (uint32_t w = 0; w < n; ++w) {
        const int kind = bamw_check_line(a, h ? samw_line(a, *h, rank, w, hidx) : samw_empty_line(a.paired != 0, w), r);
        if (kind && (!worst || kind < worst)) worst = kind;
    }
    return worst;
}
// the same where h is nullptr or points INTO a.hits (never at a copy)
SAMW_HD int bamw_check(const SamwArgs& a, uint64_t r, const sfgpu_hit* h, uint64_t rank) {
    return bamw_check(a, r, h, rank, h ? (uint64_t)(h - a.hits) : 0ull);
}

// an integer tag's type, the first of c C s S i I that holds v, and its value's bytes
SAMW_HD char bamw_int_type(uint32_t v) { return v <= 127u ? 'c' : v <= 255u ? 'C' : v <= 32767u ? 's' : v <= 65535u ? 'S' : v <= 0x7fffffffu ? 'i' : 'I'; }
SAMW_HD uint32_t bamw_int_bytes(uint32_t v) { return v <= 255u ? 1u : v <= 65535u ? 2u : 4u; }
// tag, type and value through put(i, byte) -> their bytes
template <typename Put>
SAMW_HD uint32_t bamw_put_int_tag(char t0, char t1, uint32_t v, Put put) {
    const uint32_t n = bamw_int_bytes(v);
    put(0, (uint8_t)t0); put(1, (uint8_t)t1); put(2, (uint8_t)bamw_int_type(v));
    for (uint32_t i = 0; i < n; ++i) put(3 + (int)i, (uint8_t)(v >> (8 * i)));
    return 3u + n;
}
// the bytes behind QUAL
SAMW_HD uint64_t bamw_tags_len(const SamwArgs& a, const SamwLine& l, uint64_t r) {
    SamwTags t;
    if (!samw_tags(a, l, r, &t)) return 0;
    return 3ull + bamw_int_bytes(t.nm) + 3ull + t.md_len + 1ull + 3ull + bamw_int_bytes(t.nh);
}
// Z W f and the float's bytes, behind the other tags
constexpr uint32_t kBamwZw = 7;
SAMW_HD uint64_t bamw_zw_len(const SamwArgs& a, const SamwLine& l) { return a.tag_zw_rec && l.mapped ? kBamwZw : 0u; }
// byte i of them
SAMW_HD uint8_t bamw_zw_byte(const SamwArgs& a, const SamwLine& l, uint32_t i) {
    if (i < 3u) return (uint8_t)"ZWf"[i];
    return reinterpret_cast<const uint8_t*>(a.tag_zw_f32 + (l.slot >> 1))[i - 3u];
}
SAMW_HD uint64_t bamw_line_len(const SamwArgs& a, const SamwLine& l, uint64_t r) {
    const uint8_t* seq;
    const uint64_t n = bamw_l_seq(a, l, r, &seq);
    return kBamwFixed + samw_qname_len(a, r) + 1u + 4u * bamw_cigar_ops(l) + (n + 1) / 2 + n + bamw_tags_len(a, l, r) + bamw_zw_len(a, l);
}
SAMW_HD uint64_t bamw_unit_len(const SamwArgs& a, uint64_t r, const sfgpu_hit* h, uint64_t rank, uint64_t hidx) {
    const uint32_t n = h ? samw_record_lines(*h) : samw_empty_lines(a.paired != 0);
    uint64_t len = 0;
    for (uint32_t w = 0; w < n; ++w) len += bamw_line_len(a, h ? samw_line(a, *h, rank, w, hidx) : samw_empty_line(a.paired != 0, w), r);
    return len;
}
SAMW_HD uint64_t bamw_unit_len(const SamwArgs& a, uint64_t r, const sfgpu_hit* h, uint64_t rank) {      // (h nullptr or INTO a.hits)
    return bamw_unit_len(a, r, h, rank, h ? (uint64_t)(h - a.hits) : 0ull);
}

// the kBamwFixed bytes in front of QNAME: put(i, byte); line_len is bamw_line_len, qname_len without the NUL
template <typename Put>
SAMW_HD void bamw_put_fixed(const SamwLine& l, uint32_t tid, uint64_t line_len, uint64_t qname_len, uint64_t l_seq, Put put) {
    int p = 0;
    auto le = [&](uint32_t v, int n) { for (int i = 0; i < n; ++i) put(p++, (uint8_t)(v >> (8 * i))); };
    const uint32_t pos0 = l.pos - 1u;             // POS 0 gives -1
    le((uint32_t)(line_len - 4), 4);
    le(l.mapped ? tid : 0xffffffffu, 4);
    le(pos0, 4);
    le((uint32_t)qname_len + 1u, 1);
    le(255u, 1);
    le(l.mapped ? bamw_reg2bin(pos0, pos0 + (l.ref_span ? l.ref_span : 1u)) : kBamwUnmappedBin, 2);
    le(bamw_cigar_ops(l), 2);
    le(l.flag, 2);
    le((uint32_t)l_seq, 4);
    le(l.rnext == '=' ? tid : 0xffffffffu, 4);
    le(l.pnext - 1u, 4);
    le((uint32_t)l.tlen, 4);
}
// the 4 * bamw_cigar_ops(l) bytes behind the name's NUL
template <typename Put>
SAMW_HD void bamw_put_cigar(const SamwLine& l, Put put) {
    int p = 0;
    auto le = [&](uint32_t v) { for (int i = 0; i < 4; ++i) put(p++, (uint8_t)(v >> (8 * i))); };
    if (!l.mapped) return;
    if (l.ops) { for (uint32_t i = 0; i < l.n_ops; ++i) le(l.ops[i]); return; }
    if (l.clip) le(l.clip << 4 | 4u);
    le(l.match << 4);
}

#if !defined(__HIPCC__)
// The records of a batch, serially (host only).  Pass 1 sizes and checks: returns 0 and the sizes, or the kind of the lowest
// (read, record) that breaks a rule (a read without records counts as record 0).  Pass 2 (out != nullptr) writes.
inline int bamw_serial(const SamwArgs& a, uint8_t* out, SamwSerial* res) {
    *res = SamwSerial();
    for (uint64_t r = 0; r < a.n_reads && !res->error_kind; ++r) {
        const uint64_t h0 = a.hit_off[r], h1 = a.hit_off[r + 1];
        for (uint64_t h = h0; h < h1 || (h == h0 && h0 == h1); ++h)
            if (int kind = bamw_check(a, r, h0 == h1 ? nullptr : a.hits + h, h - h0)) {
                res->error_read = r; res->error_record = h - h0; res->error_kind = kind;
                break;
            }
    }
    if (int kind = samw_merge_qual(a, res)) return kind;
    uint64_t at = 0;
    auto line = [&](const SamwLine& l, uint64_t r, uint32_t tid) {
        const uint64_t len = bamw_line_len(a, l, r), qn = samw_qname_len(a, r);
        const uint8_t* s;
        const uint64_t n = bamw_l_seq(a, l, r, &s);
        if (out) {
            uint8_t* p = out + at;
            bamw_put_fixed(l, tid, len, qn, n, [&](int i, uint8_t b) { p[i] = b; }); p += kBamwFixed;
            if (a.qname_off) for (uint64_t i = a.qname_off[r]; i < a.qname_off[r + 1]; ++i) *p++ = (uint8_t)a.qnames[i];
            else { samw_put_default_qname(a.read_index_base + r, [&](int i, char ch) { p[i] = (uint8_t)ch; }); p += qn; }
            *p++ = 0;
            bamw_put_cigar(l, [&](int i, uint8_t b) { p[i] = b; }); p += 4 * bamw_cigar_ops(l);
            const bool rev = samw_reversed(a, l);
            for (uint64_t i = 0; i < (n + 1) / 2; ++i) *p++ = rev ? bamw_packed_byte_rev(s, n, i) : bamw_packed_byte(s, n, i);
            const uint8_t* q;
            uint64_t ql;
            const bool given = samw_qual(a, l, r, &q, &ql);
            for (uint64_t i = 0; i < n; ++i) *p++ = given ? (uint8_t)((rev ? q[n - 1 - i] : q[i]) - 33u) : (uint8_t)0xff;
            SamwTags t;
            if (samw_tags(a, l, r, &t)) {
                p += bamw_put_int_tag('N', 'M', t.nm, [&](int i, uint8_t b) { p[i] = b; });
                *p++ = 'M'; *p++ = 'D'; *p++ = 'Z';
                for (uint64_t i = 0; i < t.md_len; ++i) *p++ = t.md[i];
                *p++ = 0;
                p += bamw_put_int_tag('N', 'H', t.nh, [&](int i, uint8_t b) { p[i] = b; });
            }
            for (uint32_t i = 0; i < bamw_zw_len(a, l); ++i) *p++ = bamw_zw_byte(a, l, i);
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
