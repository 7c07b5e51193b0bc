// samfmt.h -- what a mapper's SAM text says to this library, stated once: the rules samfile.read_sam_host sets.  Plain C++, host and
// device, serial; samtext.hip runs the same functions inside its kernels (WHERE the lines and their first ten tabs are, which
// lines neighbour each other and which group a line belongs to is found in parallel there; WHAT a line says, which two lines pair
// and which record they make is decided here), and tests/sam_harness.cpp runs them alone (SamSerial below).
//
// Lines end at '\n'; one '\r' directly in front of it is not part of the line; the last line may lack its '\n' (final text only:
// the reader behaves as if it were there).
// A line whose first byte is '@' is a header line: counted, otherwise skipped wherever it stands.  Every other line must have 11
// tab-separated fields (an empty line has not: BAD_FIELDS).  QNAME (1), FLAG (2), RNAME (3), POS (4), CIGAR (6) and SEQ (10) are
// read, nothing else.
//   FLAG   1-5 digits, <= 65535 (BAD_NUMBER).  Paired call: 0x1 and exactly one of 0x40 / 0x80; single-end call: no 0x1 (BAD_FLAG).
//          0x4 or 0x800: the line yields no record but belongs to its group.  0x100 lines are ordinary.
//   mapped line: RNAME is one of the handle's names, bytewise (BAD_RNAME); POS 1-10 digits, 1 .. 2^31 - 1 (BAD_NUMBER); CIGAR '*' or
//          one or more of (1-9 digits, one of MIDNSHP=X) (BAD_CIGAR); lead = the S counts behind the leading H operations and in
//          front of the first other one, qlen = the counts of M I S = X; read_len = |SEQ| unless SEQ is '*', then qlen unless CIGAR
//          is '*', then 0; above 65535, or SEQ and CIGAR both present and |SEQ| != qlen: BAD_LENGTH.  pos = POS - 1 - lead.
//   A line that breaks several rules reports the first of FIELDS, NUMBER, FLAG, RNAME, CIGAR, LENGTH.
// Groups: maximal runs of consecutive non-header lines with byte-equal QNAME; one group = one fragment, records or not.
// Pairs (paired call): a mapped 0x40 line directly followed in its group by a mapped 0x80 line on the same transcript.  A group
// with a pair yields its pairs only; otherwise every mapped line is an orphan (status 1 for 0x40, 2 for 0x80), in a single-end call
// a status-0 record.  Inside a group: left orphans, then right orphans; within a side, and among pairs or single-end records, tid
// ascending, ties in file order.
#pragma once
#include <cstdint>

#include "../../include/sfgpu.h"

#if defined(__HIPCC__)
#define SAM_HD __host__ __device__
#else
#define SAM_HD
#endif

namespace sfgpu {

constexpr uint32_t kSamTabs = 10;                 // the tabs that end fields 1 .. 10
constexpr uint32_t kSamNone = 0xffffffffu;        // no such tab / no such name

// what one line says
struct SamLine {
    uint32_t bad;        // 0, or the SFGPU_SAM_BAD_* bit of the first rule it breaks
    uint32_t q_len;      // QNAME = [line start, + q_len)
    uint32_t tid;
    int32_t pos;
    uint16_t read_len;
    uint8_t header, mapped, side, fwd;      // side: 1 = 0x40, 2 = 0x80, 0 in a single-end call
};

// [a, b) as a decimal number of 1 .. max_digits digits -> true and *v
template <typename Get>
SAM_HD inline bool sam_number(Get get, uint32_t a, uint32_t b, uint32_t max_digits, uint64_t* v) {
    if (b <= a || b - a > max_digits) return false;
    uint64_t x = 0;
    for (uint32_t p = a; p < b; ++p) {
        const unsigned char c = get(p);
        if (c < '0' || c > '9') return false;
        x = x * 10 + (uint64_t)(c - '0');
    }
    *v = x;
    return true;
}

// CIGAR [a, b), not '*': false when malformed, else the soft-clipped lead and the query length
template <typename Get>
SAM_HD inline bool sam_cigar(Get get, uint32_t a, uint32_t b, uint64_t* lead, uint64_t* qlen) {
    *lead = 0; *qlen = 0;
    if (b <= a) return false;
    int phase = 0;                                    // 0: leading H, 1: leading S, 2: behind them
    uint32_t p = a;
    while (p < b) {
        uint64_t n = 0;
        uint32_t digits = 0;
        while (p < b && get(p) >= '0' && get(p) <= '9') { n = n * 10 + (uint64_t)(get(p) - '0'); ++p; ++digits; }
        if (digits < 1 || digits > 9 || p >= b) return false;
        const unsigned char op = get(p++);
        switch (op) {
            case 'M': case 'I': case '=': case 'X': *qlen += n; phase = 2; break;
            case 'S': *qlen += n; if (phase < 2) { *lead += n; phase = 1; } break;
            case 'H': if (phase) phase = 2; break;
            case 'D': case 'N': case 'P': phase = 2; break;
            default: return false;
        }
    }
    return true;
}

// the end of the line that ends in front of the '\n' at nl: one '\r' less
template <typename Get>
SAM_HD inline uint32_t sam_line_end(Get get, uint32_t s, uint32_t nl) { return (nl > s && get(nl - 1) == '\r') ? nl - 1 : nl; }

// tab[i] = the i-th tab of the line [s, e), kSamNone behind the last (what samtext.hip gets from its scans)
template <typename Get>
SAM_HD inline void sam_find_tabs(Get get, uint32_t s, uint32_t e, uint32_t* tab) {
    uint32_t n = 0;
    for (uint32_t p = s; p < e && n < kSamTabs; ++p)
        if (get(p) == '\t') tab[n++] = p;
    for (; n < kSamTabs; ++n) tab[n] = kSamNone;
}

// The line [s, e) with its first ten tabs.  lookup(a, len) -> the index of the name at [a, a + len), or kSamNone.
template <typename Get, typename Lookup>
SAM_HD inline SamLine sam_parse_line(Get get, uint32_t s, uint32_t e, const uint32_t* tab, bool paired, Lookup lookup) {
    SamLine r = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (e > s && get(s) == '@') { r.header = 1; return r; }
    if (tab[kSamTabs - 1] == kSamNone) { r.bad = SFGPU_SAM_BAD_FIELDS; return r; }
    r.q_len = tab[0] - s;
    uint64_t flag = 0;
    if (!sam_number(get, tab[0] + 1, tab[1], 5, &flag) || flag > 65535) { r.bad = SFGPU_SAM_BAD_NUMBER; return r; }
    uint32_t bad = 0;
    const bool first = (flag & 0x40) != 0, second = (flag & 0x80) != 0;
    if (paired ? (!(flag & 0x1) || first == second) : (flag & 0x1) != 0) bad |= SFGPU_SAM_BAD_FLAG;
    r.side = paired ? (first ? 1 : 2) : 0;
    r.fwd = (flag & 0x10) ? 0 : 1;
    r.mapped = (flag & (0x4 | 0x800)) ? 0 : 1;
    if (r.mapped) {
        uint64_t pos1 = 0, lead = 0, qlen = 0;
        if (!sam_number(get, tab[2] + 1, tab[3], 10, &pos1) || pos1 < 1 || pos1 > 0x7fffffffull) bad |= SFGPU_SAM_BAD_NUMBER;
        r.tid = lookup(tab[1] + 1, tab[2] - tab[1] - 1);
        if (r.tid == kSamNone) bad |= SFGPU_SAM_BAD_RNAME;
        const uint32_t c0 = tab[4] + 1, c1 = tab[5], q0 = tab[8] + 1, q1 = tab[9];
        const bool has_cigar = !(c1 - c0 == 1 && get(c0) == '*'), has_seq = !(q1 - q0 == 1 && get(q0) == '*');
        if (has_cigar && !sam_cigar(get, c0, c1, &lead, &qlen)) bad |= SFGPU_SAM_BAD_CIGAR;
        else {
            const uint64_t len = has_seq ? (uint64_t)(q1 - q0) : qlen;      // (CIGAR '*': qlen = 0)
            if (len > 65535 || (has_seq && has_cigar && len != qlen)) bad |= SFGPU_SAM_BAD_LENGTH;
            r.read_len = (uint16_t)len;
        }
        r.pos = (int32_t)((int64_t)pos1 - 1 - (int64_t)lead);
    }
    r.bad = bad & (0u - bad);                         // the first rule in the order of the bits
    return r;
}

// is line b, which directly follows line a in a's group, the mate that makes a pair with it?
SAM_HD inline bool sam_pairs_with(const SamLine& a, const SamLine& b) {
    return a.mapped && b.mapped && a.side == 1 && b.side == 2 && a.tid == b.tid;
}

SAM_HD inline sfgpu_hit sam_pair_hit(const SamLine& a, const SamLine& b) {
    sfgpu_hit h;
    h.tid = a.tid; h.pos = a.pos; h.mate_pos = b.pos;
    const int64_t lo = a.pos < b.pos ? a.pos : b.pos;
    const int64_t ea = (int64_t)a.pos + a.read_len, eb = (int64_t)b.pos + b.read_len;
    h.frag_len = (uint32_t)((ea > eb ? ea : eb) - lo);
    h.read_len = a.read_len; h.mate_len = b.read_len;
    h.fwd = a.fwd; h.mate_fwd = b.fwd; h.mate_status = 3; h.pad_ = 0;
    return h;
}

// an orphan (status = the line's side) or a single-end record (side 0)
SAM_HD inline sfgpu_hit sam_single_hit(const SamLine& a) {
    sfgpu_hit h;
    h.tid = a.tid; h.pos = a.pos; h.mate_pos = 0; h.frag_len = 0;
    h.read_len = a.read_len; h.mate_len = 0;
    h.fwd = a.fwd; h.mate_fwd = 0; h.mate_status = a.side; h.pad_ = 0;
    return h;
}

// the order of the records: a stable sort by this key (pairs: right = false)
SAM_HD inline uint64_t sam_sort_key(uint32_t group, bool right, uint32_t tid) {
    return ((uint64_t)group << 33) | ((uint64_t)(right ? 1 : 0) << 32) | tid;
}

}  // namespace sfgpu

#ifdef SAMFMT_SERIAL
#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace sfgpu {

// The whole reader, serially, with the calling conventions of sfgpu_sam_parse_*: add() looks at the complete lines of the text,
// holds the last group of a text that is not final back, and returns what the caller may drop.
struct SamSerial {
    bool paired;
    std::map<std::string, uint32_t> tid_of;
    std::vector<sfgpu_hit> hits;
    std::vector<uint32_t> offsets{0};
    uint64_t n_lines = 0, n_header = 0, n_pairs = 0;
    uint32_t bad = 0;
    uint64_t bad_line = 0;                            // (index in the whole input)

    SamSerial(bool paired_, const std::vector<std::string>& names) : paired(paired_) {
        for (size_t i = 0; i < names.size(); ++i) tid_of.emplace(names[i], (uint32_t)i);
    }

    uint64_t add(const unsigned char* text, uint64_t n, bool final) {
        if (bad) return 0;
        auto get = [text](uint32_t p) { return text[p]; };
        auto lookup = [&](uint32_t a, uint32_t len) {
            auto it = tid_of.find(std::string(reinterpret_cast<const char*>(text) + a, len));
            return it == tid_of.end() ? kSamNone : it->second;
        };
        struct Rec { SamLine l; uint32_t s; uint64_t line; };
        std::vector<Rec> recs;                        // the non-header lines
        std::vector<uint32_t> starts;                 // of every line looked at
        uint64_t at = 0;
        while (at < n) {
            uint64_t nl = at;
            while (nl < n && text[nl] != '\n') ++nl;
            if (nl == n && !final) break;
            const uint32_t s = (uint32_t)at, e = sam_line_end(get, s, (uint32_t)nl);      // (a last line without '\n' loses its '\r' too)
            uint32_t tab[kSamTabs];
            sam_find_tabs(get, s, e, tab);
            const SamLine l = sam_parse_line(get, s, e, tab, paired, lookup);
            if (l.bad) { bad = l.bad; bad_line = n_lines + starts.size(); return 0; }
            if (!l.header) recs.push_back(Rec{l, s, (uint64_t)starts.size()});
            starts.push_back(s);
            at = nl < n ? nl + 1 : n;
        }
        auto same_name = [&](const Rec& a, const Rec& b) {
            return a.l.q_len == b.l.q_len && std::equal(text + a.s, text + a.s + a.l.q_len, text + b.s);
        };
        size_t k_end = recs.size();                   // records of whole groups
        uint64_t lines_used = starts.size(), consumed = at;
        if (!final && !recs.empty()) {
            size_t k = recs.size() - 1;
            while (k > 0 && same_name(recs[k - 1], recs[k])) --k;
            k_end = k; lines_used = recs[k].line; consumed = recs[k].s;
        }
        for (size_t a = 0; a < k_end;) {
            size_t b = a + 1;
            while (b < k_end && same_name(recs[b - 1], recs[b])) ++b;
            std::vector<std::pair<uint64_t, sfgpu_hit>> out;
            for (size_t i = a; i + 1 < b; ++i)
                if (paired && sam_pairs_with(recs[i].l, recs[i + 1].l))
                    out.emplace_back(sam_sort_key(0, false, recs[i].l.tid), sam_pair_hit(recs[i].l, recs[i + 1].l));
            n_pairs += out.size();
            if (out.empty())
                for (size_t i = a; i < b; ++i)
                    if (recs[i].l.mapped) out.emplace_back(sam_sort_key(0, recs[i].l.side == 2, recs[i].l.tid), sam_single_hit(recs[i].l));
            std::stable_sort(out.begin(), out.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
            for (auto& o : out) hits.push_back(o.second);
            offsets.push_back((uint32_t)hits.size());
            a = b;
        }
        n_lines += lines_used;
        n_header += lines_used - k_end;
        return consumed;
    }
};

}  // namespace sfgpu
#endif
