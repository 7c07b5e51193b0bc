// samcfmt.h -- what a SAM text or BAM stream says to this library when its lines stand in ANY order (a position-sorted file, what
// `samtools sort` leaves): the collated reading, stated once: the rules samfile.read_sam_collated_host / read_bam_collated_host set.
// Plain C++, host and device, serial, on top of samfmt.h / bamfmt.h: sam_parse_line, bam_parse_record, SamLine, sam_pair_hit,
// sam_single_hit and sam_sort_key are theirs, unchanged.  samcollate.hip runs these functions inside its kernels,
// tests/samcollate_harness.cpp runs them alone (SamcSerial below).
//
// The rules are samfmt.h's but for these:
// Lines   as there (header lines anywhere, "\r\n", a last line without '\n', the kinds and their order).
// Mate fields (paired call, mapped line): RNEXT (field 7) and PNEXT (field 8) are read too.  PNEXT must be 1-10 digits, 0 .. 2^31 - 1
//         (BAD_NUMBER).  The line NAMES A MATE iff FLAG lacks 0x8, RNEXT is "=" or byte-equal to RNAME, and PNEXT >= 1.  A single-end
//         call, and an unmapped line, does not look at them.
// QNAME   longer than 254 bytes (the specification's limit, and what bounds the rounds of the name sort): BAD_QNAME, the last in the
//         order of the bits; every non-header line with its 11 fields and a readable FLAG is tested.  The name-grouped readers never
//         raise it.
// Fragments   ALL non-header lines of the file with byte-equal QNAME are one fragment, wherever they stand; fragments are numbered in
//         the order of their first lines, inside a fragment the lines keep file order.
// Pairs (paired call)   lines a and b of one fragment, both mapped, on one transcript, both naming a mate, a of side 1 and b of side
//         2, a.PNEXT == b.POS and b.PNEXT == a.POS: the WRITTEN 1-based POS, not pos behind the soft-clip adjustment.  The key of such
//         a line is (tid, POS of mate 1, POS of mate 2): (tid, POS, PNEXT) for a side-1 line, (tid, PNEXT, POS) for a side-2 line.
//         Among the lines of a fragment with one key the i-th side-1 line in file order pairs with the i-th side-2 line in file
//         order; what is left over pairs with nothing.  The record is sam_pair_hit(a, b).
// A fragment with a pair yields its pairs only; otherwise every mapped line is an orphan (single-end call: a status-0 record).  The
// order is samfmt.h's: left orphans, right orphans; within a side and among pairs or single-end records tid ascending, ties in file
// order (a pair stands where its side-1 line stands).  Unmapped (0x4) and 0x800 lines belong to their fragment and yield nothing; a
// fragment without records is still a read.
// BAM: the same with the syntax taken away.  A record names a mate iff FLAG lacks 0x8, next_refID == refID and next_pos >= 0; POS and
// PNEXT are pos + 1 and next_pos + 1; l_read_name bounds the name, BAD_QNAME cannot occur.
#pragma once
#include "bamfmt.h"

namespace sfgpu {

constexpr uint32_t kSamcMaxQname = 254;

// what the collated reading adds to a SamLine
struct SamMate {
    uint32_t bad;        // 0, or the SFGPU_SAM_BAD_* bits this reading adds (samc_first_bad joins them with the line's own)
    uint32_t pos1;       // the written POS of a mapped line
    uint32_t pnext;      // PNEXT when the line names a mate, else 0
};

// the first broken rule in the order of the bits: l.bad is one bit already
SAM_HD inline uint32_t samc_first_bad(const SamLine& l, const SamMate& m) {
    const uint32_t b = l.bad | m.bad;
    return b & (0u - b);
}

// l = sam_parse_line of the line at s with these tabs
template <typename Get>
SAM_HD inline SamMate samc_line_mate(Get get, uint32_t s, const uint32_t* tab, bool paired, const SamLine& l) {
    (void)s;
    SamMate m = {0, 0, 0};
    uint64_t flag = 0, v = 0;
    if (l.header || l.bad == SFGPU_SAM_BAD_FIELDS || !sam_number(get, tab[0] + 1, tab[1], 5, &flag) || flag > 65535) return m;
    if (l.q_len > kSamcMaxQname) m.bad |= SFGPU_SAM_BAD_QNAME;
    if (!l.mapped) return m;
    if (sam_number(get, tab[2] + 1, tab[3], 10, &v) && v >= 1 && v <= 0x7fffffffull) m.pos1 = (uint32_t)v;      // (else the line is BAD_NUMBER)
    if (!paired) return m;
    if (!sam_number(get, tab[6] + 1, tab[7], 10, &v) || v > 0x7fffffffull) { m.bad |= SFGPU_SAM_BAD_NUMBER; return m; }
    const uint32_t r0 = tab[1] + 1, rn = tab[2] - r0, x0 = tab[5] + 1, xn = tab[6] - x0;
    bool same = xn == 1 && get(x0) == '=';
    if (!same && xn == rn) {
        same = true;
        for (uint32_t i = 0; same && i < rn; ++i) same = get(x0 + i) == get(r0 + i);
    }
    if (!(flag & 0x8) && same && v >= 1) m.pnext = (uint32_t)v;
    return m;
}

// l = bam_parse_record of the record at p.  next_pos = 2^31 - 1 names POS 2^31, which no mapped record has: stored as "no mate",
// which pairs with the same lines.
template <typename Get>
SAM_HD inline SamMate samc_record_mate(Get get, uint32_t p, bool paired, const SamLine& l) {
    SamMate m = {0, 0, 0};
    if (l.bad == SFGPU_SAM_BAD_FIELDS || !l.mapped) return m;
    const int32_t ref = (int32_t)bam_u32(get, p + 4), pos0 = (int32_t)bam_u32(get, p + 8);
    if (pos0 >= 0 && pos0 != 0x7fffffff) m.pos1 = (uint32_t)pos0 + 1;
    if (!paired) return m;
    const uint32_t flag = bam_u16(get, p + 18);
    const int32_t nref = (int32_t)bam_u32(get, p + 24), npos = (int32_t)bam_u32(get, p + 28);
    if (!(flag & 0x8) && nref == ref && npos >= 0 && npos != 0x7fffffff) m.pnext = (uint32_t)npos + 1;
    return m;
}

// do lines a and b of one fragment make a pair?  (which of several candidates pairs with which is the i-th / i-th rule)
SAM_HD inline bool samc_pairs_with(const SamLine& a, const SamMate& ma, const SamLine& b, const SamMate& mb) {
    return a.mapped && b.mapped && a.side == 1 && b.side == 2 && a.tid == b.tid && ma.pnext && mb.pnext && ma.pnext == mb.pos1 &&
           mb.pnext == ma.pos1;
}

// the key of a line that names a mate, without its tid: POS of mate 1 << 32 | POS of mate 2
SAM_HD inline uint64_t samc_pos_key(uint32_t side, uint32_t pos1, uint32_t pnext) {
    return side == 1 ? ((uint64_t)pos1 << 32 | pnext) : ((uint64_t)pnext << 32 | pos1);
}

}  // namespace sfgpu

#ifdef SAMCFMT_SERIAL
#include <algorithm>
#include <map>
#include <string>
#include <tuple>
#include <vector>

namespace sfgpu {

// The whole collated reader, serially, with the calling conventions of sfgpu_sam_collect_* / sfgpu_samc_finish: add() takes the
// complete lines of a text and returns what the caller may drop (nothing is held back); finish() groups, pairs and orders.
struct SamcSerial {
    struct Rec { SamLine l; SamMate m; std::string name; };
    bool paired;
    std::map<std::string, uint32_t> tid_of;
    std::vector<Rec> recs;                            // the non-header lines of the file
    std::vector<sfgpu_hit> hits;
    std::vector<uint32_t> offsets{0};
    uint64_t n_lines = 0, n_header = 0, n_pairs = 0;
    uint32_t bad = 0;
    uint64_t bad_line = 0;                            // (index in the whole input)

    SamcSerial(bool paired_, const std::vector<std::string>& names) : paired(paired_) {
        for (size_t i = 0; i < names.size(); ++i) tid_of.emplace(names[i], (uint32_t)i);
    }

    uint64_t add(const unsigned char* text, uint64_t n, bool final) {
        if (bad) return 0;
        auto get = [text](uint32_t p) { return text[p]; };
        auto lookup = [&](uint32_t a, uint32_t len) {
            auto it = tid_of.find(std::string(reinterpret_cast<const char*>(text) + a, len));
            return it == tid_of.end() ? kSamNone : it->second;
        };
        std::vector<Rec> fresh;                       // nothing of a call with a malformed line is appended
        uint64_t at = 0, lines = 0;
        while (at < n) {
            uint64_t nl = at;
            while (nl < n && text[nl] != '\n') ++nl;
            if (nl == n && !final) break;
            const uint32_t s = (uint32_t)at, e = sam_line_end(get, s, (uint32_t)nl);
            uint32_t tab[kSamTabs];
            sam_find_tabs(get, s, e, tab);
            const SamLine l = sam_parse_line(get, s, e, tab, paired, lookup);
            const SamMate m = samc_line_mate(get, s, tab, paired, l);
            if (const uint32_t b = samc_first_bad(l, m)) { bad = b; bad_line = n_lines + lines; return 0; }
            if (!l.header) fresh.push_back(Rec{l, m, std::string(reinterpret_cast<const char*>(text) + s, l.q_len)});
            ++lines;
            at = nl < n ? nl + 1 : n;
        }
        n_lines += lines;
        n_header += lines - fresh.size();
        for (Rec& r : fresh) recs.push_back(std::move(r));
        return at;
    }

    void finish() {
        std::map<std::string, uint32_t> frag_of;
        std::vector<std::vector<uint32_t>> frags;     // the lines of each fragment, in file order
        for (uint32_t i = 0; i < recs.size(); ++i) {
            auto it = frag_of.emplace(recs[i].name, (uint32_t)frags.size());
            if (it.second) frags.emplace_back();
            frags[it.first->second].push_back(i);
        }
        for (const std::vector<uint32_t>& f : frags) {
            std::map<std::tuple<uint32_t, uint64_t>, std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> by_key;
            if (paired)
                for (uint32_t i : f) {
                    const Rec& r = recs[i];
                    if (!r.l.mapped || !r.m.pnext) continue;
                    auto& both = by_key[std::make_tuple(r.l.tid, samc_pos_key(r.l.side, r.m.pos1, r.m.pnext))];
                    (r.l.side == 1 ? both.first : both.second).push_back(i);
                }
            std::vector<std::tuple<uint64_t, uint32_t, sfgpu_hit>> out;      // (sort key, the line that places the record, the record)
            for (const auto& kv : by_key) {
                const auto& both = kv.second;
                for (size_t i = 0; i < both.first.size() && i < both.second.size(); ++i) {
                    const Rec &a = recs[both.first[i]], &b = recs[both.second[i]];
                    if (samc_pairs_with(a.l, a.m, b.l, b.m))      // (true by the key)
                        out.emplace_back(sam_sort_key(0, false, a.l.tid), both.first[i], sam_pair_hit(a.l, b.l));
                }
            }
            n_pairs += out.size();
            if (out.empty())
                for (uint32_t i : f)
                    if (recs[i].l.mapped) out.emplace_back(sam_sort_key(0, recs[i].l.side == 2, recs[i].l.tid), i, sam_single_hit(recs[i].l));
            std::sort(out.begin(), out.end(), [](const auto& x, const auto& y) {
                return std::make_pair(std::get<0>(x), std::get<1>(x)) < std::make_pair(std::get<0>(y), std::get<1>(y));
            });
            for (const auto& o : out) hits.push_back(std::get<2>(o));
            offsets.push_back((uint32_t)hits.size());
        }
    }
};

}  // namespace sfgpu
#endif
