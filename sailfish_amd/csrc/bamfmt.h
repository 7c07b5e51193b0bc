// bamfmt.h -- what a mapper's BAM stream (the bytes behind the BGZF inflate) says to this library, stated once: the rules
// samfile.read_bam_host sets.  Plain C++, host and device, serial.  It is to BAM what samfmt.h is to SAM and reuses its SamLine,
// sam_pairs_with, sam_pair_hit, sam_single_hit and sam_sort_key: groups, pairs and the record order are samfmt.h's.  bamtext.hip
// runs these functions inside its kernels, tests/bam_harness.cpp runs them alone (BamSerial below, and the tile functions).
//
// The stream (all integers little-endian and unaligned): "BAM\1", l_text, the text, n_ref, per reference l_name, the name with
// its NUL, l_ref: the header, header_bytes long.  Then records: block_size, refID, pos, l_read_name (u8), mapq, bin, n_cigar_op
// (u16), flag (u16), l_seq (u32), next_refID, next_pos, tlen; the name, n_cigar_op words len << 4 | op, (l_seq + 1) / 2 bytes of
// SEQ, l_seq bytes of QUAL, tags up to 4 + block_size.  block_size, refID, pos, l_read_name, n_cigar_op, flag, l_seq, the name and
// the CIGAR words are read; nobody walks SEQ, QUAL or the tags.
//
// The chain: a record at p is followed by one at p + 4 + block_size(p).  A position whose block_size (as int32) is below 32 ends
// the chain as BROKEN: BAD_FIELDS at that record.  A position with fewer than 4 bytes left, or whose record ends behind the text,
// ends it as INCOMPLETE: in a text that is not final that record and everything behind it is not looked at, in a final text it
// is BAD_FIELDS.  A chain that arrives at the text's end exactly has ended well.
// A record (whole in the text) says, the first broken rule in the order of the SFGPU_SAM_BAD_* bits:
//   FIELDS  block_size < 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq (in 64 bits), l_read_name == 0, or the name's
//           last byte is not NUL.  The other bytes of the name are not looked at.  QNAME = the name without its NUL.
//   FLAG    as in SAM.  0x4 or 0x800: the record yields nothing but belongs to its group.
//   mapped record: pos in 0 .. 2^31 - 2 (NUMBER: POS = pos + 1 is SAM's); refID in 0 .. n_ref - 1 and its reference one of the
//           handle's names (RNAME); every op code <= 8, MIDNSHP=X (CIGAR; n_cigar_op == 0 is SAM's '*', a length of 0 is legal, the
//           kSmN placeholder of a long CIGAR is taken as it stands); l_seq == 0 is SEQ '*'; read_len = l_seq, or qlen without SEQ;
//           above 65535, or SEQ and CIGAR both there and l_seq != qlen: LENGTH.  pos = the pos field - the leading soft clip.
// A call: the text begins at stream offset = the sum of the `consumed` values returned so far; max(0, header_bytes - that sum)
// bytes are skipped.  The last group of a text that is not final is held back, and such a call that emits no group consumes
// nothing ("present more").
#pragma once
#include "samfmt.h"

namespace sfgpu {

constexpr uint32_t kBamMin = 36;                         // the shortest record: block_size and the 32 fixed bytes
// A chain value is a position (<= 2^30: the text of a call), or how the chain ended and where (q < 2^30).
constexpr uint32_t kBamBroken = 0x80000000u, kBamIncomplete = 0xc0000000u, kBamAt = 0x3fffffffu;
SAM_HD inline bool bam_ended(uint32_t v) { return (v & 0x80000000u) != 0; }
SAM_HD inline bool bam_broken(uint32_t v) { return (v & 0xc0000000u) == kBamBroken; }

template <typename Get>
SAM_HD inline uint32_t bam_u16(Get get, uint32_t p) { return (uint32_t)get(p) | (uint32_t)get(p + 1) << 8; }
template <typename Get>
SAM_HD inline uint32_t bam_u32(Get get, uint32_t p) {
    return (uint32_t)get(p) | (uint32_t)get(p + 1) << 8 | (uint32_t)get(p + 2) << 16 | (uint32_t)get(p + 3) << 24;
}

// one link of the chain: the value behind position p < n of a text of n bytes
template <typename Get>
SAM_HD inline uint32_t bam_next(Get get, uint32_t p, uint32_t n) {
    if (n - p < 4) return kBamIncomplete | p;
    const int32_t bs = (int32_t)bam_u32(get, p);
    if (bs < 32) return kBamBroken | p;
    if ((uint64_t)p + 4 + (uint64_t)bs > n) return kBamIncomplete | p;
    return p + 4 + (uint32_t)bs;
}

// ---- the chain, tile by tile -----------------------------------------------------------------------------------------------
// A tile is T consecutive positions [base, base + T).  exit[p] of a position of the tile is the first chain value, on the chain
// that begins at p, that is no position of the tile: a position at or behind the tile's end (or n, in the last tile), or how the
// chain ended.  It is found for all T positions at once: nxt[] by bam_tile_nxt, then bam_tile_rounds<T>() rounds of
// bam_tile_double from one array into the other (a chain has at most ceil(T / 36) positions in a tile).

template <uint32_t T>
SAM_HD constexpr uint32_t bam_tile_rounds() {
    uint32_t r = 0;
    while ((kBamMin << r) < T) ++r;
    return r;
}
template <uint32_t T>
SAM_HD constexpr uint32_t bam_tile_records() { return (T + kBamMin - 1) / kBamMin; }      // the most record starts in one tile

// nxt of position base + i.  A position at or behind n (the last tile) stands for itself.
template <uint32_t T, typename Get>
SAM_HD inline uint32_t bam_tile_nxt(Get get, uint32_t base, uint32_t i, uint32_t n) {
    return base + i < n ? bam_next(get, base + i, n) : base + i;
}

// one round: the new value of entry i from the T values cur[]
template <uint32_t T>
SAM_HD inline uint32_t bam_tile_double(const uint32_t* cur, uint32_t base, uint32_t i) {
    const uint32_t v = cur[i];
    return (bam_ended(v) || v - base >= T) ? v : cur[v - base];
}

// The record starts of the tile on the chain that enters it at `entry` (a chain value; no position of this tile: none):
// out[0 .. count), count <= bam_tile_records<T>(); *leave = the chain value behind them.  A position that ends the chain is no start.
template <uint32_t T, typename Get>
SAM_HD inline uint32_t bam_tile_starts(Get get, uint32_t base, uint32_t entry, uint32_t n, uint32_t* out, uint32_t* leave) {
    uint32_t count = 0, p = entry;
    while (!bam_ended(p) && p < n && p - base < T) {
        const uint32_t v = bam_next(get, p, n);
        if (!bam_ended(v)) out[count++] = p;
        p = v;
    }
    *leave = p;
    return count;
}

// From chain value v through the exit table (exit_at(p) = exit[p]) to the first value that is no position below `end`: every hop
// leaves a tile, so there are at most (end - v) / T + 1 of them.
template <typename Exit>
SAM_HD inline uint32_t bam_follow(Exit exit_at, uint32_t v, uint32_t end, uint32_t n) {
    while (!bam_ended(v) && v < end && v < n) v = exit_at(v);
    return v;
}

// ---- what a record says ----------------------------------------------------------------------------------------------------

// The record at p, whole in the text (bam_next(p) is a position).  ref_tid(r) -> the transcript of reference r < n_ref, or kSamNone.
template <typename Get, typename RefTid>
SAM_HD inline SamLine bam_parse_record(Get get, uint32_t p, bool paired, uint32_t n_ref, RefTid ref_tid) {
    SamLine r = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t bs = bam_u32(get, p);                  // (>= 32 as int32)
    const int32_t ref = (int32_t)bam_u32(get, p + 4), pos0 = (int32_t)bam_u32(get, p + 8);
    const uint32_t l_name = get(p + 12), n_cigar = bam_u16(get, p + 16), flag = bam_u16(get, p + 18), l_seq = bam_u32(get, p + 20);
    const uint64_t need = 32ull + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + l_seq;
    if (bs < need || l_name == 0 || get(p + kBamMin + l_name - 1) != 0) { r.bad = SFGPU_SAM_BAD_FIELDS; return r; }
    r.q_len = l_name - 1;
    uint32_t bad = 0;
    const bool first = (flag & 0x40) != 0, second = (flag & 0x80) != 0;
    if (paired ? (!(flag & 0x1) || first == second) : (flag & 0x1) != 0) bad |= SFGPU_SAM_BAD_FLAG;
    r.side = paired ? (first ? 1 : 2) : 0;
    r.fwd = (flag & 0x10) ? 0 : 1;
    r.mapped = (flag & (0x4 | 0x800)) ? 0 : 1;
    if (r.mapped) {
        if (pos0 < 0 || pos0 == 0x7fffffff) bad |= SFGPU_SAM_BAD_NUMBER;
        r.tid = (ref >= 0 && (uint32_t)ref < n_ref) ? ref_tid((uint32_t)ref) : kSamNone;
        if (r.tid == kSamNone) bad |= SFGPU_SAM_BAD_RNAME;
        uint64_t lead = 0, qlen = 0;
        int phase = 0;                                    // 0: leading H, 1: leading S, 2: behind them (samfmt.h's sam_cigar)
        bool ok = true;
        const uint32_t c0 = p + kBamMin + l_name;
        for (uint32_t k = 0; k < n_cigar && ok; ++k) {
            const uint32_t w = bam_u32(get, c0 + 4 * k), len = w >> 4;
            switch (w & 15u) {
                case 0: case 1: case 7: case 8: qlen += len; phase = 2; break;              // M I = X
                case 4: qlen += len; if (phase < 2) { lead += len; phase = 1; } break;        // S
                case 5: if (phase) phase = 2; break;                                         // H
                case 2: case 3: case 6: phase = 2; break;                                    // D N P
                default: ok = false;
            }
        }
        if (!ok) bad |= SFGPU_SAM_BAD_CIGAR;
        else {
            const uint64_t len = l_seq ? (uint64_t)l_seq : qlen;
            if (len > 65535 || (l_seq && n_cigar && len != qlen)) bad |= SFGPU_SAM_BAD_LENGTH;
            r.read_len = (uint16_t)len;
        }
        r.pos = (int32_t)((int64_t)pos0 - (int64_t)lead);
    }
    r.bad = bad & (0u - bad);                             // the first rule in the order of the bits
    return r;
}

}  // namespace sfgpu

#ifdef BAMFMT_SERIAL
#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace sfgpu {

// the header of a stream that holds it whole: the reference names and header_bytes; false when it is not there
inline bool bam_header(const unsigned char* s, uint64_t n, std::vector<std::string>* refs, uint64_t* header_bytes) {
    auto u32 = [&](uint64_t p) { return (uint64_t)s[p] | (uint64_t)s[p + 1] << 8 | (uint64_t)s[p + 2] << 16 | (uint64_t)s[p + 3] << 24; };
    if (n < 12 || s[0] != 'B' || s[1] != 'A' || s[2] != 'M' || s[3] != 1) return false;
    uint64_t p = 8 + u32(4);
    if (p + 4 > n) return false;
    const uint64_t n_ref = u32(p);
    p += 4;
    for (uint64_t r = 0; r < n_ref; ++r) {
        if (p + 4 > n) return false;
        const uint64_t l = u32(p);
        if (l == 0 || p + 4 + l + 4 > n) return false;
        refs->emplace_back(reinterpret_cast<const char*>(s) + p + 4, l - 1);
        p += 4 + l + 4;
    }
    *header_bytes = p;
    return true;
}

// The whole reader, serially, with the calling conventions of sfgpu_bam_parse_*: a plain walk of the chain.
struct BamSerial {
    bool paired;
    std::vector<uint32_t> ref_tid;
    uint64_t header_bytes, stream_pos = 0;
    std::vector<sfgpu_hit> hits;
    std::vector<uint32_t> offsets{0};
    uint64_t n_lines = 0, n_pairs = 0;                    // (lines: the alignment records consumed)
    uint32_t bad = 0;
    uint64_t bad_line = 0;                                // (index among the records of the whole input)

    BamSerial(bool paired_, const std::vector<std::string>& names, const std::vector<std::string>& refs, uint64_t header_bytes_)
        : paired(paired_), header_bytes(header_bytes_) {
        std::map<std::string, uint32_t> tid_of;
        for (size_t i = 0; i < names.size(); ++i) tid_of.emplace(names[i], (uint32_t)i);
        for (const std::string& r : refs) {
            auto it = tid_of.find(r);
            ref_tid.push_back(it == tid_of.end() ? kSamNone : it->second);
        }
    }

    uint64_t add(const unsigned char* text, uint64_t n, bool final) {
        if (bad) return 0;
        const uint64_t skip = header_bytes > stream_pos ? header_bytes - stream_pos : 0;
        if (skip > n) { if (final) stream_pos += n; return final ? n : 0; }
        auto get = [text](uint32_t p) { return text[p]; };
        struct Rec { SamLine l; uint32_t s; };
        std::vector<Rec> recs;
        uint32_t p = (uint32_t)skip;
        while (p < n) {
            const uint32_t v = bam_next(get, p, (uint32_t)n);
            SamLine l = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (bam_ended(v)) {
                if (!bam_broken(v) && !final) break;
                l.bad = SFGPU_SAM_BAD_FIELDS;
            } else {
                l = bam_parse_record(get, p, paired, (uint32_t)ref_tid.size(), [&](uint32_t r) { return ref_tid[r]; });
            }
            if (l.bad) { bad = l.bad; bad_line = n_lines + recs.size(); return 0; }
            recs.push_back(Rec{l, p});
            p = v;
        }
        auto same_name = [&](const Rec& a, const Rec& b) {
            return a.l.q_len == b.l.q_len && std::equal(text + a.s + kBamMin, text + a.s + kBamMin + a.l.q_len, text + b.s + kBamMin);
        };
        size_t k_end = recs.size();                       // records of whole groups
        uint64_t consumed = n;
        if (!final) {
            if (recs.empty()) return 0;
            size_t k = recs.size() - 1;
            while (k > 0 && same_name(recs[k - 1], recs[k])) --k;
            if (k == 0) return 0;
            k_end = k; consumed = recs[k].s;
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
        n_lines += k_end;
        stream_pos += consumed;
        return consumed;
    }
};

}  // namespace sfgpu
#endif
