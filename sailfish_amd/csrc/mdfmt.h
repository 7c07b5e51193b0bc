// mdfmt.h -- the NM and MD tags of a mappings line, stated once.  Plain C++, host and device: mdtag.hip runs the lane functions
// below inside its kernels, tests/mdtag_harness.cpp runs them alone (md_serial), and hits.md_tags_host is the Python statement both
// are judged by.
//
// SLOT     two per record, aligngfmt.h's and samwfmt.h's: slot 2 h + which is line `which` of record h, and the line's mate, strand
//          and bases are verifyfmt.h's job `which` (vf_job; the mate's length from the reads' offsets).  A record's missing second
//          slot has nm = 0 and an empty MD.
// CIGAR    what the writer writes for the line: with an alignment the slot's words (len << 4 | op) and POS - 1 = aln_pos[slot];
//          without one <clip>S<match>M and POS from samw_aligned over the record's pos / read_len (mate_pos / mate_len on line 1).
//          A line the writer refuses -- no base on the transcript: samw_pos_ok fails, or the slot has no operation -- has no
//          operation here either: nm = 0 and MD "0".
// WALK     q = 0 (an index into the ORIENTED mate: reverse strand means reverse-complemented codes), x = POS - 1, run = 0.
//          S n: q += n.   I n: q += n, nm += n.   D n / N n: emit <run> ^ and the n reference characters; run = 0, nm += n, x += n.
//          M n / = n / X n: per column, a MISMATCH iff x is off the transcript (x < 0 or x >= tlen), or q is past the mate's bases,
//          or either vf_code is 4, or the codes differ (verifyfmt.h's comparison: N matches nothing): emit <run> and the reference
//          character, run = 0, nm += 1; a match: ++run; then ++q, ++x.   Other operations (H, P) move nothing.   At the end: emit <run>.
//          Every MD begins and ends with a number; a mismatch directly behind a deletion reads ^AC0T.
// REFCHAR  the transcript's byte, upper-cased if it is a .. z; anything that is then not A .. Z, and a position off the transcript,
//          is N.
// STATS    slots (those that are a line); sum_nm; md_bytes; max_md_bytes; slots_plain (the CIGAR is one M operation and nm is 0).
//
// The kernels do not walk an M run column by column: a lane takes kVfStep columns with verifyfmt.h's clipped 16-byte loads and
// turns them into a 16-bit mismatch mask (md_mask16); the matches behind a lane's last mismatch reach the next lane's first token
// through a segmented scan (md_seg / md_seg_join), and a lane names its own tokens from its mask (md_lane_tokens).  Both ways are
// stated here -- md_slot_serial and md_slot_lanes -- and the harness holds them against each other and against the statement.
// Operation lengths are 28 bits, so runs and nm fit 32.
#pragma once
#include "samwfmt.h"
#include "verifyfmt.h"

namespace sfgpu {

VF_HD uint8_t md_ref_char(uint8_t b) {
    if (b >= 'a' && b <= 'z') b = (uint8_t)(b - 32);
    return (b >= 'A' && b <= 'Z') ? b : (uint8_t)'N';
}
VF_HD uint8_t md_ref_at(const char* t, uint64_t tlen, int64_t x) { return (x < 0 || x >= (int64_t)tlen) ? (uint8_t)'N' : md_ref_char((uint8_t)t[x]); }

// CIGAR of a slot: n_ops words at ops, or (ops == nullptr) own0 and own1; x0 = POS - 1
struct MdCigar { const uint32_t* ops; uint32_t own0, own1; uint32_t n_ops; int64_t x0; };
VF_HD uint32_t md_op(const MdCigar& c, uint32_t i) { return c.ops ? c.ops[i] : (i ? c.own1 : c.own0); }
VF_HD MdCigar md_slot_cigar(const sfgpu_hit& h, uint32_t which, uint64_t slot, const int32_t* aln_pos, const uint64_t* aln_op_off, const uint32_t* aln_ops) {
    MdCigar c{nullptr, 0u, 0u, 0u, 0};
    if (aln_pos) {
        c.n_ops = (uint32_t)(aln_op_off[slot + 1] - aln_op_off[slot]);
        c.ops = c.n_ops ? aln_ops + aln_op_off[slot] : nullptr;
        c.x0 = aln_pos[slot];
        return c;
    }
    const int32_t pos = which ? h.mate_pos : h.pos;
    const uint32_t len = which ? h.mate_len : h.read_len;
    if (!samw_pos_ok(pos, len)) return c;
    uint32_t p, clip, match;
    samw_aligned(pos, len, &p, &clip, &match);
    c.x0 = (int64_t)p - 1;
    if (clip) { c.own0 = clip << 4 | 4u; c.own1 = match << 4; c.n_ops = 2u; }
    else { c.own0 = match << 4; c.n_ops = 1u; }
    return c;
}
VF_HD bool md_is_match_op(uint32_t op) { return op == 0u || op == 7u || op == 8u; }
VF_HD bool md_is_del_op(uint32_t op) { return op == 2u || op == 3u; }
VF_HD bool md_plain(const MdCigar& c, uint32_t nm) { return c.n_ops == 1u && (md_op(c, 0) & 15u) == 0u && nm == 0u; }

// ---- column by column -------------------------------------------------------------------------------------------------------------
// put(ch) takes the MD's bytes in order; -> nm
template <typename Put>
VF_HD uint32_t md_put_run(uint32_t run, Put& put) {
    char d[10];
    const int n = dec_put_u32(run, [&](int i, char ch) { d[i] = ch; });
    for (int i = n - 1; i >= 0; --i) put(d[i]);
    return (uint32_t)n;
}
template <typename Put>
VF_HD uint32_t md_slot_serial(const MdCigar& c, const char* r, uint64_t len, bool fwd, const char* t, uint64_t tlen, Put put) {
    uint64_t q = 0;
    int64_t x = c.x0;
    uint32_t run = 0, nm = 0;
    for (uint32_t i = 0; i < c.n_ops; ++i) {
        const uint32_t n = md_op(c, i) >> 4, op = md_op(c, i) & 15u;
        if (op == 4u) q += n;
        else if (op == 1u) { q += n; nm += n; }
        else if (md_is_del_op(op)) {
            md_put_run(run, put); put('^');
            for (uint32_t j = 0; j < n; ++j) put((char)md_ref_at(t, tlen, x + j));
            run = 0; nm += n; x += n;
        } else if (md_is_match_op(op)) {
            for (uint32_t j = 0; j < n; ++j, ++q, ++x) {
                bool mism = x < 0 || x >= (int64_t)tlen || q >= len;
                if (!mism) {
                    const uint32_t a = vf_oriented(vf_code((unsigned char)(fwd ? r[q] : r[len - 1 - q])), fwd), b = vf_code((unsigned char)t[x]);
                    mism = a > 3u || b > 3u || a != b;
                }
                if (mism) { md_put_run(run, put); put((char)md_ref_at(t, tlen, x)); run = 0; ++nm; }
                else ++run;
            }
        }
    }
    md_put_run(run, put);
    return nm;
}

// ---- sixteen columns at a time ----------------------------------------------------------------------------------------------------
// bit i: column i of the windows is a mismatch (the mate's window and the transcript's read 0 outside their texts, and 0 is no base)
VF_HD uint32_t md_mask16(VfWin m, VfWin t, bool fwd) {
    const uint32_t cx = fwd ? 0u : 0x15151515u, cm = fwd ? 0u : 0x11u;
    const uint32_t mw[4] = {(uint32_t)m.lo, (uint32_t)(m.lo >> 32), (uint32_t)m.hi, (uint32_t)(m.hi >> 32)};
    const uint32_t tw[4] = {(uint32_t)t.lo, (uint32_t)(t.lo >> 32), (uint32_t)t.hi, (uint32_t)(t.hi >> 32)};
    uint32_t mask = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k)                   // 0x80 of bytes 0 .. 3 -> bits 24 .. 27 (no two products meet: no carry)
        mask |= (((((vf_differ4(mw[k], tw[k], cx, cm) >> 7) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu) << (4 * k);
    return mask;
}
VF_HD uint8_t md_win_byte(VfWin w, uint32_t i) { return (uint8_t)((i < 8u ? w.lo >> (8u * i) : w.hi >> (8u * (i - 8u))) & 0xFFu); }
VF_HD uint32_t md_msb(uint32_t v) {               // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 31u - (uint32_t)__clz((int)v);
#else
    return 31u - (uint32_t)__builtin_clz(v);
#endif
}
VF_HD uint32_t md_lsb(uint32_t v) {               // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffs((int)v) - 1u;
#else
    return (uint32_t)__builtin_ctz(v);
#endif
}
// What a lane's n columns (mask within them) hand on: the matches behind its last mismatch, flagged kMdCut; without a mismatch all
// its n columns, to be added to what comes from the left.  md_seg_join(left, right) is associative with 0 as its identity.
constexpr uint32_t kMdCut = 0x80000000u;
VF_HD uint32_t md_seg(uint32_t mask, uint32_t n) { return mask ? (kMdCut | (n - 1u - md_msb(mask))) : n; }
VF_HD uint32_t md_seg_join(uint32_t left, uint32_t right) { return (right & kMdCut) ? right : left + right; }
// the run a segment hands on, given the run that entered the group's columns
VF_HD uint32_t md_seg_run(uint32_t seg, uint32_t run_in) { return (seg & kMdCut) ? (seg & ~kMdCut) : seg + run_in; }
// a lane's tokens in order: tok(run, reference character) per mismatch; carry = the run that reaches the lane's first column
template <typename Tok>
VF_HD void md_lane_tokens(uint32_t mask, uint32_t carry, VfWin t, Tok&& tok) {
    uint32_t before = 0;                          // columns in front of the next token's run
    while (mask) {
        const uint32_t p = md_lsb(mask);
        tok(carry + p - before, md_ref_char(md_win_byte(t, p)));
        carry = 0; before = p + 1u; mask &= mask - 1u;
    }
}
VF_HD uint32_t md_token_len(uint32_t run) { return (uint32_t)dec_len_u32(run) + 1u; }

#if !defined(__HIPCC__)
// ... and as a group of `lanes` lanes runs a slot: an M run in steps of lanes * kVfStep columns, the lanes' segments scanned, every
// token placed from its lane's offset.  out == nullptr only counts.  -> the MD's bytes; *nm_out the slot's nm
inline uint64_t md_slot_lanes(const MdCigar& c, const char* r, uint64_t len, bool fwd, const char* t, uint64_t tlen, uint32_t lanes, char* out, uint32_t* nm_out) {
    uint64_t q = 0, at = 0;
    int64_t x = c.x0;
    uint32_t run = 0, nm = 0;
    auto number = [&](uint64_t where, uint32_t v) {
        const int nd = dec_len_u32(v);
        if (out) dec_put_fixed_u32(v, nd, 0, [&](int i, char ch) { out[where + (uint64_t)(nd - 1 - i)] = ch; });
        return (uint32_t)nd;
    };
    for (uint32_t i = 0; i < c.n_ops; ++i) {
        const uint32_t n = md_op(c, i) >> 4, op = md_op(c, i) & 15u;
        if (op == 4u) q += n;
        else if (op == 1u) { q += n; nm += n; }
        else if (md_is_del_op(op)) {
            at += number(at, run);
            if (out) { out[at] = '^'; for (uint32_t j = 0; j < n; ++j) out[at + 1 + j] = (char)md_ref_at(t, tlen, x + j); }
            at += 1ull + n; run = 0; nm += n; x += n;
        } else if (md_is_match_op(op)) {
            for (uint64_t c0 = 0; c0 < n; c0 += (uint64_t)lanes * kVfStep) {
                std::vector<uint32_t> mask(lanes), seg(lanes), bytes(lanes);
                std::vector<VfWin> tw(lanes);
                for (uint32_t l = 0; l < lanes; ++l) {
                    const uint64_t c1 = c0 + (uint64_t)l * kVfStep;
                    const uint32_t cols = c1 >= n ? 0u : (n - c1 < kVfStep ? (uint32_t)(n - c1) : kVfStep);
                    tw[l] = vf_window(t, (int64_t)tlen, x + (int64_t)c1);
                    mask[l] = cols ? md_mask16(vf_mate_window(r, (int64_t)len, fwd, (int64_t)(q + c1)), tw[l], fwd) & ((1u << cols) - 1u) : 0u;
                    seg[l] = md_seg(mask[l], cols);
                }
                uint32_t left = 0;                                   // the exclusive scan of the segments
                uint64_t place = at;
                for (uint32_t l = 0; l < lanes; ++l) {
                    md_lane_tokens(mask[l], md_seg_run(left, run), tw[l], [&](uint32_t v, uint8_t ch) {
                        const uint32_t nd = number(place, v);
                        if (out) out[place + nd] = (char)ch;
                        place += nd + 1u; ++nm;
                    });
                    left = md_seg_join(left, seg[l]);
                }
                at = place; run = md_seg_run(left, run);
            }
            q += n; x += n;
        }
    }
    at += number(at, run);
    *nm_out = nm;
    return at;
}

// the whole pass, serially (lanes == 0: column by column; else as a group of `lanes` lanes).  aln_pos / aln_op_off / aln_ops: all
// three or none.  -> 0, or 1 + the lowest record with tid >= M (nothing is emitted then)
inline uint64_t md_serial(const VfBatch& b, const int32_t* aln_pos, const uint64_t* aln_op_off, const uint32_t* aln_ops, uint32_t lanes,
                          std::vector<uint32_t>* nm, std::vector<uint64_t>* md_off, std::vector<uint8_t>* md, sfgpu_mdtag_stats* stats) {
    if (const uint64_t bad = vf_bad_tid(b)) return bad;
    const uint64_t n = b.n_rec();
    *stats = sfgpu_mdtag_stats{};
    nm->assign(2 * n, 0u); md_off->assign(2 * n + 1, 0ull); md->clear();
    vf_each_job(b, [&](uint32_t, uint32_t i, uint32_t j, const char* mate, uint64_t len, const char* tx, uint64_t tl, bool fwd, int64_t) {
        const uint64_t s = 2ull * i + j;
        const MdCigar c = md_slot_cigar(b.hits[i], j, s, aln_pos, aln_op_off, aln_ops);
        uint32_t got = 0;
        std::vector<char> bytes;
        if (lanes) {
            bytes.resize(md_slot_lanes(c, mate, len, fwd, tx, tl, lanes, nullptr, &got));
            md_slot_lanes(c, mate, len, fwd, tx, tl, lanes, bytes.data(), &got);
        } else got = md_slot_serial(c, mate, len, fwd, tx, tl, [&](char ch) { bytes.push_back(ch); });
        (*nm)[s] = got; (*md_off)[s + 1] = bytes.size();
        md->insert(md->end(), bytes.begin(), bytes.end());
        ++stats->slots; stats->sum_nm += got; stats->md_bytes += bytes.size(); stats->slots_plain += md_plain(c, got);
        if (bytes.size() > stats->max_md_bytes) stats->max_md_bytes = bytes.size();
    });
    for (uint64_t s = 0; s < 2 * n; ++s) (*md_off)[s + 1] += (*md_off)[s];
    return 0;
}
#endif

}  // namespace sfgpu
