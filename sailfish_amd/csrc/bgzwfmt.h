// bgzwfmt.h -- the arithmetic of the device BGZF writer (bgzf_write.hip), usable from device code (hipcc) and from host code
// (g++: tests/bgzw_harness.cpp is this header as plain C++, and tests/test_bgzw_cpu.py lets Python's zlib and gzip judge it).
// CRC-32, the length symbols, the length-limited code builder, the run-length form of the code lengths and the bit writer are
// gzfmt.h's, unchanged; this header adds distances.
//
// The file: members of kBgzwPayload payload bytes each (a write's last member is short: a stream is cut at multiples of the
// payload within every write), then the 28-byte EOF member.  A member is the 18-byte BGZF header (1f 8b 08 04, MTIME 0, XFL 0,
// OS 0xff, XLEN 6, 'B' 'C' 2 0, BSIZE = member bytes - 1), ONE final DEFLATE block, CRC-32 and ISIZE.  The block is a dynamic-
// Huffman block over literals and (length, distance) matches, or -- where that would not be shorter -- one stored block, so
// that a member is never longer than its payload + kBgzwStoredOverhead bytes.
//
// The parse (a function of the member's bytes alone):
//   candidates   every position i with i + 4 <= n has the hash bgzw_hash of its four bytes.  The member is walked in steps of
//                kBgzwStep positions; cand(i) = the greatest position of the steps BEFORE i's step whose hash equals i's (none
//                where there is no such position, or where i + 4 > n).  A workgroup looks a step's positions up in a table of
//                "greatest position so far" and enters them with a maximum afterwards; bgzw_candidates is the plain loop.
//   tokens       the member is cut into slices of kBgzwSlice bytes, and the greedy parse restarts at every slice: a match
//                never runs past its slice's end (or the member's).  At a token start i three distances are tried: 1, the
//                distance of the slice's previous match, and i - cand(i); each is extended byte by byte to the slice's end.
//                The longest wins, the nearer one of two equally long; it becomes a match when it is >= 3 bytes long and not a
//                3-byte match further than kBgzwTooFar away (which would cost more bits than its literals), else byte i is a
//                literal.  bgzw_slice_tokens is that loop for one slice; a lane of the kernel owns one slice.
//   codes        two histograms (literal/length with the end-of-block symbol, distance), two length-limited codes
//                (huff_lengths_serial: a member with no match, or with one distance symbol, still carries a complete code, as
//                zlib writes it), the header with HLIT, HDIST and both length sequences run-length coded as one (RFC 1951 3.2.7).
// bgzw_encode_member_serial drives all of it with plain loops: the host encoder that the device bytes are compared with.
#pragma once
#include "gzfmt.h"

namespace sfgpu {

constexpr uint32_t kBgzwPayload = 32768;            // payload bytes per member (<= 65 280; see bgzf_write.hip for the LDS budget)
constexpr uint32_t kBgzwSlice = 64;                 // the greedy parse restarts here
constexpr uint32_t kBgzwStep = 256;                 // positions per step of the candidate table
constexpr int kBgzwHashBits = 13;
constexpr uint32_t kBgzwMaxDist = 32768;
constexpr uint32_t kBgzwTooFar = 4096;              // a 3-byte match beyond this distance is not taken
constexpr int kBgzwDistSyms = 30;
constexpr uint32_t kBgzwHeaderBytes = 18, kBgzwTrailerBytes = 8, kBgzwEofBytes = 28;
constexpr uint32_t kBgzwStoredOverhead = kBgzwHeaderBytes + 5 + kBgzwTrailerBytes;      // 31
constexpr uint32_t kBgzwMaxMember = kBgzwPayload + kBgzwStoredOverhead;
static_assert(kBgzwPayload <= 65280 && kBgzwPayload <= kGzStoredMax && kBgzwPayload % kBgzwSlice == 0 && kBgzwPayload % kBgzwStep == 0, "member cut");
static_assert(kBgzwPayload <= kBgzwMaxDist && kBgzwPayload <= 65535, "a position + 1 fits 16 bits and every earlier byte of a member is in the window");

// ---------------------------------------------------------------------------------------------------------------- distances
// distance 1 .. 32 768 -> symbol 0 .. 29; *eb extra bits holding *ev
SF_GZ_HD int bgzw_dist_symbol(uint32_t dist, int* eb, uint32_t* ev) {
    const uint32_t d = dist - 1u;
    if (d < 4u) { *eb = 0; *ev = 0; return (int)d; }
    int lg = 2;
    while ((d >> (lg + 1)) != 0u) ++lg;                  // floor(log2 d), 2 .. 14
    const int e = lg - 1;
    *eb = e; *ev = d & ((1u << e) - 1u);
    return 2 * lg + (int)((d >> e) & 1u);
}

SF_GZ_HD uint32_t bgzw_hash(uint32_t four_bytes_le) { return (four_bytes_le * 2654435761u) >> (32 - kBgzwHashBits); }

// cand[i] = candidate position + 1 of position i, 0 = none; table: 1 << kBgzwHashBits entries of scratch
inline void bgzw_candidates(const uint8_t* in, uint32_t n, uint16_t* cand, uint32_t* table) {
    for (uint32_t b = 0; b < (1u << kBgzwHashBits); ++b) table[b] = 0u;
    auto hash_at = [&](uint32_t i) {
        return bgzw_hash((uint32_t)in[i] | ((uint32_t)in[i + 1] << 8) | ((uint32_t)in[i + 2] << 16) | ((uint32_t)in[i + 3] << 24));
    };
    for (uint32_t s = 0; s < n; s += kBgzwStep) {
        const uint32_t e = n - s < kBgzwStep ? n : s + kBgzwStep;
        for (uint32_t i = s; i < e; ++i) cand[i] = i + 4u <= n ? (uint16_t)table[hash_at(i)] : (uint16_t)0;
        for (uint32_t i = s; i < e; ++i) if (i + 4u <= n) table[hash_at(i)] = i + 1u;       // ascending: the greatest stays
    }
}

// ---------------------------------------------------------------------------------------------------------------- tokens
// The tokens of the slice [c0, c1): emit(position, length, distance), length 1 = a literal (distance 0).  cand_at(i) is read
// before the token at i is emitted, and only at token starts (the kernel keeps its tokens where the candidates were).
template <typename ByteAt, typename CandAt, typename Emit>
SF_GZ_HD void bgzw_slice_tokens(ByteAt byte_at, CandAt cand_at, uint32_t c0, uint32_t c1, Emit emit) {
    uint32_t i = c0, prev = 0u;
    while (i < c1) {
        const uint32_t room = c1 - i < kGzMaxMatch ? c1 - i : kGzMaxMatch;
        const uint32_t c = cand_at(i);
        uint32_t best_len = 0u, best_d = 0u;
        auto consider = [&](uint32_t d) {
            if (d == 0u || d > i || d > kBgzwMaxDist || d == best_d) return;
            uint32_t l = 0u;
            while (l < room && byte_at(i + l) == byte_at(i + l - d)) ++l;
            if (l > best_len || (l == best_len && d < best_d)) { best_len = l; best_d = d; }
        };
        consider(1u);
        consider(prev);
        consider(c ? i + 1u - c : 0u);
        if (best_len >= kGzMinMatch && !(best_len == kGzMinMatch && best_d > kBgzwTooFar)) {
            emit(i, best_len, best_d);
            prev = best_d;
            i += best_len;
        } else {
            emit(i, 1u, 0u);
            ++i;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- framing
SF_GZ_HD void bgzw_member_header(uint32_t member_bytes, uint8_t* out) {
    const uint8_t h[kBgzwHeaderBytes] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0,
                                         (uint8_t)((member_bytes - 1u) & 0xffu), (uint8_t)((member_bytes - 1u) >> 8)};
    for (uint32_t i = 0; i < kBgzwHeaderBytes; ++i) out[i] = h[i];
}
SF_GZ_HD void bgzw_member_trailer(uint32_t crc, uint32_t n, uint8_t* out) {
    for (int i = 0; i < 4; ++i) { out[i] = (uint8_t)(crc >> (8 * i)); out[4 + i] = (uint8_t)(n >> (8 * i)); }
}
// the empty member that ends a file: a final fixed-Huffman block holding the end-of-block symbol alone (03 00)
SF_GZ_HD void bgzw_eof_member(uint8_t* out) {
    bgzw_member_header(kBgzwEofBytes, out);
    out[18] = 3; out[19] = 0;
    for (uint32_t i = 20; i < kBgzwEofBytes; ++i) out[i] = 0;
}

// The header of the FINAL dynamic block for the literal/length lengths `lens` and the distance lengths `dlens` (trailing zeros
// above symbol 0 are not sent), written from bit pos0 through or32: gzfmt.h's writer.  Returns its length in bits.
template <typename Or32>
SF_GZ_HD uint32_t bgzw_write_block_header(const uint8_t* lens, const uint8_t* dlens, GzClWork* w, uint64_t pos0, Or32 or32) {
    int n_dist = kBgzwDistSyms;
    while (n_dist > 1 && dlens[n_dist - 1] == 0) --n_dist;
    return gz_write_dyn_header(1u, pos0, lens, [&](int i) { return dlens[i]; }, n_dist, w, or32);
}

// bits of one token under the two codes
SF_GZ_HD uint32_t bgzw_token_bits(const uint8_t* lens, const uint8_t* dlens, uint32_t byte, uint32_t len, uint32_t dist) {
    if (len == 1u) return lens[byte];
    int eb, deb; uint32_t ev, dev_;
    const int sym = gz_len_symbol(len, &eb, &ev), dsym = bgzw_dist_symbol(dist, &deb, &dev_);
    return (uint32_t)lens[sym] + (uint32_t)eb + (uint32_t)dlens[dsym] + (uint32_t)deb;
}
// one token at bit `pos` through or32 (a match in three pieces of <= 25 bits: length code + extra, distance code, distance
// extra); returns the bits written
template <typename Or32>
SF_GZ_HD uint32_t bgzw_put_token(Or32 or32, uint64_t pos, const uint8_t* lens, const uint16_t* codes, const uint8_t* dlens,
                                 const uint16_t* dcodes, uint32_t byte, uint32_t len, uint32_t dist) {
    if (len == 1u) { gz_put_bits(or32, pos, codes[byte], lens[byte]); return lens[byte]; }
    int eb, deb; uint32_t ev, dev_;
    const int sym = gz_len_symbol(len, &eb, &ev), dsym = bgzw_dist_symbol(dist, &deb, &dev_);
    uint32_t bits = 0;
    gz_put_bits(or32, pos, (uint32_t)codes[sym] | (ev << lens[sym]), lens[sym] + eb);
    bits += (uint32_t)lens[sym] + (uint32_t)eb;
    gz_put_bits(or32, pos + bits, dcodes[dsym], dlens[dsym]);
    bits += dlens[dsym];
    if (deb) gz_put_bits(or32, pos + bits, dev_, deb);
    return bits + (uint32_t)deb;
}

// bytes of a member coded / stored, from the bits of block header, tokens and end-of-block symbol
SF_GZ_HD uint32_t bgzw_coded_bytes(uint32_t bits) { return kBgzwHeaderBytes + (bits + 7u) / 8u + kBgzwTrailerBytes; }
SF_GZ_HD uint32_t bgzw_stored_bytes(uint32_t n) { return n + kBgzwStoredOverhead; }
// the 5 bytes of the final stored block's header
SF_GZ_HD void bgzw_stored_header(uint32_t n, uint8_t* out) {
    out[0] = 1; out[1] = (uint8_t)(n & 0xffu); out[2] = (uint8_t)(n >> 8); out[3] = (uint8_t)(~n & 0xffu); out[4] = (uint8_t)((~n >> 8) & 0xffu);
}

// ---------------------------------------------------------------------------------------------------------------- serial driver
struct BgzwSerialWork {
    uint16_t cand[kBgzwPayload];
    uint32_t table[1u << kBgzwHashBits];
    uint32_t crc_table[256];
};
struct BgzwMemberInfo { uint32_t stored, n_matches, n_literals; };      // the token counts of a stored member are 0: none is emitted

// One member (1 <= n <= kBgzwPayload), serially, into `out` (room for kBgzwMaxMember + 8 bytes, zeroed by the callee).  Returns
// the member's bytes.  emit_token(position, length, distance), when given, sees every token of the parse.
template <typename EmitToken>
inline uint32_t bgzw_encode_member_serial(const uint8_t* in, uint32_t n, uint8_t* out, BgzwSerialWork* w, BgzwMemberInfo* info,
                                          EmitToken emit_token) {
    bgzw_candidates(in, n, w->cand, w->table);
    auto tokens = [&](auto emit) {
        for (uint32_t c0 = 0; c0 < n; c0 += kBgzwSlice)
            bgzw_slice_tokens([&](uint32_t i) { return in[i]; }, [&](uint32_t i) { return (uint32_t)w->cand[i]; }, c0,
                              n - c0 < kBgzwSlice ? n : c0 + kBgzwSlice, emit);
    };
    uint32_t freq[kGzLitSyms], dfreq[kBgzwDistSyms];
    for (int s = 0; s < kGzLitSyms; ++s) freq[s] = 0;
    for (int s = 0; s < kBgzwDistSyms; ++s) dfreq[s] = 0;
    uint32_t n_matches = 0, n_literals = 0;
    tokens([&](uint32_t i, uint32_t len, uint32_t dist) {
        emit_token(i, len, dist);
        ++freq[gz_token_symbol(in[i], len)];
        if (len > 1u) { int eb; uint32_t ev; ++dfreq[bgzw_dist_symbol(dist, &eb, &ev)]; ++n_matches; } else ++n_literals;
    });
    freq[kGzEob] = 1;
    uint8_t lens[kGzLitSyms], dlens[kBgzwDistSyms];
    uint16_t codes[kGzLitSyms], dcodes[kBgzwDistSyms], order[kGzLitSyms], parent[2 * kGzLitSyms];
    uint32_t node_freq[2 * kGzLitSyms], count[kGzMaxBits + 1];
    GzClWork clw;
    huff_lengths_serial(freq, kGzLitSyms, kGzMaxBits, lens, order, parent, node_freq, count);
    for (int s = 0; s < kGzLitSyms; ++s) codes[s] = (uint16_t)huff_code_rev(lens, kGzLitSyms, s);
    huff_lengths_serial(dfreq, kBgzwDistSyms, kGzMaxBits, dlens, order, parent, node_freq, count);
    for (int s = 0; s < kBgzwDistSyms; ++s) dcodes[s] = (uint16_t)huff_code_rev(dlens, kBgzwDistSyms, s);
    const uint32_t cap = kBgzwMaxMember + 8u;
    for (uint32_t i = 0; i < cap; ++i) out[i] = 0;
    auto or32 = [&](uint32_t word, uint32_t bits) {
        for (int b = 0; b < 4; ++b) {
            const uint32_t at = 4u * word + (uint32_t)b;
            if (at < cap) out[at] |= (uint8_t)(bits >> (8 * b));
        }
    };
    uint64_t pos = 8ull * kBgzwHeaderBytes;
    const uint32_t hdr = bgzw_write_block_header(lens, dlens, &clw, pos, or32);
    uint32_t body = 0;
    tokens([&](uint32_t i, uint32_t len, uint32_t dist) { body += bgzw_token_bits(lens, dlens, in[i], len, dist); });
    const uint32_t coded = bgzw_coded_bytes(hdr + body + lens[kGzEob]), raw = bgzw_stored_bytes(n);
    for (uint32_t i = 0; i < 256; ++i) w->crc_table[i] = crc32_table_entry(i);
    const uint32_t crc = crc32_slice(0u, w->crc_table, [&](uint32_t i) { return in[i]; }, n);
    uint32_t total;
    if (coded < raw) {
        pos += hdr;
        tokens([&](uint32_t i, uint32_t len, uint32_t dist) { pos += bgzw_put_token(or32, pos, lens, codes, dlens, dcodes, in[i], len, dist); });
        gz_put_bits(or32, pos, codes[kGzEob], lens[kGzEob]);
        total = coded;
        info->stored = 0; info->n_matches = n_matches; info->n_literals = n_literals;
    } else {
        for (uint32_t i = 0; i < cap; ++i) out[i] = 0;
        bgzw_stored_header(n, out + kBgzwHeaderBytes);
        for (uint32_t i = 0; i < n; ++i) out[kBgzwHeaderBytes + 5u + i] = in[i];
        total = raw;
        info->stored = 1; info->n_matches = 0; info->n_literals = 0;
    }
    bgzw_member_header(total, out);
    bgzw_member_trailer(crc, n, out + total - kBgzwTrailerBytes);
    return total;
}

}  // namespace sfgpu
