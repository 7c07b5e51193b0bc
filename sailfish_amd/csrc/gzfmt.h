// gzfmt.h -- the arithmetic of the device gzip writer (gzwrite.hip), usable from device code (hipcc) and from host code (g++:
// tests/gzwrite_harness.cpp is this header as plain C++, and tests/test_gzwrite_cpu.py lets Python's zlib judge it).
//
// The stream (RFC 1952 around RFC 1951): a 10-byte header, DEFLATE blocks, CRC-32 and ISIZE.  The payload is cut into
// independent blocks of kGzBlockBytes.  A block is coded as ONE dynamic-Huffman block over literals and distance-1 run matches
// (length 3 .. 258, the token class of zlib's Z_RLE), followed by an empty stored block that pads it to a byte -- or, where
// that would not be shorter, as stored blocks.  Every block therefore begins and ends on a byte boundary, is never longer than
// its payload + kGzStoredOverhead bytes, and the blocks of a write can be coded in any order.
//
//   crc32_*          table entry, byte update, multiplication mod P, x^(8 n) mod P, combination of two CRCs (zlib's crc32_combine)
//   gz_len_symbol    match length -> length symbol, number and value of the extra bits
//   gz_run_len / gz_chunk_tokens   the greedy parse restated per position, so that a lane can find the tokens that START in its
//                    slice of the block from a bit mask of "equals the byte before"; gz_greedy_tokens is the plain loop
//   huff_*           length-limited code lengths from a histogram: order by (frequency, symbol), two-queue merge, leaf depths,
//                    depth counts forced to the limit by Kraft arithmetic, lengths handed out by rank; canonical codes
//   gz_cl_rle        the code-length sequence of a block header in symbols 0 .. 18 (16 / 17 / 18 are the repeats)
//   gz_write_dyn_header / gz_write_block_header / gz_header / gz_trailer / gz_stored_*   the framing (the dynamic block header is
//                    bgzwfmt.h's as well)
//   gz_encode_block_serial   all of it driven by a plain loop: the host encoder that the device stream is compared with
// Steps that the kernel runs one lane per item (rank, depth, length of rank, canonical code) are functions of one item here, so
// that the serial driver and the kernel call the same code.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SF_GZ_HD __host__ __device__ __forceinline__
#else
#define SF_GZ_HD inline
#endif

namespace sfgpu {

constexpr uint32_t kGzBlockBytes = 65536;       // payload bytes per independent block
constexpr uint32_t kGzStoredMax = 65535;        // LEN of a stored block is 16 bits
constexpr uint32_t kGzStoredOverhead = 10;      // a full block that does not compress is two stored blocks: 2 x 5 bytes
constexpr int kGzLitSyms = 286, kGzDistSyms = 2, kGzClSyms = 19;
constexpr int kGzMaxBits = 15, kGzMaxClBits = 7;
constexpr uint32_t kGzMinMatch = 3, kGzMaxMatch = 258;
constexpr int kGzEob = 256;
constexpr uint32_t kGzHeaderBytes = 10, kGzTrailerBytes = 8, kGzFinalBlockBytes = 5;

// ---------------------------------------------------------------------------------------------------------------- CRC-32
constexpr uint32_t kCrcPoly = 0xEDB88320u;      // reflected: bit 31 is x^0

SF_GZ_HD uint32_t crc32_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    return c;
}

// running standard CRC (as zlib.crc32 returns it) over one more slice; table[i] = crc32_table_entry(i)
template <typename Table, typename Byte>
SF_GZ_HD uint32_t crc32_slice(uint32_t crc, Table table, Byte byte_at, uint32_t n) {
    crc = ~crc;
    for (uint32_t i = 0; i < n; ++i) crc = table[(crc ^ byte_at(i)) & 0xffu] ^ (crc >> 8);
    return ~crc;
}

// a(x) b(x) mod P
SF_GZ_HD uint32_t crc32_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8 n) mod P
SF_GZ_HD uint32_t crc32_xpow8(uint64_t n) {
    uint32_t p = 0x80000000u, sq = 0x00800000u;         // x^0, x^8
    while (n) {
        if (n & 1u) p = crc32_mulmod(sq, p);
        sq = crc32_mulmod(sq, sq);
        n >>= 1;
    }
    return p;
}

// CRC of A || B from the CRCs of A and of B and the length of B
SF_GZ_HD uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return crc32_mulmod(crc32_xpow8(len_b), crc_a) ^ crc_b;
}

// ---------------------------------------------------------------------------------------------------------------- tokens
// length 3 .. 258 -> symbol 257 .. 285; *eb extra bits holding *ev
SF_GZ_HD int gz_len_symbol(uint32_t len, int* eb, uint32_t* ev) {
    const uint32_t l = len - kGzMinMatch;
    if (l < 8u) { *eb = 0; *ev = 0; return 257 + (int)l; }
    if (len == kGzMaxMatch) { *eb = 0; *ev = 0; return 285; }
    int lg = 3;
    while ((l >> (lg + 1)) != 0u) ++lg;                  // floor(log2 l), 3 .. 7
    const int e = lg - 2;
    *eb = e; *ev = l & ((1u << e) - 1u);
    return 257 + 4 * e + 4 + (int)((l >> e) & 3u);
}

SF_GZ_HD int gz_ctz64(uint64_t v) {                      // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}
SF_GZ_HD int gz_clz64(uint64_t v) {                      // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}

// eq(w) = 64 bits of the mask: bit i of the block is set iff 0 < i < n and byte i equals byte i - 1; words behind the block are 0.
// Number of set bits from position i on, at most kGzMaxMatch.
template <typename EqWord>
SF_GZ_HD uint32_t gz_run_len(EqWord eq, uint32_t i, uint32_t n) {
    uint32_t len = 0;
    while (len < kGzMaxMatch && i + len < n) {
        const uint32_t pos = i + len, sh = pos & 63u, avail = 64u - sh;
        const uint64_t inv = ~(eq(pos >> 6) >> sh);
        const uint32_t c = inv ? (uint32_t)gz_ctz64(inv) : 64u;      // <= avail: the shift brought zeros in
        len += c < avail ? c : avail;
        if (c < avail) break;
    }
    return len < kGzMaxMatch ? len : kGzMaxMatch;
}

// The tokens of the greedy parse that START in [c0, c1): emit(position, length), length 1 = a literal.  z = the last position
// below c0 whose mask bit is clear (anything when c0 == 0: bit 0 is clear).  Inside a run that began at z + 1 the greedy parse
// places a token at every multiple of 258 from its start: a match of min(258, what is left) when that is >= 3, else literals.
template <typename EqWord, typename Emit>
SF_GZ_HD void gz_chunk_tokens(EqWord eq, uint32_t c0, uint32_t c1, uint32_t n, int32_t z, Emit emit) {
    if (c1 > n) c1 = n;
    for (uint32_t i = c0; i < c1; ++i) {
        if (!((eq(i >> 6) >> (i & 63u)) & 1u)) { z = (int32_t)i; emit(i, 1u); continue; }
        const uint32_t q = (i - (uint32_t)z - 1u) % kGzMaxMatch;
        if (q == 0u) {
            const uint32_t len = gz_run_len(eq, i, n);
            emit(i, len >= kGzMinMatch ? len : 1u);
        } else if (q == 1u) {
            // the token before was a literal exactly when fewer than 3 bytes of the run were left there: this is its last byte
            const bool more = i + 1u < n && ((eq((i + 1u) >> 6) >> ((i + 1u) & 63u)) & 1u);
            if (!more) emit(i, 1u);
        }
    }
}

// the same parse as a plain loop over the bytes
template <typename Emit>
SF_GZ_HD void gz_greedy_tokens(const uint8_t* in, uint32_t n, Emit emit) {
    uint32_t i = 0;
    while (i < n) {
        uint32_t len = 0;
        if (i > 0) while (len < kGzMaxMatch && i + len < n && in[i + len] == in[i - 1]) ++len;
        if (len >= kGzMinMatch) { emit(i, len); i += len; }
        else { emit(i, 1u); ++i; }
    }
}

// ---------------------------------------------------------------------------------------------------------------- Huffman
SF_GZ_HD bool huff_less(uint32_t fa, int a, uint32_t fb, int b) { return fa < fb || (fa == fb && a < b); }

// rank of the used symbol `sym` in the order by (frequency, symbol); *n_used = number of used symbols
SF_GZ_HD int huff_rank(const uint32_t* freq, int n, int sym, int* n_used) {
    int r = 0, u = 0;
    const uint32_t f = freq[sym];
    for (int s = 0; s < n; ++s) {
        const uint32_t g = freq[s];
        u += g != 0u;
        r += g != 0u && huff_less(g, s, f, sym);
    }
    *n_used = u;
    return r;
}

// Two-queue Huffman merge over the n_used >= 2 leaves in rank order (leaf r = symbol order[r]).  Nodes 0 .. n_used - 1 are the
// leaves, n_used .. 2 n_used - 2 the inner nodes in creation order; the last one is the root and its own parent.  Of two equal
// weights the leaf goes first (flatter trees).
SF_GZ_HD void huff_merge(const uint32_t* freq, const uint16_t* order, int n_used, uint32_t* node_freq, uint16_t* parent) {
    for (int r = 0; r < n_used; ++r) node_freq[r] = freq[order[r]];
    int i = 0, j = n_used;
    for (int k = n_used; k < 2 * n_used - 1; ++k) {
        uint32_t sum = 0;
        for (int t = 0; t < 2; ++t) {
            int pick;
            if (i < n_used && (j >= k || node_freq[i] <= node_freq[j])) pick = i++;
            else pick = j++;
            sum += node_freq[pick];
            parent[pick] = (uint16_t)k;
        }
        node_freq[k] = sum;
    }
    parent[2 * n_used - 2] = (uint16_t)(2 * n_used - 2);
}

SF_GZ_HD int huff_depth(const uint16_t* parent, int node, int root) {
    int d = 0;
    while (node != root) { node = parent[node]; ++d; }
    return d;
}

// count[d] = leaves at depth d (deeper ones already counted at max_bits), d = 1 .. max_bits.  Moves leaves between depths until
// the Kraft sum is exactly 1: while it is too large the deepest leaf above the limit goes one down; a deficit is then paid back
// from the deepest level, whose unit always divides it.
SF_GZ_HD void huff_limit(uint32_t* count, int max_bits) {
    const uint32_t one = 1u << max_bits;
    uint32_t kraft = 0;
    for (int d = 1; d <= max_bits; ++d) kraft += count[d] << (max_bits - d);
    while (kraft > one) {
        int d = max_bits - 1;
        while (count[d] == 0u) --d;
        --count[d]; ++count[d + 1];
        kraft -= 1u << (max_bits - d - 1);
    }
    while (kraft < one) {
        int d = max_bits;
        while (count[d] == 0u) --d;
        --count[d]; ++count[d - 1];
        kraft += 1u << (max_bits - d);
    }
}

// the code length of the leaf of rank r: the rarest symbols take the longest codes
SF_GZ_HD int huff_len_of_rank(const uint32_t* count, int r, int max_bits) {
    uint32_t acc = 0;
    for (int d = max_bits; d >= 1; --d) {
        acc += count[d];
        if ((uint32_t)r < acc) return d;
    }
    return 0;
}

SF_GZ_HD uint32_t gz_rev_bits(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) { r = (r << 1) | (code & 1u); code >>= 1; }
    return r;
}

// canonical code of `sym` (RFC 1951 3.2.2) from all the lengths, bit-reversed: ready to be sent from bit 0
SF_GZ_HD uint32_t huff_code_rev(const uint8_t* lens, int n, int sym) {
    const int len = lens[sym];
    if (len == 0) return 0u;
    uint32_t code = 0;                                   // first code of this length
    for (int d = 1; d < len; ++d) {
        uint32_t c = 0;
        for (int s = 0; s < n; ++s) c += lens[s] == d;
        code = (code + c) << 1;
    }
    for (int s = 0; s < sym; ++s) code += lens[s] == len;
    return gz_rev_bits(code, len);
}

// first canonical code of every length from the depth counts: first[d], d = 1 .. max_bits
SF_GZ_HD void huff_first_codes(const uint32_t* count, int max_bits, uint32_t* first) {
    uint32_t code = 0;
    for (int d = 1; d <= max_bits; ++d) { first[d] = code; code = (code + count[d]) << 1; }
}

// Code lengths (<= max_bits, Kraft sum exactly 1) of a histogram, serially.  Fewer than two used symbols are filled up with
// symbol 0 or 1 at frequency 0, as zlib does, so that the code is complete for every inflater: a single used symbol and its
// partner get one bit each.  scratch: order[n], parent[2 n], node_freq[2 n], count[max_bits + 1] (the caller's: LDS in a kernel).
// Returns the number of coded symbols.
SF_GZ_HD int huff_lengths_serial(const uint32_t* freq, int n, int max_bits, uint8_t* lens, uint16_t* order, uint16_t* parent,
                                 uint32_t* node_freq, uint32_t* count) {
    int n_used = 0;
    for (int s = 0; s < n; ++s) { lens[s] = 0; n_used += freq[s] != 0u; }
    if (n_used < 2) {
        int only = -1;
        for (int s = 0; s < n; ++s) if (freq[s] != 0u) only = s;
        lens[only < 0 ? 0 : only] = 1;
        lens[only == 0 ? 1 : (only < 0 ? 1 : 0)] = 1;
        return 2;
    }
    for (int s = 0; s < n; ++s) {
        if (freq[s] == 0u) continue;
        int u;
        order[huff_rank(freq, n, s, &u)] = (uint16_t)s;
    }
    huff_merge(freq, order, n_used, node_freq, parent);
    for (int d = 0; d <= max_bits; ++d) count[d] = 0;
    for (int r = 0; r < n_used; ++r) {
        const int d = huff_depth(parent, r, 2 * n_used - 2);
        ++count[d < max_bits ? d : max_bits];
    }
    huff_limit(count, max_bits);
    for (int r = 0; r < n_used; ++r) lens[order[r]] = (uint8_t)huff_len_of_rank(count, r, max_bits);
    return n_used;
}

// ---------------------------------------------------------------------------------------------------------------- framing
// the low n_bits (<= 25) of `value` at bit position `pos` of an image of 32-bit words, through or32(word index, bits)
template <typename Or32>
SF_GZ_HD void gz_put_bits(Or32 or32, uint64_t pos, uint32_t value, int n_bits) {
    const uint64_t v = (uint64_t)(value & ((1u << n_bits) - 1u)) << (pos & 31u);
    or32((uint32_t)(pos >> 5), (uint32_t)v);
    if (v >> 32) or32((uint32_t)(pos >> 5) + 1u, (uint32_t)(v >> 32));
}

// The run-length form of the code-length sequence seq(0 .. n): emit(symbol 0 .. 18, extra bits, extra value).  Zeros repeat with
// 17 (3 .. 10) and 18 (11 .. 138), other lengths with 16 (3 .. 6 copies of the length before).
template <typename Seq, typename Emit>
SF_GZ_HD void gz_cl_rle(Seq seq, int n, Emit emit) {
    int i = 0;
    while (i < n) {
        const int v = seq(i);
        int r = 1;
        while (i + r < n && seq(i + r) == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) { const int t = r < 138 ? r : 138; emit(18, 7, (uint32_t)(t - 11)); r -= t; }
            if (r >= 3) { emit(17, 3, (uint32_t)(r - 3)); r = 0; }
        } else {
            emit(v, 0, 0u); --r;
            while (r >= 3) { const int t = r < 6 ? r : 6; emit(16, 2, (uint32_t)(t - 3)); r -= t; }
        }
        for (; r > 0; --r) emit(v, 0, 0u);
    }
}

SF_GZ_HD int gz_cl_order(int i) {
    const uint8_t order[kGzClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// The header of a dynamic block with the given BFINAL bit, for the literal/length lengths `lens` (trailing zeros above symbol
// 256 are not sent) and the n_dist distance lengths dist_len(0 .. n_dist - 1) exactly as the caller counts them, written from bit
// pos0 through or32.  Returns its length in bits.  `w` is the caller's scratch.
struct GzClWork {
    uint32_t cl_freq[kGzClSyms], cl_code[kGzClSyms], node_freq[2 * kGzClSyms], count[kGzMaxClBits + 1];
    uint16_t order[kGzClSyms], parent[2 * kGzClSyms];
    uint8_t cl_lens[kGzClSyms];
};
template <typename DistLen, typename Or32>
SF_GZ_HD uint32_t gz_write_dyn_header(uint32_t bfinal, uint64_t pos0, const uint8_t* lens, DistLen dist_len, int n_dist, GzClWork* w, Or32 or32) {
    uint32_t* cl_freq = w->cl_freq; uint32_t* cl_code = w->cl_code; uint8_t* cl_lens = w->cl_lens;
    int n_lit = kGzLitSyms;
    while (n_lit > 257 && lens[n_lit - 1] == 0) --n_lit;
    const int n_seq = n_lit + n_dist;
    auto seq = [&](int i) -> int { return i < n_lit ? (int)lens[i] : (int)dist_len(i - n_lit); };
    for (int s = 0; s < kGzClSyms; ++s) cl_freq[s] = 0;
    gz_cl_rle(seq, n_seq, [&](int sym, int, uint32_t) { ++cl_freq[sym]; });
    huff_lengths_serial(cl_freq, kGzClSyms, kGzMaxClBits, cl_lens, w->order, w->parent, w->node_freq, w->count);
    for (int s = 0; s < kGzClSyms; ++s) cl_code[s] = huff_code_rev(cl_lens, kGzClSyms, s);
    int n_cl = kGzClSyms;
    while (n_cl > 4 && cl_lens[gz_cl_order(n_cl - 1)] == 0) --n_cl;
    uint64_t pos = pos0;
    auto put = [&](uint32_t v, int nb) { gz_put_bits(or32, pos, v, nb); pos += (uint32_t)nb; };
    put(bfinal, 1);
    put(2u, 2);                                          // BTYPE = dynamic
    put((uint32_t)(n_lit - 257), 5);
    put((uint32_t)(n_dist - 1), 5);
    put((uint32_t)(n_cl - 4), 4);
    for (int i = 0; i < n_cl; ++i) put(cl_lens[gz_cl_order(i)], 3);
    gz_cl_rle(seq, n_seq, [&](int sym, int eb, uint32_t ev) {
        put(cl_code[sym] | (ev << cl_lens[sym]), cl_lens[sym] + eb);
    });
    return (uint32_t)(pos - pos0);
}
// this stream's blocks: not final, from bit 0; the distance code is always symbols 0 and 1 at one bit each (distance 1 is
// symbol 0), and both are sent: the count is not trimmed
template <typename Or32>
SF_GZ_HD uint32_t gz_write_block_header(const uint8_t* lens, GzClWork* w, Or32 or32) {
    return gz_write_dyn_header(0u, 0ull, lens, [](int) { return 1; }, kGzDistSyms, w, or32);
}

// bits of one token under the lengths `lens` / its code word (literal: the byte; match: length code, extra bits, the 1-bit
// distance code 0)
SF_GZ_HD uint32_t gz_token_bits(const uint8_t* lens, uint32_t byte, uint32_t len) {
    if (len == 1u) return lens[byte];
    int eb; uint32_t ev;
    const int sym = gz_len_symbol(len, &eb, &ev);
    return (uint32_t)lens[sym] + (uint32_t)eb + 1u;
}
SF_GZ_HD uint32_t gz_token_code(const uint8_t* lens, const uint16_t* codes, uint32_t byte, uint32_t len, int* n_bits) {
    if (len == 1u) { *n_bits = lens[byte]; return codes[byte]; }
    int eb; uint32_t ev;
    const int sym = gz_len_symbol(len, &eb, &ev);
    *n_bits = lens[sym] + eb + 1;
    return (uint32_t)codes[sym] | (ev << lens[sym]);
}
SF_GZ_HD int gz_token_symbol(uint32_t byte, uint32_t len) {
    if (len == 1u) return (int)byte;
    int eb; uint32_t ev;
    return gz_len_symbol(len, &eb, &ev);
}

// bytes of a block coded as dynamic block + empty stored block, from the bits of header, tokens and end-of-block symbol
SF_GZ_HD uint32_t gz_coded_bytes(uint32_t bits) { return (bits + 3u + 7u) / 8u + 4u; }
// bytes of n payload bytes as stored blocks
SF_GZ_HD uint32_t gz_stored_bytes(uint32_t n) { return n + 5u * ((n + kGzStoredMax - 1u) / kGzStoredMax); }
// byte `i` of the stored form: put(index, byte) for the 5 header bytes of the stored block that begins at payload offset `at`
template <typename Put>
SF_GZ_HD void gz_stored_header(uint32_t at, uint32_t n, Put put) {
    const uint32_t len = n - at < kGzStoredMax ? n - at : kGzStoredMax;
    const uint32_t o = at + 5u * (at / kGzStoredMax);
    put(o, (uint8_t)0);
    put(o + 1u, (uint8_t)(len & 0xffu)); put(o + 2u, (uint8_t)(len >> 8));
    put(o + 3u, (uint8_t)(~len & 0xffu)); put(o + 4u, (uint8_t)((~len >> 8) & 0xffu));
}
// where payload byte i sits in the stored form
SF_GZ_HD uint32_t gz_stored_pos(uint32_t i) { return i + 5u * (i / kGzStoredMax + 1u); }

SF_GZ_HD void gz_header(uint8_t* out) {                  // no name, no time, unknown OS
    const uint8_t h[kGzHeaderBytes] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    for (uint32_t i = 0; i < kGzHeaderBytes; ++i) out[i] = h[i];
}
// the final (empty, stored) block and the trailer: kGzFinalBlockBytes + kGzTrailerBytes bytes
SF_GZ_HD void gz_trailer(uint32_t crc, uint64_t n_bytes, uint8_t* out) {
    out[0] = 1; out[1] = 0; out[2] = 0; out[3] = 0xff; out[4] = 0xff;
    const uint32_t isize = (uint32_t)(n_bytes & 0xffffffffull);
    for (int i = 0; i < 4; ++i) { out[5 + i] = (uint8_t)(crc >> (8 * i)); out[9 + i] = (uint8_t)(isize >> (8 * i)); }
}

// One block (1 <= n <= kGzBlockBytes), serially, into `out` (room for gz_stored_bytes(n) + 8, zeroed by the callee).  Returns
// the number of bytes; *stored = 1 when the stored form was chosen, -1 if the coded form left the buffer (never: it is shorter).
SF_GZ_HD uint32_t gz_encode_block_serial(const uint8_t* in, uint32_t n, uint8_t* out, int* stored) {
    uint32_t freq[kGzLitSyms];
    for (int s = 0; s < kGzLitSyms; ++s) freq[s] = 0;
    gz_greedy_tokens(in, n, [&](uint32_t i, uint32_t len) { ++freq[gz_token_symbol(in[i], len)]; });
    freq[kGzEob] = 1;
    uint8_t lens[kGzLitSyms];
    uint16_t codes[kGzLitSyms], order[kGzLitSyms], parent[2 * kGzLitSyms];
    uint32_t node_freq[2 * kGzLitSyms], count[kGzMaxBits + 1];
    GzClWork clw;
    huff_lengths_serial(freq, kGzLitSyms, kGzMaxBits, lens, order, parent, node_freq, count);
    for (int s = 0; s < kGzLitSyms; ++s) codes[s] = (uint16_t)huff_code_rev(lens, kGzLitSyms, s);
    const uint32_t cap = gz_stored_bytes(n) + 8u;
    bool overrun = false;                                // bits behind the buffer: *stored = -1
    for (uint32_t i = 0; i < cap; ++i) out[i] = 0;
    auto or32 = [&](uint32_t w, uint32_t bits) {
        for (int b = 0; b < 4; ++b) {
            const uint32_t at = 4u * w + (uint32_t)b;
            if (at < cap) out[at] |= (uint8_t)(bits >> (8 * b));
            else if ((bits >> (8 * b)) & 0xffu) overrun = true;
        }
    };
    uint64_t pos = gz_write_block_header(lens, &clw, or32);
    uint64_t body = 0;
    gz_greedy_tokens(in, n, [&](uint32_t i, uint32_t len) { body += gz_token_bits(lens, in[i], len); });
    const uint32_t bits = (uint32_t)(pos + body + lens[kGzEob]);
    const uint32_t coded = gz_coded_bytes(bits), raw = gz_stored_bytes(n);
    if (coded < raw) {
        gz_greedy_tokens(in, n, [&](uint32_t i, uint32_t len) {
            int nb;
            const uint32_t c = gz_token_code(lens, codes, in[i], len, &nb);
            gz_put_bits(or32, pos, c, nb);
            pos += (uint32_t)nb;
        });
        gz_put_bits(or32, pos, codes[kGzEob], lens[kGzEob]);
        out[coded - 2u] = 0xff; out[coded - 1u] = 0xff;         // LEN = 0, NLEN = 0xffff of the empty stored block
        *stored = overrun ? -1 : 0;
        return coded;
    }
    for (uint32_t at = 0; at < n; at += kGzStoredMax) gz_stored_header(at, n, [&](uint32_t o, uint8_t b) { out[o] = b; });
    for (uint32_t i = 0; i < n; ++i) out[gz_stored_pos(i)] = in[i];
    *stored = 1;
    return raw;
}

}  // namespace sfgpu
