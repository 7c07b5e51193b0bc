// bgzfmt.h -- what a blocked-gzip (BGZF) member is and how it inflates, as functions both sides call: the kernel of bgzf_read.hip
// (sfgpu_bgzf_inflate_host, one wavefront per member) and plain C++ (tests/bgzf_harness.cpp compiles this header with g++ and
// runs bgz_inflate_member serially; tests/test_bgzf_cpu.py lets zlib judge it).
//
// A BGZF file is a sequence of gzip members (RFC 1952) that each hold at most 64 KB of payload, carry their own compressed size
// in a 'B','C' extra subfield (BSIZE = member bytes - 1) and are independent of one another: no match reaches before a member's
// first byte.  Member = header (bgz_parse_header) | DEFLATE body (RFC 1951) | CRC-32 | ISIZE.
//
//   bgz_parse_header   the header walk: FEXTRA subfields (others than BC are skipped), FNAME, FCOMMENT, FHCRC
//   bgz_build_table    canonical Huffman decode table from code lengths; what is accepted is what zlib's inflate_table accepts
//   BgzBits            the bit reader: 64-bit hold filled by 32-bit words, bits behind the body read as 0 and cannot be taken
//   bgz_inflate_body   the blocks of one member, written against an IO policy: the serial policy is BgzSerialIO below, the kernel's
//                      policy runs the same statements wave-uniformly and spreads copies over the lanes
//   bgz_finish         the checks behind the last block, in stream order
//   bgz_inflate_member all of it serially
//
// gzrdfmt.h (ordinary gzip, chunk by chunk) has a SIBLING of bgz_inflate_body: gzr_dyn_header + gzr_decode_chunk run the same
// statements with 64-bit output positions, a stop rule at block boundaries and a preset window.  A fix to the decode or to what
// zlib accepts belongs in both.
//
// ERRORS (SFGPU_BGZF_*, include/sfgpu.h).  The first failed check in stream order is the member's error.  Where zlib and the
// wording of RFC 1951 differ, zlib decides:
//   - an incomplete code is BAD_CODE_LENGTHS, except that a literal/length or distance code of ONE code of one bit is accepted
//     (inflate_table: "left > 0 && (type == CODES || max != 1)"), as is a distance code without any code; the unassigned code
//     words of such sets are BAD_SYMBOL when the stream uses them.  For the code-length code every incomplete set is an error.
//   - HLIT > 286 or HDIST > 30 is BAD_CODE_LENGTHS (zlib without PKZIP_BUG_WORKAROUND), though the fixed code assigns 288 / 32 code
//     words: length symbols 286 / 287 and distance symbols 30 / 31 decode, and are BAD_SYMBOL.
//   - a distance of 32768 is valid (the window is 32 KB); zlib's deflate never emits one beyond 32506.
// Bits: a symbol is decoded from the next 15 bits with zeros behind the end of the body.  If that gives a code word longer than
// what is left, or none while fewer than 15 bits are left, the member is TRUNCATED; none with 15 bits there is BAD_SYMBOL.
// A final block that ends before the last byte in front of the trailer means BSIZE is wrong about the stream: BAD_HEADER.
#pragma once
#include <cstdint>

#include "../../include/sfgpu.h"
#include "gzfmt.h"

#if defined(__HIPCC__)
#define SF_BGZ_HD __host__ __device__ __forceinline__
#define SF_BGZ_HD_NOINLINE __host__ __device__ inline __attribute__((noinline))
#else
#define SF_BGZ_HD inline
#define SF_BGZ_HD_NOINLINE inline
#endif

namespace sfgpu {

constexpr uint32_t kBgzMaxPayload = 65536;       // ISIZE of a member
constexpr uint32_t kBgzMaxMember = 65536;        // BSIZE + 1
constexpr uint32_t kBgzMinHeader = 18, kBgzTrailer = 8;
constexpr int kBgzNeedMore = -1;                 // bgz_parse_header: the bytes at hand do not decide yet
constexpr int kBgzLitFastBits = 10, kBgzDistFastBits = 8, kBgzClFastBits = 7;
constexpr int kBgzLitSyms = 288, kBgzDistSyms = 32, kBgzClSyms = 19;

struct BgzHeader {
    uint32_t hdr_len;     // where the DEFLATE body begins
    uint32_t total;       // member bytes = BSIZE + 1
};

// The header of the member that begins at byte 0 of byte(0 .. avail).  SFGPU_BGZF_OK, SFGPU_BGZF_BAD_HEADER, or kBgzNeedMore when
// `avail` bytes do not reach the end of the header.  The trailer is not looked at.
template <typename Byte>
SF_BGZ_HD int bgz_parse_header(Byte byte, uint64_t avail, BgzHeader* h) {
    if (avail < 12) {
        if (avail >= 1 && byte(0) != 0x1f) return SFGPU_BGZF_BAD_HEADER;
        if (avail >= 2 && byte(1) != 0x8b) return SFGPU_BGZF_BAD_HEADER;
        return kBgzNeedMore;
    }
    if (byte(0) != 0x1f || byte(1) != 0x8b || byte(2) != 8) return SFGPU_BGZF_BAD_HEADER;
    const uint32_t flg = byte(3);
    if (!(flg & 4u)) return SFGPU_BGZF_BAD_HEADER;                       // no FEXTRA: no BC
    const uint32_t xlen = (uint32_t)byte(10) | ((uint32_t)byte(11) << 8);
    uint64_t p = 12;
    const uint64_t xend = p + xlen;
    if (xend > avail) return xend > kBgzMaxMember ? SFGPU_BGZF_BAD_HEADER : kBgzNeedMore;
    bool found = false;
    uint32_t bsize = 0;
    while (p < xend) {
        if (p + 4 > xend) return SFGPU_BGZF_BAD_HEADER;
        const uint32_t si1 = byte(p), si2 = byte(p + 1), slen = (uint32_t)byte(p + 2) | ((uint32_t)byte(p + 3) << 8);
        if (p + 4 + slen > xend) return SFGPU_BGZF_BAD_HEADER;
        if (si1 == 'B' && si2 == 'C' && slen == 2 && !found) {
            bsize = (uint32_t)byte(p + 4) | ((uint32_t)byte(p + 5) << 8);
            found = true;
        }
        p += 4 + slen;
    }
    if (!found) return SFGPU_BGZF_BAD_HEADER;
    const uint32_t total = bsize + 1;
    for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {                     // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        for (;;) {
            if (p >= total) return SFGPU_BGZF_BAD_HEADER;
            if (p >= avail) return kBgzNeedMore;
            if (byte(p++) == 0) break;
        }
    }
    if (flg & 2u) p += 2;                                                // FHCRC
    if (p + kBgzTrailer > total) return SFGPU_BGZF_BAD_HEADER;
    h->hdr_len = (uint32_t)p;
    h->total = total;
    return SFGPU_BGZF_OK;
}

template <typename Byte>
SF_BGZ_HD uint32_t bgz_le32(Byte byte, uint64_t p) {
    return (uint32_t)byte(p) | ((uint32_t)byte(p + 1) << 8) | ((uint32_t)byte(p + 2) << 16) | ((uint32_t)byte(p + 3) << 24);
}

// ---------------------------------------------------------------------------------------------------------------- tables
// One wave's (or the serial run's) decode state.  fast[peek & mask] = (symbol << 4 | length) for code words of at most the
// table's bits, 0 otherwise; longer code words are found canonically from count[] and sym[] (the symbols in code order).
struct BgzTables {
    uint16_t lit_fast[1u << kBgzLitFastBits];
    uint16_t dist_fast[1u << kBgzDistFastBits];
    uint16_t cl_fast[1u << kBgzClFastBits];
    uint16_t lit_sym[kBgzLitSyms], dist_sym[kBgzDistSyms], cl_sym[kBgzClSyms + 1];
    uint16_t lit_count[16], dist_count[16], cl_count[16];
    uint16_t offs[16];
    uint8_t lens[kBgzLitSyms + kBgzDistSyms];
    int32_t status;       // what the lane that built the tables found
};

enum { kBgzCodes = 0, kBgzLens = 1, kBgzDists = 2 };      // zlib's codetype

// false: zlib's inflate_table rejects these lengths
SF_BGZ_HD_NOINLINE bool bgz_build_table(const uint8_t* lens, int n, int type, uint16_t* fast, int fast_bits, uint16_t* sym, uint16_t* count,
                                        uint16_t* offs) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[lens[s]];
    const uint32_t fast_n = 1u << fast_bits;
    for (uint32_t i = 0; i < fast_n; ++i) fast[i] = 0;
    int max = 15;
    while (max >= 1 && count[max] == 0) --max;
    count[0] = 0;
    if (max == 0) return type != kBgzCodes;                // no code at all: zlib hands out a table of invalid entries
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= (int)count[l];
        if (left < 0) return false;                        // over-subscribed
    }
    if (left > 0 && (type == kBgzCodes || max != 1)) return false;      // incomplete
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; ++s) if (lens[s]) sym[offs[lens[s]]++] = (uint16_t)s;
    uint32_t code = 0, k = 0;
    for (int l = 1; l <= fast_bits && l <= max; ++l) {
        for (uint32_t c = 0; c < count[l]; ++c, ++k, ++code) {
            const uint16_t e = (uint16_t)((sym[k] << 4) | l);
            for (uint32_t i = gz_rev_bits(code, l); i < fast_n; i += 1u << l) fast[i] = e;
        }
        code <<= 1;
    }
    return true;
}

// the code word that begins `bits` (15 of them, the first in bit 0) -> symbol << 4 | length, 0 when there is none
SF_BGZ_HD uint32_t bgz_decode(uint32_t bits, const uint16_t* fast, int fast_bits, const uint16_t* sym, const uint16_t* count) {
    const uint32_t e = fast[bits & ((1u << fast_bits) - 1u)];
    if (e) return e;
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = count[l];
        if (code - c < first) return ((uint32_t)sym[index + (code - first)] << 4) | (uint32_t)l;
        index += c; first += c;
        first <<= 1; code <<= 1;
    }
    return 0;
}

SF_BGZ_HD void bgz_len_base(uint32_t sym, uint32_t* base, uint32_t* extra) {     // sym 257 .. 285
    const uint32_t i = sym - 257u;
    if (i < 8u) { *base = 3u + i; *extra = 0; return; }
    if (i == 28u) { *base = 258u; *extra = 0; return; }
    const uint32_t e = (i >> 2) - 1u;
    *extra = e;
    *base = 3u + ((4u + (i & 3u)) << e);
}
SF_BGZ_HD void bgz_dist_base(uint32_t sym, uint32_t* base, uint32_t* extra) {    // sym 0 .. 29
    if (sym < 4u) { *base = 1u + sym; *extra = 0; return; }
    const uint32_t e = (sym >> 1) - 1u;
    *extra = e;
    *base = 1u + ((2u + (sym & 1u)) << e);
}

// ---------------------------------------------------------------------------------------------------------------- bits
// word(p) = the four bytes at byte offset p (a multiple of 4) of the member's frame, little-endian; the frame may begin up to
// 15 bytes before the member, so that the kernel's frame is 16-byte aligned in device memory.
struct BgzBits {
    uint64_t hold;
    uint32_t nbits;       // valid bits in hold
    uint32_t next;        // frame offset of the next word
    int64_t left;         // bits of the body not taken yet

    template <typename IO>
    SF_BGZ_HD void seek(IO& io, uint32_t byte_pos, uint32_t end_pos) {
        next = byte_pos & ~3u;
        const uint32_t skip = (byte_pos & 3u) * 8u;
        hold = (uint64_t)io.word(next) >> skip;
        nbits = 32u - skip;
        next += 4u;
        left = ((int64_t)end_pos - (int64_t)byte_pos) * 8;
    }
    template <typename IO>
    SF_BGZ_HD void fill(IO& io) {                          // afterwards nbits > 32
        if (nbits <= 32u) {
            hold |= (uint64_t)io.word(next) << nbits;
            nbits += 32u;
            next += 4u;
        }
    }
    SF_BGZ_HD uint32_t peek15() const {
        const uint32_t v = (uint32_t)hold & 0x7fffu;
        return left >= 15 ? v : v & ((1u << (uint32_t)left) - 1u);
    }
    SF_BGZ_HD bool take(uint32_t n, uint32_t* v) {         // n <= 16, n <= nbits
        if ((int64_t)n > left) return false;
        *v = (uint32_t)hold & ((1u << n) - 1u);
        hold >>= n; nbits -= n; left -= n;
        return true;
    }
    SF_BGZ_HD uint32_t byte_pos() const { return next - nbits / 8u; }      // on a byte boundary
};

struct BgzCounts {
    uint32_t n_out;
    uint32_t blocks[3];       // stored, fixed, dynamic: blocks whose header was read
};

// a code word of `tab` off the reader: SFGPU_BGZF_OK and *sym, or the error
#define SF_BGZ_SYMBOL(fast, fb, symtab, cnt, out_sym)                                   \
    do {                                                                                \
        const uint32_t e_ = io.uniform(bgz_decode(bits.peek15(), fast, fb, symtab, cnt));           \
        if (e_ == 0u || (int64_t)(e_ & 15u) > bits.left) return fail(bits.left < 15 ? SFGPU_BGZF_TRUNCATED : SFGPU_BGZF_BAD_SYMBOL); \
        uint32_t drop_;                                                                 \
        bits.take(e_ & 15u, &drop_);                                                    \
        out_sym = e_ >> 4;                                                              \
    } while (0)
#define SF_BGZ_TAKE(n, v) do { if (!bits.take(n, &(v))) return fail(SFGPU_BGZF_TRUNCATED); } while (0)

// The DEFLATE body [body_pos, end_pos) of the frame into out[0 .. cap).  IO:
//   word(p)                      see BgzBits
//   uniform(v)                   v (the kernel: v of the first lane, which tells the compiler that all lanes hold the same value)
//   single(f)                    f() once (the kernel: one lane; the tables it writes are read by all afterwards)
//   store_len(T, i, v)           T->lens[i] = v
//   put(o, b)                    out[o] = b
//   copy(o, dist, len)           out[o + i] = out[o + i - dist], i = 0 .. len in order (dist < len repeats the last dist bytes)
//   stored(o, p, len)            out[o + i] = frame byte p + i
template <typename IO>
SF_BGZ_HD int bgz_inflate_body(IO& io, BgzTables* T, uint32_t body_pos, uint32_t end_pos, uint32_t cap, BgzCounts* cnt,
                                        uint32_t* stream_end) {
    BgzBits bits;
    bits.seek(io, body_pos, end_pos);
    uint32_t o = 0, n_stored = 0, n_fixed = 0, n_dynamic = 0;
    // the counts live in registers while the symbols run and are written once, on the way out
    auto fail = [&](int kind) -> int {
        cnt->n_out = o;
        cnt->blocks[0] = n_stored; cnt->blocks[1] = n_fixed; cnt->blocks[2] = n_dynamic;
        return kind;
    };
    for (;;) {
        bits.fill(io);
        uint32_t bfinal, btype;
        SF_BGZ_TAKE(1, bfinal);
        SF_BGZ_TAKE(2, btype);
        if (btype == 3u) return fail(SFGPU_BGZF_BAD_BLOCK_TYPE);
        n_stored += btype == 0u; n_fixed += btype == 1u; n_dynamic += btype == 2u;
        if (btype == 0u) {
            uint32_t pad, len, nlen;
            SF_BGZ_TAKE(bits.nbits & 7u, pad);
            bits.fill(io);
            SF_BGZ_TAKE(16, len);
            SF_BGZ_TAKE(16, nlen);
            if (len != (nlen ^ 0xffffu)) return fail(SFGPU_BGZF_STORED_LEN);
            if ((int64_t)len * 8 > bits.left) return fail(SFGPU_BGZF_TRUNCATED);
            if (len > cap - o) return fail(SFGPU_BGZF_SIZE_MISMATCH);
            const uint32_t p = bits.byte_pos();
            io.stored(o, p, len);
            o += len;
            bits.seek(io, p + len, end_pos);
        } else {
            if (btype == 1u) {
                io.single([&]() {
                    for (int s = 0; s < kBgzLitSyms; ++s) T->lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
                    for (int s = 0; s < kBgzDistSyms; ++s) T->lens[kBgzLitSyms + s] = 5;
                    bgz_build_table(T->lens, kBgzLitSyms, kBgzLens, T->lit_fast, kBgzLitFastBits, T->lit_sym, T->lit_count, T->offs);
                    bgz_build_table(T->lens + kBgzLitSyms, kBgzDistSyms, kBgzDists, T->dist_fast, kBgzDistFastBits, T->dist_sym, T->dist_count,
                                    T->offs);
                });
            } else {
                uint32_t hlit, hdist, hclen;
                SF_BGZ_TAKE(5, hlit); SF_BGZ_TAKE(5, hdist); SF_BGZ_TAKE(4, hclen);
                hlit += 257u; hdist += 1u; hclen += 4u;
                if (hlit > 286u || hdist > 30u) return fail(SFGPU_BGZF_BAD_CODE_LENGTHS);
                for (uint32_t i = 0; i < (uint32_t)kBgzClSyms; ++i) {
                    uint32_t v = 0;
                    if (i < hclen) { bits.fill(io); SF_BGZ_TAKE(3, v); }
                    io.store_len(T, (uint32_t)gz_cl_order((int)i), v);
                }
                io.single([&]() {
                    T->status = bgz_build_table(T->lens, kBgzClSyms, kBgzCodes, T->cl_fast, kBgzClFastBits, T->cl_sym, T->cl_count, T->offs) ? 1 : 0;
                });
                if (!io.status(T)) return fail(SFGPU_BGZF_BAD_CODE_LENGTHS);
                const uint32_t total = hlit + hdist;
                uint32_t prev = 0;
                for (uint32_t i = 0; i < total;) {
                    bits.fill(io);
                    uint32_t s;
                    SF_BGZ_SYMBOL(T->cl_fast, kBgzClFastBits, T->cl_sym, T->cl_count, s);
                    if (s < 16u) {
                        // the lengths of both codes are one sequence; the distance lengths are kept behind the 288 literal slots
                        io.store_len(T, i < hlit ? i : kBgzLitSyms + (i - hlit), s);
                        prev = s; ++i;
                        continue;
                    }
                    uint32_t rep, v = 0;
                    if (s == 16u) {
                        if (i == 0u) return fail(SFGPU_BGZF_BAD_CODE_LENGTHS);
                        SF_BGZ_TAKE(2, rep); rep += 3u; v = prev;
                    } else if (s == 17u) {
                        SF_BGZ_TAKE(3, rep); rep += 3u;
                    } else {
                        SF_BGZ_TAKE(7, rep); rep += 11u;
                    }
                    if (i + rep > total) return fail(SFGPU_BGZF_BAD_CODE_LENGTHS);
                    for (uint32_t k = 0; k < rep; ++k, ++i) io.store_len(T, i < hlit ? i : kBgzLitSyms + (i - hlit), v);
                    prev = v;
                }
                for (uint32_t i = hlit; i < (uint32_t)kBgzLitSyms; ++i) io.store_len(T, i, 0u);
                for (uint32_t i = hdist; i < (uint32_t)kBgzDistSyms; ++i) io.store_len(T, kBgzLitSyms + i, 0u);
                io.single([&]() {
                    bool ok = T->lens[kGzEob] != 0;            // zlib: "missing end-of-block", checked before the tables
                    ok = ok && bgz_build_table(T->lens, kBgzLitSyms, kBgzLens, T->lit_fast, kBgzLitFastBits, T->lit_sym, T->lit_count, T->offs);
                    ok = ok && bgz_build_table(T->lens + kBgzLitSyms, kBgzDistSyms, kBgzDists, T->dist_fast, kBgzDistFastBits, T->dist_sym,
                                               T->dist_count, T->offs);
                    T->status = ok ? 1 : 0;
                });
                if (!io.status(T)) return fail(SFGPU_BGZF_BAD_CODE_LENGTHS);
            }
            for (;;) {
                bits.fill(io);
                uint32_t s;
                SF_BGZ_SYMBOL(T->lit_fast, kBgzLitFastBits, T->lit_sym, T->lit_count, s);
                if (s < 256u) {
                    if (o >= cap) return fail(SFGPU_BGZF_SIZE_MISMATCH);
                    io.put(o, s);
                    ++o;
                    continue;
                }
                if (s == (uint32_t)kGzEob) break;
                if (s > 285u) return fail(SFGPU_BGZF_BAD_SYMBOL);
                uint32_t base, extra, ev, len, dist;
                bgz_len_base(s, &base, &extra);
                SF_BGZ_TAKE(extra, ev);
                len = base + ev;
                bits.fill(io);
                SF_BGZ_SYMBOL(T->dist_fast, kBgzDistFastBits, T->dist_sym, T->dist_count, s);
                if (s > 29u) return fail(SFGPU_BGZF_BAD_SYMBOL);
                bgz_dist_base(s, &base, &extra);
                SF_BGZ_TAKE(extra, ev);
                dist = base + ev;
                if (dist > o) return fail(SFGPU_BGZF_DISTANCE_TOO_FAR);
                if (len > cap - o) return fail(SFGPU_BGZF_SIZE_MISMATCH);
                io.copy(o, dist, len);
                o += len;
            }
        }
        if (bfinal) break;
    }
    uint32_t pad;
    bits.take(bits.nbits & 7u, &pad);                      // (the bits up to the byte boundary belong to the body: they are there)
    *stream_end = bits.byte_pos();
    return fail(SFGPU_BGZF_OK);
}
#undef SF_BGZ_SYMBOL
#undef SF_BGZ_TAKE

// the checks behind the body, in stream order
SF_BGZ_HD int bgz_finish(int body_kind, uint32_t stream_end, uint32_t end_pos, uint32_t n_out, uint32_t isize, uint32_t crc, uint32_t crc_stored) {
    if (body_kind != SFGPU_BGZF_OK) return body_kind;
    if (stream_end != end_pos) return SFGPU_BGZF_BAD_HEADER;
    if (n_out != isize) return SFGPU_BGZF_SIZE_MISMATCH;
    if (crc != crc_stored) return SFGPU_BGZF_CRC_MISMATCH;
    return SFGPU_BGZF_OK;
}

// ---------------------------------------------------------------------------------------------------------------- serial
struct BgzSerialIO {
    const uint8_t* src; uint32_t n; uint8_t* out;
    uint32_t word(uint32_t p) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4u; ++k) if (p + k < n) v |= (uint32_t)src[p + k] << (8u * k);
        return v;
    }
    uint32_t uniform(uint32_t v) const { return v; }
    template <typename F> void single(F f) const { f(); }
    bool status(const BgzTables* T) const { return T->status != 0; }
    void store_len(BgzTables* T, uint32_t i, uint32_t v) const { T->lens[i] = (uint8_t)v; }
    void put(uint32_t o, uint32_t b) const { out[o] = (uint8_t)b; }
    void copy(uint32_t o, uint32_t dist, uint32_t len) const { for (uint32_t i = 0; i < len; ++i) out[o + i] = out[o + i - dist]; }
    void stored(uint32_t o, uint32_t p, uint32_t len) const { for (uint32_t i = 0; i < len; ++i) out[o + i] = src[p + i]; }
};

struct BgzMember {
    int32_t kind;             // SFGPU_BGZF_*
    uint32_t total;           // member bytes (0 when the header does not say)
    BgzCounts counts;
};

// The member at src[0 .. n) (n may reach beyond it) into dst[0 .. cap).  A member that does not lie within n is TRUNCATED.
inline BgzMember bgz_inflate_member(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap) {
    BgzMember m;
    m.total = 0; m.counts.n_out = 0; m.counts.blocks[0] = m.counts.blocks[1] = m.counts.blocks[2] = 0;
    BgzHeader h;
    auto byte = [&](uint64_t p) -> uint32_t { return src[p]; };
    m.kind = bgz_parse_header(byte, n, &h);
    if (m.kind == kBgzNeedMore) { m.kind = SFGPU_BGZF_TRUNCATED; return m; }
    if (m.kind != SFGPU_BGZF_OK) return m;
    m.total = h.total;
    if (h.total > n) { m.kind = SFGPU_BGZF_TRUNCATED; return m; }
    const uint32_t end_pos = h.total - kBgzTrailer;
    const uint32_t crc_stored = bgz_le32(byte, end_pos), isize = bgz_le32(byte, end_pos + 4u);
    if (isize > kBgzMaxPayload) { m.kind = SFGPU_BGZF_BAD_HEADER; return m; }
    BgzTables T;
    BgzSerialIO io{src, h.total, dst};
    uint32_t stream_end = 0;
    const uint32_t room = (uint64_t)isize < cap ? isize : (uint32_t)cap;
    const int body = bgz_inflate_body(io, &T, h.hdr_len, end_pos, room, &m.counts, &stream_end);
    uint32_t table[256];
    for (uint32_t i = 0; i < 256u; ++i) table[i] = crc32_table_entry(i);
    const uint32_t crc = crc32_slice(0u, table, [&](uint32_t i) -> uint32_t { return dst[i]; }, m.counts.n_out);
    m.kind = bgz_finish(body, stream_end, end_pos, m.counts.n_out, isize, crc, crc_stored);
    return m;
}

// ---------------------------------------------------------------------------------------------------------------- the file
// The member directory of src[0 .. n): the whole members in file order whose payloads fit in cap bytes, from the headers and
// trailers alone (no payload byte is touched).  out_off is the exclusive sum of the ISIZEs.  The scan stops at a header it cannot
// accept (BAD_HEADER at that member), at a member that does not end within n (with `final`: TRUNCATED at that member) and in
// front of a member whose payload does not fit.
struct BgzDirEntry {
    uint64_t in_off, out_off;
    uint32_t in_len, isize;
};
struct BgzScan {
    uint64_t n_members, consumed, n_bytes_out, error_member;
    int32_t error_kind;
};
template <typename Emit>
inline BgzScan bgz_scan(const uint8_t* src, uint64_t n, int final, uint64_t cap, Emit emit) {
    BgzScan s;
    s.n_members = s.consumed = s.n_bytes_out = 0; s.error_member = ~0ull; s.error_kind = SFGPU_BGZF_OK;
    uint64_t p = 0;
    while (p < n) {
        BgzHeader h;
        auto byte = [&](uint64_t q) -> uint32_t { return src[p + q]; };
        const int k = bgz_parse_header(byte, n - p, &h);
        if (k == kBgzNeedMore || (k == SFGPU_BGZF_OK && h.total > n - p)) {
            if (final) { s.error_member = s.n_members; s.error_kind = SFGPU_BGZF_TRUNCATED; }
            break;
        }
        const uint32_t isize = k == SFGPU_BGZF_OK ? bgz_le32(byte, h.total - 4u) : 0u;
        if (k != SFGPU_BGZF_OK || isize > kBgzMaxPayload) { s.error_member = s.n_members; s.error_kind = SFGPU_BGZF_BAD_HEADER; break; }
        if (isize > cap - s.n_bytes_out) break;
        emit(BgzDirEntry{p, s.n_bytes_out, h.total, isize});
        p += h.total; s.n_bytes_out += isize; ++s.n_members;
    }
    s.consumed = p;
    return s;
}

}  // namespace sfgpu
