// gzrdfmt.h -- how an ORDINARY gzip member (one serial DEFLATE stream of any length, RFC 1952 / 1951) is inflated in parallel
// chunks, as functions both sides call: the kernels of gz_read.hip (sfgpu_gzrd_*) and plain C++ (tests/gzrd_harness.cpp compiles
// this header with g++ and runs the whole chunked algorithm serially; tests/test_gzrd_cpu.py lets zlib judge it).  The tables, the
// bit reader and the length / distance bases are bgzfmt.h's, the CRC functions gzfmt.h's.
//
// A member's blocks are not hidden: a dynamic-Huffman block header carries enough redundancy that "does a block begin at this
// bit?" can be answered by the checks the decoder applies to every header anyway.  One call works on the bytes the caller
// holds (src[0 .. n), beginning at the byte that holds the handle's bit position):
//
//   gzr_parse_header   the general member header: CM = 8, FEXTRA / FNAME / FCOMMENT / FHCRC skipped, reserved flags BAD_HEADER
//   gzr_call_start     where this call begins: inside a member (the handle's state), at a member header, or at padding
//   gzr_cheap_test     FINDER, cheap part: bits p..p+2 = (BFINAL 0, BTYPE 2), HLIT / HDIST in range, the code-length code
//                      exactly complete -- pure ALU on four words
//   gzr_header_at      FINDER, full part: gzr_dyn_header, the statements the decoder runs at every dynamic block.  The candidate
//                      of a span (chunk_bytes of input; every span but the first) is the smallest accepted bit position in it.
//                      There is no body check, so a candidate may be false.
//   gzr_decode_chunk   PASS A and PASS B, one function against an IO policy.  A chunk starts at the known bit position or at a
//                      candidate and runs block after block.  After each non-final block it asks stop(boundary): pass A stops
//                      where the boundary IS a candidate (one look at the candidate of the span that holds the boundary: smaller
//                      candidates are thereby passed over, never repaired), pass B where pass A stopped.  A chunk also stops
//                      behind a final block whose 8 trailer bytes are at hand, and otherwise at the last boundary it completed
//                      when the input ends inside a block (or inside the trailer).
//                      Pass A writes sixteen-bit symbols into a ring of 32768 that starts as the identity (entry i = marker of
//                      byte i of the predecessor's window), so a match that reaches before the chunk copies markers; it counts
//                      its output and writes no payload.  Pass B decodes again with the resolved window as preset dictionary and
//                      writes bytes at the chunk's exact offset; a distance beyond own output + valid window is
//                      DISTANCE_TOO_FAR there, as zlib says.
//   gzr_chain          from the known start, end = next start.  The chunks reached are the call's chunks; candidates in front of
//                      the chain's end that it did not reach are false starts and their work is discarded.  An error in a chain
//                      chunk is the call's error and the chain ends in front of it; with a capacity the call takes the longest
//                      prefix whose output fits.
//   gzr_resolve        WINDOW PROPAGATION, one entry: a chunk's last 32768 symbols against its predecessor's resolved window
//   gzr_finish_call    the chunks' CRCs combined in order with the running CRC and length; behind a final block CRC-32 and
//                      ISIZE (mod 2^32) are compared: CRC_MISMATCH, SIZE_MISMATCH
//
// Error kinds are SFGPU_BGZF_* with bgzfmt.h's rule: the first failed check in stream order, zlib deciding where it and RFC 1951
// differ.  TRUNCATED inside a chunk means "the call's bytes end here": it is an error only with `final`.
#pragma once
#include <cstdint>
#include <vector>

#include "bgzfmt.h"

namespace sfgpu {

constexpr uint32_t kGzrWindow = 32768, kGzrMask = kGzrWindow - 1u;
constexpr uint32_t kGzrMarker = 0x8000u;                 // ring entry: marker | index into the predecessor's window; else a byte
constexpr uint32_t kGzrDefaultChunk = 16384;
constexpr uint64_t kGzrNone = ~0ull;
constexpr uint64_t kGzrMaxOut = 1ull << 31;              // payload of one call (a chunk that holds more cannot be emitted)
enum { kGzrStopCandidate = 0, kGzrStopFinal = 1, kGzrStopInput = 2, kGzrStopError = 3 };

// ---------------------------------------------------------------------------------------------------------------- member header
// The header of the member that begins at byte(0): SFGPU_BGZF_OK and *hdr_len (where the DEFLATE stream begins),
// SFGPU_BGZF_BAD_HEADER, or kBgzNeedMore when `avail` bytes do not reach the end of the header.
template <typename Byte>
SF_BGZ_HD int gzr_parse_header(Byte byte, uint64_t avail, uint64_t* hdr_len) {
    if (avail >= 1 && byte(0) != 0x1f) return SFGPU_BGZF_BAD_HEADER;
    if (avail >= 2 && byte(1) != 0x8b) return SFGPU_BGZF_BAD_HEADER;
    if (avail >= 3 && byte(2) != 8) return SFGPU_BGZF_BAD_HEADER;
    if (avail >= 4 && (byte(3) & 0xe0u)) return SFGPU_BGZF_BAD_HEADER;
    if (avail < 10) return kBgzNeedMore;
    const uint32_t flg = byte(3);
    uint64_t p = 10;
    if (flg & 4u) {                                                      // FEXTRA
        if (p + 2 > avail) return kBgzNeedMore;
        p += 2u + ((uint32_t)byte(p) | ((uint32_t)byte(p + 1) << 8));
        if (p > avail) return kBgzNeedMore;
    }
    for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {                     // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        for (;;) {
            if (p >= avail) return kBgzNeedMore;
            if (byte(p++) == 0) break;
        }
    }
    if (flg & 2u) p += 2;                                                // FHCRC
    if (p > avail) return kBgzNeedMore;
    *hdr_len = p;
    return SFGPU_BGZF_OK;
}

// ---------------------------------------------------------------------------------------------------------------- block headers
SF_BGZ_HD uint64_t gzr_bit_pos(const BgzBits& bits) { return (uint64_t)bits.next * 8u - bits.nbits; }

#define SF_GZR_SYMBOL(fast, fb, symtab, cnt, out_sym)                                   \
    do {                                                                                \
        const uint32_t e_ = io.uniform(bgz_decode(bits.peek15(), fast, fb, symtab, cnt));           \
        if (e_ == 0u || (int64_t)(e_ & 15u) > bits.left) return fail(bits.left < 15 ? SFGPU_BGZF_TRUNCATED : SFGPU_BGZF_BAD_SYMBOL); \
        uint32_t drop_;                                                                 \
        bits.take(e_ & 15u, &drop_);                                                    \
        out_sym = e_ >> 4;                                                              \
    } while (0)
#define SF_GZR_TAKE(n, v) do { if (!bits.take(n, &(v))) return fail(SFGPU_BGZF_TRUNCATED); } while (0)

// The header of a dynamic block behind its three type bits, into T's literal/length and distance tables: bgz_inflate_body's
// statements for BTYPE 2.  IO is the policy described there (word, uniform, single, status, store_len).
template <typename IO>
SF_BGZ_HD int gzr_dyn_header(IO& io, BgzTables* T, BgzBits& bits) {
    auto fail = [](int kind) -> int { return kind; };
    uint32_t hlit, hdist, hclen;
    bits.fill(io);
    SF_GZR_TAKE(5, hlit); SF_GZR_TAKE(5, hdist); SF_GZR_TAKE(4, hclen);
    hlit += 257u; hdist += 1u; hclen += 4u;
    if (hlit > 286u || hdist > 30u) return SFGPU_BGZF_BAD_CODE_LENGTHS;
    for (uint32_t i = 0; i < (uint32_t)kBgzClSyms; ++i) {
        uint32_t v = 0;
        if (i < hclen) { bits.fill(io); SF_GZR_TAKE(3, v); }
        io.store_len(T, (uint32_t)gz_cl_order((int)i), v);
    }
    io.single([&]() {
        T->status = bgz_build_table(T->lens, kBgzClSyms, kBgzCodes, T->cl_fast, kBgzClFastBits, T->cl_sym, T->cl_count, T->offs) ? 1 : 0;
    });
    if (!io.status(T)) return SFGPU_BGZF_BAD_CODE_LENGTHS;
    const uint32_t total = hlit + hdist;
    uint32_t prev = 0;
    for (uint32_t i = 0; i < total;) {
        bits.fill(io);
        uint32_t s;
        SF_GZR_SYMBOL(T->cl_fast, kBgzClFastBits, T->cl_sym, T->cl_count, s);
        if (s < 16u) {
            io.store_len(T, i < hlit ? i : kBgzLitSyms + (i - hlit), s);
            prev = s; ++i;
            continue;
        }
        uint32_t rep, v = 0;
        if (s == 16u) {
            if (i == 0u) return SFGPU_BGZF_BAD_CODE_LENGTHS;
            SF_GZR_TAKE(2, rep); rep += 3u; v = prev;
        } else if (s == 17u) {
            SF_GZR_TAKE(3, rep); rep += 3u;
        } else {
            SF_GZR_TAKE(7, rep); rep += 11u;
        }
        if (i + rep > total) return SFGPU_BGZF_BAD_CODE_LENGTHS;
        for (uint32_t k = 0; k < rep; ++k, ++i) io.store_len(T, i < hlit ? i : kBgzLitSyms + (i - hlit), v);
        prev = v;
    }
    for (uint32_t i = hlit; i < (uint32_t)kBgzLitSyms; ++i) io.store_len(T, i, 0u);
    for (uint32_t i = hdist; i < (uint32_t)kBgzDistSyms; ++i) io.store_len(T, kBgzLitSyms + i, 0u);
    io.single([&]() {
        bool ok = T->lens[kGzEob] != 0;                    // zlib: "missing end-of-block", checked before the tables
        ok = ok && bgz_build_table(T->lens, kBgzLitSyms, kBgzLens, T->lit_fast, kBgzLitFastBits, T->lit_sym, T->lit_count, T->offs);
        ok = ok && bgz_build_table(T->lens + kBgzLitSyms, kBgzDistSyms, kBgzDists, T->dist_fast, kBgzDistFastBits, T->dist_sym,
                                   T->dist_count, T->offs);
        T->status = ok ? 1 : 0;
    });
    if (!io.status(T)) return SFGPU_BGZF_BAD_CODE_LENGTHS;
    return SFGPU_BGZF_OK;
}

template <typename IO>
SF_BGZ_HD void gzr_fixed_tables(IO& io, BgzTables* T) {
    io.single([&]() {
        for (int s = 0; s < kBgzLitSyms; ++s) T->lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
        for (int s = 0; s < kBgzDistSyms; ++s) T->lens[kBgzLitSyms + s] = 5;
        bgz_build_table(T->lens, kBgzLitSyms, kBgzLens, T->lit_fast, kBgzLitFastBits, T->lit_sym, T->lit_count, T->offs);
        bgz_build_table(T->lens + kBgzLitSyms, kBgzDistSyms, kBgzDists, T->dist_fast, kBgzDistFastBits, T->dist_sym, T->dist_count, T->offs);
    });
}

// ---------------------------------------------------------------------------------------------------------------- the finder
// The cheap part at bit q of the call's n_bits bits; word(p) as in BgzBits (p a multiple of 4; bytes behind the input read as
// anything: no bit behind n_bits is looked at).  Necessary for gzr_header_at, so the candidates do not depend on it.
template <typename Word>
SF_BGZ_HD bool gzr_cheap_test(Word word, uint64_t q, uint64_t n_bits) {
    if (q + 17u > n_bits) return false;
    const uint32_t p = (uint32_t)(q >> 5) * 4u, sh = (uint32_t)q & 31u;
    const uint64_t a = (uint64_t)word(p) | ((uint64_t)word(p + 4u) << 32), b = (uint64_t)word(p + 8u) | ((uint64_t)word(p + 12u) << 32);
    const uint64_t lo = sh ? (a >> sh) | (b << (64u - sh)) : a, hi = b >> sh;      // bits q .. q + 64, q + 64 .. q + 128 - sh
    if ((lo & 7u) != 4u) return false;                                              // BFINAL 0, BTYPE 2 (its low bit first)
    if (((lo >> 3) & 31u) > 29u || ((lo >> 8) & 31u) > 29u) return false;           // HLIT + 257 <= 286, HDIST + 1 <= 30
    const uint32_t hclen = (uint32_t)((lo >> 13) & 15u) + 4u;
    if (q + 17u + 3u * hclen > n_bits) return false;
    uint32_t kraft = 0;                                                             // in units of 2^-7
    for (uint32_t i = 0; i < hclen; ++i) {
        const uint32_t at = 17u + 3u * i;
        const uint64_t w = at < 64u ? (lo >> at) | (at > 61u ? hi << (64u - at) : 0ull) : hi >> (at - 64u);
        const uint32_t l = (uint32_t)w & 7u;
        if (l) kraft += 128u >> l;
    }
    return kraft == 128u;
}

// The full part: does the decoder accept a dynamic block header at bit q of src[0 .. n_bytes)?
template <typename IO>
SF_BGZ_HD bool gzr_header_at(IO& io, BgzTables* T, uint64_t q, uint32_t n_bytes) {
    BgzBits bits;
    bits.seek(io, (uint32_t)(q >> 3), n_bytes);
    uint32_t v;
    if (!bits.take((uint32_t)q & 7u, &v)) return false;
    bits.fill(io);
    if (!bits.take(3u, &v) || v != 4u) return false;
    return gzr_dyn_header(io, T, bits) == SFGPU_BGZF_OK;
}

// the span that holds bit b: spans are chunk_bytes of input counted from the byte in which the call's decode starts
SF_BGZ_HD uint64_t gzr_span_of(uint64_t b, uint64_t start_byte, uint32_t chunk_bytes) { return ((b >> 3) - start_byte) / chunk_bytes; }

// pass A's stop rule: is the boundary b a candidate?  cand[s] = the candidate of span s or kGzrNone (cand[0] is never one)
SF_BGZ_HD bool gzr_is_candidate(const uint64_t* cand, uint64_t n_spans, uint64_t b, uint64_t start_byte, uint32_t chunk_bytes) {
    const uint64_t s = gzr_span_of(b, start_byte, chunk_bytes);
    return s >= 1u && s < n_spans && cand[s] == b;
}

// ---------------------------------------------------------------------------------------------------------------- the decoder
struct GzrChunkRec {
    uint64_t end_bit;         // the boundary at which the chunk stopped (behind a final block: the byte boundary in front of the trailer)
    uint64_t n_out;           // output up to there
    uint32_t blocks[3];       // stored, fixed, dynamic up to there
    int32_t status;           // kGzrStop*
    int32_t kind;             // SFGPU_BGZF_* when status is kGzrStopError
    uint32_t pad_;
};

// One chunk: the blocks from start_bit of src[0 .. n_bytes) until stop(boundary) says so, a final block ends, the input ends or a
// check fails.  `reach` = how far a match may reach before the chunk's first byte (pass A: the whole ring; pass B: the valid
// length of the resolved window).  IO is bgz_inflate_body's policy with 64-bit output positions:
//   put(o, b)  copy(o, dist, len)  stored(o, p, len)      pass A: into the ring at o & kGzrMask; pass B: bytes, o - dist < 0 is the window
template <typename IO, typename Stop>
SF_BGZ_HD int gzr_decode_chunk(IO& io, BgzTables* T, uint64_t start_bit, uint32_t n_bytes, uint32_t reach, Stop stop, GzrChunkRec* rec) {
    BgzBits bits;
    bits.seek(io, (uint32_t)(start_bit >> 3), n_bytes);
    uint64_t o = 0, c_bit = start_bit, c_o = 0;            // c_*: the last boundary the chunk completed
    uint32_t n_stored = 0, n_fixed = 0, n_dynamic = 0, c_stored = 0, c_fixed = 0, c_dynamic = 0;
    auto done = [&](int status, int kind) -> int {
        rec->end_bit = c_bit; rec->n_out = c_o;
        rec->blocks[0] = c_stored; rec->blocks[1] = c_fixed; rec->blocks[2] = c_dynamic;
        rec->status = status; rec->kind = kind; rec->pad_ = 0;
        return kind;
    };
    // the input ending inside a block is no error of the chunk: it stops at the last boundary
    auto fail = [&](int kind) -> int { return kind == SFGPU_BGZF_TRUNCATED ? done(kGzrStopInput, SFGPU_BGZF_OK) : done(kGzrStopError, kind); };
    {
        uint32_t skip;
        SF_GZR_TAKE((uint32_t)start_bit & 7u, skip);
    }
    for (;;) {
        bits.fill(io);
        uint32_t bfinal, btype;
        SF_GZR_TAKE(1, bfinal);
        SF_GZR_TAKE(2, btype);
        if (btype == 3u) return fail(SFGPU_BGZF_BAD_BLOCK_TYPE);
        n_stored += btype == 0u; n_fixed += btype == 1u; n_dynamic += btype == 2u;
        if (btype == 0u) {
            uint32_t pad, len, nlen;
            SF_GZR_TAKE(bits.nbits & 7u, pad);
            bits.fill(io);
            SF_GZR_TAKE(16, len);
            SF_GZR_TAKE(16, nlen);
            if (len != (nlen ^ 0xffffu)) return fail(SFGPU_BGZF_STORED_LEN);
            if ((int64_t)len * 8 > bits.left) return fail(SFGPU_BGZF_TRUNCATED);
            const uint32_t p = bits.byte_pos();
            io.stored(o, p, len);
            o += len;
            bits.seek(io, p + len, n_bytes);
        } else {
            if (btype == 1u) {
                gzr_fixed_tables(io, T);
            } else {
                const int k = gzr_dyn_header(io, T, bits);
                if (k != SFGPU_BGZF_OK) return fail(k);
            }
            for (;;) {
                bits.fill(io);
                uint32_t s;
                SF_GZR_SYMBOL(T->lit_fast, kBgzLitFastBits, T->lit_sym, T->lit_count, s);
                if (s < 256u) {
                    io.put(o, s);
                    ++o;
                    continue;
                }
                if (s == (uint32_t)kGzEob) break;
                if (s > 285u) return fail(SFGPU_BGZF_BAD_SYMBOL);
                uint32_t base, extra, ev, len, dist;
                bgz_len_base(s, &base, &extra);
                SF_GZR_TAKE(extra, ev);
                len = base + ev;
                bits.fill(io);
                SF_GZR_SYMBOL(T->dist_fast, kBgzDistFastBits, T->dist_sym, T->dist_count, s);
                if (s > 29u) return fail(SFGPU_BGZF_BAD_SYMBOL);
                bgz_dist_base(s, &base, &extra);
                SF_GZR_TAKE(extra, ev);
                dist = base + ev;
                if ((uint64_t)dist > o + reach) return fail(SFGPU_BGZF_DISTANCE_TOO_FAR);
                io.copy(o, dist, len);
                o += len;
            }
        }
        if (bfinal) {
            uint32_t pad;
            bits.take(bits.nbits & 7u, &pad);
            const uint32_t end = bits.byte_pos();
            if ((uint64_t)end + kBgzTrailer > n_bytes) return fail(SFGPU_BGZF_TRUNCATED);      // the member ends where its trailer is at hand
            c_bit = (uint64_t)end * 8u; c_o = o; c_stored = n_stored; c_fixed = n_fixed; c_dynamic = n_dynamic;
            return done(kGzrStopFinal, SFGPU_BGZF_OK);
        }
        c_bit = gzr_bit_pos(bits); c_o = o; c_stored = n_stored; c_fixed = n_fixed; c_dynamic = n_dynamic;
        if (io.uniform(stop(c_bit) ? 1u : 0u)) return done(kGzrStopCandidate, SFGPU_BGZF_OK);
    }
}
#undef SF_GZR_SYMBOL
#undef SF_GZR_TAKE

// window propagation, one entry: byte j of the window behind a chunk of n_out symbols, from its ring and its predecessor's
// resolved window
template <typename Ring, typename Prev>
SF_BGZ_HD uint32_t gzr_resolve(Ring ring, Prev prev, uint64_t n_out, uint32_t j) {
    const uint32_t v = ring((uint32_t)(n_out + j) & kGzrMask);
    return (v & kGzrMarker) ? prev(v & kGzrMask) : v;
}

// the carried window: byte j of the last 32 KB emitted, the old window in front when fewer than 32 KB were
template <typename Old, typename Out>
SF_BGZ_HD uint32_t gzr_carry(Old old, Out out, uint64_t n_out, uint32_t j) {
    return n_out >= kGzrWindow ? out(n_out - kGzrWindow + j) : (j + n_out < kGzrWindow ? old(j + (uint32_t)n_out) : out(j + n_out - kGzrWindow));
}

// ---------------------------------------------------------------------------------------------------------------- the call
struct GzrState {             // what a handle carries from call to call (and the 32 KB window)
    int32_t in_member;        // the bit position lies inside a member's DEFLATE stream
    uint32_t bit;             // 0 .. 7: the bit of the first unconsumed byte at which the next block begins
    uint32_t crc;             // of the member's payload so far
    uint32_t valid;           // bytes of the carried window that belong to this member
    uint64_t len;             // payload bytes of the member so far
    uint64_t members;         // members finished
};

struct GzrStart {
    int32_t kind;             // SFGPU_BGZF_OK, BAD_HEADER or TRUNCATED (at byte `at`)
    int32_t decode;           // there is a stream to decode from start_bit
    int32_t begins_member;    // ... which is a member's first block: the window is empty
    uint64_t at;              // where the padding ends: the header (or the end of the input)
    uint64_t start_bit;
};

// Zero bytes behind a member are padding, as Python's gzip treats them; anything else that is not a gzip header is BAD_HEADER.
inline GzrStart gzr_call_start(const GzrState& st, const uint8_t* src, uint64_t n, int final) {
    GzrStart s{SFGPU_BGZF_OK, 0, 0, 0, 0};
    if (st.in_member) {
        if (n == 0) { if (final) s.kind = SFGPU_BGZF_TRUNCATED; return s; }
        s.decode = 1; s.start_bit = st.bit;
        return s;
    }
    uint64_t p = 0;
    if (st.members) while (p < n && src[p] == 0) ++p;
    s.at = p;
    if (p == n) return s;
    uint64_t hdr_len = 0;
    const int k = gzr_parse_header([&](uint64_t q) -> uint32_t { return src[p + q]; }, n - p, &hdr_len);
    if (k == kBgzNeedMore) { if (final) s.kind = SFGPU_BGZF_TRUNCATED; return s; }
    if (k != SFGPU_BGZF_OK) { s.kind = k; return s; }
    s.decode = 1; s.begins_member = 1; s.start_bit = (p + hdr_len) * 8u;
    return s;
}

struct GzrChain {
    std::vector<uint32_t> span;          // the call's chunks: their spans ...
    std::vector<uint64_t> out_off;       // ... and where their output begins
    uint64_t n_out = 0, end_bit = 0, n_false = 0, need_cap = 0, error_bit = 0;
    uint64_t blocks[3] = {0, 0, 0};
    int32_t member_end = 0, error_kind = SFGPU_BGZF_OK;
};

// cand[s] / rec[s]: the candidate of span s and what pass A found from it (s = 0: from start_bit)
inline GzrChain gzr_chain(const uint64_t* cand, const GzrChunkRec* rec, uint64_t n_spans, uint64_t start_bit, uint32_t chunk_bytes, int final,
                          uint64_t cap) {
    GzrChain c;
    if (cap > kGzrMaxOut) cap = kGzrMaxOut;
    const uint64_t start_byte = start_bit >> 3;
    uint64_t s = 0, at = start_bit, reached = 0;
    bool taking = true;
    c.end_bit = start_bit;
    uint64_t walked_end = start_bit;
    for (;;) {
        const GzrChunkRec& r = rec[s];
        const bool starved = r.status == kGzrStopInput && (final || r.end_bit == at);
        if (r.status == kGzrStopError || starved) {
            if (taking && (r.status == kGzrStopError || final)) { c.error_kind = r.status == kGzrStopError ? r.kind : SFGPU_BGZF_TRUNCATED; c.error_bit = at; }
            break;
        }
        if (taking && r.n_out > cap - c.n_out) {
            if (c.span.empty()) c.need_cap = r.n_out;
            taking = false;
        }
        if (taking) {
            c.span.push_back((uint32_t)s); c.out_off.push_back(c.n_out);
            c.n_out += r.n_out; c.end_bit = r.end_bit;
            for (int t = 0; t < 3; ++t) c.blocks[t] += r.blocks[t];
            if (r.status == kGzrStopFinal) c.member_end = 1;
        }
        if (s) ++reached;
        walked_end = r.end_bit;
        if (r.status != kGzrStopCandidate) break;
        at = r.end_bit;
        s = gzr_span_of(at, start_byte, chunk_bytes);
    }
    for (uint64_t k = 1; k < n_spans; ++k) if (cand[k] != kGzrNone && cand[k] < walked_end) ++c.n_false;
    c.n_false -= reached < c.n_false ? reached : c.n_false;
    return c;
}

// Behind pass B: the chunks' CRCs in order onto the running CRC and length; with member_end the trailer's words are compared.
// Returns the kind; *st is what the next call starts from (unchanged when nothing was emitted and no member began).
inline int gzr_finish_call(GzrState* st, const GzrStart& start, const GzrChain& c, const GzrChunkRec* rec, const uint32_t* crcs,
                           uint32_t crc_stored, uint32_t isize) {
    if (c.span.empty()) return SFGPU_BGZF_OK;
    if (start.begins_member) { st->in_member = 1; st->crc = 0; st->len = 0; st->valid = 0; }
    for (size_t k = 0; k < c.span.size(); ++k) {
        const uint64_t n = rec[c.span[k]].n_out;
        st->crc = crc32_combine(st->crc, crcs[k], n);
        st->len += n;
    }
    st->valid = (uint32_t)(c.n_out + st->valid < kGzrWindow ? c.n_out + st->valid : kGzrWindow);
    st->bit = (uint32_t)c.end_bit & 7u;
    if (!c.member_end) return SFGPU_BGZF_OK;
    st->in_member = 0; st->bit = 0; st->members++;
    if (st->crc != crc_stored) return SFGPU_BGZF_CRC_MISMATCH;
    if ((uint32_t)st->len != isize) return SFGPU_BGZF_SIZE_MISMATCH;
    return SFGPU_BGZF_OK;
}

// whole bytes of the call's input that the caller may drop after the emit
inline uint64_t gzr_consumed(const GzrStart& start, const GzrChain& c) {
    if (c.span.empty()) return start.at;
    return c.member_end ? (c.end_bit >> 3) + kBgzTrailer : c.end_bit >> 3;
}

// ---------------------------------------------------------------------------------------------------------------- serial
struct GzrSerialIO {
    const uint8_t* src; uint32_t n;
    uint16_t* ring;           // pass A (else null)
    uint8_t* out;             // pass B: the chunk's payload
    const uint8_t* win;       // pass B: the resolved window in front of it
    uint32_t word(uint32_t p) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4u; ++k) if ((uint64_t)p + k < n) v |= (uint32_t)src[p + k] << (8u * k);
        return v;
    }
    uint32_t uniform(uint32_t v) const { return v; }
    template <typename F> void single(F f) const { f(); }
    bool status(const BgzTables* T) const { return T->status != 0; }
    void store_len(BgzTables* T, uint32_t i, uint32_t v) const { T->lens[i] = (uint8_t)v; }
    void put(uint64_t o, uint32_t b) const { if (ring) ring[o & kGzrMask] = (uint16_t)b; else out[o] = (uint8_t)b; }
    void copy(uint64_t o, uint32_t dist, uint32_t len) const {
        for (uint32_t i = 0; i < len; ++i) {
            if (ring) { ring[(o + i) & kGzrMask] = ring[(o + i - dist) & kGzrMask]; continue; }
            const int64_t from = (int64_t)(o + i) - (int64_t)dist;
            out[o + i] = from < 0 ? win[(int64_t)kGzrWindow + from] : out[from];
        }
    }
    void stored(uint64_t o, uint32_t p, uint32_t len) const {
        for (uint32_t i = 0; i < len; ++i) { if (ring) ring[(o + i) & kGzrMask] = src[p + i]; else out[o + i] = src[p + i]; }
    }
};

}  // namespace sfgpu
