// verifyfmt.h -- what it means to verify a hit record against the transcript's bases, stated once.  Plain C++, host and device,
// serial: verify.hip runs the same functions inside its kernels, tests/verify_harness.cpp runs them alone (vf_serial_verify below),
// and hits.verify_hits_host is the Python statement both are judged by.
//
// JOB      one mate of one record: mate_status 0 / 1 -> mate 1's bases on strand `fwd` at `pos`; 2 -> mate 2's bases on strand `fwd`
//          at `pos`; 3 -> two jobs: mate 1, `fwd`, `pos`, then mate 2, `mate_fwd`, `mate_pos`.  len = the mate's length from the reads'
//          offsets (NOT the record's 16-bit read_len / mate_len, which truncate).
// BASES    oriented base j of the mate: forward code(r[j]); reverse 3 - code(r[len - 1 - j]); code = the mapper's base_code (A C G T in
//          either case -> 0 1 2 3, anything else 4, which stays 4 on either strand).  Transcript base at x = pos + j: x < 0 or
//          x >= ref_len[tid] is OFF the transcript (`over`); otherwise the bases are compared: a MISMATCH (`mism`) when either code
//          is 4 or the codes differ.
// PASS     a job passes iff 1000 * (len - over - mism) >= min_identity_permille * len (64-bit integers); a record passes iff all its
//          jobs pass (a pair stands or falls as a whole).
// BEST     keep_best: of a read's passing records only those whose cost -- mism + over summed over the record's jobs, unsaturated -- is
//          the read's minimum survive.
// ORDER    survivors keep their order; the offsets are CSR over the same reads.
// SCORE    per survivor {mism, over, mate_mism, mate_over}, 16 bits each, saturating at 65 535; the mate fields are 0 unless the
//          status is 3.  Pass / fail and the cost use the unsaturated counts.
// ERRORS   a record with tid >= M fails the whole call (the lowest such record is named); nothing is emitted.
//
// The kernels do not walk a job byte by byte: a lane takes kVfStep oriented bases at a time from each text with one unaligned
// 16-byte load, clipped to the text (vf_window), and classifies them in registers (vf_classify).  Both ways of counting are stated
// here -- vf_job_serial and vf_job_windows -- and the harness holds them against each other and against the Python statement.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/sfgpu.h"

#if !defined(__HIPCC__)
#include <vector>
#endif

#if defined(__HIPCC__)
#define VF_HD __host__ __device__ __forceinline__
#else
#define VF_HD inline
#endif

namespace sfgpu {

constexpr uint32_t kVfStep = 16;                  // bases a lane takes per step: one 16-byte load from each text

VF_HD uint32_t vf_code(unsigned char b) {
    const unsigned char u = b & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}
VF_HD uint32_t vf_oriented(uint32_t code, bool fwd) { return code > 3u ? 4u : (fwd ? code : 3u - code); }

struct VfCount { uint64_t mism, over; };

// jobs of a record: 1 or 2; job j reads mate (0 = mate 1, 1 = mate 2) on strand fwd at pos
struct VfJob { uint32_t mate; bool fwd; int32_t pos; };
VF_HD uint32_t vf_n_jobs(const sfgpu_hit& h) { return h.mate_status == 3 ? 2u : 1u; }
VF_HD VfJob vf_job(const sfgpu_hit& h, uint32_t j) {
    if (j == 1u) return VfJob{1u, h.mate_fwd != 0, h.mate_pos};
    return VfJob{h.mate_status == 2 ? 1u : 0u, h.fwd != 0, h.pos};
}

VF_HD bool vf_passes(uint64_t len, uint64_t mism, uint64_t over, uint32_t permille) {
    return 1000ull * (len - over - mism) >= (uint64_t)permille * len;
}
VF_HD uint16_t vf_sat16(uint64_t v) { return v > 65535ull ? (uint16_t)65535u : (uint16_t)v; }

// ---- byte by byte ---------------------------------------------------------------------------------------------------------------
VF_HD VfCount vf_job_serial(const char* r, uint64_t len, bool fwd, const char* t, uint64_t tlen, int64_t pos) {
    VfCount c{0, 0};
    for (uint64_t j = 0; j < len; ++j) {
        const int64_t x = pos + (int64_t)j;
        if (x < 0 || x >= (int64_t)tlen) { ++c.over; continue; }
        const uint32_t a = vf_oriented(vf_code((unsigned char)(fwd ? r[j] : r[len - 1 - j])), fwd);
        const uint32_t b = vf_code((unsigned char)t[x]);
        if (a > 3u || b > 3u || a != b) ++c.mism;
    }
    return c;
}

// ---- sixteen bases at a time ----------------------------------------------------------------------------------------------------
struct VfWin { uint64_t lo, hi; };                // bytes 0 .. 7 and 8 .. 15 of a window, little-endian

// bytes s .. s + 15 of text[0 .. n): one 16-byte load that never leaves the text (its start is pulled inside, the bytes then shifted
// into place); positions outside the text read as 0.  Texts of fewer than 16 bytes are gathered byte by byte.
VF_HD VfWin vf_window(const char* text, int64_t n, int64_t s) {
    VfWin w{0, 0};
    if (s >= n || s + 16 <= 0) return w;
    if (n < 16) {
        for (int i = 0; i < 16; ++i) {
            const int64_t x = s + i;
            if (x < 0 || x >= n) continue;
            const uint64_t b = (unsigned char)text[x];
            if (i < 8) w.lo |= b << (8 * i); else w.hi |= b << (8 * (i - 8));
        }
        return w;
    }
    const int64_t a = s < 0 ? 0 : (s > n - 16 ? n - 16 : s);
    uint64_t v[2];
    memcpy(v, text + a, 16);
    const int d = (int)(s - a);                   // > 0: the window runs past the end; < 0: it begins in front of the text
    uint64_t lo = v[0], hi = v[1];
    if (d > 0) {                                  // byte i <- byte i + d
        if (d < 8) { lo = (lo >> (8 * d)) | (hi << (64 - 8 * d)); hi >>= 8 * d; }
        else { lo = hi >> (8 * (d - 8)); hi = 0; }
    } else if (d < 0) {                           // byte i <- byte i - e
        const int e = -d;
        if (e < 8) { hi = (hi << (8 * e)) | (lo >> (64 - 8 * e)); lo <<= 8 * e; }
        else { hi = lo << (8 * (e - 8)); lo = 0; }
    }
    w.lo = lo; w.hi = hi;
    return w;
}
VF_HD uint64_t vf_bswap64(uint64_t v) {
    v = ((v & 0x00FF00FF00FF00FFull) << 8) | ((v >> 8) & 0x00FF00FF00FF00FFull);
    v = ((v & 0x0000FFFF0000FFFFull) << 16) | ((v >> 16) & 0x0000FFFF0000FFFFull);
    return (v << 32) | (v >> 32);
}
// oriented bases j0 .. j0 + 15 of the mate as raw bytes in oriented order: on the reverse strand the mate is read downwards from
// its end (raw bytes len - j0 - 16 .. len - j0 - 1, reversed); the complement is taken when the bytes are classified
VF_HD VfWin vf_mate_window(const char* r, int64_t len, bool fwd, int64_t j0) {
    if (fwd) return vf_window(r, len, j0);
    const VfWin w = vf_window(r, len, len - j0 - 16);
    return VfWin{vf_bswap64(w.hi), vf_bswap64(w.lo)};
}
// four window bytes at a time.  x: the mate's bytes, y: the transcript's, case folded (b & 0xDF, as vf_code folds); comp_xor /
// comp_mul: 0x15151515 / 0x11 on the reverse strand, 0 / 0 on the forward strand -- A <-> T is ^ 0x15, C <-> G is ^ 0x04, and C and
// G are the letters with bit 1 set.  A mate's byte is a base iff it equals the letter rebuilt from its bits 1 .. 2 (A 00, C 01, G 11
// -> 0x41 | bits; T 10 -> 0x54).  -> 0x80 in every byte that is NOT (a base and equal to the transcript's byte)
VF_HD uint32_t vf_differ4(uint32_t x, uint32_t y, uint32_t comp_xor, uint32_t comp_mul) {
    const uint32_t a = x & 0xDFDFDFDFu, b = y & 0xDFDFDFDFu;
    const uint32_t is_t = (a >> 2) & ~(a >> 1) & 0x01010101u;
    const uint32_t canon = (0x41414141u | (a & 0x06060606u)) ^ (is_t * 0x11u);
    const uint32_t oriented = a ^ comp_xor ^ (((a >> 1) & 0x01010101u) * comp_mul);
    const uint32_t d = (a ^ canon) | (oriented ^ b);                              // a byte is 0 iff the base is one and matches
    return (((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;
}
// bits 4 k .. 4 k + 3 of `bits` -> 0x80 in bytes 0 .. 3
VF_HD uint32_t vf_spread4(uint32_t bits, int k) { return ((((bits >> (4 * k)) & 0xFu) * 0x00204081u) & 0x01010101u) << 7; }
VF_HD uint32_t vf_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}
// counts of oriented bases j0 .. j0 + 15 (those < len) against transcript positions pos + j
VF_HD VfCount vf_classify(VfWin m, VfWin t, bool fwd, int64_t j0, int64_t len, int64_t pos, int64_t tlen) {
    const int64_t x0 = pos + j0;                  // transcript position of the window's first base
    const int n = len - j0 < 16 ? (int)(len - j0) : 16;                            // bases of the mate in the window
    const int lo = x0 >= 0 ? 0 : (x0 <= -16 ? 16 : (int)-x0);                      // window bytes lo .. hi - 1 lie on the transcript
    const int hi = tlen - x0 >= 16 ? 16 : (tlen - x0 <= 0 ? 0 : (int)(tlen - x0));
    const int a = lo < n ? lo : n, b0 = hi < n ? hi : n, b = b0 > a ? b0 : a;      // bytes a .. b - 1: of the mate and on the transcript
    const uint32_t on = ((1u << b) - 1u) & ~((1u << a) - 1u);
    const uint32_t cx = fwd ? 0u : 0x15151515u, cm = fwd ? 0u : 0x11u;
    const uint32_t mw[4] = {(uint32_t)m.lo, (uint32_t)(m.lo >> 32), (uint32_t)m.hi, (uint32_t)(m.hi >> 32)};
    const uint32_t tw[4] = {(uint32_t)t.lo, (uint32_t)(t.lo >> 32), (uint32_t)t.hi, (uint32_t)(t.hi >> 32)};
    uint32_t mism = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) mism += vf_popc(vf_differ4(mw[k], tw[k], cx, cm) & vf_spread4(on, k));
    return VfCount{mism, (uint64_t)(n - (b - a))};
}
// what lane `lane` of a group of `lanes` counts of a job: windows lane, lane + lanes, ... of kVfStep bases
VF_HD VfCount vf_job_lane(const char* r, uint64_t len, bool fwd, const char* t, uint64_t tlen, int64_t pos, uint32_t lane, uint32_t lanes) {
    VfCount c{0, 0};
    for (uint64_t j0 = (uint64_t)lane * kVfStep; j0 < len; j0 += (uint64_t)lanes * kVfStep) {
        const VfWin m = vf_mate_window(r, (int64_t)len, fwd, (int64_t)j0);
        const VfWin w = vf_window(t, (int64_t)tlen, pos + (int64_t)j0);
        const VfCount k = vf_classify(m, w, fwd, (int64_t)j0, (int64_t)len, pos, (int64_t)tlen);
        c.mism += k.mism; c.over += k.over;
    }
    return c;
}
VF_HD VfCount vf_job_windows(const char* r, uint64_t len, bool fwd, const char* t, uint64_t tlen, int64_t pos, uint32_t lanes) {
    VfCount c{0, 0};
    for (uint32_t l = 0; l < lanes; ++l) {
        const VfCount k = vf_job_lane(r, len, fwd, t, tlen, pos, l, lanes);
        c.mism += k.mism; c.over += k.over;
    }
    return c;
}

// ---- a record -------------------------------------------------------------------------------------------------------------------
struct VfRecord { sfgpu_hit_score score; uint64_t cost, mism; bool pass; };       // mism: over the record's jobs, unsaturated
VF_HD VfRecord vf_record(const sfgpu_hit& h, const VfCount* job /* [vf_n_jobs] */, const uint64_t* len /* [vf_n_jobs] */, uint32_t permille) {
    VfRecord out;
    const uint32_t nj = vf_n_jobs(h);
    out.pass = true; out.cost = 0; out.mism = 0;
    for (uint32_t j = 0; j < nj; ++j) {
        out.pass = out.pass && vf_passes(len[j], job[j].mism, job[j].over, permille);
        out.cost += job[j].mism + job[j].over;
        out.mism += job[j].mism;
    }
    out.score.mism = vf_sat16(job[0].mism); out.score.over = vf_sat16(job[0].over);
    out.score.mate_mism = nj > 1 ? vf_sat16(job[1].mism) : (uint16_t)0; out.score.mate_over = nj > 1 ? vf_sat16(job[1].over) : (uint16_t)0;
    return out;
}

#if !defined(__HIPCC__)
// ---- a batch on the host: what the serial passes of this header, verifygfmt.h and aligngfmt.h walk -------------------------------
struct VfBatch {
    const char* tseq; const uint64_t* tseq_off; const uint32_t* tlen; uint64_t M;
    const char* seq1; const uint64_t* off1; const char* seq2; const uint64_t* off2;
    uint32_t n_reads; const sfgpu_hit* hits; const uint32_t* hit_off;
    uint64_t n_rec() const { return n_reads ? hit_off[n_reads] : 0; }
};
// 1 + the lowest record with tid >= M, or 0
inline uint64_t vf_bad_tid(const VfBatch& b) {
    for (uint64_t i = 0; i < b.n_rec(); ++i) if (b.hits[i].tid >= b.M) return i + 1;
    return 0;
}
// every job of the batch in order: fn(read, record, job index, mate, len, transcript, tlen, fwd, pos).  Each text is handed over on
// its own, in a block of exactly its length: a sanitizer sees every byte read outside it
template <typename Fn>
inline void vf_each_job(const VfBatch& b, Fn&& fn) {
    for (uint32_t r = 0; r < b.n_reads; ++r)
        for (uint32_t i = b.hit_off[r]; i < b.hit_off[r + 1]; ++i) {
            const sfgpu_hit& h = b.hits[i];
            for (uint32_t j = 0; j < vf_n_jobs(h); ++j) {
                const VfJob jb = vf_job(h, j);
                const uint64_t* off = jb.mate ? b.off2 : b.off1;
                const char* m = (jb.mate ? b.seq2 : b.seq1) + off[r];
                const std::vector<char> mate(m, m + (off[r + 1] - off[r])), tx(b.tseq + b.tseq_off[h.tid], b.tseq + b.tseq_off[h.tid] + b.tlen[h.tid]);
                fn(r, i, j, mate.data(), (uint64_t)mate.size(), tx.data(), (uint64_t)tx.size(), jb.fwd, (int64_t)jb.pos);
            }
        }
}
// PASS, BEST, ORDER and the stats both verification passes share, over the batch's records as scored (rec[i]: VfRecord or verifygfmt.h's
// VgRecord); kept(record, stats) adds what a survivor means to the pass's own stats
template <typename Record, typename Score, typename Stats, typename Kept>
inline void vf_select(const VfBatch& b, const std::vector<Record>& rec, bool keep_best, std::vector<sfgpu_hit>* out_hits, std::vector<uint32_t>* out_off,
                      std::vector<Score>* out_scores, Stats* stats, Kept&& kept) {
    *stats = Stats{};
    out_hits->clear(); out_scores->clear(); out_off->assign(1, 0u);
    stats->records_in = b.n_rec();
    for (uint32_t r = 0; r < b.n_reads; ++r) {
        uint64_t best = ~0ull;
        for (uint32_t i = b.hit_off[r]; i < b.hit_off[r + 1]; ++i) if (rec[i].pass && rec[i].cost < best) best = rec[i].cost;
        const size_t before = out_hits->size();
        for (uint32_t i = b.hit_off[r]; i < b.hit_off[r + 1]; ++i) {
            const Record& v = rec[i];
            if (!v.pass) { ++stats->failed_identity; continue; }
            if (keep_best && v.cost != best) { ++stats->dropped_not_best; continue; }
            out_hits->push_back(b.hits[i]); out_scores->push_back(v.score);
            kept(v, stats);
        }
        stats->reads_in += b.hit_off[r + 1] > b.hit_off[r];
        stats->reads_out += out_hits->size() > before;
        out_off->push_back((uint32_t)out_hits->size());
    }
    stats->records_out = out_hits->size();
}

// the whole pass, serially (windows = false: byte by byte; true: as a group of `lanes` lanes counts).  -> 0, or 1 + the lowest record
// with tid >= M (nothing is emitted then)
inline uint64_t vf_serial_verify(const char* tseq, const uint64_t* tseq_off, const uint32_t* tlen, uint64_t M, const char* seq1, const uint64_t* off1,
                                 const char* seq2, const uint64_t* off2, uint32_t n_reads, const sfgpu_hit* hits, const uint32_t* hit_off,
                                 uint32_t permille, bool keep_best, bool windows, uint32_t lanes, std::vector<sfgpu_hit>* out_hits,
                                 std::vector<uint32_t>* out_off, std::vector<sfgpu_hit_score>* out_scores, sfgpu_verify_stats* stats) {
    const VfBatch b{tseq, tseq_off, tlen, M, seq1, off1, seq2, off2, n_reads, hits, hit_off};
    if (const uint64_t bad = vf_bad_tid(b)) return bad;
    std::vector<VfRecord> rec(b.n_rec());
    VfCount job[2]; uint64_t len[2];
    vf_each_job(b, [&](uint32_t, uint32_t i, uint32_t j, const char* mate, uint64_t n, const char* tx, uint64_t tl, bool fwd, int64_t pos) {
        if (j == 0) { job[0] = job[1] = VfCount{0, 0}; len[0] = len[1] = 0; }
        len[j] = n;
        job[j] = windows ? vf_job_windows(mate, n, fwd, tx, tl, pos, lanes) : vf_job_serial(mate, n, fwd, tx, tl, pos);
        if (j + 1u == vf_n_jobs(b.hits[i])) rec[i] = vf_record(b.hits[i], job, len, permille);
    });
    vf_select(b, rec, keep_best, out_hits, out_off, out_scores, stats, [](const VfRecord& v, sfgpu_verify_stats* st) { st->sum_mism += v.mism; });
    return 0;
}
#endif

}  // namespace sfgpu
