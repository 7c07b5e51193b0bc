// samtext_write.hip -- the mapper's hit records as SAM alignment lines, formatted on the device from the CSR batch where it
// lies: sfgpu_sam_write_text, the mirror of samtext.hip.  WHAT a line says is samwfmt.h (the bytes of samfile._sam_text); this
// file finds where every line lies and writes it.
//
// A UNIT is what one hit record (one line, or the two lines of a pair record) or one read without records (its 4 line, or its
// 77 / 141 lines) produces.  Units are numbered in file order: the unit of hit h of read r is h + e(r), that of a record-less
// read r is hit_off[r] + e(r), with e(r) = the record-less reads in front of r.  No unit is empty, chunks end between units.
//   sizing  k_read_flags marks the record-less reads (and checks the offsets); an exclusive scan gives e.  k_record_size: one
//           lane per hit record finds its read in the CSR offsets (binary search), checks the record (samw_check: the lowest
//           offender of either kind wins an atomicMin) and writes the bytes of its unit; k_empty_size: one lane per read writes
//           the bytes of its record-less unit.  An exclusive scan (primitives.h) gives every unit its 64-bit byte start.
//           textchunks.h: the longest unit and the greedy chunk ends.
//           The quality rule (every byte in '!' .. '~') is one flat pass over each mate's bytes (k_qual_check); the lowest
//           offending byte is mapped to its read through the offsets.
//   format  k_format_units<Fmt, ZW>: one block per 4 KB tile of the output (texttile.h).  The units that overlap the tile are found
//           by binary search of the unit starts (a unit may span many tiles: SEQ is of any length).  One lane per line has Fmt
//           write it into the LDS image, clipped to the tile: the numeric parts and every run (a name, SEQ, QUAL) of at most
//           kShortCopy bytes by that lane; longer runs are queued as jobs, clipped to the tile, and made a byte per lane and step,
//           the block's wavefronts taking the jobs in turn.  Then every lane stores one aligned 16-byte group.
//           TextFmt is samwfmt.h's line: runs are copied, never inspected, on a line that goes on the reference's strand (oriented
//           != 0) from the last byte to the first, SEQ through samw_comp.  BamFmt is bamwfmt.h's record: SEQ packed two bases a
//           byte, QUAL 0xff or the quality bytes - 33.  The sizing kernels take the format as their template argument BAM.
// The chunks are planned by textchunks.h and go to the sink (sfgpu_sam_write_text*), on the device to the BGZF encoder of
// bgzf_write.hip (sfgpu_sam_write_bgzf*), or all at once into bamsort.hip's record store (sfgpu_bamsort_collect*).
#include "common.h"
#include "decfmt.h"
#include "primitives.h"
#include "samwfmt.h"
#include "bamwfmt.h"
#include "texttile.h"
#include "bamsort.h"

#include <cstring>

namespace sfgpu {
namespace {

using textchunks::kBlock;
using textchunks::kTileBytes;
using textchunks::kTileShift;
using textchunks::kDefaultChunk;
using textchunks::kMaxChunk;
using textchunks::grid_of;

constexpr uint32_t kShortCopy = 48;                       // longer names and SEQs are copied by whole wavefronts
// A run (QNAME, RNAME, SEQ or QUAL of a text line; name, packed SEQ or QUAL of a BAM record; forward or reversed alike) is queued
// as a job only when it is longer than kShortCopy bytes OF OUTPUT, and the runs of all lines are disjoint ranges of the output.
// A job is the part of one run inside one tile, at most one per run and tile.  Runs that lie whole in a tile take at least
// kShortCopy + 1 of its kTileBytes bytes each: at most kTileBytes / (kShortCopy + 1) of them; a run that does not lie whole in it
// covers its first or its last byte, and disjoint runs cannot share either: two more.  How many KINDS of run a line has -- QUAL
// adds one -- does not enter.  The `k < kJobCap` tests below can therefore not drop a job.
constexpr uint32_t kJobCap = kTileBytes / (kShortCopy + 1) + 3;
constexpr unsigned long long kNoError = ~0ull;

enum : unsigned long long { kBadOffsets = 1, kTooLong = 2, kNullBytes = 4 };
// misc: [0] flags, [1] longest unit, [2] lowest (read << 32 | record) that breaks the position rule, [3] ... whose tid is no
// reference, [4] lines, [5 .. 7] the lowest (read << 32 | record) that breaks bamwfmt.h's rules 3 .. 5 (BAM records only),
// [8] the lowest read << 32 with a quality byte outside '!' .. '~'
constexpr int kMisc = 9;
constexpr int kMiscQual = 8;
__device__ inline int misc_of_kind(int kind) { return kind <= SAMW_BAD_TID ? 1 + kind : 2 + kind; }

// offsets off[0 .. n] of `bytes`: kBadOffsets where they decrease (or are negative), kNullBytes where bytes are named but absent
template <typename Off>
__global__ void k_check_off(const void* __restrict__ bytes, const Off* __restrict__ off, uint64_t n, unsigned long long* __restrict__ misc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Off a = off[i], b = off[i + 1];
    if (a > b || a < (Off)0) atomicOr(&misc[0], kBadOffsets);
    else if (b > a && !bytes) atomicOr(&misc[0], kNullBytes);
}

// One lane per 16 quality bytes q[lo .. hi) of a mate (offsets off[0 .. n_reads], checked): the lowest byte outside '!' .. '~'
// names its read -- the last r with off[r] <= byte, the reads of 0 bases in front of it skipped -- as (r, record 0)
__global__ void k_qual_check(const uint8_t* __restrict__ q, const int64_t* __restrict__ off, uint32_t n_reads, int64_t lo, int64_t hi,
                             unsigned long long* __restrict__ misc) {
    const int64_t p0 = lo + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (p0 >= hi) return;
    const int64_t p1 = p0 + 16 < hi ? p0 + 16 : hi;
    int64_t bad = -1;
    if (p1 - p0 == 16 && ((reinterpret_cast<uintptr_t>(q) + (uint64_t)p0) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(q + p0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 15; k >= 0; --k) if (!samw_qual_ok((uint8_t)(w[k >> 2] >> (8 * (k & 3))))) bad = p0 + k;
    } else {
        for (int64_t p = p1 - 1; p >= p0; --p) if (!samw_qual_ok(q[p])) bad = p;
    }
    if (bad < 0) return;
    atomicMin(&misc[kMiscQual], (unsigned long long)(textchunks::holder_of(off, n_reads, bad) << 32));
}

// empty[r] = 1 for a read without records; the CSR offsets start at 0 and never decrease
__global__ void k_read_flags(const uint32_t* __restrict__ hit_off, uint32_t n_reads, uint32_t* __restrict__ empty,
                             unsigned long long* __restrict__ misc) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t a = hit_off[r], b = hit_off[r + 1];
    if (a > b || (r == 0 && a != 0)) atomicOr(&misc[0], kBadOffsets);
    empty[r] = a == b;
}

__device__ inline void count_lines(uint32_t n, unsigned long long* __restrict__ misc) {
    unsigned long long v = n;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & (kWave - 1)) == 0 && v) atomicAdd(&misc[4], v);
}

// A batch without posteriors runs the instantiations with ZW == false, which drop the two pointers at once: the compiler then removes
// the field's code, and those kernels are what they were before the field existed (registers and occupancy included).
template <bool ZW> __device__ __forceinline__ void without_zw(SamwArgs& a) {
    if (!ZW) { a.tag_zw_rec = nullptr; a.tag_zw_f32 = nullptr; }
}

// BAM: the units are bamwfmt.h's records (one per line) with its checks behind samwfmt.h's, else the text's lines
template <bool BAM, bool ZW>
__global__ void __launch_bounds__(kBlock)
k_record_size(SamwArgs a, uint64_t n_hits, const uint32_t* __restrict__ e_before, uint32_t* __restrict__ unit_len,
              uint32_t* __restrict__ unit_read, unsigned long long* __restrict__ misc) {
    without_zw<ZW>(a);
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t lines = 0;
    if (h < n_hits) {
        const uint64_t r = textchunks::holder_of(a.hit_off, a.n_reads, h);      // the last read whose records start at or before h
        const uint64_t rank = h - a.hit_off[r], u = h + e_before[r];
        const sfgpu_hit rec = a.hits[h];
        uint64_t len = 0;
        if (const int kind = BAM ? bamw_check(a, r, &rec, rank, h) : samw_check_a(a, rec, h))
            atomicMin(&misc[misc_of_kind(kind)], (unsigned long long)(r << 32 | rank));
        else len = BAM ? bamw_unit_len(a, r, &rec, rank, h) : samw_unit_len(a, r, &rec, rank, h);
        if (len > 0xffffffffull) { atomicOr(&misc[0], kTooLong); len = 0; }
        unit_len[u] = (uint32_t)len;
        unit_read[u] = (uint32_t)r;
        lines = samw_record_lines(rec);
    }
    count_lines(lines, misc);
}

template <bool BAM>
__global__ void __launch_bounds__(kBlock)
k_empty_size(SamwArgs a, const uint32_t* __restrict__ e_before, uint32_t* __restrict__ unit_len, uint32_t* __restrict__ unit_read,
             unsigned long long* __restrict__ misc) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t lines = 0;
    if (r < a.n_reads && a.hit_off[r] == a.hit_off[r + 1]) {
        const uint64_t u = (uint64_t)a.hit_off[r] + e_before[r];
        uint64_t len = 0;
        if (const int kind = BAM ? bamw_check(a, r, nullptr, 0) : 0) atomicMin(&misc[misc_of_kind(kind)], (unsigned long long)(r << 32));
        else len = BAM ? bamw_unit_len(a, r, nullptr, 0) : samw_unit_len(a, r, nullptr, 0);
        if (len > 0xffffffffull) { atomicOr(&misc[0], kTooLong); len = 0; }
        unit_len[u] = (uint32_t)len;
        unit_read[u] = (uint32_t)r;
        lines = samw_empty_lines(a.paired != 0);
    }
    count_lines(lines, misc);
}

// ---- format: one skeleton, k_format_units<Fmt>, for text lines (TextFmt) and BAM records (BamFmt)
// A RUN is a stretch of a line whose bytes are a function of a source array: byte i of a run of `kind` over src, of which `left`
// source units count, is Fmt::run_byte(kind, src, left, i).  A kind with kReversed set reads its source from the last unit to the first.
// A run cut by the tile's start is the run of the same kind over fewer units: `skip` output bytes use up skip * Fmt::units(kind) of
// them, from the front on a forward kind (src moves up), from the back on a reversed one (src stays where it is).
constexpr uint32_t kReversed = 4;
struct Job {
    const uint8_t* src;     // the source of the first byte that lies in the tile; a reversed kind: the run's first source unit
    uint32_t at, n;         // tile offset and bytes
    uint32_t kind, left;    // the source units from src on that count
};

// what the skeleton knows of a line when a format writes it
struct LineCtx {
    uint64_t r, rank, hidx; // the read; the record's rank among its read's records and its index in a.hits (0, 0: the read has none)
    uint32_t tid, which;
    SamwLine l;
    uint64_t s, len;        // the line's first byte in the text, and its bytes (Fmt::line_len)
};

// where a format puts a line's pieces, one after the other; `p` is the tile offset of the next byte, before or behind the tile or in it
template <typename Fmt>
struct LineOut {
    const textchunks::Tile& tile;
    Job* jobs;
    uint32_t* n_jobs;
    int64_t p;
    __device__ __forceinline__ void put(int i, uint8_t b) const { tile.put(p + i, (char)b); }     // byte i from here on; skip() then passes them
    __device__ __forceinline__ void skip(uint64_t n) { p += (int64_t)n; }
    __device__ __forceinline__ void byte(uint8_t b) { tile.put(p++, (char)b); }
    // the n bytes of a run: by this lane when short, else its part inside the tile is queued for the wavefronts
    __device__ __forceinline__ void run(uint32_t kind, const uint8_t* src, uint64_t n, uint64_t left) {
        if (n <= kShortCopy) {
            for (uint32_t i = 0; i < (uint32_t)n; ++i) tile.put(p + i, (char)Fmt::run_byte(kind, src, (uint32_t)left, i));
        } else {
            const int64_t room = (int64_t)(tile.end() - tile.base), lo = p > 0 ? p : 0, hi = p + (int64_t)n < room ? p + (int64_t)n : room;
            if (lo < hi) {
                const uint32_t k = atomicAdd(n_jobs, 1u);
                const uint64_t used = (uint64_t)(lo - p) * Fmt::units(kind);
                if (k < kJobCap) jobs[k] = Job{kind & kReversed ? src : src + used, (uint32_t)lo, (uint32_t)(hi - lo), kind, (uint32_t)(left - used)};
            }
        }
        p += (int64_t)n;
    }
};

// samwfmt.h's line: names, SEQ and QUAL are runs of bytes as given, or -- on a line that goes on the reference's strand -- from the
// last byte to the first, SEQ through samw_comp
struct TextFmt {
    enum : uint32_t { kCopy = 0, kCopyRev = kReversed, kCompRev = kReversed | 1 };
    static __device__ __forceinline__ uint32_t units(uint32_t) { return 1; }
    static __device__ __forceinline__ uint8_t run_byte(uint32_t kind, const uint8_t* __restrict__ src, uint32_t left, uint32_t i) {
        switch (kind) {
            case kCopy: return src[i];
            case kCopyRev: return src[left - 1 - i];
            default: return samw_comp(src[left - 1 - i]);
        }
    }
    static __device__ __forceinline__ uint64_t line_len(const SamwArgs& a, const SamwLine& l, uint64_t r, uint32_t tid) { return samw_line_len(a, l, r, tid); }
    static __device__ __forceinline__ void emit(const SamwArgs& a, const LineCtx& c, LineOut<TextFmt>& out) {
        auto put = [&](int i, char ch) { out.put(i, (uint8_t)ch); };
        if (a.qname_off) {
            const uint64_t o = a.qname_off[c.r], n = a.qname_off[c.r + 1] - o;
            out.run(kCopy, reinterpret_cast<const uint8_t*>(a.qnames) + o, n, n);
        } else {
            samw_put_default_qname(a.read_index_base + c.r, put);
            out.skip(samw_default_qname_len(a.read_index_base + c.r));
        }
        samw_put_head(c.l, put);                          // \t FLAG \t
        out.skip(samw_head_len(c.l));
        if (c.l.mapped) {
            const uint64_t o = a.ref_name_off[c.tid], n = a.ref_name_off[c.tid + 1] - o;
            out.run(kCopy, reinterpret_cast<const uint8_t*>(a.ref_names) + o, n, n);
        } else out.byte('*');
        samw_put_mid(c.l, put);                           // \t POS \t 255 \t CIGAR \t RNEXT \t PNEXT \t TLEN \t
        out.skip(samw_mid_len(c.l));
        const bool rev = samw_reversed(a, c.l);
        const uint8_t* src;
        uint64_t n;
        if (samw_seq(a, c.l, c.r, &src, &n)) out.run(rev ? kCompRev : kCopy, src, n, n);
        else out.byte('*');
        out.byte('\t');
        if (samw_qual(a, c.l, c.r, &src, &n)) out.run(rev ? kCopyRev : kCopy, src, n, n);
        else out.byte('*');
        SamwTags t;
        if (samw_tags(a, c.l, c.r, &t)) {                 // \t NM:i:<nm> \t MD:Z:<md> \t NH:i:<nh>; a long MD is a run like a name
            out.skip(samw_put_int_tag('N', 'M', t.nm, put));
            samw_put_md_lead(put);
            out.skip(kSamwTagLead);
            out.run(kCopy, t.md, t.md_len, t.md_len);
            out.skip(samw_put_int_tag('N', 'H', t.nh, put));
        }
        uint32_t zw;
        if (samw_zw(a, c.l, &zw)) out.skip(samw_put_zw(zw, put));     // \t ZW:f:<token>
        out.byte('\n');
    }
};

// bamwfmt.h's record: the 36 fixed bytes, the NUL and the CIGAR words by the line's lane; the name is a run copied, SEQ a run of
// bytes packed from two bases each, QUAL a run of 0xff or of the quality bytes - 33.  A packed run's units are bases: a reversed
// one cut by the tile's start keeps its parity, so the one packed byte with a 0 low nibble stays the last.
struct BamFmt {
    enum : uint32_t { kCopy = 0, kQual = 1, kFill = 2, kPack = 3, kQualRev = kReversed | kQual, kPackRev = kReversed | kPack };
    static __device__ __forceinline__ uint32_t units(uint32_t kind) { return (kind & 3u) == kPack ? 2u : 1u; }
    static __device__ __forceinline__ uint8_t run_byte(uint32_t kind, const uint8_t* __restrict__ src, uint32_t left, uint32_t i) {
        switch (kind) {
            case kCopy: return src[i];
            case kPack: return bamw_packed_byte(src, left, i);
            case kQual: return (uint8_t)(src[i] - 33u);
            case kPackRev: return bamw_packed_byte_rev(src, left, i);
            case kQualRev: return (uint8_t)(src[left - 1 - i] - 33u);
            default: return (uint8_t)0xff;
        }
    }
    static __device__ __forceinline__ uint64_t line_len(const SamwArgs& a, const SamwLine& l, uint64_t r, uint32_t) { return bamw_line_len(a, l, r); }
    static __device__ __forceinline__ void emit(const SamwArgs& a, const LineCtx& c, LineOut<BamFmt>& out) {
        auto put = [&](int i, uint8_t b) { out.put(i, b); };
        const uint64_t qn = samw_qname_len(a, c.r);
        const uint8_t* seq;
        const uint64_t n_bases = bamw_l_seq(a, c.l, c.r, &seq);
        bamw_put_fixed(c.l, c.tid, c.len, qn, n_bases, put);
        out.skip(kBamwFixed);
        if (a.qname_off) out.run(kCopy, reinterpret_cast<const uint8_t*>(a.qnames) + a.qname_off[c.r], qn, qn);
        else {
            samw_put_default_qname(a.read_index_base + c.r, [&](int i, char ch) { out.put(i, (uint8_t)ch); });
            out.skip(qn);
        }
        out.byte(0);
        bamw_put_cigar(c.l, put);
        out.skip(4 * bamw_cigar_ops(c.l));
        const bool rev = samw_reversed(a, c.l);
        out.run(rev ? kPackRev : kPack, seq, (n_bases + 1) / 2, n_bases);
        const uint8_t* qual;
        uint64_t ql;
        if (samw_qual(a, c.l, c.r, &qual, &ql)) out.run(rev ? kQualRev : kQual, qual, n_bases, n_bases);
        else out.run(kFill, seq, n_bases, n_bases);       // (the source of a kFill run is never read)
        SamwTags t;
        if (samw_tags(a, c.l, c.r, &t)) {                 // NM <t> <nm> | MD Z <md> NUL | NH <t> <nh>
            out.skip(bamw_put_int_tag('N', 'M', t.nm, put));
            out.byte('M'); out.byte('D'); out.byte('Z');
            out.run(kCopy, t.md, t.md_len, t.md_len);
            out.byte(0);
            out.skip(bamw_put_int_tag('N', 'H', t.nh, put));
        }
        for (uint32_t i = 0; i < bamw_zw_len(a, c.l); ++i) out.byte(bamw_zw_byte(a, c.l, i));    // Z W f <float>
    }
};

// One block per tile of the output; `out` is the chunk buffer, whose byte 0 is text byte out_base (a multiple of kTileBytes).  The
// units that overlap the tile are found by binary search of the unit starts (units are never empty, so the starts increase strictly).
// Two line slots per unit, a lane each: a unit's second line is absent unless it is a pair record or a record-less paired read.
// The lane of a line inside the tile has Fmt write it; then the wavefronts take the queued runs in turn, a byte per lane and step.
template <typename Fmt, bool ZW>
__global__ void __launch_bounds__(kBlock)
k_format_units(SamwArgs a, const uint32_t* __restrict__ e_before, const uint32_t* __restrict__ unit_read, const uint64_t* __restrict__ unit_start,
               uint64_t n_units, uint64_t n_bytes, uint64_t first_tile, uint64_t out_base, uint4* __restrict__ out) {
    __shared__ uint4 tile4[kBlock];
    __shared__ Job jobs[kJobCap];
    __shared__ uint32_t n_jobs;
    without_zw<ZW>(a);
    const textchunks::Tile tile(tile4, first_tile, n_bytes);
    if (threadIdx.x == 0) n_jobs = 0;
    __syncthreads();
    const uint64_t u_lo = textchunks::holder_of(unit_start, n_units, tile.base), u_hi = textchunks::holder_of(unit_start, n_units, tile.end() - 1);
    for (uint64_t slot = threadIdx.x; slot < 2 * (u_hi - u_lo + 1); slot += kBlock) {
        const uint64_t u = u_lo + (slot >> 1);
        LineCtx c;
        c.which = (uint32_t)(slot & 1);
        c.r = unit_read[u];
        c.rank = 0; c.hidx = 0;
        const uint32_t h0 = a.hit_off[c.r];
        const bool empty = h0 == a.hit_off[c.r + 1];
        sfgpu_hit rec = {};
        if (!empty) {
            c.hidx = u - e_before[c.r];
            rec = a.hits[c.hidx];
            c.rank = c.hidx - h0;
        }
        if (c.which >= (empty ? samw_empty_lines(a.paired != 0) : samw_record_lines(rec))) continue;
        c.tid = empty ? 0u : rec.tid;
        auto line = [&](uint32_t w) { return empty ? samw_empty_line(a.paired != 0, w) : samw_line(a, rec, c.rank, w, c.hidx); };
        c.s = unit_start[u];
        if (c.which) c.s += Fmt::line_len(a, line(0), c.r, c.tid);
        c.l = line(c.which);
        c.len = Fmt::line_len(a, c.l, c.r, c.tid);
        if (c.s >= tile.end() || c.s + c.len <= tile.base) continue;
        LineOut<Fmt> lo{tile, jobs, &n_jobs, (int64_t)(c.s - tile.base)};
        Fmt::emit(a, c, lo);
    }
    __syncthreads();
    const uint32_t nj = n_jobs < kJobCap ? n_jobs : kJobCap;
    const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    for (uint32_t k = wave; k < nj; k += kBlock / kWave) {
        const Job j = jobs[k];
        for (uint32_t i = lane; i < j.n; i += kWave) tile.bytes[j.at + i] = (char)Fmt::run_byte(j.kind, j.src, j.left, i);
    }
    __syncthreads();
    tile.store(out_base, out);
}

// the instantiation for a batch with (zw) or without posteriors
template <bool BAM> auto record_size_kernel(bool zw) { return zw ? k_record_size<BAM, true> : k_record_size<BAM, false>; }
template <typename Fmt> auto format_kernel(bool zw) { return zw ? k_format_units<Fmt, true> : k_format_units<Fmt, false>; }

struct Scratch {
    DevBuf<uint32_t> empty, e_before, unit_len, unit_read;
    DevBuf<uint64_t> unit_start;
    DevBuf<unsigned long long> misc;
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

namespace {

// where a batch goes: the chunks to a sink (sfgpu_sam_write_text*), to the BGZF encoder as text or as BAM records
// (sfgpu_sam_write_bgzf*), or every record at once into a store (sfgpu_bamsort_collect*; BAM)
struct Dest {
    sfgpu_text_sink sink = nullptr;
    void* user = nullptr;
    sfgpu_bgzw* z = nullptr;
    int format = SFGPU_SAMW_TEXT;
    BamRecordStore* store = nullptr;
};

// Everything up to the chunk loop is the same for every destination but for the kernels that size and check a unit.  `in` is the
// batch as the entry was given it; what a single-end batch does not use is dropped once the arguments are checked.
int sam_write(const char* who, const SamwArgs& in, uint64_t chunk_bytes, const Dest& dest, sfgpu_samwrite_result* out, sfgpu_stream stream) {
    const bool bam = dest.format == SFGPU_SAMW_BAM;
    const uint32_t n_reads = in.n_reads;
    auto fail = [&](int code, const char* what) -> int { set_error("%s: %s", who, what); return code; };
    if (!out) return fail(SFGPU_ERR_INVALID, "null result");
    memset(out, 0, sizeof(*out));
    if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
    if (!(chunk_bytes >= 16 && chunk_bytes <= kMaxChunk)) return fail(SFGPU_ERR_INVALID, "chunk_bytes must lie in [16, 2^30] (0 = default)");
    if (n_reads == 0) return SFGPU_OK;
    if (!in.hit_off) return fail(SFGPU_ERR_INVALID, "null hit offsets");
    if (!(in.ref_name_off || in.n_refs == 0)) return fail(SFGPU_ERR_INVALID, "null reference name offsets");
    if (!(!in.qnames || in.qname_off)) return fail(SFGPU_ERR_INVALID, "read names without their offsets");
    if (!((!in.seq1 || in.seq1_off) && (!in.seq2 || in.seq2_off))) return fail(SFGPU_ERR_INVALID, "bases without their offsets");
    if (!((!in.qual1 || in.seq1_off) && (!in.qual2 || in.seq2_off))) return fail(SFGPU_ERR_INVALID, "qualities of a mate whose bases are not given");
    if (!(n_reads < 0xffffffffu)) return fail(SFGPU_ERR_RANGE, "n_reads must be below 2^32 - 1");
    if (!((in.aln_pos != nullptr) == (in.aln_op_off != nullptr) && (!in.aln_ops || in.aln_pos))) return fail(SFGPU_ERR_INVALID, "an alignment is positions, offsets and operations together");
    if (!((in.tag_nm != nullptr) == (in.tag_md_off != nullptr) && (in.tag_nm != nullptr) == (in.tag_md != nullptr))) return fail(SFGPU_ERR_INVALID, "tags are nm, MD offsets and MD bytes together");
    if (in.tag_nm && !(in.seq1_off && (!in.paired || in.seq2_off))) return fail(SFGPU_ERR_INVALID, "tags of mates whose bases are not given");
    if ((in.tag_zw_rec != nullptr) != (in.tag_zw_f32 != nullptr)) return fail(SFGPU_ERR_INVALID, "posteriors are records and floats together");
    SamwArgs a = in;
    if (!a.paired) { a.seq2 = nullptr; a.seq2_off = nullptr; a.qual2 = nullptr; }
    a.oriented = a.oriented != 0;
    const bool zw = a.tag_zw_rec != nullptr;     // which instantiation of the sizing and format kernels runs

    Scratch S;
    CallScope scope;        // after S: it drains the stream before S's blocks go back to the pool
    hipStream_t st = nullptr;
    hipEvent_t ev_in = nullptr, ev_a[2] = {nullptr, nullptr}, ev_s[2] = {nullptr, nullptr};
    unsigned long long* h_misc = nullptr;     // [0 .. kMisc) misc, [kMisc] total bytes; uint32 view of [kMisc + 1]: n_hits, record-less reads;
                                              // [kMisc + 2 .. kMisc + 6): the first and the last base offset of either mate with qualities
    SF_HIP(scope.acquire(&st));
    SF_HIP(scope.event(&ev_in, hipEventDisableTiming));
    for (auto& e : ev_a) SF_HIP(scope.event(&e));
    for (auto& e : ev_s) SF_HIP(scope.event(&e));
    SF_HIP(scope.pinned_block(&h_misc, (kMisc + 6) * sizeof(unsigned long long)));
    // behind whatever the caller has queued on `stream`
    SF_HIP(hipEventRecord(ev_in, as_stream(stream)));
    SF_HIP(hipStreamWaitEvent(st, ev_in, 0));

    // ---- the arrays' shape: offsets that never decrease, the record-less reads, the number of units
    if (int rc = S.misc.reserve(kMisc, st, false)) return rc;
    if (int rc = S.empty.reserve((uint64_t)n_reads + 1, st, false)) return rc;
    if (int rc = S.e_before.reserve((uint64_t)n_reads + 1, st, false)) return rc;
    SF_HIP(hipMemsetAsync(S.misc.p, 0, kMisc * sizeof(unsigned long long), st));
    SF_HIP(hipMemsetAsync(S.misc.p + 2, 0xff, 2 * sizeof(unsigned long long), st));
    SF_HIP(hipMemsetAsync(S.misc.p + 5, 0xff, 4 * sizeof(unsigned long long), st));
    SF_HIP(hipEventRecord(ev_a[0], st));
    hipLaunchKernelGGL(k_read_flags, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, a.hit_off, n_reads, S.empty.p, S.misc.p);
    SF_HIP(hipGetLastError());
    if (a.n_refs) {
        hipLaunchKernelGGL(k_check_off<uint64_t>, dim3(grid_of(a.n_refs)), dim3(kBlock), 0, st, (const void*)a.ref_names, a.ref_name_off,
                           (uint64_t)a.n_refs, S.misc.p);
        SF_HIP(hipGetLastError());
    }
    if (a.qname_off) {
        hipLaunchKernelGGL(k_check_off<uint64_t>, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, (const void*)a.qnames, a.qname_off,
                           (uint64_t)n_reads, S.misc.p);
        SF_HIP(hipGetLastError());
    }
    for (int m = 0; m < 2; ++m) {
        const int64_t* off = m ? a.seq2_off : a.seq1_off;
        if (!off) continue;
        hipLaunchKernelGGL(k_check_off<int64_t>, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, (const void*)(m ? a.seq2 : a.seq1), off,
                           (uint64_t)n_reads, S.misc.p);
        SF_HIP(hipGetLastError());
    }
    if (int rc = exclusive_scan_u32_u32(S.empty.p, S.e_before.p, n_reads, st)) return rc;
    SF_HIP(hipEventRecord(ev_a[1], st));
    uint32_t* h_counts = reinterpret_cast<uint32_t*>(&h_misc[kMisc + 1]);
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_counts[0], a.hit_off + n_reads, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_counts[1], S.e_before.p + n_reads, 4, hipMemcpyDeviceToHost, st));
    int64_t* h_span = reinterpret_cast<int64_t*>(&h_misc[kMisc + 2]);
    for (int m = 0; m < 2; ++m) {
        if (!(m ? a.qual2 : a.qual1)) continue;
        const int64_t* off = m ? a.seq2_off : a.seq1_off;
        SF_HIP(hipMemcpyAsync(&h_span[2 * m], off, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(&h_span[2 * m + 1], off + n_reads, 8, hipMemcpyDeviceToHost, st));
    }
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&out->format_ms, ev_a[0], ev_a[1]);
    if (h_misc[0] & kBadOffsets) return fail(SFGPU_ERR_INVALID, "an offset array decreases, or the hit offsets do not start at 0");
    if (h_misc[0] & kNullBytes) return fail(SFGPU_ERR_INVALID, "offsets name bytes of a null array");
    const uint64_t n_hits = h_counts[0], n_units = n_hits + h_counts[1];
    if (n_hits && !a.hits) return fail(SFGPU_ERR_INVALID, "null hits");
    if (n_hits && a.aln_pos && !a.aln_ops) return fail(SFGPU_ERR_INVALID, "an alignment without operations");

    // ---- sizing and validation: unit lengths, unit starts, the longest unit, the lowest record that cannot be written
    if (int rc = S.unit_len.reserve(n_units + 1, st, false)) return rc;
    if (int rc = S.unit_read.reserve(n_units, st, false)) return rc;
    if (int rc = S.unit_start.reserve(n_units + 1, st, false)) return rc;
    SF_HIP(hipEventRecord(ev_s[0], st));
    for (int m = 0; m < 2; ++m) {                         // (the offsets are checked: they never decrease)
        const uint8_t* q = m ? a.qual2 : a.qual1;
        if (!q || h_span[2 * m + 1] <= h_span[2 * m]) continue;
        const uint64_t groups = ((uint64_t)(h_span[2 * m + 1] - h_span[2 * m]) + 15) / 16;
        hipLaunchKernelGGL(k_qual_check, dim3(grid_of(groups)), dim3(kBlock), 0, st, q, m ? a.seq2_off : a.seq1_off, n_reads, h_span[2 * m],
                           h_span[2 * m + 1], S.misc.p);
        SF_HIP(hipGetLastError());
    }
    if (n_hits) {
        hipLaunchKernelGGL(bam ? record_size_kernel<true>(zw) : record_size_kernel<false>(zw), dim3(grid_of(n_hits)), dim3(kBlock), 0, st, a, n_hits, S.e_before.p, S.unit_len.p, S.unit_read.p,
                           S.misc.p);
        SF_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(bam ? k_empty_size<true> : k_empty_size<false>, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, a, S.e_before.p, S.unit_len.p, S.unit_read.p, S.misc.p);
    SF_HIP(hipGetLastError());
    if (int rc = exclusive_scan_u32(S.unit_len.p, S.unit_start.p, n_units, st, false)) return rc;
    if (int rc = textchunks::line_max(S.unit_start.p, n_units, S.misc.p + 1, st)) return rc;
    SF_HIP(hipEventRecord(ev_s[1], st));
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, kMisc * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_misc[kMisc], S.unit_start.p + n_units, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&out->format_ms, ev_s[0], ev_s[1]);
    {   // the lowest (read, record) of any kind; one record breaking several rules reports the first, as samw_check / bamw_check do
        static const char* const kWhat[] = {"", "the read has no base on the transcript: SAM cannot say that", "the transcript id is not below n_refs",
                                            "the read name is not of 1 .. 254 bytes: BAM cannot say that",
                                            "the bases given differ in number from the read length, or are more than 65535",
                                            "the alignment ends beyond 2^29", "a quality byte is not in '!' .. '~'"};
        static const int kSlot[] = {0, 2, 3, 5, 6, 7, kMiscQual};
        int kind = 0;
        for (int k = 1; k <= SAMW_BAD_QUAL; ++k)
            if (h_misc[kSlot[k]] != kNoError && (!kind || h_misc[kSlot[k]] < h_misc[kSlot[kind]])) kind = k;
        if (kind) {
            const unsigned long long key = h_misc[kSlot[kind]];
            out->error_read = key >> 32; out->error_record = key & 0xffffffffull; out->error_kind = (uint32_t)kind;
            set_error("%s: read %llu, record %llu: %s", who, (unsigned long long)out->error_read, (unsigned long long)out->error_record, kWhat[kind]);
            return SFGPU_ERR_INVALID;
        }
    }
    if (h_misc[0] & kTooLong) return fail(SFGPU_ERR_RANGE, "a unit is longer than 2^32 - 1 bytes");
    const uint64_t total = h_misc[kMisc];
    out->n_bytes = total; out->n_lines = h_misc[4]; out->max_unit_bytes = h_misc[1];
    if (dest.store)            // sfgpu_bamsort_collect: every tile at once into a segment of the store, which then lists the records
        return dest.store->take(total, out->n_lines, S.unit_start.p, n_units, st, &out->format_ms, [&](uint4* buf, hipStream_t s) -> int {
            hipLaunchKernelGGL(format_kernel<BamFmt>(zw), dim3((unsigned)(((total - 1) >> kTileShift) + 1)), dim3(kBlock), 0, s, a, S.e_before.p, S.unit_read.p,
                               S.unit_start.p, n_units, total, (uint64_t)0, (uint64_t)0, buf);
            SF_HIP(hipGetLastError());
            return SFGPU_OK;
        });
    if (!dest.sink && !dest.z) return SFGPU_OK;
    if (out->max_unit_bytes > chunk_bytes) return fail(SFGPU_ERR_RANGE, "a unit (a line, or the two lines of a pair) is longer than chunk_bytes");

    // ---- the chunk plan and the format + copy + sink loop (textchunks.h), with this text's tiles
    textchunks::Stats ts;
    auto format_tiles = [&](uint64_t first_tile, uint64_t last_tile, uint64_t out_base, uint4* buf, hipStream_t s) -> int {
        hipLaunchKernelGGL(bam ? format_kernel<BamFmt>(zw) : format_kernel<TextFmt>(zw), dim3((unsigned)(last_tile - first_tile + 1)), dim3(kBlock), 0, s, a, S.e_before.p,
                           S.unit_read.p, S.unit_start.p, n_units, total, first_tile, out_base, buf);
        SF_HIP(hipGetLastError());
        return SFGPU_OK;
    };
    // the compressed formats: the chunk's device bytes go to the BGZF encoder, which copies and sinks what IT writes
    const int rc = dest.z ? textchunks::deliver_device(who, S.unit_start.p, n_units, total, chunk_bytes, st, &ts,
                                                  [&](const uint8_t* d_bytes, uint64_t n, hipStream_t ready) -> int {
                                                      return sfgpu_bgzw_write_device(dest.z, d_bytes, n, reinterpret_cast<sfgpu_stream>(ready));
                                                  }, format_tiles)
                     : textchunks::deliver(who, S.unit_start.p, n_units, total, chunk_bytes, dest.sink, dest.user, st, &ts, format_tiles);
    out->format_ms += ts.format_ms; out->d2h_ms = ts.d2h_ms; out->sink_ms = ts.sink_ms; out->n_chunks = ts.n_chunks;
    return rc;
}

}  // namespace

// ---- the entries: one per destination, each hands the batch to sam_write
extern "C" int sfgpu_sam_write_text(const sfgpu_samw_batch* batch, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
                                    sfgpu_samwrite_result* out, sfgpu_stream stream) {
    SF_REQUIRE(batch, SFGPU_ERR_INVALID, "sfgpu_sam_write_text: null batch");
    Dest dest;
    dest.sink = sink; dest.user = user;
    return sam_write("sfgpu_sam_write_text", *batch, chunk_bytes, dest, out, stream);
}

extern "C" int sfgpu_sam_write_bgzf(const sfgpu_samw_batch* batch, uint64_t chunk_bytes, sfgpu_bgzw* z, int format,
                                    sfgpu_samwrite_result* out, sfgpu_stream stream) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_sam_write_bgzf: null BGZF handle");
    SF_REQUIRE(format == SFGPU_SAMW_TEXT || format == SFGPU_SAMW_BAM, SFGPU_ERR_INVALID, "sfgpu_sam_write_bgzf: unknown format");
    SF_REQUIRE(batch, SFGPU_ERR_INVALID, "sfgpu_sam_write_bgzf: null batch");
    Dest dest;
    dest.z = z; dest.format = format;
    return sam_write("sfgpu_sam_write_bgzf", *batch, chunk_bytes, dest, out, stream);
}

// bamsort.h: the batch's BAM records, checked, sized and formatted as for sfgpu_sam_write_bgzf, into `store`
int sfgpu::samw_collect_bam(BamRecordStore* store, const SamwArgs& batch, sfgpu_samwrite_result* out, sfgpu_stream stream) {
    Dest dest;
    dest.store = store; dest.format = SFGPU_SAMW_BAM;
    return sam_write("sfgpu_bamsort_collect", batch, 0, dest, out, stream);
}
