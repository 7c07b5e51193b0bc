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
//   format  k_format: one block per 4 KB tile of the output.  The units that overlap the tile are found by binary search of the
//           unit starts (a unit may span many tiles: SEQ is of any length).  One lane per line writes the numeric parts, the
//           default QNAME and every name or SEQ of at most kShortCopy bytes into an LDS image of the tile, clipped to the tile;
//           longer names and SEQs are queued as copy jobs, clipped to the tile, and copied a byte per lane and step, the block's
//           wavefronts taking the jobs in turn.  Then every lane stores one aligned 16-byte group: global memory sees only
//           full-width coalesced stores.  Names are copied, never inspected; so are SEQ and QUAL but for the lines samwfmt.h puts
//           on the reference's strand (sfgpu_sam_write_text_q with oriented != 0): there output byte i of a run of n comes
//           from source byte n - 1 - i (SEQ through samw_comp), so a clipped job carries where its source ENDS and the lanes read
//           consecutive addresses downwards.  The quality rule (every byte in '!' .. '~') is one flat pass over each mate's bytes
//           in the sizing step (k_qual_check); the lowest offending byte is mapped to its read through the offsets.
// The chunks are planned and handed to the sink by textchunks.h, the loop of eqtext_write.hip and rowtext.h.
//
// sfgpu_sam_write_bgzf hands the chunks to the BGZF encoder (bgzf_write.hip) on the device instead, and with SFGPU_SAMW_BAM the
// lines are BAM records (WHAT a record says is bamwfmt.h): the same units, scan, tiles and chunks; the sizing kernels take the
// record sizes and bamwfmt.h's three further checks (template argument BAM), and k_format_bam builds a tile of records -- the
// fixed 36 bytes, NUL and CIGAR words by the line's lane, names copied, SEQ packed two bases a byte and QUAL filled with 0xff, or
// made of the quality bytes - 33, by whole wavefronts where they are longer than kShortCopy bytes of output; both from the last
// byte to the first on a line that goes on the reference's strand.
#include "common.h"
#include "decfmt.h"
#include "primitives.h"
#include "samwfmt.h"
#include "bamwfmt.h"
#include "textchunks.h"
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
    uint64_t a = 0, b = n_reads;                          // off[a] <= bad < off[b]
    while (b - a > 1) {
        const uint64_t mid = a + (b - a) / 2;
        if (off[mid] <= bad) a = mid; else b = mid;
    }
    atomicMin(&misc[kMiscQual], (unsigned long long)(a << 32));
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

// BAM: the units are bamwfmt.h's records (one per line) with its checks behind samwfmt.h's, else the text's lines
template <bool BAM>
__global__ void __launch_bounds__(kBlock)
k_record_size(SamwArgs a, uint64_t n_hits, const uint32_t* __restrict__ e_before, uint32_t* __restrict__ unit_len,
              uint32_t* __restrict__ unit_read, unsigned long long* __restrict__ misc) {
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t lines = 0;
    if (h < n_hits) {
        uint64_t lo = 0, hi = a.n_reads;                  // hit_off[lo] <= h < hit_off[hi]: the last such lo is the read that holds h
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (a.hit_off[mid] <= h) lo = mid; else hi = mid;
        }
        const uint64_t r = lo, rank = h - a.hit_off[r], u = h + e_before[r];
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

// the unit that holds byte x of the text (x < unit_start[n_units]); units are never empty, so the starts increase strictly
__device__ inline uint64_t unit_of(const uint64_t* __restrict__ unit_start, uint64_t n_units, uint64_t x) {
    uint64_t lo = 0, hi = n_units;                        // unit_start[lo] <= x < unit_start[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (unit_start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

struct CopyJob {
    const char* src;        // the source of the first byte that lies in the tile; a reversed job goes down from it
    uint32_t at, n;         // tile offset and bytes
    uint32_t mode;
};
enum : uint32_t { kFwd = 0, kRev = 1, kRevComp = 2 };    // as given; from the last byte to the first; that, complemented

// one block per tile of the output; `out` is the chunk buffer, whose byte 0 is text byte out_base (a multiple of kTileBytes)
__global__ void __launch_bounds__(kBlock)
k_format(SamwArgs a, const uint32_t* __restrict__ e_before, const uint32_t* __restrict__ unit_read, const uint64_t* __restrict__ unit_start,
         uint64_t n_units, uint64_t n_bytes, uint64_t first_tile, uint64_t out_base, uint4* __restrict__ out) {
    __shared__ uint4 tile4[kBlock];
    __shared__ CopyJob jobs[kJobCap];
    __shared__ uint32_t n_jobs;
    char* tile = reinterpret_cast<char*>(tile4);
    const uint64_t ti = first_tile + blockIdx.x, base = ti << kTileShift;
    tile4[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);      // (the bytes behind the end of the text)
    if (threadIdx.x == 0) n_jobs = 0;
    __syncthreads();
    const uint64_t end = base + kTileBytes < n_bytes ? base + kTileBytes : n_bytes;      // base < n_bytes: the grid ends with the chunk
    const uint64_t u_lo = unit_of(unit_start, n_units, base), u_hi = unit_of(unit_start, n_units, end - 1);
    auto put_at = [&](int64_t p, char ch) {               // tile offset p, which may lie before or behind the tile
        if (p >= 0 && p < (int64_t)kTileBytes) tile[p] = ch;
    };
    // bytes src[0 .. n) to text offset s: by this lane when short, else queued for the wavefronts (the part inside the tile)
    auto copy = [&](const char* src, uint64_t s, uint64_t n, uint32_t mode) {
        if (n <= kShortCopy) {
            const int64_t p0 = (int64_t)(s - base);
            if (mode == kFwd) for (uint32_t i = 0; i < (uint32_t)n; ++i) put_at(p0 + i, src[i]);
            else for (uint32_t i = 0; i < (uint32_t)n; ++i) put_at(p0 + i, mode == kRev ? src[n - 1 - i] : (char)samw_comp((uint8_t)src[n - 1 - i]));
            return;
        }
        const uint64_t lo = s > base ? s : base, hi = s + n < end ? s + n : end;
        if (lo >= hi) return;
        const uint32_t k = atomicAdd(&n_jobs, 1u);
        if (k < kJobCap) jobs[k] = CopyJob{mode == kFwd ? src + (lo - s) : src + (n - 1 - (lo - s)), (uint32_t)(lo - base), (uint32_t)(hi - lo), mode};
    };
    // two line slots per unit: a unit's second line is absent unless it is a pair record or a record-less paired read.  (With an
    // alignment given -- the _a entries -- a line's CIGAR is its slot's operations, put one after the other through put_at.)
    for (uint64_t slot = threadIdx.x; slot < 2 * (u_hi - u_lo + 1); slot += kBlock) {
        const uint64_t u = u_lo + (slot >> 1);
        const uint32_t which = (uint32_t)(slot & 1);
        const uint64_t r = unit_read[u];
        const uint32_t h0 = a.hit_off[r];
        const bool empty = h0 == a.hit_off[r + 1];
        sfgpu_hit rec = {};
        uint64_t rank = 0, h = 0;
        if (!empty) {
            h = u - e_before[r];
            rec = a.hits[h];
            rank = h - h0;
        }
        if (which >= (empty ? samw_empty_lines(a.paired != 0) : samw_record_lines(rec))) continue;
        const uint32_t tid = empty ? 0u : rec.tid;
        uint64_t s = unit_start[u];
        if (which) s += samw_line_len(a, empty ? samw_empty_line(a.paired != 0, 0) : samw_line(a, rec, rank, 0, h), r, tid);
        const SamwLine l = empty ? samw_empty_line(a.paired != 0, which) : samw_line(a, rec, rank, which, h);
        if (s >= end || s + samw_line_len(a, l, r, tid) <= base) continue;
        // QNAME
        if (a.qname_off) {
            const uint64_t o = a.qname_off[r], n = a.qname_off[r + 1] - o;
            copy(a.qnames + o, s, n, kFwd);
            s += n;
        } else {
            const int64_t p0 = (int64_t)(s - base);
            samw_put_default_qname(a.read_index_base + r, [&](int i, char ch) { put_at(p0 + i, ch); });
            s += samw_default_qname_len(a.read_index_base + r);
        }
        {   // \t FLAG \t
            const int64_t p0 = (int64_t)(s - base);
            samw_put_head(l, [&](int i, char ch) { put_at(p0 + i, ch); });
            s += samw_head_len(l);
        }
        // RNAME
        if (l.mapped) {
            const uint64_t o = a.ref_name_off[tid], n = a.ref_name_off[tid + 1] - o;
            copy(a.ref_names + o, s, n, kFwd);
            s += n;
        } else {
            put_at((int64_t)(s - base), '*');
            s += 1;
        }
        {   // \t POS \t 255 \t CIGAR \t RNEXT \t PNEXT \t TLEN \t
            const int64_t p0 = (int64_t)(s - base);
            samw_put_mid(l, [&](int i, char ch) { put_at(p0 + i, ch); });
            s += samw_mid_len(l);
        }
        // SEQ
        const uint8_t* seq;
        uint64_t sl;
        const bool rev = samw_reversed(a, l);
        if (samw_seq(a, l, r, &seq, &sl)) copy(reinterpret_cast<const char*>(seq), s, sl, rev ? kRevComp : kFwd);
        else put_at((int64_t)(s - base), '*');
        s += sl;
        put_at((int64_t)(s - base), '\t');
        s += 1;
        // QUAL
        if (samw_qual(a, l, r, &seq, &sl)) copy(reinterpret_cast<const char*>(seq), s, sl, rev ? kRev : kFwd);
        else put_at((int64_t)(s - base), '*');
        s += sl;
        put_at((int64_t)(s - base), '\n');
    }
    __syncthreads();
    // the long names, SEQs and QUALs: the wavefronts take the jobs in turn, a byte per lane and step
    const uint32_t nj = n_jobs < kJobCap ? n_jobs : kJobCap;
    const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    for (uint32_t k = wave; k < nj; k += kBlock / kWave) {
        const CopyJob j = jobs[k];
        if (j.mode == kFwd) for (uint32_t i = lane; i < j.n; i += kWave) tile[j.at + i] = j.src[i];
        else if (j.mode == kRev) for (uint32_t i = lane; i < j.n; i += kWave) tile[j.at + i] = *(j.src - i);
        else for (uint32_t i = lane; i < j.n; i += kWave) tile[j.at + i] = (char)samw_comp((uint8_t) * (j.src - i));
    }
    __syncthreads();
    const uint64_t g = base + 16ull * threadIdx.x;
    if (g < n_bytes) out[(g - out_base) >> 4] = tile4[threadIdx.x];
}

// ---- BAM records (bamwfmt.h): the same tiles, units and scan; a unit's lines are records
struct BamJob {
    const uint8_t* src;     // kCopy, kQual: the first byte that lies in the tile; kPack: the base of the first packed byte that does;
                            // the reversed kinds: the run's first source byte
    uint32_t at, n;         // tile offset and bytes
    uint32_t kind, left;    // kPack: the bases from src on; the reversed kinds: the source bytes not yet used up in front of the tile
};
// a name; bases packed; 0xff; qualities - 33; and the last two from the last source byte to the first (the bases complemented)
enum : uint32_t { kCopy = 0, kPack = 1, kFill = 2, kQual = 3, kPackRev = 4, kQualRev = 5 };

// byte i of a run of `kind` over src, of which `left` bytes count (kPack, kPackRev: bases; kQualRev: qualities)
__device__ __forceinline__ uint8_t bam_run_byte(uint32_t kind, const uint8_t* __restrict__ src, uint32_t left, uint32_t i) {
    switch (kind) {
        case kCopy: return src[i];
        case kPack: return bamw_packed_byte(src, left, i);
        case kQual: return (uint8_t)(src[i] - 33u);
        case kPackRev: return bamw_packed_byte_rev(src, left, i);
        case kQualRev: return (uint8_t)(src[left - 1 - i] - 33u);
        default: return (uint8_t)0xff;
    }
}

// k_format for BAM records.  One lane per record writes the 36 fixed bytes, the NUL, the CIGAR words, the default QNAME and
// every name, packed SEQ or QUAL run of at most kShortCopy bytes; longer ones are queued, clipped to the tile, and done by the
// wavefronts in turn, a byte per lane and step: a name copied, a packed byte made from its two bases, a QUAL byte set to 0xff or
// to its quality - 33.  A reversed run cut by the tile's start is the reversed run of fewer source bytes: skipping `skip` output
// bytes leaves the first n - skip qualities, or the first n_bases - 2 * skip bases (of the same parity, so the one packed byte
// with a 0 low nibble stays the last).
__global__ void __launch_bounds__(kBlock)
k_format_bam(SamwArgs a, const uint32_t* __restrict__ e_before, const uint32_t* __restrict__ unit_read, const uint64_t* __restrict__ unit_start,
             uint64_t n_units, uint64_t n_bytes, uint64_t first_tile, uint64_t out_base, uint4* __restrict__ out) {
    __shared__ uint4 tile4[kBlock];
    __shared__ BamJob jobs[kJobCap];
    __shared__ uint32_t n_jobs;
    uint8_t* tile = reinterpret_cast<uint8_t*>(tile4);
    const uint64_t ti = first_tile + blockIdx.x, base = ti << kTileShift;
    tile4[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    if (threadIdx.x == 0) n_jobs = 0;
    __syncthreads();
    const uint64_t end = base + kTileBytes < n_bytes ? base + kTileBytes : n_bytes;
    const uint64_t u_lo = unit_of(unit_start, n_units, base), u_hi = unit_of(unit_start, n_units, end - 1);
    auto put_at = [&](int64_t p, uint8_t b) {
        if (p >= 0 && p < (int64_t)kTileBytes) tile[p] = b;
    };
    // output bytes [s, s + n) of `kind` from src (kPack, kPackRev: n packed bytes of n_bases bases; kQualRev: n_bases = n)
    auto run = [&](uint32_t kind, const uint8_t* src, uint64_t s, uint64_t n, uint64_t n_bases) {
        if (n <= kShortCopy) {
            const int64_t p0 = (int64_t)(s - base);
            for (uint32_t i = 0; i < (uint32_t)n; ++i) put_at(p0 + i, bam_run_byte(kind, src, (uint32_t)n_bases, i));
            return;
        }
        const uint64_t lo = s > base ? s : base, hi = s + n < end ? s + n : end;
        if (lo >= hi) return;
        const uint32_t k = atomicAdd(&n_jobs, 1u);
        if (k >= kJobCap) return;
        const uint64_t skip = lo - s;
        const bool packed = kind == kPack || kind == kPackRev;
        jobs[k] = BamJob{kind == kCopy || kind == kQual ? src + skip : kind == kPack ? src + 2 * skip : src, (uint32_t)(lo - base), (uint32_t)(hi - lo),
                         kind, packed ? (uint32_t)(n_bases - 2 * skip) : kind == kQualRev ? (uint32_t)(n_bases - skip) : 0u};
    };
    for (uint64_t slot = threadIdx.x; slot < 2 * (u_hi - u_lo + 1); slot += kBlock) {
        const uint64_t u = u_lo + (slot >> 1);
        const uint32_t which = (uint32_t)(slot & 1);
        const uint64_t r = unit_read[u];
        const uint32_t h0 = a.hit_off[r];
        const bool empty = h0 == a.hit_off[r + 1];
        sfgpu_hit rec = {};
        uint64_t rank = 0, h = 0;
        if (!empty) {
            h = u - e_before[r];
            rec = a.hits[h];
            rank = h - h0;
        }
        if (which >= (empty ? samw_empty_lines(a.paired != 0) : samw_record_lines(rec))) continue;
        const uint32_t tid = empty ? 0u : rec.tid;
        uint64_t s = unit_start[u];
        if (which) s += bamw_line_len(a, empty ? samw_empty_line(a.paired != 0, 0) : samw_line(a, rec, rank, 0, h), r);
        const SamwLine l = empty ? samw_empty_line(a.paired != 0, which) : samw_line(a, rec, rank, which, h);
        const uint64_t len = bamw_line_len(a, l, r), qn = samw_qname_len(a, r);
        if (s >= end || s + len <= base) continue;
        const uint8_t* seq;
        const uint64_t n_bases = bamw_l_seq(a, l, r, &seq);
        {
            const int64_t p0 = (int64_t)(s - base);
            bamw_put_fixed(l, tid, len, qn, n_bases, [&](int i, uint8_t b) { put_at(p0 + i, b); });
            s += kBamwFixed;
        }
        if (a.qname_off) run(kCopy, reinterpret_cast<const uint8_t*>(a.qnames) + a.qname_off[r], s, qn, 0);
        else {
            const int64_t p0 = (int64_t)(s - base);
            samw_put_default_qname(a.read_index_base + r, [&](int i, char ch) { put_at(p0 + i, (uint8_t)ch); });
        }
        s += qn;
        put_at((int64_t)(s - base), 0);
        s += 1;
        {
            const int64_t p0 = (int64_t)(s - base);
            bamw_put_cigar(l, [&](int i, uint8_t b) { put_at(p0 + i, b); });
            s += 4 * bamw_cigar_ops(l);
        }
        const bool rev = samw_reversed(a, l);
        run(rev ? kPackRev : kPack, seq, s, (n_bases + 1) / 2, n_bases);
        s += (n_bases + 1) / 2;
        const uint8_t* qual;
        uint64_t ql;
        if (samw_qual(a, l, r, &qual, &ql)) run(rev ? kQualRev : kQual, qual, s, n_bases, n_bases);
        else run(kFill, nullptr, s, n_bases, 0);
    }
    __syncthreads();
    const uint32_t nj = n_jobs < kJobCap ? n_jobs : kJobCap;
    const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    for (uint32_t k = wave; k < nj; k += kBlock / kWave) {
        const BamJob j = jobs[k];
        for (uint32_t i = lane; i < j.n; i += kWave) tile[j.at + i] = bam_run_byte(j.kind, j.src, j.left, i);
    }
    __syncthreads();
    const uint64_t g = base + 16ull * threadIdx.x;
    if (g < n_bytes) out[(g - out_base) >> 4] = tile4[threadIdx.x];
}

struct Scratch {
    DevBuf<uint32_t> empty, e_before, unit_len, unit_read;
    DevBuf<uint64_t> unit_start;
    DevBuf<unsigned long long> misc;
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

namespace {

// sfgpu_sam_write_text[_q] (sink), sfgpu_sam_write_bgzf[_q] (z; format SFGPU_SAMW_TEXT or SFGPU_SAMW_BAM) and sfgpu_bamsort_collect
// (store; SFGPU_SAMW_BAM): everything up to the chunk loop is the same but for the kernels that size and check a unit
int sam_write(const char* who, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, int paired, const char* d_ref_names,
              const uint64_t* d_ref_name_off, uint32_t n_refs, const char* d_qnames, const uint64_t* d_qname_off, const uint8_t* d_seq1,
              const int64_t* d_seq1_off, const uint8_t* d_seq2, const int64_t* d_seq2_off, const uint8_t* d_qual1, const uint8_t* d_qual2, int oriented,
              uint64_t read_index_base, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user, sfgpu_bgzw* z, int format,
              sfgpu_samwrite_result* out, sfgpu_stream stream, BamRecordStore* store, const int32_t* d_aln_pos = nullptr,
              const uint64_t* d_aln_op_off = nullptr, const uint32_t* d_aln_ops = nullptr) {
    const bool bam = format == SFGPU_SAMW_BAM;
    auto fail = [&](int code, const char* what) -> int { set_error("%s: %s", who, what); return code; };
    if (!out) return fail(SFGPU_ERR_INVALID, "null result");
    memset(out, 0, sizeof(*out));
    if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
    if (!(chunk_bytes >= 16 && chunk_bytes <= kMaxChunk)) return fail(SFGPU_ERR_INVALID, "chunk_bytes must lie in [16, 2^30] (0 = default)");
    if (n_reads == 0) return SFGPU_OK;
    if (!d_hit_offsets) return fail(SFGPU_ERR_INVALID, "null hit offsets");
    if (!(d_ref_name_off || n_refs == 0)) return fail(SFGPU_ERR_INVALID, "null reference name offsets");
    if (!(!d_qnames || d_qname_off)) return fail(SFGPU_ERR_INVALID, "read names without their offsets");
    if (!((!d_seq1 || d_seq1_off) && (!d_seq2 || d_seq2_off))) return fail(SFGPU_ERR_INVALID, "bases without their offsets");
    if (!((!d_qual1 || d_seq1_off) && (!d_qual2 || d_seq2_off))) return fail(SFGPU_ERR_INVALID, "qualities of a mate whose bases are not given");
    if (!(n_reads < 0xffffffffu)) return fail(SFGPU_ERR_RANGE, "n_reads must be below 2^32 - 1");
    if (!((d_aln_pos != nullptr) == (d_aln_op_off != nullptr) && (!d_aln_ops || d_aln_pos))) return fail(SFGPU_ERR_INVALID, "an alignment is positions, offsets and operations together");
    SamwArgs a = {d_hits, d_hit_offsets, n_reads, paired, d_ref_names, d_ref_name_off, n_refs, d_qnames, d_qname_off,
                  d_seq1, d_seq1_off, paired ? d_seq2 : nullptr, paired ? d_seq2_off : nullptr, read_index_base,
                  d_qual1, paired ? d_qual2 : nullptr, oriented != 0, d_aln_pos, d_aln_op_off, d_aln_ops};

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
    hipLaunchKernelGGL(k_read_flags, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, d_hit_offsets, n_reads, S.empty.p, S.misc.p);
    SF_HIP(hipGetLastError());
    if (n_refs) {
        hipLaunchKernelGGL(k_check_off<uint64_t>, dim3(grid_of(n_refs)), dim3(kBlock), 0, st, (const void*)d_ref_names, d_ref_name_off,
                           (uint64_t)n_refs, S.misc.p);
        SF_HIP(hipGetLastError());
    }
    if (d_qname_off) {
        hipLaunchKernelGGL(k_check_off<uint64_t>, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, (const void*)d_qnames, d_qname_off,
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
    SF_HIP(hipMemcpyAsync(&h_counts[0], d_hit_offsets + n_reads, 4, hipMemcpyDeviceToHost, st));
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
    if (n_hits && !d_hits) return fail(SFGPU_ERR_INVALID, "null hits");
    if (n_hits && d_aln_pos && !d_aln_ops) return fail(SFGPU_ERR_INVALID, "an alignment without operations");

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
        hipLaunchKernelGGL(bam ? k_record_size<true> : k_record_size<false>, dim3(grid_of(n_hits)), dim3(kBlock), 0, st, a, n_hits, S.e_before.p, S.unit_len.p, S.unit_read.p,
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
    if (store)              // sfgpu_bamsort_collect: every tile at once into a segment of the store, which then lists the records
        return store->take(total, out->n_lines, S.unit_start.p, n_units, st, &out->format_ms, [&](uint4* buf, hipStream_t s) -> int {
            hipLaunchKernelGGL(k_format_bam, dim3((unsigned)(((total - 1) >> kTileShift) + 1)), dim3(kBlock), 0, s, a, S.e_before.p, S.unit_read.p,
                               S.unit_start.p, n_units, total, (uint64_t)0, (uint64_t)0, buf);
            SF_HIP(hipGetLastError());
            return SFGPU_OK;
        });
    if (!sink && !z) return SFGPU_OK;
    if (out->max_unit_bytes > chunk_bytes) return fail(SFGPU_ERR_RANGE, "a unit (a line, or the two lines of a pair) is longer than chunk_bytes");

    // ---- the chunk plan and the format + copy + sink loop (textchunks.h), with this text's tiles
    textchunks::Stats ts;
    auto format_tiles = [&](uint64_t first_tile, uint64_t last_tile, uint64_t out_base, uint4* buf, hipStream_t s) -> int {
        hipLaunchKernelGGL(bam ? k_format_bam : k_format, dim3((unsigned)(last_tile - first_tile + 1)), dim3(kBlock), 0, s, a, S.e_before.p,
                           S.unit_read.p, S.unit_start.p, n_units, total, first_tile, out_base, buf);
        SF_HIP(hipGetLastError());
        return SFGPU_OK;
    };
    // the compressed formats: the chunk's device bytes go to the BGZF encoder, which copies and sinks what IT writes
    const int rc = z ? textchunks::deliver_device(who, S.unit_start.p, n_units, total, chunk_bytes, st, &ts,
                                                  [&](const uint8_t* d_bytes, uint64_t n, hipStream_t ready) -> int {
                                                      return sfgpu_bgzw_write_device(z, d_bytes, n, reinterpret_cast<sfgpu_stream>(ready));
                                                  }, format_tiles)
                     : textchunks::deliver(who, S.unit_start.p, n_units, total, chunk_bytes, sink, user, st, &ts, format_tiles);
    out->format_ms += ts.format_ms; out->d2h_ms = ts.d2h_ms; out->sink_ms = ts.sink_ms; out->n_chunks = ts.n_chunks;
    return rc;
}

}  // namespace

extern "C" int sfgpu_sam_write_text_q(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, int paired,
                                      const char* d_ref_names, const uint64_t* d_ref_name_off, uint32_t n_refs, const char* d_qnames,
                                      const uint64_t* d_qname_off, const uint8_t* d_seq1, const int64_t* d_seq1_off, const uint8_t* d_seq2,
                                      const int64_t* d_seq2_off, uint64_t read_index_base, uint64_t chunk_bytes, sfgpu_text_sink sink,
                                      void* user, sfgpu_samwrite_result* out, sfgpu_stream stream, const uint8_t* d_qual1,
                                      const uint8_t* d_qual2, int oriented) {
    return sam_write("sfgpu_sam_write_text", d_hits, d_hit_offsets, n_reads, paired, d_ref_names, d_ref_name_off, n_refs, d_qnames, d_qname_off,
                     d_seq1, d_seq1_off, d_seq2, d_seq2_off, d_qual1, d_qual2, oriented, read_index_base, chunk_bytes, sink, user, nullptr,
                     SFGPU_SAMW_TEXT, out, stream, nullptr);
}

extern "C" int sfgpu_sam_write_text_a(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, int paired,
                                      const char* d_ref_names, const uint64_t* d_ref_name_off, uint32_t n_refs, const char* d_qnames,
                                      const uint64_t* d_qname_off, const uint8_t* d_seq1, const int64_t* d_seq1_off, const uint8_t* d_seq2,
                                      const int64_t* d_seq2_off, uint64_t read_index_base, uint64_t chunk_bytes, sfgpu_text_sink sink,
                                      void* user, sfgpu_samwrite_result* out, sfgpu_stream stream, const uint8_t* d_qual1,
                                      const uint8_t* d_qual2, int oriented, const int32_t* d_aln_pos, const uint64_t* d_aln_op_off, const uint32_t* d_aln_ops) {
    return sam_write("sfgpu_sam_write_text", d_hits, d_hit_offsets, n_reads, paired, d_ref_names, d_ref_name_off, n_refs, d_qnames, d_qname_off,
                     d_seq1, d_seq1_off, d_seq2, d_seq2_off, d_qual1, d_qual2, oriented, read_index_base, chunk_bytes, sink, user, nullptr,
                     SFGPU_SAMW_TEXT, out, stream, nullptr, d_aln_pos, d_aln_op_off, d_aln_ops);
}

extern "C" int sfgpu_sam_write_bgzf_a(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, int paired,
                                      const char* d_ref_names, const uint64_t* d_ref_name_off, uint32_t n_refs, const char* d_qnames,
                                      const uint64_t* d_qname_off, const uint8_t* d_seq1, const int64_t* d_seq1_off, const uint8_t* d_seq2,
                                      const int64_t* d_seq2_off, uint64_t read_index_base, uint64_t chunk_bytes, sfgpu_bgzw* z, int format,
                                      sfgpu_samwrite_result* out, sfgpu_stream stream, const uint8_t* d_qual1, const uint8_t* d_qual2,
                                      int oriented, const int32_t* d_aln_pos, const uint64_t* d_aln_op_off, const uint32_t* d_aln_ops) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_sam_write_bgzf: null BGZF handle");
    SF_REQUIRE(format == SFGPU_SAMW_TEXT || format == SFGPU_SAMW_BAM, SFGPU_ERR_INVALID, "sfgpu_sam_write_bgzf: unknown format");
    return sam_write("sfgpu_sam_write_bgzf", d_hits, d_hit_offsets, n_reads, paired, d_ref_names, d_ref_name_off, n_refs, d_qnames, d_qname_off,
                     d_seq1, d_seq1_off, d_seq2, d_seq2_off, d_qual1, d_qual2, oriented, read_index_base, chunk_bytes, nullptr, nullptr, z, format,
                     out, stream, nullptr, d_aln_pos, d_aln_op_off, d_aln_ops);
}

extern "C" int sfgpu_sam_write_text(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, int paired,
                                    const char* d_ref_names, const uint64_t* d_ref_name_off, uint32_t n_refs, const char* d_qnames,
                                    const uint64_t* d_qname_off, const uint8_t* d_seq1, const int64_t* d_seq1_off, const uint8_t* d_seq2,
                                    const int64_t* d_seq2_off, uint64_t read_index_base, uint64_t chunk_bytes, sfgpu_text_sink sink,
                                    void* user, sfgpu_samwrite_result* out, sfgpu_stream stream) {
    return sfgpu_sam_write_text_q(d_hits, d_hit_offsets, n_reads, paired, d_ref_names, d_ref_name_off, n_refs, d_qnames, d_qname_off, d_seq1,
                                  d_seq1_off, d_seq2, d_seq2_off, read_index_base, chunk_bytes, sink, user, out, stream, nullptr, nullptr, 0);
}

extern "C" int sfgpu_sam_write_bgzf_q(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, int paired,
                                      const char* d_ref_names, const uint64_t* d_ref_name_off, uint32_t n_refs, const char* d_qnames,
                                      const uint64_t* d_qname_off, const uint8_t* d_seq1, const int64_t* d_seq1_off, const uint8_t* d_seq2,
                                      const int64_t* d_seq2_off, uint64_t read_index_base, uint64_t chunk_bytes, sfgpu_bgzw* z, int format,
                                      sfgpu_samwrite_result* out, sfgpu_stream stream, const uint8_t* d_qual1, const uint8_t* d_qual2,
                                      int oriented) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_sam_write_bgzf: null BGZF handle");
    SF_REQUIRE(format == SFGPU_SAMW_TEXT || format == SFGPU_SAMW_BAM, SFGPU_ERR_INVALID, "sfgpu_sam_write_bgzf: unknown format");
    return sam_write("sfgpu_sam_write_bgzf", d_hits, d_hit_offsets, n_reads, paired, d_ref_names, d_ref_name_off, n_refs, d_qnames, d_qname_off,
                     d_seq1, d_seq1_off, d_seq2, d_seq2_off, d_qual1, d_qual2, oriented, read_index_base, chunk_bytes, nullptr, nullptr, z, format,
                     out, stream, nullptr);
}

extern "C" int sfgpu_sam_write_bgzf(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, int paired,
                                    const char* d_ref_names, const uint64_t* d_ref_name_off, uint32_t n_refs, const char* d_qnames,
                                    const uint64_t* d_qname_off, const uint8_t* d_seq1, const int64_t* d_seq1_off, const uint8_t* d_seq2,
                                    const int64_t* d_seq2_off, uint64_t read_index_base, uint64_t chunk_bytes, sfgpu_bgzw* z, int format,
                                    sfgpu_samwrite_result* out, sfgpu_stream stream) {
    return sfgpu_sam_write_bgzf_q(d_hits, d_hit_offsets, n_reads, paired, d_ref_names, d_ref_name_off, n_refs, d_qnames, d_qname_off, d_seq1,
                                  d_seq1_off, d_seq2, d_seq2_off, read_index_base, chunk_bytes, z, format, out, stream, nullptr, nullptr, 0);
}

// bamsort.h: the batch's BAM records, checked, sized and formatted as for sfgpu_sam_write_bgzf_q, into `store`
int sfgpu::samw_collect_bam(BamRecordStore* store, const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, int paired,
                            const char* d_ref_names, const uint64_t* d_ref_name_off, uint32_t n_refs, const char* d_qnames,
                            const uint64_t* d_qname_off, const uint8_t* d_seq1, const int64_t* d_seq1_off, const uint8_t* d_seq2,
                            const int64_t* d_seq2_off, uint64_t read_index_base, sfgpu_samwrite_result* out, sfgpu_stream stream,
                            const uint8_t* d_qual1, const uint8_t* d_qual2, int oriented, const int32_t* d_aln_pos, const uint64_t* d_aln_op_off, const uint32_t* d_aln_ops) {
    return sam_write("sfgpu_bamsort_collect", d_hits, d_hit_offsets, n_reads, paired, d_ref_names, d_ref_name_off, n_refs, d_qnames, d_qname_off,
                     d_seq1, d_seq1_off, d_seq2, d_seq2_off, d_qual1, d_qual2, oriented, read_index_base, 0, nullptr, nullptr, nullptr, SFGPU_SAMW_BAM,
                     out, stream, store, d_aln_pos, d_aln_op_off, d_aln_ops);
}
