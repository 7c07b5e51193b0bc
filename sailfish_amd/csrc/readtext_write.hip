// readtext_write.hip -- a batch of reads as FASTA / FASTQ text, formatted on the device from the arrays where they lie:
// sfgpu_reads_write_text and sfgpu_reads_write_bgzf, the mirror of readtext.hip.  WHAT a record says is readwfmt.h (the bytes of
// readfile.reads_text_host); this file selects the records, finds where every one lies and writes it.
//
// A UNIT is one selected record: its two (FASTA) or four (FASTQ) lines.  Units are numbered in input order; the records that are
// not selected get NO unit, so that no unit is empty (a record is at least 3 bytes) and chunks end between units.
//   select  k_flags: one lane per record, flag[r] = the record is selected; an exclusive scan gives every selected record its unit.
//   size    k_unit_size: one lane per record writes its unit's record and bytes, and finds the FASTA record whose first base is
//           '>'.  An exclusive scan (primitives.h) gives every unit its 64-bit byte start; textchunks.h: the longest unit and the
//           greedy chunk ends.
//   check   k_newline_check: the rule "no '\n' in a name, the bases or the qualities" is one flat pass over each array, one aligned
//           16-byte group per lane.  A '\n' is mapped to its record by binary search of the offsets, ignored where that record is
//           not selected, else the lowest (record << 8 | kind) wins an atomicMin.
//   format  k_format_reads: one block per 4 KB tile of the output (texttile.h).  The units that overlap the tile are found by binary
//           search of the unit starts (a record may span many tiles), and the block strides over them: a tile of 3-byte FASTA
//           records holds more units than the block has lanes.  The lane of a unit writes its single bytes ('@', '>', '\n', '+'),
//           a generated name and every run (name, bases, qualities) of at most kShortCopy bytes; longer runs are clipped to the
//           tile, queued, and copied a byte per lane and step by whole wavefronts.  Then every lane stores one aligned 16-byte group.
// The run queue below is this file's own: samtext_write.hip's Job / LineOut serve runs that are reversed, complemented and packed.
// The chunks are planned by textchunks.h and go to the sink (sfgpu_reads_write_text) or, on the device, to the BGZF encoder of
// bgzf_write.hip (sfgpu_reads_write_bgzf).
#include "common.h"
#include "primitives.h"
#include "readwfmt.h"
#include "texttile.h"

#include <cstring>

namespace sfgpu {
namespace {

using textchunks::kBlock;
using textchunks::kTileBytes;
using textchunks::kTileShift;
using textchunks::kDefaultChunk;
using textchunks::kMaxChunk;
using textchunks::grid_of;

constexpr uint32_t kShortCopy = 48;                       // longer names, bases and qualities are copied by whole wavefronts
// A run is queued only when it is longer than kShortCopy bytes, and the runs of all records are disjoint ranges of the output.  A
// job is the part of one run inside one tile.  Runs that lie whole in a tile take at least kShortCopy + 1 of its bytes each; a run
// that does not lie whole in it covers its first or its last byte, and disjoint runs cannot share either: two more.  The
// `k < kJobCap` test below can therefore not drop a job.
constexpr uint32_t kJobCap = kTileBytes / (kShortCopy + 1) + 3;

enum : unsigned long long { kBadOffsets = 1, kTooLong = 2, kNullBytes = 4 };
// misc: [0] flags, [1] the longest unit, [2] the lowest (record << 8 | kind) that cannot be written
constexpr int kMisc = 3;
constexpr int kMiscError = 2;

// offsets off[0 .. n] of `bytes`: kBadOffsets where they decrease (or are negative), kNullBytes where bytes are named but absent
template <typename Off>
__global__ void k_check_off(const void* __restrict__ bytes, const Off* __restrict__ off, uint64_t n, unsigned long long* __restrict__ misc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Off a = off[i], b = off[i + 1];
    if (a > b || a < (Off)0) atomicOr(&misc[0], kBadOffsets);
    else if (b > a && !bytes) atomicOr(&misc[0], kNullBytes);
}

__global__ void k_flags(const uint8_t* __restrict__ select, uint64_t n_reads, uint32_t* __restrict__ flag) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_reads) flag[r] = !select || select[r] != 0;
}

// one lane per record: a selected record r is unit unit_of[r]
__global__ void __launch_bounds__(kBlock)
k_unit_size(ReadwArgs a, const uint32_t* __restrict__ unit_of, uint32_t* __restrict__ unit_len, uint32_t* __restrict__ unit_read,
            unsigned long long* __restrict__ misc) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_reads || !readw_selected(a, r)) return;
    const uint32_t u = unit_of[r];
    uint64_t len = readw_record_len(a, r);
    if (readw_fasta_seq_start(a, r)) atomicMin(&misc[kMiscError], readw_error_key(r, SFGPU_READW_FASTA_SEQ_START));
    if (len > 0xffffffffull) { atomicOr(&misc[0], kTooLong); len = 0; }
    unit_len[u] = (uint32_t)len;
    unit_read[u] = (uint32_t)r;
}

// One lane per aligned 16-byte group of bytes[lo .. hi) (offsets off[0 .. n_reads], checked; lo = off[0], hi = off[n_reads]).  The
// groups are aligned in memory, not in the array, which may begin anywhere: the first and the last group are clipped to the array.
// The records of a group's '\n' bytes never decrease with the byte, so the first one in a selected record is the group's lowest.
template <typename Off>
__global__ void __launch_bounds__(kBlock)
k_newline_check(const uint8_t* __restrict__ bytes, const Off* __restrict__ off, uint64_t n_reads, uint64_t lo, uint64_t hi,
                const uint8_t* __restrict__ select, int kind, unsigned long long* __restrict__ misc) {
    const uintptr_t first = reinterpret_cast<uintptr_t>(bytes + lo) & ~(uintptr_t)15;
    const uintptr_t g = first + 16ull * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    const uintptr_t begin = reinterpret_cast<uintptr_t>(bytes + lo), end = reinterpret_cast<uintptr_t>(bytes + hi);
    if (g >= end) return;
    const uintptr_t p0 = g > begin ? g : begin, p1 = g + 16 < end ? g + 16 : end;
    if (p1 - p0 == 16) {                                  // the whole group lies in the array: one 16-byte load says whether to look
        const uint4 v = *reinterpret_cast<const uint4*>(g);
        const uint32_t w[4] = {v.x ^ 0x0a0a0a0au, v.y ^ 0x0a0a0a0au, v.z ^ 0x0a0a0a0au, v.w ^ 0x0a0a0a0au};
        uint32_t any = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) any |= (w[k] - 0x01010101u) & ~w[k] & 0x80808080u;       // nonzero iff a byte of the word is 0
        if (!any) return;
    }
    for (uintptr_t p = p0; p < p1; ++p) {
        if (*reinterpret_cast<const uint8_t*>(p) != '\n') continue;
        const uint64_t r = textchunks::holder_of(off, n_reads, (Off)(p - reinterpret_cast<uintptr_t>(bytes)));
        if (select && !select[r]) continue;
        atomicMin(&misc[kMiscError], readw_error_key(r, kind));
        return;
    }
}

// the part of a run inside the tile, for the wavefronts
struct Job {
    const uint8_t* src;     // the source of the first byte that lies in the tile
    uint32_t at, n;         // tile offset and bytes
};

// where a record's pieces go, one after the other; `p` is the tile offset of the next byte, before or behind the tile or in it
struct RecordOut {
    const textchunks::Tile& tile;
    Job* jobs;
    uint32_t* n_jobs;
    int64_t p;
    __device__ __forceinline__ void byte(uint8_t b) { tile.put(p++, (char)b); }
    // the n bytes of a run: by this lane when short, else its part inside the tile is queued for the wavefronts
    __device__ __forceinline__ void run(const uint8_t* __restrict__ src, uint64_t n) {
        const int64_t room = (int64_t)(tile.end() - tile.base), lo = p > 0 ? p : 0, hi = p + (int64_t)n < room ? p + (int64_t)n : room;
        if (lo < hi) {
            if (n <= kShortCopy) {
                for (int64_t i = lo; i < hi; ++i) tile.bytes[i] = (char)src[i - p];
            } else {
                const uint32_t k = atomicAdd(n_jobs, 1u);
                if (k < kJobCap) jobs[k] = Job{src + (lo - p), (uint32_t)lo, (uint32_t)(hi - lo)};
            }
        }
        p += (int64_t)n;
    }
};

// One block per tile of the output; `out` is the chunk buffer, whose byte 0 is text byte out_base (a multiple of kTileBytes).  The
// units that overlap the tile are found by binary search of the unit starts (units are never empty, so the starts increase
// strictly); the block strides over them.  Then the wavefronts take the queued runs in turn, a byte per lane and step.
__global__ void __launch_bounds__(kBlock)
k_format_reads(ReadwArgs a, const uint32_t* __restrict__ unit_read, const uint64_t* __restrict__ unit_start, uint64_t n_units,
               uint64_t n_bytes, uint64_t first_tile, uint64_t out_base, uint4* __restrict__ out) {
    __shared__ uint4 tile4[kBlock];
    __shared__ Job jobs[kJobCap];
    __shared__ uint32_t n_jobs;
    const textchunks::Tile tile(tile4, first_tile, n_bytes);
    if (threadIdx.x == 0) n_jobs = 0;
    __syncthreads();
    const uint64_t u_lo = textchunks::holder_of(unit_start, n_units, tile.base), u_hi = textchunks::holder_of(unit_start, n_units, tile.end() - 1);
    const bool fastq = readw_fastq(a);
    for (uint64_t u = u_lo + threadIdx.x; u <= u_hi; u += kBlock) {
        const uint64_t r = unit_read[u];
        RecordOut o{tile, jobs, &n_jobs, (int64_t)(unit_start[u] - tile.base)};
        const int64_t b0 = a.off[r];
        const uint64_t len = (uint64_t)(a.off[r + 1] - b0);
        o.byte(fastq ? '@' : '>');
        if (a.name_off) {
            const uint64_t n0 = a.name_off[r];
            o.run(a.names + n0, a.name_off[r + 1] - n0);
        } else {
            const uint64_t index = a.read_index_base + r;
            readw_put_default_name(index, [&](int i, char ch) { tile.put(o.p + i, ch); });
            o.p += readw_default_name_len(index);
        }
        o.byte('\n');
        o.run(a.bases + b0, len);
        o.byte('\n');
        if (fastq) {
            o.byte('+');
            o.byte('\n');
            o.run(a.qual + b0, len);
            o.byte('\n');
        }
    }
    __syncthreads();
    const uint32_t nj = n_jobs < kJobCap ? n_jobs : kJobCap;
    const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    for (uint32_t k = wave; k < nj; k += kBlock / kWave) {
        const Job j = jobs[k];
        for (uint32_t i = lane; i < j.n; i += kWave) tile.bytes[j.at + i] = (char)j.src[i];
    }
    __syncthreads();
    tile.store(out_base, out);
}

struct Scratch {
    DevBuf<uint32_t> flag, unit_of, unit_len, unit_read;
    DevBuf<uint64_t> unit_start;
    DevBuf<unsigned long long> misc;
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

namespace {

// the flat pass over bytes[lo .. hi), the offsets checked; nothing to do for an absent or empty array
template <typename Off>
int newline_check(const ReadwArgs& a, const uint8_t* bytes, const Off* off, uint64_t lo, uint64_t hi, int kind, unsigned long long* d_misc, hipStream_t st) {
    if (!bytes || hi <= lo) return SFGPU_OK;
    const uint64_t groups = (hi - lo + 15) / 16 + 1;      // the groups are aligned in memory: one more where the array begins inside a group
    hipLaunchKernelGGL(k_newline_check<Off>, dim3(grid_of(groups)), dim3(kBlock), 0, st, bytes, off, a.n_reads, lo, hi, a.select, kind, d_misc);
    SF_HIP(hipGetLastError());
    return SFGPU_OK;
}

// Everything up to the chunk loop is the same for both destinations: the chunks go to a sink, or to the BGZF encoder `z`.
int reads_write(const char* who, const ReadwArgs& a, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user, sfgpu_bgzw* z,
                sfgpu_readwrite_result* out, sfgpu_stream stream) {
    auto fail = [&](int code, const char* what) -> int { set_error("%s: %s", who, what); return code; };
    if (!out) return fail(SFGPU_ERR_INVALID, "null result");
    memset(out, 0, sizeof(*out));
    out->n_reads = a.n_reads;
    if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
    if (!(chunk_bytes >= 16 && chunk_bytes <= kMaxChunk)) return fail(SFGPU_ERR_INVALID, "chunk_bytes must lie in [16, 2^30] (0 = default)");
    if (a.n_reads == 0) return SFGPU_OK;
    if (!a.off) return fail(SFGPU_ERR_INVALID, "null base offsets");
    if (!(!a.names || a.name_off)) return fail(SFGPU_ERR_INVALID, "read names without their offsets");
    if (!(a.n_reads < 0xffffffffull)) return fail(SFGPU_ERR_RANGE, "n_reads must be below 2^32 - 1");
    const uint64_t n_reads = a.n_reads;

    Scratch S;
    CallScope scope;        // after S: it drains the stream before S's blocks go back to the pool
    hipStream_t st = nullptr;
    hipEvent_t ev_in = nullptr, ev_a[2] = {nullptr, nullptr}, ev_s[2] = {nullptr, nullptr};
    unsigned long long* h_misc = nullptr;     // [0 .. kMisc) misc, [kMisc] total bytes, [kMisc + 1] the first and [kMisc + 2] the last base
                                              // offset, [kMisc + 3], [kMisc + 4] those of the names; uint32 view of [kMisc + 5]: selected records
    SF_HIP(scope.acquire(&st));
    SF_HIP(scope.event(&ev_in, hipEventDisableTiming));
    for (auto& e : ev_a) SF_HIP(scope.event(&e));
    for (auto& e : ev_s) SF_HIP(scope.event(&e));
    SF_HIP(scope.pinned_block(&h_misc, (kMisc + 6) * sizeof(unsigned long long)));
    // behind whatever the caller has queued on `stream`
    SF_HIP(hipEventRecord(ev_in, as_stream(stream)));
    SF_HIP(hipStreamWaitEvent(st, ev_in, 0));

    // ---- the arrays' shape and the selection: offsets that never decrease, the unit of every selected record
    if (int rc = S.misc.reserve(kMisc, st, false)) return rc;
    if (int rc = S.flag.reserve(n_reads + 1, st, false)) return rc;
    if (int rc = S.unit_of.reserve(n_reads + 1, st, false)) return rc;
    SF_HIP(hipMemsetAsync(S.misc.p, 0, kMisc * sizeof(unsigned long long), st));
    SF_HIP(hipMemsetAsync(S.misc.p + kMiscError, 0xff, sizeof(unsigned long long), st));
    SF_HIP(hipEventRecord(ev_a[0], st));
    hipLaunchKernelGGL(k_check_off<int64_t>, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, (const void*)a.bases, a.off, n_reads, S.misc.p);
    SF_HIP(hipGetLastError());
    if (a.name_off) {
        hipLaunchKernelGGL(k_check_off<uint64_t>, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, (const void*)a.names, a.name_off, n_reads, S.misc.p);
        SF_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_flags, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, a.select, n_reads, S.flag.p);
    SF_HIP(hipGetLastError());
    if (int rc = exclusive_scan_u32_u32(S.flag.p, S.unit_of.p, n_reads, st)) return rc;
    SF_HIP(hipEventRecord(ev_a[1], st));
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_misc[kMisc + 1], a.off, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_misc[kMisc + 2], a.off + n_reads, 8, hipMemcpyDeviceToHost, st));
    h_misc[kMisc + 3] = h_misc[kMisc + 4] = 0;
    if (a.name_off) {
        SF_HIP(hipMemcpyAsync(&h_misc[kMisc + 3], a.name_off, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(&h_misc[kMisc + 4], a.name_off + n_reads, 8, hipMemcpyDeviceToHost, st));
    }
    SF_HIP(hipMemcpyAsync(&h_misc[kMisc + 5], S.unit_of.p + n_reads, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&out->format_ms, ev_a[0], ev_a[1]);
    if (h_misc[0] & kBadOffsets) return fail(SFGPU_ERR_INVALID, "an offset array decreases or is negative");
    if (h_misc[0] & kNullBytes) return fail(SFGPU_ERR_INVALID, "offsets name bytes of a null array");
    const uint64_t n_units = *reinterpret_cast<const uint32_t*>(&h_misc[kMisc + 5]);
    out->n_selected = n_units;
    if (n_units == 0) return SFGPU_OK;

    // ---- sizing and validation: unit lengths, unit starts, the longest unit, the lowest record that cannot be written
    if (int rc = S.unit_len.reserve(n_units + 1, st, false)) return rc;
    if (int rc = S.unit_read.reserve(n_units, st, false)) return rc;
    if (int rc = S.unit_start.reserve(n_units + 1, st, false)) return rc;
    SF_HIP(hipEventRecord(ev_s[0], st));
    if (a.name_off) if (int rc = newline_check(a, a.names, a.name_off, h_misc[kMisc + 3], h_misc[kMisc + 4], SFGPU_READW_NAME_NEWLINE, S.misc.p, st)) return rc;
    if (int rc = newline_check(a, a.bases, a.off, h_misc[kMisc + 1], h_misc[kMisc + 2], SFGPU_READW_SEQ_NEWLINE, S.misc.p, st)) return rc;
    if (int rc = newline_check(a, a.qual, a.off, h_misc[kMisc + 1], h_misc[kMisc + 2], SFGPU_READW_QUAL_NEWLINE, S.misc.p, st)) return rc;
    hipLaunchKernelGGL(k_unit_size, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, a, S.unit_of.p, S.unit_len.p, S.unit_read.p, S.misc.p);
    SF_HIP(hipGetLastError());
    if (int rc = exclusive_scan_u32(S.unit_len.p, S.unit_start.p, n_units, st, false)) return rc;
    if (int rc = textchunks::line_max(S.unit_start.p, n_units, S.misc.p + 1, st)) return rc;
    SF_HIP(hipEventRecord(ev_s[1], st));
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, kMisc * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_misc[kMisc], S.unit_start.p + n_units, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&out->format_ms, ev_s[0], ev_s[1]);
    if (h_misc[kMiscError] != kReadwNoError) {
        static const char* const kWhat[] = {"", "the name holds a line end", "the bases hold a line end", "the qualities hold a line end",
                                            "the first base of a FASTA record is '>'"};
        const unsigned long long key = h_misc[kMiscError];
        out->error_record = key >> 8; out->error_kind = (int32_t)(key & 0xff);
        set_error("%s: record %llu: %s", who, (unsigned long long)out->error_record, kWhat[out->error_kind <= 4 ? out->error_kind : 0]);
        return SFGPU_ERR_FORMAT;
    }
    if (h_misc[0] & kTooLong) return fail(SFGPU_ERR_RANGE, "a record is longer than 2^32 - 1 bytes");
    const uint64_t total = h_misc[kMisc];
    out->n_bytes = total; out->max_record_bytes = h_misc[1];
    if (!sink && !z) return SFGPU_OK;
    if (out->max_record_bytes > chunk_bytes) return fail(SFGPU_ERR_RANGE, "a record is longer than chunk_bytes");

    // ---- the chunk plan and the format + copy + sink loop (textchunks.h), with this text's tiles
    textchunks::Stats ts;
    auto format_tiles = [&](uint64_t first_tile, uint64_t last_tile, uint64_t out_base, uint4* buf, hipStream_t s) -> int {
        hipLaunchKernelGGL(k_format_reads, dim3((unsigned)(last_tile - first_tile + 1)), dim3(kBlock), 0, s, a, S.unit_read.p, S.unit_start.p, n_units,
                           total, first_tile, out_base, buf);
        SF_HIP(hipGetLastError());
        return SFGPU_OK;
    };
    // compressed: the chunk's device bytes go to the BGZF encoder, which copies and sinks what IT writes
    const int rc = z ? textchunks::deliver_device(who, S.unit_start.p, n_units, total, chunk_bytes, st, &ts,
                                                  [&](const uint8_t* d_bytes, uint64_t n, hipStream_t ready) -> int {
                                                      return sfgpu_bgzw_write_device(z, d_bytes, n, reinterpret_cast<sfgpu_stream>(ready));
                                                  }, format_tiles)
                     : textchunks::deliver(who, S.unit_start.p, n_units, total, chunk_bytes, sink, user, st, &ts, format_tiles);
    out->format_ms += ts.format_ms; out->d2h_ms = ts.d2h_ms; out->sink_ms = ts.sink_ms; out->n_chunks = ts.n_chunks;
    return rc;
}

}  // namespace

extern "C" int sfgpu_reads_write_text(const uint8_t* d_bases, const int64_t* d_off, uint64_t n_reads, const uint8_t* d_qual,
                                      const uint8_t* d_names, const uint64_t* d_name_off, uint64_t read_index_base,
                                      const uint8_t* d_select, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
                                      sfgpu_readwrite_result* out, sfgpu_stream stream) {
    const ReadwArgs batch{d_bases, d_off, n_reads, d_qual, d_names, d_name_off, read_index_base, d_select};
    return reads_write("sfgpu_reads_write_text", batch, chunk_bytes, sink, user, nullptr, out, stream);
}

extern "C" int sfgpu_reads_write_bgzf(const uint8_t* d_bases, const int64_t* d_off, uint64_t n_reads, const uint8_t* d_qual,
                                      const uint8_t* d_names, const uint64_t* d_name_off, uint64_t read_index_base,
                                      const uint8_t* d_select, uint64_t chunk_bytes, sfgpu_bgzw* z, sfgpu_readwrite_result* out,
                                      sfgpu_stream stream) {
    SF_REQUIRE(z, SFGPU_ERR_INVALID, "sfgpu_reads_write_bgzf: null BGZF handle");
    const ReadwArgs batch{d_bases, d_off, n_reads, d_qual, d_names, d_name_off, read_index_base, d_select};
    return reads_write("sfgpu_reads_write_bgzf", batch, chunk_bytes, nullptr, nullptr, z, out, stream);
}
