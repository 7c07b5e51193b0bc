// readtext.hip -- FASTA / FASTQ records parsed on the device: sfgpu_reads_parse_host, and sfgpu_reads_parse_device for a text that
// is in device memory already (what bgzf_read.hip inflated); sfgpu_reads_names_match (k_names_match) compares the names of mates.  What a record is, is decided by readfmt.h (the same functions run
// serially in tests/readfile_harness.cpp); this file is the passes around them.  The two entries differ in how the text and the
// newline counts of its 16-byte groups get there; from the scan of the counts on they are one function, parse_counted.
//
// The host text goes through two pinned buffers in sub-chunks of kSubBytes; the copy of sub-chunk c + 1 runs on the copy stream
// while the '\n' bytes of sub-chunk c are counted.  A '\n' is appended behind the text, so the remainder (readfmt.h) is a line of
// the device text like any other and L = the number of '\n' bytes on the device.  Then, over the whole text:
//   k_line_ends         scan of the counts -> where every line ends (textlines.h)
//   k_reads_lines       one lane per line: rf_line -> header flag, bases of the line, the FASTQ checks (atomic min over
//                       (record << 8 | kind)) and the last non-empty line (atomic max)
//   two scans           header flags -> the record of every line; bases per line -> where the line's bases go (dst)
//   k_reads_rec_lines   the line that opens each record
//   k_reads_cut         one lane: records the text holds, the error, the cut at max_reads / cap_bases (binary search), consumed
//   k_reads_emit        one lane per record: d_off, the name span, and for the name blob (the _n entries) the name's length and start
//   k_names_gather      the _n entries: behind a scan of the name lengths, one lane per 16-byte group of the name blob (see there)
//   k_reads_compact     one block per 4 KB tile of the packed bases: each lane finds the line its 16 output bytes begin in by
//                       binary search in dst, gathers them (one unaligned 16-byte read when they lie in one line, byte by byte
//                       across line ends) and issues one 16-byte store.  The qualities of a FASTQ text (the _q entries) are a
//                       second run of the same kernel with the line selector 2: a record's quality line lies two lines behind
//                       its sequence line and is of the same length (readfmt.h checks that), so dst says where its bytes go
#include "common.h"
#include "primitives.h"
#include "readfmt.h"
#include "textlines.h"

namespace sfgpu {
namespace {

using textlines::kBlock;
using textlines::grid_of;
using textlines::nl_mask;
constexpr uint64_t kSubBytes = 4ull << 20;               // staged sub-chunk (a multiple of 16)
constexpr uint32_t kTileBytes = 4096;                    // kBlock lanes x one 16-byte store

__global__ void k_reads_count(const uint4* __restrict__ buf, uint64_t g0, uint64_t g1, uint32_t* __restrict__ nl_cnt) {
    const uint64_t g = g0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= g1) return;
    nl_cnt[g] = __popc(nl_mask(buf[g]));
}

// cnt[0] += bytes that are neither '\n' nor '\r', cnt[1] += '\n' bytes (rf_all_blank and the line count of a text without records)
__global__ void k_reads_blank(const unsigned char* __restrict__ bytes, uint64_t n, unsigned long long* __restrict__ cnt) {
    const uint64_t p0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16u;
    unsigned long long other = 0, nl = 0;
    for (uint64_t p = p0; p < n && p < p0 + 16u; ++p) {
        const unsigned char b = bytes[p];
        nl += b == '\n';
        other += b != '\n' && b != '\r';
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) { other += __shfl_xor(other, o); nl += __shfl_xor(nl, o); }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (other) atomicAdd(&cnt[0], other);
        if (nl) atomicAdd(&cnt[1], nl);
    }
}

struct Bounds {
    const uint32_t* line_end;
    __device__ void operator()(uint32_t j, uint32_t* s, uint32_t* e) const { *s = j ? line_end[j - 1] + 1 : 0; *e = line_end[j]; }
};
struct Bytes {
    const unsigned char* p;
    __device__ unsigned char operator()(uint32_t i) const { return p[i]; }
};

// misc[0] = first error of the line checks, misc[1] = T (1 + the last non-empty usable line)
__global__ void k_reads_lines(const unsigned char* __restrict__ bytes, int format, int final, uint32_t L, const uint32_t* __restrict__ line_end,
                              uint32_t* __restrict__ hdr, uint32_t* __restrict__ seq, unsigned long long* __restrict__ misc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long t = 0;
    if (i < L) {
        const RfLine r = rf_line(format, final, i, L, Bytes{bytes}, Bounds{line_end});
        hdr[i] = r.header;
        seq[i] = r.seq;
        if (r.error) atomicMin(&misc[0], ((unsigned long long)(i >> 2) << 8) | (unsigned long long)r.error);
        if (r.len) t = (unsigned long long)i + 1;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(t, o);
        t = other > t ? other : t;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && t) atomicMax(&misc[1], t);
}

// rec_line[r] = the line that opens record r; rec_line[H] = L
__global__ void k_reads_rec_lines(uint32_t L, const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ hdr_scan,
                                  uint32_t* __restrict__ rec_line) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > L) return;
    if (i == L) { rec_line[hdr_scan[L]] = L; return; }
    if (hdr[i]) rec_line[hdr_scan[i]] = i;
}

// res: [0] error, [1] records emitted, [2] their bases, [3] consumed, [4] records the text holds, [5] error line, [6] lines before the cut
__global__ void k_reads_cut(int format, int final, uint32_t L, uint64_t n_bytes, uint64_t max_reads, uint64_t cap_bases,
                            const uint32_t* __restrict__ line_end, const uint32_t* __restrict__ hdr_scan, const uint32_t* __restrict__ dst,
                            const uint32_t* __restrict__ rec_line, const unsigned long long* __restrict__ misc,
                            unsigned long long* __restrict__ res) {
    if (blockIdx.x || threadIdx.x) return;
    const RfCount c = rf_count_records(format, final, L, (uint32_t)misc[1], hdr_scan[L]);
    const unsigned long long err = rf_final_error(misc[0], c);
    res[0] = err; res[4] = c.records;
    res[1] = res[2] = res[3] = res[5] = res[6] = 0;
    if (err != kReadsNoError) { res[5] = rf_error_line(err, c); return; }
    auto off_of = [&](uint32_t r) -> uint64_t { return dst[rec_line[r]]; };
    const uint32_t R = rf_cut(c.records, max_reads, cap_bases, off_of);
    const uint32_t rl = rec_line[R];
    uint32_t s = 0, e = 0;
    if (rl < L) Bounds{line_end}(rl, &s, &e);
    res[1] = R; res[2] = off_of(R); res[3] = rf_consumed(final, R, c.records, n_bytes, s); res[6] = rl;
}

// name_len / name_src (both or neither; R + 1 entries, the last one 0): the bytes of record r's name and where they begin, for the blob
__global__ void k_reads_emit(const unsigned char* __restrict__ bytes, uint32_t R, const uint32_t* __restrict__ line_end,
                             const uint32_t* __restrict__ dst, const uint32_t* __restrict__ rec_line, int64_t* __restrict__ d_off,
                             uint64_t* __restrict__ d_name_span, uint32_t* __restrict__ name_len, uint32_t* __restrict__ name_src) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > R) return;
    const uint32_t line = rec_line[r];
    d_off[r] = (int64_t)dst[line];
    if (r == R) {
        if (name_len) { name_len[r] = 0; name_src[r] = 0; }
        return;
    }
    if (!d_name_span && !name_len) return;
    uint32_t s, e;
    Bounds{line_end}(line, &s, &e);
    const uint32_t len = rf_name_len(Bytes{bytes}, s, rf_line_len(Bytes{bytes}, s, e));
    if (d_name_span) {
        d_name_span[2 * (uint64_t)r] = (uint64_t)s + 1;
        d_name_span[2 * (uint64_t)r + 1] = len;
    }
    if (name_len) { name_len[r] = len; name_src[r] = s + 1; }
}

// 16 bytes from byte p of the text (the buffer holds a whole group behind the last one that is read)
__device__ inline uint4 load_unaligned16(const uint4* __restrict__ buf, uint32_t p) {
    const uint4 a = buf[p >> 4], b = buf[(p >> 4) + 1];
    const uint32_t t[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t ws = (p & 15u) >> 2, bs = (p & 3u) * 8;
    uint32_t u[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) u[j] = ws == 0 ? t[j] : ws == 1 ? t[j + 1] : ws == 2 ? t[j + 2] : t[j + 3];
    uint4 v;
    v.x = __funnelshift_r(u[0], u[1], bs); v.y = __funnelshift_r(u[1], u[2], bs);
    v.z = __funnelshift_r(u[2], u[3], bs); v.w = __funnelshift_r(u[3], u[4], bs);
    return v;
}

// lines [0, Lc) carry the n_bases bases of the emitted records; dst[Lc] = n_bases.  SEL = 0 gathers the bases; SEL = 2 (FASTQ)
// the bytes of the line two behind each line that carries bases: the qualities, to the same places
template <uint32_t SEL>
__global__ void __launch_bounds__(kBlock) k_reads_compact(const uint4* __restrict__ buf, uint32_t Lc, uint32_t n_bases,
                                                          const uint32_t* __restrict__ line_end, const uint32_t* __restrict__ dst,
                                                          uint4* __restrict__ out) {
    const uint32_t o = (blockIdx.x * (uint32_t)kBlock + threadIdx.x) * 16u;
    if (o >= n_bases) return;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(buf);
    const uint32_t cnt = n_bases - o < 16u ? n_bases - o : 16u;
    uint32_t lo = 0, hi = Lc;                                // dst[lo] <= o < dst[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (dst[mid] <= o) lo = mid; else hi = mid;
    }
    uint32_t i = lo;
    uint32_t src = (i + SEL ? line_end[i + SEL - 1] + 1 : 0) + (o - dst[i]);
    uint32_t avail = dst[i + 1] - o;
    if (avail >= 16u) {                                      // (then cnt == 16)
        out[o >> 4] = load_unaligned16(buf, src);
        return;
    }
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < cnt;) {
        if (avail == 0) {                                    // on to the next line that carries bases (there is one: k < cnt)
            ++i;
            src = line_end[i + SEL - 1] + 1;
            avail = dst[i + 1] - dst[i];
            continue;
        }
        const uint32_t take = avail < cnt - k ? avail : cnt - k;
        for (uint32_t j = 0; j < take; ++j, ++k) {
            const uint32_t b = bytes[src + j];
#pragma unroll
            for (int q = 0; q < 4; ++q) if ((k >> 2) == (uint32_t)q) w[q] |= b << (8 * (k & 3u));
        }
        avail -= take;
    }
    if (cnt == 16u) { out[o >> 4] = make_uint4(w[0], w[1], w[2], w[3]); return; }
    unsigned char* tail = reinterpret_cast<unsigned char*>(out) + o;
    for (uint32_t k = 0; k < cnt; ++k) tail[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3u)));
}

// v with only its first take bytes (1 .. 15), moved up by k bytes (k + take <= 16): one piece of a 16-byte group of the name blob
__device__ inline uint4 place_bytes(uint4 v, uint32_t take, uint32_t k) {
    auto kept = [take](uint32_t word, uint32_t q) -> uint32_t {           // word q of v with the bytes behind `take` cleared
        const uint32_t left = take > 4u * q ? take - 4u * q : 0u;
        return left >= 4u ? word : left ? word & ((1u << (8u * left)) - 1u) : 0u;
    };
    const uint32_t m0 = kept(v.x, 0), m1 = kept(v.y, 1), m2 = kept(v.z, 2), m3 = kept(v.w, 3);
    const uint32_t ws = k >> 2, bs = (k & 3u) * 8u;                       // whole words, then bits
    const uint32_t a0 = ws == 0 ? m0 : 0u;
    const uint32_t a1 = ws == 0 ? m1 : ws == 1 ? m0 : 0u;
    const uint32_t a2 = ws == 0 ? m2 : ws == 1 ? m1 : ws == 2 ? m0 : 0u;
    const uint32_t a3 = ws == 0 ? m3 : ws == 1 ? m2 : ws == 2 ? m1 : m0;
    return make_uint4(a0 << bs, __funnelshift_l(a0, a1, bs), __funnelshift_l(a1, a2, bs), __funnelshift_l(a2, a3, bs));
}

// The name blob, in the form of k_reads_compact: one lane per 16-byte group of the OUTPUT.  name_off[0 .. R] = exclusive sum of the
// name lengths (n_name = name_off[R]), name_src[r] = where record r's name begins in the text.  The lane finds its record by binary
// search (rf_blob_record).  A group that lies within one name is one unaligned 16-byte read; any other group -- with names of 10 to
// 40 bytes, most of them -- is put together from one unaligned 16-byte read per name it touches, masked to the bytes taken and
// moved to their place in registers: no byte loop, so a long name costs what its bytes cost.  One aligned 16-byte store; the last
// group is filled up with zeros.  The first R + 1 lanes also widen name_off to the 64 bits the writers take.
__global__ void __launch_bounds__(kBlock) k_names_gather(const uint4* __restrict__ buf, uint32_t R, uint32_t n_name,
                                                         const uint32_t* __restrict__ name_off, const uint32_t* __restrict__ name_src,
                                                         uint4* __restrict__ out, uint64_t* __restrict__ d_name_off) {
    const uint32_t g = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (g <= R) d_name_off[g] = name_off[g];
    if (g >= (n_name + 15u) / 16u) return;
    const uint32_t o = g * 16u;
    const uint32_t cnt = n_name - o < 16u ? n_name - o : 16u;
    uint32_t i = rf_blob_record(R, o, [&](uint32_t r) { return name_off[r]; });
    uint32_t src = name_src[i] + (o - name_off[i]);
    uint32_t avail = name_off[i + 1] - o;
    if (avail >= 16u) {                                      // (then cnt == 16)
        out[g] = load_unaligned16(buf, src);
        return;
    }
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t k = 0; k < cnt;) {
        if (avail == 0) {                                    // on to the next record (one with a byte exists: k < cnt <= n_name - o)
            ++i;
            src = name_src[i];
            avail = name_off[i + 1] - name_off[i];
            continue;
        }
        const uint32_t take = avail < cnt - k ? avail : cnt - k;
        const uint4 v = place_bytes(load_unaligned16(buf, src), take, k);      // src < n_bytes: the buffer holds a group more
        w.x |= v.x; w.y |= v.y; w.z |= v.z; w.w |= v.w;
        k += take; src += take; avail -= take;
    }
    out[g] = w;
}

struct Bytes64 {
    const unsigned char* p;
    __device__ unsigned char operator()(uint64_t i) const { return p[i]; }
};

// Mates compared by the stem rule (readfmt.h): first = the lowest read whose two names disagree.  One lane per read settles the
// stem lengths and, where the stem has at most kWave bytes, the bytes too (rf_mates_agree).  A read whose stems are equally long
// and longer than that is left for the whole wavefront: the reads so marked are taken one after the other, lane l comparing the
// bytes l, l + kWave, ... -- a 5 000-byte name keeps 64 lanes busy for 79 steps, not one lane for 5 000.
__global__ void __launch_bounds__(kBlock) k_names_match(const unsigned char* __restrict__ names1, const uint64_t* __restrict__ off1,
                                                        const unsigned char* __restrict__ names2, const uint64_t* __restrict__ off2,
                                                        uint64_t n_reads, unsigned long long* __restrict__ first) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const Bytes64 b1{names1}, b2{names2};
    uint64_t s1 = 0, s2 = 0, stem = 0;
    bool differ = false, wide = false;
    if (r < n_reads) {
        s1 = off1[r]; s2 = off2[r];
        const uint64_t len1 = off1[r + 1] - s1, len2 = off2[r + 1] - s2;
        stem = rf_mate_stem_len(b1, s1, len1);
        if (stem != rf_mate_stem_len(b2, s2, len2)) differ = true;
        else if (stem > (uint64_t)kWave) wide = true;
        else differ = !rf_mates_agree(b1, s1, len1, b2, s2, len2);
    }
    for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1) {       // wave-uniform
        const int src = __ffsll(todo) - 1;
        const uint64_t a1 = __shfl(s1, src), a2 = __shfl(s2, src), m = __shfl(stem, src);
        bool d = false;
        for (uint64_t k = lane; k < m; k += kWave) d |= b1(a1 + k) != b2(a2 + k);
        const bool any = __ballot(d) != 0;
        if ((int)lane == src) differ = any;
    }
    unsigned long long bad = differ ? (unsigned long long)r : ~0ull;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(bad, o);
        bad = other < bad ? other : bad;
    }
    if (lane == 0 && bad != ~0ull) atomicMin(first, bad);
}

const char* kind_text(int kind) {
    switch (kind) {
        case SFGPU_READS_BAD_START: return "the record does not begin with '@' (the text with neither '>' nor '@')";
        case SFGPU_READS_MISSING_PLUS: return "the third line does not begin with '+'";
        case SFGPU_READS_LENGTH_MISMATCH: return "quality and sequence differ in length";
        case SFGPU_READS_TRUNCATED: return "the last record has fewer than four lines";
        default: return "malformed";
    }
}

struct ReadScratch {
    DevBuf<uint4> text;
    DevBuf<uint32_t> nl_cnt, nl_scan, line_end, hdr, seq, hdr_scan, dst, rec_line;
    DevBuf<uint32_t> name_len, name_src, name_scan;     // the name blob only
    DevBuf<unsigned long long> misc;        // [0] first line error, [1] T, [2 .. 8] k_reads_cut's results
};

// Everything behind the newline counts, for both entries: text = the n_bytes, the appended '\n', zeros up to the end of its 16-byte
// group and one more group of zeros; S.nl_cnt holds the count of every group (work queued on st); S.misc is initialised.
// after_counts() runs behind the first wait for st (the host entry reads the times of its staged copies there).
template <typename AfterCounts>
int parse_counted(ReadScratch& S, const uint4* text, uint64_t n_bytes, int format, int final, uint64_t max_reads, uint8_t* d_bases,
                  uint8_t* d_qual, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, uint8_t* d_names, uint64_t cap_names,
                  uint64_t* d_name_off, uint64_t* n_name_bytes, sfgpu_reads_result* out, hipStream_t st, hipEvent_t* ev_p,
                  unsigned long long* h_res, AfterCounts after_counts) {
    const uint64_t n_groups = (n_bytes + 1 + 15) / 16;
    // ---- lines
    SF_HIP(hipEventRecord(ev_p[1], st));
    if (int r = exclusive_scan_u32_u32(S.nl_cnt.p, S.nl_scan.p, n_groups, st)) return r;
    SF_HIP(hipEventRecord(ev_p[2], st));
    SF_HIP(hipMemcpyAsync(&h_res[7], S.nl_scan.p + n_groups, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    after_counts();
    const uint32_t L = (uint32_t)h_res[7];                // >= 1: the appended '\n'
    out->n_lines = (uint64_t)L - 1 + (uint64_t)final;
    for (DevBuf<uint32_t>* b : {&S.line_end, &S.hdr, &S.seq, &S.hdr_scan, &S.dst, &S.rec_line})
        if (int r = b->reserve((uint64_t)L + 2, st, false)) return r;
    SF_HIP(hipEventRecord(ev_p[3], st));
    hipLaunchKernelGGL(textlines::k_line_ends, dim3(grid_of(n_groups)), dim3(kBlock), 0, st, text, n_groups, S.nl_scan.p, S.line_end.p);
    SF_HIP(hipGetLastError());
    const unsigned char* d_bytes = reinterpret_cast<const unsigned char*>(text);
    hipLaunchKernelGGL(k_reads_lines, dim3(grid_of(L)), dim3(kBlock), 0, st, d_bytes, format, final, L, S.line_end.p, S.hdr.p, S.seq.p, S.misc.p);
    SF_HIP(hipGetLastError());
    if (int r = exclusive_scan_u32_u32(S.hdr.p, S.hdr_scan.p, L, st)) return r;
    if (int r = exclusive_scan_u32_u32(S.seq.p, S.dst.p, L, st)) return r;
    hipLaunchKernelGGL(k_reads_rec_lines, dim3(grid_of((uint64_t)L + 1)), dim3(kBlock), 0, st, L, S.hdr.p, S.hdr_scan.p, S.rec_line.p);
    SF_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_reads_cut, dim3(1), dim3(kWave), 0, st, format, final, L, n_bytes, max_reads, cap_bases, S.line_end.p, S.hdr_scan.p,
                       S.dst.p, S.rec_line.p, S.misc.p, S.misc.p + 2);
    SF_HIP(hipGetLastError());
    SF_HIP(hipEventRecord(ev_p[4], st));
    SF_HIP(hipMemcpyAsync(h_res, S.misc.p + 2, 7 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    // a format error and the cap_bases range error do not leave at once: the kernel times below are still reported
    int rc = SFGPU_OK;
    bool emitting = false;
    if (h_res[0] != kReadsNoError) {
        out->error_record = h_res[0] >> 8; out->error_kind = (int32_t)(h_res[0] & 0xff); out->error_line = h_res[5];
        set_error("reads text: record %llu (line %llu of this text): %s", (unsigned long long)out->error_record,
                  (unsigned long long)out->error_line, kind_text(out->error_kind));
        rc = SFGPU_ERR_FORMAT;
    } else if (h_res[1] == 0 && h_res[4] > 0 && max_reads > 0) {
        set_error("sfgpu_reads_parse_host: the first record alone has more than cap_bases = %llu bases", (unsigned long long)cap_bases);
        rc = SFGPU_ERR_RANGE;
    } else {
        // ---- emission
        const uint32_t R = (uint32_t)h_res[1], n_bases = (uint32_t)h_res[2], Lc = (uint32_t)h_res[6];
        if (d_names)
            for (DevBuf<uint32_t>* b : {&S.name_len, &S.name_src, &S.name_scan})
                if (int r = b->reserve((uint64_t)R + 2, st, false)) return r;
        SF_HIP(hipEventRecord(ev_p[5], st));
        emitting = true;                                  // (a blob beyond cap_names stops it half way: its time is reported all the same)
        hipLaunchKernelGGL(k_reads_emit, dim3(grid_of((uint64_t)R + 1)), dim3(kBlock), 0, st, d_bytes, R, S.line_end.p, S.dst.p, S.rec_line.p,
                           d_off, d_name_span, d_names ? S.name_len.p : nullptr, d_names ? S.name_src.p : nullptr);
        SF_HIP(hipGetLastError());
        if (d_names) {
            // the blob's size decides whether the call emits anything, and the gather's grid: one more wait, only with names
            if (int r = exclusive_scan_u32_u32(S.name_len.p, S.name_scan.p, R, st)) return r;
            h_res[7] = 0;
            SF_HIP(hipMemcpyAsync(&h_res[7], S.name_scan.p + R, 4, hipMemcpyDeviceToHost, st));
            SF_HIP(hipStreamSynchronize(st));
            const uint32_t n_name = (uint32_t)h_res[7];
            if (n_name > cap_names) {
                set_error("reads text: the names of the %llu records need %llu bytes, more than cap_names = %llu",
                          (unsigned long long)R, (unsigned long long)n_name, (unsigned long long)cap_names);
                rc = SFGPU_ERR_RANGE;
            } else {
                const uint64_t lanes = (uint64_t)R + 1 > (n_name + 15ull) / 16 ? (uint64_t)R + 1 : (n_name + 15ull) / 16;
                hipLaunchKernelGGL(k_names_gather, dim3(grid_of(lanes)), dim3(kBlock), 0, st, text, R, n_name, S.name_scan.p, S.name_src.p,
                                   reinterpret_cast<uint4*>(d_names), d_name_off);
                SF_HIP(hipGetLastError());
                if (n_name_bytes) *n_name_bytes = n_name;
            }
        }
        if (rc == SFGPU_OK && n_bases) {
            hipLaunchKernelGGL(k_reads_compact<0>, dim3((n_bases + kTileBytes - 1) / kTileBytes), dim3(kBlock), 0, st, text, Lc, n_bases,
                               S.line_end.p, S.dst.p, reinterpret_cast<uint4*>(d_bases));
            SF_HIP(hipGetLastError());
            if (d_qual && format == SFGPU_READS_FASTQ) {
                hipLaunchKernelGGL(k_reads_compact<2>, dim3((n_bases + kTileBytes - 1) / kTileBytes), dim3(kBlock), 0, st, text, Lc, n_bases,
                                   S.line_end.p, S.dst.p, reinterpret_cast<uint4*>(d_qual));
                SF_HIP(hipGetLastError());
            }
        }
        if (rc == SFGPU_OK) { out->n_reads = R; out->n_bases = n_bases; out->consumed = h_res[3]; }
    }
    SF_HIP(hipEventRecord(ev_p[6], st));
    SF_HIP(hipStreamSynchronize(st));
    double lines = 0.0;                                   // both halves or neither
    if (add_elapsed(&lines, ev_p[1], ev_p[2]) && add_elapsed(&lines, ev_p[3], ev_p[4])) out->ms_kernels += lines;
    if (emitting) add_elapsed(&out->ms_kernels, ev_p[5], ev_p[6]);
    return rc;
}

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_reads_parse_host(const char* h_text, uint64_t n_bytes, int final, uint64_t max_reads, uint8_t* d_bases,
                                      uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, sfgpu_reads_result* out,
                                      sfgpu_stream stream) {
    return sfgpu_reads_parse_host_n(h_text, n_bytes, final, max_reads, d_bases, nullptr, cap_bases, d_off, d_name_span, nullptr, 0, nullptr, nullptr,
                                    out, stream);
}

extern "C" int sfgpu_reads_parse_host_q(const char* h_text, uint64_t n_bytes, int final, uint64_t max_reads, uint8_t* d_bases,
                                        uint8_t* d_qual, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, sfgpu_reads_result* out,
                                        sfgpu_stream stream) {
    return sfgpu_reads_parse_host_n(h_text, n_bytes, final, max_reads, d_bases, d_qual, cap_bases, d_off, d_name_span, nullptr, 0, nullptr, nullptr,
                                    out, stream);
}

extern "C" int sfgpu_reads_parse_host_n(const char* h_text, uint64_t n_bytes, int final, uint64_t max_reads, uint8_t* d_bases,
                                        uint8_t* d_qual, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, uint8_t* d_names,
                                        uint64_t cap_names, uint64_t* d_name_off, uint64_t* n_name_bytes, sfgpu_reads_result* out,
                                        sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_reads_parse_host: null result");
    memset(out, 0, sizeof(*out));
    out->error_record = ~0ull; out->error_line = ~0ull;
    SF_REQUIRE(n_bytes <= kReadsMaxBytes, SFGPU_ERR_RANGE, "sfgpu_reads_parse_host: more than 2^30 bytes in one call");
    SF_REQUIRE(n_bytes == 0 || h_text, SFGPU_ERR_INVALID, "sfgpu_reads_parse_host: null text");
    SF_REQUIRE(d_off && (d_bases || cap_bases == 0), SFGPU_ERR_INVALID, "sfgpu_reads_parse_host: null output");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_bases) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_reads_parse_host: d_bases must be 16-byte aligned");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_qual) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_reads_parse_host: d_qual must be 16-byte aligned");
    if (n_name_bytes) *n_name_bytes = 0;
    SF_REQUIRE(!d_names || ((reinterpret_cast<uintptr_t>(d_names) & 15u) == 0 && (cap_names & 15u) == 0), SFGPU_ERR_INVALID,
               "sfgpu_reads_parse_host: d_names must be 16-byte aligned and cap_names a multiple of 16");
    SF_REQUIRE(!d_names || d_name_off, SFGPU_ERR_INVALID, "sfgpu_reads_parse_host: a name blob without room for its offsets");
    final = final ? 1 : 0;
    hipStream_t st = as_stream(stream);
    SF_HIP(hipMemsetAsync(d_off, 0, sizeof(int64_t), st));
    if (d_names) SF_HIP(hipMemsetAsync(d_name_off, 0, sizeof(uint64_t), st));
    if (n_bytes == 0) { SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }
    const int format = rf_format_of((unsigned char)h_text[0]);
    out->format = format;
    if (format == SFGPU_READS_NONE) {
        SF_HIP(hipStreamSynchronize(st));
        if (rf_all_blank(h_text, n_bytes)) {
            for (uint64_t p = 0; p < n_bytes; ++p) out->n_lines += h_text[p] == '\n';
            out->n_lines += (uint64_t)final;
            out->consumed = final ? n_bytes : 0;
            return SFGPU_OK;
        }
        out->error_record = 0; out->error_line = 0; out->error_kind = SFGPU_READS_BAD_START;
        set_error("reads text: record 0: %s", kind_text(SFGPU_READS_BAD_START));
        return SFGPU_ERR_FORMAT;
    }

    // device text: the n_bytes, the appended '\n', zeros up to the group's end and one more group of zeros (load_unaligned16)
    const uint64_t n1 = n_bytes + 1, n_groups = (n1 + 15) / 16;
    const uint64_t n_sub = (n_bytes + kSubBytes - 1) / kSubBytes;
    ReadScratch S;
    CallScope scope;        // after S: it drains both streams before S's blocks go back to the pool; nothing is released while a copy still reads the pinned buffers
    hipStream_t cs = nullptr;
    char* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr}, ev_c0[2] = {nullptr, nullptr}, ev_c1[2] = {nullptr, nullptr};
    hipEvent_t ev_p[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    unsigned long long* h_res = nullptr;
    bool in_flight[2] = {false, false};

    // a slot's times are read when the slot is taken again, and at the end
    auto collect = [&](int slot) {
        if (!in_flight[slot]) return;
        (void)hipEventSynchronize(ev_c1[slot]);
        add_elapsed(&out->ms_copy, ev_h2d[slot], ev_copied[slot]);
        add_elapsed(&out->ms_kernels, ev_c0[slot], ev_c1[slot]);
        in_flight[slot] = false;
    };
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.acquire(&cs));
    for (int b = 0; b < 2 && (uint64_t)b < n_sub; ++b) {
        SF_HIP(scope.pinned_block(&pinned[b], (n_bytes < kSubBytes ? n_bytes : kSubBytes) + 48));
        for (hipEvent_t* e : {&ev_h2d[b], &ev_copied[b], &ev_c0[b], &ev_c1[b]}) SF_HIP(scope.event(e));
    }
    for (auto& e : ev_p) SF_HIP(scope.event(&e));
    SF_HIP(scope.pinned_block(&h_res, 8 * sizeof(unsigned long long)));
    if (int r = S.text.reserve(n_groups + 1, st, false)) return r;
    if (int r = S.nl_cnt.reserve(n_groups + 1, st, false)) return r;
    if (int r = S.nl_scan.reserve(n_groups + 1, st, false)) return r;
    if (int r = S.misc.reserve(16, st, false)) return r;
    SF_HIP(hipMemsetAsync(S.misc.p, 0xff, 8, st));
    SF_HIP(hipMemsetAsync(S.misc.p + 1, 0, 8, st));
    SF_HIP(hipEventRecord(ev_p[0], st));
    SF_HIP(hipStreamWaitEvent(cs, ev_p[0], 0));          // the copies stay behind whatever `stream` held and behind the reservations

    // ---- staged copy; the newlines of sub-chunk c are counted while sub-chunk c + 1 is copied
    for (uint64_t c = 0; c < n_sub; ++c) {
        const int slot = (int)(c & 1);
        collect(slot);                                   // its previous copy has left the pinned buffer
        const uint64_t p = c * kSubBytes, q = (c + 1 == n_sub) ? n_bytes : p + kSubBytes;
        uint64_t m = q - p;
        memcpy(pinned[slot], h_text + p, m);
        if (c + 1 == n_sub) {
            pinned[slot][m++] = '\n';
            const uint64_t padded = ((m + 15) & ~15ull) + 16;
            memset(pinned[slot] + m, 0, padded - m);
            m = padded;
        }
        SF_HIP(hipEventRecord(ev_h2d[slot], cs));
        SF_HIP(hipMemcpyAsync(reinterpret_cast<char*>(S.text.p) + p, pinned[slot], m, hipMemcpyHostToDevice, cs));
        SF_HIP(hipEventRecord(ev_copied[slot], cs));
        const uint64_t g0 = p / 16, g1 = (c + 1 == n_sub) ? n_groups : q / 16;
        SF_HIP(hipStreamWaitEvent(st, ev_copied[slot], 0));
        SF_HIP(hipEventRecord(ev_c0[slot], st));
        hipLaunchKernelGGL(k_reads_count, dim3(grid_of(g1 - g0)), dim3(kBlock), 0, st, S.text.p, g0, g1, S.nl_cnt.p);
        SF_HIP(hipGetLastError());
        SF_HIP(hipEventRecord(ev_c1[slot], st));
        in_flight[slot] = true;
    }

    return parse_counted(S, S.text.p, n_bytes, format, final, max_reads, d_bases, d_qual, cap_bases, d_off, d_name_span, d_names, cap_names, d_name_off,
                         n_name_bytes, out, st, ev_p, h_res,
                         [&]() { collect(0); collect(1); });
}

extern "C" int sfgpu_reads_parse_device(uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, uint64_t max_reads, uint8_t* d_bases,
                                        uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, sfgpu_reads_result* out,
                                        sfgpu_stream stream) {
    return sfgpu_reads_parse_device_n(d_text, n_bytes, cap_text, final, max_reads, d_bases, nullptr, cap_bases, d_off, d_name_span, nullptr, 0,
                                      nullptr, nullptr, out, stream);
}

extern "C" int sfgpu_reads_parse_device_q(uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, uint64_t max_reads, uint8_t* d_bases,
                                          uint8_t* d_qual, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, sfgpu_reads_result* out,
                                          sfgpu_stream stream) {
    return sfgpu_reads_parse_device_n(d_text, n_bytes, cap_text, final, max_reads, d_bases, d_qual, cap_bases, d_off, d_name_span, nullptr, 0,
                                      nullptr, nullptr, out, stream);
}

extern "C" int sfgpu_reads_parse_device_n(uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, uint64_t max_reads, uint8_t* d_bases,
                                          uint8_t* d_qual, uint64_t cap_bases, int64_t* d_off, uint64_t* d_name_span, uint8_t* d_names,
                                          uint64_t cap_names, uint64_t* d_name_off, uint64_t* n_name_bytes, sfgpu_reads_result* out,
                                          sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_reads_parse_device: null result");
    memset(out, 0, sizeof(*out));
    out->error_record = ~0ull; out->error_line = ~0ull;
    SF_REQUIRE(n_bytes <= kReadsMaxBytes, SFGPU_ERR_RANGE, "sfgpu_reads_parse_device: more than 2^30 bytes in one call");
    SF_REQUIRE(n_bytes == 0 || d_text, SFGPU_ERR_INVALID, "sfgpu_reads_parse_device: null text");
    SF_REQUIRE(d_off && (d_bases || cap_bases == 0), SFGPU_ERR_INVALID, "sfgpu_reads_parse_device: null output");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_bases) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_reads_parse_device: d_bases must be 16-byte aligned");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_qual) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_reads_parse_device: d_qual must be 16-byte aligned");
    if (n_name_bytes) *n_name_bytes = 0;
    SF_REQUIRE(!d_names || ((reinterpret_cast<uintptr_t>(d_names) & 15u) == 0 && (cap_names & 15u) == 0), SFGPU_ERR_INVALID,
               "sfgpu_reads_parse_device: d_names must be 16-byte aligned and cap_names a multiple of 16");
    SF_REQUIRE(!d_names || d_name_off, SFGPU_ERR_INVALID, "sfgpu_reads_parse_device: a name blob without room for its offsets");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_reads_parse_device: d_text must be 16-byte aligned");
    const uint64_t n1 = n_bytes + 1, n_groups = (n1 + 15) / 16, padded = 16 * n_groups + 16;
    SF_REQUIRE(n_bytes == 0 || cap_text >= padded, SFGPU_ERR_INVALID,
               "sfgpu_reads_parse_device: cap_text must hold the text, its '\\n', the rest of that 16-byte group and one group more");
    final = final ? 1 : 0;
    hipStream_t st = as_stream(stream);
    SF_HIP(hipMemsetAsync(d_off, 0, sizeof(int64_t), st));
    if (d_names) SF_HIP(hipMemsetAsync(d_name_off, 0, sizeof(uint64_t), st));
    if (n_bytes == 0) { SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }

    ReadScratch S;          // S.text stays empty: the text is the caller's
    CallScope scope;        // after S, as in sfgpu_reads_parse_host
    hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr;
    hipEvent_t ev_p[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    unsigned long long* h_res = nullptr;                 // [0 .. 8) parse_counted's, [8] the first byte, [8 .. 10) the blank counts
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_c0));
    SF_HIP(scope.event(&ev_c1));
    for (auto& e : ev_p) SF_HIP(scope.event(&e));
    SF_HIP(scope.pinned_block(&h_res, 10 * sizeof(unsigned long long)));
    h_res[8] = 0;
    SF_HIP(hipMemcpyAsync(&h_res[8], d_text, 1, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const int format = rf_format_of((unsigned char)(h_res[8] & 0xffu));
    out->format = format;
    if (int r = S.misc.reserve(16, st, false)) return r;
    if (format == SFGPU_READS_NONE) {
        SF_HIP(hipMemsetAsync(S.misc.p, 0, 16, st));
        hipLaunchKernelGGL(k_reads_blank, dim3(grid_of((n_bytes + 15) / 16)), dim3(kBlock), 0, st, d_text, n_bytes, S.misc.p);
        SF_HIP(hipGetLastError());
        SF_HIP(hipMemcpyAsync(&h_res[8], S.misc.p, 16, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        if (h_res[8] == 0) {
            out->n_lines = h_res[9] + (uint64_t)final;
            out->consumed = final ? n_bytes : 0;
            return SFGPU_OK;
        }
        out->error_record = 0; out->error_line = 0; out->error_kind = SFGPU_READS_BAD_START;
        set_error("reads text: record 0: %s", kind_text(SFGPU_READS_BAD_START));
        return SFGPU_ERR_FORMAT;
    }
    SF_HIP(hipMemsetAsync(d_text + n_bytes, '\n', 1, st));
    SF_HIP(hipMemsetAsync(d_text + n1, 0, padded - n1, st));
    if (int r = S.nl_cnt.reserve(n_groups + 1, st, false)) return r;
    if (int r = S.nl_scan.reserve(n_groups + 1, st, false)) return r;
    SF_HIP(hipMemsetAsync(S.misc.p, 0xff, 8, st));
    SF_HIP(hipMemsetAsync(S.misc.p + 1, 0, 8, st));
    const uint4* text = reinterpret_cast<const uint4*>(d_text);
    SF_HIP(hipEventRecord(ev_c0, st));
    hipLaunchKernelGGL(k_reads_count, dim3(grid_of(n_groups)), dim3(kBlock), 0, st, text, (uint64_t)0, n_groups, S.nl_cnt.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipEventRecord(ev_c1, st));
    return parse_counted(S, text, n_bytes, format, final, max_reads, d_bases, d_qual, cap_bases, d_off, d_name_span, d_names, cap_names, d_name_off,
                         n_name_bytes, out, st, ev_p, h_res,
                         [&]() { add_elapsed(&out->ms_kernels, ev_c0, ev_c1); });
}

extern "C" int sfgpu_reads_names_match(const uint8_t* d_names1, const uint64_t* d_off1, const uint8_t* d_names2, const uint64_t* d_off2,
                                       uint64_t n_reads, uint64_t* first_mismatch, sfgpu_stream stream) {
    SF_REQUIRE(first_mismatch, SFGPU_ERR_INVALID, "sfgpu_reads_names_match: null result");
    *first_mismatch = ~0ull;
    SF_REQUIRE(n_reads == 0 || (d_off1 && d_off2), SFGPU_ERR_INVALID, "sfgpu_reads_names_match: null offsets");
    SF_REQUIRE(n_reads <= kReadsMaxBytes, SFGPU_ERR_RANGE, "sfgpu_reads_names_match: more than 2^30 reads in one call");
    if (n_reads == 0) return SFGPU_OK;
    hipStream_t st = as_stream(stream);
    DevBuf<unsigned long long> first;
    CallScope scope;        // after the scratch, as in sfgpu_reads_parse_host
    unsigned long long* h_first = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.pinned_block(&h_first, sizeof(unsigned long long)));
    if (int r = first.reserve(1, st, false)) return r;
    SF_HIP(hipMemsetAsync(first.p, 0xff, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_names_match, dim3(grid_of(n_reads)), dim3(kBlock), 0, st, d_names1, d_off1, d_names2, d_off2, n_reads, first.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(h_first, first.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    *first_mismatch = *h_first;
    return SFGPU_OK;
}
