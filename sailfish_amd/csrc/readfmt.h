// readfmt.h -- what a FASTA / FASTQ record is, as functions both sides call: the kernels of readtext.hip (sfgpu_reads_parse_host)
// and plain C++ (tests/readfile_harness.cpp compiles this header with g++ and runs the same rules serially).
//
// A parse call sees a text of n bytes that begins at a record start; its first byte fixes the format ('>' FASTA, '@' FASTQ).
// LINES.  With NL '\n' bytes the text has L = NL + 1 lines: line i runs from behind the (i - 1)-th '\n' to the i-th, and the last
// one, the REMAINDER, from behind the last '\n' to the end of the text (it may be empty).  With final == 1 the remainder is a
// line like any other (the last line of a file may lack its '\n'); with final == 0 it is an unfinished line: FASTQ ignores it,
// FASTA only asks whether it begins with '>'.  One '\r' directly before the line end is not part of the line.
// FASTQ.  Line i has kind i mod 4 (header, sequence, plus, quality) and belongs to record i / 4 -- nothing else is looked at, so a
// quality line that begins with '@' or '+' is a quality line.  With T = 1 + the last non-empty usable line, the text holds
// ceil(T / 4) records when final (a record whose four lines are not all there is TRUNCATED) and floor(T / 4) otherwise: empty
// lines behind the last record belong to nobody.
// FASTA.  A line that begins with '>' opens a record; every other line adds its bytes to the open record.  With H header lines
// the text holds H records when final and H - 1 otherwise (the last one is still open).
// ERRORS.  Every line of a record the text holds is checked; the smallest (record << 8 | kind) wins, and a call that reports an
// error emits nothing.
#pragma once
#include <cstdint>

#include "../../include/sfgpu.h"

#if defined(__HIPCC__)
#define SF_READFMT_HD __host__ __device__ __forceinline__
#else
#define SF_READFMT_HD inline
#endif

namespace sfgpu {

constexpr uint64_t kReadsMaxBytes = 1ull << 30;           // one call's text: every offset of it fits 32 bits
constexpr unsigned long long kReadsNoError = ~0ull;

SF_READFMT_HD int rf_format_of(unsigned char first) {
    return first == '>' ? SFGPU_READS_FASTA : first == '@' ? SFGPU_READS_FASTQ : SFGPU_READS_NONE;
}

// a text of nothing but line ends holds no record and is no error (what is left of a file behind its last record)
inline bool rf_all_blank(const char* text, uint64_t n) {
    uint64_t p = 0;
    while (p < n && (text[p] == '\n' || text[p] == '\r')) ++p;
    return p == n;
}

// bytes of the line [s, e) without the '\r' of a CRLF line end
template <typename Byte>
SF_READFMT_HD uint32_t rf_line_len(Byte byte, uint32_t s, uint32_t e) {
    return (e > s && byte(e - 1) == '\r') ? e - s - 1 : e - s;
}

struct RfLine {
    uint32_t len;        // bytes without the line end
    uint32_t header;     // 1: the line opens a record
    uint32_t seq;        // bases the line adds to its record
    int32_t error;       // SFGPU_READS_* of the check this line fails, 0 = none (FASTQ only; the record is i / 4)
};

// Line i of L.  byte(p) -> the p-th byte of the text; bounds(j, &s, &e) -> where line j begins and ends (its '\n', or the end
// of the text for the remainder).
template <typename Byte, typename Bounds>
SF_READFMT_HD RfLine rf_line(int format, int final, uint32_t i, uint32_t L, Byte byte, Bounds bounds) {
    uint32_t s, e;
    bounds(i, &s, &e);
    RfLine r;
    r.len = rf_line_len(byte, s, e);
    r.header = 0; r.seq = 0; r.error = 0;
    const bool unfinished = !final && i == L - 1;
    if (format == SFGPU_READS_FASTA) {
        r.header = (e > s && byte(s) == '>') ? 1u : 0u;
        if (!r.header && !unfinished) r.seq = r.len;
        return r;
    }
    r.header = (i & 3u) == 0 ? 1u : 0u;
    if (unfinished) { r.len = 0; return r; }                 // not a line yet: neither checked nor counted as non-empty
    switch (i & 3u) {
        case 0: if (!(e > s && byte(s) == '@')) r.error = SFGPU_READS_BAD_START; break;
        case 1: r.seq = r.len; break;
        case 2: if (!(e > s && byte(s) == '+')) r.error = SFGPU_READS_MISSING_PLUS; break;
        default: {
            uint32_t qs, qe;
            bounds(i - 2, &qs, &qe);
            if (rf_line_len(byte, qs, qe) != r.len) r.error = SFGPU_READS_LENGTH_MISMATCH;
        }
    }
    return r;
}

// name of the record whose header line is [s, s + len): the bytes behind the '>' / '@' up to the first space or tab
template <typename Byte>
SF_READFMT_HD uint32_t rf_name_len(Byte byte, uint32_t s, uint32_t len) {
    uint32_t k = 1;
    while (k < len && byte(s + k) != ' ' && byte(s + k) != '\t') ++k;
    return k - 1;
}

// NAME BLOB.  The names of the records a call emits (those in front of the max_reads / cap_bases cut, not all the text holds) lie
// back to back: name_off[r] = the sum of the name lengths of the records before r (name_off[0] = 0), name_off[R] = the bytes of the
// blob.  A name may be empty.  rf_blob_record says whose byte the blob's byte o is: the r < R with name_off[r] <= o < name_off[r + 1]
// (there is one for every o < name_off[R]; records with empty names own no byte).
template <typename Off>
SF_READFMT_HD uint32_t rf_blob_record(uint32_t R, uint32_t o, Off name_off) {
    uint32_t lo = 0, hi = R;                                 // name_off(lo) <= o < name_off(hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (name_off(mid) <= o) lo = mid; else hi = mid;
    }
    return lo;
}

// MATES.  The stem of a name of len bytes at s: the name without a trailing "/1" or "/2" (the mark some tools put on the mates of a
// pair), whichever of the two digits it is; any other name is its own stem.  Two mates AGREE iff their stems are of equal length
// and equal bytes: x/1 ~ x/2 ~ x, while x/3 is not x.
template <typename Byte>
SF_READFMT_HD uint64_t rf_mate_stem_len(Byte byte, uint64_t s, uint64_t len) {
    return (len >= 2 && byte(s + len - 2) == '/' && (byte(s + len - 1) == '1' || byte(s + len - 1) == '2')) ? len - 2 : len;
}

template <typename Byte1, typename Byte2>
SF_READFMT_HD bool rf_mates_agree(Byte1 byte1, uint64_t s1, uint64_t len1, Byte2 byte2, uint64_t s2, uint64_t len2) {
    const uint64_t m = rf_mate_stem_len(byte1, s1, len1);
    if (m != rf_mate_stem_len(byte2, s2, len2)) return false;
    for (uint64_t k = 0; k < m; ++k)
        if (byte1(s1 + k) != byte2(s2 + k)) return false;
    return true;
}

struct RfCount {
    uint32_t records;     // records the text holds
    uint32_t truncated;   // FASTQ, final: the last of them lacks lines
    uint32_t usable;      // lines that count (L, or L - 1 with an unfinished remainder in FASTQ)
};

// T = 1 + the last usable line with len > 0 (0 without one); H = header lines among the L lines
SF_READFMT_HD RfCount rf_count_records(int format, int final, uint32_t L, uint32_t T, uint32_t H) {
    RfCount c;
    c.truncated = 0;
    if (format == SFGPU_READS_FASTA) {
        c.usable = L;
        c.records = final ? H : (H ? H - 1 : 0);
        return c;
    }
    c.usable = final ? L : L - 1;
    c.records = final ? (T + 3) / 4 : T / 4;
    c.truncated = (final && 4ull * c.records > c.usable) ? 1u : 0u;
    return c;
}

// the error a call reports: what the line checks found (smallest (record << 8 | kind), all lines) cut down to the records the
// text holds, and the truncated last record
SF_READFMT_HD unsigned long long rf_final_error(unsigned long long line_error, const RfCount c) {
    unsigned long long err = kReadsNoError;
    if (line_error != kReadsNoError && (line_error >> 8) < c.records) err = line_error;
    if (c.truncated) {
        const unsigned long long t = ((unsigned long long)(c.records - 1) << 8) | (unsigned long long)SFGPU_READS_TRUNCATED;
        if (t < err) err = t;
    }
    return err;
}

// line of the failed check within the call's text: the line itself, or for TRUNCATED the first line that is missing
SF_READFMT_HD uint64_t rf_error_line(unsigned long long err, const RfCount c) {
    const uint64_t rec = err >> 8;
    switch ((int)(err & 0xff)) {
        case SFGPU_READS_MISSING_PLUS: return 4 * rec + 2;
        case SFGPU_READS_LENGTH_MISMATCH: return 4 * rec + 3;
        case SFGPU_READS_TRUNCATED: return c.usable;
        default: return 4 * rec;
    }
}

// records emitted: the largest R <= min(records, max_reads) with off(R) <= cap_bases; off(r) = bases before record r, never decreasing
template <typename Off>
SF_READFMT_HD uint32_t rf_cut(uint32_t records, uint64_t max_reads, uint64_t cap_bases, Off off) {
    uint32_t lo = 0, hi = (uint64_t)records < max_reads ? records : (uint32_t)max_reads;
    if (off(hi) <= cap_bases) return hi;
    while (hi - lo > 1) {                                    // off(lo) <= cap_bases < off(hi)
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off(mid) <= cap_bases) lo = mid; else hi = mid;
    }
    return lo;
}

// bytes through the end of record R - 1: where the line that opens record R begins; everything when the last record of a final
// text goes out (empty lines behind it go with it)
SF_READFMT_HD uint64_t rf_consumed(int final, uint32_t R, uint32_t records, uint64_t n_bytes, uint32_t next_record_begin) {
    if (R == 0) return 0;
    return (final && R == records) ? n_bytes : next_record_begin;
}

}  // namespace sfgpu
