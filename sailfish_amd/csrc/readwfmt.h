// readwfmt.h -- what a FASTA / FASTQ record says when it is WRITTEN, as functions both sides call: the kernels of readtext_write.hip
// (sfgpu_reads_write_text, sfgpu_reads_write_bgzf) and plain C++ (tests/readwrite_harness.cpp compiles this header with g++ and runs
// the same rules serially).  The mirror of readfmt.h; the host statement it is judged by is readfile.reads_text_host.
//
// A BATCH is n_reads records (n_reads < 2^32 - 1): the bases back to back with int64 offsets off[0 .. n_reads], optionally the
// qualities, which share the bases' offsets (readfile.ReadFile(quals=True).last_quals), optionally the names back to back with
// 64-bit offsets name_off[0 .. n_reads] (ReadFile(names="device").last_names), and optionally a selector of one byte a record:
// nonzero = write it, no selector = write all.  The TEXT is the selected records in input order; nothing is written for the others.
//   FASTQ (qualities given)   '@' name '\n' bases '\n' '+' '\n' qualities '\n'     name + 2 len + 6 bytes
//   FASTA (no qualities)      '>' name '\n' bases '\n'                              name + len + 3 bytes, never wrapped
// Bases and qualities are written as given, in the orientation as sequenced; a record of 0 bases has empty lines.  Without names
// the name of record r is 'r' and the decimal of read_index_base + r: the SAM writer's QNAME (samwfmt.h).  A name may be empty.
// ERRORS.  Only selected records are checked; the smallest (record << 8 | kind) wins, as in readfmt.h, and a call that reports one
// writes nothing.  Kind 1: a name holds '\n'; 2: the bases hold '\n'; 3: the qualities hold '\n'; 4: FASTA and the first base is
// '>' (the line would open a record).  A '\r' is written as given: the promise is lines without '\n', not CRLF hygiene.
// ROUND TRIP.  Parsing the text of a batch without an error by readfmt.h's rules (final = 1) yields exactly the selected records,
// names, bases and qualities unchanged, provided no name holds a blank and no line ends in '\r'.
#pragma once
#include <cstdint>

#include "../../include/sfgpu.h"
#include "decfmt.h"

#if defined(__HIPCC__)
#define READW_HD __host__ __device__ __forceinline__
#else
#define READW_HD inline
#endif

namespace sfgpu {

constexpr unsigned long long kReadwNoError = ~0ull;
constexpr uint32_t kReadwFastqFixed = 6;          // '@' '\n' '\n' '+' '\n' '\n'
constexpr uint32_t kReadwFastaFixed = 3;          // '>' '\n' '\n'

struct ReadwArgs {
    const uint8_t* bases;
    const int64_t* off;             // n_reads + 1
    uint64_t n_reads;
    const uint8_t* qual;            // shares `off`; NULL: FASTA
    const uint8_t* names;
    const uint64_t* name_off;       // n_reads + 1; NULL: generated names
    uint64_t read_index_base;
    const uint8_t* select;          // n_reads; NULL: every record
};

READW_HD bool readw_fastq(const ReadwArgs& a) { return a.qual != nullptr; }
READW_HD bool readw_selected(const ReadwArgs& a, uint64_t r) { return !a.select || a.select[r] != 0; }
READW_HD unsigned long long readw_error_key(uint64_t r, int kind) { return (unsigned long long)r << 8 | (unsigned long long)kind; }

// the generated name of the record with running index `index`: the SAM writer's default QNAME
READW_HD uint32_t readw_default_name_len(uint64_t index) { return 1u + (uint32_t)dec_len_u64(index); }
template <typename Put>
READW_HD void readw_put_default_name(uint64_t index, Put put) {             // put(i, ch): byte i of the name
    const int nd = dec_len_u64(index);
    put(0, 'r');
    dec_put_u64(index, [&](int i, char ch) { put(nd - i, ch); });
}

READW_HD uint64_t readw_name_len(const ReadwArgs& a, uint64_t r) {
    return a.name_off ? a.name_off[r + 1] - a.name_off[r] : (uint64_t)readw_default_name_len(a.read_index_base + r);
}
READW_HD uint64_t readw_seq_len(const ReadwArgs& a, uint64_t r) { return (uint64_t)(a.off[r + 1] - a.off[r]); }

// bytes of record r in the text
READW_HD uint64_t readw_record_len(const ReadwArgs& a, uint64_t r) {
    const uint64_t len = readw_seq_len(a, r);
    return readw_name_len(a, r) + (readw_fastq(a) ? 2 * len + kReadwFastqFixed : len + kReadwFastaFixed);
}

// kind 4, the one check that is a record's own (the '\n' checks are flat passes over the bytes on the device)
READW_HD bool readw_fasta_seq_start(const ReadwArgs& a, uint64_t r) {
    return !readw_fastq(a) && a.off[r + 1] > a.off[r] && a.bases[a.off[r]] == '>';
}

// the lowest kind record r breaks, 0 = none: what the flat passes and readw_fasta_seq_start find together
READW_HD int readw_check(const ReadwArgs& a, uint64_t r) {
    if (a.name_off)
        for (uint64_t i = a.name_off[r]; i < a.name_off[r + 1]; ++i)
            if (a.names[i] == '\n') return SFGPU_READW_NAME_NEWLINE;
    for (int64_t i = a.off[r]; i < a.off[r + 1]; ++i)
        if (a.bases[i] == '\n') return SFGPU_READW_SEQ_NEWLINE;
    if (a.qual)
        for (int64_t i = a.off[r]; i < a.off[r + 1]; ++i)
            if (a.qual[i] == '\n') return SFGPU_READW_QUAL_NEWLINE;
    return readw_fasta_seq_start(a, r) ? SFGPU_READW_FASTA_SEQ_START : 0;
}

#if !defined(__HIPCC__)
// The whole text, serially (host only; the judge of the kernels is still reads_text_host).  Pass 1 (out == nullptr) sizes and
// checks; pass 2 (room for n_bytes) writes.
struct ReadwSerial {
    uint64_t n_selected = 0, n_bytes = 0, max_record_bytes = 0, error_record = 0;
    int error_kind = 0;
};

inline ReadwSerial readw_serial(const ReadwArgs& a, uint8_t* out) {
    ReadwSerial s;
    unsigned long long err = kReadwNoError;
    for (uint64_t r = 0; r < a.n_reads; ++r) {
        if (!readw_selected(a, r)) continue;
        ++s.n_selected;
        if (const int kind = readw_check(a, r)) {
            if (readw_error_key(r, kind) < err) err = readw_error_key(r, kind);
            continue;
        }
        const uint64_t len = readw_record_len(a, r);
        s.n_bytes += len;
        if (len > s.max_record_bytes) s.max_record_bytes = len;
    }
    if (err != kReadwNoError) {
        s.error_record = err >> 8; s.error_kind = (int)(err & 0xff);
        s.n_bytes = 0; s.max_record_bytes = 0;
        return s;
    }
    if (!out) return s;
    uint8_t* p = out;
    for (uint64_t r = 0; r < a.n_reads; ++r) {
        if (!readw_selected(a, r)) continue;
        *p++ = readw_fastq(a) ? '@' : '>';
        if (a.name_off) for (uint64_t i = a.name_off[r]; i < a.name_off[r + 1]; ++i) *p++ = a.names[i];
        else { readw_put_default_name(a.read_index_base + r, [&](int i, char ch) { p[i] = (uint8_t)ch; }); p += readw_default_name_len(a.read_index_base + r); }
        *p++ = '\n';
        for (int64_t i = a.off[r]; i < a.off[r + 1]; ++i) *p++ = a.bases[i];
        *p++ = '\n';
        if (readw_fastq(a)) {
            *p++ = '+'; *p++ = '\n';
            for (int64_t i = a.off[r]; i < a.off[r + 1]; ++i) *p++ = a.qual[i];
            *p++ = '\n';
        }
    }
    return s;
}
#endif

}  // namespace sfgpu
