// bamwrite_harness.cpp -- csrc/bamwfmt.h alone, as plain C++: the serial record writer (bamw_serial) behind a C interface for
// tests/test_bamwrite_cpu.py, which compares its bytes with samfile.sam_to_bam(samfile._sam_text(...)).  The per-unit functions the
// kernels call (bamw_unit_len, bamw_check) are cross-checked against the serial pass on the way.
#include "bamwfmt.h"

using namespace sfgpu;

namespace {

SamwArgs args_of(const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off, uint32_t n_refs,
                 const char* q, const uint64_t* q_off, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2, const int64_t* s2_off,
                 uint64_t read_index_base) {
    return SamwArgs{static_cast<const sfgpu_hit*>(hits), hit_off, n_reads, paired, ref, ref_off, n_refs, q, q_off, s1, s1_off,
                    paired ? s2 : nullptr, paired ? s2_off : nullptr, read_index_base};
}

}  // namespace

extern "C" {

// out[0 .. 8): n_bytes, n_lines, n_units, max_unit_bytes, error_kind, error_read, error_record, 1 when the per-unit sizes disagree
int bamw_harness_size(const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off,
                      uint32_t n_refs, const char* q, const uint64_t* q_off, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2,
                      const int64_t* s2_off, uint64_t read_index_base, uint64_t* out) {
    const SamwArgs a = args_of(hits, hit_off, n_reads, paired, ref, ref_off, n_refs, q, q_off, s1, s1_off, s2, s2_off, read_index_base);
    SamwSerial res;
    const int kind = bamw_serial(a, nullptr, &res);
    uint64_t sum = 0, longest = 0, units = 0;
    auto unit = [&](uint64_t len) {
        sum += len; ++units;
        if (len > longest) longest = len;
    };
    for (uint64_t r = 0; !kind && r < a.n_reads; ++r) {
        const uint64_t h0 = a.hit_off[r], h1 = a.hit_off[r + 1];
        if (h0 == h1) unit(bamw_unit_len(a, r, nullptr, 0));
        for (uint64_t h = h0; h < h1; ++h) unit(bamw_unit_len(a, r, a.hits + h, h - h0));
    }
    out[0] = res.n_bytes; out[1] = res.n_lines; out[2] = res.n_units; out[3] = res.max_unit_bytes;
    out[4] = (uint64_t)kind; out[5] = res.error_read; out[6] = res.error_record;
    out[7] = !kind && (sum != res.n_bytes || longest != res.max_unit_bytes || units != res.n_units);
    return kind;
}

// the records into `bytes`, which has room for the n_bytes bamw_harness_size gave; returns the error kind (nothing is written then)
int bamw_harness_format(const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off,
                        uint32_t n_refs, const char* q, const uint64_t* q_off, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2,
                        const int64_t* s2_off, uint64_t read_index_base, uint8_t* bytes) {
    const SamwArgs a = args_of(hits, hit_off, n_reads, paired, ref, ref_off, n_refs, q, q_off, s1, s1_off, s2, s2_off, read_index_base);
    SamwSerial res;
    return bamw_serial(a, bytes, &res);
}

uint32_t bamw_harness_reg2bin(uint32_t beg, uint32_t end) { return bamw_reg2bin(beg, end); }

}  // extern "C"
