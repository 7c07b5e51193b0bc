// samqual_harness.cpp -- csrc/samwfmt.h and csrc/bamwfmt.h alone, as plain C++, with the inputs sfgpu_sam_write_text adds: the
// qualities of either mate and the orientation.  The serial writers (samw_serial, bamw_serial) behind one C call for
// tests/test_samqual_cpu.py, which compares their bytes with samfile._sam_text(..., quals=, oriented=) and sam_to_bam of it, and --
// with -DSAMQ_HARNESS_MAIN -- a stand-alone program over case files for the sanitizer run.  The per-unit sizes the kernels take
// (samw_unit_len, bamw_unit_len) are cross-checked against the serial pass on the way.
#include "bamwfmt.h"

#include <cstdio>
#include <string>
#include <vector>

using namespace sfgpu;

namespace {

// out[0 .. 8): n_bytes, n_lines, n_units, max_unit_bytes, error_kind, error_read, error_record, 1 when the per-unit sizes disagree;
// bytes != nullptr (room for the n_bytes a first call gave): the text or the records, unless the batch cannot be written
int run(int bam, const SamwArgs& a, uint64_t* out, uint8_t* bytes) {
    SamwSerial res;
    const int kind = bam ? bamw_serial(a, nullptr, &res) : samw_serial(a, nullptr, &res);
    uint64_t sum = 0, longest = 0, units = 0;
    auto unit = [&](uint64_t len) {
        sum += len; ++units;
        if (len > longest) longest = len;
    };
    for (uint64_t r = 0; !kind && r < a.n_reads; ++r) {
        const uint64_t h0 = a.hit_off[r], h1 = a.hit_off[r + 1];
        if (h0 == h1) unit(bam ? bamw_unit_len(a, r, nullptr, 0) : samw_unit_len(a, r, nullptr, 0));
        for (uint64_t h = h0; h < h1; ++h) unit(bam ? bamw_unit_len(a, r, a.hits + h, h - h0) : samw_unit_len(a, r, a.hits + h, h - h0));
    }
    out[0] = res.n_bytes; out[1] = res.n_lines; out[2] = res.n_units; out[3] = res.max_unit_bytes;
    out[4] = (uint64_t)kind; out[5] = res.error_read; out[6] = res.error_record;
    out[7] = !kind && (sum != res.n_bytes || longest != res.max_unit_bytes || units != res.n_units);
    if (kind || !bytes) return kind;
    SamwSerial again;
    const int k2 = bam ? bamw_serial(a, bytes, &again) : samw_serial(a, reinterpret_cast<char*>(bytes), &again);
    if (k2 || again.n_bytes != res.n_bytes) out[7] = 1;
    return k2;
}

SamwArgs args_of(const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off, uint32_t n_refs,
                 const char* q, const uint64_t* q_off, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2, const int64_t* s2_off,
                 const uint8_t* k1, const uint8_t* k2, int oriented, uint64_t read_index_base) {
    SamwArgs a = {static_cast<const sfgpu_hit*>(hits), hit_off, n_reads, paired, ref, ref_off, n_refs, q, q_off, s1, s1_off,
                  paired ? s2 : nullptr, paired ? s2_off : nullptr, read_index_base};
    a.qual1 = k1; a.qual2 = paired ? k2 : nullptr; a.oriented = oriented;
    return a;
}

}  // namespace

extern "C" {

// the arrays of sfgpu_sam_write_text (host pointers); k1 / k2: the qualities at the offsets of s1 / s2, nullptr for none.
// Returns -1 for qualities of a mate whose bases are not given (the entry's SFGPU_ERR_INVALID), else the error kind.
int samq_harness(int bam, const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off,
                 uint32_t n_refs, const char* q, const uint64_t* q_off, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2,
                 const int64_t* s2_off, const uint8_t* k1, const uint8_t* k2, int oriented, uint64_t read_index_base, uint64_t* out,
                 uint8_t* bytes) {
    if ((k1 && !s1_off) || (k2 && !s2_off)) return -1;
    return run(bam, args_of(hits, hit_off, n_reads, paired, ref, ref_off, n_refs, q, q_off, s1, s1_off, s2, s2_off, k1, k2, oriented, read_index_base),
               out, bytes);
}

uint8_t samq_comp(uint8_t c) { return samw_comp(c); }

}  // extern "C"

#ifdef SAMQ_HARNESS_MAIN
// samqual_harness_san CASE...: a case file is 16 uint64 (n_reads, n_hits, paired, n_refs, has names, has seq1, has seq2,
// read_index_base, bytes of the reference names, of the read names, of seq1, of seq2, has qual1, has qual2, oriented, bam) and then
// the arrays in the order of the call (hits, hit offsets, reference names, their offsets, read names, offsets, seq1, offsets, seq2,
// offsets, qual1, qual2; absent ones left out).  Writes CASE.out (the text or the records) and prints one line per case.
namespace {

template <typename T>
bool take(FILE* f, std::vector<T>* v, uint64_t n) {
    v->resize(n);
    return n == 0 || fread(v->data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        uint64_t h[16];
        if (fread(h, 8, 16, f) != 16) { fprintf(stderr, "%s: short header\n", argv[i]); return 2; }
        std::vector<sfgpu_hit> hits;
        std::vector<uint32_t> hit_off;
        std::vector<char> ref, q;
        std::vector<uint64_t> ref_off, q_off;
        std::vector<uint8_t> s1, s2, k1, k2;
        std::vector<int64_t> s1_off, s2_off;
        bool ok = take(f, &hits, h[1]) && take(f, &hit_off, h[0] + 1) && take(f, &ref, h[8]) && take(f, &ref_off, h[3] + 1);
        if (h[4]) ok = ok && take(f, &q, h[9]) && take(f, &q_off, h[0] + 1);
        if (h[5]) ok = ok && take(f, &s1, h[10]) && take(f, &s1_off, h[0] + 1);
        if (h[6]) ok = ok && take(f, &s2, h[11]) && take(f, &s2_off, h[0] + 1);
        if (h[12]) ok = ok && take(f, &k1, h[10] ? h[10] : 1);
        if (h[13]) ok = ok && take(f, &k2, h[11] ? h[11] : 1);
        fclose(f);
        if (!ok) { fprintf(stderr, "%s: short file\n", argv[i]); return 2; }
        const SamwArgs a = args_of(hits.data(), hit_off.data(), (uint32_t)h[0], (int)h[2], ref.data(), ref_off.data(), (uint32_t)h[3],
                                   h[4] ? q.data() : nullptr, h[4] ? q_off.data() : nullptr, h[5] ? s1.data() : nullptr,
                                   h[5] ? s1_off.data() : nullptr, h[6] ? s2.data() : nullptr, h[6] ? s2_off.data() : nullptr,
                                   h[12] ? k1.data() : nullptr, h[13] ? k2.data() : nullptr, (int)h[14], h[7]);
        uint64_t out[8];
        const int kind = run((int)h[15], a, out, nullptr);
        std::vector<uint8_t> bytes(kind ? 0 : out[0]);
        if (!kind) {
            if (run((int)h[15], a, out, bytes.data()) || out[7]) { fprintf(stderr, "%s: the passes disagree\n", argv[i]); return 3; }
            FILE* o = fopen((std::string(argv[i]) + ".out").c_str(), "wb");
            if (!o || fwrite(bytes.data(), 1, bytes.size(), o) != bytes.size()) { fprintf(stderr, "%s: cannot write the output\n", argv[i]); return 2; }
            fclose(o);
        }
        printf("%s kind=%d read=%llu record=%llu bytes=%llu lines=%llu units=%llu longest=%llu mismatch=%llu\n", argv[i], kind,
               (unsigned long long)out[5], (unsigned long long)out[6], (unsigned long long)out[0], (unsigned long long)out[1],
               (unsigned long long)out[2], (unsigned long long)out[3], (unsigned long long)out[7]);
    }
    return 0;
}
#endif
