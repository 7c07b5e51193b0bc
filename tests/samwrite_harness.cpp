// samwrite_harness.cpp -- csrc/samwfmt.h alone, as plain C++: the serial writer (samw_serial) behind a C interface for
// tests/test_samwrite_cpu.py, which compares its bytes with samfile._sam_text, and -- with -DSAMW_HARNESS_MAIN -- a stand-alone
// program over case files for the sanitizer run.  The per-unit functions the kernels call (samw_unit_len, samw_check) are
// cross-checked against the serial pass on the way.
#include "samwfmt.h"

#include <cstdio>
#include <string>
#include <vector>

using namespace sfgpu;

namespace {

// out[0 .. 8): n_bytes, n_lines, n_units, max_unit_bytes, error_kind, error_read, error_record, 1 when the per-unit sizes disagree
int size_of(const SamwArgs& a, uint64_t* out) {
    SamwSerial res;
    const int kind = samw_serial(a, nullptr, &res);
    uint64_t sum = 0, longest = 0, units = 0;
    auto unit = [&](uint64_t len) {
        sum += len; ++units;
        if (len > longest) longest = len;
    };
    for (uint64_t r = 0; !kind && r < a.n_reads; ++r) {
        const uint64_t h0 = a.hit_off[r], h1 = a.hit_off[r + 1];
        if (h0 == h1) unit(samw_unit_len(a, r, nullptr, 0));
        for (uint64_t h = h0; h < h1; ++h) unit(samw_unit_len(a, r, a.hits + h, h - h0));
    }
    out[0] = res.n_bytes; out[1] = res.n_lines; out[2] = res.n_units; out[3] = res.max_unit_bytes;
    out[4] = (uint64_t)kind; out[5] = res.error_read; out[6] = res.error_record;
    out[7] = !kind && (sum != res.n_bytes || longest != res.max_unit_bytes || units != res.n_units);
    return kind;
}

}  // namespace

extern "C" {

// the arrays of sfgpu_sam_write_text (host pointers); q_off == nullptr: default names, s1_off / s2_off == nullptr: '*'
int samw_harness_size(const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off,
                      uint32_t n_refs, const char* q, const uint64_t* q_off, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2,
                      const int64_t* s2_off, uint64_t read_index_base, uint64_t* out) {
    const SamwArgs a = {static_cast<const sfgpu_hit*>(hits), hit_off, n_reads, paired, ref, ref_off, n_refs, q, q_off, s1, s1_off,
                        paired ? s2 : nullptr, paired ? s2_off : nullptr, read_index_base};
    return size_of(a, out);
}

// the text into `text`, which has room for the n_bytes samw_harness_size gave; returns the error kind (nothing is written then)
int samw_harness_format(const void* hits, const uint32_t* hit_off, uint32_t n_reads, int paired, const char* ref, const uint64_t* ref_off,
                        uint32_t n_refs, const char* q, const uint64_t* q_off, const uint8_t* s1, const int64_t* s1_off, const uint8_t* s2,
                        const int64_t* s2_off, uint64_t read_index_base, char* text) {
    const SamwArgs a = {static_cast<const sfgpu_hit*>(hits), hit_off, n_reads, paired, ref, ref_off, n_refs, q, q_off, s1, s1_off,
                        paired ? s2 : nullptr, paired ? s2_off : nullptr, read_index_base};
    SamwSerial res;
    return samw_serial(a, text, &res);
}

}  // extern "C"

#ifdef SAMW_HARNESS_MAIN
// samwrite_harness_san CASE...: a case file is 12 uint64 (n_reads, n_hits, paired, n_refs, has names, has seq1, has seq2,
// read_index_base, bytes of the reference names, of the read names, of seq1, of seq2) and then the arrays in the order of the
// call (hits, hit offsets, reference names, their offsets, read names, offsets, seq1, offsets, seq2, offsets; absent ones left
// out).  Writes CASE.out (the text) and prints one line per case.
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
        uint64_t h[12];
        if (fread(h, 8, 12, f) != 12) { fprintf(stderr, "%s: short header\n", argv[i]); return 2; }
        std::vector<sfgpu_hit> hits;
        std::vector<uint32_t> hit_off;
        std::vector<char> ref, q;
        std::vector<uint64_t> ref_off, q_off;
        std::vector<uint8_t> s1, s2;
        std::vector<int64_t> s1_off, s2_off;
        bool ok = take(f, &hits, h[1]) && take(f, &hit_off, h[0] + 1) && take(f, &ref, h[8]) && take(f, &ref_off, h[3] + 1);
        if (h[4]) ok = ok && take(f, &q, h[9]) && take(f, &q_off, h[0] + 1);
        if (h[5]) ok = ok && take(f, &s1, h[10]) && take(f, &s1_off, h[0] + 1);
        if (h[6]) ok = ok && take(f, &s2, h[11]) && take(f, &s2_off, h[0] + 1);
        fclose(f);
        if (!ok) { fprintf(stderr, "%s: short file\n", argv[i]); return 2; }
        const SamwArgs a = {hits.data(), hit_off.data(), (uint32_t)h[0], (int)h[2], ref.data(), ref_off.data(), (uint32_t)h[3],
                            h[4] ? q.data() : nullptr, h[4] ? q_off.data() : nullptr, h[5] ? s1.data() : nullptr, h[5] ? s1_off.data() : nullptr,
                            h[6] ? s2.data() : nullptr, h[6] ? s2_off.data() : nullptr, h[7]};
        uint64_t out[8];
        const int kind = size_of(a, out);
        std::vector<char> text(kind ? 0 : out[0]);
        if (!kind) {
            SamwSerial res;
            if (samw_serial(a, text.data(), &res) || res.n_bytes != out[0]) { fprintf(stderr, "%s: the passes disagree\n", argv[i]); return 3; }
            FILE* o = fopen((std::string(argv[i]) + ".out").c_str(), "wb");
            if (!o || fwrite(text.data(), 1, text.size(), o) != text.size()) { fprintf(stderr, "%s: cannot write the text\n", argv[i]); return 2; }
            fclose(o);
        }
        printf("%s kind=%d read=%llu record=%llu bytes=%llu lines=%llu units=%llu longest=%llu mismatch=%llu\n", argv[i], kind,
               (unsigned long long)out[5], (unsigned long long)out[6], (unsigned long long)out[0], (unsigned long long)out[1],
               (unsigned long long)out[2], (unsigned long long)out[3], (unsigned long long)out[7]);
    }
    return 0;
}
#endif
