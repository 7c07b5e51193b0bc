// Host harness for tests/test_readnames_cpu.py and tests/test_gpu_readnames.py: the name blob and the mate-name rule of
// sailfish_amd/csrc/readfmt.h compiled as plain C++ (g++ -shared; nothing but libstdc++ is linked) and run serially, with loops
// where readtext.hip has k_reads_emit, a scan, k_names_gather and k_names_match.  The records come from the serial parse of
// tests/readfile_harness.cpp, which this file includes.  One parse call = one sfgpu_reads_parse_host_n call without qualities:
// same return code and result struct, host arrays in place of device arrays (names: cap_names bytes, name_off: n + 2 entries).
// With -DREADNAMES_HARNESS_MAIN the same code is a program that runs case files (tests/test_readnames_cpu.py writes them).
#include "readfile_harness.cpp"

// -1: rf_blob_record disagrees with the back-to-back copy (a fault of the header, never expected)
extern "C" int readnames_harness_parse(const char* text, uint64_t n, int final, uint64_t max_reads, uint8_t* bases, uint64_t cap_bases,
                                       int64_t* off, uint64_t* span, uint8_t* names, uint64_t cap_names, uint64_t* name_off,
                                       uint64_t* n_name_bytes, sfgpu_reads_result* out) {
    if (n_name_bytes) *n_name_bytes = 0;
    if (names && ((reinterpret_cast<uintptr_t>(names) & 15u) || (cap_names & 15u) || !name_off)) {
        memset(out, 0, sizeof(*out));
        out->error_record = ~0ull; out->error_line = ~0ull;
        return SFGPU_ERR_INVALID;
    }
    std::vector<uint64_t> own_span(span ? 0 : 2 * n + 2);
    uint64_t* sp = span ? span : own_span.data();
    if (name_off) name_off[0] = 0;
    const int rc = readfile_harness_parse(text, n, final, max_reads, bases, cap_bases, off, sp, out);
    if (rc != SFGPU_OK || !names) return rc;
    const uint32_t R = (uint32_t)out->n_reads;
    std::vector<uint32_t> scan(R + 1, 0);                                  // the exclusive sum, in the 32 bits the device uses
    for (uint32_t r = 0; r < R; ++r) scan[r + 1] = scan[r] + (uint32_t)sp[2 * r + 1];
    const uint32_t total = scan[R];
    if (total > cap_names) {                                               // an error emits nothing
        const sfgpu_reads_result kept = *out;
        memset(out, 0, sizeof(*out));
        out->error_record = ~0ull; out->error_line = ~0ull;
        out->format = kept.format; out->n_lines = kept.n_lines;
        return SFGPU_ERR_RANGE;
    }
    for (uint32_t r = 0; r <= R; ++r) name_off[r] = scan[r];
    for (uint32_t r = 0; r < R; ++r) memcpy(names + scan[r], text + sp[2 * r], scan[r + 1] - scan[r]);
    for (uint32_t o = total; o < ((total + 15u) & ~15u); ++o) names[o] = 0;  // what the device may write behind the blob
    for (uint32_t o = 0; o < total; ++o) {                                 // the same bytes found the way the gather finds them
        const uint32_t r = rf_blob_record(R, o, [&](uint32_t i) { return scan[i]; });
        if (!(scan[r] <= o && o < scan[r + 1]) || names[o] != (uint8_t)text[sp[2 * r] + (o - scan[r])]) return -1;
    }
    if (n_name_bytes) *n_name_bytes = total;
    return SFGPU_OK;
}

extern "C" uint64_t readnames_harness_stem_len(const uint8_t* name, uint64_t len) {
    return rf_mate_stem_len([&](uint64_t p) { return name[p]; }, 0, len);
}

// the lowest read whose names disagree; UINT64_MAX: none
extern "C" uint64_t readnames_harness_match(const uint8_t* names1, const uint64_t* off1, const uint8_t* names2, const uint64_t* off2,
                                            uint64_t n_reads) {
    auto b1 = [&](uint64_t p) { return names1[p]; };
    auto b2 = [&](uint64_t p) { return names2[p]; };
    for (uint64_t r = 0; r < n_reads; ++r)
        if (!rf_mates_agree(b1, off1[r], off1[r + 1] - off1[r], b2, off2[r], off2[r + 1] - off2[r])) return r;
    return ~0ull;
}

#ifdef READNAMES_HARNESS_MAIN
// A case file is uint64 words, then bytes.  kind 0 (parse): [0, n, final, max_reads, cap_bases, cap_names] + text -> <file>.out =
// [rc, n_reads, n_bases, consumed, n_name_bytes] + name_off[0 .. n_reads] + the blob.  kind 1 (match): [1, n_reads, bytes1, bytes2]
// + off1 + off2 (n_reads + 1 words each) + blob 1 + blob 2 -> <file>.out = [first].  One line per file on stdout.
#include <cstdio>
#include <cstdlib>
#include <string>

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    uint8_t buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + got);
    fclose(f);
    return v;
}

static void dump(const std::string& path, const std::vector<uint64_t>& words, const uint8_t* bytes, size_t n_bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { perror(path.c_str()); exit(2); }
    fwrite(words.data(), 8, words.size(), f);
    if (n_bytes) fwrite(bytes, 1, n_bytes, f);
    fclose(f);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        const std::vector<uint8_t> file = slurp(argv[a]);
        uint64_t w[6] = {0, 0, 0, 0, 0, 0};
        if (file.size() < 32) { fprintf(stderr, "%s: short case file\n", argv[a]); return 2; }
        memcpy(w, file.data(), 8);
        const size_t head = w[0] == 0 ? 48 : 32;
        if (file.size() < head) { fprintf(stderr, "%s: short case file\n", argv[a]); return 2; }
        memcpy(w, file.data(), head);
        if (w[0] == 0) {
            const uint64_t n = w[1];
            if (file.size() != head + n) { fprintf(stderr, "%s: bad case file\n", argv[a]); return 2; }
            std::vector<char> text(file.begin() + head, file.end());               // exactly n bytes: a read behind them is caught
            std::vector<uint8_t> bases(n + 1);
            std::vector<int64_t> off(n + 2);
            std::vector<uint64_t> name_off(n + 2);
            uint8_t* names = static_cast<uint8_t*>(aligned_alloc(16, w[5] ? (w[5] + 15) & ~15ull : 16));   // cap_names bytes, no more
            uint64_t n_name = 0;
            sfgpu_reads_result res;
            const int rc = readnames_harness_parse(text.data(), n, (int)w[2], w[3], bases.data(), w[4], off.data(), nullptr, names, w[5],
                                                   name_off.data(), &n_name, &res);
            std::vector<uint64_t> words = {(uint64_t)(int64_t)rc, res.n_reads, res.n_bases, res.consumed, n_name};
            if (rc == SFGPU_OK) words.insert(words.end(), name_off.begin(), name_off.begin() + res.n_reads + 1);
            dump(std::string(argv[a]) + ".out", words, names, rc == SFGPU_OK ? n_name : 0);
            printf("%s rc=%d reads=%llu name_bytes=%llu\n", argv[a], rc, (unsigned long long)res.n_reads, (unsigned long long)n_name);
            free(names);
        } else {
            const uint64_t n = w[1], nb1 = w[2], nb2 = w[3];
            if (file.size() != head + 16 * (n + 1) + nb1 + nb2) { fprintf(stderr, "%s: bad case file\n", argv[a]); return 2; }
            std::vector<uint64_t> off1(n + 1), off2(n + 1);
            memcpy(off1.data(), file.data() + head, 8 * (n + 1));
            memcpy(off2.data(), file.data() + head + 8 * (n + 1), 8 * (n + 1));
            const uint8_t* p = file.data() + head + 16 * (n + 1);
            const std::vector<uint8_t> b1(p, p + nb1), b2(p + nb1, p + nb1 + nb2);
            const uint64_t first = readnames_harness_match(b1.data(), off1.data(), b2.data(), off2.data(), n);
            dump(std::string(argv[a]) + ".out", {first}, nullptr, 0);
            printf("%s first=%llu\n", argv[a], (unsigned long long)first);
        }
    }
    return 0;
}
#endif
