// Host harness for tests/test_samcollate_cpu.py: sailfish_amd/csrc/samcfmt.h compiled as plain C++ (g++ -Wall -Wextra -Werror;
// nothing but libstdc++ is linked) -- the serial collated reader (SamcSerial) behind a small C interface, fed whole or in blocks
// with the caller-side carry that sfgpu_sam_collect_* expect.  With -DSAMC_HARNESS_MAIN the same source is a stand-alone program
// (built with -fsanitize=address,undefined by the test): `prog paired|single names_file file...` reads every file whole and in
// blocks of 1, 7, 64 and 4096 bytes, requires the same records each time and prints one line per file.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define SAMCFMT_SERIAL
#include "samcfmt.h"

using namespace sfgpu;

namespace {

// the whole text in blocks of block_bytes (0 = one block): the unconsumed tail stays in front of the next block, and a call that
// consumed nothing is presented twice as much the next time (what readfile's carriers do with "present more"); then finish()
void feed(SamcSerial& m, const unsigned char* text, uint64_t n, uint64_t block_bytes) {
    if (block_bytes == 0) {
        m.add(text, n, true);
    } else {
        std::vector<unsigned char> buf;
        uint64_t at = 0, want = block_bytes;
        do {
            const uint64_t room = want > buf.size() ? want - buf.size() : block_bytes;
            const uint64_t take = n - at < room ? n - at : room;
            buf.insert(buf.end(), text + at, text + at + take);
            at += take;
            const uint64_t used = m.add(buf.data(), buf.size(), at == n);
            buf.erase(buf.begin(), buf.begin() + (long)used);
            want = used ? block_bytes : 2 * buf.size();
        } while (at < n && !m.bad);
    }
    if (!m.bad) m.finish();
}

// names: back to back, '\n' behind each
std::vector<std::string> split_names(const char* names, uint64_t n) {
    std::vector<std::string> out;
    uint64_t a = 0;
    for (uint64_t p = 0; p < n; ++p)
        if (names[p] == '\n') { out.emplace_back(names + a, p - a); a = p + 1; }
    return out;
}

}  // namespace

extern "C" void* samc_harness_new(int paired, const char* names, uint64_t names_bytes) {
    return new SamcSerial(paired != 0, split_names(names, names_bytes));
}
extern "C" void samc_harness_free(void* h) { delete static_cast<SamcSerial*>(h); }

// out: [0] bad kind, [1] bad line (0-based), [2] reads, [3] hits, [4] lines, [5] header lines, [6] pairs
extern "C" void samc_harness_read(void* h, const unsigned char* text, uint64_t n, uint64_t block_bytes, uint64_t* out) {
    SamcSerial& m = *static_cast<SamcSerial*>(h);
    feed(m, text, n, block_bytes);
    out[0] = m.bad; out[1] = m.bad_line; out[2] = m.offsets.size() - 1; out[3] = m.hits.size(); out[4] = m.n_lines; out[5] = m.n_header;
    out[6] = m.n_pairs;
}

extern "C" void samc_harness_export(void* h, sfgpu_hit* hits, uint32_t* offsets) {
    SamcSerial& m = *static_cast<SamcSerial*>(h);
    if (!m.hits.empty()) memcpy(hits, m.hits.data(), m.hits.size() * sizeof(sfgpu_hit));
    memcpy(offsets, m.offsets.data(), m.offsets.size() * sizeof(uint32_t));
}

#ifdef SAMC_HARNESS_MAIN
static bool slurp(const char* path, std::vector<unsigned char>& text) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "%s: cannot open\n", path); return false; }
    unsigned char tmp[4096];
    for (size_t got; (got = fread(tmp, 1, sizeof tmp, f)) > 0;) text.insert(text.end(), tmp, tmp + got);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s paired|single names_file file...\n", argv[0]); return 2; }
    const bool paired = strcmp(argv[1], "paired") == 0;
    std::vector<unsigned char> nm;
    if (!slurp(argv[2], nm)) return 2;
    const std::vector<std::string> names = split_names(reinterpret_cast<const char*>(nm.data()), nm.size());
    for (int a = 3; a < argc; ++a) {
        std::vector<unsigned char> text;
        if (!slurp(argv[a], text)) return 2;
        SamcSerial whole(paired, names);
        feed(whole, text.data(), text.size(), 0);
        for (uint64_t block : {1ull, 7ull, 64ull, 4096ull}) {
            SamcSerial m(paired, names);
            feed(m, text.data(), text.size(), block);
            bool same = m.bad == whole.bad && m.bad_line == whole.bad_line;
            if (same && !m.bad)
                same = m.offsets == whole.offsets && m.hits.size() == whole.hits.size() && m.n_lines == whole.n_lines &&
                       m.n_header == whole.n_header && m.n_pairs == whole.n_pairs &&
                       (m.hits.empty() || memcmp(m.hits.data(), whole.hits.data(), m.hits.size() * sizeof(sfgpu_hit)) == 0);
            if (!same) {
                fprintf(stderr, "%s: blocks of %llu bytes give another result\n", argv[a], (unsigned long long)block);
                return 1;
            }
        }
        printf("%s bad=%u line=%llu reads=%zu hits=%zu lines=%llu header=%llu pairs=%llu\n", argv[a], whole.bad,
               (unsigned long long)whole.bad_line, whole.offsets.size() - 1, whole.hits.size(), (unsigned long long)whole.n_lines,
               (unsigned long long)whole.n_header, (unsigned long long)whole.n_pairs);
    }
    return 0;
}
#endif
