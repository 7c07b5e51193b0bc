// Host harness for tests/test_gmap_cpu.py: sailfish_amd/csrc/gtffmt.h compiled as plain C++ (g++ -Wall -Wextra -Werror; nothing but
// libstdc++ is linked) -- the serial gene map (GtSerialMap) behind a small C interface, fed whole or in blocks with the caller-side
// carry that sfgpu_gmap_add_text_* expect.  With -DGMAP_HARNESS_MAIN the same source is a stand-alone program (built with
// -fsanitize=address,undefined by the test): `prog gtf|tsv key file...` maps every file whole and in blocks of 1, 7 and 64 bytes,
// requires the same map each time and prints one line per file.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define GTFFMT_SERIAL_MAP
#include "gtffmt.h"

using namespace sfgpu;

namespace {

// the whole text in blocks of block_bytes (0 = one block): the unconsumed tail stays in front of the next block
void feed(GtSerialMap& m, const unsigned char* text, uint64_t n, uint64_t block_bytes) {
    if (block_bytes == 0) { m.add(text, n, true); return; }
    std::vector<unsigned char> buf;
    uint64_t at = 0;
    do {
        const uint64_t take = n - at < block_bytes ? n - at : block_bytes;
        buf.insert(buf.end(), text + at, text + at + take);
        at += take;
        const uint64_t used = m.add(buf.data(), buf.size(), at == n);
        buf.erase(buf.begin(), buf.begin() + (long)used);
    } while (at < n);
}

}  // namespace

extern "C" void* gmap_harness_new(int gtf, const char* key, uint32_t key_len) { return new GtSerialMap(gtf, std::string(key, key_len)); }
extern "C" void gmap_harness_free(void* h) { delete static_cast<GtSerialMap*>(h); }

// out: [0] host-only flags, [1] transcripts, [2] genes, [3] bytes of the transcript names, [4] of the gene names, [5] lines, [6] records
extern "C" void gmap_harness_map(void* h, const unsigned char* text, uint64_t n, uint64_t block_bytes, uint64_t* out) {
    GtSerialMap& m = *static_cast<GtSerialMap*>(h);
    feed(m, text, n, block_bytes);
    if (!m.flags) m.finish();
    out[0] = m.flags; out[1] = m.transcript_names.size(); out[2] = m.gene_names.size(); out[3] = out[4] = 0;
    for (auto& s : m.transcript_names) out[3] += s.size();
    for (auto& s : m.gene_names) out[4] += s.size();
    out[5] = m.n_lines; out[6] = m.n_records;
}

extern "C" void gmap_harness_export(void* h, char* tnames, uint64_t* tname_off, uint32_t* t2g, char* gnames, uint64_t* gname_off) {
    GtSerialMap& m = *static_cast<GtSerialMap*>(h);
    uint64_t at = 0;
    for (size_t i = 0; i < m.transcript_names.size(); ++i) {
        tname_off[i] = at; t2g[i] = m.t2g[i];
        memcpy(tnames + at, m.transcript_names[i].data(), m.transcript_names[i].size());
        at += m.transcript_names[i].size();
    }
    tname_off[m.transcript_names.size()] = at;
    at = 0;
    for (size_t i = 0; i < m.gene_names.size(); ++i) {
        gname_off[i] = at;
        memcpy(gnames + at, m.gene_names[i].data(), m.gene_names[i].size());
        at += m.gene_names[i].size();
    }
    gname_off[m.gene_names.size()] = at;
}

#ifdef GMAP_HARNESS_MAIN
int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s gtf|tsv key file...\n", argv[0]); return 2; }
    const int gtf = strcmp(argv[1], "gtf") == 0;
    for (int a = 3; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<unsigned char> text;
        unsigned char tmp[4096];
        for (size_t got; (got = fread(tmp, 1, sizeof tmp, f)) > 0;) text.insert(text.end(), tmp, tmp + got);
        fclose(f);
        GtSerialMap whole(gtf, argv[2]);
        feed(whole, text.data(), text.size(), 0);
        if (!whole.flags) whole.finish();
        for (uint64_t block : {1ull, 7ull, 64ull}) {
            GtSerialMap m(gtf, argv[2]);
            feed(m, text.data(), text.size(), block);
            if (!m.flags) m.finish();
            if (m.flags && whole.flags) continue;            // flagged either way: no map, and the counts stop where the flag rose
            if (m.flags != whole.flags || m.transcript_names != whole.transcript_names || m.gene_names != whole.gene_names ||
                m.t2g != whole.t2g || m.n_lines != whole.n_lines || m.n_records != whole.n_records) {
                fprintf(stderr, "%s: blocks of %llu bytes give another map\n", argv[a], (unsigned long long)block);
                return 1;
            }
        }
        printf("%s flags=%u transcripts=%zu genes=%zu lines=%llu records=%llu\n", argv[a], whole.flags, whole.transcript_names.size(),
               whole.gene_names.size(), (unsigned long long)whole.n_lines, (unsigned long long)whole.n_records);
    }
    return 0;
}
#endif
