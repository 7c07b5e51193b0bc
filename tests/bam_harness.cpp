// Host harness for tests/test_bam_cpu.py: sailfish_amd/csrc/bamfmt.h compiled as plain C++ (g++ -Wall -Wextra -Werror; nothing but
// libstdc++ is linked).  Two things behind a small C interface: the serial reader (BamSerial: a plain walk of the record chain), fed
// whole or in blocks with the caller-side carry that sfgpu_bam_parse_* expect; and the tile functions the kernels of bamtext.hip
// run, driven here the way those kernels drive them (exit table per tile by pointer doubling, supertiles, tile entries, the
// record starts of every tile), whose record starts must be those of the plain walk.  With -DBAM_HARNESS_MAIN the same source is a
// stand-alone program (built with -fsanitize=address,undefined by the test): `prog paired|single names_file file...` reads every
// file whole and in blocks of 1, 7, 64 and 4096 bytes, requires the same records each time, compares the tile functions at three
// tile sizes with the plain walk, and prints one line per file.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#define BAMFMT_SERIAL
#include "bamfmt.h"

using namespace sfgpu;

namespace {

// the whole stream in blocks of block_bytes (0 = one block): the unconsumed tail stays in front of the next block, and a call that
// consumed nothing is presented twice as much the next time (what readfile's carriers do with "present more")
void feed(BamSerial& m, const unsigned char* text, uint64_t n, uint64_t block_bytes) {
    if (block_bytes == 0) { m.add(text, n, true); return; }
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

// names: back to back, '\n' behind each
std::vector<std::string> split_names(const char* names, uint64_t n) {
    std::vector<std::string> out;
    uint64_t a = 0;
    for (uint64_t p = 0; p < n; ++p)
        if (names[p] == '\n') { out.emplace_back(names + a, p - a); a = p + 1; }
    return out;
}

// the record starts of text[skip, n) and the chain value behind them, by the plain walk
uint32_t plain_walk(const unsigned char* text, uint32_t skip, uint32_t n, std::vector<uint32_t>* starts) {
    auto get = [text](uint32_t p) { return text[p]; };
    uint32_t p = skip;
    while (p < n) {
        const uint32_t v = bam_next(get, p, n);
        if (bam_ended(v)) return v;
        starts->push_back(p);
        p = v;
    }
    return p;
}

// the same by the tile functions, staged as bamtext.hip stages them: tiles of T bytes, supertiles of S tiles
template <uint32_t T>
uint32_t tiled_walk(const unsigned char* text, uint32_t skip, uint32_t n, uint32_t S, std::vector<uint32_t>* starts) {
    auto get = [text](uint32_t p) { return text[p]; };
    const uint32_t n_tiles = (n + T - 1) / T, n_super = (n_tiles + S - 1) / S;
    std::vector<uint32_t> exit_tab((size_t)n_tiles * T), a(T), b(T);
    for (uint32_t t = 0; t < n_tiles; ++t) {              // the tile pass
        const uint32_t base = t * T;
        for (uint32_t i = 0; i < T; ++i) a[i] = bam_tile_nxt<T>(get, base, i, n);
        for (uint32_t r = 0; r < bam_tile_rounds<T>(); ++r) {
            for (uint32_t i = 0; i < T; ++i) b[i] = bam_tile_double<T>(a.data(), base, i);
            a.swap(b);
        }
        for (uint32_t i = 0; i < T; ++i) exit_tab[(size_t)base + i] = a[i];
    }
    auto exit_at = [&](uint32_t p) { return exit_tab[p]; };
    std::vector<uint32_t> super_exit((size_t)n_super * T), super_entry(n_super), tile_entry(n_tiles);
    auto send_of = [&](uint32_t s) { const uint64_t e = ((uint64_t)s + 1) * S * T; return e < n ? (uint32_t)e : n; };
    for (uint32_t s = 0; s < n_super; ++s)                // the link pass: per entry offset into the first tile
        for (uint32_t o = 0; o < T; ++o)
            if ((uint64_t)s * S * T + o < n) super_exit[(size_t)s * T + o] = bam_follow(exit_at, s * S * T + o, send_of(s), n);
    uint32_t v = skip;
    for (uint32_t s = 0; s < n_super; ++s) {              // one walk over the supertiles
        const uint32_t sbase = s * S * T;
        super_entry[s] = v;
        if (bam_ended(v) || v >= send_of(s)) continue;
        v = v - sbase < T ? super_exit[(size_t)s * T + (v - sbase)] : bam_follow(exit_at, v, send_of(s), n);
    }
    for (uint32_t s = 0; s < n_super; ++s) {              // every tile its entry
        uint32_t w = super_entry[s];
        for (uint32_t t = s * S; t < (s + 1) * S && t < n_tiles; ++t) {
            const bool in = !bam_ended(w) && w >= t * T && w - t * T < T && w < n;
            tile_entry[t] = in ? w : 0xffffffffu;
            if (in) w = exit_at(w);
        }
    }
    std::vector<uint32_t> list(bam_tile_records<T>());
    for (uint32_t t = 0; t < n_tiles; ++t) {              // enumerate
        uint32_t leave;
        const uint32_t c = bam_tile_starts<T>(get, t * T, tile_entry[t], n, list.data(), &leave);
        starts->insert(starts->end(), list.begin(), list.begin() + c);
    }
    return v;
}

// 0 when the tile functions give the plain walk's starts and end at every tile size, else the tile size that does not
uint32_t chain_mismatch(const unsigned char* text, uint32_t skip, uint32_t n) {
    std::vector<uint32_t> want, got;
    const uint32_t end = skip <= n ? plain_walk(text, skip, n, &want) : skip;
    if (skip > n) return 0;
    got.clear(); if (tiled_walk<64>(text, skip, n, 4, &got) != end || got != want) return 64;
    got.clear(); if (tiled_walk<256>(text, skip, n, 3, &got) != end || got != want) return 256;
    got.clear(); if (tiled_walk<4096>(text, skip, n, 64, &got) != end || got != want) return 4096;
    return 0;
}

struct Harness {
    BamSerial m;
    Harness(bool paired, const std::vector<std::string>& names, const std::vector<std::string>& refs, uint64_t header_bytes)
        : m(paired, names, refs, header_bytes) {}
};

}  // namespace

// the header is read from `text` (the whole stream); null when it is not there
extern "C" void* bam_harness_new(int paired, const char* names, uint64_t names_bytes, const unsigned char* text, uint64_t n) {
    std::vector<std::string> refs;
    uint64_t header_bytes = 0;
    if (!bam_header(text, n, &refs, &header_bytes)) return nullptr;
    return new Harness(paired != 0, split_names(names, names_bytes), refs, header_bytes);
}
extern "C" void bam_harness_free(void* h) { delete static_cast<Harness*>(h); }

// out: [0] bad kind, [1] bad record (0-based), [2] reads, [3] hits, [4] records, [5] pairs, [6] header_bytes
extern "C" void bam_harness_read(void* h, const unsigned char* text, uint64_t n, uint64_t block_bytes, uint64_t* out) {
    BamSerial& m = static_cast<Harness*>(h)->m;
    feed(m, text, n, block_bytes);
    out[0] = m.bad; out[1] = m.bad_line; out[2] = m.offsets.size() - 1; out[3] = m.hits.size(); out[4] = m.n_lines; out[5] = m.n_pairs;
    out[6] = m.header_bytes;
}

extern "C" void bam_harness_export(void* h, sfgpu_hit* hits, uint32_t* offsets) {
    BamSerial& m = static_cast<Harness*>(h)->m;
    if (!m.hits.empty()) memcpy(hits, m.hits.data(), m.hits.size() * sizeof(sfgpu_hit));
    memcpy(offsets, m.offsets.data(), m.offsets.size() * sizeof(uint32_t));
}

// the tile functions against the plain walk over text[skip, n): 0, or the tile size that differs
extern "C" uint32_t bam_harness_chain(const unsigned char* text, uint64_t skip, uint64_t n) { return chain_mismatch(text, (uint32_t)skip, (uint32_t)n); }

#ifdef BAM_HARNESS_MAIN
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
        std::vector<std::string> refs;
        uint64_t header_bytes = 0;
        if (!bam_header(text.data(), text.size(), &refs, &header_bytes)) { fprintf(stderr, "%s: no BAM header\n", argv[a]); return 1; }
        BamSerial whole(paired, names, refs, header_bytes);
        feed(whole, text.data(), text.size(), 0);
        for (uint64_t block : {1ull, 7ull, 64ull, 4096ull}) {
            BamSerial m(paired, names, refs, header_bytes);
            feed(m, text.data(), text.size(), block);
            bool same = m.bad == whole.bad && m.bad_line == whole.bad_line;
            if (same && !m.bad)
                same = m.offsets == whole.offsets && m.hits.size() == whole.hits.size() && m.n_lines == whole.n_lines && m.n_pairs == whole.n_pairs &&
                       (m.hits.empty() || memcmp(m.hits.data(), whole.hits.data(), m.hits.size() * sizeof(sfgpu_hit)) == 0);
            if (!same) {
                fprintf(stderr, "%s: blocks of %llu bytes give another result\n", argv[a], (unsigned long long)block);
                return 1;
            }
        }
        if (const uint32_t T = chain_mismatch(text.data(), (uint32_t)header_bytes, (uint32_t)text.size())) {
            fprintf(stderr, "%s: tiles of %u bytes give other record starts than the plain walk\n", argv[a], T);
            return 1;
        }
        printf("%s bad=%u record=%llu reads=%zu hits=%zu records=%llu pairs=%llu\n", argv[a], whole.bad, (unsigned long long)whole.bad_line,
               whole.offsets.size() - 1, whole.hits.size(), (unsigned long long)whole.n_lines, (unsigned long long)whole.n_pairs);
    }
    return 0;
}
#endif
