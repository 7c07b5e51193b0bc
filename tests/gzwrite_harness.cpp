// Host harness for tests/test_gzwrite_cpu.py and tests/test_gpu_gzwrite.py: sailfish_amd/csrc/gzfmt.h compiled as plain C++
// (nothing but libstdc++ is linked).  Python's zlib judges what it writes.
//   gzwrite_harness crc <file> <seed>            CRC-32 of the file three ways: bytewise, in random slices (empty ones included)
//                                                 combined by crc32_combine, and in 64-byte slices weighted by x^(8 x bytes behind)
//   gzwrite_harness huff <file>                  lines "max_bits n f_0 .. f_{n-1}" -> lines "lens l_0 .." and "codes c_0 .." (bit-reversed)
//   gzwrite_harness enc <in> <out> [w_1 w_2 ..]  the serial encoder: one gzip member, the payload written in pieces of w_i bytes (the rest
//                                                 in one piece); also checks that the per-slice parse of the kernel gives the greedy tokens.
//                                                 Prints "blocks B stored S bytes_in N bytes_out M"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "gzfmt.h"

using namespace sfgpu;

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static uint64_t rng_state;
static uint64_t next64() {            // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static uint32_t table[256];

static uint32_t crc_of(const uint8_t* p, uint64_t n) {
    return crc32_slice(0u, table, [&](uint32_t i) { return p[i]; }, (uint32_t)n);
}

static int cmd_crc(const char* path, uint64_t seed) {
    const std::vector<uint8_t> d = slurp(path);
    const uint64_t n = d.size();
    const uint32_t whole = crc_of(d.data(), n);
    rng_state = seed;
    uint32_t sliced = 0;
    uint64_t at = 0;
    int extra = 3;                     // a few empty slices behind the end as well
    while (at < n || extra-- > 0) {
        uint64_t len = (next64() & 7) == 0 ? 0 : next64() % (n - at + 1);
        if ((next64() & 1) && len > 100) len %= 100;
        sliced = crc32_combine(sliced, crc_of(d.data() + at, len), len);
        at += len;
    }
    uint32_t lanes = 0;
    for (uint64_t c0 = 0; c0 < n; c0 += 64) {
        const uint64_t len = n - c0 < 64 ? n - c0 : 64;
        lanes ^= crc32_mulmod(crc32_xpow8(n - c0 - len), crc_of(d.data() + c0, len));
    }
    std::printf("%08x %08x %08x\n", whole, sliced, lanes);
    return 0;
}

static int cmd_huff(const char* path) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        int max_bits, n;
        is >> max_bits >> n;
        std::vector<uint32_t> freq(n), node_freq(2 * n), count(kGzMaxBits + 1);
        for (auto& v : freq) is >> v;
        std::vector<uint8_t> lens(n);
        std::vector<uint16_t> order(n), parent(2 * n);
        huff_lengths_serial(freq.data(), n, max_bits, lens.data(), order.data(), parent.data(), node_freq.data(), count.data());
        std::printf("lens");
        for (int s = 0; s < n; ++s) std::printf(" %d", (int)lens[s]);
        std::printf("\ncodes");
        for (int s = 0; s < n; ++s) std::printf(" %u", huff_code_rev(lens.data(), n, s));
        std::printf("\n");
    }
    return 0;
}

struct Tok { uint32_t pos, len; };

// the parse as the kernel runs it: the mask words, the last clear bit before every 64-byte slice, one gz_chunk_tokens per slice
static std::vector<Tok> lane_tokens(const uint8_t* in, uint32_t n) {
    std::vector<uint64_t> eq((n + 63) / 64 + 8, 0);
    for (uint32_t i = 1; i < n; ++i) if (in[i] == in[i - 1]) eq[i >> 6] |= 1ull << (i & 63);
    std::vector<Tok> out;
    int32_t z = -1;
    for (uint32_t c0 = 0; c0 < n; c0 += 64) {
        gz_chunk_tokens([&](uint32_t w) { return eq[w]; }, c0, c0 + 64, n, z, [&](uint32_t p, uint32_t l) { out.push_back({p, l}); });
        const uint64_t clear = ~eq[c0 >> 6];
        if (clear) z = (int32_t)(c0 + 63 - (uint32_t)gz_clz64(clear));
    }
    return out;
}

static int cmd_enc(int argc, char** argv) {
    const std::vector<uint8_t> d = slurp(argv[2]);
    std::vector<uint64_t> writes;
    uint64_t used = 0;
    for (int a = 4; a < argc; ++a) {
        uint64_t w = std::strtoull(argv[a], nullptr, 10);
        if (w > d.size() - used) w = d.size() - used;
        writes.push_back(w); used += w;
    }
    if (used < d.size() || writes.empty()) writes.push_back(d.size() - used);
    std::vector<uint8_t> out(kGzHeaderBytes);
    gz_header(out.data());
    std::vector<uint8_t> blk(gz_stored_bytes(kGzBlockBytes) + 8);
    uint32_t crc = 0;
    uint64_t total = 0, at = 0, n_blocks = 0, n_stored = 0;
    for (uint64_t w : writes) {
        for (uint64_t b = 0; b < w; b += kGzBlockBytes) {
            const uint32_t n = w - b < kGzBlockBytes ? (uint32_t)(w - b) : kGzBlockBytes;
            const uint8_t* in = d.data() + at + b;
            std::vector<Tok> greedy;
            gz_greedy_tokens(in, n, [&](uint32_t p, uint32_t l) { greedy.push_back({p, l}); });
            const std::vector<Tok> lanes = lane_tokens(in, n);
            bool same = greedy.size() == lanes.size();
            for (size_t i = 0; same && i < greedy.size(); ++i) same = greedy[i].pos == lanes[i].pos && greedy[i].len == lanes[i].len;
            if (!same) { std::fprintf(stderr, "the per-slice parse differs from the greedy parse in the block at %" PRIu64 "\n", at + b); return 1; }
            int stored = 0;
            const uint32_t m = gz_encode_block_serial(in, n, blk.data(), &stored);
            if (stored < 0) { std::fprintf(stderr, "the coded form left its buffer in the block at %" PRIu64 "\n", at + b); return 1; }
            out.insert(out.end(), blk.begin(), blk.begin() + m);
            ++n_blocks; n_stored += (uint64_t)stored;
        }
        crc = crc32_combine(crc, crc_of(d.data() + at, w), w);
        at += w; total += w;
    }
    uint8_t tail[kGzFinalBlockBytes + kGzTrailerBytes];
    gz_trailer(crc, total, tail);
    out.insert(out.end(), tail, tail + sizeof(tail));
    std::ofstream o(argv[3], std::ios::binary);
    o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)out.size());
    std::printf("blocks %" PRIu64 " stored %" PRIu64 " bytes_in %" PRIu64 " bytes_out %zu\n", n_blocks, n_stored, total, out.size());
    return o ? 0 : 2;
}

int main(int argc, char** argv) {
    for (uint32_t i = 0; i < 256; ++i) table[i] = crc32_table_entry(i);
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "crc" && argc == 4) return cmd_crc(argv[2], std::strtoull(argv[3], nullptr, 10));
    if (cmd == "huff" && argc == 3) return cmd_huff(argv[2]);
    if (cmd == "enc" && argc >= 4) return cmd_enc(argc, argv);
    std::fprintf(stderr, "usage: %s crc <file> <seed> | huff <file> | enc <in> <out> [write sizes]\n", argv[0]);
    return 2;
}
