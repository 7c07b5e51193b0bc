// Host harness for tests/test_bgzw_cpu.py and tests/test_gpu_bgzw.py: sailfish_amd/csrc/bgzwfmt.h compiled as plain C++
// (nothing but libstdc++ is linked) and loaded with ctypes.  Python's zlib and gzip judge what it writes.
//   bgzw_harness_payload      kBgzwPayload
//   bgzw_harness_encode       the serial encoder's file for src[0 .. n) written in pieces of writes[i] bytes (the rest, if any, in one
//                             more piece): the members of every piece, then the EOF member.  Returns the file's bytes, -1 when `cap`
//                             is too small.  stats = members, stored members, matches, literals
//   bgzw_harness_tokens       the tokens of one member's parse as (position, length, distance) triples, length 1 = a literal
//   bgzw_harness_dist_symbol  distance -> symbol, extra bits, extra value
#include <cstdint>
#include <vector>

#include "bgzwfmt.h"

using namespace sfgpu;

extern "C" uint32_t bgzw_harness_payload() { return kBgzwPayload; }

extern "C" int64_t bgzw_harness_encode(const uint8_t* src, uint64_t n, const uint64_t* writes, uint32_t n_writes, uint8_t* dst, uint64_t cap,
                                       uint64_t* stats) {
    std::vector<uint64_t> pieces;
    uint64_t used = 0;
    for (uint32_t i = 0; i < n_writes; ++i) {
        const uint64_t w = writes[i] < n - used ? writes[i] : n - used;
        pieces.push_back(w); used += w;
    }
    if (used < n) pieces.push_back(n - used);
    std::vector<BgzwSerialWork> work(1);
    std::vector<uint8_t> member(kBgzwMaxMember + 8);
    for (int k = 0; k < 4; ++k) stats[k] = 0;
    uint64_t at = 0, out = 0;
    for (uint64_t w : pieces) {
        for (uint64_t b = 0; b < w; b += kBgzwPayload) {
            const uint32_t len = w - b < kBgzwPayload ? (uint32_t)(w - b) : kBgzwPayload;
            BgzwMemberInfo info;
            const uint32_t m = bgzw_encode_member_serial(src + at + b, len, member.data(), work.data(), &info, [](uint32_t, uint32_t, uint32_t) {});
            if (out + m > cap) return -1;
            for (uint32_t i = 0; i < m; ++i) dst[out + i] = member[i];
            out += m;
            stats[0] += 1; stats[1] += info.stored; stats[2] += info.n_matches; stats[3] += info.n_literals;
        }
        at += w;
    }
    if (out + kBgzwEofBytes > cap) return -1;
    bgzw_eof_member(dst + out);
    return (int64_t)(out + kBgzwEofBytes);
}

extern "C" uint32_t bgzw_harness_tokens(const uint8_t* src, uint32_t n, uint32_t* triples, uint32_t cap) {
    std::vector<BgzwSerialWork> work(1);
    std::vector<uint8_t> member(kBgzwMaxMember + 8);
    BgzwMemberInfo info;
    uint32_t k = 0;
    bgzw_encode_member_serial(src, n, member.data(), work.data(), &info, [&](uint32_t pos, uint32_t len, uint32_t dist) {
        if (k < cap) { triples[3 * k] = pos; triples[3 * k + 1] = len; triples[3 * k + 2] = dist; }
        ++k;
    });
    return k;
}

extern "C" int bgzw_harness_dist_symbol(uint32_t dist, int* eb, uint32_t* ev) { return bgzw_dist_symbol(dist, eb, ev); }
