"""The decimal helpers of the device class-file writer (sailfish_amd/csrc/decfmt.h, used by eqtext_write.hip) compiled as plain
C++ with g++ and compared with snprintf("%u") / ("%llu"): digit counts, the multiply-high divisions, zero-padded fixed-width
digits and the formatted strings, over every digit boundary and a few million random values.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "decfmt.h"

using namespace sfgpu;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next64() {            // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static long long failures = 0;
static void fail(const char* what, unsigned long long v, const char* want, const std::string& got) {
    if (failures++ < 20) std::printf("FAIL %s v=%llu want=%s got=%s\n", what, v, want, got.c_str());
}

static std::string put_u32(uint32_t v) {
    char buf[32]; memset(buf, '?', sizeof(buf));
    const int n = dec_put_u32(v, [&](int i, char ch) { buf[31 - i] = ch; });
    return std::string(buf + 32 - n, n);
}
static std::string put_u64(uint64_t v) {
    char buf[32]; memset(buf, '?', sizeof(buf));
    const int n = dec_put_u64(v, [&](int i, char ch) { buf[31 - i] = ch; });
    return std::string(buf + 32 - n, n);
}

static void check_u32(uint32_t v) {
    char want[32];
    const int n = std::snprintf(want, sizeof(want), "%u", v);
    if (dec_len_u32(v) != n) fail("len32", v, want, std::to_string(dec_len_u32(v)));
    if (dec_len_u64(v) != n) fail("len64of32", v, want, std::to_string(dec_len_u64(v)));
    if (dec_div10(v) != v / 10u) fail("div10", v, want, std::to_string(dec_div10(v)));
    if (dec_div100(v) != v / 100u) fail("div100", v, want, std::to_string(dec_div100(v)));
    if (put_u32(v) != want) fail("put32", v, want, put_u32(v));
    if (put_u64(v) != want) fail("put64of32", v, want, put_u64(v));
    // fixed width: leading zeros
    char z[16], zw[16];
    memset(z, 0, sizeof(z));
    if (v < 1000000000u) {
        dec_put_fixed_u32(v, 9, 0, [&](int i, char ch) { z[8 - i] = ch; });
        std::snprintf(zw, sizeof(zw), "%09u", v);
        if (std::string(z) != zw) fail("fixed9", v, zw, z);
    }
}

static void check_u64(uint64_t v) {
    char want[32];
    const int n = std::snprintf(want, sizeof(want), "%llu", (unsigned long long)v);
    if (dec_len_u64(v) != n) fail("len64", v, want, std::to_string(dec_len_u64(v)));
    if (put_u64(v) != want) fail("put64", v, want, put_u64(v));
}

int main(int argc, char** argv) {
    const long long n_random = argc > 1 ? std::atoll(argv[1]) : 1000000;
    long long checked = 0;
    // every power of ten and its neighbours, powers of two and their neighbours, the ends of both ranges
    std::vector<uint64_t> edges = {0, 1, 2, 9, 10, 11, 99, 100, 101, 4294967294ull, 4294967295ull, 4294967296ull, 4294967297ull,
                                   18446744073709551614ull, 18446744073709551615ull};
    uint64_t p = 1;
    for (int e = 0; e < 20; ++e) {
        for (int64_t d = -2; d <= 2; ++d) edges.push_back(p + (uint64_t)d);
        for (uint64_t m = 2; m <= 9; ++m) if (e < 19 || m == 1) edges.push_back(p * m), edges.push_back(p * m - 1);
        if (e < 19) p *= 10;
    }
    for (int b = 1; b < 64; ++b) for (int64_t d = -1; d <= 1; ++d) edges.push_back((1ull << b) + (uint64_t)d);
    for (uint64_t v : edges) {
        check_u64(v); ++checked;
        if (v <= 0xffffffffull) check_u32((uint32_t)v);
    }
    // the divisions by multiply-high: every multiple of 10 / 100 and the value below it, sampled densely at the top of the range
    for (uint64_t v = 4294000000ull; v <= 4294967295ull; ++v) {
        if (dec_div10((uint32_t)v) != (uint32_t)v / 10u || dec_div100((uint32_t)v) != (uint32_t)v / 100u) fail("divtop", v, "", "");
    }
    for (long long i = 0; i < n_random; ++i) {
        const uint64_t r = next64();
        check_u32((uint32_t)r);                                  // uniform 32-bit
        check_u32((uint32_t)(r >> 32) >> (next64() & 31));       // every magnitude
        check_u64(r);                                            // uniform 64-bit
        check_u64(r >> (next64() & 63));                         // every magnitude
        checked += 4;
    }
    std::printf("checked %lld failures %lld\n", checked, failures);
    return failures ? 1 : 0;
}
"""


def test_decimal_helpers_match_snprintf(tmp_path):
    src = tmp_path / "decfmt_harness.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "decfmt_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "sailfish_amd", "csrc"),
                           str(src), "-o", str(exe)])
    r = subprocess.run([str(exe), "1000000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    checked, failures = (int(x) for x in r.stdout.split()[-3::2])
    assert failures == 0 and checked >= 4_000_000, r.stdout
