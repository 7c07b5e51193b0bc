"""The %g formatter of the device quant.sf writer (sailfish_amd/csrc/gfmt.h, used by quant_write.hip) compiled as plain C++ with
g++ and compared with snprintf("%g") -- random bit patterns, the window the 128-bit path covers, column-shaped values, every
exactly representable tie with both neighbours, every power of ten -- and, for a sample of every set, with Python's "%g", which
is what writer.fmt_g prints.  A NaN is expected as "nan" whatever its sign (glibc prints "-nan" for a set sign bit).  No GPU."""
import os
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HARNESS = r"""
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gfmt.h"

using namespace sfgpu;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next64() {            // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static double unit() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }      // [0, 1)

static long long failures = 0, checked = 0, n_slow = 0, seen = 0;
static FILE* sample = nullptr;
static long long sample_every = 1;

static void check(double x) {
    uint64_t bits;
    memcpy(&bits, &x, 8);
    char want[64];
    if (std::isnan(x)) std::strcpy(want, "nan");
    else std::snprintf(want, sizeof(want), "%g", x);
    bool slow = false;
    const uint32_t r = gfmt_decode(x, &slow);
    if (slow) ++n_slow;
    char buf[32];
    memset(buf, 0, sizeof(buf));
    int puts = 0, bad = 0;
    const int len = gfmt_len(r);
    const int ret = gfmt_put(r, [&](int i, char ch) {
        ++puts;
        if (i < 0 || i >= len || len > kGfmtMaxLen || buf[len - 1 - i]) ++bad; else buf[len - 1 - i] = ch;
    });
    ++checked;
    if (bad || ret != len || puts != len || len > kGfmtMaxLen || len != (int)std::strlen(want) || std::memcmp(buf, want, (size_t)len) != 0) {
        if (failures++ < 20) std::printf("FAIL bits=%016" PRIx64 " want=%s got=%s len=%d puts=%d bad=%d\n", bits, want, buf, len, puts, bad);
    }
    if (sample && (seen++ % sample_every) == 0) std::fprintf(sample, "%016" PRIx64 " %s\n", bits, buf);
}

static void end_set(const char* name) {
    std::printf("set %s checked %lld failures %lld slow %lld\n", name, checked, failures, n_slow);
    checked = failures = n_slow = 0;
}

static void with_neighbours(double f) {
    check(f); check(std::nextafter(f, 0.0)); check(std::nextafter(f, INFINITY));
    check(-f);
}

int main(int argc, char** argv) {
    const long long n = argc > 1 ? std::atoll(argv[1]) : 1000000;       // random bit patterns; the other sets scale with it
    if (argc > 2) sample = std::fopen(argv[2], "w");

    sample_every = 61;
    for (long long i = 0; i < n; ++i) {
        const uint64_t b = next64();
        double x;
        memcpy(&x, &b, 8);
        check(x);
    }
    end_set("random_bits");

    for (long long i = 0; i < n; ++i) {
        double x = std::pow(10.0, -16.0 + 54.0 * unit());
        if (x < 1e-16) x = 1e-16;
        if (x > 1e38) x = 1e38;
        check((i & 7) == 0 ? -x : x);
    }
    end_set("window");

    for (long long i = 0; i < n / 4; ++i) {
        const double u = unit();
        double t = u * u; t *= t; t *= t; t *= 1e6;                      // u^8 1e6
        if (t < 1e-13) t = 0.0;
        check(t);
        check((double)(next64() % 400000001ull));                        // integers up to 4e8
        check((double)(1 + next64() % 100000) - unit());                 // lengths minus a fraction
        check((double)(next64() % 400000001ull) * unit());
    }
    end_set("columns");

    // exactly representable ties (d + 1/2) 10^j = (2 d + 1) 5^j 2^(j - 1), with both neighbours
    sample_every = 7;
    long long ties = 0;
    for (int j = -12; j <= 16; ++j) {
        uint64_t p5 = 1;
        for (int i = 0; i < (j < 0 ? -j : j); ++i) p5 *= 5;
        for (int it = 0; it < 4000; ++it) {
            uint64_t odd = 2 * (100000 + next64() % 900000) + 1;         // 2 d + 1
            uint64_t N;
            if (j >= 0) {
                const uint64_t lim = ((1ull << 53) - 1) / p5;            // (2 d + 1) 5^j < 2^53
                if (lim < 200001) break;
                if (odd > lim) odd = 200001 + 2 * (next64() % ((lim - 200001) / 2 + 1));
                N = odd * p5;
            } else {
                if (p5 > 1999999) break;
                uint64_t k = odd / p5;                                   // an odd multiple of 5^-j in [200001, 1999999]
                if ((k & 1) == 0) ++k;
                if (k * p5 < 200001) k += 2;
                if (k * p5 > 1999999) { if (k < 2) continue; k -= 2; }
                if (k * p5 < 200001 || k * p5 > 1999999) continue;
                N = k;
            }
            with_neighbours(std::ldexp((double)N, j - 1));
            ++ties;
        }
    }
    std::printf("ties %lld\n", ties);
    end_set("ties");

    sample_every = 1;
    for (int k = -320; k <= 308; ++k) {
        char s[32];
        std::snprintf(s, sizeof(s), "1e%d", k);
        const double p = std::strtod(s, nullptr);
        check(p); check(std::nextafter(p, 0.0)); check(-p);
        if (k < 308) { std::snprintf(s, sizeof(s), "9.999995e%d", k); with_neighbours(std::strtod(s, nullptr)); }
    }
    const double edges[] = {0.0001, 9.9999949999e-05, 9.9999995e-05, 99999.95, 999999.5, 999999.4999999999, 1e5, 1e6, 0.0, -0.0, 5e-324,
                            DBL_MIN, DBL_MAX, INFINITY, -INFINITY, 1e22, 1e23, 1.0, 0.5, 123456.5, 1234565.0, 0.1, 100.0, 1e-5, 0.00012345650000000001,
                            1.3877787807814457e-17, 1.7014118346046923e38, 3.4028236692093846e38};
    for (double x : edges) with_neighbours(x);
    const uint64_t nans[] = {0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff0000000000001ull, 0xffffffffffffffffull};
    for (uint64_t b : nans) { double x; memcpy(&x, &b, 8); check(x); }
    end_set("edges");
    if (sample) std::fclose(sample);
    return 0;
}
"""


def _sets(stdout):
    out = {}
    for line in stdout.splitlines():
        w = line.split()
        if w and w[0] == "set":
            out[w[1]] = dict(checked=int(w[3]), failures=int(w[5]), slow=int(w[7]))
        elif w and w[0] == "ties":
            out["n_ties"] = int(w[1])
    return out


def test_gfmt_matches_snprintf_and_python(tmp_path):
    src = tmp_path / "gfmt_harness.cpp"
    src.write_text(HARNESS)
    exe = tmp_path / "gfmt_harness"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "sailfish_amd", "csrc"),
                           str(src), "-o", str(exe)])
    sample = tmp_path / "sample.txt"
    r = subprocess.run([str(exe), "4200000", str(sample)], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    s = _sets(r.stdout)
    assert set(s) == {"random_bits", "window", "columns", "ties", "edges", "n_ties"}, r.stdout
    for name in ("random_bits", "window", "columns", "ties", "edges"):
        assert s[name]["failures"] == 0, r.stdout
    assert s["random_bits"]["checked"] >= 4_000_000 and s["window"]["checked"] >= 4_000_000 and s["columns"]["checked"] >= 1_000_000
    assert s["n_ties"] >= 40_000 and s["ties"]["checked"] == 4 * s["n_ties"]
    assert s["edges"]["checked"] >= 629 * 3 + 628 * 4
    # the claim the design rests on: the 128-bit path covers everything a quant.sf column holds; the slow path is exercised
    assert s["window"]["slow"] == 0 and s["columns"]["slow"] == 0, r.stdout
    assert s["random_bits"]["slow"] > 0 and s["edges"]["slow"] > 0, r.stdout
    # the sample against Python's "%g" (writer.fmt_g)
    n = 0
    with open(sample) as f:
        for line in f:
            bits, got = line.split()
            x = struct.unpack("<d", struct.pack("<Q", int(bits, 16)))[0]
            want = "nan" if x != x else "%g" % x
            assert got == want, (bits, got, want)
            n += 1
    assert n >= 200_000
