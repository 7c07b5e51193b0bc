// genes_harness.cpp -- the two host/device headers of the gene-level path compiled as plain C++ (tests/test_genes_cpu.py, and
// tests/test_gpu_genes.py for the raw-double fold):
//   genes_harness value N [sample]   gfmt_value(gfmt_decode(x)) against strtod(snprintf("%g", x)) by bit pattern (any NaN for a NaN)
//                                    over the value families of test_gfmt_cpu.py and N quant-like values
//   genes_harness fold TABLE [printed]   genefold.h run serially: TABLE holds one row per line, "gene length eff tpm num_reads" with
//                                    the doubles as 16 hex digits; genes come out in first-appearance order, "gene len eff tpm nr"
//                                    in hex.  With `printed` every double goes through gfmt_decode -> gfmt_value first.
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "genefold.h"
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

static uint64_t bits_of(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
static double of_bits(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }

static long long failures = 0, checked = 0, n_slow = 0, n_cross = 0, seen = 0;

static void check(double x) {
    char tok[64];
    std::snprintf(tok, sizeof(tok), "%g", x);
    const double want = std::strtod(tok, nullptr);
    bool dslow = false, vslow = false;
    const uint32_t r = gfmt_decode(x, &dslow);
    const double got = gfmt_value(r, &vslow);
    if (vslow) ++n_slow;
    ++checked;
    const bool ok = std::isnan(want) ? std::isnan(got) : bits_of(got) == bits_of(want);
    if (!ok && failures++ < 20)
        std::printf("FAIL x=%016" PRIx64 " token=%s want=%016" PRIx64 " got=%016" PRIx64 " slow=%d\n", bits_of(x), tok, bits_of(want), bits_of(got), (int)vslow);
    // the slow half is exact for every record: where the fast half answered, the two agree (a sample: it is slow)
    if (!vslow && (seen++ % 64) == 0) {
        const double s = gfmt_value_slow(r);
        ++n_cross;
        const bool same = std::isnan(got) ? std::isnan(s) : bits_of(s) == bits_of(got);
        if (!same && failures++ < 20) std::printf("FAIL slow-vs-fast x=%016" PRIx64 " fast=%016" PRIx64 " slow=%016" PRIx64 "\n", bits_of(x), bits_of(got), bits_of(s));
    }
}

static void end_set(const char* name) {
    std::printf("set %s checked %lld failures %lld slow %lld cross %lld\n", name, checked, failures, n_slow, n_cross);
    checked = failures = n_slow = n_cross = 0;
}

static void with_neighbours(double f) {
    check(f); check(std::nextafter(f, 0.0)); check(std::nextafter(f, INFINITY));
    check(-f);
}

static int run_value(long long n) {
    for (long long i = 0; i < n / 4; ++i) check(of_bits(next64()));
    end_set("random_bits");

    // quant-like: tokens between 1e-16 and 1e9
    for (long long i = 0; i < n / 4; ++i) {
        const double u = unit();
        double t = u * u; t *= t; t *= t; t *= 1e6;                      // u^8 1e6
        if (t < 1e-13) t = 0.0;
        check(t);
        check((double)(next64() % 400000001ull));                        // integers up to 4e8
        check((double)(1 + next64() % 100000) - unit());                 // lengths minus a fraction
        check((double)(next64() % 400000001ull) * unit());
        double w = std::pow(10.0, -16.0 + 25.0 * unit());                // the whole span, log-uniform
        if (w < 1e-16) w = 1e-16;
        if (w >= 9.999995e8) w = 9.99999e8;
        check(w);
    }
    end_set("columns");

    // exactly representable ties (d + 1/2) 10^j = (2 d + 1) 5^j 2^(j - 1), with both neighbours
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

    for (int k = -320; k <= 308; ++k) {
        char s[32];
        std::snprintf(s, sizeof(s), "1e%d", k);
        const double p = std::strtod(s, nullptr);
        check(p); check(std::nextafter(p, 0.0)); check(-p);
        if (k < 308) { std::snprintf(s, sizeof(s), "9.999995e%d", k); with_neighbours(std::strtod(s, nullptr)); }
        for (int it = 0; it < 40; ++it) {                                // six random digits in every decade
            std::snprintf(s, sizeof(s), "%u.%05ue%d", (unsigned)(1 + next64() % 9), (unsigned)(next64() % 100000), k);
            const double v = std::strtod(s, nullptr);
            if (std::isfinite(v)) check(v);
        }
    }
    end_set("decades");

    for (uint64_t m = 1; m < 4096; ++m) check(of_bits(m));               // the smallest denormals, one by one
    for (int i = 0; i < 200000; ++i) check(of_bits(next64() >> 12));     // denormals
    for (int i = 0; i < 4096; ++i) check(of_bits((1ull << 52) - 2048 + i));      // across the denormal / normal border
    end_set("denormals");

    const double edges[] = {0.0001, 9.9999949999e-05, 9.9999995e-05, 99999.95, 999999.5, 999999.4999999999, 1e5, 1e6, 0.0, -0.0, 5e-324,
                            DBL_MIN, DBL_MAX, INFINITY, -INFINITY, 1e22, 1e23, 1.0, 0.5, 123456.5, 1234565.0, 0.1, 100.0, 1e-5, 0.00012345650000000001,
                            1.3877787807814457e-17, 1.7014118346046923e38, 3.4028236692093846e38, 7.41098e-324, 2.22507e-308, 2.22508e-308, 1.79769e308};
    for (double x : edges) with_neighbours(x);
    const uint64_t nans[] = {0x7ff8000000000000ull, 0xfff8000000000000ull, 0x7ff0000000000001ull, 0xffffffffffffffffull};
    for (uint64_t b : nans) check(of_bits(b));
    end_set("edges");
    return 0;
}

static int run_fold(const char* path, bool printed) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<uint64_t> order;                                         // gene ids by first appearance
    std::map<uint64_t, std::vector<GeneRow>> rows;
    uint64_t gene, length, e, t, c;
    while (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &gene, &length, &e, &t, &c) == 5) {
        GeneRow r;
        r.length = (double)length; r.eff = of_bits(e); r.tpm = of_bits(t); r.num_reads = of_bits(c);
        if (printed) {
            bool slow;
            r.eff = gfmt_value(gfmt_decode(r.eff, &slow), &slow);
            r.tpm = gfmt_value(gfmt_decode(r.tpm, &slow), &slow);
            r.num_reads = gfmt_value(gfmt_decode(r.num_reads, &slow), &slow);
        }
        if (!rows.count(gene)) order.push_back(gene);
        rows[gene].push_back(r);
    }
    std::fclose(f);
    for (uint64_t g : order) {
        const std::vector<GeneRow>& v = rows[g];
        const GeneSums s = gene_fold(v.size(), [&](uint64_t i) { return v[i]; });
        std::printf("%" PRIu64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", g, bits_of(s.length), bits_of(s.eff), bits_of(s.tpm),
                    bits_of(s.num_reads));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && std::strcmp(argv[1], "value") == 0) return run_value(std::atoll(argv[2]));
    if (argc >= 3 && std::strcmp(argv[1], "fold") == 0) return run_fold(argv[2], argc > 3 && std::strcmp(argv[3], "printed") == 0);
    std::fprintf(stderr, "usage: genes_harness value N | fold TABLE [printed]\n");
    return 2;
}
