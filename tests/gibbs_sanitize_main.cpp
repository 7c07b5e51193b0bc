// stand-alone program over csrc/gibbsfmt.h and csrc/rng.h (through the harness's functions) for a build with
// -fsanitize=address,undefined: tests/test_chain_cpu.py compiles and runs it.  A small class table with an empty class, a singleton,
// a heavy class and a wide one, a few chains and rounds, and the chain in both forms; exits 0 when every sample sums to the reads.
#include "sampling_harness.cpp"

#include <cstdio>

int main() {
    const uint64_t M = 2400, C = 70;
    std::vector<uint32_t> rowptr(C + 1, 0), ids;
    std::vector<uint64_t> counts(C, 0);
    for (uint64_t c = 0; c < C; ++c) {
        const uint32_t k = c == 5 ? 0u : (c == 6 ? 1u : 2u + (uint32_t)(c % 4));
        for (uint32_t i = 0; i < k; ++i) ids.push_back((uint32_t)(c * 3 + i * 2));
        if (c == 40) ids.back() = 2399;                                        // spans more than kWideSpan ids: wide
        counts[c] = k == 0 ? 0 : (c == 9 ? 250000 : 100 + 37 * c);             // class 9 is heavy
        rowptr[c + 1] = (uint32_t)ids.size();
    }
    std::vector<uint8_t> kind(C, 0);
    kind[40] = 1; kind[9] = 2;
    std::vector<double> len(M), mass(M);
    uint64_t R = 0;
    for (uint64_t c = 0; c < C; ++c) R += counts[c];
    for (uint64_t t = 0; t < M; ++t) { len[t] = 0.5 + (double)(t % 977); mass[t] = (t % 5) ? 1.0 / (double)M : 0.0; }
    const uint32_t n_chains = 5, n_samples = 13;                               // the last round emits 3 of 5 chains
    std::vector<int32_t> out((size_t)n_samples * M);
    if (gibbs_serial(M, C, rowptr.data(), ids.data(), counts.data(), len.data(), mass.data(), R, n_chains, 7, n_samples, kind.data(), 2, out.data())) return 2;
    for (uint32_t s = 0; s < n_samples; ++s) {
        uint64_t sum = 0;
        for (uint64_t t = 0; t < M; ++t) sum += (uint64_t)out[(size_t)s * M + t];
        if (sum != R) { std::printf("sample %u sums to %llu, not %llu\n", s, (unsigned long long)sum, (unsigned long long)R); return 1; }
    }
    const double w[5] = {5.0, 1.0, 1e-3, 4.0, 2.0};
    std::vector<uint32_t> draws(200 * 5);
    for (int light = 0; light < 2; ++light)
        for (uint32_t last = 0; last < 5; ++last) {
            draw_chain(light, w, 5, light ? 1400u : 3000000u, last, 777 + last, 200, draws.data());
            for (int d = 0; d < 200; ++d) {
                uint64_t sum = 0;
                for (int i = 0; i < 5; ++i) sum += draws[d * 5 + i];
                if (sum != (light ? 1400u : 3000000u)) return 1;
            }
        }
    std::printf("sanitize ok\n");
    return 0;
}
