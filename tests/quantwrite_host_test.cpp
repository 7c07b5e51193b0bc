// Host program for tests/test_gpu_quantwrite.py: transcripts read from a column file (name, Length, and the bits of
// EffectiveLength and estCount in hex, tab separated), then writeAbundances (include/sfgpu_sailfish.hpp) with and without
// noEffectiveLengthCorrection.  The test compares the files with Python's bytes for the same columns.
//   quantwrite_host_test <columns file> <num mapped> <out quant.sf> <out quant.sf, no length correction> [<unwritable path>]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "sfgpu_sailfish.hpp"

using namespace sailfish::gpu;

static double from_bits(const std::string& hex) {
    const uint64_t b = std::strtoull(hex.c_str(), nullptr, 16);
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: %s columns.tsv num_mapped out.sf out_nolen.sf [unwritable]\n", argv[0]); return 2; }
    try {
        ReadExperiment exp;
        std::ifstream cf(argv[1]);
        std::string line;
        while (std::getline(cf, line)) {
            std::istringstream ls(line);
            std::string name, len, eff, cnt;
            std::getline(ls, name, '\t'); std::getline(ls, len, '\t'); std::getline(ls, eff, '\t'); std::getline(ls, cnt, '\t');
            exp.transcripts().emplace_back(exp.transcripts().size(), name.c_str(), static_cast<uint32_t>(std::strtoul(len.c_str(), nullptr, 10)));
            exp.transcripts().back().EffectiveLength = from_bits(eff);
            exp.transcripts().back().setEstCount(from_bits(cnt));
        }
        exp.numMappedFragmentsAtomic() += std::strtoull(argv[2], nullptr, 10);
        SailfishOpts sopt;
        writeAbundances(argv[3], exp, sopt);
        sopt.noEffectiveLengthCorrection = true;
        writeAbundances(argv[4], exp, sopt);
        std::printf("wrote %llu rows\n", (unsigned long long)exp.transcripts().size());
        if (argc > 5) {
            try {
                writeAbundances(argv[5], exp, sopt);
                std::printf("unwritable path accepted\n");
                return 1;
            } catch (const std::runtime_error& e) {
                std::printf("refused: %s\n", e.what());
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
