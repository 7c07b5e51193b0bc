// Host program for tests/test_gpu_genes.py: transcripts read from a column file (name, Length, the bits of EffectiveLength and
// estCount in hex, and the gene's name, tab separated), then aggregateEstimatesToGeneLevel (include/sfgpu_sailfish.hpp) with a
// transcript -> gene-name callable over that table.  The test compares the file with the Python device path's for the same columns.
//   genes_host_test <columns file> <num mapped> <out quant.genes.sf> [<unwritable path>]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>

#include "sfgpu_sailfish.hpp"

using namespace sailfish::gpu;

static double from_bits(const std::string& hex) {
    const uint64_t b = std::strtoull(hex.c_str(), nullptr, 16);
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s columns.tsv num_mapped out.genes.sf [unwritable]\n", argv[0]); return 2; }
    try {
        ReadExperiment exp;
        std::unordered_map<std::string, std::string> geneOf;
        std::ifstream cf(argv[1]);
        std::string line;
        while (std::getline(cf, line)) {
            std::istringstream ls(line);
            std::string name, len, eff, cnt, gene;
            std::getline(ls, name, '\t'); std::getline(ls, len, '\t'); std::getline(ls, eff, '\t'); std::getline(ls, cnt, '\t');
            std::getline(ls, gene, '\t');
            exp.transcripts().emplace_back(exp.transcripts().size(), name.c_str(), static_cast<uint32_t>(std::strtoul(len.c_str(), nullptr, 10)));
            exp.transcripts().back().EffectiveLength = from_bits(eff);
            exp.transcripts().back().setEstCount(from_bits(cnt));
            geneOf[name] = gene;
        }
        exp.numMappedFragmentsAtomic() += std::strtoull(argv[2], nullptr, 10);
        SailfishOpts sopt;
        auto geneName = [&](const std::string& t) { return geneOf.at(t); };
        aggregateEstimatesToGeneLevel(geneName, exp, sopt, argv[3]);
        std::printf("folded %llu rows\n", (unsigned long long)exp.transcripts().size());
        if (argc > 4) {
            try {
                aggregateEstimatesToGeneLevel(geneName, exp, sopt, argv[4]);
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
