// Host program for tests/test_gpu_gmap.py: transcripts read from a column file (name, Length, the bits of EffectiveLength and
// estCount in hex, tab separated), the gene map read on the device by readTranscriptToGeneMap (include/sfgpu_sailfish.hpp), then
// the overload of aggregateEstimatesToGeneLevel that takes the map's handle.  The test compares the file with the Python one.
//   gmap_host_test <columns file> <num mapped> <gene map> <key> <out quant.genes.sf> [<block bytes>]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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
    if (argc < 6) { std::fprintf(stderr, "usage: %s columns.tsv num_mapped gene_map key out.genes.sf [block_bytes]\n", argv[0]); return 2; }
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
        const size_t block = argc > 6 ? std::strtoull(argv[6], nullptr, 10) : (size_t(32) << 20);
        auto tgm = readTranscriptToGeneMap(argv[3], argv[4], block);
        aggregateEstimatesToGeneLevel(*tgm, exp, sopt, argv[5]);
        std::printf("mapped %llu transcripts to %llu genes, folded %llu rows\n", (unsigned long long)tgm->numTranscripts(),
                    (unsigned long long)tgm->numGenes(), (unsigned long long)exp.transcripts().size());
        try {
            readTranscriptToGeneMap(std::string(argv[3]) + ".absent", argv[4]);
            std::printf("absent map accepted\n");
            return 1;
        } catch (const std::runtime_error& e) {
            std::printf("refused: %s\n", e.what());
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
