// Host program for tests/test_gpu_eqwrite.py: a table built through the adaptor (addGroup from reads, insertGroup with large
// counts), writeEquivCounts (include/sfgpu_sailfish.hpp) to a file, loadEquivClasses of that file into a second experiment,
// and the two finished tables compared.  The test compares the file with Python's bytes.
//   eqwrite_host_test <names file> <out eq_classes.txt> [<unwritable path>]
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "sfgpu_sailfish.hpp"

using namespace sailfish::gpu;

struct Table {
    std::vector<uint32_t> rowptr, ids;
    std::vector<uint64_t> counts, hashes;
};

static Table table_of(EquivalenceClassBuilder& eq) {
    const uint64_t C = eq.numClasses(), nnz = eq.numNonzeros();
    Table t;
    t.rowptr.resize(C + 1); t.ids.resize(nnz ? nnz : 1); t.counts.resize(C ? C : 1); t.hashes.resize(C ? C : 1);
    check(sfgpu_eq_export_host(eq.handle(), t.rowptr.data(), t.ids.data(), t.counts.data(), t.hashes.data()), "sfgpu_eq_export_host");
    return t;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s names.txt out_eq_classes.txt [unwritable]\n", argv[0]); return 2; }
    try {
        ReadExperiment exp, back;
        std::ifstream nf(argv[1]);
        std::string name;
        while (std::getline(nf, name)) {
            exp.transcripts().emplace_back(exp.transcripts().size(), name.c_str(), 1000u);
            back.transcripts().emplace_back(back.transcripts().size(), name.c_str(), 1000u);
        }
        const uint32_t M = static_cast<uint32_t>(exp.transcripts().size());
        if (M < 16) { std::fprintf(stderr, "need >= 16 names\n"); return 2; }
        auto& eq = exp.equivalenceClassBuilder();
        eq.start();
        std::vector<double> w;
        uint64_t x = 88172645463325252ull;                        // xorshift64
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
        for (int r = 0; r < 200000; ++r) {
            const uint32_t k = 1 + static_cast<uint32_t>(rnd() % 6), base = static_cast<uint32_t>(rnd() % 3000);
            std::vector<uint32_t> lab(k);
            for (uint32_t i = 0; i < k; ++i) lab[i] = (base * 7 + i * 13) % M;
            eq.addGroup(TranscriptGroup(lab), w);
        }
        std::vector<uint32_t> wide(250);
        for (uint32_t i = 0; i < 250; ++i) wide[i] = (i * 31 + 5) % M;
        eq.insertGroup(TranscriptGroup(wide), 4000000000u);
        eq.insertGroup(TranscriptGroup(std::vector<uint32_t>{M - 1}), 999999999u);
        eq.finish();
        writeEquivCounts(argv[2], exp);

        auto& eq2 = back.equivalenceClassBuilder();
        eq2.start();
        loadEquivClasses(argv[2], back);
        eq2.finish();
        const Table a = table_of(eq), b = table_of(eq2);
        if (eq.numClasses() != eq2.numClasses() || a.rowptr != b.rowptr || a.ids != b.ids || a.counts != b.counts || a.hashes != b.hashes) {
            std::printf("tables differ\n");
            return 1;
        }
        std::printf("round trip ok: %llu classes, %llu ids, %llu reads\n", (unsigned long long)eq.numClasses(),
                    (unsigned long long)eq.numNonzeros(), (unsigned long long)eq.totalReads());
        if (argc > 3) {
            try {
                writeEquivCounts(argv[3], exp);
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
