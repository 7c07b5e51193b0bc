// Host program for tests/test_gpu_eqfile.py: loadEquivClasses (include/sfgpu_sailfish.hpp) folds a class file into the
// adaptor's builder; the finished table is written as raw arrays for the test to compare with Python's.
//   eqfile_host_test <class file> <names file> <out.bin> [<malformed class file>]
// out.bin: u64 C, u64 nnz, u64 mapped, u64 observed, rowptr u32[C + 1], ids u32[nnz], counts u64[C], hashes u64[C]
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "sfgpu_sailfish.hpp"

using namespace sailfish::gpu;

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s eq_classes.txt names.txt out.bin [bad.txt]\n", argv[0]); return 2; }
    try {
        ReadExperiment exp;
        std::ifstream nf(argv[2]);
        std::string name;
        while (std::getline(nf, name)) exp.transcripts().emplace_back(exp.transcripts().size(), name.c_str(), 1000u);
        auto& eq = exp.equivalenceClassBuilder();
        eq.start();
        loadEquivClasses(argv[1], exp);
        eq.finish();
        const uint64_t C = eq.numClasses(), nnz = eq.numNonzeros();
        std::vector<uint32_t> rowptr(C + 1), ids(nnz ? nnz : 1);
        std::vector<uint64_t> counts(C ? C : 1), hashes(C ? C : 1);
        check(sfgpu_eq_export_host(eq.handle(), rowptr.data(), ids.data(), counts.data(), hashes.data()), "sfgpu_eq_export_host");
        std::ofstream out(argv[3], std::ios::binary);
        const uint64_t head[4] = {C, nnz, exp.numMappedFragments(), exp.numObservedFragmentsAtomic().load()};
        out.write(reinterpret_cast<const char*>(head), sizeof(head));
        out.write(reinterpret_cast<const char*>(rowptr.data()), (C + 1) * 4);
        out.write(reinterpret_cast<const char*>(ids.data()), nnz * 4);
        out.write(reinterpret_cast<const char*>(counts.data()), C * 8);
        out.write(reinterpret_cast<const char*>(hashes.data()), C * 8);
        std::printf("loaded %llu classes, %llu ids, %llu mapped\n", (unsigned long long)C, (unsigned long long)nnz,
                    (unsigned long long)exp.numMappedFragments());
        if (argc > 4) {
            eq.start();
            try {
                loadEquivClasses(argv[4], exp);
                std::printf("malformed file accepted\n");
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
