// Host program for tests/test_gpu_gzwrite.py: writeBootstraps (include/sfgpu_sailfish.hpp) on a sample matrix made on the host and
// uploaded; the test inflates the file with Python's gzip and compares it with the raw matrix written next to it.
//   gzwrite_host_test <out bootstraps.gz> <out raw payload> [<unwritable path>]
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "sfgpu_sailfish.hpp"

using namespace sailfish::gpu;

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s out.gz out.raw [unwritable]\n", argv[0]); return 2; }
    try {
        const uint64_t n_samples = 9, M = 12345;
        std::vector<int32_t> h(n_samples * M);
        uint64_t x = 88172645463325252ull;                        // xorshift64
        for (auto& v : h) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            v = (x & 7) < 5 ? 0 : static_cast<int32_t>((x >> 8) % 300);
        }
        DeviceBuf<int32_t> d(h);
        writeBootstraps(argv[1], d.get(), n_samples, M, sizeof(int32_t));
        std::ofstream raw(argv[2], std::ios::binary);
        raw.write(reinterpret_cast<const char*>(h.data()), static_cast<std::streamsize>(h.size() * sizeof(int32_t)));
        std::printf("wrote %llu samples of %llu\n", (unsigned long long)n_samples, (unsigned long long)M);
        if (argc > 3) {
            try {
                writeBootstraps(argv[3], d.get(), n_samples, M, sizeof(int32_t));
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
