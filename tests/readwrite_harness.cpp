// readwrite_harness.cpp -- sailfish_amd/csrc/readwfmt.h run serially on the host (no HIP): the rules the kernels of
// readtext_write.hip apply, for tests/test_readwrite_cpu.py, which judges them by readfile.reads_text_host.
//   readw_harness_size    res[0 .. 5) = selected records, bytes, longest record, error kind, error record; res[5] = 1 when the sum
//                         of readw_record_len over the selected records is not what readw_serial counts
//   readw_harness_format  the text into `out` (room for exactly the bytes readw_harness_size reported); returns the error kind
// With -DREADW_HARNESS_MAIN the same source is a program: every argument is a case file (tests/test_readwrite_cpu.py writes them),
// read into buffers exactly as large as the contract says; it prints one line a file and writes the text to <file>.out.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "readwfmt.h"

using namespace sfgpu;

static ReadwArgs args_of(const uint8_t* bases, const int64_t* off, uint64_t n_reads, const uint8_t* qual, const uint8_t* names,
                         const uint64_t* name_off, uint64_t base, const uint8_t* select) {
    return ReadwArgs{bases, off, n_reads, qual, names, name_off, base, select};
}

extern "C" int readw_harness_size(const uint8_t* bases, const int64_t* off, uint64_t n_reads, const uint8_t* qual, const uint8_t* names,
                                  const uint64_t* name_off, uint64_t base, const uint8_t* select, uint64_t* res) {
    const ReadwArgs a = args_of(bases, off, n_reads, qual, names, name_off, base, select);
    const ReadwSerial s = readw_serial(a, nullptr);
    res[0] = s.n_selected; res[1] = s.n_bytes; res[2] = s.max_record_bytes; res[3] = (uint64_t)s.error_kind; res[4] = s.error_record; res[5] = 0;
    if (!s.error_kind) {
        uint64_t sum = 0, longest = 0;
        for (uint64_t r = 0; r < n_reads; ++r) {
            if (!readw_selected(a, r)) continue;
            const uint64_t len = readw_record_len(a, r);
            sum += len;
            if (len > longest) longest = len;
        }
        res[5] = sum != s.n_bytes || longest != s.max_record_bytes;
    }
    return s.error_kind;
}

extern "C" int readw_harness_format(const uint8_t* bases, const int64_t* off, uint64_t n_reads, const uint8_t* qual, const uint8_t* names,
                                    const uint64_t* name_off, uint64_t base, const uint8_t* select, uint8_t* out) {
    return readw_serial(args_of(bases, off, n_reads, qual, names, name_off, base, select), out).error_kind;
}

#ifdef READW_HARNESS_MAIN
// a case file: 7 uint64 (n_reads, qualities given, names given, selector given, index base, bytes of bases, bytes of names), then
// off[n_reads + 1], the bases, the qualities, name_off[n_reads + 1], the names, the selector -- each present only where given
template <typename T>
static T* slurp(FILE* f, uint64_t n) {
    T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));       // exactly n elements: the sanitizer sees the first byte behind them
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        uint64_t head[7];
        if (fread(head, 8, 7, f) != 7) { fprintf(stderr, "short case file\n"); return 2; }
        const uint64_t n = head[0];
        int64_t* off = slurp<int64_t>(f, n + 1);
        uint8_t* bases = slurp<uint8_t>(f, head[5]);
        uint8_t* qual = head[1] ? slurp<uint8_t>(f, head[5]) : nullptr;
        uint64_t* name_off = head[2] ? slurp<uint64_t>(f, n + 1) : nullptr;
        uint8_t* names = head[2] ? slurp<uint8_t>(f, head[6]) : nullptr;
        uint8_t* select = head[3] ? slurp<uint8_t>(f, n) : nullptr;
        fclose(f);
        uint64_t res[6];
        const int kind = readw_harness_size(bases, off, n, qual, names, name_off, head[4], select, res);
        if (kind) {
            printf("%s kind=%d record=%llu mismatch=%d\n", argv[i], kind, (unsigned long long)res[4], (int)res[5]);
        } else {
            uint8_t* out = static_cast<uint8_t*>(malloc(res[1] ? res[1] : 1));
            readw_harness_format(bases, off, n, qual, names, name_off, head[4], select, out);
            std::vector<char> path(strlen(argv[i]) + 5);
            snprintf(path.data(), path.size(), "%s.out", argv[i]);
            FILE* o = fopen(path.data(), "wb");
            if (!o || fwrite(out, 1, res[1], o) != res[1]) { fprintf(stderr, "cannot write %s\n", path.data()); return 2; }
            fclose(o);
            printf("%s kind=0 selected=%llu bytes=%llu longest=%llu mismatch=%d\n", argv[i], (unsigned long long)res[0], (unsigned long long)res[1],
                   (unsigned long long)res[2], (int)res[5]);
            free(out);
        }
        free(off); free(bases); free(qual); free(name_off); free(names); free(select);
    }
    return 0;
}
#endif
