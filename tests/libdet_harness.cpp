// libdet_harness.cpp -- csrc/libdetfmt.h alone, for tests/test_libdet_cpu.py: as a shared library (the functions below through ctypes)
// and, with -DLIBDET_HARNESS_MAIN, as a stand-alone program that reads tests/libdet_corpus.py's batch with the statement's counters
// and runs the serial pass over it, every array in a heap block of exactly its size (built with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "libdetfmt.h"

using namespace sfgpu;

static_assert(sizeof(sfgpu_libdet_stats) == (6 + 3 * SFGPU_LIBDET_KINDS) * sizeof(uint64_t), "the stats are 45 counters back to back");

static sfgpu_libdet_opts make_opts(uint32_t max_read_occs, int paired, int dovetail, int has_expected, int type, int orientation, int strandedness) {
    sfgpu_libdet_opts o;
    o.max_read_occs = max_read_occs; o.paired_library = paired; o.can_dovetail = dovetail; o.has_expected = has_expected;
    o.expected = sfgpu_libfmt{(uint8_t)type, (uint8_t)orientation, (uint8_t)strandedness, 0};
    return o;
}

extern "C" {

// reads [first, first + n) of the batch: adds to stats[45], takes the votes off *remaining
void lh_library_kinds(const sfgpu_hit* hits, const uint32_t* off, uint32_t first, uint32_t n, uint32_t max_read_occs, int paired, int dovetail, int has_expected,
                      int type, int orientation, int strandedness, int64_t* remaining, uint64_t* stats) {
    const sfgpu_libdet_opts o = make_opts(max_read_occs, paired, dovetail, has_expected, type, orientation, strandedness);
    sfgpu_libdet_stats st;
    memcpy(&st, stats, sizeof st);
    ld_serial(hits, off + first, n, &o, remaining, &st);
    memcpy(stats, &st, sizeof st);
}

uint32_t lh_kind(const sfgpu_hit* h, int dovetail) { return ld_kind(*h, dovetail != 0); }

uint32_t lh_compat_mask(int type, int orientation, int strandedness) {
    return ld_compat_mask(sfgpu_libfmt{(uint8_t)type, (uint8_t)orientation, (uint8_t)strandedness, 0});
}

uint32_t lh_vote(uint32_t mask, int paired) { return ld_vote(mask, paired != 0); }

int32_t lh_decide(const uint64_t* votes_kind, int paired, uint32_t permille, uint64_t min_votes) { return ld_decide(votes_kind, paired != 0, permille, min_votes); }

}  // extern "C"

#ifdef LIBDET_HARNESS_MAIN
// the file: n_reads, n_rec, n_cases (uint64 each); the records; the offsets; per case 9 uint64 -- max_read_occs, paired, dovetail,
// has_expected, type, orientation, strandedness, the vote budget, reads per call -- then the 45 expected counters and the expected rest of the budget
template <typename T> static T* exact(const unsigned char*& at, size_t n) {
    T* p = (T*)malloc(n > 0 ? n * sizeof(T) : 1);
    memcpy(p, at, n * sizeof(T));
    at += n * sizeof(T);
    return p;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> buf;
    unsigned char chunk[1 << 16];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
    fclose(f);
    const unsigned char* at = buf.data();
    uint64_t* head = exact<uint64_t>(at, 3);
    const uint64_t n_reads = head[0], n_rec = head[1], n_cases = head[2];
    sfgpu_hit* hits = exact<sfgpu_hit>(at, n_rec);
    uint32_t* off = exact<uint32_t>(at, n_reads + 1);
    int bad = 0;
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint64_t* cs = exact<uint64_t>(at, 9);
        uint64_t* want = exact<uint64_t>(at, 46);
        const sfgpu_libdet_opts o = make_opts((uint32_t)cs[0], (int)cs[1], (int)cs[2], (int)cs[3], (int)cs[4], (int)cs[5], (int)cs[6]);
        int64_t remaining = (int64_t)cs[7];
        sfgpu_libdet_stats st;
        memset(&st, 0, sizeof st);
        for (uint64_t a = 0; a < n_reads; a += cs[8]) {
            const uint64_t n = n_reads - a < cs[8] ? n_reads - a : cs[8];
            ld_serial(hits, off + a, (uint32_t)n, &o, &remaining, &st);
        }
        if (memcmp(&st, want, sizeof st) != 0 || (uint64_t)remaining != want[45]) { printf("case %llu differs\n", (unsigned long long)c); bad = 1; }
        free(cs); free(want);
    }
    free(off); free(hits); free(head);
    if (bad) return 1;
    printf("libdet harness ok: %llu reads, %llu records, %llu cases\n", (unsigned long long)n_reads, (unsigned long long)n_rec, (unsigned long long)n_cases);
    return 0;
}
#endif
