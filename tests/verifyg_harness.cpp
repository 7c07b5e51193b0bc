// verifyg_harness.cpp -- csrc/verifygfmt.h alone, as plain C++ (g++ -Wall -Wextra -Werror): a job's banded edit distance in plain loops
// (vg_job_serial) and as a group of lanes runs it (vg_band_group), and the whole pass run serially.  tests/test_verifyg_cpu.py compares
// them with hits.verify_hits_gapped_host.  Built with -DVERIFYG_HARNESS_MAIN (and -fsanitize=address,undefined) it is a stand-alone
// program: it reads cases with their expected results from a file (tests/verifyg_corpus.py: blob) and runs both forms over them; every
// text is copied to a block of its own size first (vf_each_job), so a byte read outside a mate or a transcript is a sanitizer
// report.
#include "verifygfmt.h"

#include <cstdio>
#include <cstring>

using namespace sfgpu;

extern "C" {

// lanes = 0: the plain loops; else as a group of vg_width(k) lanes, stopping early above max_edits (-> ~0)
uint64_t vgh_job(const char* r, uint64_t len, int fwd, const char* t, uint64_t tlen, int64_t pos, uint32_t k, int lanes, uint64_t max_edits) {
    return lanes ? vg_band_group(r, len, fwd != 0, t, tlen, pos, k, vg_width(k), max_edits, nullptr, nullptr) : vg_job_serial(r, len, fwd != 0, t, tlen, pos, k);
}

// the whole pass; -> the number of survivors (the outputs have room for the input's records), or -(1 + the lowest record with tid >= M)
int64_t vgh_verify(const char* tseq, const uint64_t* tseq_off, const uint32_t* tlen, uint64_t M, const char* seq1, const uint64_t* off1, const char* seq2,
                   const uint64_t* off2, uint32_t n_reads, const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t permille, int keep_best, uint32_t k, int lanes,
                   sfgpu_hit* out_hits, uint32_t* out_off, sfgpu_hit_gscore* out_scores, sfgpu_verify_gstats* stats) {
    std::vector<sfgpu_hit> h; std::vector<uint32_t> o; std::vector<sfgpu_hit_gscore> s;
    const uint64_t bad = vg_serial_verify(tseq, tseq_off, tlen, M, seq1, off1, seq2, off2, n_reads, hits, hit_off, permille, keep_best != 0, k, lanes != 0, &h, &o, &s, stats);
    if (bad) return -(int64_t)bad;
    if (!h.empty()) { memcpy(out_hits, h.data(), h.size() * sizeof(sfgpu_hit)); memcpy(out_scores, s.data(), s.size() * sizeof(sfgpu_hit_gscore)); }
    memcpy(out_off, o.data(), o.size() * 4);
    return (int64_t)h.size();
}

}

#ifdef VERIFYG_HARNESS_MAIN
#include "hit_harness.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t n_cases = 0, hd[11];
    while (fread(hd, 8, 11, f) == 11) {
        const uint64_t n_out = hd[9];
        HarnessBatch b; std::vector<uint64_t> want_stats; std::vector<uint32_t> want_off;
        std::vector<sfgpu_hit> want_hits; std::vector<sfgpu_hit_gscore> want_scores;
        if (!b.read(f, hd, 8) || !take(f, &want_hits, n_out) || !take(f, &want_off, b.n_reads + 1) || !take(f, &want_scores, n_out) ||
            !take(f, &want_stats, 8)) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)n_cases); return 2; }
        for (int lanes = 0; lanes < 2; ++lanes) {
            std::vector<sfgpu_hit> h; std::vector<uint32_t> o; std::vector<sfgpu_hit_gscore> s; sfgpu_verify_gstats st;
            const uint64_t bad = vg_serial_verify(b.ts.data(), b.toff.data(), b.tl.data(), b.M, b.s1.data(), b.o1.data(), b.paired ? b.s2.data() : nullptr, b.paired ? b.o2.data() : nullptr,
                                                  (uint32_t)b.n_reads, b.hits.data(), b.hoff.data(), (uint32_t)hd[6], hd[7] != 0, (uint32_t)hd[10], lanes != 0, &h, &o, &s, &st);
            const uint64_t got_stats[8] = {st.records_in, st.records_out, st.reads_in, st.reads_out, st.failed_identity, st.dropped_not_best, st.sum_edits, st.rescued};
            const bool ok = !bad && h.size() == n_out && o == want_off && (n_out == 0 || (!memcmp(h.data(), want_hits.data(), n_out * sizeof(sfgpu_hit)) &&
                            !memcmp(s.data(), want_scores.data(), n_out * sizeof(sfgpu_hit_gscore)))) && !memcmp(got_stats, want_stats.data(), sizeof got_stats);
            if (!ok) { fprintf(stderr, "case %llu (%s): differs from the statement\n", (unsigned long long)n_cases, lanes ? "lanes" : "serial"); return 1; }
        }
        ++n_cases;
    }
    fclose(f);
    printf("verifyg harness ok: %llu cases\n", (unsigned long long)n_cases);
    return 0;
}
#endif
