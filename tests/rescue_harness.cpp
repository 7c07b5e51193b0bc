// rescue_harness.cpp -- csrc/rescuefmt.h alone, as plain C++ (g++ -Wall -Wextra -Werror): a job searched byte by byte and as the
// kernel's wavefront searches it (packed tiles, early stops, the tightening budget), and the whole pass run serially.
// tests/test_rescue_cpu.py compares them with hits.rescue_mates_host.  Built with -DRESCUE_HARNESS_MAIN (and
// -fsanitize=address,undefined) it is a stand-alone program: it reads cases with their expected results from a file
// (tests/rescue_corpus.py: blob) and runs both ways over them; every text is copied to a block of its own size first
// (rs_serial_rescue), so a byte read outside a mate or a transcript is a sanitizer report.
#include "rescuefmt.h"

#include <cstdio>
#include <cstring>

using namespace sfgpu;

extern "C" {

// the window of a job -> candidates (lo / hi written)
uint64_t rsh_window(int64_t p, uint64_t la, uint64_t lb, uint64_t tlen, int f, uint32_t window, int64_t* lo, int64_t* hi) {
    const RsWindow w = rs_window(p, la, lb, tlen, f != 0, window);
    *lo = w.lo; *hi = w.hi;
    return rs_n_candidates(w);
}

int64_t rsh_budget(uint64_t lb, uint32_t permille) { return rs_budget(lb, permille); }

// one job: the mate (oriented on strand mfwd) over the window of an anchor -> mism << 32 | x, or all ones
uint64_t rsh_job(const char* m, uint64_t lb, int mfwd, const char* t, uint64_t tlen, int64_t lo, int64_t hi, uint32_t permille, int lanes) {
    const RsWindow w{lo, hi};
    return lanes ? rs_job_lanes(m, lb, mfwd != 0, t, tlen, w, permille) : rs_job_serial(m, lb, mfwd != 0, t, tlen, w, permille);
}

// the whole pass; -> the number of output records (the outputs have room for the input's records), or -(1 + the lowest record with tid >= M)
int64_t rsh_rescue(const char* tseq, const uint64_t* tseq_off, const uint32_t* tlen, uint64_t M, const char* seq1, const uint64_t* off1, const char* seq2,
                   const uint64_t* off2, uint32_t n_reads, const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t permille, uint32_t window, int lanes,
                   sfgpu_hit* out_hits, uint32_t* out_off, uint16_t* out_mism, sfgpu_rescue_stats* stats) {
    const VfBatch b{tseq, tseq_off, tlen, M, seq1, off1, seq2, off2, n_reads, hits, hit_off};
    std::vector<sfgpu_hit> h; std::vector<uint32_t> o; std::vector<uint16_t> mm;
    const uint64_t bad = rs_serial_rescue(b, permille, window, lanes != 0, &h, &o, &mm, stats);
    if (bad) return -(int64_t)bad;
    if (!h.empty()) { memcpy(out_hits, h.data(), h.size() * sizeof(sfgpu_hit)); memcpy(out_mism, mm.data(), mm.size() * 2); }
    memcpy(out_off, o.data(), o.size() * 4);
    return (int64_t)h.size();
}

}

#ifdef RESCUE_HARNESS_MAIN
#include "hit_harness.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t n_cases = 0, hd[11];
    while (fread(hd, 8, 11, f) == 11) {
        const uint64_t n_out = hd[9];
        HarnessBatch b; std::vector<uint64_t> want_stats; std::vector<uint32_t> want_off; std::vector<sfgpu_hit> want_hits; std::vector<uint16_t> want_mism;
        if (!b.read(f, hd, 8) || !b.paired || !take(f, &want_hits, n_out) || !take(f, &want_off, b.n_reads + 1) || !take(f, &want_mism, n_out) ||
            !take(f, &want_stats, 8)) { fprintf(stderr, "case %llu: short file\n", (unsigned long long)n_cases); return 2; }
        for (int lanes = 0; lanes < 2; ++lanes) {
            std::vector<sfgpu_hit> h; std::vector<uint32_t> o; std::vector<uint16_t> mm; sfgpu_rescue_stats st;
            const VfBatch vb{b.ts.data(), b.toff.data(), b.tl.data(), b.M, b.s1.data(), b.o1.data(), b.s2.data(), b.o2.data(), (uint32_t)b.n_reads, b.hits.data(), b.hoff.data()};
            const uint64_t bad = rs_serial_rescue(vb, (uint32_t)hd[6], (uint32_t)hd[7], lanes != 0, &h, &o, &mm, &st);
            const uint64_t got_stats[8] = {st.reads_eligible, st.records_orphan, st.jobs_with_candidates, st.candidates, st.reads_rescued, st.records_rescued,
                                           st.records_dropped, st.sum_mism};
            const bool ok = !bad && h.size() == n_out && o == want_off && mm == want_mism &&
                            (n_out == 0 || !memcmp(h.data(), want_hits.data(), n_out * sizeof(sfgpu_hit))) && !memcmp(got_stats, want_stats.data(), sizeof got_stats);
            if (!ok) { fprintf(stderr, "case %llu (%s): differs from the statement\n", (unsigned long long)n_cases, lanes ? "lanes" : "serial"); return 1; }
        }
        ++n_cases;
    }
    fclose(f);
    printf("rescue harness ok: %llu cases\n", (unsigned long long)n_cases);
    return 0;
}
#endif
