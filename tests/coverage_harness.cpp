// coverage_harness.cpp -- csrc/coverfmt.h alone, as plain C++ (g++ -Wall -Wextra -Werror): the coverage pass as the header states it
// serially (CovSerial: add per batch, finish, the runs, the summary columns, the bytes of the file), for tests/test_coverage_cpu.py to
// compare with hits.coverage_host and coverage.coverage_text_host.  Built with -DCOVERAGE_HARNESS_MAIN (and
// -fsanitize=address,undefined) it is a stand-alone program: it reads the corpus with its expected result from a file
// (tests/coverage_corpus.py: blob), every array in a block of exactly its size, and runs the pass over it.
#include "coverfmt.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace sfgpu;

extern "C" {

void* ch_open(const uint32_t* ref_len, uint64_t M) { return new CovSerial(ref_len, M); }
void ch_close(void* c) { delete static_cast<CovSerial*>(c); }

// -> 0; -(1 + the lowest record whose tid is no transcript); 1 + the lowest record whose p is refused; INT64_MIN: the lines would
// reach 2^32; INT64_MIN + 1: after finish.  p and the alignment (all three or none) may be NULL
int64_t ch_add(void* c, const void* hits, const uint32_t* hit_off, uint32_t n_reads, const double* p, const int32_t* aln_pos, const uint64_t* aln_op_off,
               const uint32_t* aln_ops) {
    return static_cast<CovSerial*>(c)->add(static_cast<const sfgpu_hit*>(hits), hit_off, n_reads, p, aln_pos, aln_op_off, aln_ops);
}

// out[9]: reads, records, lines, intervals, empty_intervals, bases_added, runs, bases_covered, residue
void ch_finish(void* c, uint64_t* out) {
    CovSerial* s = static_cast<CovSerial*>(c);
    s->finish();
    const uint64_t v[9] = {s->stats.reads, s->stats.records, s->stats.lines, s->stats.intervals, s->stats.empty_intervals, s->stats.bases_added,
                           (uint64_t)s->r_tid.size(), s->covered, s->residue};
    memcpy(out, v, sizeof v);
}

void ch_runs(void* c, uint32_t* tid, uint32_t* start, uint32_t* end, uint64_t* sum) {
    const CovSerial* s = static_cast<const CovSerial*>(c);
    const size_t n = s->r_tid.size();
    if (!n) return;
    memcpy(tid, s->r_tid.data(), 4 * n); memcpy(start, s->r_start.data(), 4 * n); memcpy(end, s->r_end.data(), 4 * n); memcpy(sum, s->r_sum.data(), 8 * n);
}

// cols[3 M]: CoveredFraction, MeanDepth, MaxDepth
void ch_summary(void* c, double* cols) {
    const CovSerial* s = static_cast<const CovSerial*>(c);
    const size_t M = s->len.size();
    if (!M) return;
    memcpy(cols, s->frac.data(), 8 * M); memcpy(cols + M, s->mean.data(), 8 * M); memcpy(cols + 2 * M, s->maxd.data(), 8 * M);
}

// the file's bytes -> their number; out == NULL: only counted
uint64_t ch_text(void* c, const char* names, const uint64_t* name_off, char* out) {
    const std::string t = static_cast<const CovSerial*>(c)->text(names, name_off);
    if (out && !t.empty()) memcpy(out, t.data(), t.size());
    return t.size();
}

uint64_t ch_weight(double p) { return cov_weight(p); }
int ch_p_bad(double p) { return cov_p_bad(p); }
uint64_t ch_div128(uint64_t hi, uint64_t lo, uint32_t d) { return cov_div128(hi, lo, d); }
double ch_depth(uint64_t sum) { return cov_depth(sum); }

}

#ifdef COVERAGE_HARNESS_MAIN
template <typename T>
static bool take(FILE* f, std::vector<T>* v, uint64_t n) {
    v->resize(n);
    return n == 0 || fread(v->data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t hd[8];      // M, reads, records, words, runs, text bytes, flags (1: p, 2: alignments), name bytes
    std::vector<uint32_t> ref_len, off, a_ops, w_tid, w_start, w_end; std::vector<sfgpu_hit> hits; std::vector<double> p, w_cols; std::vector<int32_t> a_pos;
    std::vector<uint64_t> a_off, w_sum, w_stats, nm_off; std::vector<char> nm, w_text;
    if (fread(hd, 8, 8, f) != 8 || !take(f, &ref_len, hd[0]) || !take(f, &hits, hd[2]) || !take(f, &off, hd[1] + 1) || !take(f, &p, hd[2]) || !take(f, &a_pos, 2 * hd[2]) ||
        !take(f, &a_off, 2 * hd[2] + 1) || !take(f, &a_ops, hd[3]) || !take(f, &w_tid, hd[4]) || !take(f, &w_start, hd[4]) || !take(f, &w_end, hd[4]) ||
        !take(f, &w_sum, hd[4]) || !take(f, &w_cols, 3 * hd[0]) || !take(f, &w_stats, 9) || !take(f, &nm_off, hd[0] + 1) || !take(f, &nm, hd[7]) || !take(f, &w_text, hd[5])) {
        fprintf(stderr, "short file\n"); return 2;
    }
    fclose(f);
    const bool with_p = hd[6] & 1, with_aln = hd[6] & 2;
    // once whole, once read by read: the result does not depend on the batches
    for (int split = 0; split < 2; ++split) {
        CovSerial c(ref_len.data(), hd[0]);
        if (!split) {
            if (c.add(hits.data(), off.data(), (uint32_t)hd[1], with_p ? p.data() : nullptr, with_aln ? a_pos.data() : nullptr, with_aln ? a_off.data() : nullptr,
                      with_aln ? a_ops.data() : nullptr)) { fprintf(stderr, "add refused the corpus\n"); return 1; }
        } else {
            for (uint64_t r = 0; r < hd[1]; ++r) {
                const uint64_t h0 = off[r], h1 = off[r + 1];
                const std::vector<sfgpu_hit> h(hits.begin() + h0, hits.begin() + h1);
                const std::vector<double> pp(p.begin() + h0, p.begin() + h1);
                const std::vector<int32_t> ap(a_pos.begin() + 2 * h0, a_pos.begin() + 2 * h1);
                std::vector<uint64_t> ao(a_off.begin() + 2 * h0, a_off.begin() + 2 * h1 + 1);
                const std::vector<uint32_t> ops(a_ops.begin() + ao.front(), a_ops.begin() + ao.back());
                const uint64_t first = ao.front();
                for (auto& v : ao) v -= first;
                const uint32_t o2[2] = {0, (uint32_t)(h1 - h0)};
                if (c.add(h.data(), o2, 1, with_p ? pp.data() : nullptr, with_aln ? ap.data() : nullptr, with_aln ? ao.data() : nullptr, with_aln ? ops.data() : nullptr)) {
                    fprintf(stderr, "add refused read %llu\n", (unsigned long long)r); return 1;
                }
            }
        }
        uint64_t st[9];
        ch_finish(&c, st);
        const std::string text = c.text(nm.data(), nm_off.data());
        const bool ok = !memcmp(st, w_stats.data(), sizeof st) && c.r_tid == w_tid && c.r_start == w_start && c.r_end == w_end && c.r_sum == w_sum &&
                        !memcmp(c.frac.data(), w_cols.data(), 8 * hd[0]) && !memcmp(c.mean.data(), w_cols.data() + hd[0], 8 * hd[0]) &&
                        !memcmp(c.maxd.data(), w_cols.data() + 2 * hd[0], 8 * hd[0]) && text.size() == w_text.size() && !memcmp(text.data(), w_text.data(), text.size());
        if (!ok) { fprintf(stderr, "%s: differs from the statement\n", split ? "read by read" : "whole"); return 1; }
        if (c.add(hits.data(), off.data(), 0, nullptr, nullptr, nullptr, nullptr) != INT64_MIN + 1) { fprintf(stderr, "add after finish was not refused\n"); return 1; }
    }
    printf("coverage harness ok: %llu reads, %llu records, %llu runs\n", (unsigned long long)hd[1], (unsigned long long)hd[2], (unsigned long long)hd[4]);
    return 0;
}
#endif
