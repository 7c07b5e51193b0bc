// covgenome_harness.cpp -- csrc/covgfmt.h alone, built with g++ (no HIP): CovGenomeSerial behind a C interface for
// tests/test_covgenome_cpu.py, which compares it with the Python statement hits.coverage_genome_host in the runs, the counters and the
// bytes of the text.
#include <cstring>

#include "covgfmt.h"

using sfgpu::CovGenomeSerial;

extern "C" {

int64_t cgh_check(const uint8_t* status, const int32_t* chrom, const int8_t* strand, const uint64_t* exon_off, const uint32_t* exon_start, const uint32_t* exon_len,
                  uint64_t M, uint32_t n_chrom) {
    return CovGenomeSerial::check(status, chrom, strand, exon_off, exon_start, exon_len, M, n_chrom);
}

void* cgh_project(const uint8_t* status, const int32_t* chrom, const int8_t* strand, const uint64_t* exon_off, const uint32_t* exon_start, const uint32_t* exon_len,
                  const uint32_t* ref_len, uint64_t M, const uint32_t* t_tid, const uint32_t* t_start, const uint32_t* t_end, const uint64_t* t_sum, uint64_t n_runs) {
    CovGenomeSerial* g = new CovGenomeSerial;
    g->project(status, chrom, strand, exon_off, exon_start, exon_len, ref_len, M, t_tid, t_start, t_end, t_sum, n_runs);
    return g;
}

void cgh_close(void* h) { delete static_cast<CovGenomeSerial*>(h); }

// n_pieces, n_events, n_keys, n_runs, bases_covered, runs_unplaced, bases_unplaced, bases_off_model, transcripts_placed, transcripts_length_mismatch
void cgh_stats(void* h, uint64_t* out) {
    const CovGenomeSerial& g = *static_cast<CovGenomeSerial*>(h);
    const uint64_t v[10] = {g.count.pieces, g.n_events, g.n_keys, g.r_chrom.size(), g.bases_covered, g.count.runs_unplaced, g.count.bases_unplaced,
                            g.count.bases_off_model, g.placed, g.length_mismatch};
    std::memcpy(out, v, sizeof v);
}

void cgh_runs(void* h, uint32_t* chrom, uint32_t* start, uint32_t* end, uint64_t* sum) {
    const CovGenomeSerial& g = *static_cast<CovGenomeSerial*>(h);
    const size_t n = g.r_chrom.size();
    if (!n) return;
    std::memcpy(chrom, g.r_chrom.data(), n * 4); std::memcpy(start, g.r_start.data(), n * 4);
    std::memcpy(end, g.r_end.data(), n * 4); std::memcpy(sum, g.r_sum.data(), n * 8);
}

// the file's size; written to `out` where that is not null
uint64_t cgh_text(void* h, const char* names, const uint64_t* name_off, char* out) {
    const std::string s = static_cast<CovGenomeSerial*>(h)->text(names, name_off);
    if (out) std::memcpy(out, s.data(), s.size());
    return s.size();
}

}  // extern "C"
