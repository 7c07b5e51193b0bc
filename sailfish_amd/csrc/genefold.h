// genefold.h -- one gene of aggregateEstimatesToGeneLevel (src/SailfishUtils.cpp:988-1031, restated in genes.py
// aggregate_estimates_to_gene_level) as a function both sides call: the fold kernel of genes.hip with one lane per gene, and
// plain C++ (tests/genes_harness.cpp compiles this header with g++ and compares it with the Python loop bit by bit).
// The rows of a gene are folded in the order given, one IEEE operation per operation of the source and none fused (the library
// and the harness are compiled with -ffp-contract=off):
//   * TPM and NumReads are running sums that start at 0.0;
//   * totalTPM accumulates the RUNNING TPM sum after each add (the reference's quirk: the weights below are
//     tpm_i / (sum of prefix sums), not tpm_i / sum);
//   * with totalTPM > denorm_min, Length and EffectiveLength are weighted by tpm_i / totalTPM, otherwise by 1.0 / n (a NaN total
//     compares false and takes the second branch, as in the reference).
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SF_GENEFOLD_HD __host__ __device__ __forceinline__
#else
#define SF_GENEFOLD_HD inline
#endif

namespace sfgpu {

struct GeneRow {
    double length, eff, tpm, num_reads;       // Length enters as the double of the integer
};

struct GeneSums {
    double length, eff, tpm, num_reads;
};

// row(i) -> GeneRow of the gene's i-th row, i in [0, n); n >= 1
template <typename Row>
SF_GENEFOLD_HD GeneSums gene_fold(uint64_t n, Row row) {
    const uint64_t one = 1;
    double denorm_min;
    memcpy(&denorm_min, &one, 8);             // std::numeric_limits<double>::denorm_min()
    GeneSums g;
    g.tpm = 0.0; g.num_reads = 0.0;
    double total_tpm = 0.0;
    for (uint64_t i = 0; i < n; ++i) {
        const GeneRow r = row(i);
        g.tpm += r.tpm;
        g.num_reads += r.num_reads;
        total_tpm += g.tpm;
    }
    g.length = 0.0; g.eff = 0.0;
    if (total_tpm > denorm_min) {
        for (uint64_t i = 0; i < n; ++i) {
            const GeneRow r = row(i);
            const double frac = r.tpm / total_tpm;
            g.length += r.length * frac;
            g.eff += r.eff * frac;
        }
    } else {
        const double frac = 1.0 / (double)n;
        for (uint64_t i = 0; i < n; ++i) {
            const GeneRow r = row(i);
            g.length += r.length * frac;
            g.eff += r.eff * frac;
        }
    }
    return g;
}

}  // namespace sfgpu
