// genes.hip -- the `--geneMap` step on the device (aggregateEstimatesToGeneLevel, src/SailfishUtils.cpp:929-1037): the rows of
// quant.sf folded into genes from the columns where they lie (sfgpu_genes_aggregate), and the rows of quant.genes.sf written
// from the result (sfgpu_genes_write_text, the kGene instance of rowtext.h).  Contracts in sfgpu.h.
//   1. round    as_printed: every double becomes the one strtod reads back from its %g token.  k_round does gfmt_decode_fast
//               -> gfmt_value_fast in registers; a cell outside either window is left pending and k_round_slow, a kernel of its
//               own (its limb arrays live in scratch memory), finishes it.
//   2. group    a stable radix sort (primitives.h) of (gene id, row): the rows of a gene become consecutive, in row order.
//   3. order    the heads of the sorted groups are flagged and scanned (group number of every sorted position, group starts);
//               a group's first row is its smallest, so the flags "row r opens a gene", scanned over the rows, give every
//               gene its output line: genes come out in order of their first rows, without a second sort.
//   4. gather   one pass over the sorted positions copies the four columns into group order: consecutive lanes write
//               consecutive addresses, and the fold below reads each gene from consecutive addresses.
//   5. fold     one lane per gene runs gene_fold (genefold.h, the function the host harness runs) over its rows and stores the
//               gene at its output line.  A gene is one serial chain of IEEE additions by definition, so the parallelism is
//               across genes: ~24 000 genes of ~8 rows fill the device for microseconds, while ONE gene that holds every
//               row is folded by one lane at memory latency, two passes of dependent adds: measured, 0.20 s for one gene of
//               1 000 000 rows on an MI355X (tools/genes_probe.py, profiles/genes_probe.json).  That case stays correct -- it is the same function -- and is reported as
//               max_rows_per_gene.
#include "common.h"
#include "genefold.h"
#include "gfmt.h"
#include "primitives.h"
#include "rowtext.h"

#include <cstring>

namespace sfgpu {
namespace {

using textchunks::kBlock;
using textchunks::grid_of;

constexpr uint64_t kMaxRows = 0xffffffffull;

struct Cols3 {
    const double* c[3];
};

// misc[0] = 1 when a row's gene id is not below n_gene_ids
__global__ void k_check_ids(const uint32_t* __restrict__ gene_of_row, uint64_t n_rows, uint64_t n_gene_ids, unsigned long long* __restrict__ misc) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rows && gene_of_row[r] >= n_gene_ids) atomicOr(&misc[0], 1ull);
}

// val[col * n_rows + r] = the printed value of column col, row r, where both fast halves answer; otherwise pend holds
// kGfmtPending (no record yet) or the record whose value is outstanding, and the cell is counted in misc[1].  pend = 0: done
// (no record is 0: a record with digits has D >= 1)
__global__ void __launch_bounds__(kBlock)
k_round(Cols3 cols, uint64_t n_rows, double* __restrict__ val, uint32_t* __restrict__ pend, unsigned long long* __restrict__ misc) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double* __restrict__ col = blockIdx.y == 0 ? cols.c[0] : blockIdx.y == 1 ? cols.c[1] : cols.c[2];
    uint32_t p = 0;
    if (r < n_rows) {
        const uint64_t i = (uint64_t)blockIdx.y * n_rows + r;
        const uint32_t g = gfmt_decode_fast(col[r]);
        p = g;
        if (g != kGfmtPending) {
            bool vp;
            const double v = gfmt_value_fast(g, &vp);
            if (!vp) { val[i] = v; p = 0; }
        }
        pend[i] = p;
    }
    const unsigned long long m = __ballot(p != 0);
    if (m && (threadIdx.x & (kWave - 1)) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(&misc[1], (unsigned long long)__popcll(m));
}

// the pending cells, launched over all cells: most lanes leave at once
__global__ void __launch_bounds__(kBlock)
k_round_slow(Cols3 cols, uint64_t n_rows, double* __restrict__ val, const uint32_t* __restrict__ pend) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const uint64_t i = (uint64_t)blockIdx.y * n_rows + r;
    uint32_t g = pend[i];
    if (g == 0) return;
    if (g == kGfmtPending) {
        const double* __restrict__ col = blockIdx.y == 0 ? cols.c[0] : blockIdx.y == 1 ? cols.c[1] : cols.c[2];
        g = gfmt_decode_slow(col[r]);
    }
    bool slow;
    val[i] = gfmt_value(g, &slow);
}

__global__ void k_keys(const uint32_t* __restrict__ gene_of_row, uint64_t n_rows, uint64_t* __restrict__ key, uint32_t* __restrict__ row) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    key[r] = gene_of_row[r];
    row[r] = (uint32_t)r;
}

// head[i] = 1 where sorted position i opens a group; opens[row] = 1 for the row at such a position (opens is zeroed before)
__global__ void k_heads(const uint64_t* __restrict__ key, const uint32_t* __restrict__ row, uint64_t n_rows, uint32_t* __restrict__ head,
                        uint32_t* __restrict__ opens) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t h = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
    head[i] = h;
    if (h) opens[row[i]] = 1u;
}

// grp[i] = heads before position i (so a head at i opens group grp[i]); gstart[group] = its first position, gstart[n_groups] = n_rows
__global__ void k_group_starts(const uint32_t* __restrict__ head, const uint32_t* __restrict__ grp, uint64_t n_rows, uint32_t* __restrict__ gstart) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_rows) return;
    if (i == n_rows) gstart[grp[n_rows]] = (uint32_t)n_rows;
    else if (head[i]) gstart[grp[i]] = (uint32_t)i;
}

// the columns in group order: position i takes row row[i]
__global__ void k_gather(const uint32_t* __restrict__ row, uint64_t n_rows, const uint32_t* __restrict__ length, const double* __restrict__ eff,
                         const double* __restrict__ tpm, const double* __restrict__ num_reads, uint32_t* __restrict__ g_length,
                         double* __restrict__ g_eff, double* __restrict__ g_tpm, double* __restrict__ g_num_reads) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t r = row[i];
    g_length[i] = length[r];
    g_eff[i] = eff[r];
    g_tpm[i] = tpm[r];
    g_num_reads[i] = num_reads[r];
}

// one lane per group; its output line is the number of genes opened by earlier rows than its first row
__global__ void __launch_bounds__(kBlock)
k_fold(const uint32_t* __restrict__ gstart, uint64_t n_groups, const uint64_t* __restrict__ key, const uint32_t* __restrict__ row,
       const uint32_t* __restrict__ line_of_row, const uint32_t* __restrict__ g_length, const double* __restrict__ g_eff,
       const double* __restrict__ g_tpm, const double* __restrict__ g_num_reads, uint32_t* __restrict__ gene_id_out,
       double* __restrict__ length_out, double* __restrict__ eff_out, double* __restrict__ tpm_out, double* __restrict__ num_reads_out,
       unsigned long long* __restrict__ misc) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long n = 0;
    if (j < n_groups) {
        const uint64_t a = gstart[j];
        n = gstart[j + 1] - a;
        const GeneSums s = gene_fold(n, [&](uint64_t i) {
            GeneRow r;
            r.length = (double)g_length[a + i]; r.eff = g_eff[a + i]; r.tpm = g_tpm[a + i]; r.num_reads = g_num_reads[a + i];
            return r;
        });
        const uint32_t line = line_of_row[row[a]];
        gene_id_out[line] = (uint32_t)key[a];
        length_out[line] = s.length; eff_out[line] = s.eff; tpm_out[line] = s.tpm; num_reads_out[line] = s.num_reads;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(n, o);
        n = other > n ? other : n;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && n) atomicMax(&misc[2], n);
}

struct GeneScratch {
    DevBuf<double> val, g_col;
    DevBuf<uint32_t> pend, row_in, row_out, head, grp, opens, line_of_row, gstart, g_length;
    DevBuf<uint64_t> key_in, key_out;
    DevBuf<unsigned long long> misc;          // [0] bad id, [1] slow cells, [2] longest gene
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_genes_aggregate(const uint32_t* d_gene_of_row, const uint32_t* d_length, const double* d_eff, const double* d_tpm,
                                     const double* d_num_reads, uint64_t n_rows, uint64_t n_gene_ids, int as_printed,
                                     uint32_t* d_gene_id_out, double* d_length_out, double* d_eff_out, double* d_tpm_out,
                                     double* d_num_reads_out, sfgpu_genes_result* out, sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_genes_aggregate: null result");
    memset(out, 0, sizeof(*out));
    if (n_rows == 0) return SFGPU_OK;
    SF_REQUIRE(d_gene_of_row && d_length && d_eff && d_tpm && d_num_reads, SFGPU_ERR_INVALID, "sfgpu_genes_aggregate: null column");
    SF_REQUIRE(d_gene_id_out && d_length_out && d_eff_out && d_tpm_out && d_num_reads_out, SFGPU_ERR_INVALID, "sfgpu_genes_aggregate: null output");
    SF_REQUIRE(n_rows < kMaxRows, SFGPU_ERR_RANGE, "sfgpu_genes_aggregate: n_rows must be below 2^32 - 1");
    SF_REQUIRE(n_gene_ids > 0 && n_gene_ids <= 0x100000000ull, SFGPU_ERR_INVALID, "sfgpu_genes_aggregate: n_gene_ids must lie in [1, 2^32] when there are rows");

    GeneScratch S;
    CallScope scope;        // after S: it drains the stream before S's blocks go back to the pool
    hipStream_t st = nullptr;
    hipEvent_t ev_in = nullptr, ev_t[2] = {nullptr, nullptr};
    unsigned long long* h_misc = nullptr;     // [0 .. 2] misc, [3] groups
    const unsigned grid = grid_of(n_rows);
    SF_HIP(scope.acquire(&st));
    SF_HIP(scope.event(&ev_in, hipEventDisableTiming));
    for (auto& e : ev_t) SF_HIP(scope.event(&e));
    SF_HIP(scope.pinned_block(&h_misc, 4 * sizeof(unsigned long long)));
    // behind whatever the caller has queued on `stream`
    SF_HIP(hipEventRecord(ev_in, as_stream(stream)));
    SF_HIP(hipStreamWaitEvent(st, ev_in, 0));

    if (int rc = S.misc.reserve(4, st, false)) return rc;
    if (as_printed) {
        if (int rc = S.val.reserve(3 * n_rows, st, false)) return rc;
        if (int rc = S.pend.reserve(3 * n_rows, st, false)) return rc;
    }
    for (DevBuf<uint64_t>* b : {&S.key_in, &S.key_out}) if (int rc = b->reserve(n_rows, st, false)) return rc;
    for (DevBuf<uint32_t>* b : {&S.row_in, &S.row_out}) if (int rc = b->reserve(n_rows, st, false)) return rc;
    for (DevBuf<uint32_t>* b : {&S.head, &S.grp, &S.opens, &S.line_of_row, &S.gstart}) if (int rc = b->reserve(n_rows + 1, st, false)) return rc;
    if (int rc = S.g_length.reserve(n_rows, st, false)) return rc;
    if (int rc = S.g_col.reserve(3 * n_rows, st, false)) return rc;

    SF_HIP(hipEventRecord(ev_t[0], st));
    SF_HIP(hipMemsetAsync(S.misc.p, 0, 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_check_ids, dim3(grid), dim3(kBlock), 0, st, d_gene_of_row, n_rows, n_gene_ids, S.misc.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    SF_REQUIRE(!h_misc[0], SFGPU_ERR_INVALID, "sfgpu_genes_aggregate: a gene id is not below n_gene_ids");

    // ---- 1. round to printed
    const double* eff = d_eff; const double* tpm = d_tpm; const double* num_reads = d_num_reads;
    if (as_printed) {
        const Cols3 cols = {{d_eff, d_tpm, d_num_reads}};
        hipLaunchKernelGGL(k_round, dim3(grid, 3), dim3(kBlock), 0, st, cols, n_rows, S.val.p, S.pend.p, S.misc.p);
        SF_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_round_slow, dim3(grid, 3), dim3(kBlock), 0, st, cols, n_rows, S.val.p, S.pend.p);
        SF_HIP(hipGetLastError());
        eff = S.val.p; tpm = S.val.p + n_rows; num_reads = S.val.p + 2 * n_rows;
    }
    // ---- 2. group: stable sort of (gene id, row)
    int id_bits = 1;
    while (id_bits < 32 && (n_gene_ids - 1) >> id_bits) ++id_bits;
    hipLaunchKernelGGL(k_keys, dim3(grid), dim3(kBlock), 0, st, d_gene_of_row, n_rows, S.key_in.p, S.row_in.p);
    SF_HIP(hipGetLastError());
    if (int rc = sort_pairs_u64_u32(S.key_in.p, S.key_out.p, S.row_in.p, S.row_out.p, n_rows, st, id_bits, false)) return rc;
    // ---- 3. group heads, group starts, the output line of every gene
    SF_HIP(hipMemsetAsync(S.opens.p, 0, (n_rows + 1) * sizeof(uint32_t), st));
    SF_HIP(hipMemsetAsync(S.head.p + n_rows, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_heads, dim3(grid), dim3(kBlock), 0, st, S.key_out.p, S.row_out.p, n_rows, S.head.p, S.opens.p);
    SF_HIP(hipGetLastError());
    if (int rc = exclusive_scan_u32_u32(S.head.p, S.grp.p, n_rows, st)) return rc;
    if (int rc = exclusive_scan_u32_u32(S.opens.p, S.line_of_row.p, n_rows, st)) return rc;
    hipLaunchKernelGGL(k_group_starts, dim3(grid_of(n_rows + 1)), dim3(kBlock), 0, st, S.head.p, S.grp.p, n_rows, S.gstart.p);
    SF_HIP(hipGetLastError());
    unsigned long long n_groups = 0;
    {
        uint32_t* h_groups = reinterpret_cast<uint32_t*>(&h_misc[3]);
        SF_HIP(hipMemcpyAsync(h_groups, S.grp.p + n_rows, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        // ---- 4. gather (does not need the count)
        hipLaunchKernelGGL(k_gather, dim3(grid), dim3(kBlock), 0, st, S.row_out.p, n_rows, d_length, eff, tpm, num_reads, S.g_length.p,
                           S.g_col.p, S.g_col.p + n_rows, S.g_col.p + 2 * n_rows);
        SF_HIP(hipGetLastError());
        SF_HIP(hipStreamSynchronize(st));
        n_groups = *h_groups;
    }
    SF_REQUIRE(n_groups > 0 && n_groups <= n_rows && n_groups <= n_gene_ids, SFGPU_ERR_HIP, "sfgpu_genes_aggregate: the grouping pass lost its count");
    // ---- 5. fold
    hipLaunchKernelGGL(k_fold, dim3(grid_of(n_groups)), dim3(kBlock), 0, st, S.gstart.p, (uint64_t)n_groups, S.key_out.p, S.row_out.p,
                       S.line_of_row.p, S.g_length.p, S.g_col.p, S.g_col.p + n_rows, S.g_col.p + 2 * n_rows, d_gene_id_out, d_length_out,
                       d_eff_out, d_tpm_out, d_num_reads_out, S.misc.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipEventRecord(ev_t[1], st));
    SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&out->aggregate_ms, ev_t[0], ev_t[1]);
    out->n_rows = n_rows; out->n_genes = n_groups; out->n_slow = h_misc[1]; out->max_rows_per_gene = h_misc[2];
    return SFGPU_OK;
}

extern "C" int sfgpu_genes_write_text(const char* d_names, const uint64_t* d_name_off, uint64_t n_gene_ids, const uint32_t* d_gene_id,
                                      const double* d_length, const double* d_eff, const double* d_tpm, const double* d_num_reads,
                                      uint64_t n_rows, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
                                      sfgpu_quant_write_result* out, sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_genes_write_text: null result");
    memset(out, 0, sizeof(*out));
    if (chunk_bytes == 0) chunk_bytes = rowtext::kDefaultChunk;
    SF_REQUIRE(chunk_bytes >= 16 && chunk_bytes <= rowtext::kMaxChunk, SFGPU_ERR_INVALID,
               "sfgpu_genes_write_text: chunk_bytes must lie in [16, 2^30] (0 = default)");
    if (n_rows == 0) return SFGPU_OK;
    SF_REQUIRE(d_name_off && d_gene_id && d_length && d_eff && d_tpm && d_num_reads, SFGPU_ERR_INVALID, "sfgpu_genes_write_text: null column");
    SF_REQUIRE(n_rows < rowtext::kMaxRows, SFGPU_ERR_RANGE, "sfgpu_genes_write_text: n_rows must be below 2^32 - 1");
    SF_REQUIRE(n_gene_ids > 0 && n_gene_ids <= 0x100000000ull, SFGPU_ERR_INVALID, "sfgpu_genes_write_text: n_gene_ids must lie in [1, 2^32] when there are rows");
    const rowtext::Cols cols = {{d_length, d_eff, d_tpm, d_num_reads}};
    return rowtext::write_rows<true>("sfgpu_genes_write_text", d_names, d_name_off, n_gene_ids, d_gene_id, cols, n_rows, chunk_bytes, sink, user,
                                     out, stream);
}
