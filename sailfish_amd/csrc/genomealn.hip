// genomealn.hip -- sfgpu_galn_*: a batch of hit records and their alignment slots rewritten into genome terms through the exon blocks,
// for a second alignment writer opened over the chromosomes.  WHAT a kept record, a spliced CIGAR, a reversed MD and the counters are
// is csrc/galnfmt.h, stated once and run here unchanged; this file is only the way the work is laid out.
//
//   open           the model is validated by sfgpu_covg_open (covgfmt.h's rule, coverage_genome.hip's kernels), copied onto the handle
//                  and the block lengths scanned into 64-bit prefix sums (block e of transcript t starts at prefix[e] - prefix[exon_off[t]]).
//   k_galn_size    a lane per record: its fate, and of a kept one each line's interval, output words and MD bytes (galn_line with a
//                  put that only counts).  The start block is a binary search of the prefix sums; a line with many words or many
//                  blocks crossed loops in its lane.  The counters are summed a wavefront, then a block in LDS, and leave as one integer
//                  atomic a block each.
//   scans          keep flags -> new record index (32 bits); words and MD bytes per OLD slot, 0 for dropped records -> 64-bit offsets,
//                  which therefore are the new slots' offsets too.
//   k_galn_reads   a lane per read: the new hit_off[r] is the new index at the old hit_off[r]; reads that lost every record.
//   k_galn_emit    a lane per old slot of a kept record: line 0's lane writes the record and src_record; every lane its slot's
//                  position, nm and offsets, the words by the same walk (word k of a - line at its end - 1 - k), the MD copied or
//                  reversed.  Plain vector stores.
#include "common.h"
#include "galnfmt.h"
#include "primitives.h"
#include "texttile.h"

struct sfgpu_galn {
    uint64_t M = 0, E = 0;
    sfgpu::DevBuf<uint8_t> status;
    sfgpu::DevBuf<int32_t> chrom;
    sfgpu::DevBuf<int8_t> strand;
    sfgpu::DevBuf<uint64_t> exon_off, prefix;              // exon_off[M + 1], prefix[E + 1]
    sfgpu::DevBuf<uint32_t> exon_start, exon_len;          // [E], [E + 1]
};

namespace sfgpu {
namespace {

using textchunks::kBlock;
using textchunks::grid_of;

enum { kGaBadTid = kGaCounters, kGaBadOff, kGaSlots };      // the lowest record whose tid is no transcript; the lowest read whose offsets decrease

struct GalnModelDev {
    const uint8_t* status;
    const int32_t* chrom;
    const int8_t* strand;
    const uint64_t *exon_off, *prefix;
    const uint32_t *exon_start, *exon_len;
    uint64_t M;
};

__device__ __forceinline__ void galn_count_out(unsigned long long v, unsigned long long* __restrict__ at) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & (kWave - 1)) == 0 && v) atomicAdd(at, v);
}

__device__ __forceinline__ GalnBlocks galn_blocks_of(const GalnModelDev& G, uint64_t t) {
    const uint64_t e0 = G.exon_off[t];
    return GalnBlocks{G.prefix + e0, G.exon_start + e0, G.exon_len + e0, G.exon_off[t + 1] - e0, G.prefix[e0], (int)G.strand[t]};
}

// the offsets start at 0 and never decrease (then every record index below n = hit_off[n_reads] is some read's)
__global__ void __launch_bounds__(kBlock)
k_galn_check_off(const uint32_t* __restrict__ hit_off, uint32_t n_reads, unsigned long long* __restrict__ ctr) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_reads) return;
    if (hit_off[r] > hit_off[r + 1] || (r == 0 && hit_off[0] != 0)) atomicMin(&ctr[kGaBadOff], (unsigned long long)r);
}

__global__ void __launch_bounds__(kBlock)
k_galn_size(const GalnModelDev G, const sfgpu_galn_batch B, uint64_t n, uint32_t* __restrict__ keep, uint32_t* __restrict__ n_words /* [2 n + 1] */,
            uint32_t* __restrict__ n_md /* [2 n + 1] */, int32_t* __restrict__ lo /* [2 n] */, int32_t* __restrict__ hi, unsigned long long* __restrict__ ctr) {
    __shared__ unsigned long long s_ctr[kGaCounters];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long c[kGaCounters];
#pragma unroll
    for (int k = 0; k < kGaCounters; ++k) c[k] = 0;
    if (threadIdx.x < kGaCounters) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    if (i < n) {
        const sfgpu_hit h = B.hits[i];
        uint32_t kept = 0, words[2] = {0, 0}, md[2] = {0, 0};
        int64_t l_lo[2] = {0, 0}, l_hi[2] = {0, 0};
        if (h.tid >= G.M) atomicMin(&ctr[kGaBadTid], (unsigned long long)i);
        else {
            const uint64_t t = h.tid;
            const bool two = h.mate_status == 3;
            c[kGaRecordsIn] = 1;
            if (G.status[t] != 0 || G.exon_off[t + 1] == G.exon_off[t]) c[kGaUnplaced] = 1;
            else {
                const GalnBlocks K = galn_blocks_of(G, t);
                GalnLine line[2];
                uint32_t in_words[2] = {0, 0};
                int kind[2] = {GALN_KEPT, GALN_KEPT};
                for (uint32_t j = 0; j < (two ? 2u : 1u); ++j) {
                    const GalnWords w = galn_line_words(h, j, 2 * i + j, B.aln_pos, B.aln_op_off, B.aln_ops);
                    line[j].n_out = 0; line[j].n_N = 0; line[j].beyond = 0; line[j].lo = 0; line[j].hi = 0;
                    kind[j] = galn_line(w, K, &line[j], [](uint32_t, uint32_t) {});
                    in_words[j] = w.n;
                }
                const int fate = galn_merge(kind[0], two, kind[1]);
                if (fate == GALN_UNALIGNABLE) c[kGaUnalignable] = 1;
                else if (fate != GALN_KEPT) c[kGaOffRange] = 1;
                else {
                    kept = 1; c[kGaRecordsOut] = 1;
                    for (uint32_t j = 0; j < (two ? 2u : 1u); ++j) {
                        const uint64_t s = 2 * i + j;
                        words[j] = line[j].n_out; l_lo[j] = line[j].lo; l_hi[j] = line[j].hi;
                        if (B.tag_md_off) md[j] = (uint32_t)(B.tag_md_off[s + 1] - B.tag_md_off[s]);
                        c[kGaLines] += 1; c[kGaLinesSpliced] += line[j].n_N != 0; c[kGaNOps] += line[j].n_N; c[kGaLinesReversed] += K.strand < 0;
                        c[kGaBeyond] += line[j].beyond; c[kGaWordsIn] += in_words[j]; c[kGaWordsOut] += line[j].n_out;
                    }
                }
            }
        }
        keep[i] = kept;
        for (uint32_t j = 0; j < 2; ++j) { n_words[2 * i + j] = words[j]; n_md[2 * i + j] = md[j]; lo[2 * i + j] = (int32_t)l_lo[j]; hi[2 * i + j] = (int32_t)l_hi[j]; }
    }
    // thirteen counters: the wavefronts' sums meet in the block's LDS and leave as one atomic a block each (one a wavefront each made
    // 2 M atomics on thirteen addresses of a 10 M-record batch, which took longer than everything else together)
#pragma unroll
    for (int k = 0; k < kGaCounters; ++k) galn_count_out(c[k], &s_ctr[k]);
    __syncthreads();
    if (threadIdx.x < kGaCounters && s_ctr[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], s_ctr[threadIdx.x]);
}

// lane r <= n_reads: the new offset; lane r < n_reads: whether the read lost every record
__global__ void __launch_bounds__(kBlock)
k_galn_reads(const uint32_t* __restrict__ hit_off, uint32_t n_reads, const uint32_t* __restrict__ new_idx /* [n + 1] */, uint32_t* __restrict__ off_out,
             unsigned long long* __restrict__ ctr) {
    const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long emptied = 0;
    if (r <= n_reads) {
        const uint32_t a = new_idx[hit_off[r]];
        off_out[r] = a;
        if (r < n_reads) emptied = hit_off[r + 1] > hit_off[r] && new_idx[hit_off[r + 1]] == a;
    }
    galn_count_out(emptied, &ctr[kGaReadsEmptied]);
}

__global__ void __launch_bounds__(kBlock)
k_galn_emit(const GalnModelDev G, const sfgpu_galn_batch B, const sfgpu_galn_out O, uint64_t n, uint64_t n_out, const uint32_t* __restrict__ keep,
            const uint32_t* __restrict__ new_idx, const uint64_t* __restrict__ w_off /* [2 n + 1] */, const uint64_t* __restrict__ m_off,
            const int32_t* __restrict__ lo, const int32_t* __restrict__ hi) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= 2 * n) return;
    const uint64_t i = s >> 1;
    if (!keep[i]) return;
    const uint64_t j = new_idx[i];
    if (j >= n_out) return;                                // (never: the index is the scan of the same flags)
    const uint32_t which = (uint32_t)(s & 1u);
    const uint64_t os = 2 * j + which, wa = w_off[s], we = w_off[s + 1];
    const sfgpu_hit h = B.hits[i];
    const uint64_t t = h.tid;
    const GalnBlocks K = galn_blocks_of(G, t);
    O.aln_op_off[os] = wa;
    if (O.tag_md_off) O.tag_md_off[os] = m_off[s];
    if (os + 1 == 2 * n_out) {                             // the closing offsets: every later slot is a dropped record's and holds nothing
        O.aln_op_off[os + 1] = we;
        if (O.tag_md_off) O.tag_md_off[os + 1] = m_off[s + 1];
    }
    if (which == 0) {
        O.hits[j] = galn_record(h, (uint32_t)G.chrom[t], K.strand, lo[s], hi[s], lo[s + 1], hi[s + 1]);
        O.src_record[j] = (uint32_t)i;
    }
    const bool is_line = which == 0 || h.mate_status == 3;
    O.aln_pos[os] = is_line ? lo[s] : 0;
    if (O.aln_nm) O.aln_nm[os] = is_line && B.aln_nm ? B.aln_nm[s] : 0u;
    if (O.tag_nm) O.tag_nm[os] = is_line && B.tag_nm ? B.tag_nm[s] : 0u;
    if (!is_line) return;
    const GalnWords w = galn_line_words(h, which, s, B.aln_pos, B.aln_op_off, B.aln_ops);
    const uint64_t cnt = we - wa;
    const bool rev = K.strand < 0;
    uint32_t* __restrict__ ops = O.aln_ops;
    const uint64_t cap = O.cap_ops;
    galn_walk(w, K, [&](uint32_t k, uint32_t v) {
        const uint64_t at = wa + (rev ? cnt - 1 - k : (uint64_t)k);
        if (k < cnt && at < cap) ops[at] = v;              // (always: the count is the same walk's)
    });
    if (B.tag_md_off && O.tag_md) {
        const uint64_t a = B.tag_md_off[s], len = B.tag_md_off[s + 1] - a, at = m_off[s];
        if (len == m_off[s + 1] - at && at + len <= O.cap_md) {
            if (!rev) for (uint64_t q = 0; q < len; ++q) O.tag_md[at + q] = B.tag_md[a + q];
            else galn_md_reverse(B.tag_md + a, len, O.tag_md + at);
        }
    }
}

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_galn_open(sfgpu_galn** out, const uint8_t* d_status, const int32_t* d_chrom, const int8_t* d_strand, const uint64_t* d_exon_off,
                               const uint32_t* d_exon_start, const uint32_t* d_exon_len, uint64_t M, uint32_t n_chrom, sfgpu_stream stream) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_galn_open: null handle pointer");
    *out = nullptr;
    // the rule a model is refused by is the coverage's, run by its own entry: nulls, counts, offsets, blocks, chromosomes and strands
    sfgpu_covg* checked = nullptr;
    int rc = sfgpu_covg_open(&checked, d_status, d_chrom, d_strand, d_exon_off, d_exon_start, d_exon_len, M, n_chrom, stream);
    if (rc) return rc;
    (void)sfgpu_covg_close(checked);
    hipStream_t st = as_stream(stream);
    sfgpu_galn* g = new sfgpu_galn;
    struct Guard { sfgpu_galn* g; ~Guard() { delete g; } } guard{g};
    StreamSyncOnExit sync_first{st};
    unsigned long long h_E = 0;
    SF_HIP(hipMemcpyAsync(&h_E, d_exon_off + M, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint64_t E = h_E;
    if ((rc = g->status.reserve(M + 1, st, false)) || (rc = g->chrom.reserve(M + 1, st, false)) || (rc = g->strand.reserve(M + 1, st, false)) ||
        (rc = g->exon_off.reserve(M + 1, st, false)) || (rc = g->exon_start.reserve(E + 1, st, false)) || (rc = g->exon_len.reserve(E + 1, st, false)) ||
        (rc = g->prefix.reserve(E + 1, st, false)))
        return rc;
    if (M) {
        SF_HIP(hipMemcpyAsync(g->status.p, d_status, M, hipMemcpyDeviceToDevice, st));
        SF_HIP(hipMemcpyAsync(g->chrom.p, d_chrom, M * 4, hipMemcpyDeviceToDevice, st));
        SF_HIP(hipMemcpyAsync(g->strand.p, d_strand, M, hipMemcpyDeviceToDevice, st));
    }
    SF_HIP(hipMemcpyAsync(g->exon_off.p, d_exon_off, (M + 1) * 8, hipMemcpyDeviceToDevice, st));
    SF_HIP(hipMemsetAsync(g->exon_len.p, 0, (E + 1) * 4, st));
    if (E) {
        SF_HIP(hipMemcpyAsync(g->exon_start.p, d_exon_start, E * 4, hipMemcpyDeviceToDevice, st));
        SF_HIP(hipMemcpyAsync(g->exon_len.p, d_exon_len, E * 4, hipMemcpyDeviceToDevice, st));
    }
    if ((rc = exclusive_scan_u32(g->exon_len.p, g->prefix.p, E, st, true))) return rc;
    g->M = M; g->E = E;
    guard.g = nullptr;
    *out = g;
    return SFGPU_OK;
}

extern "C" int sfgpu_galn_close(sfgpu_galn* g) {
    if (!g) return SFGPU_OK;
    (void)hipDeviceSynchronize();
    delete g;
    return SFGPU_OK;
}

extern "C" int sfgpu_galn_project(sfgpu_galn* g, const sfgpu_galn_batch* batch, const sfgpu_galn_out* out, uint64_t* n_ops, uint64_t* n_md,
                                  sfgpu_galn_stats* stats, sfgpu_stream stream) {
    SF_REQUIRE(g && batch && out && n_ops && n_md && stats, SFGPU_ERR_INVALID, "sfgpu_galn_project: null pointer");
    const sfgpu_galn_batch& B = *batch;
    const sfgpu_galn_out& O = *out;
    SF_REQUIRE(B.hit_off && O.hit_off && O.aln_op_off, SFGPU_ERR_INVALID, "sfgpu_galn_project: null offsets");
    SF_REQUIRE((B.aln_pos && B.aln_op_off && B.aln_ops) || (!B.aln_pos && !B.aln_op_off && !B.aln_ops), SFGPU_ERR_INVALID,
               "sfgpu_galn_project: an alignment is aln_pos, aln_op_off and aln_ops, or none of them");
    SF_REQUIRE(!B.aln_nm || B.aln_pos, SFGPU_ERR_INVALID, "sfgpu_galn_project: aln_nm without an alignment");
    SF_REQUIRE((B.tag_nm && B.tag_md_off && B.tag_md) || (!B.tag_nm && !B.tag_md_off && !B.tag_md), SFGPU_ERR_INVALID,
               "sfgpu_galn_project: tags are tag_nm, tag_md_off and tag_md, or none of them");
    SF_REQUIRE(!B.tag_nm || (O.tag_nm && O.tag_md_off && (O.tag_md || O.cap_md == 0)), SFGPU_ERR_INVALID, "sfgpu_galn_project: tags given, but no room for them");
    SF_REQUIRE(O.aln_ops || O.cap_ops == 0, SFGPU_ERR_INVALID, "sfgpu_galn_project: null operations");
    hipStream_t st = as_stream(stream);
    const uint32_t R = B.n_reads;
    *n_ops = 0; *n_md = 0; *stats = sfgpu_galn_stats{};
    if (R == 0) {                             // no read: one offset each, nothing else
        SF_HIP(hipMemsetAsync(O.hit_off, 0, 4, st));
        SF_HIP(hipMemsetAsync(O.aln_op_off, 0, 8, st));
        if (B.tag_md_off) SF_HIP(hipMemsetAsync(O.tag_md_off, 0, 8, st));
        SF_HIP(hipStreamSynchronize(st));
        return SFGPU_OK;
    }
    DevBuf<unsigned long long> ctr;
    DevBuf<uint32_t> keep, new_idx, n_words, n_mdb;
    DevBuf<int32_t> lo, hi;
    DevBuf<uint64_t> w_off, m_off;
    CallScope scope;                          // (declared after the buffers: it drains the stream before scratch goes back)
    SF_HIP(scope.adopt(st));
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};             // start; sized; scanned; written
    for (auto& e : ev) SF_HIP(scope.event(&e));
    int rc;
    if ((rc = ctr.reserve(kGaSlots, st, false))) return rc;
    unsigned long long h[kGaSlots] = {0};
    h[kGaBadTid] = h[kGaBadOff] = ~0ull;
    uint32_t h_n = 0;
    SF_HIP(hipEventRecord(ev[0], st));
    SF_HIP(hipMemcpyAsync(ctr.p, h, sizeof h, hipMemcpyHostToDevice, st));
    if (R) {
        hipLaunchKernelGGL(k_galn_check_off, dim3(grid_of(R)), dim3(kBlock), 0, st, B.hit_off, R, ctr.p);
        SF_CHECK_LAUNCH();
        SF_HIP(hipMemcpyAsync(&h_n, B.hit_off + R, 4, hipMemcpyDeviceToHost, st));
    }
    SF_HIP(hipMemcpyAsync(h, ctr.p, sizeof h, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h[kGaBadOff] != ~0ull) {
        set_error("sfgpu_galn_project: the hit offsets of read %llu decrease or do not start at 0", h[kGaBadOff]);
        return SFGPU_ERR_INVALID;
    }
    const uint64_t n = h_n;
    SF_REQUIRE(n == 0 || (B.hits && O.hits && O.aln_pos && O.src_record), SFGPU_ERR_INVALID, "sfgpu_galn_project: null records");
    if ((rc = keep.reserve(n + 1, st, false)) || (rc = new_idx.reserve(n + 1, st, false)) || (rc = n_words.reserve(2 * n + 1, st, false)) ||
        (rc = n_mdb.reserve(2 * n + 1, st, false)) || (rc = lo.reserve(2 * n + 1, st, false)) || (rc = hi.reserve(2 * n + 1, st, false)) ||
        (rc = w_off.reserve(2 * n + 1, st, false)) || (rc = m_off.reserve(2 * n + 1, st, false)))
        return rc;
    const GalnModelDev G = {g->status.p, g->chrom.p, g->strand.p, g->exon_off.p, g->prefix.p, g->exon_start.p, g->exon_len.p, g->M};
    SF_HIP(hipMemsetAsync(keep.p, 0, (n + 1) * 4, st));
    SF_HIP(hipMemsetAsync(n_words.p, 0, (2 * n + 1) * 4, st));
    SF_HIP(hipMemsetAsync(n_mdb.p, 0, (2 * n + 1) * 4, st));
    if (n) {
        hipLaunchKernelGGL(k_galn_size, dim3(grid_of(n)), dim3(kBlock), 0, st, G, B, n, keep.p, n_words.p, n_mdb.p, lo.p, hi.p, ctr.p);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipEventRecord(ev[1], st));
    if ((rc = exclusive_scan_u32_u32(keep.p, new_idx.p, n, st))) return rc;
    if ((rc = exclusive_scan_u32(n_words.p, w_off.p, 2 * n, st, false))) return rc;
    if ((rc = exclusive_scan_u32(n_mdb.p, m_off.p, 2 * n, st, false))) return rc;
    SF_HIP(hipEventRecord(ev[2], st));
    uint32_t h_out = 0;
    unsigned long long h_words = 0, h_md = 0;
    SF_HIP(hipMemcpyAsync(h, ctr.p, sizeof h, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_out, new_idx.p + n, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_words, w_off.p + 2 * n, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h_md, m_off.p + 2 * n, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h[kGaBadTid] != ~0ull) {
        set_error("sfgpu_galn_project: record %llu names transcript >= %llu", h[kGaBadTid], (unsigned long long)g->M);
        return SFGPU_ERR_RANGE;
    }
    SF_REQUIRE(h_out == h[kGaRecordsOut] && h_words == h[kGaWordsOut], SFGPU_ERR_HIP, "sfgpu_galn_project: the counts lost their way");
    *n_ops = h_words; *n_md = h_md;
    if (h_words > O.cap_ops || h_md > O.cap_md) {
        set_error("sfgpu_galn_project: %llu operations and %llu MD bytes do not fit the room for %llu and %llu", h_words, h_md,
                  (unsigned long long)O.cap_ops, (unsigned long long)O.cap_md);
        return SFGPU_ERR_RANGE;
    }
    const uint64_t n_out = h_out;
    SF_HIP(hipMemsetAsync(O.aln_op_off, 0, 8, st));           // the offsets of a batch that keeps nothing
    if (B.tag_md_off) SF_HIP(hipMemsetAsync(O.tag_md_off, 0, 8, st));
    hipLaunchKernelGGL(k_galn_reads, dim3(grid_of((uint64_t)R + 1)), dim3(kBlock), 0, st, B.hit_off, R, (const uint32_t*)new_idx.p, O.hit_off, ctr.p);
    SF_CHECK_LAUNCH();
    if (n_out) {
        hipLaunchKernelGGL(k_galn_emit, dim3(grid_of(2 * n)), dim3(kBlock), 0, st, G, B, O, n, n_out, (const uint32_t*)keep.p, (const uint32_t*)new_idx.p,
                           (const uint64_t*)w_off.p, (const uint64_t*)m_off.p, (const int32_t*)lo.p, (const int32_t*)hi.p);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipEventRecord(ev[3], st));
    SF_HIP(hipMemcpyAsync(h, ctr.p, sizeof h, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    stats->records_in = h[kGaRecordsIn]; stats->records_out = h[kGaRecordsOut]; stats->records_unplaced = h[kGaUnplaced];
    stats->records_unalignable = h[kGaUnalignable]; stats->records_off_range = h[kGaOffRange]; stats->reads_emptied = h[kGaReadsEmptied];
    stats->lines = h[kGaLines]; stats->lines_spliced = h[kGaLinesSpliced]; stats->n_operations = h[kGaNOps]; stats->lines_reversed = h[kGaLinesReversed];
    stats->columns_beyond_model = h[kGaBeyond]; stats->words_in = h[kGaWordsIn]; stats->words_out = h[kGaWordsOut];
    add_elapsed(&stats->project_ms, ev[0], ev[3]); add_elapsed(&stats->size_ms, ev[0], ev[1]);
    add_elapsed(&stats->scan_ms, ev[1], ev[2]); add_elapsed(&stats->emit_ms, ev[2], ev[3]);
    return SFGPU_OK;
}
