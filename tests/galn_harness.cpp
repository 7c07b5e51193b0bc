// galn_harness.cpp -- csrc/galnfmt.h alone, built with g++ (no HIP): GalnSerial behind a C interface for tests/test_galn_cpu.py, which
// compares it with the Python statement hits.project_alignments_host in every array and counter.
#include <cstring>

#include "galnfmt.h"

using sfgpu::GalnSerial;

extern "C" {

// -> the handle, or nullptr where a record names no transcript (*bad_record then says which)
void* gah_project(const uint8_t* status, const int32_t* chrom, const int8_t* strand, const uint64_t* exon_off, const uint32_t* exon_start, const uint32_t* exon_len,
                  uint64_t M, const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t n_reads, const int32_t* aln_pos, const uint64_t* aln_op_off,
                  const uint32_t* aln_ops, const uint32_t* aln_nm, const uint32_t* tag_nm, const uint64_t* tag_md_off, const uint8_t* tag_md, int64_t* bad_record) {
    GalnSerial* g = new GalnSerial;
    *bad_record = g->project(status, chrom, strand, exon_off, exon_start, exon_len, M, hits, hit_off, n_reads, aln_pos, aln_op_off, aln_ops, aln_nm, tag_nm,
                             tag_md_off, tag_md);
    if (*bad_record >= 0) { delete g; return nullptr; }
    return g;
}

void gah_close(void* h) { delete static_cast<GalnSerial*>(h); }

// the counters in the order of hits.GENOME_ALN_STATS, then the records, the words and the MD bytes
void gah_sizes(void* h, uint64_t* out) {
    const GalnSerial& g = *static_cast<GalnSerial*>(h);
    std::memcpy(out, g.count, sizeof g.count);
    out[sfgpu::kGaCounters] = g.hits.size(); out[sfgpu::kGaCounters + 1] = g.ops.size(); out[sfgpu::kGaCounters + 2] = g.md.size();
}

void gah_arrays(void* h, sfgpu_hit* hits, uint32_t* hit_off, int32_t* pos, uint32_t* nm, uint64_t* op_off, uint32_t* ops, uint32_t* tag_nm, uint64_t* md_off,
                uint8_t* md, uint32_t* src_record) {
    const GalnSerial& g = *static_cast<GalnSerial*>(h);
    auto copy = [](void* to, const void* from, size_t n) { if (n) std::memcpy(to, from, n); };
    copy(hits, g.hits.data(), g.hits.size() * sizeof(sfgpu_hit)); copy(hit_off, g.hit_off.data(), g.hit_off.size() * 4);
    copy(pos, g.pos.data(), g.pos.size() * 4); copy(nm, g.nm.data(), g.nm.size() * 4); copy(op_off, g.op_off.data(), g.op_off.size() * 8);
    copy(ops, g.ops.data(), g.ops.size() * 4); copy(tag_nm, g.tag_nm.data(), g.tag_nm.size() * 4); copy(md_off, g.md_off.data(), g.md_off.size() * 8);
    copy(md, g.md.data(), g.md.size()); copy(src_record, g.src_record.data(), g.src_record.size() * 4);
}

// the MD of a line on a - transcript
void gah_md_reverse(const uint8_t* in, uint64_t n, uint8_t* out) { sfgpu::galn_md_reverse(in, n, out); }

}  // extern "C"
