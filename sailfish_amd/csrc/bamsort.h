// bamsort.h -- what samtext_write.hip and bamsort.hip share: the batch of sfgpu_sam_write_bgzf_q, checked, sized and formatted by
// samtext_write.hip's own code (sam_write, k_format_units<BamFmt>), lands in a record store instead of an encoder.
#pragma once
#include "common.h"
#include "samwfmt.h"

#include <functional>

namespace sfgpu {

struct BamRecordStore {
    // A batch that passed every check: `total` bytes of n_records BAM records in n_units units whose byte starts are
    // d_unit_start[0 .. n_units] (device, alive until st has drained).  format_all(buf, s) enqueues on s the kernels that write the
    // batch's bytes to buf (16-byte aligned, room for total rounded up to 16).  *format_ms += the device time.  Returns a status;
    // on anything but SFGPU_OK the store is as it was.
    virtual int take(uint64_t total, uint64_t n_records, const uint64_t* d_unit_start, uint64_t n_units, hipStream_t st, double* format_ms,
                     const std::function<int(uint4*, hipStream_t)>& format_all) = 0;
protected:
    ~BamRecordStore() = default;
};

// The batch of a writer entry (include/sfgpu.h), as the entry was given it: the widest argument list of the families, in the
// order of SamwArgs' fields.  Every layer behind the entries takes the struct.
inline SamwArgs samw_batch(const sfgpu_hit* d_hits, const uint32_t* d_hit_offsets, uint32_t n_reads, int paired, const char* d_ref_names,
                           const uint64_t* d_ref_name_off, uint32_t n_refs, const char* d_qnames, const uint64_t* d_qname_off,
                           const uint8_t* d_seq1, const int64_t* d_seq1_off, const uint8_t* d_seq2, const int64_t* d_seq2_off,
                           uint64_t read_index_base, const uint8_t* d_qual1, const uint8_t* d_qual2, int oriented, const int32_t* d_aln_pos,
                           const uint64_t* d_aln_op_off, const uint32_t* d_aln_ops, const sfgpu_samw_tags* tags,
                           const sfgpu_samw_post* post) {
    return SamwArgs{d_hits, d_hit_offsets, n_reads, paired, d_ref_names, d_ref_name_off, n_refs, d_qnames, d_qname_off, d_seq1, d_seq1_off,
                    d_seq2, d_seq2_off, read_index_base, d_qual1, d_qual2, oriented, d_aln_pos, d_aln_op_off, d_aln_ops,
                    tags ? tags->d_nm : nullptr, tags ? tags->d_md_off : nullptr, tags ? tags->d_md : nullptr,
                    post ? post->d_zw_rec : nullptr, post ? post->d_zw_f32 : nullptr};
}

int samw_collect_bam(BamRecordStore* store, const SamwArgs& batch, sfgpu_samwrite_result* out, sfgpu_stream stream);

}  // namespace sfgpu
