// bamsort.h -- what samtext_write.hip and bamsort.hip share: the batch of sfgpu_sam_write_bgzf, checked, sized and formatted by
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

int samw_collect_bam(BamRecordStore* store, const SamwArgs& batch, sfgpu_samwrite_result* out, sfgpu_stream stream);

}  // namespace sfgpu
