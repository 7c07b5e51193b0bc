// covwrite.h -- what the transcript coverage (coverage.hip) and the genome coverage (coverage_genome.hip) share: the state of a
// transcript handle, which the projection reads, and the bedGraph writer over a run table (id, start, end, sum) with a name per id.
// cov_write is defined once, in coverage.hip, with its kernels.
#pragma once
#include "common.h"
#include "coverfmt.h"
#include "primitives.h"
#include "texttile.h"

struct sfgpu_cov {
    uint64_t M = 0, N = 0;                                 // transcripts, slots
    sfgpu::DevBuf<uint64_t> base, slot;                    // base[M + 1], slot[N]
    sfgpu_cov_stats stats{};
    bool finished = false;
    sfgpu_cov_result res{};
    sfgpu::DevBuf<uint32_t> r_tid, r_start, r_end;         // the runs
    sfgpu::DevBuf<uint64_t> r_sum;
    sfgpu::DevBuf<double> col;                             // CoveredFraction[M], MeanDepth[M], MaxDepth[M]
    uint64_t state_bytes() const {
        return 8 * (base.cap + slot.cap + r_sum.cap + col.cap) + 4 * (r_tid.cap + r_start.cap + r_end.cap);
    }
};

namespace sfgpu {

// the rows of a finished handle: run r is (id[r], start[r], end[r], sum[r]) and names[name_off[id] .. name_off[id + 1]) names its row
struct CovRunTable {
    const uint32_t *id, *start, *end;
    const uint64_t* sum;
    uint64_t n_rows, n_names;
};
struct CovWriteStats {                                     // of one write
    uint64_t n_bytes = 0, n_chunks = 0, max_row_bytes = 0;
    double format_ms = 0.0, d2h_ms = 0.0, sink_ms = 0.0;
};

// `out` starts zeroed; the caller has checked its handle and copies the figures into its own result
int cov_write(const char* who, const CovRunTable& T, const char* d_names, const uint64_t* d_name_off, uint64_t chunk_bytes, sfgpu_text_sink sink, void* user,
              sfgpu_bgzw* z, CovWriteStats* out, sfgpu_stream stream);

}  // namespace sfgpu
