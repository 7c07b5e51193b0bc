// mapidx.h -- the mapper's index handle (sfgpu_index): built and searched by mapper.hip, whose transcript text verify.hip reads.
#pragma once
#include "common.h"

struct sfgpu_index {
    uint32_t k = 31, shift = 0, max_occ = 1000, n_seeds = 2;
    uint32_t seed_len = 0;                 // != 0: scan mode with seeds of this many bases (the default: min(19, k)); 0: end seeds
    uint64_t n_valid = 0, n_slots = 0, M = 0, n_buckets = 0;
    sfgpu::DevBuf<uint64_t> keys; sfgpu::DevBuf<uint32_t> tid, tpos, bucket;
    sfgpu::DevBuf<char> tseq; sfgpu::DevBuf<uint64_t> tseq_off; sfgpu::DevBuf<uint32_t> tlen;      // the transcripts' text (scan mode extends matches on it; sfgpu_hits_verify compares reads with it)
};
