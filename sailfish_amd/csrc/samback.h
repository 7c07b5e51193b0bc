// samback.h -- the back end the alignment readers share (samtext.hip: SAM text, bamtext.hip: BAM records): from "one SamLine per
// alignment" (kept packed: Lines), the records in file order (rec_line[k] = the line of record k; bamtext.hip passes the identity)
// and the group heads to pairs, survivors, sort keys and sfgpu_hit records.  What pairs and which record two lines make is
// samfmt.h's.  The handle's name table (XXH64, linear probing, a byte compare behind every hash match) lies here too.
#pragma once
#include "common.h"
#include "samfmt.h"
#include "xxh64_device.h"

namespace sfgpu {
namespace samback {

constexpr int kBlock = 256;

// ---- the name table of a handle (built by sfgpu_sam_open) --------------------------------------------------------------------

// XXH64 over the name's bytes as little-endian words, the last one zero-padded (a hash only: equality is the byte compare)
__device__ inline uint64_t name_hash(const unsigned char* q, uint32_t n) {
    return xxh64_words([q, n](uint32_t i) {
        uint32_t w = 0;
        for (uint32_t b = 0; b < 4 && 4 * i + b < n; ++b) w |= (uint32_t)q[4 * i + b] << (8 * b);
        return w;
    }, (n + 3) / 4);
}

struct NameTable {
    const unsigned char* blob;
    const uint64_t* off;          // [M + 1]
    const uint32_t* slot;         // [mask + 1]: 0 = empty, else the name's index + 1
    uint32_t mask;
    __device__ bool is(uint32_t t, const unsigned char* q, uint32_t n) const {
        if (off[t + 1] - off[t] != n) return false;
        const unsigned char* a = blob + off[t];
        for (uint32_t i = 0; i < n; ++i)
            if (a[i] != q[i]) return false;
        return true;
    }
    __device__ uint32_t find(const unsigned char* q, uint32_t n) const {
        uint32_t at = (uint32_t)name_hash(q, n) & mask;
        for (uint32_t probe = 0; probe <= mask; ++probe, at = (at + 1) & mask) {
            const uint32_t v = slot[at];
            if (v == 0) return kSamNone;
            if (is(v - 1, q, n)) return v - 1;
        }
        return kSamNone;
    }
};

// ---- lines, groups, pairs, records -----------------------------------------------------------------------------------------

// what k_sam_lines keeps of a line: read_len | mapped << 16 | fwd << 17 | side << 18
__device__ inline uint32_t pack_line(const SamLine& l) {
    return (uint32_t)l.read_len | (uint32_t)l.mapped << 16 | (uint32_t)l.fwd << 17 | (uint32_t)l.side << 18;
}
struct Lines {
    const uint32_t* info;
    const uint32_t* tid;
    const int32_t* pos;
    __device__ SamLine operator()(uint32_t j) const {
        const uint32_t w = info[j];
        SamLine l = {0, 0, tid[j], pos[j], (uint16_t)(w & 0xffffu), 0, (uint8_t)((w >> 16) & 1u), (uint8_t)((w >> 18) & 3u), (uint8_t)((w >> 17) & 1u)};
        return l;
    }
};

__device__ inline uint32_t group_of(const uint32_t* head, const uint32_t* head_scan, uint32_t k) { return head_scan[k] + head[k] - 1u; }

// records below Kc: pair_head[k], has_pair[group] (preset to 0)
[[maybe_unused]] static __global__ void k_sam_pairs(uint32_t Kc, const uint32_t* __restrict__ rec_line, const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_scan,
                            Lines lines, uint32_t* __restrict__ pair_head, uint32_t* __restrict__ has_pair) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Kc) return;
    const bool ph = k + 1 < Kc && !head[k + 1] && sam_pairs_with(lines(rec_line[k]), lines(rec_line[k + 1]));
    pair_head[k] = ph ? 1u : 0u;
    if (ph) has_pair[group_of(head, head_scan, k)] = 1u;
}

// surv[k] = record k yields a record (K entries, 0 from Kc on); *n_pairs += the pair heads.  No lane leaves before the ballot.
[[maybe_unused]] static __global__ void __launch_bounds__(kBlock) k_sam_survive(uint32_t K, uint32_t Kc, const uint32_t* __restrict__ rec_line, const uint32_t* __restrict__ head,
                                                        const uint32_t* __restrict__ head_scan, Lines lines, const uint32_t* __restrict__ pair_head,
                                                        const uint32_t* __restrict__ has_pair, uint32_t* __restrict__ surv,
                                                        unsigned long long* __restrict__ n_pairs) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    bool pair = false;
    if (k < K) {
        bool s = false;
        if (k < Kc) {
            pair = pair_head[k] != 0;
            s = has_pair[group_of(head, head_scan, k)] ? pair : lines(rec_line[k]).mapped != 0;
        }
        surv[k] = s ? 1u : 0u;
    }
    const unsigned long long b = __ballot(pair);
    if ((threadIdx.x & (kWave - 1)) == 0 && b) atomicAdd(n_pairs, (unsigned long long)__popcll(b));
}

// off[group] = the survivors in front of its head; the survivors' sort keys, their values = the record
[[maybe_unused]] static __global__ void k_sam_keys(uint32_t Kc, const uint32_t* __restrict__ rec_line, const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_scan,
                           Lines lines, const uint32_t* __restrict__ surv, const uint32_t* __restrict__ surv_scan, uint32_t* __restrict__ off,
                           uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Kc) return;
    const uint32_t g = group_of(head, head_scan, k), at = surv_scan[k];
    if (head[k]) off[g] = at;
    if (!surv[k]) return;
    const SamLine l = lines(rec_line[k]);
    key[at] = sam_sort_key(g, l.side == 2, l.tid);        // (a pair head is a left mate)
    val[at] = k;
}

[[maybe_unused]] static __global__ void k_sam_write(uint32_t n_hits, const uint32_t* __restrict__ order, const uint32_t* __restrict__ rec_line,
                            const uint32_t* __restrict__ pair_head, Lines lines, sfgpu_hit* __restrict__ hits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_hits) return;
    const uint32_t k = order[i];
    const SamLine a = lines(rec_line[k]);
    hits[i] = pair_head[k] ? sam_pair_hit(a, lines(rec_line[k + 1])) : sam_single_hit(a);
}

}  // namespace samback
}  // namespace sfgpu

// the handle of sfgpu_sam_open; sfgpu_bam_open holds one for its names
struct sfgpu_sam {
    bool paired = false;
    uint64_t M = 0;
    uint32_t mask = 0;
    sfgpu::DevBuf<unsigned char> blob;
    sfgpu::DevBuf<uint64_t> off;
    sfgpu::DevBuf<uint32_t> slot;
};
