// samfront.h -- the line front end the SAM text readers share (samtext.hip: name-grouped files; samcollate.hip: the collated
// reading): from a text of whole lines on the device, as 16-byte groups, to "one SamLine per line", kept packed.  What a line says is
// samfmt.h's.  No pass walks a line.
//   k_sam_count        per group: its '\n' and its '\t' bytes
//   scans, k_sam_line_ends   where line j ends, and how many tabs stand in front of it
//   k_sam_tabs         per group: the tab at p is tab number (tabs in front of p) - (tabs in front of its line) of line (newlines in
//                      front of p); the first ten of a line are stored.  SEQ's length is a difference of two of them, so nobody
//                      reads SEQ or QUAL.
//   k_sam_lines        one lane per line: samfmt.h's sam_parse_line over FLAG, RNAME, POS and CIGAR; RNAME is looked up in the
//                      handle's table.  The lowest malformed line is a 64-bit min (one atomic per wavefront that holds one).
//   k_sam_compact      behind a scan: the non-header lines ("records of the text"), in order
#pragma once
#include "common.h"
#include "primitives.h"
#include "samback.h"
#include "samfmt.h"
#include "textlines.h"

namespace sfgpu {
namespace samfront {

using textlines::eq_mask;
using textlines::range_mask;
using namespace samback;

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
constexpr uint64_t kMaxBytes = 1ull << 30;               // one call
constexpr unsigned long long kNoBad = ~0ull;

struct Bytes {
    const unsigned char* p;
    __device__ unsigned char operator()(uint32_t i) const { return p[i]; }
};


[[maybe_unused]] static __global__ void k_sam_count(const uint4* __restrict__ buf, uint64_t n_groups, uint64_t n_text, uint32_t* __restrict__ nl_cnt,
                            uint32_t* __restrict__ tab_cnt) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint4 v = buf[g];
    const uint32_t in = range_mask(g * 16, 0, n_text);
    nl_cnt[g] = __popc(eq_mask(v, '\n') & in);
    tab_cnt[g] = __popc(eq_mask(v, '\t') & in);
}

// line_end[j] = the '\n' that ends line j; line_tab0[j] = the tabs in front of line j
[[maybe_unused]] static __global__ void k_sam_line_ends(const uint4* __restrict__ buf, uint64_t n_groups, uint64_t n_text, const uint32_t* __restrict__ nl_scan,
                                const uint32_t* __restrict__ tab_scan, uint32_t* __restrict__ line_end, uint32_t* __restrict__ line_tab0) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint4 v = buf[g];
    const uint32_t in = range_mask(g * 16, 0, n_text);
    uint32_t nl = eq_mask(v, '\n') & in;
    const uint32_t tabs = eq_mask(v, '\t') & in;
    uint32_t at = nl_scan[g];
    const uint32_t t0 = tab_scan[g];
    if (g == 0) line_tab0[0] = 0;
    while (nl) {
        const int i = __ffs(nl) - 1;
        nl &= nl - 1;
        line_end[at] = (uint32_t)(g * 16 + i);
        line_tab0[at + 1] = t0 + __popc(tabs & ((1u << i) - 1u));
        ++at;
    }
}

// tab_pos[ord * L + j] = the ord-th tab of line j, ord < kSamTabs (the array is preset to kSamNone)
[[maybe_unused]] static __global__ void k_sam_tabs(const uint4* __restrict__ buf, uint64_t n_groups, uint64_t n_text, const uint32_t* __restrict__ nl_scan,
                           const uint32_t* __restrict__ tab_scan, const uint32_t* __restrict__ line_tab0, uint32_t L,
                           uint32_t* __restrict__ tab_pos) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint4 v = buf[g];
    const uint32_t in = range_mask(g * 16, 0, n_text);
    const uint32_t tabs = eq_mask(v, '\t') & in;
    if (!tabs) return;
    const uint32_t nl = eq_mask(v, '\n') & in;
    const uint32_t j0 = nl_scan[g];
    uint32_t t = tab_scan[g];
    for (uint32_t w = tabs; w; w &= w - 1, ++t) {
        const int i = __ffs(w) - 1;
        const uint32_t j = j0 + __popc(nl & ((1u << i) - 1u));
        if (j >= L) return;                               // (the text ends in a '\n': no tab stands behind the last line)
        const uint32_t ord = t - line_tab0[j];
        if (ord < kSamTabs) tab_pos[(uint64_t)ord * L + j] = (uint32_t)(g * 16 + i);
    }
}

// One lane per line.  No lane leaves before the shuffles.
[[maybe_unused]] static __global__ void __launch_bounds__(kBlock) k_sam_lines(const unsigned char* __restrict__ bytes, uint32_t L, const uint32_t* __restrict__ line_end,
                                                      const uint32_t* __restrict__ tab_pos, int paired, NameTable T, uint32_t* __restrict__ info,
                                                      uint32_t* __restrict__ tid, int32_t* __restrict__ pos, uint32_t* __restrict__ isrec,
                                                      unsigned long long* __restrict__ first_bad) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = kNoBad;
    if (j < L) {
        const Bytes get{bytes};
        const uint32_t s = j ? line_end[j - 1] + 1 : 0;
        const uint32_t e = sam_line_end(get, s, line_end[j]);
        uint32_t tab[kSamTabs];
#pragma unroll
        for (uint32_t o = 0; o < kSamTabs; ++o) tab[o] = tab_pos[(uint64_t)o * L + j];
        const SamLine l = sam_parse_line(get, s, e, tab, paired != 0, [&](uint32_t a, uint32_t n) { return T.find(bytes + a, n); });
        info[j] = pack_line(l); tid[j] = l.tid; pos[j] = l.pos; isrec[j] = l.header ? 0u : 1u;
        if (l.bad) key = ((unsigned long long)j << 8) | l.bad;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other < key ? other : key;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && key != kNoBad) atomicMin(first_bad, key);
}

[[maybe_unused]] static __global__ void k_sam_compact(uint32_t L, const uint32_t* __restrict__ isrec, const uint32_t* __restrict__ rec_scan, uint32_t* __restrict__ rec_line) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < L && isrec[j]) rec_line[rec_scan[j]] = j;
}

// what the front end leaves on the device
struct Front {
    DevBuf<uint32_t> nl_cnt, nl_scan, tab_cnt, tab_scan, line_end, line_tab0, tab_pos, info, tid, isrec, rec_scan;
    DevBuf<int32_t> pos;
    DevBuf<unsigned long long> word;              // [0] the lowest malformed line, [1] a counter of the caller's (zeroed)
};

// The text [0, n_text) ends in a '\n' (whole lines).  -> *L, its lines; with L != 0 the line arrays of F (line_end, tab_pos, info, tid,
// pos, isrec) and word[0] are launched on st, nothing of them waited for.  h32: a pinned word.
inline int sam_front_lines(const sfgpu_sam* m, Front& F, const uint4* text, uint64_t n_text, hipStream_t st, uint32_t* h32, uint32_t* L) {
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(text);
    const uint64_t n_groups = (n_text + 15) / 16;
    *L = 0;
    for (DevBuf<uint32_t>* b : {&F.nl_cnt, &F.nl_scan, &F.tab_cnt, &F.tab_scan}) if (int r = b->reserve(n_groups + 2, st, false)) return r;
    if (int r = F.word.reserve(2, st, false)) return r;
    hipLaunchKernelGGL(k_sam_count, dim3(grid_of(n_groups)), dim3(kBlock), 0, st, text, n_groups, n_text, F.nl_cnt.p, F.tab_cnt.p);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(F.nl_cnt.p, F.nl_scan.p, n_groups, st)) return r;
    if (int r = exclusive_scan_u32_u32(F.tab_cnt.p, F.tab_scan.p, n_groups, st)) return r;
    SF_HIP(hipMemcpyAsync(&h32[0], F.nl_scan.p + n_groups, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t n_lines = h32[0];
    if (n_lines == 0) return SFGPU_OK;
    for (DevBuf<uint32_t>* b : {&F.line_end, &F.line_tab0, &F.info, &F.tid, &F.isrec, &F.rec_scan}) if (int r = b->reserve((uint64_t)n_lines + 2, st, false)) return r;
    if (int r = F.pos.reserve((uint64_t)n_lines + 2, st, false)) return r;
    if (int r = F.tab_pos.reserve((uint64_t)kSamTabs * n_lines, st, false)) return r;
    SF_HIP(hipMemsetAsync(F.tab_pos.p, 0xff, (uint64_t)kSamTabs * n_lines * 4, st));
    SF_HIP(hipMemsetAsync(F.word.p, 0xff, 8, st));
    SF_HIP(hipMemsetAsync(F.word.p + 1, 0, 8, st));
    hipLaunchKernelGGL(k_sam_line_ends, dim3(grid_of(n_groups)), dim3(kBlock), 0, st, text, n_groups, n_text, F.nl_scan.p, F.tab_scan.p, F.line_end.p,
                       F.line_tab0.p);
    SF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sam_tabs, dim3(grid_of(n_groups)), dim3(kBlock), 0, st, text, n_groups, n_text, F.nl_scan.p, F.tab_scan.p, F.line_tab0.p, n_lines,
                       F.tab_pos.p);
    SF_CHECK_LAUNCH();
    const NameTable T{m->blob.p, m->off.p, m->slot.p, m->mask};
    hipLaunchKernelGGL(k_sam_lines, dim3(grid_of(n_lines)), dim3(kBlock), 0, st, bytes, n_lines, F.line_end.p, F.tab_pos.p, m->paired ? 1 : 0, T, F.info.p,
                       F.tid.p, F.pos.p, F.isrec.p, F.word.p);
    SF_CHECK_LAUNCH();
    *L = n_lines;
    return SFGPU_OK;
}

}  // namespace samfront
}  // namespace sfgpu
