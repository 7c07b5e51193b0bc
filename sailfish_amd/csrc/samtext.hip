// samtext.hip -- a mapper's SAM text turned into sfgpu_hit records and read offsets on the device: sfgpu_sam_*.  What a line says,
// which lines pair and what record they make is decided by samfmt.h (the same functions run serially in tests/sam_harness.cpp);
// this file is the passes around them.  No pass walks a line: the cost of a call depends on its bytes and its lines, not on how
// long a line or how large a group is.
//
// The text (whole lines) lies on the device as 16-byte groups.  The line front end -- k_sam_count, k_sam_line_ends, k_sam_tabs,
// k_sam_lines, k_sam_compact: where the lines and their tabs are and what each line says -- is samfront.h (the collated reading of
// samcollate.hip runs it too).  Then
//   k_sam_heads        record k begins a group when its QNAME differs from record k - 1's; a scan of the heads numbers the groups;
//                      the last head is where a text that is not final is cut
//   k_sam_pairs        pair heads are a neighbour test (sam_pairs_with); "this group has a pair" is a plain store of 1 by every pair
//                      head into the group's flag: the segmented OR without a segment walk
//   k_sam_survive, scan, k_sam_keys   the lines that yield a record, compacted; d_off[group] = the survivors in front of its head;
//                      key = (group, right orphan, tid)
//   sort_pairs_u64_u32 (stable: ties stay in file order), k_sam_write   the records, sam_pair_hit / sam_single_hit
// Everything from k_sam_pairs on lies in samback.h: bamtext.hip runs the same kernels behind its own front end.  The host text is
// staged by textstage.h.
#include "common.h"
#include "primitives.h"
#include "samback.h"
#include "samfmt.h"
#include "samfront.h"
#include "textlines.h"
#include "textstage.h"
#include "xxh64_device.h"

namespace sfgpu {
namespace {

using namespace samback;
using namespace samfront;

// ---- the name table -------------------------------------------------------------------------------------------------------

// every name into the table; *flag |= 1: a name occurs twice, 2: the offsets decrease or a name has 2^32 bytes or more
__global__ void k_sam_table(const unsigned char* __restrict__ blob, const uint64_t* __restrict__ off, uint32_t M, uint32_t* __restrict__ slot,
                            uint32_t mask, uint32_t* __restrict__ flag) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    if (off[t + 1] < off[t] || off[t + 1] - off[t] > 0xfffffffeull) { atomicOr(flag, 2u); return; }
    const unsigned char* q = blob + off[t];
    const uint32_t n = (uint32_t)(off[t + 1] - off[t]);
    const NameTable T{blob, off, slot, mask};
    uint32_t at = (uint32_t)name_hash(q, n) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe, at = (at + 1) & mask) {
        const uint32_t old = atomicCAS(&slot[at], 0u, t + 1);
        if (old == 0) return;
        if (T.is(old - 1, q, n)) { atomicOr(flag, 1u); return; }
    }
}

// ---- groups, pairs, records -----------------------------------------------------------------------------------------------

// head[k] = record k's QNAME differs from record k - 1's
__global__ void k_sam_heads(const unsigned char* __restrict__ bytes, uint32_t K, const uint32_t* __restrict__ rec_line,
                            const uint32_t* __restrict__ line_end, const uint32_t* __restrict__ tab_pos, uint32_t* __restrict__ head) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    if (k == 0) { head[0] = 1; return; }
    const uint32_t j = rec_line[k], i = rec_line[k - 1];
    const uint32_t sj = line_end[j - 1] + 1, si = i ? line_end[i - 1] + 1 : 0;        // (j > i >= 0; tab 0 of a record exists)
    const uint32_t n = tab_pos[j] - sj;
    bool same = tab_pos[i] - si == n;
    for (uint32_t b = 0; same && b < n; ++b) same = bytes[sj + b] == bytes[si + b];
    head[k] = same ? 0u : 1u;
}

// the last head: cut[0] = its record, cut[1] = its line, cut[2] = where that line begins
__global__ void k_sam_cut(uint32_t K, const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_scan, const uint32_t* __restrict__ rec_line,
                          const uint32_t* __restrict__ line_end, uint32_t* __restrict__ cut) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K || !head[k] || head_scan[k] + 1 != head_scan[K]) return;
    const uint32_t j = rec_line[k];
    cut[0] = k; cut[1] = j; cut[2] = j ? line_end[j - 1] + 1 : 0;
}

struct Scratch : Front {                          // (word[1]: the pairs)
    DevBuf<uint4> text;
    DevBuf<uint32_t> rec_line, head, head_scan, pair_head, has_pair, surv, surv_scan, val, val2, cut;
    DevBuf<uint64_t> key, key2;
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

namespace {

// The text on the device: [0, n_text) ends in a '\n' (whole lines); `used` of its bytes are the caller's (n_text - used = 1 when
// the '\n' of the last line was supplied).  h: 8 pinned 64-bit words.
int parse_device_text(sfgpu_sam* m, Scratch& S, const uint4* text, uint64_t n_text, uint64_t used, bool final, sfgpu_hit* d_hits,
                      uint64_t cap_hits, uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, hipStream_t st, uint64_t* h) {
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(text);
    uint32_t* h32 = reinterpret_cast<uint32_t*>(h);
    if (int r = S.cut.reserve(4, st, false)) return r;
    uint32_t L = 0;
    if (int r = sam_front_lines(m, S, text, n_text, st, h32, &L)) return r;
    if (L == 0) return SFGPU_OK;

    // ---- the lines
    if (int r = exclusive_scan_u32_u32(S.isrec.p, S.rec_scan.p, L, st)) return r;
    SF_HIP(hipMemcpyAsync(&h[1], S.word.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h32[0], S.rec_scan.p + L, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h[1] != kNoBad) {
        res->bad = (uint32_t)(h[1] & 0xffu);
        res->bad_line = h[1] >> 8;
        set_error("sfgpu_sam_parse: line %llu of the text is malformed (SFGPU_SAM_BAD_* %u)", (unsigned long long)res->bad_line, res->bad);
        return SFGPU_ERR_FORMAT;
    }
    const uint32_t K = h32[0];
    if (K == 0) {                                         // header lines only
        res->n_lines = res->n_header = L;
        res->consumed = used;
        return SFGPU_OK;
    }

    // ---- the groups
    for (DevBuf<uint32_t>* b : {&S.rec_line, &S.head, &S.head_scan, &S.pair_head, &S.has_pair, &S.surv, &S.surv_scan})
        if (int r = b->reserve((uint64_t)K + 2, st, false)) return r;
    hipLaunchKernelGGL(k_sam_compact, dim3(grid_of(L)), dim3(kBlock), 0, st, L, S.isrec.p, S.rec_scan.p, S.rec_line.p);
    SF_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sam_heads, dim3(grid_of(K)), dim3(kBlock), 0, st, bytes, K, S.rec_line.p, S.line_end.p, S.tab_pos.p, S.head.p);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(S.head.p, S.head_scan.p, K, st)) return r;
    hipLaunchKernelGGL(k_sam_cut, dim3(grid_of(K)), dim3(kBlock), 0, st, K, S.head.p, S.head_scan.p, S.rec_line.p, S.line_end.p, S.cut.p);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(&h32[0], S.head_scan.p + K, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h32[1], S.cut.p, 12, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t n_groups_seen = h32[0];
    const uint32_t Kc = final ? K : h32[1], n_reads = final ? n_groups_seen : n_groups_seen - 1;
    const uint64_t n_lines = final ? L : h32[2], consumed = final ? used : h32[3];
    if (n_reads == 0) {                                   // one group, held back: the header lines in front of it may go
        res->n_lines = res->n_header = n_lines;
        res->consumed = consumed;
        return SFGPU_OK;
    }

    // ---- the records
    const Lines lines{S.info.p, S.tid.p, S.pos.p};
    SF_HIP(hipMemsetAsync(S.has_pair.p, 0, (uint64_t)n_reads * 4, st));
    if (m->paired) {
        hipLaunchKernelGGL(k_sam_pairs, dim3(grid_of(Kc)), dim3(kBlock), 0, st, Kc, S.rec_line.p, S.head.p, S.head_scan.p, lines, S.pair_head.p,
                           S.has_pair.p);
        SF_CHECK_LAUNCH();
    } else {
        SF_HIP(hipMemsetAsync(S.pair_head.p, 0, (uint64_t)Kc * 4, st));
    }
    hipLaunchKernelGGL(k_sam_survive, dim3(grid_of(K)), dim3(kBlock), 0, st, K, Kc, S.rec_line.p, S.head.p, S.head_scan.p, lines, S.pair_head.p,
                       S.has_pair.p, S.surv.p, S.word.p + 1);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(S.surv.p, S.surv_scan.p, K, st)) return r;
    SF_HIP(hipMemcpyAsync(&h32[0], S.surv_scan.p + K, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h[1], S.word.p + 1, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t n_hits = h32[0];
    if (n_hits > cap_hits || n_reads > cap_reads) {
        res->need_hits = n_hits; res->need_reads = n_reads;
        set_error("sfgpu_sam_parse: %u records in %u reads do not fit cap_hits = %llu, cap_reads = %llu", n_hits, n_reads,
                  (unsigned long long)cap_hits, (unsigned long long)cap_reads);
        return SFGPU_ERR_CAPACITY;
    }
    for (DevBuf<uint64_t>* b : {&S.key, &S.key2}) if (int r = b->reserve((uint64_t)n_hits + 2, st, false)) return r;
    for (DevBuf<uint32_t>* b : {&S.val, &S.val2}) if (int r = b->reserve((uint64_t)n_hits + 2, st, false)) return r;
    hipLaunchKernelGGL(k_sam_keys, dim3(grid_of(Kc)), dim3(kBlock), 0, st, Kc, S.rec_line.p, S.head.p, S.head_scan.p, lines, S.surv.p, S.surv_scan.p, d_off,
                       S.key.p, S.val.p);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(d_off + n_reads, S.surv_scan.p + K, 4, hipMemcpyDeviceToDevice, st));
    if (n_hits) {
        int group_bits = 1;
        while (group_bits < 31 && (1u << group_bits) < n_reads) ++group_bits;
        if (int r = sort_pairs_u64_u32(S.key.p, S.key2.p, S.val.p, S.val2.p, n_hits, st, 33 + group_bits, false)) return r;
        hipLaunchKernelGGL(k_sam_write, dim3(grid_of(n_hits)), dim3(kBlock), 0, st, n_hits, S.val2.p, S.rec_line.p, S.pair_head.p, lines, d_hits);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipStreamSynchronize(st));
    res->n_lines = n_lines; res->n_header = n_lines - Kc; res->n_reads = n_reads; res->n_hits = n_hits; res->n_pairs = h[1];
    res->consumed = consumed;
    return SFGPU_OK;
}

int check_parse_args(const char* who, sfgpu_sam* m, const void* text, uint64_t n_bytes, sfgpu_hit* d_hits, uint64_t cap_hits, uint32_t* d_off,
                     sfgpu_sam_result* res) {
    if (!m || !res) { set_error("%s: null handle or result", who); return SFGPU_ERR_INVALID; }
    memset(res, 0, sizeof(*res));
    if (n_bytes > kMaxBytes) { set_error("%s: more than 2^30 bytes in one call", who); return SFGPU_ERR_RANGE; }
    if ((n_bytes && !text) || !d_off || (cap_hits && !d_hits)) { set_error("%s: null array", who); return SFGPU_ERR_INVALID; }
    return SFGPU_OK;
}

}  // namespace

extern "C" int sfgpu_sam_open(sfgpu_sam** out, const char* d_names, const uint64_t* d_name_off, uint64_t M, int paired, sfgpu_stream stream) {
    SF_REQUIRE(out && d_name_off, SFGPU_ERR_INVALID, "sfgpu_sam_open: null handle or offsets");
    SF_REQUIRE(M < 0xffffffffull - 1, SFGPU_ERR_RANGE, "sfgpu_sam_open: 2^32 - 1 names or more");
    hipStream_t st = as_stream(stream);
    sfgpu_sam* m = new sfgpu_sam;
    m->paired = paired != 0;
    m->M = M;
    uint64_t size = 64;
    while (size < 2 * M) size *= 2;
    m->mask = (uint32_t)(size - 1);
    DevBuf<uint32_t> flag;
    auto build = [&]() -> int {
        CallScope scope;
        uint64_t* h = nullptr;
        SF_HIP(scope.adopt(st));
        SF_HIP(scope.pinned_block(&h, 2 * sizeof(uint64_t)));
        if (int r = m->off.reserve(M + 1, st, false)) return r;
        if (int r = m->slot.reserve(size, st, false)) return r;
        if (int r = flag.reserve(1, st, false)) return r;
        SF_HIP(hipMemcpyAsync(m->off.p, d_name_off, (M + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        SF_HIP(hipMemcpyAsync(&h[0], d_name_off + M, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(&h[1], d_name_off, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        const uint64_t n_bytes = h[0];
        SF_REQUIRE(h[1] == 0 && (d_names || n_bytes == 0), SFGPU_ERR_INVALID, "sfgpu_sam_open: offsets must start at 0 over non-null names");
        if (int r = m->blob.reserve(n_bytes + 1, st, false)) return r;
        if (n_bytes) SF_HIP(hipMemcpyAsync(m->blob.p, d_names, n_bytes, hipMemcpyDeviceToDevice, st));
        SF_HIP(hipMemsetAsync(m->slot.p, 0, size * 4, st));
        SF_HIP(hipMemsetAsync(flag.p, 0, 4, st));
        if (M) {
            hipLaunchKernelGGL(k_sam_table, dim3(grid_of(M)), dim3(kBlock), 0, st, m->blob.p, m->off.p, (uint32_t)M, m->slot.p, m->mask, flag.p);
            SF_CHECK_LAUNCH();
        }
        uint32_t* h32 = reinterpret_cast<uint32_t*>(h);
        SF_HIP(hipMemcpyAsync(h32, flag.p, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        SF_REQUIRE(!(h32[0] & 2u), SFGPU_ERR_INVALID, "sfgpu_sam_open: the name offsets decrease");
        SF_REQUIRE(!(h32[0] & 1u), SFGPU_ERR_INVALID, "sfgpu_sam_open: a transcript name occurs twice");
        return SFGPU_OK;
    };
    const int rc = build();
    if (rc != SFGPU_OK) { (void)hipStreamSynchronize(st); delete m; return rc; }
    *out = m;
    return SFGPU_OK;
}

extern "C" int sfgpu_sam_close(sfgpu_sam* m) {
    if (!m) return SFGPU_OK;
    (void)hipDeviceSynchronize();
    delete m;
    return SFGPU_OK;
}

extern "C" int sfgpu_sam_parse_host(sfgpu_sam* m, const char* h_text, uint64_t n_bytes, int final, sfgpu_hit* d_hits, uint64_t cap_hits,
                                    uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream) {
    if (int r = check_parse_args("sfgpu_sam_parse_host", m, h_text, n_bytes, d_hits, cap_hits, d_off, res)) return r;
    hipStream_t st = as_stream(stream);
    SF_HIP(hipMemsetAsync(d_off, 0, 4, st));
    uint64_t used = n_bytes;
    if (!final) while (used && h_text[used - 1] != '\n') --used;
    if (used == 0) { SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }
    const bool append = h_text[used - 1] != '\n';            // (final only)
    const uint64_t n_text = used + (append ? 1 : 0);

    Scratch S;
    CallScope scope;        // after S: it drains both streams before S's blocks go back to the pool
    HostStage H;
    if (int r = stage_host_text(scope, H, S.text, h_text, used, append, st)) return r;
    const int rc = parse_device_text(m, S, S.text.p, n_text, used, final != 0, d_hits, cap_hits, d_off, cap_reads, res, st, H.h);
    SF_HIP(hipEventRecord(H.ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_copy, H.ev_c0, H.ev_c1);
    add_elapsed(&res->ms_kernels, H.ev_k0, H.ev_k1);
    return rc;
}

extern "C" int sfgpu_sam_parse_device(sfgpu_sam* m, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, sfgpu_hit* d_hits,
                                      uint64_t cap_hits, uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream) {
    if (int r = check_parse_args("sfgpu_sam_parse_device", m, d_text, n_bytes, d_hits, cap_hits, d_off, res)) return r;
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_sam_parse_device: d_text must be 16-byte aligned");
    SF_REQUIRE(n_bytes == 0 || cap_text >= ((n_bytes + 1 + 15) & ~15ull) + 16, SFGPU_ERR_INVALID,
               "sfgpu_sam_parse_device: cap_text must hold the text, a '\\n', the rest of that 16-byte group and one group more");
    hipStream_t st = as_stream(stream);
    SF_HIP(hipMemsetAsync(d_off, 0, 4, st));
    if (n_bytes == 0) { SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }
    Scratch S;
    DevBuf<unsigned long long> last;
    CallScope scope;        // after the scratch, as in sfgpu_sam_parse_host
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;
    uint64_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_k0));
    SF_HIP(scope.event(&ev_k1));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint64_t)));
    if (int r = last.reserve(1, st, false)) return r;
    SF_HIP(hipEventRecord(ev_k0, st));
    SF_HIP(hipMemsetAsync(last.p, 0, 8, st));
    hipLaunchKernelGGL(textlines::k_last_nl, dim3(grid_of((n_bytes + 15) / 16)), dim3(kBlock), 0, st, d_text, n_bytes, last.p);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(&h[7], last.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint64_t used = final ? n_bytes : h[7];
    int rc = SFGPU_OK;
    if (used) {
        uint64_t n_text = used;
        if (final && h[7] != n_bytes) {                      // the last line lacks its '\n': it goes into the slack
            SF_HIP(hipMemsetAsync(d_text + n_bytes, '\n', 1, st));
            n_text = n_bytes + 1;
        }
        rc = parse_device_text(m, S, reinterpret_cast<const uint4*>(d_text), n_text, used, final != 0, d_hits, cap_hits, d_off, cap_reads, res, st, h);
    }
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_kernels, ev_k0, ev_k1);
    return rc;
}
