// bamtext.hip -- a mapper's BAM record stream (the bytes behind the BGZF inflate) turned into sfgpu_hit records and read offsets on
// the device: sfgpu_bam_*.  What the stream says is bamfmt.h; the back end (pairs, survivors, the stable sort, the records) is
// samback.h, the kernels samtext.hip runs.
// The front end -- the record chain, resolved exactly and in parallel, and k_bam_records -- is bamfront.h (the collated reading of
// samcollate.hip runs it too).  Here:
//   k_bam_heads     record k begins a group when its name differs from record k - 1's
// and samback.h, with rec_line = the identity.
#include "bamfmt.h"
#include "bamfront.h"
#include "common.h"
#include "primitives.h"
#include "samback.h"
#include "textstage.h"

namespace sfgpu {
namespace {

using namespace samback;
using namespace bamfront;

// ---- the records ----------------------------------------------------------------------------------------------------------

// ref_tid[r] = the transcript that reference r names, kSamNone when none does
__global__ void k_bam_refs(const unsigned char* __restrict__ ref_blob, const uint64_t* __restrict__ ref_off, uint32_t n_ref, NameTable T,
                           uint32_t* __restrict__ ref_tid, uint32_t* __restrict__ flag) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_ref) return;
    if (ref_off[r + 1] < ref_off[r] || ref_off[r + 1] - ref_off[r] > 0xfffffffeull) { atomicOr(flag, 2u); ref_tid[r] = kSamNone; return; }
    ref_tid[r] = T.find(ref_blob + ref_off[r], (uint32_t)(ref_off[r + 1] - ref_off[r]));
}

// head[k] = record k's name differs from record k - 1's
__global__ void k_bam_heads(const unsigned char* __restrict__ bytes, uint32_t K, const uint32_t* __restrict__ rec_off, const uint32_t* __restrict__ name_len,
                            uint32_t* __restrict__ head) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    if (k == 0) { head[0] = 1; return; }
    const uint32_t n = name_len[k], a = rec_off[k] + kBamMin, b = rec_off[k - 1] + kBamMin;
    bool same = name_len[k - 1] == n;
    for (uint32_t i = 0; same && i < n; ++i) same = bytes[a + i] == bytes[b + i];
    head[k] = same ? 0u : 1u;
}

// the last head: cut[0] = its record, cut[1] = where that record begins
__global__ void k_bam_cut(uint32_t K, const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_scan, const uint32_t* __restrict__ rec_off,
                          uint32_t* __restrict__ cut) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K || !head[k] || head_scan[k] + 1 != head_scan[K]) return;
    cut[0] = k; cut[1] = rec_off[k];
}

struct Scratch : Chain {
    DevBuf<uint4> text;
    DevBuf<uint32_t> info, tid, name_len, rec_line, head, head_scan, pair_head, has_pair, surv, surv_scan, val, val2, cut;
    DevBuf<int32_t> pos;
    DevBuf<uint64_t> key, key2;
    DevBuf<unsigned long long> word;              // [0] the lowest malformed record, [1] the pairs
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;


namespace {

// The text on the device: bytes[0, n) in a buffer of whole 16-byte groups.  h: 8 pinned 64-bit words.
int parse_device_text(sfgpu_bam* m, Scratch& S, const unsigned char* bytes, uint64_t n, bool final, sfgpu_hit* d_hits, uint64_t cap_hits, uint32_t* d_off,
                      uint64_t cap_reads, sfgpu_sam_result* res, hipStream_t st, uint64_t* h) {
    uint32_t* h32 = reinterpret_cast<uint32_t*>(h);
    const uint64_t skip = m->header_bytes > m->stream_pos ? m->header_bytes - m->stream_pos : 0;
    if (skip > n) {                                       // the header goes on: present more
        if (final) { res->consumed = n; m->stream_pos += n; }
        return SFGPU_OK;
    }
    uint32_t K = 0, last = 0;
    if (int r = resolve_chain(S, bytes, (uint32_t)skip, (uint32_t)n, &K, &last, st, h32)) return r;
    const bool chain_bad = bam_ended(last) && (bam_broken(last) || final);     // BAD_FIELDS at record K

    // ---- the records
    if (int r = S.word.reserve(2, st, false)) return r;
    if (int r = S.cut.reserve(4, st, false)) return r;
    for (DevBuf<uint32_t>* b : {&S.info, &S.tid, &S.name_len, &S.rec_line, &S.head, &S.head_scan, &S.pair_head, &S.has_pair, &S.surv, &S.surv_scan})
        if (int r = b->reserve((uint64_t)K + 2, st, false)) return r;
    if (int r = S.pos.reserve((uint64_t)K + 2, st, false)) return r;
    h[1] = kNoBad;
    if (K) {
        SF_HIP(hipMemsetAsync(S.word.p, 0xff, 8, st));
        SF_HIP(hipMemsetAsync(S.word.p + 1, 0, 8, st));
        hipLaunchKernelGGL(k_bam_records, dim3(grid_of(K)), dim3(kBlock), 0, st, bytes, K, S.rec_off.p, m->names->paired ? 1 : 0, m->n_ref, m->ref_tid.p,
                           S.info.p, S.tid.p, S.pos.p, S.name_len.p, S.rec_line.p, S.word.p);
        SF_CHECK_LAUNCH();
        SF_HIP(hipMemcpyAsync(&h[1], S.word.p, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
    }
    if (h[1] != kNoBad || chain_bad) {
        res->bad = h[1] != kNoBad ? (uint32_t)(h[1] & 0xffu) : (uint32_t)SFGPU_SAM_BAD_FIELDS;
        res->bad_line = h[1] != kNoBad ? h[1] >> 8 : K;
        set_error("sfgpu_bam_parse: record %llu of the text is malformed (SFGPU_SAM_BAD_* %u)", (unsigned long long)res->bad_line, res->bad);
        return SFGPU_ERR_FORMAT;
    }
    if (K == 0) {
        if (final) { res->consumed = n; m->stream_pos += n; }
        return SFGPU_OK;
    }

    // ---- the groups
    hipLaunchKernelGGL(k_bam_heads, dim3(grid_of(K)), dim3(kBlock), 0, st, bytes, K, S.rec_off.p, S.name_len.p, S.head.p);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(S.head.p, S.head_scan.p, K, st)) return r;
    hipLaunchKernelGGL(k_bam_cut, dim3(grid_of(K)), dim3(kBlock), 0, st, K, S.head.p, S.head_scan.p, S.rec_off.p, S.cut.p);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(&h32[0], S.head_scan.p + K, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h32[1], S.cut.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t n_groups_seen = h32[0];
    const uint32_t Kc = final ? K : h32[1], n_reads = final ? n_groups_seen : n_groups_seen - 1;
    const uint64_t consumed = final ? n : h32[2];
    if (n_reads == 0) return SFGPU_OK;                    // one group, held back: present more

    // ---- the records of the groups: samback.h
    const Lines lines{S.info.p, S.tid.p, S.pos.p};
    SF_HIP(hipMemsetAsync(S.has_pair.p, 0, (uint64_t)n_reads * 4, st));
    if (m->names->paired) {
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
        set_error("sfgpu_bam_parse: %u records in %u reads do not fit cap_hits = %llu, cap_reads = %llu", n_hits, n_reads,
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
    res->n_lines = Kc; res->n_reads = n_reads; res->n_hits = n_hits; res->n_pairs = h[1];
    res->consumed = consumed;
    m->stream_pos += consumed;
    return SFGPU_OK;
}

int check_parse_args(const char* who, sfgpu_bam* m, const void* text, uint64_t n_bytes, sfgpu_hit* d_hits, uint64_t cap_hits, uint32_t* d_off,
                     sfgpu_sam_result* res) {
    if (!m || !res) { set_error("%s: null handle or result", who); return SFGPU_ERR_INVALID; }
    memset(res, 0, sizeof(*res));
    if (n_bytes > kMaxBytes) { set_error("%s: more than 2^30 bytes in one call", who); return SFGPU_ERR_RANGE; }
    if ((n_bytes && !text) || !d_off || (cap_hits && !d_hits)) { set_error("%s: null array", who); return SFGPU_ERR_INVALID; }
    return SFGPU_OK;
}

}  // namespace

extern "C" int sfgpu_bam_close(sfgpu_bam* m) {
    if (!m) return SFGPU_OK;
    (void)sfgpu_sam_close(m->names);                      // (synchronises the device)
    delete m;
    return SFGPU_OK;
}

extern "C" int sfgpu_bam_open(sfgpu_bam** out, const char* d_names, const uint64_t* d_name_off, uint64_t M, const char* d_ref_names,
                              const uint64_t* d_ref_off, uint64_t n_ref, uint64_t header_bytes, int paired, sfgpu_stream stream) {
    SF_REQUIRE(out && d_ref_off, SFGPU_ERR_INVALID, "sfgpu_bam_open: null handle or reference offsets");
    SF_REQUIRE(n_ref < 0x7fffffffull, SFGPU_ERR_RANGE, "sfgpu_bam_open: 2^31 - 1 references or more");
    hipStream_t st = as_stream(stream);
    sfgpu_bam* m = new sfgpu_bam;
    m->n_ref = (uint32_t)n_ref;
    m->header_bytes = header_bytes;
    DevBuf<uint32_t> flag;
    auto build = [&]() -> int {
        if (int r = sfgpu_sam_open(&m->names, d_names, d_name_off, M, paired, stream)) return r;
        CallScope scope;
        uint32_t* h32 = nullptr;
        SF_HIP(scope.adopt(st));
        SF_HIP(scope.pinned_block(&h32, 4 * sizeof(uint32_t)));
        if (int r = m->ref_tid.reserve(n_ref + 1, st, false)) return r;
        if (int r = flag.reserve(1, st, false)) return r;
        SF_HIP(hipMemsetAsync(flag.p, 0, 4, st));
        if (n_ref) {
            SF_REQUIRE(d_ref_names != nullptr, SFGPU_ERR_INVALID, "sfgpu_bam_open: null reference names");
            const NameTable T{m->names->blob.p, m->names->off.p, m->names->slot.p, m->names->mask};
            hipLaunchKernelGGL(k_bam_refs, dim3(grid_of(n_ref)), dim3(kBlock), 0, st, reinterpret_cast<const unsigned char*>(d_ref_names), d_ref_off,
                               (uint32_t)n_ref, T, m->ref_tid.p, flag.p);
            SF_CHECK_LAUNCH();
        }
        SF_HIP(hipMemcpyAsync(h32, flag.p, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        SF_REQUIRE(!(h32[0] & 2u), SFGPU_ERR_INVALID, "sfgpu_bam_open: the reference offsets decrease");
        return SFGPU_OK;
    };
    const int rc = build();
    if (rc != SFGPU_OK) { (void)hipStreamSynchronize(st); (void)sfgpu_bam_close(m); return rc; }
    *out = m;
    return SFGPU_OK;
}

extern "C" int sfgpu_bam_parse_host(sfgpu_bam* m, const char* h_text, uint64_t n_bytes, int final, sfgpu_hit* d_hits, uint64_t cap_hits,
                                    uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream) {
    if (int r = check_parse_args("sfgpu_bam_parse_host", m, h_text, n_bytes, d_hits, cap_hits, d_off, res)) return r;
    hipStream_t st = as_stream(stream);
    SF_HIP(hipMemsetAsync(d_off, 0, 4, st));
    if (n_bytes == 0) { SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }

    Scratch S;
    CallScope scope;        // after S: it drains both streams before S's blocks go back to the pool
    HostStage H;
    if (int r = stage_host_text(scope, H, S.text, h_text, n_bytes, false, st)) return r;
    const int rc = parse_device_text(m, S, reinterpret_cast<const unsigned char*>(S.text.p), n_bytes, final != 0, d_hits, cap_hits, d_off, cap_reads, res, st, H.h);
    SF_HIP(hipEventRecord(H.ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_copy, H.ev_c0, H.ev_c1);
    add_elapsed(&res->ms_kernels, H.ev_k0, H.ev_k1);
    return rc;
}

extern "C" int sfgpu_bam_parse_device(sfgpu_bam* m, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final, sfgpu_hit* d_hits,
                                      uint64_t cap_hits, uint32_t* d_off, uint64_t cap_reads, sfgpu_sam_result* res, sfgpu_stream stream) {
    if (int r = check_parse_args("sfgpu_bam_parse_device", m, d_text, n_bytes, d_hits, cap_hits, d_off, res)) return r;
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_bam_parse_device: d_text must be 16-byte aligned");
    SF_REQUIRE(n_bytes == 0 || cap_text >= ((n_bytes + 1 + 15) & ~15ull) + 16, SFGPU_ERR_INVALID,
               "sfgpu_bam_parse_device: cap_text must hold the text, one byte more, the rest of that 16-byte group and one group more");
    hipStream_t st = as_stream(stream);
    SF_HIP(hipMemsetAsync(d_off, 0, 4, st));
    if (n_bytes == 0) { SF_HIP(hipStreamSynchronize(st)); return SFGPU_OK; }
    Scratch S;
    CallScope scope;        // after the scratch, as in sfgpu_bam_parse_host
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;
    uint64_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_k0));
    SF_HIP(scope.event(&ev_k1));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint64_t)));
    SF_HIP(hipEventRecord(ev_k0, st));
    const int rc = parse_device_text(m, S, d_text, n_bytes, final != 0, d_hits, cap_hits, d_off, cap_reads, res, st, h);
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_kernels, ev_k0, ev_k1);
    return rc;
}
