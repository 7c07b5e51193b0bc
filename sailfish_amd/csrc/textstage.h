// textstage.h -- a host text on its way to the device for the calls that look at it whole (sfgpu_sam_parse_host, sfgpu_bam_parse_host,
// sfgpu_sam_collect_host, sfgpu_bam_collect_host): two pinned buffers, sub-chunks of kStageBytes on a copy stream of the call's
// own, the compute stream made to wait for the last of them.
#pragma once
#include <cstring>

#include "common.h"

namespace sfgpu {

constexpr uint64_t kStageBytes = 4ull << 20;             // staged sub-chunk (a multiple of 16)

struct HostStage {
    hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;      // around the copies; around the caller's kernels
    uint64_t* h = nullptr;                               // 8 pinned 64-bit words for the caller
};

// h_text[0, used), a '\n' behind it when `append`, zeros up to the end of its last 16-byte group -> text (reserved here: whole groups
// and one more).  Returns with st waiting for the last copy and ev_k0 recorded on it; the caller records ev_k1 behind its kernels.
// `scope` (declared behind the caller's scratch) owns the streams, events and pinned blocks.
inline int stage_host_text(CallScope& scope, HostStage& H, DevBuf<uint4>& text, const char* h_text, uint64_t used, bool append, hipStream_t st) {
    const uint64_t n_text = used + (append ? 1 : 0), n_groups = (n_text + 15) / 16, n_sub = (used + kStageBytes - 1) / kStageBytes;
    hipStream_t cs = nullptr;
    char* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev_slot[2] = {nullptr, nullptr};
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.acquire(&cs));
    for (int b = 0; b < 2 && (uint64_t)b < n_sub; ++b) {
        SF_HIP(scope.pinned_block(&pinned[b], (used < kStageBytes ? used : kStageBytes) + 48));
        SF_HIP(scope.event(&ev_slot[b]));
    }
    for (hipEvent_t* e : {&H.ev_c0, &H.ev_c1, &H.ev_k0, &H.ev_k1}) SF_HIP(scope.event(e));
    SF_HIP(scope.pinned_block(&H.h, 8 * sizeof(uint64_t)));
    if (int r = text.reserve(n_groups + 1, st, false)) return r;
    SF_HIP(hipEventRecord(H.ev_k0, st));
    SF_HIP(hipStreamWaitEvent(cs, H.ev_k0, 0));              // the copies stay behind whatever `stream` held and behind the reservation
    SF_HIP(hipEventRecord(H.ev_c0, cs));
    for (uint64_t c = 0; c < n_sub; ++c) {
        const int slot = (int)(c & 1);
        if (c >= 2) SF_HIP(hipEventSynchronize(ev_slot[slot]));      // its previous copy has left the pinned buffer
        const uint64_t p = c * kStageBytes, q = (c + 1 == n_sub) ? used : p + kStageBytes;
        uint64_t n = q - p;
        memcpy(pinned[slot], h_text + p, n);
        if (c + 1 == n_sub) {
            if (append) pinned[slot][n++] = '\n';
            const uint64_t padded = (n + 15) & ~15ull;
            memset(pinned[slot] + n, 0, padded - n);
            n = padded;
        }
        SF_HIP(hipMemcpyAsync(reinterpret_cast<char*>(text.p) + p, pinned[slot], n, hipMemcpyHostToDevice, cs));
        SF_HIP(hipEventRecord(ev_slot[slot], cs));
    }
    SF_HIP(hipEventRecord(H.ev_c1, cs));
    SF_HIP(hipStreamWaitEvent(st, H.ev_c1, 0));
    SF_HIP(hipEventRecord(H.ev_k0, st));
    return SFGPU_OK;
}

}  // namespace sfgpu
