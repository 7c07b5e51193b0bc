// slotpipe.h -- the one host driver of the device writers whose kernel turns fixed units of input into byte strings of varying
// length (gzwrite.hip: 64 KB gzip blocks; bgzf_write.hip: 32 KB BGZF members).  On the compute stream `st` a batch of units is
// encoded into slots, the lengths are scanned and k_slot_compact moves the slots into out[batch & 1]; on the copy stream `cs` its
// bytes go through two pinned buffers in pieces of <= chunk_bytes to the sink.  The order that must hold: a batch is enqueued
// only when every copy out of its out[] buffer has been waited for and the sizes of the batch before have been read; piece p + 1
// is queued into the other pinned buffer before piece p is waited for; a failed write drains both streams and ends the file.
#pragma once
#include "common.h"
#include "primitives.h"
#include "slotcompact.h"

namespace sfgpu {

struct SlotPipe {
    sfgpu_text_sink sink_fn = nullptr;
    void* user = nullptr;
    uint64_t chunk_bytes = 0;
    bool broken = false;                                // a write failed: the file cannot be continued
    uint64_t n_bytes_in = 0, n_bytes_out = 0, n_chunks = 0;
    double encode_ms = 0, d2h_ms = 0, sink_ms = 0;
    hipStream_t st = nullptr, cs = nullptr;
    hipEvent_t ev_in = nullptr, ev_e0 = nullptr, ev_e1 = nullptr, ev_c0[2] = {nullptr, nullptr}, ev_c1[2] = {nullptr, nullptr};
    char* pinned[2] = {nullptr, nullptr};
    uint64_t pinned_cap = 0;
    uint64_t* h_total = nullptr;                        // bytes of the batch just encoded
    DevBuf<uint4> slots;
    DevBuf<uint32_t> len;
    DevBuf<uint64_t> off;
    DevBuf<uint8_t> out[2];
    CallScope scope;                                    // last, so that it drains before the DevBufs go
    ~SlotPipe() {
        scope.drain();
        for (char* p : pinned) if (p) pinned_free(p);   // the staging buffers grow between writes: not the scope's
    }

    // `who`: the entry, for the messages.  chunk 0 = the default
    int open(const char* who, sfgpu_text_sink sink, void* sink_user, uint64_t chunk) {
        if (!sink) { set_error("%s: null sink", who); return SFGPU_ERR_INVALID; }
        sink_fn = sink; user = sink_user; chunk_bytes = chunk ? chunk : 32ull << 20;
        if (chunk_bytes < 16 || chunk_bytes > 1ull << 30) { set_error("%s: chunk_bytes must lie in [16, 2^30] (0 = default)", who); return SFGPU_ERR_INVALID; }
        SF_HIP(scope.acquire(&st));
        SF_HIP(scope.acquire(&cs));
        SF_HIP(scope.event(&ev_in, hipEventDisableTiming));
        for (hipEvent_t* e : {&ev_e0, &ev_e1, &ev_c0[0], &ev_c1[0], &ev_c0[1], &ev_c1[1]}) SF_HIP(scope.event(e));
        SF_HIP(scope.pinned_block(&h_total, sizeof(uint64_t)));
        return SFGPU_OK;
    }

    int sink(const char* bytes, uint64_t n, const char* who) {
        const auto t0 = std::chrono::steady_clock::now();
        const int stop = sink_fn(bytes, n, user);
        sink_ms += ms_since(t0);
        n_chunks++;
        if (stop) {
            broken = true;
            set_error("%s: the sink refused a chunk", who);
            return SFGPU_ERR_IO;
        }
        n_bytes_out += n;
        return SFGPU_OK;
    }

    // *r = the writer's own counters `own` and the ones every result struct carries
    template <typename Result>
    void report(Result* r, const Result& own) const {
        *r = own;
        r->n_bytes_in = n_bytes_in; r->n_bytes_out = n_bytes_out; r->n_chunks = n_chunks;
        r->encode_ms = encode_ms; r->d2h_ms = d2h_ms; r->sink_ms = sink_ms;
    }

    // n_bytes > 0 at d_src, behind whatever the caller has queued on `stream`, through the sink, on behalf of the entry `who`.
    //   launch_encode(src, bytes, n_units, slots, len)   the encode kernel on st: unit u of the batch into slot u, its bytes into len[u]
    //   queue_meta_copies(n_units)                       the writer's own device-to-host copies on st, behind the batch; returns a status
    //   after_batch(first_unit, n_units)                 on the host, when those copies have arrived and before the next batch is enqueued
    // Any failure leaves the pipe broken and drained: nothing may stay in flight behind a failed write.
    template <uint32_t kUnitBytes, uint32_t kSlotBytes, uint32_t kBatchUnits, typename Launch, typename MetaCopies, typename AfterBatch>
    int write(const uint8_t* d_src, uint64_t n_bytes, sfgpu_stream stream, const char* who, Launch launch_encode, MetaCopies queue_meta_copies,
              AfterBatch after_batch) {
        struct Guard { SlotPipe* p; bool ok; ~Guard() { if (!ok) { p->broken = true; p->scope.drain(); } } } guard{this, false};
        static_assert(kSlotBytes % 16 == 0, "slots are stored 16 bytes at a time");
        SF_HIP(hipEventRecord(ev_in, as_stream(stream)));          // behind whatever the caller has queued on `stream`
        SF_HIP(hipStreamWaitEvent(st, ev_in, 0));
        const uint64_t n_units = (n_bytes + kUnitBytes - 1) / kUnitBytes;
        const uint64_t n_batches = (n_units + kBatchUnits - 1) / kBatchUnits;
        const uint64_t max_nu = n_units < kBatchUnits ? n_units : kBatchUnits;
        // staging: as large as a piece of this write can get, at most chunk_bytes (nothing is in flight between writes)
        const uint64_t stage = chunk_bytes < max_nu * kSlotBytes ? chunk_bytes : max_nu * kSlotBytes;
        if (stage > pinned_cap) {
            for (int b = 0; b < 2; ++b) {
                if (pinned[b]) { pinned_free(pinned[b]); pinned[b] = nullptr; }
                pinned_cap = 0;
                SF_HIP(pinned_malloc(&pinned[b], stage));
            }
            pinned_cap = stage;
        }
        if (int rc = slots.reserve(max_nu * (kSlotBytes / 16), st, false)) return rc;
        if (int rc = len.reserve(max_nu + 1, st, false)) return rc;
        if (int rc = off.reserve(max_nu + 1, st, false)) return rc;
        for (int b = 0; b < 2 && (uint64_t)b < n_batches; ++b) if (int rc = out[b].reserve(max_nu * kSlotBytes, st, false)) return rc;

        auto batch_units = [&](uint64_t i) -> uint32_t {
            return (uint32_t)(n_units - i * kBatchUnits < kBatchUnits ? n_units - i * kBatchUnits : kBatchUnits);
        };
        // encode + scan + compact of batch i on st into out[i & 1]; every copy that read this buffer has been waited for, and the
        // sizes of the batch before have been read
        auto enqueue = [&](uint64_t i) -> int {
            const uint32_t nu = batch_units(i);
            const uint64_t b0 = i * kBatchUnits * (uint64_t)kUnitBytes;
            const uint64_t bytes = n_bytes - b0 < (uint64_t)nu * kUnitBytes ? n_bytes - b0 : (uint64_t)nu * kUnitBytes;
            SF_HIP(hipEventRecord(ev_e0, st));
            launch_encode(d_src + b0, bytes, nu, slots.p, len.p);
            SF_HIP(hipGetLastError());
            if (int rc = exclusive_scan_u32(len.p, off.p, nu, st, false)) return rc;
            hipLaunchKernelGGL(k_slot_compact<kSlotBytes>, dim3(nu), dim3(256), 0, st, reinterpret_cast<const uint8_t*>(slots.p), off.p, out[i & 1].p);
            SF_HIP(hipGetLastError());
            SF_HIP(hipEventRecord(ev_e1, st));
            SF_HIP(hipMemcpyAsync(h_total, off.p + nu, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            return queue_meta_copies(nu);
        };
        int pb = 0;                                     // pinned buffer of the next piece
        auto copy_piece = [&](int p, const uint8_t* d, uint64_t n) -> int {
            SF_HIP(hipEventRecord(ev_c0[p], cs));
            SF_HIP(hipMemcpyAsync(pinned[p], d, n, hipMemcpyDeviceToHost, cs));
            SF_HIP(hipEventRecord(ev_c1[p], cs));
            return SFGPU_OK;
        };
        if (int rc = enqueue(0)) return rc;
        for (uint64_t i = 0; i < n_batches; ++i) {
            SF_HIP(hipStreamSynchronize(st));           // batch i is encoded, its size and the writer's metadata are here
            add_elapsed(&encode_ms, ev_e0, ev_e1);
            const uint64_t total = *h_total;
            after_batch(i * kBatchUnits, batch_units(i));
            if (i + 1 < n_batches) if (int rc = enqueue(i + 1)) return rc;
            const uint8_t* d_out = out[i & 1].p;
            const uint64_t chunk = pinned_cap < chunk_bytes ? pinned_cap : chunk_bytes;
            if (int rc = copy_piece(pb, d_out, total < chunk ? total : chunk)) return rc;
            for (uint64_t at = 0; at < total;) {
                const uint64_t n = total - at < chunk ? total - at : chunk, next = at + n;
                if (next < total) if (int rc = copy_piece(pb ^ 1, d_out + next, total - next < chunk ? total - next : chunk)) return rc;
                SF_HIP(hipEventSynchronize(ev_c1[pb]));
                add_elapsed(&d2h_ms, ev_c0[pb], ev_c1[pb]);
                if (int rc = sink(pinned[pb], n, who)) return rc;
                at = next; pb ^= 1;
            }
        }
        n_bytes_in += n_bytes;
        guard.ok = true;
        return SFGPU_OK;
    }
};

}  // namespace sfgpu
