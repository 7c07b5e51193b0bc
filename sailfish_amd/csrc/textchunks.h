// textchunks.h -- what the device text writers (eqtext_write.hip: eq_classes.txt, quant_write.hip: quant.sf) share behind their
// sizing passes: the longest line, the greedy chunk plan, and the two-buffer format -> copy -> sink loop.  A writer has the
// 64-bit byte start of every line on the device (line_start[n_lines] = the total) and a step "format tiles [a, b] of the text
// into this buffer"; tiles are kTileBytes of the OUTPUT, aligned in the text's byte offsets, and a chunk's buffer starts at the
// tile that holds its first byte.  Chunk c + 1 is formatted and copied to its pinned buffer while the sink consumes chunk c.
// deliver_device is the second consumer: the chunk's bytes stay on the device and go to a function (the BGZF encoder of
// samtext_write.hip's compressed formats) while chunk c + 1 is formatted.
#pragma once
#include "common.h"

namespace sfgpu {
namespace textchunks {

constexpr int kBlock = 256;
constexpr uint32_t kTileBytes = 4096;                     // kBlock lanes x one 16-byte store
constexpr int kTileShift = 12;
constexpr uint64_t kDefaultChunk = 32ull << 20;           // the reader's limits (eqtext.hip)
constexpr uint64_t kMaxChunk = 1ull << 30;

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// a fixed grid strides over the lines: one atomic per wavefront of a few thousand, not of every 64 lines (they serialise on the address)
constexpr unsigned kLineMaxBlocks = 1024;
static __global__ void k_line_max(const uint64_t* __restrict__ line_start, uint64_t n_lines, unsigned long long* __restrict__ longest) {
    unsigned long long len = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_lines; c += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long l = line_start[c + 1] - line_start[c];
        len = l > len ? l : len;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(len, o);
        len = other > len ? other : len;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) atomicMax(longest, len);
}

// greedy chunks, one thread: chunk i holds lines [plan[2 i - 2], plan[2 i]) and ends at byte plan[2 i + 1].  Every line fits
// a chunk (checked by the host before the launch), so every chunk takes at least one line; *n_planned = number of chunks.
static __global__ void k_chunk_plan(const uint64_t* __restrict__ line_start, uint64_t n_lines, uint64_t chunk_bytes, uint64_t cap,
                                    uint64_t* __restrict__ plan, unsigned long long* __restrict__ n_planned) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t c = 0, n = 0;
    while (c < n_lines && n < cap) {
        const uint64_t limit = line_start[c] + chunk_bytes;
        uint64_t lo = c + 1, hi = n_lines + 1;            // line_start[lo] <= limit < line_start[hi] (line_start[n_lines + 1] = infinity)
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (line_start[mid] <= limit) lo = mid; else hi = mid;
        }
        plan[2 * n] = lo; plan[2 * n + 1] = line_start[lo];
        ++n;
        c = lo;
    }
    *n_planned = n;
}

// *d_longest (zeroed by the caller) = the longest line, on st
inline int line_max(const uint64_t* d_line_start, uint64_t n_lines, unsigned long long* d_longest, hipStream_t st) {
    hipLaunchKernelGGL(k_line_max, dim3(grid_of(n_lines) < kLineMaxBlocks ? grid_of(n_lines) : kLineMaxBlocks), dim3(kBlock), 0, st,
                       d_line_start, n_lines, d_longest);
    SF_HIP(hipGetLastError());
    return SFGPU_OK;
}

struct Stats {                             // added to, never reset: the caller's sizing pass has counted into format_ms already
    uint64_t n_chunks = 0;
    double format_ms = 0.0, d2h_ms = 0.0, sink_ms = 0.0;
};

// everything the loop owns; the scope comes last, so that it is destroyed first and both streams have drained before a block
// goes back (a copy may still write the pinned buffers)
struct Pipe {
    DevBuf<uint64_t> plan;
    DevBuf<unsigned long long> n;
    DevBuf<uint4> out[2];
    CallScope scope;
};

// The chunk plan of a text of `total` bytes in n_lines lines (every line at most chunk_bytes long: the caller has checked), on st:
// *h_plan (pinned, the scope's) holds per chunk its line end and its byte end.  Two consecutive greedy chunks hold more than
// chunk_bytes together, which bounds their number.
inline int plan_chunks(const char* who, Pipe& P, const uint64_t* d_line_start, uint64_t n_lines, uint64_t total, uint64_t chunk_bytes,
                       hipStream_t st, Stats* stats, uint64_t** h_plan_out, uint64_t* n_chunks_out) {
    hipEvent_t ev_p[2] = {nullptr, nullptr};
    uint64_t* h_plan = nullptr;
    unsigned long long* h_n = nullptr;
    for (auto& e : ev_p) SF_HIP(P.scope.event(&e));
    SF_HIP(P.scope.pinned_block(&h_n, sizeof(unsigned long long)));
    const uint64_t plan_cap = 2 * (total / chunk_bytes) + 2;
    if (int rc = P.plan.reserve(2 * plan_cap, st, false)) return rc;
    if (int rc = P.n.reserve(1, st, false)) return rc;
    SF_HIP(P.scope.pinned_block(&h_plan, 2 * plan_cap * sizeof(uint64_t)));
    SF_HIP(hipEventRecord(ev_p[0], st));
    hipLaunchKernelGGL(k_chunk_plan, dim3(1), dim3(kWave), 0, st, d_line_start, n_lines, chunk_bytes, plan_cap, P.plan.p, P.n.p);
    SF_HIP(hipGetLastError());
    SF_HIP(hipEventRecord(ev_p[1], st));
    SF_HIP(hipMemcpyAsync(h_n, P.n.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint64_t n_chunks = *h_n;
    SF_HIP(hipMemcpyAsync(h_plan, P.plan.p, 2 * n_chunks * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&stats->format_ms, ev_p[0], ev_p[1]);
    if (n_chunks == 0 || h_plan[2 * n_chunks - 2] != n_lines || h_plan[2 * n_chunks - 1] != total) {
        set_error("%s: the chunk plan does not cover the table", who);
        return SFGPU_ERR_HIP;
    }
    *h_plan_out = h_plan; *n_chunks_out = n_chunks;
    return SFGPU_OK;
}

// Plans the chunks of a text of `total` bytes in n_lines lines (every line at most chunk_bytes long: the caller has checked) and
// hands them to `sink` in order.  format_tiles(first_tile, last_tile, out_base, out, st) enqueues on st the kernels that write
// tiles first_tile .. last_tile into `out`, whose byte 0 is text byte out_base = first_tile * kTileBytes, and returns a status.
// `who` names the entry point in error messages.  st is the caller's stream (the sizing pass ran on it); it is drained on return.
template <typename FormatTiles>
int deliver(const char* who, const uint64_t* d_line_start, uint64_t n_lines, uint64_t total, uint64_t chunk_bytes, sfgpu_text_sink sink,
            void* user, hipStream_t st, Stats* stats, FormatTiles format_tiles) {
    Pipe P;
    hipStream_t cs = nullptr;
    char* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev_f0[2] = {nullptr, nullptr}, ev_f1[2] = {nullptr, nullptr}, ev_c0[2] = {nullptr, nullptr}, ev_c1[2] = {nullptr, nullptr};
    uint64_t* h_plan = nullptr;
    uint64_t n_chunks = 0;
    SF_HIP(P.scope.adopt(st));
    SF_HIP(P.scope.acquire(&cs));
    if (int rc = plan_chunks(who, P, d_line_start, n_lines, total, chunk_bytes, st, stats, &h_plan, &n_chunks)) return rc;

    // ---- format + copy + sink, two buffers: chunk i + 1 is formatted and copied while the sink holds chunk i
    const uint64_t stage_bytes = total < chunk_bytes ? total : chunk_bytes;
    const uint64_t out_groups = (stage_bytes + 2 * kTileBytes) / 16 + 1;
    for (int b = 0; b < 2 && (uint64_t)b < n_chunks; ++b) {
        SF_HIP(P.scope.pinned_block(&pinned[b], stage_bytes));
        if (int rc = P.out[b].reserve(out_groups, st, false)) return rc;
        for (hipEvent_t* e : {&ev_f0[b], &ev_f1[b], &ev_c0[b], &ev_c1[b]}) SF_HIP(P.scope.event(e));
    }
    auto chunk_begin = [&](uint64_t i) -> uint64_t { return i ? h_plan[2 * i - 1] : 0; };
    // format on st into out[slot], then the copy on cs into pinned[slot]; the slot's previous chunk has left the sink, and
    // its copy (which read out[slot]) was waited for before that
    auto enqueue = [&](uint64_t i) -> int {
        const int slot = (int)(i & 1);
        const uint64_t b0 = chunk_begin(i), b1 = h_plan[2 * i + 1];
        const uint64_t first_tile = b0 >> kTileShift, last_tile = (b1 - 1) >> kTileShift, out_base = first_tile << kTileShift;
        SF_HIP(hipEventRecord(ev_f0[slot], st));
        if (int rc = format_tiles(first_tile, last_tile, out_base, P.out[slot].p, st)) return rc;
        SF_HIP(hipEventRecord(ev_f1[slot], st));
        SF_HIP(hipStreamWaitEvent(cs, ev_f1[slot], 0));
        SF_HIP(hipEventRecord(ev_c0[slot], cs));
        SF_HIP(hipMemcpyAsync(pinned[slot], reinterpret_cast<const char*>(P.out[slot].p) + (b0 - out_base), b1 - b0, hipMemcpyDeviceToHost, cs));
        SF_HIP(hipEventRecord(ev_c1[slot], cs));
        return SFGPU_OK;
    };
    if (int rc = enqueue(0)) return rc;
    for (uint64_t i = 0; i < n_chunks; ++i) {
        const int slot = (int)(i & 1);
        if (i + 1 < n_chunks) if (int rc = enqueue(i + 1)) return rc;
        SF_HIP(hipEventSynchronize(ev_c1[slot]));
        add_elapsed(&stats->format_ms, ev_f0[slot], ev_f1[slot]);
        add_elapsed(&stats->d2h_ms, ev_c0[slot], ev_c1[slot]);
        const auto t0 = std::chrono::steady_clock::now();
        const int stop = sink(pinned[slot], h_plan[2 * i + 1] - chunk_begin(i), user);
        stats->sink_ms += ms_since(t0);
        stats->n_chunks++;
        if (stop) {
            set_error("%s: the sink refused a chunk", who);
            return SFGPU_ERR_IO;
        }
    }
    return SFGPU_OK;
}

// The same plan and the same tiles, but the chunk stays on the device: consume(d_bytes, n_bytes, ready) is called per chunk in
// order with a stream `ready` behind which the chunk's bytes are complete; it returns a status when it is done with the bytes
// (synchronous, as a sink is).  Chunk i + 1 is formatted on st meanwhile.
template <typename Consume, typename FormatTiles>
int deliver_device(const char* who, const uint64_t* d_line_start, uint64_t n_lines, uint64_t total, uint64_t chunk_bytes, hipStream_t st,
                   Stats* stats, Consume consume, FormatTiles format_tiles) {
    Pipe P;
    hipStream_t ready = nullptr;
    hipEvent_t ev_f0[2] = {nullptr, nullptr}, ev_f1[2] = {nullptr, nullptr};
    uint64_t* h_plan = nullptr;
    uint64_t n_chunks = 0;
    SF_HIP(P.scope.adopt(st));
    SF_HIP(P.scope.acquire(&ready));
    if (int rc = plan_chunks(who, P, d_line_start, n_lines, total, chunk_bytes, st, stats, &h_plan, &n_chunks)) return rc;
    const uint64_t stage_bytes = total < chunk_bytes ? total : chunk_bytes;
    const uint64_t out_groups = (stage_bytes + 2 * kTileBytes) / 16 + 1;
    for (int b = 0; b < 2 && (uint64_t)b < n_chunks; ++b) {
        if (int rc = P.out[b].reserve(out_groups, st, false)) return rc;
        for (hipEvent_t* e : {&ev_f0[b], &ev_f1[b]}) SF_HIP(P.scope.event(e));
    }
    auto chunk_begin = [&](uint64_t i) -> uint64_t { return i ? h_plan[2 * i - 1] : 0; };
    auto out_base = [&](uint64_t i) -> uint64_t { return (chunk_begin(i) >> kTileShift) << kTileShift; };
    // format on st into out[slot]: the slot's previous chunk has been consumed
    auto enqueue = [&](uint64_t i) -> int {
        const int slot = (int)(i & 1);
        const uint64_t b0 = chunk_begin(i), b1 = h_plan[2 * i + 1];
        SF_HIP(hipEventRecord(ev_f0[slot], st));
        if (int rc = format_tiles(b0 >> kTileShift, (b1 - 1) >> kTileShift, out_base(i), P.out[slot].p, st)) return rc;
        SF_HIP(hipEventRecord(ev_f1[slot], st));
        return SFGPU_OK;
    };
    if (int rc = enqueue(0)) return rc;
    for (uint64_t i = 0; i < n_chunks; ++i) {
        const int slot = (int)(i & 1);
        SF_HIP(hipStreamWaitEvent(ready, ev_f1[slot], 0));      // before chunk i + 1 is queued: the consumer waits for chunk i alone
        if (i + 1 < n_chunks) if (int rc = enqueue(i + 1)) return rc;
        const uint64_t b0 = chunk_begin(i);
        const int rc = consume(reinterpret_cast<const uint8_t*>(P.out[slot].p) + (b0 - out_base(i)), h_plan[2 * i + 1] - b0, ready);
        if (rc != SFGPU_OK) return rc;                          // (a consumer that failed may not have waited for the chunk)
        SF_HIP(hipEventSynchronize(ev_f1[slot]));               // the consumer has waited behind it: this returns at once
        add_elapsed(&stats->format_ms, ev_f0[slot], ev_f1[slot]);
        stats->n_chunks++;
    }
    return SFGPU_OK;
}

}  // namespace textchunks
}  // namespace sfgpu
