// eqtext.hip -- the class section of an eq_classes.txt file (GZipWriter::writeEquivCounts, src/GZipWriter.cpp:51-92) parsed
// on the device and folded into a builder: sfgpu_eq_add_text_host.
//
// The host stages the text through a pinned buffer in chunks that end at a '\n' (the next chunk starts behind it); the copy
// of chunk c + 1 runs while chunk c is parsed and folded.  A chunk is parsed in two passes over 16-byte groups:
//   pass 1  k_text_count: '\n' and '\t' per group -> two exclusive scans (primitives.h) give every group its line and tab
//           index; textlines.h's k_line_ends writes where each line ends.
//   heads   k_text_line_head: one lane per line reads the leading k (the label length) and checks that the line holds
//           exactly k + 2 fields; a scan of the k gives rowptr before a single id is parsed.
//   pass 2  k_text_parse: one lane per group; every field that STARTS in the group is parsed by the lane that owns its
//           first byte and stored at rowptr[line] + field - 1 (ids) or counts[line].  Work is per token, so a label of
//           100 000 ids is as parallel as 100 000 one-id labels.
// The first bad line (atomic min over (line << 8 | kind)) fails the whole chunk before anything is folded.  The fold is
// the builder's weighted upsert (sfgpu_eq_add_weighted_device): equal labels add their counts.
#include "common.h"
#include "primitives.h"
#include "textlines.h"

#include <cstring>

namespace sfgpu {
namespace {

using textlines::grid_of;
constexpr int kTextBlock = textlines::kBlock;
constexpr uint64_t kTextDefaultChunk = 32ull << 20;      // bytes per staged chunk
constexpr uint64_t kTextMaxChunk = 1ull << 30;           // lines and ids of one chunk stay far below the builder's u32 limits
constexpr unsigned long long kNoError = ~0ull;

struct Masks {
    uint32_t nl, tab, digit;
};

__device__ inline Masks group_masks(const uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    Masks m{0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t b = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
        m.nl |= (uint32_t)(b == '\n') << i;
        m.tab |= (uint32_t)(b == '\t') << i;
        m.digit |= (uint32_t)(b - '0' < 10u) << i;
    }
    return m;
}

__device__ inline void report(unsigned long long* err, uint64_t line, int kind) {
    atomicMin(err, ((unsigned long long)line << 8) | (unsigned long long)kind);
}

// tabs before byte p of the chunk
__device__ inline uint32_t tabs_before(const uint4* __restrict__ buf, const uint32_t* __restrict__ tab_scan, uint64_t p) {
    const Masks m = group_masks(buf[p >> 4]);
    return tab_scan[p >> 4] + __popc(m.tab & ((1u << (p & 15)) - 1u));
}

__global__ void k_text_count(const uint4* __restrict__ buf, uint64_t n_groups, uint32_t* __restrict__ nl_cnt,
                             uint32_t* __restrict__ tab_cnt) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const Masks m = group_masks(buf[g]);       // (the zero bytes behind the chunk count as neither)
    nl_cnt[g] = __popc(m.nl);
    tab_cnt[g] = __popc(m.tab);
}

// one lane per line: k, the field count, and the tab index the line starts at
__global__ void k_text_line_head(const uint4* __restrict__ buf, uint32_t n_lines, const uint32_t* __restrict__ line_end,
                                 const uint32_t* __restrict__ tab_scan, uint32_t* __restrict__ lens, uint32_t* __restrict__ tab_base,
                                 unsigned long long* __restrict__ err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(buf);
    const uint64_t s = i ? (uint64_t)line_end[i - 1] + 1 : 0, e = line_end[i];
    const uint32_t t0 = tabs_before(buf, tab_scan, s);
    tab_base[i] = t0;
    lens[i] = 0;
    if (e == s) { report(err, i, SFGPU_EQTEXT_EMPTY_FIELD); return; }       // empty line
    uint64_t k = 0, p = s;
    while (p < e && p - s < 11 && bytes[p] - '0' < 10u) k = k * 10 + (bytes[p++] - '0');
    if (p - s > 10) { report(err, i, SFGPU_EQTEXT_BAD_K); return; }
    if (p == s) return;                       // the first field is empty or not a number: k_text_parse reports the byte
    if (p < e && bytes[p] != '\t') return;    // ... likewise a stray byte inside it
    // k ids need >= 2 k bytes ("d\t" each): a larger k cannot be right, and the bound keeps the ids of a chunk below its bytes / 2
    if (k == 0 || k > (e - s) / 2) { report(err, i, SFGPU_EQTEXT_BAD_K); return; }
    const uint32_t tabs = tabs_before(buf, tab_scan, e) - t0;
    if ((uint64_t)tabs != k + 1) { report(err, i, SFGPU_EQTEXT_BAD_K); return; }
    lens[i] = (uint32_t)k;
}

// one 16-byte group: byte classes, empty fields, and every field that starts in the group; returns the sum of the counts it stored
__device__ inline uint64_t parse_group(const uint4* __restrict__ buf, uint64_t g, uint64_t n_bytes, const uint32_t* __restrict__ nl_scan,
                                       const uint32_t* __restrict__ tab_scan, const uint32_t* __restrict__ rowptr,
                                       const uint32_t* __restrict__ tab_base, uint64_t n_transcripts, uint32_t* __restrict__ ids,
                                       uint64_t* __restrict__ counts, unsigned long long* __restrict__ err) {
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(buf);
    const Masks m = group_masks(buf[g]);
    const uint64_t base = g * 16;
    const uint32_t valid = (n_bytes - base >= 16) ? 0xffffu : ((1u << (n_bytes - base)) - 1u);
    const uint32_t sep = m.nl | m.tab;
    const bool prev_sep = g == 0 || bytes[base - 1] == '\n' || bytes[base - 1] == '\t';     // (a virtual '\n' before the chunk)
    const uint32_t after_sep = ((sep << 1) | (prev_sep ? 1u : 0u)) & 0xffffu;
    auto line_of = [&](int i) -> uint32_t { return nl_scan[g] + __popc(m.nl & ((1u << i) - 1u)); };
    const uint32_t bad = valid & ~(sep | m.digit);
    if (bad) { report(err, line_of(__ffs(bad) - 1), SFGPU_EQTEXT_BAD_CHAR); }
    const uint32_t empty = valid & sep & after_sep;                                      // "\t\t", leading / trailing tab, empty line
    if (empty) { report(err, line_of(__ffs(empty) - 1), SFGPU_EQTEXT_EMPTY_FIELD); }
    uint64_t stored = 0;
    uint32_t starts = valid & m.digit & after_sep;
    while (starts) {
        const int i = __ffs(starts) - 1;
        starts &= starts - 1;
        const uint32_t line = line_of(i);
        const uint32_t r0 = rowptr[line], k = rowptr[line + 1] - r0;
        if (k == 0) continue;                                  // a line whose head failed (reported there, or by the byte checks)
        const uint32_t field = tab_scan[g] + __popc(m.tab & ((1u << i) - 1u)) - tab_base[line];
        if (field == 0 || field > k + 1) continue;             // k itself (parsed by the head pass)
        uint64_t p = base + i, v = 0;
        int nd = 0;
        bool over = false;
        for (; p < n_bytes && nd < 21; ++p, ++nd) {            // (every chunk ends in '\n': the walk stops inside it)
            const uint32_t d = bytes[p] - '0';
            if (d >= 10u) break;
            if (v > (~0ull - d) / 10) over = true;
            v = v * 10 + d;
        }
        if (field <= k) {
            if (over || nd > 10 || v >= n_transcripts) { report(err, line, SFGPU_EQTEXT_ID_RANGE); continue; }
            ids[r0 + field - 1] = (uint32_t)v;
        } else {
            if (over || nd > 20) { report(err, line, SFGPU_EQTEXT_COUNT_RANGE); continue; }
            counts[line] = v;
            stored += v;
        }
    }
    return stored;
}

// one lane per 16-byte group; the sum of the counts goes out with one atomic per wavefront (one per line serialised on the address)
__global__ void k_text_parse(const uint4* __restrict__ buf, uint64_t n_bytes, uint64_t n_groups, const uint32_t* __restrict__ nl_scan,
                             const uint32_t* __restrict__ tab_scan, const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ tab_base,
                             uint64_t n_transcripts, uint32_t* __restrict__ ids, uint64_t* __restrict__ counts,
                             unsigned long long* __restrict__ err, unsigned long long* __restrict__ sum) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long local = 0;
    if (g < n_groups) local = parse_group(buf, g, n_bytes, nl_scan, tab_scan, rowptr, tab_base, n_transcripts, ids, counts, err);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) local += __shfl_xor(local, o);
    if ((threadIdx.x & (kWave - 1)) == 0 && local) atomicAdd(sum, local);
}

const char* kind_text(int kind) {
    switch (kind) {
        case SFGPU_EQTEXT_BAD_CHAR: return "a byte that is not a digit, tab or newline";
        case SFGPU_EQTEXT_EMPTY_FIELD: return "an empty line or field";
        case SFGPU_EQTEXT_BAD_K: return "the label length k is 0 or not followed by exactly k ids and a count";
        case SFGPU_EQTEXT_ID_RANGE: return "a transcript id >= the number of transcripts";
        case SFGPU_EQTEXT_COUNT_RANGE: return "a count that does not fit 64 bits";
        case SFGPU_EQTEXT_LONG_LINE: return "a line longer than the chunk size";
        default: return "malformed";
    }
}

// chunk scratch, device side (grow-only)
struct TextScratch {
    DevBuf<uint4> bytes[2];
    DevBuf<uint32_t> nl_cnt, tab_cnt, nl_scan, tab_scan, line_end, lens, rowptr, tab_base, ids;
    DevBuf<uint64_t> counts;
    DevBuf<unsigned long long> misc;        // [0] first error, [1] sum of counts
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

extern "C" int sfgpu_eq_add_text_host(sfgpu_eq* eq, const char* h_text, uint64_t n_bytes, uint64_t n_transcripts,
                                      uint64_t chunk_bytes, sfgpu_eqtext_result* out) {
    SF_REQUIRE(eq && out, SFGPU_ERR_INVALID, "sfgpu_eq_add_text_host: null pointer");
    memset(out, 0, sizeof(*out));
    out->err_line = ~0ull;
    SF_REQUIRE(n_bytes == 0 || h_text, SFGPU_ERR_INVALID, "sfgpu_eq_add_text_host: null text");
    SF_REQUIRE(n_transcripts <= (1ull << 32), SFGPU_ERR_INVALID, "sfgpu_eq_add_text_host: n_transcripts > 2^32");
    if (chunk_bytes == 0) chunk_bytes = kTextDefaultChunk;
    SF_REQUIRE(chunk_bytes >= 16 && chunk_bytes <= kTextMaxChunk, SFGPU_ERR_INVALID,
               "sfgpu_eq_add_text_host: chunk_bytes must lie in [16, 2^30] (0 = default)");
    if (n_bytes == 0) return SFGPU_OK;

    // chunk boundaries: up to chunk_bytes bytes ending in '\n'; the final piece may lack it (a '\n' is appended in staging)
    auto chunk_end = [&](uint64_t pos) -> uint64_t {
        if (n_bytes - pos <= chunk_bytes) return n_bytes;
        const void* nl = memrchr(h_text + pos, '\n', chunk_bytes);
        return nl ? (uint64_t)(static_cast<const char*>(nl) - h_text) + 1 : 0;
    };

    TextScratch S;
    CallScope scope;        // after S: it drains both streams before S's blocks go back to the pool; nothing is released while a copy still reads the pinned buffers
    hipStream_t st = nullptr, cs = nullptr;
    char* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_h2d[2] = {nullptr, nullptr}, ev_p[4] = {nullptr, nullptr, nullptr, nullptr};
    unsigned long long* h_misc = nullptr;
    uint64_t line_base = 0;
    auto fail = [&](int code, uint64_t line, int kind) -> int {
        out->err_line = line; out->err_kind = kind;
        set_error("eq_classes text: class line %llu: %s", (unsigned long long)line, kind_text(kind));
        return code;
    };

    SF_HIP(scope.acquire(&st));
    SF_HIP(scope.acquire(&cs));
    const uint64_t stage_cap = chunk_bytes + 32;
    for (int b = 0; b < 2; ++b) {
        SF_HIP(scope.pinned_block(&pinned[b], stage_cap));
        SF_HIP(scope.event(&ev_copied[b]));
        SF_HIP(scope.event(&ev_h2d[b]));
    }
    for (auto& e : ev_p) SF_HIP(scope.event(&e));
    SF_HIP(scope.pinned_block(&h_misc, 4 * sizeof(unsigned long long)));
    if (int rc = S.misc.reserve(2, st, false)) return rc;

    // host copy into pinned[slot] + its H2D on the copy stream; returns the staged size (a multiple of 16 is read by the kernels)
    uint64_t staged[2] = {0, 0};
    auto stage = [&](uint64_t pos, uint64_t end, int slot) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        uint64_t n = end - pos;
        memcpy(pinned[slot], h_text + pos, n);
        if (h_text[end - 1] != '\n') pinned[slot][n++] = '\n';          // the final line may lack its newline
        const uint64_t padded = (n + 15) & ~15ull;
        memset(pinned[slot] + n, 0, padded + 16 - n);
        out->stage_ms += ms_since(t0);
        if (int rc = S.bytes[slot].reserve(padded / 16 + 1, cs, false)) return rc;
        SF_HIP(hipEventRecord(ev_h2d[slot], cs));
        SF_HIP(hipMemcpyAsync(S.bytes[slot].p, pinned[slot], padded + 16, hipMemcpyHostToDevice, cs));
        SF_HIP(hipEventRecord(ev_copied[slot], cs));
        staged[slot] = n;
        return SFGPU_OK;
    };

    uint64_t pos = 0, end = chunk_end(0);
    int slot = 0;
    if (end == 0) return fail(SFGPU_ERR_RANGE, 0, SFGPU_EQTEXT_LONG_LINE);
    if (int rc = stage(pos, end, slot)) return rc;
    while (pos < n_bytes) {
        const uint64_t n = staged[slot], n_groups = (n + 15) / 16;
        SF_HIP(hipStreamWaitEvent(st, ev_copied[slot], 0));
        for (DevBuf<uint32_t>* b : {&S.nl_cnt, &S.tab_cnt, &S.nl_scan, &S.tab_scan})
            if (int rc = b->reserve(n_groups + 1, st, false)) return rc;
        SF_HIP(hipMemsetAsync(S.misc.p, 0xff, 8, st));
        SF_HIP(hipMemsetAsync(S.misc.p + 1, 0, 8, st));
        SF_HIP(hipEventRecord(ev_p[0], st));
        hipLaunchKernelGGL(k_text_count, dim3(grid_of(n_groups)), dim3(kTextBlock), 0, st, S.bytes[slot].p, n_groups, S.nl_cnt.p, S.tab_cnt.p);
        SF_HIP(hipGetLastError());
        if (int rc = exclusive_scan_u32_u32(S.nl_cnt.p, S.nl_scan.p, n_groups, st)) return rc;
        if (int rc = exclusive_scan_u32_u32(S.tab_cnt.p, S.tab_scan.p, n_groups, st)) return rc;
        SF_HIP(hipEventRecord(ev_p[1], st));
        SF_HIP(hipMemcpyAsync(&h_misc[2], S.nl_scan.p + n_groups, 4, hipMemcpyDeviceToHost, st));
        // the next chunk is staged while this one is parsed (its buffers were freed by the previous chunk's synchronisations)
        const uint64_t npos = end, nend = (npos < n_bytes) ? chunk_end(npos) : npos;
        if (npos < n_bytes && nend != 0) if (int rc = stage(npos, nend, slot ^ 1)) return rc;
        SF_HIP(hipStreamSynchronize(st));
        const uint32_t n_lines = (uint32_t)h_misc[2];
        for (DevBuf<uint32_t>* b : {&S.line_end, &S.lens, &S.rowptr, &S.tab_base})
            if (int rc = b->reserve((uint64_t)n_lines + 1, st, false)) return rc;
        if (int rc = S.counts.reserve((uint64_t)n_lines + 1, st, false)) return rc;
        if (int rc = S.ids.reserve(n / 2 + 1, st, false)) return rc;
        SF_HIP(hipEventRecord(ev_p[2], st));
        hipLaunchKernelGGL(textlines::k_line_ends, dim3(grid_of(n_groups)), dim3(kTextBlock), 0, st, S.bytes[slot].p, n_groups, S.nl_scan.p, S.line_end.p);
        SF_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_text_line_head, dim3(grid_of(n_lines)), dim3(kTextBlock), 0, st, S.bytes[slot].p, n_lines, S.line_end.p,
                           S.tab_scan.p, S.lens.p, S.tab_base.p, S.misc.p);
        SF_HIP(hipGetLastError());
        if (int rc = exclusive_scan_u32_u32(S.lens.p, S.rowptr.p, n_lines, st)) return rc;
        hipLaunchKernelGGL(k_text_parse, dim3(grid_of(n_groups)), dim3(kTextBlock), 0, st, S.bytes[slot].p, n, n_groups, S.nl_scan.p,
                           S.tab_scan.p, S.rowptr.p, S.tab_base.p, n_transcripts, S.ids.p, S.counts.p, S.misc.p, S.misc.p + 1);
        SF_HIP(hipGetLastError());
        SF_HIP(hipEventRecord(ev_p[3], st));
        SF_HIP(hipMemcpyAsync(&h_misc[0], S.misc.p, 16, hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(&h_misc[2], S.rowptr.p + n_lines, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        double parse = 0.0;                                   // both halves or neither
        if (add_elapsed(&parse, ev_p[0], ev_p[1]) && add_elapsed(&parse, ev_p[2], ev_p[3])) out->parse_ms += parse;
        add_elapsed(&out->h2d_ms, ev_h2d[slot], ev_copied[slot]);
        if (h_misc[0] != kNoError) return fail(SFGPU_ERR_FORMAT, line_base + (h_misc[0] >> 8), (int)(h_misc[0] & 0xff));
        const uint64_t n_ids = (uint32_t)h_misc[2];
        const auto t0 = std::chrono::steady_clock::now();
        if (int rc = sfgpu_eq_add_weighted_device(eq, S.ids.p, S.rowptr.p, S.counts.p, n_lines)) return rc;     // returns after the fold has run
        out->fold_ms += ms_since(t0);
        out->n_lines += n_lines; out->n_ids += n_ids; out->sum_counts += h_misc[1]; out->n_chunks++;
        line_base += n_lines;
        if (npos < n_bytes && nend == 0) return fail(SFGPU_ERR_RANGE, line_base, SFGPU_EQTEXT_LONG_LINE);
        pos = npos; end = nend; slot ^= 1;
    }
    return SFGPU_OK;
}
