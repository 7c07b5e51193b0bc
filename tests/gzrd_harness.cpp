// gzrd_harness.cpp -- sailfish_amd/csrc/gzrdfmt.h as plain C++ (g++, a shared object, nothing but libstdc++): the whole chunked
// inflate of ordinary gzip run serially -- finder, pass A, chain, window propagation, pass B, trailer -- behind the four calls of
// the ABI (open / plan / emit / close) and reported in the fields of sfgpu_gzrd_result.  tests/test_gzrd_cpu.py lets zlib judge
// it; tests/test_gpu_gzrd.py compares sfgpu_gzrd_* with it.  The timing fields stay 0.
#include <cstring>
#include <vector>

#include "gzrdfmt.h"

using namespace sfgpu;

namespace {

struct Handle {
    uint32_t chunk_bytes;
    GzrState st;
    std::vector<uint8_t> win;                    // the carried window
    // the plan
    bool planned = false;
    std::vector<uint8_t> src;
    GzrStart start;
    GzrChain chain;
    std::vector<uint64_t> cand;
    std::vector<GzrChunkRec> rec;
    std::vector<std::vector<uint16_t>> ring;     // per span that has a chunk
    std::vector<std::vector<uint8_t>> resolved;  // per chain chunk but the last: the window behind it
    uint32_t crc_stored = 0, isize = 0;
    sfgpu_gzrd_result res;
};

uint64_t chunk_start(const Handle* h, size_t k) { return k == 0 ? h->start.start_bit : h->cand[h->chain.span[k]]; }

}  // namespace

extern "C" int gzrd_harness_open(void** out, uint32_t chunk_bytes) {
    if (chunk_bytes && chunk_bytes < 64) return SFGPU_ERR_RANGE;
    Handle* h = new Handle;
    h->chunk_bytes = chunk_bytes ? chunk_bytes : kGzrDefaultChunk;
    memset(&h->st, 0, sizeof(h->st));
    h->win.assign(kGzrWindow, 0);
    *out = h;
    return SFGPU_OK;
}

extern "C" int gzrd_harness_close(void* z) {
    delete static_cast<Handle*>(z);
    return SFGPU_OK;
}

extern "C" int gzrd_harness_plan(void* z, const uint8_t* h_src, uint64_t n, int final, uint64_t cap, sfgpu_gzrd_result* res) {
    Handle* h = static_cast<Handle*>(z);
    memset(res, 0, sizeof(*res));
    res->error_offset = ~0ull;
    h->planned = true;
    h->chain = GzrChain();
    h->src.assign(h_src, h_src + n);
    h->src.resize(n + 64, 0);
    const uint8_t* src = h->src.data();
    h->start = gzr_call_start(h->st, src, n, final);
    auto leave = [&]() -> int { h->res = *res; return res->error_kind == SFGPU_BGZF_OK ? SFGPU_OK : SFGPU_ERR_FORMAT; };
    if (h->start.kind != SFGPU_BGZF_OK) { res->error_kind = h->start.kind; res->error_offset = h->start.at; return leave(); }
    res->consumed = h->start.at;
    if (!h->start.decode) return leave();

    const uint64_t start_bit = h->start.start_bit, start_byte = start_bit >> 3, n_bits = n * 8;
    const uint64_t n_spans = n > start_byte ? (n - start_byte + h->chunk_bytes - 1) / h->chunk_bytes : 1;
    h->cand.assign(n_spans, kGzrNone);
    h->rec.assign(n_spans, GzrChunkRec());
    h->ring.assign(n_spans, std::vector<uint16_t>());
    BgzTables T;
    GzrSerialIO io{src, (uint32_t)n, nullptr, nullptr, nullptr};
    // ---- the finder
    for (uint64_t s = 1; s < n_spans; ++s) {
        const uint64_t q0 = (start_byte + s * h->chunk_bytes) * 8, q1 = q0 + (uint64_t)h->chunk_bytes * 8 < n_bits ? q0 + (uint64_t)h->chunk_bytes * 8 : n_bits;
        for (uint64_t q = q0; q < q1; ++q) {
            if (!gzr_cheap_test([&](uint32_t p) { return io.word(p); }, q, n_bits)) continue;
            if (gzr_header_at(io, &T, q, (uint32_t)n)) { h->cand[s] = q; ++res->n_candidates; break; }
        }
    }
    // ---- pass A
    for (uint64_t s = 0; s < n_spans; ++s) {
        if (s && h->cand[s] == kGzrNone) continue;
        h->ring[s].resize(kGzrWindow);
        for (uint32_t i = 0; i < kGzrWindow; ++i) h->ring[s][i] = (uint16_t)(kGzrMarker | i);
        io.ring = h->ring[s].data();
        gzr_decode_chunk(io, &T, s ? h->cand[s] : start_bit, (uint32_t)n, kGzrWindow,
                         [&](uint64_t b) { return gzr_is_candidate(h->cand.data(), n_spans, b, start_byte, h->chunk_bytes); }, &h->rec[s]);
    }
    // ---- the chain
    h->chain = gzr_chain(h->cand.data(), h->rec.data(), n_spans, start_bit, h->chunk_bytes, final, cap);
    const GzrChain& c = h->chain;
    res->consumed = gzr_consumed(h->start, c);
    res->n_bytes_out = c.n_out; res->n_chunks = c.span.size(); res->n_false_starts = c.n_false;
    res->n_stored_blocks = c.blocks[0]; res->n_fixed_blocks = c.blocks[1]; res->n_dynamic_blocks = c.blocks[2];
    res->need_cap = c.need_cap; res->member_end = c.member_end;
    if (c.error_kind != SFGPU_BGZF_OK) { res->error_kind = c.error_kind; res->error_offset = c.error_bit >> 3; }
    if (c.member_end) {
        auto byte = [&](uint64_t p) -> uint32_t { return src[p]; };
        h->crc_stored = bgz_le32(byte, c.end_bit >> 3); h->isize = bgz_le32(byte, (c.end_bit >> 3) + 4);
    }
    // ---- window propagation
    h->resolved.assign(c.span.size() ? c.span.size() - 1 : 0, std::vector<uint8_t>());
    for (size_t k = 0; k + 1 < c.span.size(); ++k) {
        const uint8_t* prev = k ? h->resolved[k - 1].data() : h->win.data();
        const uint16_t* ring = h->ring[c.span[k]].data();
        h->resolved[k].resize(kGzrWindow);
        for (uint32_t j = 0; j < kGzrWindow; ++j)
            h->resolved[k][j] = (uint8_t)gzr_resolve([&](uint32_t i) -> uint32_t { return ring[i]; }, [&](uint32_t i) -> uint32_t { return prev[i]; },
                                                     h->rec[c.span[k]].n_out, j);
    }
    return leave();
}

extern "C" int gzrd_harness_emit(void* z, uint8_t* dst, sfgpu_gzrd_result* res) {
    Handle* h = static_cast<Handle*>(z);
    if (!h->planned) return SFGPU_ERR_STATE;
    h->planned = false;
    *res = h->res;
    const GzrChain& c = h->chain;
    if (c.span.empty()) return res->error_kind == SFGPU_BGZF_OK ? SFGPU_OK : SFGPU_ERR_FORMAT;
    const uint32_t n = (uint32_t)(h->src.size() - 64);
    BgzTables T;
    std::vector<uint32_t> crcs(c.span.size());
    uint32_t table[256];
    for (uint32_t i = 0; i < 256u; ++i) table[i] = crc32_table_entry(i);
    const uint32_t valid0 = h->start.begins_member ? 0u : h->st.valid;
    for (size_t k = 0; k < c.span.size(); ++k) {
        const GzrChunkRec& r = h->rec[c.span[k]];
        uint8_t* out = dst + c.out_off[k];
        GzrSerialIO io{h->src.data(), n, nullptr, out, k ? h->resolved[k - 1].data() : h->win.data()};
        const uint64_t valid = valid0 + c.out_off[k] < kGzrWindow ? valid0 + c.out_off[k] : kGzrWindow;
        GzrChunkRec again;
        gzr_decode_chunk(io, &T, chunk_start(h, k), n, (uint32_t)valid, [&](uint64_t b) { return b == r.end_bit; }, &again);
        if (again.status == kGzrStopError) {
            res->error_kind = again.kind; res->error_offset = chunk_start(h, k) >> 3;
            return SFGPU_ERR_FORMAT;
        }
        crcs[k] = crc32_slice(0u, table, [&](uint32_t i) -> uint32_t { return out[i]; }, (uint32_t)r.n_out);
    }
    std::vector<uint8_t> win(kGzrWindow);
    for (uint32_t j = 0; j < kGzrWindow; ++j)
        win[j] = (uint8_t)gzr_carry([&](uint32_t i) -> uint32_t { return h->win[i]; }, [&](uint64_t i) -> uint32_t { return dst[i]; }, c.n_out, j);
    h->win.swap(win);
    const int k = gzr_finish_call(&h->st, h->start, c, h->rec.data(), crcs.data(), h->crc_stored, h->isize);
    if (k != SFGPU_BGZF_OK) { res->error_kind = k; res->error_offset = chunk_start(h, c.span.size() - 1) >> 3; }
    return res->error_kind == SFGPU_BGZF_OK ? SFGPU_OK : SFGPU_ERR_FORMAT;
}

// the bit positions at which the chunks of the last plan start -> their number
extern "C" uint64_t gzrd_harness_chain(void* z, uint64_t* starts, uint64_t cap) {
    Handle* h = static_cast<Handle*>(z);
    for (size_t k = 0; k < h->chain.span.size() && k < cap; ++k) starts[k] = chunk_start(h, k);
    return h->chain.span.size();
}

// the candidates of the last plan (kGzrNone for a span without one) -> the number of spans
extern "C" uint64_t gzrd_harness_candidates(void* z, uint64_t* cand, uint64_t cap) {
    Handle* h = static_cast<Handle*>(z);
    for (size_t s = 0; s < h->cand.size() && s < cap; ++s) cand[s] = h->cand[s];
    return h->cand.size();
}

// a plain serial walk of the DEFLATE stream that begins at start_bit of src[0 .. n): the bit positions at which its blocks start
// -> their number; blocks[3] by type, *end_status = how the walk ended (kGzrStop*)
extern "C" uint64_t gzrd_harness_walk(const uint8_t* h_src, uint64_t n, uint64_t start_bit, uint64_t* starts, uint64_t cap, uint32_t* blocks,
                                      int32_t* end_status) {
    std::vector<uint8_t> src(h_src, h_src + n);
    src.resize(n + 64, 0);
    std::vector<uint16_t> ring(kGzrWindow, 0);
    BgzTables T;
    GzrSerialIO io{src.data(), (uint32_t)n, ring.data(), nullptr, nullptr};
    GzrChunkRec rec;
    uint64_t k = 0;
    if (k < cap) starts[k] = start_bit;
    ++k;
    gzr_decode_chunk(io, &T, start_bit, (uint32_t)n, kGzrWindow, [&](uint64_t b) { if (k < cap) starts[k] = b; ++k; return false; }, &rec);
    for (int t = 0; t < 3; ++t) blocks[t] = rec.blocks[t];
    *end_status = rec.status;
    // (the last boundary recorded is where a final block starts, or behind the last whole block when the input ends)
    return rec.status == kGzrStopFinal ? k : k - 1;
}
