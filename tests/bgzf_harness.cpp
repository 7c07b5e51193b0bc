// bgzf_harness.cpp -- sailfish_amd/csrc/bgzfmt.h as plain C++ (g++, a shared object, nothing but libstdc++): the member directory and
// the serial inflater over a whole file, reported in the fields of sfgpu_bgzf_result.  tests/test_bgzf_cpu.py lets zlib judge
// it; tests/test_gpu_bgzf.py compares sfgpu_bgzf_inflate_host with it.
#include <cstring>
#include <vector>

#include "bgzfmt.h"

using namespace sfgpu;

// src[0 .. n) -> dst[0 .. cap); the timing fields stay 0.  Returns SFGPU_OK or SFGPU_ERR_FORMAT.
extern "C" int bgzf_harness_inflate(const uint8_t* src, uint64_t n, int final, uint8_t* dst, uint64_t cap, sfgpu_bgzf_result* out) {
    memset(out, 0, sizeof(*out));
    std::vector<BgzDirEntry> dir;
    const BgzScan s = bgz_scan(src, n, final ? 1 : 0, cap, [&](const BgzDirEntry& e) { dir.push_back(e); });
    out->n_members = s.n_members; out->consumed = s.consumed; out->n_bytes_out = s.n_bytes_out;
    out->error_member = s.error_member; out->error_kind = s.error_kind;
    for (uint64_t m = 0; m < dir.size(); ++m) {
        const BgzDirEntry& e = dir[m];
        const BgzMember r = bgz_inflate_member(src + e.in_off, e.in_len, dst + e.out_off, e.isize);
        out->n_stored_blocks += r.counts.blocks[0]; out->n_fixed_blocks += r.counts.blocks[1]; out->n_dynamic_blocks += r.counts.blocks[2];
        if (r.kind != SFGPU_BGZF_OK && m < out->error_member) { out->error_member = m; out->error_kind = r.kind; }
    }
    return out->error_kind == SFGPU_BGZF_OK ? SFGPU_OK : SFGPU_ERR_FORMAT;
}

// one member alone, as bgz_inflate_member reports it: the kind; *n_out bytes were written
extern "C" int bgzf_harness_member(const uint8_t* src, uint64_t n, uint8_t* dst, uint64_t cap, uint32_t* n_out, uint32_t* blocks) {
    const BgzMember r = bgz_inflate_member(src, n, dst, cap);
    *n_out = r.counts.n_out;
    for (int k = 0; k < 3; ++k) blocks[k] = r.counts.blocks[k];
    return r.kind;
}
