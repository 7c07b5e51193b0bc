// baifmt.h -- the coordinate-sorted BAM file and its BAI index, stated once: the order of the records, the way the sorted
// stream is cut into BGZF members, what a virtual file offset is and what the index says, so that its bytes are determined.
// Plain C++, host and device, serial: bamsort.hip runs the same functions inside its kernels, tests/bamsort_harness.cpp runs them
// alone (bai_serial_sort / bai_serial_index below), and samfile.write_bam(sort="coordinate") / samfile.build_bai are the Python
// statements both are judged by.  WHAT a record says is bamwfmt.h and is not stated again here.
//
// ORDER   the records of all batches, each on its own (the two records of a pair unit separate), in stable order of the key
//         (uint32)refID << 32 | (uint32)(pos + 1): records with refID -1 come last, ties keep write order, across batches too.
// HEADER  @HD VN:1.6 SO:coordinate, then the @SQ lines of the unsorted file.
// STREAM  the header is the encoder's first write (its last member short); the sorted record stream follows in writes that are
//         multiples of kBaiMember bytes but the last: stream byte x lies in member first_member + x / kBaiMember at offset
//         x % kBaiMember, whatever the pieces were.  Records may straddle members.
// V(x)    coffset(member holding x) << 16 | offset in its payload; V(end of the stream) = coffset(EOF member) << 16.
// EXTENT  of a record with refID >= 0: beg = pos, end = pos + the reference-consuming CIGAR lengths (M D N = X), at least beg + 1;
//         bin = reg2bin(beg, end).
// CHUNKS  a maximal run of records consecutive in the file with the same (refID, bin) is one chunk (vbeg of the first, vend of
//         the last); nothing else is merged.
// PER REFERENCE  n_bin, the bins in ascending number with their chunks in file order, then pseudo-bin 37450 with the two chunks
//         (V(start of the first record), V(end of the last)) and (n_mapped, n_unmapped by FLAG 0x4); then n_intv =
//         ((max end - 1) >> 14) + 1 and the linear index: entry w is the smallest vbeg of the records whose windows
//         beg >> 14 .. (end - 1) >> 14 include w, an entry no record touches takes the next touched entry to its right (the last
//         entry is always touched).  A reference without records is n_bin = 0, n_intv = 0.
// LAYOUT  "BAI\1", n_ref, the references, n_no_coor (uint64): the records with refID < 0.  Everything little-endian.
// The store holds fewer than 2^32 records.  bamwfmt.h's rule 5 bounds end by 2^29: at most kBaiMaxWindows windows a reference.
#pragma once
#include "bamwfmt.h"

#if !defined(__HIPCC__)
#include <algorithm>
#include <map>
#include <vector>
#endif

namespace sfgpu {

constexpr uint32_t kBaiMember = 32768;            // payload bytes of a full BGZF member (bgzwfmt.h's kBgzwPayload)
constexpr uint32_t kBaiPseudoBin = 37450;
constexpr uint32_t kBaiWindowShift = 14;
constexpr uint32_t kBaiMaxWindows = 1u << (29 - 14);
constexpr uint64_t kBaiNoCoorKey = 0xffffffffull << 32;       // keys at or above it: refID < 0

SAMW_HD uint64_t bai_key(int32_t ref, int32_t pos) { return (uint64_t)(uint32_t)ref << 32 | (uint32_t)(pos + 1); }

// the sorted file's header text in front of the @SQ lines
inline const char* bai_hd_line() { return "@HD\tVN:1.6\tSO:coordinate\n"; }

SAMW_HD uint32_t bai_le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// what the index reads of a record (p: its block_size field)
struct BaiRecord {
    uint32_t len;                                 // 4 + block_size
    int32_t ref, pos;
    uint32_t flag, beg, end, bin;                 // extent and bin: of a record with ref >= 0
};
SAMW_HD BaiRecord bai_record(const uint8_t* p) {
    BaiRecord r;
    r.len = 4u + bai_le32(p);
    r.ref = (int32_t)bai_le32(p + 4);
    r.pos = (int32_t)bai_le32(p + 8);
    const uint32_t l_name = p[12], n_cigar = (uint32_t)p[16] | (uint32_t)p[17] << 8;
    r.flag = (uint32_t)p[18] | (uint32_t)p[19] << 8;
    uint32_t span = 0;
    const uint8_t* c = p + kBamwFixed + l_name;
    for (uint32_t k = 0; k < n_cigar; ++k) {      // at most 65 535 words
        const uint32_t w = bai_le32(c + 4 * k), op = w & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += w >> 4;
    }
    r.beg = (uint32_t)r.pos;
    r.end = r.beg + (span ? span : 1u);
    r.bin = r.ref >= 0 ? bamw_reg2bin(r.beg, r.end) : 0u;
    return r;
}
SAMW_HD uint64_t bai_bin_key(const BaiRecord& r) { return (uint64_t)(uint32_t)r.ref << 32 | r.bin; }

// V(x) of byte x of a record stream of `total` bytes whose first member is first_member; coff[0 .. n_members] are the members'
// file offsets, coff[n_members] that of the EOF member
SAMW_HD uint64_t bai_voffset(uint64_t x, uint64_t total, uint64_t first_member, const uint64_t* coff, uint64_t n_members) {
    if (x >= total) return coff[n_members] << 16;
    return coff[first_member + x / kBaiMember] << 16 | (x % kBaiMember);
}

// the bytes of a reference with nb bins (the pseudo-bin not counted) of nc chunks in all and n_intv windows
SAMW_HD uint64_t bai_ref_bytes(uint64_t nb, uint64_t nc, uint64_t n_intv, bool has_records) {
    return 4u + 8u * nb + 16u * nc + (has_records ? 40u : 0u) + 4u + 8u * n_intv;
}

#if !defined(__HIPCC__)
// the records of a stream (host only): offsets of their block_size fields; false where the chain does not end at n
inline bool bai_serial_records(const uint8_t* s, uint64_t n, std::vector<uint64_t>* at) {
    uint64_t p = 0;
    while (p < n) {
        if (n - p < kBamwFixed) return false;
        const uint64_t len = 4ull + bai_le32(s + p);
        if (len < kBamwFixed || p + len > n) return false;
        at->push_back(p);
        p += len;
    }
    return true;
}

// ORDER: `recs` (records in write order, n bytes) sorted into out; returns the number of records, or -1 on a broken chain
inline int64_t bai_serial_sort(const uint8_t* recs, uint64_t n, uint8_t* out) {
    std::vector<uint64_t> at;
    if (!bai_serial_records(recs, n, &at)) return -1;
    std::vector<uint32_t> order(at.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
    auto key = [&](uint32_t i) { return bai_key((int32_t)bai_le32(recs + at[i] + 4), (int32_t)bai_le32(recs + at[i] + 8)); };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    uint64_t o = 0;
    for (uint32_t i : order) {
        const uint64_t len = 4ull + bai_le32(recs + at[i]);
        std::copy(recs + at[i], recs + at[i] + len, out + o);
        o += len;
    }
    return (int64_t)at.size();
}

// The index of a sorted record stream s[0 .. n) whose first member is first_member of the file's member_sizes[0 .. n_members)
// (compressed bytes, the EOF member not among them).  Returns the bytes, -1 on a broken chain, -2 where the keys descend.
inline int64_t bai_serial_index(const uint8_t* s, uint64_t n, uint32_t n_ref, const uint32_t* member_sizes, uint64_t n_members,
                                uint64_t first_member, std::vector<uint8_t>* out) {
    std::vector<uint64_t> at, coff(n_members + 1, 0);
    if (!bai_serial_records(s, n, &at)) return -1;
    for (uint64_t m = 0; m < n_members; ++m) coff[m + 1] = coff[m] + member_sizes[m];
    struct Ref {
        std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
        std::vector<uint64_t> lin;
        uint64_t vbeg = 0, vend = 0, n_mapped = 0, n_unmapped = 0;
        bool any = false;
    };
    std::vector<Ref> refs(n_ref);
    uint64_t no_coor = 0, last_key = 0, last_bin_key = ~0ull;
    for (size_t i = 0; i < at.size(); ++i) {
        const BaiRecord r = bai_record(s + at[i]);
        const uint64_t k = bai_key(r.ref, r.pos);
        if (k < last_key) return -2;
        last_key = k;
        if (r.ref < 0 || (uint32_t)r.ref >= n_ref) { ++no_coor; continue; }
        const uint64_t vbeg = bai_voffset(at[i], n, first_member, coff.data(), n_members);
        const uint64_t vend = bai_voffset(at[i] + r.len, n, first_member, coff.data(), n_members);
        Ref& R = refs[(uint32_t)r.ref];
        auto& chunks = R.bins[r.bin];
        if (bai_bin_key(r) == last_bin_key) chunks.back().second = vend;
        else chunks.push_back({vbeg, vend});
        last_bin_key = bai_bin_key(r);
        if (!R.any) { R.any = true; R.vbeg = vbeg; }
        R.vend = vend;
        (r.flag & 4u ? R.n_unmapped : R.n_mapped)++;
        const uint32_t w0 = r.beg >> kBaiWindowShift, w1 = (r.end - 1u) >> kBaiWindowShift;
        if (R.lin.size() < (size_t)w1 + 1) R.lin.resize((size_t)w1 + 1, ~0ull);
        for (uint32_t w = w0; w <= w1; ++w) if (vbeg < R.lin[w]) R.lin[w] = vbeg;
    }
    auto le = [&](uint64_t v, int bytes) { for (int b = 0; b < bytes; ++b) out->push_back((uint8_t)(v >> (8 * b))); };
    out->clear();
    for (char c : {'B', 'A', 'I', '\1'}) out->push_back((uint8_t)c);
    le(n_ref, 4);
    for (Ref& R : refs) {
        le(R.any ? R.bins.size() + 1 : 0, 4);
        for (auto& b : R.bins) {
            le(b.first, 4); le(b.second.size(), 4);
            for (auto& c : b.second) { le(c.first, 8); le(c.second, 8); }
        }
        if (R.any) { le(kBaiPseudoBin, 4); le(2, 4); le(R.vbeg, 8); le(R.vend, 8); le(R.n_mapped, 8); le(R.n_unmapped, 8); }
        for (size_t w = R.lin.size(); w-- > 1;) if (R.lin[w - 1] == ~0ull) R.lin[w - 1] = R.lin[w];
        le(R.lin.size(), 4);
        for (uint64_t v : R.lin) le(v, 8);
    }
    le(no_coor, 8);
    return (int64_t)out->size();
}
#endif

}  // namespace sfgpu
