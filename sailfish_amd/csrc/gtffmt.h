// gtffmt.h -- what a --geneMap file says, for both of its forms (GTF and the two-column map): the one statement of the rules that
// genes.TranscriptGeneMap.from_gtf / .from_file set.  Plain C++, host and device, serial; genemap.hip runs the same functions inside
// its kernels (one wavefront per line finds WHERE a field starts in parallel; WHETHER a field carries a key, and what its value
// is, is decided here), and tests/gmap_harness.cpp runs them alone.
//
// Whitespace (WS): bytes 0x09-0x0D, 0x1C-0x1F and 0x20 -- what Python's str.strip() / str.split() remove among ASCII.
// Lines end at '\n'; a '\r' directly in front of it is not part of the line; the last line may lack its '\n'.
//
// GTF line: skipped when its first byte is '#' or it has fewer than 9 tab-separated columns (an empty or all-WS line has fewer, or
// an empty column 8: no record either way).  Only column 8 is read; it is split at EVERY ';' (also inside quotes, as the host
// reader does).  A field is stripped of WS and dropped when empty; its key is the bytes up to the first 0x20 (or all of it), its
// value the rest stripped of WS, then of all leading and trailing '"'.  The first field with a given key wins.  The line is a record
// iff it has the key transcript_id with a non-empty value; the record carries that id and either "key absent" or the value (maybe
// empty) of the aggregation key.
// GTF map: per distinct transcript id the gene is the value of the first record, in file order, that carries the key ("" when none
// does); transcripts in bytewise order, a prefix first (strcmp, Python's sorted); genes numbered by first appearance in that order.
// Two-column map: tokens are maximal runs of non-WS bytes over the whole file (parity carries across lines and blocks); consecutive
// pairs are (transcript, gene), a trailing odd token is dropped; no dedupe; genes numbered by first appearance in file order;
// transcripts in a stable bytewise sort.
//
// Host-only inputs, flagged (GT_HOST_*), never parsed: a byte >= 0x80, a NUL, a '\r' not followed by '\n' (Python's universal
// newlines end a line there), a transcript id, key value or token longer than kGmapNameCap bytes.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GT_HD __host__ __device__
#else
#define GT_HD
#endif

namespace sfgpu {

constexpr uint32_t kGmapNameCap = 256;

enum : uint32_t { GT_HOST_HIGH_BYTE = 1, GT_HOST_NUL = 2, GT_HOST_LONE_CR = 4, GT_HOST_LONG_NAME = 8 };

GT_HD inline bool gt_ws(unsigned char b) { return (b >= 0x09 && b <= 0x0D) || (b >= 0x1C && b <= 0x20); }

// the host-only flag of byte p of a text of n bytes (get(p + 1) is read only below n)
template <typename Get>
GT_HD inline uint32_t gt_byte_flag(Get get, uint64_t p, uint64_t n) {
    const unsigned char b = get(p);
    if (b >= 0x80) return GT_HOST_HIGH_BYTE;
    if (b == 0) return GT_HOST_NUL;
    if (b == '\r' && (p + 1 >= n || get(p + 1) != '\n')) return GT_HOST_LONE_CR;
    return 0;
}

// Can any field have this key?  Not an empty one, not one that holds a separator (';', tab, line end, the 0x20 that ends a key),
// not one that begins with WS (the field is stripped first).
GT_HD inline bool gt_key_usable(const unsigned char* key, uint32_t klen) {
    if (klen == 0 || gt_ws(key[0])) return false;
    for (uint32_t i = 0; i < klen; ++i)
        if (key[i] == ';' || key[i] == '\t' || key[i] == '\n' || key[i] == '\r' || key[i] == 0x20) return false;
    return true;
}

// Does the field that begins at f -- the start of column 8 or the byte behind a ';'; the column is [.., b) -- have this (usable)
// key?  Then *v = where its value begins: behind the first 0x20, or the field's end when the stripped field is the key alone.
template <typename Get>
GT_HD inline bool gt_field_has_key(Get get, uint32_t f, uint32_t b, const unsigned char* key, uint32_t klen, uint32_t* v) {
    while (f < b && gt_ws(get(f))) ++f;
    if (b - f < klen) return false;
    for (uint32_t i = 0; i < klen; ++i)
        if (get(f + i) != key[i]) return false;
    uint32_t q = f + klen;
    if (q < b && get(q) == 0x20) { *v = q + 1; return true; }
    if (gt_ws(key[klen - 1])) return false;              // the strip would have cut the key short
    while (q < b && gt_ws(get(q))) ++q;                  // (a ';' is not WS)
    if (q < b && get(q) != ';') return false;
    *v = q;
    return true;
}

// the value of the field whose value begins at v: [*vs, *vs + *vl)
template <typename Get>
GT_HD inline void gt_field_value(Get get, uint32_t v, uint32_t b, uint32_t* vs, uint32_t* vl) {
    uint32_t e = v;
    while (e < b && get(e) != ';') ++e;
    while (v < e && gt_ws(get(v))) ++v;
    while (e > v && gt_ws(get(e - 1))) --e;
    while (v < e && get(v) == '"') ++v;
    while (e > v && get(e - 1) == '"') --e;
    *vs = v; *vl = e - v;
}

// the line without its '\r' ([s, e) excludes the '\n')
template <typename Get>
GT_HD inline uint32_t gt_line_end(Get get, uint32_t s, uint32_t e) { return (e > s && get(e - 1) == '\r') ? e - 1 : e; }

struct GtKey {
    const unsigned char* p;
    uint32_t len;
    bool usable;
};

struct GtRec {
    uint32_t t_s, t_len;        // the transcript id; t_len == 0: the line is no record
    uint32_t g_s, g_len;        // the value of the aggregation key
    uint32_t has_key;
    uint32_t flags;             // GT_HOST_LONG_NAME
};

GT_HD inline const unsigned char* gt_tid_key() { return reinterpret_cast<const unsigned char*>("transcript_id"); }
constexpr uint32_t kGtTidKeyLen = 13;

// what is left once the two fields are found (f_* = where the value of the first field with that key begins; found_*: there is one)
template <typename Get>
GT_HD inline GtRec gt_record_of(Get get, uint32_t b, bool found_t, uint32_t v_t, bool found_g, uint32_t v_g) {
    GtRec r = {0, 0, 0, 0, 0, 0};
    if (!found_t) return r;
    gt_field_value(get, v_t, b, &r.t_s, &r.t_len);
    if (r.t_len == 0) return r;
    if (found_g) { gt_field_value(get, v_g, b, &r.g_s, &r.g_len); r.has_key = 1; }
    if (r.t_len > kGmapNameCap || r.g_len > kGmapNameCap) r.flags = GT_HOST_LONG_NAME;
    return r;
}

// one line [s, e) (no '\n'), serially
template <typename Get>
GT_HD inline GtRec gt_gtf_line(Get get, uint32_t s, uint32_t e, GtKey key) {
    const GtRec none = {0, 0, 0, 0, 0, 0};
    e = gt_line_end(get, s, e);
    if (e == s || get(s) == '#') return none;
    uint32_t tabs = 0, a = e, b = e;
    for (uint32_t p = s; p < e; ++p) {
        if (get(p) != '\t') continue;
        if (++tabs == 8) a = p + 1;
        if (tabs == 9) { b = p; break; }
    }
    if (tabs < 8) return none;
    bool found_t = false, found_g = false;
    uint32_t v_t = 0, v_g = 0;
    for (uint32_t f = a;;) {
        if (!found_t) found_t = gt_field_has_key(get, f, b, gt_tid_key(), kGtTidKeyLen, &v_t);
        if (!found_g && key.usable) found_g = gt_field_has_key(get, f, b, key.p, key.len, &v_g);
        while (f < b && get(f) != ';') ++f;
        if (f >= b) break;
        ++f;
    }
    return gt_record_of(get, b, found_t, v_t, found_g, v_g);
}

}  // namespace sfgpu

#ifdef GTFFMT_SERIAL_MAP
// The maps, serially, on the host: what tests/gmap_harness.cpp compares with the Python readers.  Text is fed in blocks; whole lines
// are consumed and the caller carries the tail (as sfgpu_gmap_add_text_* do).
#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace sfgpu {

struct GtSerialMap {
    int gtf;
    std::string key;
    uint32_t flags = 0;
    uint64_t n_lines = 0, n_records = 0;
    std::vector<std::string> strs;          // GTF: (id, value) per record; two-column: the tokens
    std::vector<char> has;                  // GTF: per record
    std::vector<std::string> transcript_names, gene_names;
    std::vector<uint32_t> t2g;

    GtSerialMap(int gtf_, const std::string& key_) : gtf(gtf_), key(key_) {}

    // -> bytes consumed (the text up to its last '\n'; all of it when final)
    uint64_t add(const unsigned char* text, uint64_t n, bool final) {
        uint64_t used = n;
        if (!final) { while (used && text[used - 1] != '\n') --used; }
        auto get = [&](uint64_t p) { return text[p]; };
        for (uint64_t p = 0; p < used; ++p) flags |= gt_byte_flag(get, p, used);
        if (flags) return used;
        const GtKey k = {reinterpret_cast<const unsigned char*>(key.data()), (uint32_t)key.size(),
                         gt_key_usable(reinterpret_cast<const unsigned char*>(key.data()), (uint32_t)key.size())};
        if (gtf) {
            for (uint64_t s = 0; s < used;) {
                uint64_t e = s;
                while (e < used && text[e] != '\n') ++e;
                ++n_lines;
                const GtRec r = gt_gtf_line(get, (uint32_t)s, (uint32_t)e, k);
                flags |= r.flags;
                if (r.t_len) {
                    strs.emplace_back(reinterpret_cast<const char*>(text) + r.t_s, r.t_len);
                    strs.emplace_back(reinterpret_cast<const char*>(text) + r.g_s, r.g_len);
                    has.push_back((char)r.has_key);
                    ++n_records;
                }
                s = e + 1;
            }
        } else {
            for (uint64_t p = 0; p < used; ++p) n_lines += text[p] == '\n';
            if (used && text[used - 1] != '\n') ++n_lines;
            for (uint64_t p = 0; p < used;) {
                if (gt_ws(text[p])) { ++p; continue; }
                uint64_t q = p;
                while (q < used && !gt_ws(text[q])) ++q;
                if (q - p > kGmapNameCap) flags |= GT_HOST_LONG_NAME;
                strs.emplace_back(reinterpret_cast<const char*>(text) + p, q - p);
                ++n_records;
                p = q;
            }
        }
        return used;
    }

    void finish() {
        std::vector<std::string> names, genes;      // the items in the order the genes are numbered in
        if (gtf) {
            std::map<std::string, std::pair<bool, std::string>> first;      // bytewise order (char_traits<char>::compare is memcmp)
            for (size_t r = 0; r < has.size(); ++r) {
                auto it = first.emplace(strs[2 * r], std::make_pair(false, std::string())).first;
                if (!it->second.first && has[r]) it->second = std::make_pair(true, strs[2 * r + 1]);
            }
            for (auto& kv : first) { names.push_back(kv.first); genes.push_back(kv.second.second); }
        } else {
            for (size_t i = 0; i + 1 < strs.size(); i += 2) { names.push_back(strs[i]); genes.push_back(strs[i + 1]); }
        }
        std::map<std::string, uint32_t> id;
        std::vector<uint32_t> g(names.size());
        for (size_t i = 0; i < names.size(); ++i) {
            auto it = id.find(genes[i]);
            if (it == id.end()) { it = id.emplace(genes[i], (uint32_t)gene_names.size()).first; gene_names.push_back(genes[i]); }
            g[i] = it->second;
        }
        std::vector<uint32_t> order(names.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
        if (!gtf) std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return names[x] < names[y]; });
        for (uint32_t i : order) { transcript_names.push_back(names[i]); t2g.push_back(g[i]); }
    }
};

}  // namespace sfgpu
#endif
