// genemap.hip -- the --geneMap file (GTF or `transcript gene` pairs) read on the device, and the join of the transcript names with
// it: sfgpu_gmap_*.  What a file says is decided by gtffmt.h (the same functions run serially in tests/gmap_harness.cpp); this file
// is the passes around them.
//
// add_text: the consumed text (whole lines) lies on the device as 16-byte groups.
//   k_gmap_count      per group: its '\n' bytes (and, two-column form, its token starts), the host-only byte flags
//   scan, k_gmap_line_ends   where every line ends (textlines.h's kernel with the mask cut to the consumed length)
//   k_gtf_lines       ONE WAVEFRONT PER LINE.  A GTF line is hundreds of bytes, so one lane per line would walk 64 different cache
//                     lines a byte at a time; a wavefront reads its line in 1 KB steps, 16 bytes per lane, coalesced.  Step one
//                     counts the tabs (popcount per lane, prefix sum over the wave) up to the 8th and 9th: column 8 is [a, b).
//                     Step two walks column 8 the same way: every lane looks for ';' in its 16 bytes and runs gtffmt.h's
//                     gt_field_has_key at the field starts it owns (the byte behind each ';', and a); the first field with a key
//                     is the lowest set lane of a ballot.  The steps carry the tab count and the "found" state, so a line of any
//                     length is read once.  The two values are cut by gt_record_of.  The bytes a field test reads beyond the lane's
//                     own group were loaded by the same wavefront in the same step: they come from the L1, no LDS stage is kept.
//   k_tsv_tokens      two-column form: one lane per group walks the tokens that start in it
//   scans, k_gmap_append   the names of the records, compacted into the handle's blob (one lane per name)
// finish: the string sort is rank refinement in rounds of 8 bytes (rank_strings, ranksort.h): the key of a round is the next 8 bytes of each
// name, big-endian and zero-padded (no NUL in a name, so a prefix sorts first); two stable sort_pairs_u64_u32 passes, by key and
// then by the current run, order the names by (run, key), and a new run starts wherever either changes.  The first order is file
// order and every pass is stable, so inside a run of equal names the records stay in file order: "the first record that carries
// the key" is an atomic min over the run, and the tie rule of the two-column form is free.  Genes are numbered by the same sort
// over the gene value of every item: the first item of a run (the smallest position, by stability) is flagged in item order, and a
// scan of the flags is the id.
// lookup: one lane per row, a bytewise lower_bound in the sorted names.
#include "common.h"
#include "gtffmt.h"
#include "primitives.h"
#include "ranksort.h"
#include "textlines.h"

namespace sfgpu {
namespace {

// the 16-byte-group scheme of textlines.h (newline counts per group, their scan, line ends), with every mask cut to the text's length
constexpr int kBlock = 256;
inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
constexpr uint64_t kSubBytes = 4ull << 20;               // staged sub-chunk (a multiple of 16)
constexpr uint64_t kMaxBytes = 1ull << 30;               // one add call
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kLinesPerBlock = kBlock / kWave;

struct Bytes {
    const unsigned char* p;
    __device__ unsigned char operator()(uint64_t i) const { return p[i]; }
};

using textlines::eq_mask;
using textlines::range_mask;

__device__ inline bool word_has_zero(uint32_t w) { return ((w - 0x01010101u) & ~w & 0x80808080u) != 0; }

// nl_cnt[g] = '\n' bytes of group g below n_text; tok_cnt[g] (two-column form) = tokens that start in it; *flags |= the host-only
// flags of the bytes below n_flag
__global__ void k_gmap_count(const uint4* __restrict__ buf, uint64_t n_groups, uint64_t n_text, uint64_t n_flag, uint32_t* __restrict__ nl_cnt,
                             uint32_t* __restrict__ tok_cnt, uint32_t* __restrict__ flags) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint4 v = buf[g];
    const uint64_t p0 = g * 16;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(buf);
    nl_cnt[g] = __popc(eq_mask(v, '\n') & range_mask(p0, 0, n_text));
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    bool odd = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) odd |= (w[i] & 0x80808080u) != 0 || word_has_zero(w[i]) || word_has_zero(w[i] ^ 0x0d0d0d0du);
    if (odd) {
        uint32_t f = 0;
        for (uint64_t p = p0; p < p0 + 16 && p < n_flag; ++p) f |= gt_byte_flag(Bytes{bytes}, p, n_flag);
        if (f) atomicOr(flags, f);
    }
    if (tok_cnt) {
        uint32_t tok = 0;                                  // bit i = byte i is not WS
        for (uint64_t p = p0; p < p0 + 16 && p < n_text; ++p) tok |= (uint32_t)!gt_ws(bytes[p]) << (p - p0);
        const uint32_t prev = (g && !gt_ws(bytes[p0 - 1])) ? 1u : 0u;
        tok_cnt[g] = __popc(tok & ~((tok << 1) | prev));
    }
}

// line_end[j] = the byte at which line j ends, for the '\n' bytes below n_text only: textlines::k_line_ends takes every '\n' of the last
// group, and behind a device text that group holds the caller's tail, not zeros -- the mask is cut exactly as k_gmap_count cuts the
// count that sized line_end
__global__ void k_gmap_line_ends(const uint4* __restrict__ buf, uint64_t n_groups, uint64_t n_text, const uint32_t* __restrict__ nl_scan,
                                 uint32_t* __restrict__ line_end) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    uint32_t nl = eq_mask(buf[g], '\n') & range_mask(g * 16, 0, n_text);
    uint32_t at = nl_scan[g];
    while (nl) {
        const int i = __ffs(nl) - 1;
        nl &= nl - 1;
        line_end[at++] = (uint32_t)(g * 16 + i);
    }
}

// the tokens that start in group g: start[k], len[k] for k = tok_scan[g] ...
__global__ void k_tsv_tokens(const unsigned char* __restrict__ bytes, uint64_t n_groups, uint64_t n_text, const uint32_t* __restrict__ tok_scan,
                             uint32_t* __restrict__ start, uint32_t* __restrict__ len, uint32_t* __restrict__ flags) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    uint32_t at = tok_scan[g];
    if (tok_scan[g + 1] == at) return;
    const uint64_t p0 = g * 16;
    bool prev = g && !gt_ws(bytes[p0 - 1]);
    for (uint64_t p = p0; p < p0 + 16 && p < n_text; ++p) {
        const bool in = !gt_ws(bytes[p]);
        if (in && !prev) {
            uint64_t q = p + 1;
            while (q < n_text && q - p <= kGmapNameCap && !gt_ws(bytes[q])) ++q;
            if (q - p > kGmapNameCap) atomicOr(flags, (uint32_t)GT_HOST_LONG_NAME);
            start[at] = (uint32_t)p; len[at] = (uint32_t)(q - p); ++at;
        }
        prev = in;
    }
}

__device__ inline uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= (uint32_t)o) v += t;
    }
    return v;
}

// position (0-based) of the k-th (1-based) set bit of m
__device__ inline uint32_t nth_bit(uint32_t m, uint32_t k) {
    for (uint32_t i = 1; i < k; ++i) m &= m - 1;
    return (uint32_t)__ffs(m) - 1u;
}

// One wavefront per line (see the head of the file).  Every branch around a shuffle or a ballot is wave-uniform: the line, its
// bounds and the loop states are the same in all 64 lanes.
__global__ void __launch_bounds__(kBlock) k_gtf_lines(const uint4* __restrict__ buf, uint32_t L, const uint32_t* __restrict__ line_end,
                                                      const unsigned char* __restrict__ key, uint32_t klen, int key_usable,
                                                      uint32_t* __restrict__ t_s, uint32_t* __restrict__ t_len, uint32_t* __restrict__ g_s,
                                                      uint32_t* __restrict__ g_len, uint32_t* __restrict__ has, uint32_t* __restrict__ isrec,
                                                      uint32_t* __restrict__ flags) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t line = blockIdx.x * kLinesPerBlock + (threadIdx.x >> 6);
    if (line >= L) return;
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(buf);
    const Bytes get{bytes};
    const uint32_t s = line ? line_end[line - 1] + 1 : 0;
    const uint32_t e = gt_line_end(get, s, line_end[line]);
    GtRec r = {0, 0, 0, 0, 0, 0};
    if (e > s && bytes[s] != '#') {
        // ---- column 8 = [a, b): behind the 8th tab, up to the 9th or the line's end
        uint32_t tabs = 0, a = e, b = e;
        for (uint32_t base = s & ~15u; base < e && tabs < 9; base += kWave * 16) {
            const uint32_t p0 = base + lane * 16;
            uint32_t m = 0;
            if (p0 < e) m = eq_mask(buf[p0 >> 4], '\t') & range_mask(p0, s, e);
            const uint32_t incl = wave_inclusive_sum(__popc(m), lane);
            const uint32_t before = tabs + incl - __popc(m);
            const bool has8 = before < 8 && before + __popc(m) >= 8, has9 = before < 9 && before + __popc(m) >= 9;
            const uint32_t pos8 = has8 ? p0 + nth_bit(m, 8 - before) : 0, pos9 = has9 ? p0 + nth_bit(m, 9 - before) : 0;
            const unsigned long long b8 = __ballot(has8), b9 = __ballot(has9);
            if (b8) a = __shfl(pos8, __ffsll(b8) - 1) + 1;
            if (b9) b = __shfl(pos9, __ffsll(b9) - 1);
            tabs += __shfl(incl, kWave - 1);
        }
        if (tabs >= 8) {
            // ---- the first field with each key
            bool found_t = false, found_g = !key_usable;
            uint32_t v_t = 0, v_g = 0;
            for (uint32_t base = a & ~15u; base < b && !(found_t && found_g); base += kWave * 16) {
                const uint32_t p0 = base + lane * 16;
                uint32_t starts = 0;                              // bit i: a field starts at p0 + i (i = 16: behind a ';' in byte 15)
                if (p0 < b) starts = (eq_mask(buf[p0 >> 4], ';') & range_mask(p0, a, b)) << 1;
                if (a >= p0 && a < p0 + 16) starts |= 1u << (a - p0);
                uint32_t my_t = kNone, my_g = kNone;
                for (uint32_t w = starts; w; w &= w - 1) {
                    const uint32_t f = p0 + (uint32_t)__ffs(w) - 1u;
                    uint32_t v;
                    if (!found_t && my_t == kNone && gt_field_has_key(get, f, b, gt_tid_key(), kGtTidKeyLen, &v)) my_t = v;
                    if (!found_g && my_g == kNone && gt_field_has_key(get, f, b, key, klen, &v)) my_g = v;
                }
                if (!found_t) {
                    const unsigned long long bt = __ballot(my_t != kNone);
                    if (bt) { v_t = __shfl(my_t, __ffsll(bt) - 1); found_t = true; }
                }
                if (!found_g) {
                    const unsigned long long bg = __ballot(my_g != kNone);
                    if (bg) { v_g = __shfl(my_g, __ffsll(bg) - 1); found_g = true; }
                }
            }
            r = gt_record_of(get, b, found_t, v_t, found_g && key_usable, v_g);
        }
    }
    if (lane == 0) {
        t_s[line] = r.t_s; t_len[line] = r.t_len; g_s[line] = r.g_s; g_len[line] = r.g_len; has[line] = r.has_key;
        isrec[line] = r.t_len ? 1u : 0u;
        if (r.flags) atomicOr(flags, r.flags);
    }
}

// the records among the lines: names 2r (id) and 2r + 1 (value) of this call, has_out[r]
__global__ void k_gtf_scatter(uint32_t L, const uint32_t* __restrict__ isrec, const uint32_t* __restrict__ rec_scan, const uint32_t* __restrict__ t_s,
                              const uint32_t* __restrict__ t_len, const uint32_t* __restrict__ g_s, const uint32_t* __restrict__ g_len,
                              const uint32_t* __restrict__ has, uint32_t* __restrict__ start, uint32_t* __restrict__ len,
                              uint32_t* __restrict__ has_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L || !isrec[i]) return;
    const uint32_t r = rec_scan[i];
    start[2 * (uint64_t)r] = t_s[i]; len[2 * (uint64_t)r] = t_len[i];
    start[2 * (uint64_t)r + 1] = g_s[i]; len[2 * (uint64_t)r + 1] = g_len[i];
    has_out[r] = has[i];
}

// name k of this call -> blob[base + scan[k] ..), off[k + 1] = base + scan[k + 1]   (off points at the entry of the call's first name)
__global__ void k_gmap_append(const unsigned char* __restrict__ bytes, uint64_t K, const uint32_t* __restrict__ start, const uint32_t* __restrict__ len,
                              const uint64_t* __restrict__ scan, uint64_t base, unsigned char* __restrict__ blob, uint64_t* __restrict__ off) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const unsigned char* src = bytes + start[k];
    unsigned char* dst = blob + base + scan[k];
    const uint32_t n = len[k];
    for (uint32_t i = 0; i < n; ++i) dst[i] = src[i];
    off[k + 1] = base + scan[k + 1];
}

// ---- the string sort (ranksort.h) ------------------------------------------------------------------------------------------

// the names of the handle: name 2 * rec + which of record rec = sel[item] (sel == null: the item itself); kNone: the empty name
struct Names {
    const unsigned char* blob;
    const uint64_t* off;
    const uint32_t* sel;
    uint32_t which;
    __device__ void span(uint32_t item, uint64_t* s, uint64_t* n) const {
        const uint32_t rec = sel ? sel[item] : item;
        if (rec == kNone) { *s = 0; *n = 0; return; }
        const uint64_t k = 2 * (uint64_t)rec + which;
        *s = off[k]; *n = off[k + 1] - off[k];
    }
    // ranksort.h's view of the names
    __device__ uint64_t key(uint32_t item, uint32_t round) const {
        uint64_t s, len, k = 0;
        span(item, &s, &len);
        const uint64_t at = 8ull * round;
        for (uint32_t i = 0; i < 8; ++i) k = (k << 8) | (at + i < len ? blob[s + at + i] : 0u);
        return k;
    }
    __device__ uint64_t bytes(uint32_t item) const {
        uint64_t s, len;
        span(item, &s, &len);
        return len;
    }
};

using ranksort::RankScratch;
using ranksort::rank_strings;

// ---- finish ---------------------------------------------------------------------------------------------------------------

// GTF: per run of equal ids, the position of its head and the first position (file order) whose record carries the key
__global__ void k_gtf_first(uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ run, const uint32_t* __restrict__ has,
                            uint32_t* __restrict__ head_pos, uint32_t* __restrict__ first_pos) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = run[j];
    if (j == 0 || run[j - 1] != r) head_pos[r] = j;
    if (has[perm[j]]) atomicMin(&first_pos[r], j);
}

__global__ void k_gtf_pick(uint32_t T, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ head_pos, const uint32_t* __restrict__ first_pos,
                           uint32_t* __restrict__ ts, uint32_t* __restrict__ gs) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    ts[t] = perm[head_pos[t]];
    gs[t] = first_pos[t] == kNone ? kNone : perm[first_pos[t]];
}

// the first item (in item order) of every distinct gene value: first[item] = 1
__global__ void k_gene_first(uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ run, uint32_t* __restrict__ first) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (j == 0 || run[j - 1] != run[j]) first[perm[j]] = 1;
}

// the id of a run = the flags in front of its first item; gene_src[id] = the record whose value names the gene
__global__ void k_gene_ids(uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ run, const uint32_t* __restrict__ first_scan,
                           const uint32_t* __restrict__ gs, uint32_t* __restrict__ id_of_run, uint32_t* __restrict__ gene_src) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    if (j == 0 || run[j - 1] != run[j]) {
        const uint32_t id = first_scan[perm[j]];
        id_of_run[run[j]] = id;
        gene_src[id] = gs ? gs[perm[j]] : perm[j];
    }
}

__global__ void k_gene_assign(uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ run, const uint32_t* __restrict__ id_of_run,
                              uint32_t* __restrict__ gid) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) gid[perm[j]] = id_of_run[run[j]];
}

// two-column form: the items in sorted order
__global__ void k_tsv_order(uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ gid, uint32_t* __restrict__ ts,
                            uint32_t* __restrict__ t2g) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    ts[j] = perm[j]; t2g[j] = gid[perm[j]];
}

__global__ void k_name_len(Names nm, uint32_t n, uint32_t* __restrict__ len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t s, l;
    nm.span(i, &s, &l);
    len[i] = (uint32_t)l;
}

__global__ void k_name_copy(Names nm, uint32_t n, const uint64_t* __restrict__ scan, unsigned char* __restrict__ out, uint64_t* __restrict__ off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    off[i] = scan[i];
    if (i == n) return;
    uint64_t s, l;
    nm.span(i, &s, &l);
    for (uint64_t k = 0; k < l; ++k) out[scan[i] + k] = nm.blob[s + k];
}

// ---- lookup ---------------------------------------------------------------------------------------------------------------

// is name a (bytes, a prefix first) below name b?
__device__ inline bool name_less(const unsigned char* a, uint64_t na, const unsigned char* b, uint64_t nb) {
    const uint64_t n = na < nb ? na : nb;
    for (uint64_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return a[i] < b[i];
    return na < nb;
}

__global__ void k_gmap_lookup(const unsigned char* __restrict__ tn, const uint64_t* __restrict__ tn_off, const uint32_t* __restrict__ t2g, uint32_t T,
                              const unsigned char* __restrict__ names, const uint64_t* __restrict__ name_off, uint64_t n_rows,
                              uint32_t* __restrict__ gene_of_row, unsigned long long* __restrict__ n_past) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const unsigned char* q = names + name_off[r];
    const uint64_t nq = name_off[r + 1] - name_off[r];
    uint32_t lo = 0, hi = T;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (name_less(tn + tn_off[mid], tn_off[mid + 1] - tn_off[mid], q, nq)) lo = mid + 1; else hi = mid;
    }
    if (lo < T) { gene_of_row[r] = t2g[lo]; return; }
    gene_of_row[r] = kNone;
    atomicAdd(n_past, 1ull);
}

struct AddScratch {
    DevBuf<uint4> text;
    DevBuf<uint32_t> nl_cnt, nl_scan, tok_cnt, tok_scan, line_end, t_s, t_len, g_s, g_len, has, isrec, rec_scan, start, len, misc;
    DevBuf<uint64_t> len_scan;
};

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

struct sfgpu_gmap {
    int kind = SFGPU_GMAP_GTF;
    bool finished = false;
    uint32_t flags = 0;
    uint32_t key_len = 0;
    bool key_usable = false;
    DevBuf<unsigned char> key;
    // the names of the records: GTF (id, value) per record, two-column form the tokens; name k = blob[off[k] .. off[k + 1])
    DevBuf<unsigned char> blob;
    DevBuf<uint64_t> off;
    DevBuf<uint32_t> has;                   // GTF: per record
    uint64_t n_names = 0, blob_bytes = 0;
    // the tables
    DevBuf<unsigned char> tn, gn;
    DevBuf<uint64_t> tn_off, gn_off;
    DevBuf<uint32_t> t2g;
    uint64_t T = 0, G = 0, tn_bytes = 0, gn_bytes = 0;
};

namespace {

// the text on the device: [0, n_text) ends in a '\n' (whole lines), flags are looked for below n_flag
int add_device_text(sfgpu_gmap* m, AddScratch& S, const uint4* text, uint64_t n_text, uint64_t n_flag, sfgpu_gmap_add_result* res, hipStream_t st,
                    uint32_t* h) {
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(text);
    const uint64_t n_groups = (n_text + 15) / 16;
    const bool tsv = m->kind == SFGPU_GMAP_TSV;
    if (int r = S.misc.reserve(4, st, false)) return r;
    if (int r = S.nl_cnt.reserve(n_groups + 2, st, false)) return r;
    if (int r = S.nl_scan.reserve(n_groups + 2, st, false)) return r;
    if (tsv) {
        if (int r = S.tok_cnt.reserve(n_groups + 2, st, false)) return r;
        if (int r = S.tok_scan.reserve(n_groups + 2, st, false)) return r;
    }
    SF_HIP(hipMemsetAsync(S.misc.p, 0, 16, st));
    hipLaunchKernelGGL(k_gmap_count, dim3(grid_of(n_groups)), dim3(kBlock), 0, st, text, n_groups, n_text, n_flag, S.nl_cnt.p,
                       tsv ? S.tok_cnt.p : nullptr, S.misc.p);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(S.nl_cnt.p, S.nl_scan.p, n_groups, st)) return r;
    if (tsv) if (int r = exclusive_scan_u32_u32(S.tok_cnt.p, S.tok_scan.p, n_groups, st)) return r;
    SF_HIP(hipMemcpyAsync(&h[0], S.nl_scan.p + n_groups, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h[1], S.misc.p, 4, hipMemcpyDeviceToHost, st));
    if (tsv) SF_HIP(hipMemcpyAsync(&h[2], S.tok_scan.p + n_groups, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t L = h[0];
    res->n_lines = L;
    auto flagged = [&](uint32_t f) { m->flags |= f; res->needs_host = m->flags; return SFGPU_OK; };
    if (h[1]) return flagged(h[1]);

    uint64_t K = 0;                                        // names this call adds
    if (tsv) {
        K = h[2];
        if (K == 0) return SFGPU_OK;
        if (int r = S.start.reserve(K + 2, st, false)) return r;
        if (int r = S.len.reserve(K + 2, st, false)) return r;
        hipLaunchKernelGGL(k_tsv_tokens, dim3(grid_of(n_groups)), dim3(kBlock), 0, st, bytes, n_groups, n_text, S.tok_scan.p, S.start.p, S.len.p, S.misc.p);
        SF_CHECK_LAUNCH();
    } else {
        if (L == 0) return SFGPU_OK;
        for (DevBuf<uint32_t>* b : {&S.line_end, &S.t_s, &S.t_len, &S.g_s, &S.g_len, &S.has, &S.isrec, &S.rec_scan})
            if (int r = b->reserve((uint64_t)L + 2, st, false)) return r;
        hipLaunchKernelGGL(k_gmap_line_ends, dim3(grid_of(n_groups)), dim3(kBlock), 0, st, text, n_groups, n_text, S.nl_scan.p, S.line_end.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_gtf_lines, dim3((L + kLinesPerBlock - 1) / kLinesPerBlock), dim3(kBlock), 0, st, text, L, S.line_end.p, m->key.p,
                           m->key_len, m->key_usable ? 1 : 0, S.t_s.p, S.t_len.p, S.g_s.p, S.g_len.p, S.has.p, S.isrec.p, S.misc.p);
        SF_CHECK_LAUNCH();
        if (int r = exclusive_scan_u32_u32(S.isrec.p, S.rec_scan.p, L, st)) return r;
        SF_HIP(hipMemcpyAsync(&h[2], S.rec_scan.p + L, 4, hipMemcpyDeviceToHost, st));
    }
    SF_HIP(hipMemcpyAsync(&h[1], S.misc.p, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h[1]) return flagged(h[1]);
    if (!tsv) {
        const uint64_t R = h[2];
        if (R == 0) return SFGPU_OK;
        K = 2 * R;
        SF_REQUIRE(m->n_names / 2 + R <= 0xffffffffull - 1, SFGPU_ERR_RANGE, "sfgpu_gmap_add_text: more than 2^32 - 1 records");
        if (int r = S.start.reserve(K + 2, st, false)) return r;
        if (int r = S.len.reserve(K + 2, st, false)) return r;
        if (int r = m->has.reserve(m->n_names / 2 + R, st, true, m->n_names / 2)) return r;
        hipLaunchKernelGGL(k_gtf_scatter, dim3(grid_of(L)), dim3(kBlock), 0, st, L, S.isrec.p, S.rec_scan.p, S.t_s.p, S.t_len.p, S.g_s.p, S.g_len.p,
                           S.has.p, S.start.p, S.len.p, m->has.p + m->n_names / 2);
        SF_CHECK_LAUNCH();
        res->n_records = R;
    } else {
        SF_REQUIRE((m->n_names + K) / 2 <= 0xffffffffull - 1, SFGPU_ERR_RANGE, "sfgpu_gmap_add_text: more than 2^32 - 1 pairs");
        res->n_records = K;
    }
    // ---- the names into the handle
    if (int r = S.len_scan.reserve(K + 2, st, false)) return r;
    if (int r = exclusive_scan_u32(S.len.p, S.len_scan.p, K, st, false)) return r;
    uint64_t* h_total = reinterpret_cast<uint64_t*>(&h[4]);
    SF_HIP(hipMemcpyAsync(h_total, S.len_scan.p + K, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint64_t add_bytes = *h_total;
    if (int r = m->blob.reserve(m->blob_bytes + add_bytes + 1, st, true, m->blob_bytes)) return r;
    if (int r = m->off.reserve(m->n_names + K + 1, st, true, m->n_names + 1)) return r;
    hipLaunchKernelGGL(k_gmap_append, dim3(grid_of(K)), dim3(kBlock), 0, st, bytes, K, S.start.p, S.len.p, S.len_scan.p, m->blob_bytes, m->blob.p,
                       m->off.p + m->n_names);
    SF_CHECK_LAUNCH();
    SF_HIP(hipStreamSynchronize(st));
    m->n_names += K;
    m->blob_bytes += add_bytes;
    return SFGPU_OK;
}

// names 0 .. n of nm, back to back
int build_names(Names nm, uint32_t n, DevBuf<unsigned char>& out, DevBuf<uint64_t>& off, uint64_t* n_bytes, DevBuf<uint32_t>& len,
                DevBuf<uint64_t>& scan, uint64_t* h_total, hipStream_t st) {
    if (int r = len.reserve((uint64_t)n + 2, st, false)) return r;
    if (int r = scan.reserve((uint64_t)n + 2, st, false)) return r;
    if (int r = off.reserve((uint64_t)n + 1, st, false)) return r;
    if (n) {
        hipLaunchKernelGGL(k_name_len, dim3(grid_of(n)), dim3(kBlock), 0, st, nm, n, len.p);
        SF_CHECK_LAUNCH();
    }
    if (int r = exclusive_scan_u32(len.p, scan.p, n, st, false)) return r;
    SF_HIP(hipMemcpyAsync(h_total, scan.p + n, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    *n_bytes = *h_total;
    if (int r = out.reserve(*n_bytes + 1, st, false)) return r;
    hipLaunchKernelGGL(k_name_copy, dim3(grid_of((uint64_t)n + 1)), dim3(kBlock), 0, st, nm, n, scan.p, out.p, off.p);
    SF_CHECK_LAUNCH();
    return SFGPU_OK;
}

}  // namespace

extern "C" int sfgpu_gmap_open(sfgpu_gmap** out, int kind, const char* key, uint32_t key_len) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_gmap_open: null handle");
    SF_REQUIRE(kind == SFGPU_GMAP_GTF || kind == SFGPU_GMAP_TSV, SFGPU_ERR_INVALID, "sfgpu_gmap_open: kind is neither GTF nor TSV");
    SF_REQUIRE(key || key_len == 0, SFGPU_ERR_INVALID, "sfgpu_gmap_open: null key");
    sfgpu_gmap* m = new sfgpu_gmap;
    m->kind = kind;
    m->key_len = key_len;
    m->key_usable = kind == SFGPU_GMAP_GTF && gt_key_usable(reinterpret_cast<const unsigned char*>(key), key_len);
    int rc = m->key.reserve((uint64_t)key_len + 1, nullptr, false);
    if (rc == SFGPU_OK) rc = m->off.reserve(1, nullptr, false);
    if (rc == SFGPU_OK) {
        hipError_t e = hipMemsetAsync(m->off.p, 0, sizeof(uint64_t), nullptr);
        if (e == hipSuccess && key_len) e = hipMemcpyAsync(m->key.p, key, key_len, hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) { set_error("sfgpu_gmap_open: %s", hipGetErrorString(e)); rc = SFGPU_ERR_HIP; }
    }
    if (rc != SFGPU_OK) { delete m; return rc; }
    *out = m;
    return SFGPU_OK;
}

extern "C" int sfgpu_gmap_from_host(sfgpu_gmap** out, const char* h_tnames, const uint64_t* h_tname_off, const uint32_t* h_t2g,
                                    uint64_t n_transcripts, const char* h_gnames, const uint64_t* h_gname_off, uint64_t n_genes) {
    SF_REQUIRE(out && h_tname_off && h_gname_off && (h_t2g || n_transcripts == 0), SFGPU_ERR_INVALID, "sfgpu_gmap_from_host: null argument");
    SF_REQUIRE(n_transcripts <= 0xffffffffull - 1 && n_genes <= 0xffffffffull - 1, SFGPU_ERR_RANGE, "sfgpu_gmap_from_host: more than 2^32 - 1 names");
    const uint64_t tb = h_tname_off[n_transcripts], gb = h_gname_off[n_genes];
    SF_REQUIRE(h_tname_off[0] == 0 && h_gname_off[0] == 0 && (h_tnames || tb == 0) && (h_gnames || gb == 0), SFGPU_ERR_INVALID,
               "sfgpu_gmap_from_host: offsets must start at 0 over non-null names");
    for (uint64_t g = 0; g < n_genes; ++g)
        SF_REQUIRE(h_gname_off[g] <= h_gname_off[g + 1], SFGPU_ERR_INVALID, "sfgpu_gmap_from_host: gene name offsets decrease");
    for (uint64_t t = 0; t < n_transcripts; ++t) {
        SF_REQUIRE(h_tname_off[t] <= h_tname_off[t + 1] && h_t2g[t] < n_genes, SFGPU_ERR_INVALID,
                   "sfgpu_gmap_from_host: transcript name offsets decrease, or a gene id is not below n_genes");
        if (t == 0) continue;
        const uint64_t na = h_tname_off[t] - h_tname_off[t - 1], nb = h_tname_off[t + 1] - h_tname_off[t];
        const int c = memcmp(h_tnames + h_tname_off[t - 1], h_tnames + h_tname_off[t], na < nb ? na : nb);
        SF_REQUIRE(c < 0 || (c == 0 && na <= nb), SFGPU_ERR_INVALID, "sfgpu_gmap_from_host: the transcript names are not sorted bytewise");
    }
    sfgpu_gmap* m = new sfgpu_gmap;
    int rc = m->tn.reserve(tb + 1, nullptr, false);
    if (rc == SFGPU_OK) rc = m->gn.reserve(gb + 1, nullptr, false);
    if (rc == SFGPU_OK) rc = m->tn_off.reserve(n_transcripts + 1, nullptr, false);
    if (rc == SFGPU_OK) rc = m->gn_off.reserve(n_genes + 1, nullptr, false);
    if (rc == SFGPU_OK) rc = m->t2g.reserve(n_transcripts + 1, nullptr, false);
    if (rc == SFGPU_OK) {
        hipError_t e = hipMemcpy(m->tn_off.p, h_tname_off, (n_transcripts + 1) * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(m->gn_off.p, h_gname_off, (n_genes + 1) * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess && tb) e = hipMemcpy(m->tn.p, h_tnames, tb, hipMemcpyHostToDevice);
        if (e == hipSuccess && gb) e = hipMemcpy(m->gn.p, h_gnames, gb, hipMemcpyHostToDevice);
        if (e == hipSuccess && n_transcripts) e = hipMemcpy(m->t2g.p, h_t2g, n_transcripts * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("sfgpu_gmap_from_host: %s", hipGetErrorString(e)); rc = SFGPU_ERR_HIP; }
    }
    if (rc != SFGPU_OK) { delete m; return rc; }
    m->T = n_transcripts; m->G = n_genes; m->tn_bytes = tb; m->gn_bytes = gb; m->finished = true;
    *out = m;
    return SFGPU_OK;
}

extern "C" int sfgpu_gmap_close(sfgpu_gmap* m) {
    if (!m) return SFGPU_OK;
    (void)hipDeviceSynchronize();
    delete m;
    return SFGPU_OK;
}

extern "C" int sfgpu_gmap_add_text_host(sfgpu_gmap* m, const char* h_text, uint64_t n_bytes, int final, sfgpu_gmap_add_result* res,
                                        sfgpu_stream stream) {
    SF_REQUIRE(m && res, SFGPU_ERR_INVALID, "sfgpu_gmap_add_text_host: null handle or result");
    memset(res, 0, sizeof(*res));
    res->needs_host = m->flags;
    SF_REQUIRE(!m->finished, SFGPU_ERR_STATE, "sfgpu_gmap_add_text_host: the map is finished");
    SF_REQUIRE(n_bytes <= kMaxBytes, SFGPU_ERR_RANGE, "sfgpu_gmap_add_text_host: more than 2^30 bytes in one call");
    SF_REQUIRE(n_bytes == 0 || h_text, SFGPU_ERR_INVALID, "sfgpu_gmap_add_text_host: null text");
    uint64_t used = n_bytes;
    if (!final) while (used && h_text[used - 1] != '\n') --used;
    if (used == 0) {
        SF_REQUIRE(final || n_bytes == 0, SFGPU_ERR_RANGE, "sfgpu_gmap_add_text_host: no line ends within the text");
        return SFGPU_OK;
    }
    res->consumed = used;
    if (m->flags) return SFGPU_OK;                           // flagged: the host reader takes the file
    const bool append = h_text[used - 1] != '\n';            // (final only)
    const uint64_t n_text = used + (append ? 1 : 0), n_groups = (n_text + 15) / 16, n_sub = (used + kSubBytes - 1) / kSubBytes;
    hipStream_t st = as_stream(stream);

    AddScratch S;
    CallScope scope;        // after S: it drains both streams before S's blocks go back to the pool
    hipStream_t cs = nullptr;
    char* pinned[2] = {nullptr, nullptr};
    hipEvent_t ev_slot[2] = {nullptr, nullptr}, ev_c0 = nullptr, ev_c1 = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;
    uint32_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.acquire(&cs));
    for (int b = 0; b < 2 && (uint64_t)b < n_sub; ++b) {
        SF_HIP(scope.pinned_block(&pinned[b], (used < kSubBytes ? used : kSubBytes) + 48));
        SF_HIP(scope.event(&ev_slot[b]));
    }
    for (hipEvent_t* e : {&ev_c0, &ev_c1, &ev_k0, &ev_k1}) SF_HIP(scope.event(e));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint32_t)));
    if (int r = S.text.reserve(n_groups + 1, st, false)) return r;
    SF_HIP(hipEventRecord(ev_k0, st));
    SF_HIP(hipStreamWaitEvent(cs, ev_k0, 0));                // the copies stay behind whatever `stream` held and behind the reservation
    SF_HIP(hipEventRecord(ev_c0, cs));
    for (uint64_t c = 0; c < n_sub; ++c) {
        const int slot = (int)(c & 1);
        if (c >= 2) SF_HIP(hipEventSynchronize(ev_slot[slot]));      // its previous copy has left the pinned buffer
        const uint64_t p = c * kSubBytes, q = (c + 1 == n_sub) ? used : p + kSubBytes;
        uint64_t n = q - p;
        memcpy(pinned[slot], h_text + p, n);
        if (c + 1 == n_sub) {
            if (append) pinned[slot][n++] = '\n';
            const uint64_t padded = (n + 15) & ~15ull;
            memset(pinned[slot] + n, 0, padded - n);
            n = padded;
        }
        SF_HIP(hipMemcpyAsync(reinterpret_cast<char*>(S.text.p) + p, pinned[slot], n, hipMemcpyHostToDevice, cs));
        SF_HIP(hipEventRecord(ev_slot[slot], cs));
    }
    SF_HIP(hipEventRecord(ev_c1, cs));
    SF_HIP(hipStreamWaitEvent(st, ev_c1, 0));
    SF_HIP(hipEventRecord(ev_k0, st));
    const int rc = add_device_text(m, S, S.text.p, n_text, used, res, st, h);
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_copy, ev_c0, ev_c1);
    add_elapsed(&res->ms_kernels, ev_k0, ev_k1);
    return rc;
}

extern "C" int sfgpu_gmap_add_text_device(sfgpu_gmap* m, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final,
                                          sfgpu_gmap_add_result* res, sfgpu_stream stream) {
    SF_REQUIRE(m && res, SFGPU_ERR_INVALID, "sfgpu_gmap_add_text_device: null handle or result");
    memset(res, 0, sizeof(*res));
    res->needs_host = m->flags;
    SF_REQUIRE(!m->finished, SFGPU_ERR_STATE, "sfgpu_gmap_add_text_device: the map is finished");
    SF_REQUIRE(n_bytes <= kMaxBytes, SFGPU_ERR_RANGE, "sfgpu_gmap_add_text_device: more than 2^30 bytes in one call");
    SF_REQUIRE(n_bytes == 0 || d_text, SFGPU_ERR_INVALID, "sfgpu_gmap_add_text_device: null text");
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_gmap_add_text_device: d_text must be 16-byte aligned");
    SF_REQUIRE(n_bytes == 0 || cap_text >= ((n_bytes + 1 + 15) & ~15ull) + 16, SFGPU_ERR_INVALID,
               "sfgpu_gmap_add_text_device: cap_text must hold the text, a '\\n', the rest of that 16-byte group and one group more");
    if (n_bytes == 0) return SFGPU_OK;
    hipStream_t st = as_stream(stream);
    AddScratch S;
    CallScope scope;        // after S, as in sfgpu_gmap_add_text_host
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;
    uint32_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_k0));
    SF_HIP(scope.event(&ev_k1));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint32_t)));
    DevBuf<unsigned long long> last;
    if (int r = last.reserve(1, st, false)) return r;
    SF_HIP(hipEventRecord(ev_k0, st));
    SF_HIP(hipMemsetAsync(last.p, 0, 8, st));
    hipLaunchKernelGGL(textlines::k_last_nl, dim3(grid_of((n_bytes + 15) / 16)), dim3(kBlock), 0, st, d_text, n_bytes, last.p);
    SF_CHECK_LAUNCH();
    unsigned long long* h_last = reinterpret_cast<unsigned long long*>(&h[6]);
    SF_HIP(hipMemcpyAsync(h_last, last.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    uint64_t used = final ? n_bytes : *h_last;
    int rc = SFGPU_OK;
    if (used == 0) {
        set_error("sfgpu_gmap_add_text_device: no line ends within the text");
        rc = SFGPU_ERR_RANGE;
    } else {
        res->consumed = used;
        if (!m->flags) {
            uint64_t n_text = used;
            if (*h_last != n_bytes && final) {               // the last line lacks its '\n': it goes into the slack
                SF_HIP(hipMemsetAsync(d_text + n_bytes, '\n', 1, st));
                n_text = n_bytes + 1;
            }
            rc = add_device_text(m, S, reinterpret_cast<const uint4*>(d_text), n_text, used, res, st, h);
        }
    }
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_kernels, ev_k0, ev_k1);
    return rc;
}

extern "C" int sfgpu_gmap_finish(sfgpu_gmap* m, sfgpu_gmap_result* res, sfgpu_stream stream) {
    SF_REQUIRE(m && res, SFGPU_ERR_INVALID, "sfgpu_gmap_finish: null handle or result");
    memset(res, 0, sizeof(*res));
    res->needs_host = m->flags;
    SF_REQUIRE(!m->finished, SFGPU_ERR_STATE, "sfgpu_gmap_finish: the map is finished already");
    SF_REQUIRE(m->flags == 0, SFGPU_ERR_STATE, "sfgpu_gmap_finish: the file holds what only the host reader parses (needs_host)");
    hipStream_t st = as_stream(stream);
    const bool tsv = m->kind == SFGPU_GMAP_TSV;
    const uint32_t N = (uint32_t)(m->n_names / 2);          // records / pairs (a trailing odd token is dropped)
    res->n_records = N;

    RankScratch R;
    DevBuf<uint32_t> perm, run, head_pos, first_pos, ts, gs, first, first_scan, id_of_run, gene_src, gid, len;
    DevBuf<uint64_t> scan;
    CallScope scope;        // after the scratch: it drains the stream before the blocks go back to the pool
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint32_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev0));
    SF_HIP(scope.event(&ev1));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint32_t)));
    uint64_t* h_total = reinterpret_cast<uint64_t*>(&h[4]);
    SF_HIP(hipEventRecord(ev0, st));

    const Names ids{m->blob.p, m->off.p, nullptr, 0};
    uint32_t items = N;                                      // what the genes are numbered over: GTF the distinct transcripts, sorted
    const uint32_t* d_ts = nullptr;                          // item -> record of its transcript name (null: itself)
    const uint32_t* d_gs = nullptr;                          // item -> record of its gene value (null: itself; kNone: "")
    if (!tsv) {
        uint32_t T = 0;
        if (int r = rank_strings(ids, N, R, perm, run, &T, &res->sort_rounds, h, st)) return r;
        items = T;
        for (DevBuf<uint32_t>* b : {&head_pos, &first_pos, &ts, &gs}) if (int r = b->reserve((uint64_t)T + 2, st, false)) return r;
        if (T) {
            SF_HIP(hipMemsetAsync(first_pos.p, 0xff, (uint64_t)T * 4, st));
            hipLaunchKernelGGL(k_gtf_first, dim3(grid_of(N)), dim3(kBlock), 0, st, N, perm.p, run.p, m->has.p, head_pos.p, first_pos.p);
            SF_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_gtf_pick, dim3(grid_of(T)), dim3(kBlock), 0, st, T, perm.p, head_pos.p, first_pos.p, ts.p, gs.p);
            SF_CHECK_LAUNCH();
            SF_HIP(hipStreamSynchronize(st));                // perm and run are reused by the next sort
        }
        d_ts = ts.p; d_gs = gs.p;
    }
    // ---- genes: numbered by first appearance among the items
    uint32_t G = 0;
    if (int r = rank_strings(Names{m->blob.p, m->off.p, d_gs, 1}, items, R, perm, run, &G, nullptr, h, st)) return r;
    for (DevBuf<uint32_t>* b : {&first, &first_scan, &id_of_run, &gene_src, &gid}) if (int r = b->reserve((uint64_t)items + 2, st, false)) return r;
    if (int r = m->t2g.reserve((uint64_t)items + 1, st, false)) return r;
    if (items) {
        SF_HIP(hipMemsetAsync(first.p, 0, ((uint64_t)items + 1) * 4, st));
        hipLaunchKernelGGL(k_gene_first, dim3(grid_of(items)), dim3(kBlock), 0, st, items, perm.p, run.p, first.p);
        SF_CHECK_LAUNCH();
        if (int r = exclusive_scan_u32_u32(first.p, first_scan.p, items, st)) return r;
        hipLaunchKernelGGL(k_gene_ids, dim3(grid_of(items)), dim3(kBlock), 0, st, items, perm.p, run.p, first_scan.p, d_gs, id_of_run.p, gene_src.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_gene_assign, dim3(grid_of(items)), dim3(kBlock), 0, st, items, perm.p, run.p, id_of_run.p, tsv ? gid.p : m->t2g.p);
        SF_CHECK_LAUNCH();
        SF_HIP(hipStreamSynchronize(st));
    }
    // ---- two-column form: the pairs in a stable sort by transcript name
    if (tsv) {
        uint32_t distinct = 0;
        if (int r = rank_strings(ids, items, R, perm, run, &distinct, &res->sort_rounds, h, st)) return r;
        if (int r = ts.reserve((uint64_t)items + 2, st, false)) return r;
        if (items) {
            hipLaunchKernelGGL(k_tsv_order, dim3(grid_of(items)), dim3(kBlock), 0, st, items, perm.p, gid.p, ts.p, m->t2g.p);
            SF_CHECK_LAUNCH();
        }
        d_ts = ts.p;
    }
    // ---- the tables
    if (int r = build_names(Names{m->blob.p, m->off.p, d_ts, 0}, items, m->tn, m->tn_off, &m->tn_bytes, len, scan, h_total, st)) return r;
    if (int r = build_names(Names{m->blob.p, m->off.p, gene_src.p, 1}, G, m->gn, m->gn_off, &m->gn_bytes, len, scan, h_total, st)) return r;
    SF_HIP(hipEventRecord(ev1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_kernels, ev0, ev1);
    m->T = items; m->G = G; m->finished = true;
    res->n_transcripts = items; res->n_genes = G; res->tname_bytes = m->tn_bytes; res->gname_bytes = m->gn_bytes;
    return SFGPU_OK;
}

extern "C" int sfgpu_gmap_export(sfgpu_gmap* m, char* d_tnames, uint64_t* d_tname_off, uint32_t* d_t2g, char* d_gnames, uint64_t* d_gname_off,
                                 sfgpu_stream stream) {
    SF_REQUIRE(m, SFGPU_ERR_INVALID, "sfgpu_gmap_export: null handle");
    SF_REQUIRE(m->finished, SFGPU_ERR_STATE, "sfgpu_gmap_export: the map is not finished");
    hipStream_t st = as_stream(stream);
    if (d_tnames && m->tn_bytes) SF_HIP(hipMemcpyAsync(d_tnames, m->tn.p, m->tn_bytes, hipMemcpyDeviceToDevice, st));
    if (d_tname_off) SF_HIP(hipMemcpyAsync(d_tname_off, m->tn_off.p, (m->T + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    if (d_t2g && m->T) SF_HIP(hipMemcpyAsync(d_t2g, m->t2g.p, m->T * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (d_gnames && m->gn_bytes) SF_HIP(hipMemcpyAsync(d_gnames, m->gn.p, m->gn_bytes, hipMemcpyDeviceToDevice, st));
    if (d_gname_off) SF_HIP(hipMemcpyAsync(d_gname_off, m->gn_off.p, (m->G + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    SF_HIP(hipStreamSynchronize(st));
    return SFGPU_OK;
}

extern "C" int sfgpu_gmap_lookup(sfgpu_gmap* m, const char* d_names, const uint64_t* d_name_off, uint64_t n_rows, uint32_t* d_gene_of_row,
                                 uint64_t* n_past, sfgpu_stream stream) {
    SF_REQUIRE(m && n_past, SFGPU_ERR_INVALID, "sfgpu_gmap_lookup: null handle or counter");
    *n_past = 0;
    SF_REQUIRE(m->finished, SFGPU_ERR_STATE, "sfgpu_gmap_lookup: the map is not finished");
    if (n_rows == 0) return SFGPU_OK;
    SF_REQUIRE(d_name_off && d_gene_of_row, SFGPU_ERR_INVALID, "sfgpu_gmap_lookup: null array");
    hipStream_t st = as_stream(stream);
    DevBuf<unsigned long long> past;
    CallScope scope;
    unsigned long long* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.pinned_block(&h, sizeof(unsigned long long)));
    if (int r = past.reserve(1, st, false)) return r;
    SF_HIP(hipMemsetAsync(past.p, 0, 8, st));
    hipLaunchKernelGGL(k_gmap_lookup, dim3(grid_of(n_rows)), dim3(kBlock), 0, st, m->tn.p, m->tn_off.p, m->t2g.p, (uint32_t)m->T,
                       reinterpret_cast<const unsigned char*>(d_names), d_name_off, n_rows, d_gene_of_row, past.p);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(h, past.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    *n_past = *h;
    return SFGPU_OK;
}
