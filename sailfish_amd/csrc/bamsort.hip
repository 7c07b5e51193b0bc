// bamsort.hip -- the coordinate-sorted BAM file and its BAI index, written from the device: sfgpu_bamsort_open / _collect / _finish /
// _close.  WHAT the file and the index say is baifmt.h (order, member cut, virtual offsets, chunks, linear index, layout); this file
// keeps the records, orders them and builds the index.
//   collect  the batch of sfgpu_sam_write_bgzf goes through samtext_write.hip's own checks, sizing, scan and k_format_units<BamFmt>
//            (bamsort.h) into ONE device segment per batch: nothing already stored is ever moved.  k_unit_records counts the records
//            of every unit (the second record of a pair unit starts 4 + block_size behind the first), a scan numbers them, and
//            k_append, one lane per unit, lists key, 64-bit address and length of each.
//   finish   one stable sort_pairs_u64_u32 of (key, index); the lengths in sorted order, scanned to 64-bit stream starts; k_gather
//            makes the sorted stream a piece at a time -- one lane per 16-byte group of the piece finds its record by binary search,
//            reads 16 source bytes at any alignment (two aligned loads and funnel shifts) or assembles a group that straddles
//            records in registers, and issues one aligned 16-byte store -- and each piece (a multiple of kBaiMember bytes but the
//            last) goes to sfgpu_bgzw_write_device while the next one is gathered: the extra memory is two pieces.
//   index    behind the last member: the members' offsets are a scan of the encoder's tracked sizes; k_index_records, one lane per
//            sorted record, computes extent, bin, vbeg, vend (and n_intv by atomicMax, the 0x4 count by atomicAdd); k_heads flags
//            the run heads, a scan numbers the chunks, k_chunks fills them, a stable sort by (refID << 32 | bin) groups them into
//            bins; k_bin_heads + scan number the bins; k_ref_sizes (one lane per reference, binary searches, no atomics) sizes the
//            references and a scan places them; k_windows lowers the linear index with 64-bit atomicMin; k_write_chunks,
//            k_write_bins and k_write_refs (which also backfills its reference's windows from the right, at most kBaiMaxWindows)
//            store the index as 32-bit words at the scanned offsets.  The bytes go to their sink through textchunks.h.
// No workgroup waits for another; every loop is bounded: binary searches by 64 steps, a record's CIGAR by 65 535 words, a group's
// assembly by 16 bytes, a record's windows and a reference's backfill by kBaiMaxWindows.
// Device memory: the records + 20 B per record while collecting; finish adds 28 B per record for the order and the stream starts,
// 40 B per record and 28 B per chunk for the index, and two pieces.  Nothing is spilled to the host.
#include "common.h"
#include "primitives.h"
#include "baifmt.h"
#include "bamsort.h"
#include "textchunks.h"

#include <new>
#include <vector>

namespace sfgpu {
namespace {

constexpr int kBlock = 256;
constexpr uint64_t kSegSlack = 48;                        // k_format_units stores whole 16-byte groups; k_gather reads 32 aligned bytes
constexpr uint64_t kDefaultPiece = 32ull << 20;
constexpr uint64_t kNoValue = ~0ull;
inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// the first i in [0, n) with a[i] >= x, n when there is none
__device__ inline uint64_t lower_bound(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_iota(uint32_t* __restrict__ v, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

// ---- collect
__global__ void k_unit_records(const uint8_t* __restrict__ seg, const uint64_t* __restrict__ unit_start, uint64_t n_units, uint32_t* __restrict__ cnt) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_units) return;
    const uint64_t s = unit_start[u], len = unit_start[u + 1] - s;
    cnt[u] = 4ull + bai_le32(seg + s) < len ? 2u : 1u;
}

__global__ void k_append(const uint8_t* __restrict__ seg, const uint64_t* __restrict__ unit_start, uint64_t n_units, const uint32_t* __restrict__ before,
                         uint64_t* __restrict__ key, uint64_t* __restrict__ addr, uint32_t* __restrict__ len) {
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_units) return;
    const uint64_t s = unit_start[u], e = unit_start[u + 1];
    const uint32_t k = before[u], n = before[u + 1] - k;
    const uint64_t first = 4ull + bai_le32(seg + s);
    auto put = [&](uint32_t at, uint64_t p, uint64_t l) {
        key[at] = bai_key((int32_t)bai_le32(seg + p + 4), (int32_t)bai_le32(seg + p + 8));
        addr[at] = reinterpret_cast<uint64_t>(seg + p);
        len[at] = (uint32_t)l;
    };
    put(k, s, n == 2 ? first : e - s);
    if (n == 2) put(k + 1, s + first, e - s - first);
}

// ---- finish: the order and the stream
__global__ void k_sorted_len(const uint32_t* __restrict__ len, const uint32_t* __restrict__ perm, uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = len[perm[i]];
}

__global__ void k_first_no_coor(const uint64_t* __restrict__ key_s, uint64_t n, unsigned long long* __restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = lower_bound(key_s, n, kBaiNoCoorKey);
}

// 16 bytes from p, any alignment: the two aligned groups that hold them (the second may lie behind the bytes: kSegSlack)
__device__ inline uint4 load_unaligned16(const uint8_t* p) {
    const uint64_t ad = reinterpret_cast<uint64_t>(p);
    const uint4* g = reinterpret_cast<const uint4*>(ad & ~15ull);
    const uint4 a = g[0], b = g[1];
    const uint32_t t[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t ws = (uint32_t)(ad & 15u) >> 2, bs = (uint32_t)(ad & 3u) * 8;
    uint32_t u[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) u[j] = ws == 0 ? t[j] : ws == 1 ? t[j + 1] : ws == 2 ? t[j + 2] : t[j + 3];
    uint4 v;
    v.x = __funnelshift_r(u[0], u[1], bs); v.y = __funnelshift_r(u[1], u[2], bs);
    v.z = __funnelshift_r(u[2], u[3], bs); v.w = __funnelshift_r(u[3], u[4], bs);
    return v;
}

// stream bytes [base, base + n_bytes) into out: one lane per 16-byte group; start[0 .. n] are the sorted records' stream starts
// (start[n] = the stream's bytes, base + n_bytes <= start[n]), record i lies at addr[perm[i]]; no record is empty
__global__ void __launch_bounds__(kBlock)
k_gather(const uint64_t* __restrict__ start, uint64_t n, const uint64_t* __restrict__ addr, const uint32_t* __restrict__ perm, uint64_t base,
         uint64_t n_bytes, uint4* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= (n_bytes + 15) / 16) return;
    const uint64_t o = base + 16 * g;
    const uint32_t cnt = n_bytes - 16 * g < 16 ? (uint32_t)(n_bytes - 16 * g) : 16u;
    uint64_t lo = 0, hi = n;                              // start[lo] <= o < start[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= o) lo = mid; else hi = mid;
    }
    uint64_t i = lo;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(addr[perm[i]]) + (o - start[i]);
    uint64_t avail = start[i + 1] - o;
    if (avail >= 16) {                                    // (then cnt == 16)
        out[g] = load_unaligned16(src);
        return;
    }
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < cnt;) {                      // at most 16 bytes, and a record change costs no byte but has one behind it
        if (avail == 0) {                                 // (k < cnt: a further record exists)
            ++i;
            src = reinterpret_cast<const uint8_t*>(addr[perm[i]]);
            avail = start[i + 1] - start[i];
            continue;
        }
        w[k >> 2] |= (uint32_t)*src << (8 * (k & 3));
        ++src; --avail; ++k;
    }
    out[g] = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- the index
struct IndexArrays {
    uint64_t *bin_key, *vbeg, *vend;                      // per sorted record
    uint32_t *beg, *end;
    unsigned long long* n_unmapped;                       // per reference
    uint32_t* n_intv;
};

__global__ void __launch_bounds__(kBlock)
k_index_records(const uint64_t* __restrict__ addr, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ start, uint64_t n,
                uint32_t n_refs, uint64_t first_member, const uint64_t* __restrict__ coff, uint64_t n_members, IndexArrays x) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const BaiRecord r = bai_record(reinterpret_cast<const uint8_t*>(addr[perm[i]]));
    x.vbeg[i] = bai_voffset(start[i], start[n], first_member, coff, n_members);
    x.vend[i] = bai_voffset(start[i + 1], start[n], first_member, coff, n_members);
    if (r.ref < 0 || (uint32_t)r.ref >= n_refs) { x.bin_key[i] = kNoValue; x.beg[i] = 0; x.end[i] = 0; return; }
    x.bin_key[i] = bai_bin_key(r);
    x.beg[i] = r.beg; x.end[i] = r.end;
    uint32_t w1 = (r.end - 1u) >> kBaiWindowShift;
    if (w1 >= kBaiMaxWindows) w1 = kBaiMaxWindows - 1;    // (bamwfmt.h's rule 5: cannot happen)
    atomicMax(&x.n_intv[r.ref], w1 + 1u);
    if (r.flag & 4u) atomicAdd(&x.n_unmapped[r.ref], 1ull);
}

__global__ void k_heads(const uint64_t* __restrict__ bin_key, uint64_t n, uint32_t* __restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) head[i] = bin_key[i] != kNoValue && (i == 0 || bin_key[i - 1] != bin_key[i]);
}

// cid: the exclusive scan of the heads.  The head of a run writes its chunk's key and start, the last record of the run its end
__global__ void k_chunks(const uint64_t* __restrict__ bin_key, const uint64_t* __restrict__ vbeg, const uint64_t* __restrict__ vend,
                         const uint32_t* __restrict__ cid, uint64_t n, uint64_t* __restrict__ ckey, uint64_t* __restrict__ cbeg, uint64_t* __restrict__ cend) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || bin_key[i] == kNoValue) return;
    const bool head = cid[i + 1] != cid[i];
    const uint32_t c = head ? cid[i] : cid[i] - 1u;       // (a record that is no head has a head in front of it)
    if (head) { ckey[c] = bin_key[i]; cbeg[c] = vbeg[i]; }
    if (i + 1 == n || bin_key[i + 1] != bin_key[i]) cend[c] = vend[i];
}

__global__ void k_bin_heads(const uint64_t* __restrict__ ckey_s, uint64_t n, uint32_t* __restrict__ head) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) head[j] = j == 0 || ckey_s[j - 1] != ckey_s[j];
}

// bin b's key and first sorted chunk; bin_first[n_bins] = n_chunks is set by the host
__global__ void k_bins(const uint64_t* __restrict__ ckey_s, const uint32_t* __restrict__ bid, uint64_t n_chunks, uint64_t* __restrict__ bin_key,
                       uint32_t* __restrict__ bin_first) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_chunks || bid[j + 1] == bid[j]) return;
    bin_key[bid[j]] = ckey_s[j];
    bin_first[bid[j]] = (uint32_t)j;
}

struct RefShape { uint64_t fb, nb, fc, nc, fr, fr1; };
__device__ inline RefShape ref_shape(uint32_t r, const uint64_t* __restrict__ bin_key, uint64_t n_bins, const uint32_t* __restrict__ bin_first,
                                     const uint64_t* __restrict__ key_s, uint64_t n) {
    RefShape s;
    const uint64_t k0 = (uint64_t)r << 32, k1 = ((uint64_t)r + 1) << 32;
    s.fb = lower_bound(bin_key, n_bins, k0);
    s.nb = lower_bound(bin_key, n_bins, k1) - s.fb;
    s.fc = bin_first[s.fb];
    s.nc = bin_first[s.fb + s.nb] - s.fc;
    s.fr = lower_bound(key_s, n, k0);
    s.fr1 = lower_bound(key_s, n, k1);
    return s;
}

// the 32-bit words of reference r, and its windows
__global__ void k_ref_sizes(uint32_t n_refs, const uint64_t* __restrict__ bin_key, uint64_t n_bins, const uint32_t* __restrict__ bin_first,
                            const uint64_t* __restrict__ key_s, uint64_t n, const uint32_t* __restrict__ n_intv, uint32_t* __restrict__ ref_words) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_refs) return;
    const RefShape s = ref_shape((uint32_t)r, bin_key, n_bins, bin_first, key_s, n);
    ref_words[r] = (uint32_t)(bai_ref_bytes(s.nb, s.nc, n_intv[r], s.fr1 > s.fr) / 4);
}

__global__ void __launch_bounds__(kBlock)
k_windows(const uint64_t* __restrict__ bin_key, const uint64_t* __restrict__ vbeg, const uint32_t* __restrict__ beg, const uint32_t* __restrict__ end,
          uint64_t n, const uint64_t* __restrict__ lin_off, unsigned long long* __restrict__ lin) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || bin_key[i] == kNoValue) return;
    const uint32_t r = (uint32_t)(bin_key[i] >> 32);
    const uint64_t n_w = lin_off[r + 1] - lin_off[r];
    uint64_t w1 = (end[i] - 1u) >> kBaiWindowShift;
    if (w1 >= n_w) w1 = n_w - 1;                          // (n_w >= 1: this record raised it; w1 < n_w <= kBaiMaxWindows)
    for (uint64_t w = beg[i] >> kBaiWindowShift; w <= w1; ++w) atomicMin(&lin[lin_off[r] + w], (unsigned long long)vbeg[i]);
}

__device__ inline void put64(uint32_t* __restrict__ out, uint64_t word, uint64_t v) { out[word] = (uint32_t)v; out[word + 1] = (uint32_t)(v >> 32); }

// sorted chunk j at its place behind its bin's head
__global__ void k_write_chunks(const uint64_t* __restrict__ ckey_s, const uint32_t* __restrict__ cperm, const uint64_t* __restrict__ cbeg,
                               const uint64_t* __restrict__ cend, const uint32_t* __restrict__ bid, uint64_t n_chunks, const uint64_t* __restrict__ bin_key,
                               uint64_t n_bins, const uint32_t* __restrict__ bin_first, const uint64_t* __restrict__ ref_off, uint32_t* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_chunks) return;
    const uint64_t b = bid[j + 1] != bid[j] ? bid[j] : bid[j] - 1u;
    const uint32_t r = (uint32_t)(ckey_s[j] >> 32);
    const uint64_t fb = lower_bound(bin_key, n_bins, (uint64_t)r << 32), fc = bin_first[fb];
    const uint64_t word = 2 + ref_off[r] + 1 + 2 * (b - fb + 1) + 4 * (j - fc);
    put64(out, word, cbeg[cperm[j]]);
    put64(out, word + 2, cend[cperm[j]]);
}

__global__ void k_write_bins(const uint64_t* __restrict__ bin_key, uint64_t n_bins, const uint32_t* __restrict__ bin_first,
                             const uint64_t* __restrict__ ref_off, uint32_t* __restrict__ out) {
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bins) return;
    const uint32_t r = (uint32_t)(bin_key[b] >> 32);
    const uint64_t fb = lower_bound(bin_key, n_bins, (uint64_t)r << 32), fc = bin_first[fb];
    const uint64_t word = 2 + ref_off[r] + 1 + 2 * (b - fb) + 4 * (bin_first[b] - fc);
    out[word] = (uint32_t)bin_key[b];
    out[word + 1] = bin_first[b + 1] - bin_first[b];
}

// lane r < n_refs: n_bin, the pseudo-bin, n_intv and the windows of reference r, backfilled from the right; lane n_refs: the
// magic, n_ref and n_no_coor
__global__ void k_write_refs(uint32_t n_refs, const uint64_t* __restrict__ bin_key, uint64_t n_bins, const uint32_t* __restrict__ bin_first,
                             const uint64_t* __restrict__ key_s, uint64_t n, const uint64_t* __restrict__ vbeg, const uint64_t* __restrict__ vend,
                             const unsigned long long* __restrict__ n_unmapped, const uint64_t* __restrict__ lin_off,
                             const unsigned long long* __restrict__ lin, const uint64_t* __restrict__ ref_off, uint32_t* __restrict__ out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_refs) return;
    if (r == n_refs) {
        out[0] = 0x01494142u;                             // "BAI\1"
        out[1] = n_refs;
        put64(out, 2 + ref_off[n_refs], n - lower_bound(key_s, n, kBaiNoCoorKey));
        return;
    }
    const RefShape s = ref_shape((uint32_t)r, bin_key, n_bins, bin_first, key_s, n);
    const bool has = s.fr1 > s.fr;
    uint64_t word = 2 + ref_off[r];
    out[word] = has ? (uint32_t)s.nb + 1u : 0u;
    word += 1 + 2 * s.nb + 4 * s.nc;
    if (has) {
        out[word] = kBaiPseudoBin; out[word + 1] = 2u;
        put64(out, word + 2, vbeg[s.fr]);
        put64(out, word + 4, vend[s.fr1 - 1]);
        put64(out, word + 6, (s.fr1 - s.fr) - n_unmapped[r]);
        put64(out, word + 8, n_unmapped[r]);
        word += 10;
    }
    const uint64_t l0 = lin_off[r], n_w = lin_off[r + 1] - l0;      // at most kBaiMaxWindows
    out[word] = (uint32_t)n_w;
    unsigned long long right = kNoValue;
    for (uint64_t w = n_w; w-- > 0;) {
        const unsigned long long v = lin[l0 + w];
        if (v != kNoValue) right = v;
        put64(out, word + 1 + 2 * w, right);
    }
}

// the index as "lines" of one tile each, for textchunks::deliver
__global__ void k_tile_lines(uint64_t n_bytes, uint64_t n_lines, uint64_t* __restrict__ line_start) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n_lines) return;
    const uint64_t s = k * textchunks::kTileBytes;
    line_start[k] = s < n_bytes ? s : n_bytes;
}

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

struct sfgpu_bamsort final : BamRecordStore {
    std::vector<void*> segs;
    uint64_t seg_bytes = 0;
    DevBuf<uint64_t> key, addr;
    DevBuf<uint32_t> len;
    uint64_t n = 0, peak = 0;
    bool finished = false;
    ~sfgpu_bamsort() {
        (void)hipDeviceSynchronize();
        for (void* p : segs) pool_free(p);
    }
    uint64_t held() const { return seg_bytes + key.cap * 8 + addr.cap * 8 + len.cap * 4; }

    int take(uint64_t total, uint64_t n_records, const uint64_t* d_unit_start, uint64_t n_units, hipStream_t st, double* format_ms,
             const std::function<int(uint4*, hipStream_t)>& format_all) override {
        if (n + n_records >= (1ull << 32)) {
            set_error("sfgpu_bamsort_collect: the store would hold 2^32 records or more");
            return SFGPU_ERR_RANGE;
        }
        DevBuf<uint32_t> cnt, before;
        CallScope scope;                                  // after the scratch: st has drained before it goes back
        hipEvent_t ev[2] = {nullptr, nullptr};
        uint32_t* h_n = nullptr;
        SF_HIP(scope.adopt(st));
        for (auto& e : ev) SF_HIP(scope.event(&e));
        SF_HIP(scope.pinned_block(&h_n, sizeof(uint32_t)));
        if (int rc = cnt.reserve(n_units + 1, st, false)) return rc;
        if (int rc = before.reserve(n_units + 1, st, false)) return rc;
        if (int rc = key.reserve(n + n_records, st, true, n)) return rc;
        if (int rc = addr.reserve(n + n_records, st, true, n)) return rc;
        if (int rc = len.reserve(n + n_records, st, true, n)) return rc;
        const uint64_t bytes = (total + 15) / 16 * 16 + kSegSlack;
        uint8_t* seg = nullptr;
        SF_HIP(pool_malloc(&seg, bytes));
        struct Guard { void* p; hipStream_t s; ~Guard() { if (p) { (void)hipStreamSynchronize(s); pool_free(p); } } } guard{seg, st};
        SF_HIP(hipEventRecord(ev[0], st));
        if (int rc = format_all(reinterpret_cast<uint4*>(seg), st)) return rc;
        hipLaunchKernelGGL(k_unit_records, dim3(grid_of(n_units)), dim3(kBlock), 0, st, seg, d_unit_start, n_units, cnt.p);
        SF_HIP(hipGetLastError());
        if (int rc = exclusive_scan_u32_u32(cnt.p, before.p, n_units, st)) return rc;
        SF_HIP(hipMemcpyAsync(h_n, before.p + n_units, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        if (*h_n != n_records) {                          // the sizing pass and the formatted records disagree: nothing is listed
            set_error("sfgpu_bamsort_collect: %u records found in a batch of %llu", *h_n, (unsigned long long)n_records);
            return SFGPU_ERR_HIP;
        }
        hipLaunchKernelGGL(k_append, dim3(grid_of(n_units)), dim3(kBlock), 0, st, seg, d_unit_start, n_units, before.p, key.p + n, addr.p + n, len.p + n);
        SF_HIP(hipGetLastError());
        SF_HIP(hipEventRecord(ev[1], st));
        SF_HIP(hipStreamSynchronize(st));
        add_elapsed(format_ms, ev[0], ev[1]);
        guard.p = nullptr;
        segs.push_back(seg);
        seg_bytes += bytes;
        n += n_records;
        if (held() > peak) peak = held();
        return SFGPU_OK;
    }
};

extern "C" int sfgpu_bamsort_open(sfgpu_bamsort** out) {
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_bamsort_open: null handle pointer");
    *out = new (std::nothrow) sfgpu_bamsort;
    SF_REQUIRE(*out, SFGPU_ERR_HIP, "sfgpu_bamsort_open: out of host memory");
    return SFGPU_OK;
}

extern "C" int sfgpu_bamsort_collect(sfgpu_bamsort* b, const sfgpu_samw_batch* batch, sfgpu_samwrite_result* out, sfgpu_stream stream) {
    SF_REQUIRE(b, SFGPU_ERR_INVALID, "sfgpu_bamsort_collect: null handle");
    SF_REQUIRE(!b->finished, SFGPU_ERR_STATE, "sfgpu_bamsort_collect: the store is finished");
    SF_REQUIRE(batch, SFGPU_ERR_INVALID, "sfgpu_bamsort_collect: null batch");
    return samw_collect_bam(b, *batch, out, stream);
}

extern "C" int sfgpu_bamsort_finish(sfgpu_bamsort* b, sfgpu_bgzw* z, uint32_t n_refs, uint64_t piece_bytes, sfgpu_text_sink index_sink,
                                    void* user, sfgpu_bamsort_result* res, sfgpu_stream stream) {
    const char* who = "sfgpu_bamsort_finish";
    SF_REQUIRE(b && z && res, SFGPU_ERR_INVALID, "sfgpu_bamsort_finish: null argument");
    SF_REQUIRE(!b->finished, SFGPU_ERR_STATE, "sfgpu_bamsort_finish: the store is finished already");
    memset(res, 0, sizeof(*res));
    if (piece_bytes == 0) piece_bytes = kDefaultPiece;
    SF_REQUIRE(piece_bytes >= 16 && piece_bytes <= (1ull << 30), SFGPU_ERR_INVALID, "sfgpu_bamsort_finish: piece_bytes must lie in [16, 2^30] (0 = default)");
    piece_bytes = piece_bytes < kBaiMember ? kBaiMember : piece_bytes / kBaiMember * kBaiMember;
    const uint32_t* d_sizes = nullptr;
    uint64_t first_member = 0;
    if (int rc = sfgpu_bgzw_member_sizes(z, &d_sizes, &first_member)) return rc;
    b->finished = true;
    const uint64_t n = b->n;

    DevBuf<uint64_t> key_s, start, coff, bin_key, vbeg, vend, ckey, ckey_s, cbeg, cend, bkey, ref_off, lin_off, line_start;
    DevBuf<uint32_t> vals, perm, len_s, beg, end, head, cid, cvals, cperm, bhead, bid, bin_first, n_intv, ref_words, idx;
    DevBuf<unsigned long long> n_unmapped, lin, misc;
    DevBuf<uint4> piece[2];
    CallScope scope;                                      // after the scratch: it drains before any block goes back
    hipStream_t st = nullptr, ready = nullptr;
    hipEvent_t ev_in = nullptr, ev_s[2] = {nullptr, nullptr}, ev_g0[2] = {nullptr, nullptr}, ev_g1[2] = {nullptr, nullptr};
    unsigned long long* h = nullptr;                      // [0] stream bytes, [1] records with a reference, [2] chunks / bins, [3] words, [4] windows
    SF_HIP(scope.acquire(&st));
    SF_HIP(scope.acquire(&ready));
    SF_HIP(scope.event(&ev_in, hipEventDisableTiming));
    for (hipEvent_t* e : {&ev_s[0], &ev_s[1], &ev_g0[0], &ev_g0[1], &ev_g1[0], &ev_g1[1]}) SF_HIP(scope.event(e));
    SF_HIP(scope.pinned_block(&h, 5 * sizeof(unsigned long long)));
    SF_HIP(hipEventRecord(ev_in, as_stream(stream)));
    SF_HIP(hipStreamWaitEvent(st, ev_in, 0));
    auto transient = [&]() -> uint64_t {
        uint64_t t = 0;
        for (const DevBuf<uint64_t>* d : {&key_s, &start, &coff, &bin_key, &vbeg, &vend, &ckey, &ckey_s, &cbeg, &cend, &bkey, &ref_off, &lin_off, &line_start}) t += d->cap * 8;
        for (const DevBuf<uint32_t>* d : {&vals, &perm, &len_s, &beg, &end, &head, &cid, &cvals, &cperm, &bhead, &bid, &bin_first, &n_intv, &ref_words, &idx}) t += d->cap * 4;
        return t + (n_unmapped.cap + lin.cap + misc.cap) * 8 + (piece[0].cap + piece[1].cap) * 16;
    };
    auto note_peak = [&] { if (b->held() + transient() > b->peak) b->peak = b->held() + transient(); };

    // ---- the order, the stream starts
    uint64_t total = 0, n_coor = 0;
    if (int rc = start.reserve(n + 1, st, false)) return rc;
    if (int rc = key_s.reserve(n + 1, st, false)) return rc;
    if (int rc = perm.reserve(n + 1, st, false)) return rc;
    if (n) {
        if (int rc = vals.reserve(n, st, false)) return rc;
        if (int rc = len_s.reserve(n + 1, st, false)) return rc;
        if (int rc = misc.reserve(1, st, false)) return rc;
        SF_HIP(hipEventRecord(ev_s[0], st));
        hipLaunchKernelGGL(k_iota, dim3(grid_of(n)), dim3(kBlock), 0, st, vals.p, n);
        SF_HIP(hipGetLastError());
        if (int rc = sort_pairs_u64_u32(b->key.p, key_s.p, vals.p, perm.p, n, st, 64, false)) return rc;
        SF_HIP(hipEventRecord(ev_s[1], st));
        hipLaunchKernelGGL(k_sorted_len, dim3(grid_of(n)), dim3(kBlock), 0, st, b->len.p, perm.p, n, len_s.p);
        SF_HIP(hipGetLastError());
        if (int rc = exclusive_scan_u32(len_s.p, start.p, n, st, false)) return rc;
        hipLaunchKernelGGL(k_first_no_coor, dim3(1), dim3(kWave), 0, st, key_s.p, n, misc.p);
        SF_HIP(hipGetLastError());
        SF_HIP(hipMemcpyAsync(&h[0], start.p + n, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(&h[1], misc.p, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        add_elapsed(&res->sort_ms, ev_s[0], ev_s[1]);
        total = h[0]; n_coor = h[1];
    } else {
        SF_HIP(hipMemsetAsync(start.p, 0, 8, st));
    }
    res->n_records = n; res->n_no_coor = n - n_coor; res->n_bytes = total;

    // ---- the stream, a piece at a time: piece i + 1 is gathered while piece i is encoded, copied and sunk
    const uint64_t n_pieces = (total + piece_bytes - 1) / piece_bytes;
    for (int s = 0; s < 2 && (uint64_t)s < n_pieces; ++s)
        if (int rc = piece[s].reserve(((total < piece_bytes ? total : piece_bytes) + 15) / 16, st, false)) return rc;
    note_peak();
    auto piece_len = [&](uint64_t i) -> uint64_t { return total - i * piece_bytes < piece_bytes ? total - i * piece_bytes : piece_bytes; };
    auto enqueue = [&](uint64_t i) -> int {
        const int s = (int)(i & 1);
        SF_HIP(hipEventRecord(ev_g0[s], st));
        hipLaunchKernelGGL(k_gather, dim3(grid_of((piece_len(i) + 15) / 16)), dim3(kBlock), 0, st, start.p, n, b->addr.p, perm.p, i * piece_bytes, piece_len(i),
                           piece[s].p);
        SF_HIP(hipGetLastError());
        SF_HIP(hipEventRecord(ev_g1[s], st));
        return SFGPU_OK;
    };
    if (n_pieces) if (int rc = enqueue(0)) return rc;
    for (uint64_t i = 0; i < n_pieces; ++i) {
        const int s = (int)(i & 1);
        SF_HIP(hipStreamWaitEvent(ready, ev_g1[s], 0));
        if (i + 1 < n_pieces) if (int rc = enqueue(i + 1)) return rc;
        if (int rc = sfgpu_bgzw_write_device(z, piece[s].p, piece_len(i), reinterpret_cast<sfgpu_stream>(ready))) return rc;
        SF_HIP(hipEventSynchronize(ev_g1[s]));
        add_elapsed(&res->gather_ms, ev_g0[s], ev_g1[s]);
        res->n_pieces++;
    }
    res->state_bytes = b->peak;
    if (!index_sink) return SFGPU_OK;

    // ---- the index
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t n_members = 0;
    if (int rc = sfgpu_bgzw_member_sizes(z, &d_sizes, &n_members)) return rc;
    if (int rc = coff.reserve(n_members + 1, st, false)) return rc;
    if (n_members) { if (int rc = exclusive_scan_u32(d_sizes, coff.p, n_members, st, false)) return rc; }
    else SF_HIP(hipMemsetAsync(coff.p, 0, 8, st));
    for (DevBuf<uint64_t>* d : {&bin_key, &vbeg, &vend}) if (int rc = d->reserve(n + 1, st, false)) return rc;
    for (DevBuf<uint32_t>* d : {&beg, &end, &head, &cid}) if (int rc = d->reserve(n + 1, st, false)) return rc;
    if (int rc = n_intv.reserve((uint64_t)n_refs + 1, st, false)) return rc;
    if (int rc = n_unmapped.reserve((uint64_t)n_refs + 1, st, false)) return rc;
    if (int rc = ref_words.reserve((uint64_t)n_refs + 1, st, false)) return rc;
    if (int rc = ref_off.reserve((uint64_t)n_refs + 1, st, false)) return rc;
    if (int rc = lin_off.reserve((uint64_t)n_refs + 1, st, false)) return rc;
    SF_HIP(hipMemsetAsync(n_intv.p, 0, ((uint64_t)n_refs + 1) * 4, st));
    SF_HIP(hipMemsetAsync(n_unmapped.p, 0, ((uint64_t)n_refs + 1) * 8, st));
    uint64_t n_chunks = 0, n_bins = 0;
    if (n) {
        const IndexArrays x = {bin_key.p, vbeg.p, vend.p, beg.p, end.p, n_unmapped.p, n_intv.p};
        hipLaunchKernelGGL(k_index_records, dim3(grid_of(n)), dim3(kBlock), 0, st, b->addr.p, perm.p, start.p, n, n_refs, first_member, coff.p, n_members, x);
        SF_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_heads, dim3(grid_of(n)), dim3(kBlock), 0, st, bin_key.p, n, head.p);
        SF_HIP(hipGetLastError());
        if (int rc = exclusive_scan_u32_u32(head.p, cid.p, n, st)) return rc;
        h[2] = 0;
        SF_HIP(hipMemcpyAsync(&h[2], cid.p + n, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        n_chunks = (uint32_t)h[2];
    }
    if (n_chunks >= (1ull << 28)) { set_error("%s: the index would hold 2^28 chunks or more", who); return SFGPU_ERR_RANGE; }
    for (DevBuf<uint64_t>* d : {&ckey, &ckey_s, &cbeg, &cend, &bkey}) if (int rc = d->reserve(n_chunks + 1, st, false)) return rc;
    for (DevBuf<uint32_t>* d : {&cvals, &cperm, &bhead, &bid, &bin_first}) if (int rc = d->reserve(n_chunks + 2, st, false)) return rc;
    if (n_chunks) {
        hipLaunchKernelGGL(k_chunks, dim3(grid_of(n)), dim3(kBlock), 0, st, bin_key.p, vbeg.p, vend.p, cid.p, n, ckey.p, cbeg.p, cend.p);
        SF_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_iota, dim3(grid_of(n_chunks)), dim3(kBlock), 0, st, cvals.p, n_chunks);
        SF_HIP(hipGetLastError());
        if (int rc = sort_pairs_u64_u32(ckey.p, ckey_s.p, cvals.p, cperm.p, n_chunks, st, 64, false)) return rc;
        hipLaunchKernelGGL(k_bin_heads, dim3(grid_of(n_chunks)), dim3(kBlock), 0, st, ckey_s.p, n_chunks, bhead.p);
        SF_HIP(hipGetLastError());
        if (int rc = exclusive_scan_u32_u32(bhead.p, bid.p, n_chunks, st)) return rc;
        h[2] = 0;
        SF_HIP(hipMemcpyAsync(&h[2], bid.p + n_chunks, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        n_bins = (uint32_t)h[2];
        hipLaunchKernelGGL(k_bins, dim3(grid_of(n_chunks)), dim3(kBlock), 0, st, ckey_s.p, bid.p, n_chunks, bkey.p, bin_first.p);
        SF_HIP(hipGetLastError());
    }
    {
        const uint32_t last = (uint32_t)n_chunks;             // bin_first[n_bins] = n_chunks
        SF_HIP(hipMemcpyAsync(bin_first.p + n_bins, &last, 4, hipMemcpyHostToDevice, st));
        SF_HIP(hipStreamSynchronize(st));                     // (`last` lives on this frame)
    }
    hipLaunchKernelGGL(k_ref_sizes, dim3(grid_of((uint64_t)n_refs + 1)), dim3(kBlock), 0, st, n_refs, bkey.p, n_bins, bin_first.p, key_s.p, n, n_intv.p, ref_words.p);
    SF_HIP(hipGetLastError());
    if (n_refs) {
        if (int rc = exclusive_scan_u32(ref_words.p, ref_off.p, n_refs, st, false)) return rc;
        if (int rc = exclusive_scan_u32(n_intv.p, lin_off.p, n_refs, st, false)) return rc;
    } else {
        SF_HIP(hipMemsetAsync(ref_off.p, 0, 8, st));
        SF_HIP(hipMemsetAsync(lin_off.p, 0, 8, st));
    }
    SF_HIP(hipMemcpyAsync(&h[3], ref_off.p + n_refs, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h[4], lin_off.p + n_refs, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint64_t n_words = 2 + h[3] + 2, n_windows = h[4], index_bytes = 4 * n_words;
    if (int rc = idx.reserve(n_words + 4, st, false)) return rc;
    if (int rc = lin.reserve(n_windows + 1, st, false)) return rc;
    SF_HIP(hipMemsetAsync(lin.p, 0xff, (n_windows + 1) * 8, st));
    if (n) {
        hipLaunchKernelGGL(k_windows, dim3(grid_of(n)), dim3(kBlock), 0, st, bin_key.p, vbeg.p, beg.p, end.p, n, lin_off.p, lin.p);
        SF_HIP(hipGetLastError());
    }
    if (n_chunks) {
        hipLaunchKernelGGL(k_write_chunks, dim3(grid_of(n_chunks)), dim3(kBlock), 0, st, ckey_s.p, cperm.p, cbeg.p, cend.p, bid.p, n_chunks, bkey.p, n_bins,
                           bin_first.p, ref_off.p, idx.p);
        SF_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_write_bins, dim3(grid_of(n_bins)), dim3(kBlock), 0, st, bkey.p, n_bins, bin_first.p, ref_off.p, idx.p);
        SF_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_write_refs, dim3(grid_of((uint64_t)n_refs + 1)), dim3(kBlock), 0, st, n_refs, bkey.p, n_bins, bin_first.p, key_s.p, n, vbeg.p, vend.p,
                       n_unmapped.p, lin_off.p, lin.p, ref_off.p, idx.p);
    SF_HIP(hipGetLastError());
    // the bytes to their sink, a tile a "line"
    const uint64_t n_lines = (index_bytes + textchunks::kTileBytes - 1) / textchunks::kTileBytes;
    if (int rc = line_start.reserve(n_lines + 1, st, false)) return rc;
    hipLaunchKernelGGL(k_tile_lines, dim3(grid_of(n_lines + 1)), dim3(kBlock), 0, st, index_bytes, n_lines, line_start.p);
    SF_HIP(hipGetLastError());
    note_peak();
    res->state_bytes = b->peak;
    textchunks::Stats ts;
    const uint8_t* d_idx = reinterpret_cast<const uint8_t*>(idx.p);
    const int rc = textchunks::deliver(who, line_start.p, n_lines, index_bytes, textchunks::kDefaultChunk, index_sink, user, st, &ts,
                                       [&](uint64_t first_tile, uint64_t last_tile, uint64_t out_base, uint4* buf, hipStream_t s) -> int {
                                           (void)first_tile;
                                           const uint64_t e = (last_tile + 1) * textchunks::kTileBytes < index_bytes ? (last_tile + 1) * textchunks::kTileBytes : index_bytes;
                                           SF_HIP(hipMemcpyAsync(buf, d_idx + out_base, e - out_base, hipMemcpyDeviceToDevice, s));
                                           return SFGPU_OK;
                                       });
    if (rc) return rc;
    res->index_bytes = index_bytes; res->n_index_chunks = n_chunks; res->n_index_bins = n_bins;
    res->index_ms = ms_since(t0);
    return SFGPU_OK;
}

extern "C" int sfgpu_bamsort_close(sfgpu_bamsort* b) {
    SF_REQUIRE(b, SFGPU_ERR_INVALID, "sfgpu_bamsort_close: null handle");
    delete b;
    return SFGPU_OK;
}
