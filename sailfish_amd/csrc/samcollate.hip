// samcollate.hip -- the collated reading of a SAM text or BAM stream whose lines stand in any order (a position-sorted file):
// sfgpu_samc_*, sfgpu_sam_collect_*, sfgpu_bam_collect_*.  What the lines say, which are one fragment and which two pair is
// samcfmt.h (the same functions run serially in tests/samcollate_harness.cpp); this file is the passes around them.  Everything is
// one lane per line or record, scans and sorts: no pass walks a fragment, no workgroup waits for another.
//
// collect   the front end of the name-grouped reader of the format (samfront.h: 16-byte-group counting, tab scans, k_sam_lines;
//           bamfront.h: the record chain, k_bam_records), unchanged, then
//   k_samc_line_mates / k_samc_record_mates   one lane per line: samcfmt.h's mate fields (the written POS, PNEXT when the line names
//                     a mate) and the QNAME test; a malformed line joins the 64-bit min of the front end, so the lowest line and
//                     its first rule win across both kernels
//   k_samc_append     the line records of the call behind those of the handle (the arrays grow by doubling)
//   scan, k_samc_names   the name lengths, computed once, place the names; the blob is gathered by 16-byte groups of the OUTPUT, in
//                     the manner of readtext.hip's k_names_gather: a lane finds the name its group begins in by binary search
//                     and issues one aligned 16-byte store.  The names of a call begin at a 16-byte boundary of the blob.
// finish
//   rank_strings      ranksort.h over (length byte, name bytes): equal ranks are byte-equal names
//   k_samc_first, k_samc_frag_keys, sort_pairs_u64_u32   the first line of each fragment; the lines ordered by (first line of their
//                     fragment, file order): order[], the rec_line[] of samback.h; heads and their scan number the fragments
//   pairing           the lines that name a mate, side-1 lines in front of side-2 lines (two scans: a stable partition), sorted by
//                     (POS of mate 1, POS of mate 2) and then by (fragment, tid), both stable: runs of one key hold n1 side-1 lines
//                     and then n2 side-2 lines in file order.  Run heads, two scans, k_samc_partner: the i-th side-1 line takes
//                     the i-th side-2 line when i < n2.  The result is partner[], pair_head[] and has_pair[].
// emit      samback.h as it is over the slice (k_sam_survive, k_sam_keys, the stable sort by sam_sort_key), with the heads scanned
//           over the slice so that `group` is relative to it, and k_samc_write, which reads the mate from partner[].
#include "bamfront.h"
#include "common.h"
#include "primitives.h"
#include "ranksort.h"
#include "samback.h"
#include "samcfmt.h"
#include "samfront.h"
#include "textlines.h"
#include "textstage.h"

namespace sfgpu {
namespace {

using namespace samback;

inline unsigned grid_of(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
constexpr uint64_t kMaxBytes = 1ull << 30;               // one collect call
constexpr uint64_t kMaxLines = 0xffffffffull - 1;        // one collection
constexpr unsigned long long kNoBad = ~0ull;

struct Bytes {
    const unsigned char* p;
    __device__ unsigned char operator()(uint32_t i) const { return p[i]; }
};

// ---- collect --------------------------------------------------------------------------------------------------------------

// the lowest key of the wavefront into *first_bad.  No lane leaves before the shuffles.
__device__ inline void min_bad(unsigned long long key, unsigned long long* first_bad) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other < key ? other : key;
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && key != kNoBad) atomicMin(first_bad, key);
}

// One lane per line of the text, behind k_sam_lines.  What samc_line_mate asks of the SamLine is put together from what k_sam_lines
// left: header (isrec), BAD_FIELDS (no tenth tab), q_len (the first tab), mapped (info; 0 where FLAG was no number).
__global__ void __launch_bounds__(kBlock) k_samc_line_mates(const unsigned char* __restrict__ bytes, uint32_t L, const uint32_t* __restrict__ line_end,
                                                            const uint32_t* __restrict__ tab_pos, int paired, const uint32_t* __restrict__ info,
                                                            const uint32_t* __restrict__ isrec, uint32_t* __restrict__ pos1, uint32_t* __restrict__ pnext,
                                                            uint32_t* __restrict__ qlen, uint32_t* __restrict__ nsrc, unsigned long long* __restrict__ first_bad) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = kNoBad;
    if (j < L) {
        const uint32_t s = j ? line_end[j - 1] + 1 : 0;
        SamMate m = {0, 0, 0};
        uint32_t q = 0;
        if (isrec[j]) {
            uint32_t tab[kSamTabs];
#pragma unroll
            for (uint32_t o = 0; o < kSamTabs; ++o) tab[o] = tab_pos[(uint64_t)o * L + j];
            SamLine l = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            l.bad = tab[kSamTabs - 1] == kSamNone ? (uint32_t)SFGPU_SAM_BAD_FIELDS : 0u;
            if (!l.bad) {
                l.q_len = q = tab[0] - s;
                l.mapped = (uint8_t)((info[j] >> 16) & 1u);
                l.side = (uint8_t)((info[j] >> 18) & 3u);
                m = samc_line_mate(Bytes{bytes}, s, tab, paired != 0, l);
            }
        }
        pos1[j] = m.pos1; pnext[j] = m.pnext; qlen[j] = q; nsrc[j] = s;
        if (m.bad) key = ((unsigned long long)j << 8) | (m.bad & (0u - m.bad));
    }
    min_bad(key, first_bad);
}

// One lane per record of the stream, behind k_bam_records (a record that is BAD_FIELDS has mapped = 0 there: nothing of it is read)
__global__ void __launch_bounds__(kBlock) k_samc_record_mates(const unsigned char* __restrict__ bytes, uint32_t K, const uint32_t* __restrict__ rec_off,
                                                              int paired, const uint32_t* __restrict__ info, uint32_t* __restrict__ pos1,
                                                              uint32_t* __restrict__ pnext, uint32_t* __restrict__ nsrc) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    SamLine l = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    l.mapped = (uint8_t)((info[k] >> 16) & 1u);
    const SamMate m = samc_record_mate(Bytes{bytes}, rec_off[k], paired != 0, l);
    pos1[k] = m.pos1; pnext[k] = m.pnext; nsrc[k] = rec_off[k] + kBamMin;
}

// what a collection holds per line
struct LineArrays {
    uint32_t* info;
    uint32_t* tid;
    int32_t* pos;
    uint32_t* pos1;
    uint32_t* pnext;
    uint32_t* name_len;
};

// record k of the call (line rec_line[k] of its text) -> line base + k of the collection; nlen[k] = its name's length
__global__ void k_samc_append(uint32_t K, const uint32_t* __restrict__ rec_line, const uint32_t* __restrict__ info, const uint32_t* __restrict__ tid,
                              const int32_t* __restrict__ pos, const uint32_t* __restrict__ pos1, const uint32_t* __restrict__ pnext,
                              const uint32_t* __restrict__ qlen, uint64_t base, LineArrays out, uint32_t* __restrict__ nlen) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const uint32_t j = rec_line[k];
    const uint64_t d = base + k;
    out.info[d] = info[j]; out.tid[d] = tid[j]; out.pos[d] = pos[j]; out.pos1[d] = pos1[j]; out.pnext[d] = pnext[j];
    out.name_len[d] = nlen[k] = qlen[j];
}

// The names of the call, back to back from `out` on (a 16-byte boundary of the blob, `at0` bytes into it): one lane per 16-byte
// group of the OUTPUT.  nscan[0 .. K] = the exclusive sum of the name lengths (n_name = nscan[K]); name k begins at nsrc[rec_line[k]]
// of the text.  The lane finds the name its group begins in by binary search (the last k with nscan[k] <= its first byte: empty names
// in front of it are skipped), takes its 16 bytes from that name and the ones behind it, and issues one 16-byte store; the last
// group is filled up with zeros.  The first K lanes also say where each name lies.
__global__ void __launch_bounds__(kBlock) k_samc_names(const unsigned char* __restrict__ bytes, uint32_t K, uint32_t n_name, const uint32_t* __restrict__ nscan,
                                                       const uint32_t* __restrict__ rec_line, const uint32_t* __restrict__ nsrc, uint4* __restrict__ out,
                                                       uint64_t at0, uint64_t* __restrict__ name_at) {
    const uint32_t g = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (g < K) name_at[g] = at0 + nscan[g];
    if (g >= (n_name + 15u) / 16u) return;
    const uint32_t o = g * 16u;
    const uint32_t cnt = n_name - o < 16u ? n_name - o : 16u;
    uint32_t lo = 0, hi = K;                              // nscan[lo] <= o < nscan[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (nscan[mid] <= o) lo = mid; else hi = mid;
    }
    uint32_t i = lo, end = nscan[i + 1], src = nsrc[rec_line[i]] + (o - nscan[i]);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (uint32_t b = 0; b < cnt; ++b) {
        while (o + b >= end) { ++i; end = nscan[i + 1]; src = nsrc[rec_line[i]]; }      // (a name with a byte exists: o + b < n_name)
        w[b >> 2] |= (uint32_t)bytes[src++] << (8 * (b & 3));
    }
    out[g] = make_uint4(w[0], w[1], w[2], w[3]);
}

struct CollectScratch {
    DevBuf<uint32_t> pos1, pnext, qlen, nsrc, rec_line, nlen, nscan;
};
struct SamScratch : CollectScratch {
    DevBuf<uint4> text;
    samfront::Front F;
};
struct BamScratch : CollectScratch {
    DevBuf<uint4> text;
    bamfront::Chain C;
    DevBuf<uint32_t> info, tid, name_len;
    DevBuf<int32_t> pos;
    DevBuf<unsigned long long> word;
};

// ---- finish ---------------------------------------------------------------------------------------------------------------

// ranksort.h's view of the collection: string i = one byte that holds the name's length (<= 254: samcfmt.h) and the name's bytes, so
// that the zero padding of a round's key never makes two different names equal
struct LenNames {
    const unsigned char* blob;
    const uint64_t* at;
    const uint32_t* len;
    __device__ uint64_t key(uint32_t item, uint32_t round) const {
        const uint32_t n = len[item];
        const unsigned char* q = blob + at[item];
        uint64_t k = 0;
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t x = 8u * round + i;
            k = (k << 8) | (x == 0 ? n : x - 1 < n ? (uint32_t)q[x - 1] : 0u);
        }
        return k;
    }
    __device__ uint64_t bytes(uint32_t item) const { return (uint64_t)len[item] + 1; }
};

// first[r] = the first line (file order) of the r-th name: by stability the line at the head of its run
__global__ void k_samc_first(uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ run, uint32_t* __restrict__ first) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n && (j == 0 || run[j] != run[j - 1])) first[run[j]] = perm[j];
}

// key[line] = the first line of its fragment; iota
__global__ void k_samc_frag_keys(uint32_t n, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ run, const uint32_t* __restrict__ first,
                                 uint64_t* __restrict__ key, uint32_t* __restrict__ iota) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    key[perm[j]] = first[run[j]];
    iota[j] = j;
}

__global__ void k_samc_heads(uint32_t n, const uint64_t* __restrict__ key_sorted, uint32_t* __restrict__ head) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) head[k] = (k == 0 || key_sorted[k] != key_sorted[k - 1]) ? 1u : 0u;
}

// frag_start[g] = the position in order[] of fragment g's first line; frag_start[n_reads] = n
__global__ void k_samc_frag_starts(uint32_t n, const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_scan, uint32_t* __restrict__ frag_start) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > n) return;
    if (k == n) { frag_start[head_scan[n]] = n; return; }
    if (head[k]) frag_start[head_scan[k]] = k;
}

// which positions of order[] name a mate: side-1 lines and side-2 lines apart
__global__ void k_samc_mated(uint32_t n, const uint32_t* __restrict__ order, const uint32_t* __restrict__ info, const uint32_t* __restrict__ pnext,
                             uint32_t* __restrict__ is1, uint32_t* __restrict__ is2) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t j = order[k], w = info[j];
    const bool mated = ((w >> 16) & 1u) && pnext[j] != 0;
    const uint32_t side = (w >> 18) & 3u;
    is1[k] = (mated && side == 1) ? 1u : 0u;
    is2[k] = (mated && side == 2) ? 1u : 0u;
}

struct PairKeys {
    const uint32_t* order;
    const uint32_t* head;
    const uint32_t* head_scan;
    const uint32_t* info;
    const uint32_t* tid;
    const uint32_t* pos1;
    const uint32_t* pnext;
    __device__ uint32_t side(uint32_t k) const { return (info[order[k]] >> 18) & 3u; }
    __device__ uint64_t positions(uint32_t k) const { const uint32_t j = order[k]; return samc_pos_key((info[j] >> 18) & 3u, pos1[j], pnext[j]); }
    __device__ uint64_t frag_tid(uint32_t k) const { return (uint64_t)group_of(head, head_scan, k) << 32 | tid[order[k]]; }
};

// the mated positions, side-1 ones first, each side in the order of order[]: val[] and the key of the first sort
__global__ void k_samc_mated_list(uint32_t n, PairKeys pk, const uint32_t* __restrict__ is1, const uint32_t* __restrict__ is1_scan,
                                  const uint32_t* __restrict__ is2, const uint32_t* __restrict__ is2_scan, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n || !(is1[k] | is2[k])) return;
    const uint32_t at = is1[k] ? is1_scan[k] : is1_scan[n] + is2_scan[k];
    key[at] = pk.positions(k);
    val[at] = k;
}

__global__ void k_samc_second_keys(uint32_t m, PairKeys pk, const uint32_t* __restrict__ val, uint64_t* __restrict__ key) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < m) key[p] = pk.frag_tid(val[p]);
}

// behind both sorts: a run of one (fragment, tid, POS of mate 1, POS of mate 2) begins at p; side-1 lines
__global__ void k_samc_run_heads(uint32_t m, PairKeys pk, const uint32_t* __restrict__ val, uint32_t* __restrict__ run_head, uint32_t* __restrict__ one) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint32_t k = val[p];
    one[p] = pk.side(k) == 1 ? 1u : 0u;
    run_head[p] = (p == 0 || pk.frag_tid(k) != pk.frag_tid(val[p - 1]) || pk.positions(k) != pk.positions(val[p - 1])) ? 1u : 0u;
}

__global__ void k_samc_run_starts(uint32_t m, const uint32_t* __restrict__ run_head, const uint32_t* __restrict__ run_scan, uint32_t* __restrict__ run_start) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > m) return;
    if (p == m) { run_start[run_scan[m]] = m; return; }
    if (run_head[p]) run_start[run_scan[p]] = p;
}

// the i-th side-1 line of a run takes the i-th side-2 line (they stand behind the run's n1 side-1 lines) when there is one
__global__ void k_samc_partner(uint32_t m, const uint32_t* __restrict__ val, const uint32_t* __restrict__ run_head, const uint32_t* __restrict__ run_scan,
                               const uint32_t* __restrict__ run_start, const uint32_t* __restrict__ one, const uint32_t* __restrict__ one_scan,
                               const uint32_t* __restrict__ head, const uint32_t* __restrict__ head_scan, uint32_t* __restrict__ partner,
                               uint32_t* __restrict__ pair_head, uint32_t* __restrict__ has_pair) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m || !one[p]) return;
    const uint32_t r = run_scan[p] + run_head[p] - 1u, rs = run_start[r], re = run_start[r + 1];
    const uint32_t n1 = one_scan[re] - one_scan[rs], n2 = (re - rs) - n1, i = p - rs;
    if (i >= n2) return;
    const uint32_t k = val[p];
    partner[k] = val[rs + n1 + i];
    pair_head[k] = 1u;
    has_pair[group_of(head, head_scan, k)] = 1u;
}

// ---- emit -----------------------------------------------------------------------------------------------------------------

// samback.h's k_sam_write with the mate taken from partner[]: order[i] is relative to position k0 of rec_line[]
__global__ void k_samc_write(uint32_t n_hits, const uint32_t* __restrict__ order, uint32_t k0, const uint32_t* __restrict__ rec_line,
                             const uint32_t* __restrict__ pair_head, const uint32_t* __restrict__ partner, Lines lines, sfgpu_hit* __restrict__ hits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_hits) return;
    const uint32_t k = k0 + order[i];
    const SamLine a = lines(rec_line[k]);
    hits[i] = pair_head[k] ? sam_pair_hit(a, lines(rec_line[partner[k]])) : sam_single_hit(a);
}

}  // namespace
}  // namespace sfgpu

using namespace sfgpu;

struct sfgpu_samc {
    bool paired = false, finished = false;
    uint64_t n = 0;                               // lines collected
    uint64_t name_bytes = 0;                      // of the blob in use (a multiple of 16: the names of a call begin at a boundary)
    DevBuf<uint32_t> info, tid, pos1, pnext, name_len;
    DevBuf<int32_t> pos;
    DevBuf<uint64_t> name_at;
    DevBuf<uint4> blob;
    // from finish on
    uint32_t n_reads = 0;
    DevBuf<uint32_t> order, head, frag_start, partner, pair_head, has_pair;
    sfgpu_samc_info info_out = {};

    uint64_t state_bytes() const {
        uint64_t b = 0;
        for (const DevBuf<uint32_t>* a : {&info, &tid, &pos1, &pnext, &name_len, &order, &head, &frag_start, &partner, &pair_head, &has_pair}) b += a->cap * 4;
        return b + pos.cap * 4 + name_at.cap * 8 + blob.cap * 16;
    }
};

namespace {

int check_collect_args(const char* who, const void* handle, bool handle_paired, sfgpu_samc* c, const void* text, uint64_t n_bytes, sfgpu_sam_result* res) {
    if (!handle || !c || !res) { set_error("%s: null handle or result", who); return SFGPU_ERR_INVALID; }
    memset(res, 0, sizeof(*res));
    if (c->finished) { set_error("%s: the collection is finished", who); return SFGPU_ERR_STATE; }
    if (handle_paired != c->paired) { set_error("%s: the parser handle and the collection differ in `paired`", who); return SFGPU_ERR_INVALID; }
    if (n_bytes > kMaxBytes) { set_error("%s: more than 2^30 bytes in one call", who); return SFGPU_ERR_RANGE; }
    if (n_bytes && !text) { set_error("%s: null text", who); return SFGPU_ERR_INVALID; }
    return SFGPU_OK;
}

// K records of the call's text (record k = line rec_line[k] of the front end's arrays) behind the collection's lines
int append_records(sfgpu_samc* c, CollectScratch& S, const unsigned char* bytes, uint32_t K, const uint32_t* info, const uint32_t* tid, const int32_t* pos,
                   const uint32_t* qlen, hipStream_t st, uint32_t* h32) {
    if (K == 0) return SFGPU_OK;
    if (c->n + K >= kMaxLines) { set_error("sfgpu_samc: 2^32 - 1 lines or more in one collection"); return SFGPU_ERR_RANGE; }
    const uint64_t need = c->n + K;
    for (DevBuf<uint32_t>* b : {&c->info, &c->tid, &c->pos1, &c->pnext, &c->name_len}) if (int r = b->reserve(need, st, true, c->n)) return r;
    if (int r = c->pos.reserve(need, st, true, c->n)) return r;
    if (int r = c->name_at.reserve(need, st, true, c->n)) return r;
    for (DevBuf<uint32_t>* b : {&S.nlen, &S.nscan}) if (int r = b->reserve((uint64_t)K + 2, st, false)) return r;
    const LineArrays out{c->info.p, c->tid.p, c->pos.p, c->pos1.p, c->pnext.p, c->name_len.p};
    hipLaunchKernelGGL(k_samc_append, dim3(grid_of(K)), dim3(kBlock), 0, st, K, S.rec_line.p, info, tid, pos, S.pos1.p, S.pnext.p, qlen, c->n, out, S.nlen.p);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(S.nlen.p, S.nscan.p, K, st)) return r;      // (at most 2^30 bytes of text: the sum fits)
    SF_HIP(hipMemcpyAsync(&h32[0], S.nscan.p + K, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t n_name = h32[0];
    const uint64_t groups = (n_name + 15ull) / 16;
    if (int r = c->blob.reserve(c->name_bytes / 16 + groups + 1, st, true, c->name_bytes / 16)) return r;
    const uint64_t lanes = K > groups ? K : groups;
    hipLaunchKernelGGL(k_samc_names, dim3(grid_of(lanes)), dim3(kBlock), 0, st, bytes, K, n_name, S.nscan.p, S.rec_line.p, S.nsrc.p,
                       c->blob.p + c->name_bytes / 16, c->name_bytes, c->name_at.p + c->n);
    SF_CHECK_LAUNCH();
    SF_HIP(hipStreamSynchronize(st));
    c->n = need;
    c->name_bytes += groups * 16;
    return SFGPU_OK;
}

// The SAM text on the device: [0, n_text) ends in a '\n'; `used` of its bytes are the caller's.  h: 8 pinned 64-bit words.
int collect_sam_text(sfgpu_sam* m, sfgpu_samc* c, SamScratch& S, const uint4* text, uint64_t n_text, uint64_t used, sfgpu_sam_result* res, hipStream_t st, uint64_t* h) {
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(text);
    uint32_t* h32 = reinterpret_cast<uint32_t*>(h);
    samfront::Front& F = S.F;
    uint32_t L = 0;
    if (int r = samfront::sam_front_lines(m, F, text, n_text, st, h32, &L)) return r;
    if (L == 0) return SFGPU_OK;
    for (DevBuf<uint32_t>* b : {&S.pos1, &S.pnext, &S.qlen, &S.nsrc}) if (int r = b->reserve((uint64_t)L + 2, st, false)) return r;
    hipLaunchKernelGGL(k_samc_line_mates, dim3(grid_of(L)), dim3(kBlock), 0, st, bytes, L, F.line_end.p, F.tab_pos.p, c->paired ? 1 : 0, F.info.p, F.isrec.p,
                       S.pos1.p, S.pnext.p, S.qlen.p, S.nsrc.p, F.word.p);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(F.isrec.p, F.rec_scan.p, L, st)) return r;
    SF_HIP(hipMemcpyAsync(&h[1], F.word.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h32[0], F.rec_scan.p + L, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h[1] != kNoBad) {
        res->bad = (uint32_t)(h[1] & 0xffu);
        res->bad_line = h[1] >> 8;
        set_error("sfgpu_sam_collect: line %llu of the text is malformed (SFGPU_SAM_BAD_* %u)", (unsigned long long)res->bad_line, res->bad);
        return SFGPU_ERR_FORMAT;
    }
    const uint32_t K = h32[0];
    if (K) {
        if (int r = S.rec_line.reserve((uint64_t)K + 2, st, false)) return r;
        hipLaunchKernelGGL(samfront::k_sam_compact, dim3(grid_of(L)), dim3(kBlock), 0, st, L, F.isrec.p, F.rec_scan.p, S.rec_line.p);
        SF_CHECK_LAUNCH();
        if (int r = append_records(c, S, bytes, K, F.info.p, F.tid.p, F.pos.p, S.qlen.p, st, h32)) return r;
    }
    res->n_lines = L; res->n_header = L - K; res->consumed = used;
    return SFGPU_OK;
}

// The BAM stream on the device: bytes[0, n) in a buffer of whole 16-byte groups
int collect_bam_text(sfgpu_bam* m, sfgpu_samc* c, BamScratch& S, const unsigned char* bytes, uint64_t n, bool final, sfgpu_sam_result* res, hipStream_t st, uint64_t* h) {
    uint32_t* h32 = reinterpret_cast<uint32_t*>(h);
    const uint64_t skip = m->header_bytes > m->stream_pos ? m->header_bytes - m->stream_pos : 0;
    if (skip > n) {                                       // the header goes on: present more
        if (final) { res->consumed = n; m->stream_pos += n; }
        return SFGPU_OK;
    }
    bamfront::Chain& C = S.C;
    DevBuf<uint32_t>&info = S.info, &tid = S.tid, &name_len = S.name_len;
    DevBuf<int32_t>& pos = S.pos;
    DevBuf<unsigned long long>& word = S.word;
    uint32_t K = 0, last = 0;
    if (int r = bamfront::resolve_chain(C, bytes, (uint32_t)skip, (uint32_t)n, &K, &last, st, h32)) return r;
    const bool chain_bad = bam_ended(last) && (bam_broken(last) || final);     // BAD_FIELDS at record K
    h[1] = kNoBad;
    if (K) {
        for (DevBuf<uint32_t>* b : {&info, &tid, &name_len, &S.rec_line, &S.pos1, &S.pnext, &S.nsrc}) if (int r = b->reserve((uint64_t)K + 2, st, false)) return r;
        if (int r = pos.reserve((uint64_t)K + 2, st, false)) return r;
        if (int r = word.reserve(2, st, false)) return r;
        SF_HIP(hipMemsetAsync(word.p, 0xff, 8, st));
        hipLaunchKernelGGL(bamfront::k_bam_records, dim3(grid_of(K)), dim3(kBlock), 0, st, bytes, K, C.rec_off.p, c->paired ? 1 : 0, m->n_ref, m->ref_tid.p, info.p, tid.p,
                           pos.p, name_len.p, S.rec_line.p, word.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_samc_record_mates, dim3(grid_of(K)), dim3(kBlock), 0, st, bytes, K, C.rec_off.p, c->paired ? 1 : 0, info.p, S.pos1.p, S.pnext.p,
                           S.nsrc.p);
        SF_CHECK_LAUNCH();
        SF_HIP(hipMemcpyAsync(&h[1], word.p, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
    }
    if (h[1] != kNoBad || chain_bad) {
        res->bad = h[1] != kNoBad ? (uint32_t)(h[1] & 0xffu) : (uint32_t)SFGPU_SAM_BAD_FIELDS;
        res->bad_line = h[1] != kNoBad ? h[1] >> 8 : K;
        set_error("sfgpu_bam_collect: record %llu of the text is malformed (SFGPU_SAM_BAD_* %u)", (unsigned long long)res->bad_line, res->bad);
        return SFGPU_ERR_FORMAT;
    }
    if (int r = append_records(c, S, bytes, K, info.p, tid.p, pos.p, name_len.p, st, h32)) return r;
    const uint64_t consumed = bam_ended(last) ? (last & kBamAt) : n;      // (an incomplete record, text not final: up to where it begins)
    res->n_lines = K; res->consumed = consumed;
    m->stream_pos += consumed;
    return SFGPU_OK;
}

}  // namespace

extern "C" int sfgpu_samc_open(sfgpu_samc** out, int paired, sfgpu_stream stream) {
    (void)stream;
    SF_REQUIRE(out, SFGPU_ERR_INVALID, "sfgpu_samc_open: null handle");
    sfgpu_samc* c = new sfgpu_samc;
    c->paired = paired != 0;
    *out = c;
    return SFGPU_OK;
}

extern "C" int sfgpu_samc_close(sfgpu_samc* c) {
    if (!c) return SFGPU_OK;
    (void)hipDeviceSynchronize();
    delete c;
    return SFGPU_OK;
}

extern "C" int sfgpu_sam_collect_host(sfgpu_sam* m, sfgpu_samc* c, const char* h_text, uint64_t n_bytes, int final, sfgpu_sam_result* res,
                                      sfgpu_stream stream) {
    if (int r = check_collect_args("sfgpu_sam_collect_host", m, m && m->paired, c, h_text, n_bytes, res)) return r;
    hipStream_t st = as_stream(stream);
    uint64_t used = n_bytes;
    if (!final) while (used && h_text[used - 1] != '\n') --used;
    if (used == 0) return SFGPU_OK;
    const bool append = h_text[used - 1] != '\n';            // (final only)
    SamScratch S;
    CallScope scope;        // after S: it drains both streams before S's blocks go back to the pool
    HostStage H;
    if (int r = stage_host_text(scope, H, S.text, h_text, used, append, st)) return r;
    const int rc = collect_sam_text(m, c, S, S.text.p, used + (append ? 1 : 0), used, res, st, H.h);
    SF_HIP(hipEventRecord(H.ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_copy, H.ev_c0, H.ev_c1);
    add_elapsed(&res->ms_kernels, H.ev_k0, H.ev_k1);
    c->info_out.ms_collect += res->ms_kernels;
    return rc;
}

extern "C" int sfgpu_sam_collect_device(sfgpu_sam* m, sfgpu_samc* c, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final,
                                        sfgpu_sam_result* res, sfgpu_stream stream) {
    if (int r = check_collect_args("sfgpu_sam_collect_device", m, m && m->paired, c, d_text, n_bytes, res)) return r;
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_sam_collect_device: d_text must be 16-byte aligned");
    SF_REQUIRE(n_bytes == 0 || cap_text >= ((n_bytes + 1 + 15) & ~15ull) + 16, SFGPU_ERR_INVALID,
               "sfgpu_sam_collect_device: cap_text must hold the text, a '\\n', the rest of that 16-byte group and one group more");
    if (n_bytes == 0) return SFGPU_OK;
    hipStream_t st = as_stream(stream);
    SamScratch S;
    DevBuf<unsigned long long> last;
    CallScope scope;        // after the scratch, as in sfgpu_sam_collect_host
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;
    uint64_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_k0));
    SF_HIP(scope.event(&ev_k1));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint64_t)));
    if (int r = last.reserve(1, st, false)) return r;
    SF_HIP(hipEventRecord(ev_k0, st));
    SF_HIP(hipMemsetAsync(last.p, 0, 8, st));
    hipLaunchKernelGGL(textlines::k_last_nl, dim3(grid_of((n_bytes + 15) / 16)), dim3(kBlock), 0, st, d_text, n_bytes, last.p);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(&h[7], last.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint64_t used = final ? n_bytes : h[7];
    int rc = SFGPU_OK;
    if (used) {
        uint64_t n_text = used;
        if (final && h[7] != n_bytes) {                      // the last line lacks its '\n': it goes into the slack
            SF_HIP(hipMemsetAsync(d_text + n_bytes, '\n', 1, st));
            n_text = n_bytes + 1;
        }
        rc = collect_sam_text(m, c, S, reinterpret_cast<const uint4*>(d_text), n_text, used, res, st, h);
    }
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_kernels, ev_k0, ev_k1);
    c->info_out.ms_collect += res->ms_kernels;
    return rc;
}

extern "C" int sfgpu_bam_collect_host(sfgpu_bam* m, sfgpu_samc* c, const char* h_text, uint64_t n_bytes, int final, sfgpu_sam_result* res,
                                      sfgpu_stream stream) {
    if (int r = check_collect_args("sfgpu_bam_collect_host", m, m && m->names->paired, c, h_text, n_bytes, res)) return r;
    if (n_bytes == 0) return SFGPU_OK;
    hipStream_t st = as_stream(stream);
    BamScratch S;
    CallScope scope;        // after S, as in sfgpu_sam_collect_host
    HostStage H;
    if (int r = stage_host_text(scope, H, S.text, h_text, n_bytes, false, st)) return r;
    const int rc = collect_bam_text(m, c, S, reinterpret_cast<const unsigned char*>(S.text.p), n_bytes, final != 0, res, st, H.h);
    SF_HIP(hipEventRecord(H.ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_copy, H.ev_c0, H.ev_c1);
    add_elapsed(&res->ms_kernels, H.ev_k0, H.ev_k1);
    c->info_out.ms_collect += res->ms_kernels;
    return rc;
}

extern "C" int sfgpu_bam_collect_device(sfgpu_bam* m, sfgpu_samc* c, uint8_t* d_text, uint64_t n_bytes, uint64_t cap_text, int final,
                                        sfgpu_sam_result* res, sfgpu_stream stream) {
    if (int r = check_collect_args("sfgpu_bam_collect_device", m, m && m->names->paired, c, d_text, n_bytes, res)) return r;
    SF_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15u) == 0, SFGPU_ERR_INVALID, "sfgpu_bam_collect_device: d_text must be 16-byte aligned");
    SF_REQUIRE(n_bytes == 0 || cap_text >= ((n_bytes + 1 + 15) & ~15ull) + 16, SFGPU_ERR_INVALID,
               "sfgpu_bam_collect_device: cap_text must hold the text, one byte more, the rest of that 16-byte group and one group more");
    if (n_bytes == 0) return SFGPU_OK;
    hipStream_t st = as_stream(stream);
    BamScratch S;
    CallScope scope;        // after S
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;
    uint64_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_k0));
    SF_HIP(scope.event(&ev_k1));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint64_t)));
    SF_HIP(hipEventRecord(ev_k0, st));
    const int rc = collect_bam_text(m, c, S, d_text, n_bytes, final != 0, res, st, h);
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_kernels, ev_k0, ev_k1);
    c->info_out.ms_collect += res->ms_kernels;
    return rc;
}

extern "C" int sfgpu_samc_finish(sfgpu_samc* c, sfgpu_samc_info* info, sfgpu_stream stream) {
    SF_REQUIRE(c && info, SFGPU_ERR_INVALID, "sfgpu_samc_finish: null handle or info");
    SF_REQUIRE(!c->finished, SFGPU_ERR_STATE, "sfgpu_samc_finish: the collection is finished already");
    hipStream_t st = as_stream(stream);
    const uint32_t n = (uint32_t)c->n;
    ranksort::RankScratch R;
    DevBuf<uint32_t> perm, run, first, iota, head_scan, is1, is1_scan, is2, is2_scan, val, val2, val3, run_head, run_scan, run_start, one, one_scan, surv,
        surv_scan;
    DevBuf<uint64_t> key, key2;
    DevBuf<unsigned long long> word;
    CallScope scope;        // after the scratch
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;
    uint64_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_k0));
    SF_HIP(scope.event(&ev_k1));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint64_t)));
    uint32_t* h32 = reinterpret_cast<uint32_t*>(h);
    SF_HIP(hipEventRecord(ev_k0, st));
    sfgpu_samc_info& I = c->info_out;
    I.n_lines = n;
    if (int r = c->frag_start.reserve(2, st, false)) return r;
    if (n == 0) SF_HIP(hipMemsetAsync(c->frag_start.p, 0, 4, st));
    if (n) {
        // ---- the fragments
        uint32_t n_names = 0;
        const LenNames names{reinterpret_cast<const unsigned char*>(c->blob.p), c->name_at.p, c->name_len.p};
        if (int r = ranksort::rank_strings(names, n, R, perm, run, &n_names, &I.sort_rounds, h32, st)) return r;
        for (DevBuf<uint32_t>* b : {&first, &iota, &head_scan, &c->order, &c->head, &c->partner, &c->pair_head, &surv, &surv_scan})
            if (int r = b->reserve((uint64_t)n + 2, st, false)) return r;
        for (DevBuf<uint32_t>* b : {&c->frag_start, &c->has_pair}) if (int r = b->reserve((uint64_t)n_names + 2, st, false)) return r;
        for (DevBuf<uint64_t>* b : {&key, &key2}) if (int r = b->reserve((uint64_t)n + 2, st, false)) return r;
        if (int r = word.reserve(2, st, false)) return r;
        hipLaunchKernelGGL(k_samc_first, dim3(grid_of(n)), dim3(kBlock), 0, st, n, perm.p, run.p, first.p);
        SF_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_samc_frag_keys, dim3(grid_of(n)), dim3(kBlock), 0, st, n, perm.p, run.p, first.p, key.p, iota.p);
        SF_CHECK_LAUNCH();
        if (int r = sort_pairs_u64_u32(key.p, key2.p, iota.p, c->order.p, n, st, 32, false)) return r;
        hipLaunchKernelGGL(k_samc_heads, dim3(grid_of(n)), dim3(kBlock), 0, st, n, key2.p, c->head.p);
        SF_CHECK_LAUNCH();
        if (int r = exclusive_scan_u32_u32(c->head.p, head_scan.p, n, st)) return r;
        hipLaunchKernelGGL(k_samc_frag_starts, dim3(grid_of((uint64_t)n + 1)), dim3(kBlock), 0, st, n, c->head.p, head_scan.p, c->frag_start.p);
        SF_CHECK_LAUNCH();
        c->n_reads = n_names;

        // ---- the pairs
        SF_HIP(hipMemsetAsync(c->partner.p, 0xff, (uint64_t)n * 4, st));
        SF_HIP(hipMemsetAsync(c->pair_head.p, 0, (uint64_t)n * 4, st));
        SF_HIP(hipMemsetAsync(c->has_pair.p, 0, (uint64_t)n_names * 4, st));
        if (c->paired) {
            for (DevBuf<uint32_t>* b : {&is1, &is1_scan, &is2, &is2_scan}) if (int r = b->reserve((uint64_t)n + 2, st, false)) return r;
            hipLaunchKernelGGL(k_samc_mated, dim3(grid_of(n)), dim3(kBlock), 0, st, n, c->order.p, c->info.p, c->pnext.p, is1.p, is2.p);
            SF_CHECK_LAUNCH();
            if (int r = exclusive_scan_u32_u32(is1.p, is1_scan.p, n, st)) return r;
            if (int r = exclusive_scan_u32_u32(is2.p, is2_scan.p, n, st)) return r;
            SF_HIP(hipMemcpyAsync(&h32[0], is1_scan.p + n, 4, hipMemcpyDeviceToHost, st));
            SF_HIP(hipMemcpyAsync(&h32[1], is2_scan.p + n, 4, hipMemcpyDeviceToHost, st));
            SF_HIP(hipStreamSynchronize(st));
            const uint32_t m = h32[0] + h32[1];
            if (h32[0] && h32[1]) {
                for (DevBuf<uint32_t>* b : {&val, &val2, &val3, &run_head, &run_scan, &run_start, &one, &one_scan}) if (int r = b->reserve((uint64_t)m + 2, st, false)) return r;
                const PairKeys pk{c->order.p, c->head.p, head_scan.p, c->info.p, c->tid.p, c->pos1.p, c->pnext.p};
                hipLaunchKernelGGL(k_samc_mated_list, dim3(grid_of(n)), dim3(kBlock), 0, st, n, pk, is1.p, is1_scan.p, is2.p, is2_scan.p, key.p, val.p);
                SF_CHECK_LAUNCH();
                if (int r = sort_pairs_u64_u32(key.p, key2.p, val.p, val2.p, m, st, 64, false)) return r;
                hipLaunchKernelGGL(k_samc_second_keys, dim3(grid_of(m)), dim3(kBlock), 0, st, m, pk, val2.p, key.p);
                SF_CHECK_LAUNCH();
                if (int r = sort_pairs_u64_u32(key.p, key2.p, val2.p, val3.p, m, st, 64, false)) return r;
                hipLaunchKernelGGL(k_samc_run_heads, dim3(grid_of(m)), dim3(kBlock), 0, st, m, pk, val3.p, run_head.p, one.p);
                SF_CHECK_LAUNCH();
                if (int r = exclusive_scan_u32_u32(run_head.p, run_scan.p, m, st)) return r;
                if (int r = exclusive_scan_u32_u32(one.p, one_scan.p, m, st)) return r;
                hipLaunchKernelGGL(k_samc_run_starts, dim3(grid_of((uint64_t)m + 1)), dim3(kBlock), 0, st, m, run_head.p, run_scan.p, run_start.p);
                SF_CHECK_LAUNCH();
                hipLaunchKernelGGL(k_samc_partner, dim3(grid_of(m)), dim3(kBlock), 0, st, m, val3.p, run_head.p, run_scan.p, run_start.p, one.p, one_scan.p,
                                   c->head.p, head_scan.p, c->partner.p, c->pair_head.p, c->has_pair.p);
                SF_CHECK_LAUNCH();
            }
        }

        // ---- what the collection yields
        const Lines lines{c->info.p, c->tid.p, c->pos.p};
        SF_HIP(hipMemsetAsync(word.p, 0, 16, st));
        hipLaunchKernelGGL(k_sam_survive, dim3(grid_of(n)), dim3(kBlock), 0, st, n, n, c->order.p, c->head.p, head_scan.p, lines, c->pair_head.p, c->has_pair.p,
                           surv.p, word.p + 1);
        SF_CHECK_LAUNCH();
        if (int r = exclusive_scan_u32_u32(surv.p, surv_scan.p, n, st)) return r;
        SF_HIP(hipMemcpyAsync(&h32[0], surv_scan.p + n, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(&h32[1], head_scan.p + n, 4, hipMemcpyDeviceToHost, st));
        SF_HIP(hipMemcpyAsync(&h[1], word.p + 1, 8, hipMemcpyDeviceToHost, st));
        SF_HIP(hipStreamSynchronize(st));
        I.n_hits = h32[0]; I.n_pairs = h[1];
        if (h32[1] != n_names) { set_error("sfgpu_samc_finish: the name sort and the fragment order disagree (%u names, %u fragments)", n_names, h32[1]); return SFGPU_ERR_HIP; }
    }
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&I.ms_finish, ev_k0, ev_k1);
    I.n_reads = c->n_reads;
    c->finished = true;
    I.state_bytes = c->state_bytes();
    *info = I;
    return SFGPU_OK;
}

extern "C" int sfgpu_samc_emit(sfgpu_samc* c, uint64_t first_read, uint64_t n_reads, sfgpu_hit* d_hits, uint64_t cap_hits, uint32_t* d_off,
                               sfgpu_sam_result* res, sfgpu_stream stream) {
    if (!c || !res) { set_error("sfgpu_samc_emit: null handle or result"); return SFGPU_ERR_INVALID; }
    memset(res, 0, sizeof(*res));
    SF_REQUIRE(c->finished, SFGPU_ERR_STATE, "sfgpu_samc_emit: the collection is not finished");
    SF_REQUIRE(d_off && (!cap_hits || d_hits), SFGPU_ERR_INVALID, "sfgpu_samc_emit: null array");
    SF_REQUIRE(first_read <= c->n_reads && n_reads <= c->n_reads - first_read, SFGPU_ERR_RANGE, "sfgpu_samc_emit: the slice reaches beyond the collection's fragments");
    hipStream_t st = as_stream(stream);
    DevBuf<uint32_t> head_scan, surv, surv_scan, val, val2;
    DevBuf<uint64_t> key, key2;
    DevBuf<unsigned long long> word;
    CallScope scope;        // after the scratch
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;
    uint64_t* h = nullptr;
    SF_HIP(scope.adopt(st));
    SF_HIP(scope.event(&ev_k0));
    SF_HIP(scope.event(&ev_k1));
    SF_HIP(scope.pinned_block(&h, 8 * sizeof(uint64_t)));
    uint32_t* h32 = reinterpret_cast<uint32_t*>(h);
    SF_HIP(hipEventRecord(ev_k0, st));
    if (n_reads == 0) {
        SF_HIP(hipMemsetAsync(d_off, 0, 4, st));
        SF_HIP(hipStreamSynchronize(st));
        return SFGPU_OK;
    }
    SF_HIP(hipMemcpyAsync(&h32[0], c->frag_start.p + first_read, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h32[1], c->frag_start.p + first_read + n_reads, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t k0 = h32[0], K = h32[1] - h32[0];       // (K >= n_reads >= 1: every fragment has a line)
    for (DevBuf<uint32_t>* b : {&head_scan, &surv, &surv_scan}) if (int r = b->reserve((uint64_t)K + 2, st, false)) return r;
    if (int r = word.reserve(1, st, false)) return r;
    SF_HIP(hipMemsetAsync(word.p, 0, 8, st));
    const Lines lines{c->info.p, c->tid.p, c->pos.p};
    if (int r = exclusive_scan_u32_u32(c->head.p + k0, head_scan.p, K, st)) return r;      // `group` relative to the slice
    hipLaunchKernelGGL(k_sam_survive, dim3(grid_of(K)), dim3(kBlock), 0, st, K, K, c->order.p + k0, c->head.p + k0, head_scan.p, lines, c->pair_head.p + k0,
                       c->has_pair.p + first_read, surv.p, word.p);
    SF_CHECK_LAUNCH();
    if (int r = exclusive_scan_u32_u32(surv.p, surv_scan.p, K, st)) return r;
    SF_HIP(hipMemcpyAsync(&h32[0], surv_scan.p + K, 4, hipMemcpyDeviceToHost, st));
    SF_HIP(hipMemcpyAsync(&h[1], word.p, 8, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    const uint32_t n_hits = h32[0];
    if (n_hits > cap_hits) {
        res->need_hits = n_hits; res->need_reads = n_reads;
        set_error("sfgpu_samc_emit: %u records do not fit cap_hits = %llu", n_hits, (unsigned long long)cap_hits);
        return SFGPU_ERR_CAPACITY;
    }
    for (DevBuf<uint64_t>* b : {&key, &key2}) if (int r = b->reserve((uint64_t)n_hits + 2, st, false)) return r;
    for (DevBuf<uint32_t>* b : {&val, &val2}) if (int r = b->reserve((uint64_t)n_hits + 2, st, false)) return r;
    hipLaunchKernelGGL(k_sam_keys, dim3(grid_of(K)), dim3(kBlock), 0, st, K, c->order.p + k0, c->head.p + k0, head_scan.p, lines, surv.p, surv_scan.p, d_off,
                       key.p, val.p);
    SF_CHECK_LAUNCH();
    SF_HIP(hipMemcpyAsync(d_off + n_reads, surv_scan.p + K, 4, hipMemcpyDeviceToDevice, st));
    if (n_hits) {
        int group_bits = 1;
        while (group_bits < 31 && (1u << group_bits) < n_reads) ++group_bits;
        if (int r = sort_pairs_u64_u32(key.p, key2.p, val.p, val2.p, n_hits, st, 33 + group_bits, false)) return r;
        hipLaunchKernelGGL(k_samc_write, dim3(grid_of(n_hits)), dim3(kBlock), 0, st, n_hits, val2.p, k0, c->order.p, c->pair_head.p, c->partner.p, lines, d_hits);
        SF_CHECK_LAUNCH();
    }
    SF_HIP(hipEventRecord(ev_k1, st));
    SF_HIP(hipStreamSynchronize(st));
    add_elapsed(&res->ms_kernels, ev_k0, ev_k1);
    res->n_reads = n_reads; res->n_hits = n_hits; res->n_pairs = h[1];
    return SFGPU_OK;
}
