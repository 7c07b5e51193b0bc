// aligngfmt.h -- gapped alignment of a job: the path through verifygfmt.h's band, as CIGAR words and a position, stated once.  Plain
// C++, host and device, on top of verifygfmt.h: the same cells D[i][d], the same sub, the free start row, the band k = max_indel
// (1 .. 15).  align_gapped.hip runs the band (hitgroup.h: hit_band_dev) and ag_walk below inside its kernel, tests/aligng_harness.cpp runs them alone
// (ag_serial_align), and hits.align_hits_host is the Python statement both are judged by.  The tie rules are part of the contract.
//
// CANDIDATES of cell (i, d):  DIAG iff D[i-1][d] + sub(i, pos + i + d) == D[i][d];  INS iff d < k and D[i-1][d+1] + 1 == D[i][d];
//          DEL iff d > -k and D[i][d-1] + 1 == D[i][d].  (Every cell of rows 0 .. len - 1 has one.)
// END      among the d with D[len-1][d] == edits the one of least |d|; on a tie the negative one.
// WALK     back from (len - 1, d_end) until i == -1.  If the column chosen just before (the one to its right) was DEL and DEL is a
//          candidate, DEL; else if it was INS and INS is a candidate, INS; else the first candidate of DIAG, INS, DEL.  DIAG emits an M
//          column (i, x = pos + i + d), then i -= 1; INS an I column (i), then i -= 1, d += 1; DEL a D column (x = pos + i + d), then
//          d -= 1.  (The continuation preference keeps a gap of two bases one run.)
// TRIM     at either end columns are dropped until an M column with 0 <= x < tlen remains: dropped M and I columns are that end's
//          soft clip, dropped D columns vanish.  No column left: the job is UNALIGNABLE and has 0 operations (x0 = 0, nm = 0, and
//          `clipped` counts all its bases).  A job of 0 bases is unalignable.
// RESULT   x0: the transcript position of the first remaining column; the operations as BAM CIGAR words len << 4 | op (M 0, I 1, D 2,
//          S 4), adjacent equal columns merged, in reference order (the job's bases are oriented: SAM's order); nm: the remaining M
//          columns whose sub is 1 plus the I and D columns; clipped: the bases in S.  nm + clipped + trimmed D columns == edits.
//          A job whose ungapped count is 0 gets <len>M at pos from the rule itself; the lanes skip the recurrence for it.
// SLOTS    two per record: slot 2 h + j is job j of record h (verifyfmt.h's jobs); a record's missing second job is an empty slot
//          (x0 = 0, nm = 0, no operations) and no job.
// STATS    jobs; jobs_traced (ungapped count > 0: the recurrence ran); unalignable; sum_nm; words (operations over all slots);
//          scratch_bytes (of the largest slice; the whole batch's, 8 * width * ceil(len / 16) per traced job, where nothing is sliced).
//
// Lanes are DIAGONALS, as in verifygfmt.h, and the forward pass IS its band function handed `cells` (vg_band_group; hit_band_dev on
// the device): its row plus one exchange, the lower neighbour's new cell; ag_lane_cand (stated there, beside the row it reads)
// turns a row into 4 bits a lane -- the three candidates and sub -- and every kVfStep rows a lane has one 64-bit word: step q of a job is `width` consecutive words.  ag_walk walks back over those words, the
// same in every lane of the group (`fetch` hands it lane l's word of step q), and streams its columns into ag_column, which merges,
// trims and, given the slot's place [lo, hi) in the operations, writes each run where it belongs, from the right end: the first pass
// (ops == nullptr) only counts.  Operation lengths are 28 bits: mates shorter than 2^28 bases.
#pragma once
#include "verifygfmt.h"

namespace sfgpu {

constexpr uint32_t kAgM = 0u, kAgI = 1u, kAgD = 2u, kAgS = 4u;              // BAM's operation codes
constexpr uint32_t kAgOff = 3u;                                            // here only: an M column off the transcript

VF_HD uint64_t ag_steps(uint64_t len) { return (len + kVfStep - 1u) / kVfStep; }
VF_HD uint64_t ag_scratch_bytes(uint64_t len, uint32_t width) { return 8ull * width * ag_steps(len); }

// WALK's choice (a cell without a candidate does not exist; it would be taken as DIAG, so that the walk ends)
VF_HD uint32_t ag_pick(uint32_t cand, uint32_t prev) {
    if (prev == kAgDel && (cand & kAgDel)) return kAgDel;
    if (prev == kAgIns && (cand & kAgIns)) return kAgIns;
    return (cand & kAgDiag) ? kAgDiag : (cand & kAgIns) ? kAgIns : (cand & kAgDel) ? kAgDel : kAgDiag;
}

// ---- the columns of a walk, from the right end to the left: TRIM and RESULT as a stream -----------------------------------------
// x never rises along a walk, so M columns off the transcript come first (x >= tlen) or last (x < 0); they are their own kind of
// run (kAgOff) and a run is kept or dropped as a whole.
struct AgTrace {
    uint32_t started;      // an M column on the transcript has been seen
    uint32_t kind, run;    // the open run
    uint32_t runs;         // runs begun since `started`, the open one included
    uint32_t kept;         // ... up to the last run of M columns on the transcript: the runs that remain
    uint32_t clip_r;       // M and I columns in front of the first kept one: the right end's soft clip
    uint32_t tail, tail_d; // M / I and D columns since the last kept one: the left end's soft clip and trimmed D, once the walk ends
    uint32_t head_d;       // D columns in front of the first kept column
    uint32_t nm, nm_tail;  // nm up to the last kept column; I and D columns since
    int64_t x0;            // x of the last kept column
};
VF_HD uint32_t ag_n_ops(const AgTrace& w) { return w.started ? w.kept + (w.tail ? 1u : 0u) + (w.clip_r ? 1u : 0u) : 0u; }
VF_HD uint32_t ag_clipped(const AgTrace& w) { return w.clip_r + w.tail; }
VF_HD uint32_t ag_trimmed_d(const AgTrace& w) { return w.head_d + w.tail_d; }
// the open run to its place: run number r from the right (0-based) of a slot [lo, hi) is word hi - (clip_r > 0) - 1 - r.  A run
// that will not remain may be handed in: it falls in front of lo, or on lo where the left clip is written over it afterwards.
VF_HD void ag_close(const AgTrace& w, uint32_t* ops, int64_t lo, int64_t hi) {
    if (!ops || !w.started || w.kind == kAgOff) return;
    const int64_t at = hi - (w.clip_r ? 1 : 0) - (int64_t)w.runs;
    if (at >= lo && at < hi) ops[at] = w.run << 4 | w.kind;
}
VF_HD void ag_column(AgTrace& w, uint32_t kind /* kAgM, kAgI, kAgD, kAgOff */, int64_t x, uint32_t sub, uint32_t* ops, int64_t lo, int64_t hi) {
    if (!w.started) {
        if (kind != kAgM) { w.clip_r += kind != kAgD; w.head_d += kind == kAgD; return; }
        w.started = 1u; w.kind = kAgM; w.run = 0u; w.runs = 1u;
    } else if (kind != w.kind) {
        ag_close(w, ops, lo, hi);
        w.kind = kind; w.run = 0u; ++w.runs;
    }
    ++w.run;
    if (kind == kAgM) { w.kept = w.runs; w.nm += w.nm_tail + sub; w.nm_tail = 0u; w.tail = 0u; w.tail_d = 0u; w.x0 = x; }
    else { w.nm_tail += kind != kAgOff; w.tail += kind != kAgD; w.tail_d += kind == kAgD; }
}
VF_HD void ag_finish(AgTrace& w, uint32_t* ops, int64_t lo, int64_t hi) {
    ag_close(w, ops, lo, hi);
    if (!w.started) { w.nm = 0u; w.x0 = 0; return; }
    if (ops && w.tail && lo < hi) ops[lo] = w.tail << 4 | kAgS;
    if (ops && w.clip_r && lo < hi) ops[hi - 1] = w.clip_r << 4 | kAgS;
}
// a job whose ungapped count is 0 (len > 0): what the walk gives without walking
VF_HD AgTrace ag_all_match(uint64_t len, int64_t pos, uint32_t* ops, int64_t lo, int64_t hi) {
    AgTrace w{};
    w.started = 1u; w.kind = kAgM; w.run = (uint32_t)len; w.runs = w.kept = 1u; w.x0 = pos;
    ag_close(w, ops, lo, hi);
    return w;
}

// WALK over the stored cells: fetch(q, l) -> lane l's word of step q (rows 16 q .. 16 q + 15, 4 bits a row)
template <typename Fetch>
VF_HD AgTrace ag_walk(uint64_t len, int64_t pos, uint64_t tlen, uint32_t k, uint32_t lane_end, Fetch& fetch, uint32_t* ops, int64_t lo, int64_t hi) {
    AgTrace w{};
    int64_t i = (int64_t)len - 1;
    uint32_t lane = lane_end, prev = 0u;
    while (i >= 0) {
        const uint64_t word = fetch((uint64_t)i / kVfStep, lane);
        const uint32_t c = (uint32_t)(word >> (4u * ((uint32_t)i % kVfStep))) & 0xFu;
        const uint32_t op = ag_pick(c & 7u, prev);
        const int64_t x = pos + i + (int64_t)lane - (int64_t)k;
        if (op == kAgDiag) { ag_column(w, (x >= 0 && x < (int64_t)tlen) ? kAgM : kAgOff, x, c >> 3, ops, lo, hi); --i; }
        else if (op == kAgIns) { ag_column(w, kAgI, x, 1u, ops, lo, hi); --i; ++lane; }
        else { ag_column(w, kAgD, x, 1u, ops, lo, hi); --lane; }
        prev = op;
    }
    ag_finish(w, ops, lo, hi);
    return w;
}

#if !defined(__HIPCC__)
struct AgAlignment { int64_t x0; uint64_t nm, clipped, trimmed_d, edits; std::vector<uint32_t> ops; };

// ---- the rule in plain loops: the whole matrix, the walk into a list of columns, then TRIM and RESULT on the list ----------------
inline AgAlignment ag_job_serial(const char* r, uint64_t len, bool fwd, const char* t, uint64_t tlen, int64_t pos, uint32_t k) {
    AgAlignment out{0, 0, 0, 0, 0, {}};
    if (len == 0) return out;
    const uint32_t n = 2u * k + 1u;
    std::vector<uint64_t> D((len + 1) * n, 0);                      // row i is D[(i + 1) * n ..]
    std::vector<uint8_t> S(len * n);
    for (uint64_t i = 0; i < len; ++i) {
        const uint32_t a = vf_oriented(vf_code((unsigned char)(fwd ? r[i] : r[len - 1 - i])), fwd);
        const uint64_t* P = &D[i * n];
        uint64_t* C = &D[(i + 1) * n];
        for (uint32_t l = 0; l < n; ++l) {
            const int64_t x = pos + (int64_t)i + (int64_t)l - (int64_t)k;
            const bool on = x >= 0 && x < (int64_t)tlen;
            S[i * n + l] = (on && a <= 3u && vf_code((unsigned char)t[x]) == a) ? 0u : 1u;
            uint64_t v = P[l] + S[i * n + l];
            if (l + 1u < n && P[l + 1u] + 1u < v) v = P[l + 1u] + 1u;
            C[l] = v;
        }
        for (uint32_t l = 1; l < n; ++l) if (C[l - 1u] + 1u < C[l]) C[l] = C[l - 1u] + 1u;
    }
    const uint64_t* L = &D[len * n];
    out.edits = L[0];
    for (uint32_t l = 1; l < n; ++l) out.edits = L[l] < out.edits ? L[l] : out.edits;
    int64_t d = 0;
    for (int64_t a = 0; a <= (int64_t)k; ++a) {
        if (L[k - a] == out.edits) { d = -a; break; }
        if (L[k + a] == out.edits) { d = a; break; }
    }
    struct Col { uint32_t kind; int64_t x; uint32_t sub; };
    std::vector<Col> cols;
    int64_t i = (int64_t)len - 1;
    uint32_t prev = 0;
    while (i >= 0) {
        const uint32_t l = (uint32_t)(d + (int64_t)k);
        const uint64_t here = D[(i + 1) * n + l];
        const bool diag = D[i * n + l] + S[i * n + l] == here, ins = d < (int64_t)k && D[i * n + l + 1u] + 1u == here,
                   del = d > -(int64_t)k && D[(i + 1) * n + l - 1u] + 1u == here;
        uint32_t op;
        if (prev == kAgDel && del) op = kAgDel;
        else if (prev == kAgIns && ins) op = kAgIns;
        else op = diag ? kAgDiag : ins ? kAgIns : kAgDel;
        const int64_t x = pos + i + d;
        if (op == kAgDiag) { cols.push_back(Col{kAgM, x, S[i * n + l]}); --i; }
        else if (op == kAgIns) { cols.push_back(Col{kAgI, x, 1u}); --i; ++d; }
        else { cols.push_back(Col{kAgD, x, 1u}); --d; }
        prev = op;
    }
    std::vector<Col> c(cols.rbegin(), cols.rend());                  // reference order
    auto remains = [&](const Col& q) { return q.kind == kAgM && q.x >= 0 && q.x < (int64_t)tlen; };
    size_t a = 0, b = c.size();
    uint64_t clip_l = 0, clip_r = 0;
    while (a < b && !remains(c[a])) { if (c[a].kind == kAgD) ++out.trimmed_d; else ++clip_l; ++a; }
    while (b > a && !remains(c[b - 1])) { if (c[b - 1].kind == kAgD) ++out.trimmed_d; else ++clip_r; --b; }
    out.clipped = clip_l + clip_r;
    if (a == b) return out;
    out.x0 = c[a].x;
    if (clip_l) out.ops.push_back((uint32_t)clip_l << 4 | kAgS);
    for (size_t j = a; j < b; ++j) {
        out.nm += c[j].sub;
        if (j > a && c[j].kind == c[j - 1].kind) out.ops.back() += 1u << 4;
        else out.ops.push_back(1u << 4 | c[j].kind);
    }
    if (clip_r) out.ops.push_back((uint32_t)clip_r << 4 | kAgS);
    return out;
}

// ... and as a group of vg_width(k) lanes runs it: the shortcut, the forward pass into scratch, the walk twice (count, then write)
inline AgAlignment ag_job_lanes(const char* r, uint64_t len, bool fwd, const char* t, uint64_t tlen, int64_t pos, uint32_t k, uint64_t ungapped) {
    AgAlignment out{0, 0, 0, 0, 0, {}};
    if (len == 0) return out;
    AgTrace w;
    if (ungapped == 0) {
        out.ops.resize(1);
        w = ag_all_match(len, pos, out.ops.data(), 0, 1);
    } else {
        const uint32_t width = vg_width(k);
        std::vector<uint64_t> cells(width * ag_steps(len));
        uint32_t lane_end = 0;
        vg_band_group(r, len, fwd, t, tlen, pos, k, width, 0, cells.data(), &lane_end);
        auto fetch = [&](uint64_t q, uint32_t l) { return cells[q * width + l]; };
        w = ag_walk(len, pos, tlen, k, lane_end, fetch, nullptr, 0, 0);
        out.ops.assign(ag_n_ops(w), 0xFFFFFFFFu);
        const AgTrace again = ag_walk(len, pos, tlen, k, lane_end, fetch, out.ops.data(), 0, (int64_t)out.ops.size());
        if (ag_n_ops(again) != ag_n_ops(w)) out.ops.assign(1, 0xFFFFFFFFu);      // (never: the harness would report it)
    }
    out.x0 = w.x0; out.nm = w.nm; out.clipped = ag_clipped(w); out.trimmed_d = ag_trimmed_d(w);
    out.edits = out.nm + out.clipped + out.trimmed_d;
    return out;
}

// the whole pass, serially (lanes = false: ag_job_serial for every job; true: as the kernel lays it out).  Outputs per slot; `extra`
// (may be null) gets {clipped, trimmed_d, edits} per slot.  -> 0, or 1 + the lowest record with tid >= M (nothing is emitted then)
inline uint64_t ag_serial_align(const char* tseq, const uint64_t* tseq_off, const uint32_t* tlen, uint64_t M, const char* seq1, const uint64_t* off1,
                                const char* seq2, const uint64_t* off2, uint32_t n_reads, const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t k,
                                bool lanes, std::vector<int32_t>* pos, std::vector<uint32_t>* nm, std::vector<uint64_t>* op_off, std::vector<uint32_t>* ops,
                                std::vector<uint64_t>* extra, sfgpu_align_gstats* stats) {
    const VfBatch b{tseq, tseq_off, tlen, M, seq1, off1, seq2, off2, n_reads, hits, hit_off};
    if (const uint64_t bad = vf_bad_tid(b)) return bad;
    const uint64_t n = b.n_rec();
    *stats = sfgpu_align_gstats{};
    pos->assign(2 * n, 0); nm->assign(2 * n, 0u); ops->clear();
    if (extra) extra->assign(6 * n, 0ull);
    std::vector<uint64_t> words(2 * n, 0ull);                        // operations per slot
    vf_each_job(b, [&](uint32_t, uint32_t i, uint32_t j, const char* mate, uint64_t len, const char* tx, uint64_t tl, bool fwd, int64_t p) {
        const VfCount c = vf_job_serial(mate, len, fwd, tx, tl, p);
        const uint64_t ungapped = c.mism + c.over;
        const AgAlignment a = lanes ? ag_job_lanes(mate, len, fwd, tx, tl, p, k, ungapped) : ag_job_serial(mate, len, fwd, tx, tl, p, k);
        const uint64_t s = 2ull * i + j;
        (*pos)[s] = (int32_t)a.x0; (*nm)[s] = (uint32_t)a.nm; words[s] = a.ops.size();
        ops->insert(ops->end(), a.ops.begin(), a.ops.end());
        if (extra) { (*extra)[3 * s] = a.clipped; (*extra)[3 * s + 1] = a.trimmed_d; (*extra)[3 * s + 2] = a.edits; }
        ++stats->jobs; stats->jobs_traced += ungapped > 0; stats->unalignable += a.ops.empty(); stats->sum_nm += a.nm;
        if (ungapped > 0) stats->scratch_bytes += ag_scratch_bytes(len, vg_width(k));
    });
    op_off->assign(1, 0ull);
    for (uint64_t s = 0; s < 2 * n; ++s) op_off->push_back(op_off->back() + words[s]);
    stats->words = ops->size();
    return 0;
}
#endif

}  // namespace sfgpu
