// covgfmt.h -- the transcripts' coverage runs (coverfmt.h) projected through the exon structure onto the chromosomes, and the bedGraph
// rows written of the result, stated once.  Plain C++, host and device: coverage_genome.hip runs the functions below inside its
// kernels, tests/covgenome_harness.cpp runs them alone (CovGenomeSerial), and hits.coverage_genome_host is the Python statement both
// are judged by.
//
// MODEL    every transcript has a status; 0 means placed.  A placed transcript has a chromosome id c, a strand (+1 / -1) and exon
//          blocks e_0 .. e_{k-1} in TRANSCRIPT order: block i is (gs_i, len_i), gs_i 0-based on the chromosome, len_i >= 1, and
//          toff_i = sum of len_j for j < i.  On + the blocks ascend along the chromosome, on - they descend; they never overlap (they
//          may touch).  L = sum of len_i.  All positions are uint32 and gs_i + len_i <= 2^32 - 1.
// PROJECT  a run [a, b) of sum s on a placed transcript gives one piece for every block with [a', b') = [a, b) n [toff_i, toff_i +
//          len_i) not empty: on + the piece [gs_i + (a' - toff_i), gs_i + (b' - toff_i)), on - the piece [gs_i + len_i - (b' - toff_i),
//          gs_i + len_i - (a' - toff_i)).  The run's bases at x >= L have no place: they are dropped and counted (bases_off_model).
//          The runs of a transcript that is not placed are dropped whole and counted (runs_unplaced, bases_unplaced).
// EVENTS   a piece [lo, hi) on chromosome c is the two events (c << 32 | lo, +s) and (c << 32 | hi, -s), modulo 2^64.  The transcript
//          handle's kCovMaxLines keeps every genomic sum below 2^64.
// SUMS     events of equal key are added; keys whose delta is 0 disappear; one inclusive scan over the keys in ascending order gives
//          the sum that holds from a key to the next.  A chromosome's deltas sum to 0, so the scan is not segmented and no run crosses
//          into the next chromosome.
// RUNS     maximal stretches of one chromosome with the same nonzero sum, by chromosome id, then start.  Because keys of delta 0 are
//          dropped, the sums of neighbouring keys differ, so the stretches between neighbouring keys ARE the maximal ones: pieces that
//          touch with equal depth merge by the rule itself, not by a later pass.
// ROW      chrom \t start \t end \t %g(depth) \n, depth = (double)sum 2^-32: coverfmt.h's cov_depth and cov_row_tail.  No header line.
// Every step is integer arithmetic: any order of the events and any reduction tree give the same bits.
#pragma once
#include <cstdint>

#include "coverfmt.h"

#if !defined(__HIPCC__)
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#endif

namespace sfgpu {

constexpr uint64_t kCovgMaxEvents = 0xffffffffull;         // the events stay below 2^32 - 1: their index is the sort's 32-bit payload
constexpr uint64_t kCovgMaxPos = 0xffffffffull;            // gs + len <= 2^32 - 1

COV_HD uint64_t covg_key(uint32_t chrom, uint64_t pos) { return (uint64_t)chrom << 32 | pos; }

// block i of a placed transcript's model is well formed next to block i + 1 (has_next): both inside the positions, not empty, and
// following each other the way the strand says without overlapping
COV_HD bool covg_block_ok(uint64_t gs, uint64_t len, bool has_next, uint64_t gs_next, uint64_t len_next, int strand) {
    if (len == 0 || gs + len > kCovgMaxPos) return false;
    if (!has_next) return true;
    return strand > 0 ? gs + len <= gs_next : gs_next + len_next <= gs;
}

// the piece of [a, b) (already clipped to [0, L)) in the block (gs, len) at transcript offset toff; the caller knows they intersect
COV_HD void covg_piece(uint64_t a, uint64_t b, uint64_t toff, uint64_t gs, uint64_t len, int strand, uint64_t* lo, uint64_t* hi) {
    const uint64_t a1 = (a > toff ? a : toff) - toff, b1 = (b < toff + len ? b : toff + len) - toff;
    if (strand > 0) { *lo = gs + a1; *hi = gs + b1; }
    else { *lo = gs + len - b1; *hi = gs + len - a1; }
}

struct CovgCount { uint64_t pieces, runs_unplaced, bases_unplaced, bases_off_model; };

#if !defined(__HIPCC__)
// The whole of it, serially (host only).  The model's arrays are the ones sfgpu_covg_open takes.
struct CovGenomeSerial {
    std::vector<uint32_t> r_chrom, r_start, r_end;         // the runs
    std::vector<uint64_t> r_sum;
    CovgCount count{0, 0, 0, 0};
    uint64_t n_events = 0, n_keys = 0, bases_covered = 0, placed = 0, length_mismatch = 0;

    // -> -1, or the lowest transcript whose model is refused
    static int64_t check(const uint8_t* status, const int32_t* chrom, const int8_t* strand, const uint64_t* exon_off, const uint32_t* exon_start,
                         const uint32_t* exon_len, uint64_t M, uint32_t n_chrom) {
        for (uint64_t t = 0; t < M; ++t) {
            if (exon_off[t] > exon_off[t + 1] || (t == 0 && exon_off[0] != 0)) return (int64_t)t;
            const bool placed = status[t] == 0;
            if (placed && (chrom[t] < 0 || (uint32_t)chrom[t] >= n_chrom || (strand[t] != 1 && strand[t] != -1))) return (int64_t)t;
            for (uint64_t e = exon_off[t]; e < exon_off[t + 1]; ++e) {
                const bool next = placed && e + 1 < exon_off[t + 1];
                if (!covg_block_ok(exon_start[e], exon_len[e], next, next ? exon_start[e + 1] : 0, next ? exon_len[e + 1] : 0, placed ? strand[t] : 1)) return (int64_t)t;
            }
        }
        return -1;
    }

    void project(const uint8_t* status, const int32_t* chrom, const int8_t* strand, const uint64_t* exon_off, const uint32_t* exon_start, const uint32_t* exon_len,
                 const uint32_t* ref_len, uint64_t M, const uint32_t* t_tid, const uint32_t* t_start, const uint32_t* t_end, const uint64_t* t_sum, uint64_t n_runs) {
        std::vector<uint64_t> L(M, 0);
        for (uint64_t t = 0; t < M; ++t) {
            for (uint64_t e = exon_off[t]; e < exon_off[t + 1]; ++e) L[t] += exon_len[e];
            if (status[t] == 0) { ++placed; length_mismatch += L[t] != ref_len[t]; }
        }
        std::vector<std::pair<uint64_t, uint64_t>> ev;
        for (uint64_t r = 0; r < n_runs; ++r) {
            const uint64_t t = t_tid[r], a = t_start[r];
            uint64_t b = t_end[r];
            if (status[t] != 0) { ++count.runs_unplaced; count.bases_unplaced += b - a; continue; }
            if (b > L[t]) { count.bases_off_model += b - (a > L[t] ? a : L[t]); b = L[t]; }
            uint64_t toff = 0;
            for (uint64_t e = exon_off[t]; e < exon_off[t + 1] && a < b; toff += exon_len[e], ++e) {
                if (toff + exon_len[e] <= a || toff >= b) continue;
                uint64_t lo, hi;
                covg_piece(a, b, toff, exon_start[e], exon_len[e], strand[t], &lo, &hi);
                ev.emplace_back(covg_key((uint32_t)chrom[t], lo), t_sum[r]);
                ev.emplace_back(covg_key((uint32_t)chrom[t], hi), 0ull - t_sum[r]);
                ++count.pieces;
            }
        }
        n_events = ev.size();
        std::sort(ev.begin(), ev.end(), [](const std::pair<uint64_t, uint64_t>& x, const std::pair<uint64_t, uint64_t>& y) { return x.first < y.first; });
        uint64_t sum = 0;
        bool open = false;
        for (size_t i = 0; i < ev.size();) {
            uint64_t d = 0;
            size_t j = i;
            for (; j < ev.size() && ev[j].first == ev[i].first; ++j) d += ev[j].second;
            const uint64_t key = ev[i].first;
            i = j;
            if (d == 0) continue;
            ++n_keys;
            if (open) { r_end.push_back((uint32_t)key); bases_covered += r_end.back() - r_start.back(); }
            sum += d;
            open = sum != 0;
            if (open) { r_chrom.push_back((uint32_t)(key >> 32)); r_start.push_back((uint32_t)key); r_sum.push_back(sum); }
        }
    }
    // the file: names[name_off[c] .. name_off[c + 1]) is chromosome c's
    std::string text(const char* names, const uint64_t* name_off) const {
        std::string out;
        for (size_t r = 0; r < r_chrom.size(); ++r) {
            out.append(names + name_off[r_chrom[r]], names + name_off[r_chrom[r] + 1]);
            bool slow;
            const uint32_t rec = gfmt_decode(cov_depth(r_sum[r]), &slow);
            const size_t at = out.size();
            out.resize(at + cov_row_tail_len(r_start[r], r_end[r], rec));
            cov_row_tail(r_start[r], r_end[r], rec, [&](int i, char ch) { out[at + (size_t)i] = ch; });
        }
        return out;
    }
};
#endif

}  // namespace sfgpu
