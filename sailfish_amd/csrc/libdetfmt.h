// libdetfmt.h -- what library format a hit record shows, how a read and a batch are tallied by it, and how a library's format is
// decided from the tally, stated once.  Plain C++, host and device: libdet.hip runs the functions below inside its kernels,
// tests/libdet_harness.cpp runs them alone (ld_serial), and hits.library_kinds_host / hits.decide_library_format are the Python
// statement both are judged by.  The observed format of a record is the reference's hitType, and what an expected format accepts is
// its compatibleHit (src/SailfishUtils.cpp:157-289), as csrc/filter.hip's compat_pair / compat_single apply them.
//
// KIND     of a record, 13 of them (kLdNames):
//          0 .. 5   ISF ISR OSF OSR MSF MSR   mate_status 3.  s1 = pos (forward) or pos + read_len (reverse), s2 likewise of the
//                   mate: the sum in uint32, then read as int32, as compat_pair has them.  Mates on different strands: the forward
//                   one is mate 1 -> *SF with I iff s1 <= s2 + stretch, else O; the forward one is mate 2 -> *SR with I iff
//                   s2 <= s1 + stretch.  stretch is the other mate's length iff dovetailing is allowed, else 0.  Both forward: MSF;
//                   both reverse: MSR.  (The comparison is taken in 64 bits: it is compat_pair's wherever that one's int32 sum does
//                   not overflow.)
//          6 .. 9   LF LR RF RR               orphans: status 1 (left) or 2 (right), forward or reverse
//          10, 11   SF SR                     status 0
//          12       other                     any other status byte: never votes, compatible with nothing
// MASK     ld_compat_mask(expected): the kinds that compat_pair (0 .. 5) and compat_single (6 .. 11) accept for `expected`.
// READ     with records [off[r], off[r + 1]): none -> `reads` only; more than max_read_occs -> `reads_over_occs` and nothing else
//          (the filter drops such a read too); else reads_mapped, mask = the OR of 1 << kind over its records, records_kind[k] for
//          every record, reads_kind[k] for a one-bit mask and reads_mixed for any other, reads_compatible iff an expected format is
//          given and mask & ld_compat_mask(expected) != 0.
// VOTE     a mapped read votes iff its mask has one bit and that bit is a voting kind: 0 .. 5 in a paired library, 10 and 11 in a
//          single-end one (orphans never vote).  Only the first *remaining_votes voters count, in read order and across calls -- as
//          the fragment-length sample takes "the first N qualifying reads" -- so the tally does not depend on the batches' cut.
// DECIDE   ld_decide(votes_kind, paired, permille, min_votes), integers only.  Paired: T = ISF + ISR, A = OSF + OSR, M = MSF + MSR;
//          T + A + M < min_votes (or no vote at all): undetermined.  The orientation is the largest of T, A, M, ties in that order;
//          s = its *SF counter, n = its sum: sense (SA, or S for M) iff 1000 s >= permille n, antisense (AS / A) iff
//          1000 (n - s) >= permille n, else unstranded.  Single end: the same with s = SF, n = SF + SR.  permille: 501 .. 1000.
//          -> the format as formatID (type | orientation << 1 | strandedness << 3), or -1.
#pragma once
#include <cstdint>

#include "../../include/sfgpu.h"

#if defined(__HIPCC__)
#define LD_HD __host__ __device__ __forceinline__
#else
#define LD_HD inline
#endif

namespace sfgpu {

enum : uint32_t { kLdISF = 0, kLdISR, kLdOSF, kLdOSR, kLdMSF, kLdMSR, kLdLF, kLdLR, kLdRF, kLdRR, kLdSF, kLdSR, kLdOther, kLdKinds };
static_assert(kLdKinds == SFGPU_LIBDET_KINDS, "the kinds of include/sfgpu.h");
constexpr uint32_t kLdNoVote = 0xFF;
constexpr uint32_t kLdPermilleMin = 501, kLdPermilleMax = 1000;
// sfgpu_libfmt's values (include/sfgpu.h)
enum : uint8_t { kLdSame = 0, kLdAway = 1, kLdToward = 2, kLdNone = 3 };
enum : uint8_t { kLdSA = 0, kLdAS = 1, kLdS = 2, kLdA = 3, kLdU = 4 };

LD_HD uint32_t ld_kind(const sfgpu_hit& h, bool dovetail) {
    const bool f1 = h.fwd != 0, f2 = h.mate_fwd != 0;
    switch (h.mate_status) {
        case 0: return f1 ? kLdSF : kLdSR;
        case 1: return f1 ? kLdLF : kLdLR;
        case 2: return f1 ? kLdRF : kLdRR;
        case 3: break;
        default: return kLdOther;
    }
    if (f1 == f2) return f1 ? kLdMSF : kLdMSR;
    const int64_t s1 = (int32_t)(f1 ? (uint32_t)h.pos : (uint32_t)h.pos + (uint32_t)h.read_len);
    const int64_t s2 = (int32_t)(f2 ? (uint32_t)h.mate_pos : (uint32_t)h.mate_pos + (uint32_t)h.mate_len);
    if (f1) return s1 <= s2 + (dovetail ? (int64_t)h.mate_len : 0) ? kLdISF : kLdOSF;
    return s2 <= s1 + (dovetail ? (int64_t)h.read_len : 0) ? kLdISR : kLdOSR;
}

// does `e` accept a record of this kind?
LD_HD bool ld_kind_compatible(sfgpu_libfmt e, uint32_t kind) {
    const uint8_t es = e.strandedness;
    if (kind <= kLdMSR) {                                     // a pair: the observed orientation and strandedness must be e's
        const uint8_t oo = kind <= kLdISR ? kLdToward : kind <= kLdOSR ? kLdAway : kLdSame;
        const uint8_t os = kind == kLdMSF ? kLdS : kind == kLdMSR ? kLdA : (kind & 1u) ? kLdAS : kLdSA;
        return e.orientation == oo && (es == kLdU || es == os);
    }
    if (kind >= kLdOther) return false;
    const bool fwd = ((kind - kLdLF) & 1u) == 0;
    const bool sense = es == kLdU || es == kLdS, anti = es == kLdU || es == kLdA;
    if (kind >= kLdSF) return fwd ? sense : anti;
    if (e.orientation == kLdSame) return es == kLdU || (es == kLdS && fwd) || (es == kLdA && !fwd);
    const bool left = kind <= kLdLR;                          // a right orphan stands where its left mate's opposite would
    return (fwd == left) ? sense : anti;
}

LD_HD uint32_t ld_compat_mask(sfgpu_libfmt e) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < kLdKinds; ++k) m |= (uint32_t)ld_kind_compatible(e, k) << k;
    return m;
}

LD_HD uint32_t ld_voting_mask(bool paired) { return paired ? 0x3Fu : (1u << kLdSF | 1u << kLdSR); }

// a mapped read's vote from its mask: the kind, or kLdNoVote
LD_HD uint32_t ld_vote(uint32_t mask, bool paired) {
    if (mask == 0 || (mask & (mask - 1)) != 0 || !(mask & ld_voting_mask(paired))) return kLdNoVote;
    uint32_t k = 0;
    while (!((mask >> k) & 1u)) ++k;
    return k;
}

LD_HD int32_t ld_format_id(uint8_t type, uint8_t orientation, uint8_t strandedness) {
    return (int32_t)((type & 1u) | (orientation & 3u) << 1 | (strandedness & 7u) << 3);
}

LD_HD int32_t ld_decide(const uint64_t* v, bool paired, uint32_t permille, uint64_t min_votes) {
    uint64_t s, n; uint8_t orientation = kLdNone; bool same = false;
    if (paired) {
        const uint64_t T = v[kLdISF] + v[kLdISR], A = v[kLdOSF] + v[kLdOSR], M = v[kLdMSF] + v[kLdMSR];
        if (T + A + M < min_votes || T + A + M == 0) return -1;
        if (T >= A && T >= M) { orientation = kLdToward; s = v[kLdISF]; n = T; }
        else if (A >= M) { orientation = kLdAway; s = v[kLdOSF]; n = A; }
        else { orientation = kLdSame; s = v[kLdMSF]; n = M; same = true; }
    } else {
        s = v[kLdSF]; n = v[kLdSF] + v[kLdSR];
        if (n < min_votes || n == 0) return -1;
        same = true;                                          // one mate: S / A, as for matching pairs
    }
    uint8_t strand = kLdU;
    if (1000 * s >= (uint64_t)permille * n) strand = same ? kLdS : kLdSA;
    else if (1000 * (n - s) >= (uint64_t)permille * n) strand = same ? kLdA : kLdAS;
    return ld_format_id(paired ? 1 : 0, orientation, strand);
}

#if !defined(__HIPCC__)
// The whole pass, serially (host only): adds to *st, takes the votes off *remaining_votes.
inline void ld_serial(const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t n_reads, const sfgpu_libdet_opts* o, int64_t* remaining_votes,
                      sfgpu_libdet_stats* st) {
    const bool paired = o->paired_library != 0, dovetail = o->can_dovetail != 0;
    const uint32_t compat = o->has_expected ? ld_compat_mask(o->expected) : 0u;
    st->reads += n_reads;
    for (uint32_t r = 0; r < n_reads; ++r) {
        const uint32_t b = hit_off[r], n = hit_off[r + 1] - b;
        if (!n) continue;
        if (n > o->max_read_occs) { st->reads_over_occs++; continue; }
        st->reads_mapped++;
        uint32_t mask = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t k = ld_kind(hits[b + i], dovetail);
            mask |= 1u << k;
            st->records_kind[k]++;
        }
        if (mask & (mask - 1)) st->reads_mixed++;
        else { uint32_t k = 0; while (!((mask >> k) & 1u)) ++k; st->reads_kind[k]++; }
        if (mask & compat) st->reads_compatible++;
        const uint32_t vote = ld_vote(mask, paired);
        if (vote != kLdNoVote && *remaining_votes > 0) { st->votes_kind[vote]++; st->votes++; --*remaining_votes; }
    }
}
#endif

}  // namespace sfgpu
