// postfmt.h -- the posterior probability of every record of a read under a weight per transcript, and the ZW:f: value a mappings
// file holds for it, stated once.  Plain C++, host and device: posterior.hip runs the functions below inside its kernels,
// tests/posterior_harness.cpp runs them alone (post_serial), and hits.posteriors_host is the Python statement both are judged by.
//
// WEIGHT   x_h = w[tid_h]; a weight below 2^-960 reads as 0, so that no subnormal enters a sum.  Every record is a candidate of its
//          own: a transcript that holds two records of a read has two terms.  A weight that is negative, NaN, infinite or above
//          2^960 is an error of the call (post_weight_bad); 64 000 such weights still sum below DBL_MAX.
// SUM      S = post_sum(x) over the read's n records, in a FIXED ORDER, so that every implementation gives the same bits:
//          64 accumulators a_j = x_j + x_{j+64} + x_{j+128} + ..., serially and ascending, a_j = 0 where there is no x_j; then for
//          k = 32, 16, 8, 4, 2, 1: a_j <- a_j + a_{j xor k} for every j at once; S = a_0.  IEEE addition commutes, so after step k
//          a_j = a_{j xor k} and a_0 is the sum of the plain halving tree (a_j += a_{j+k} for j < k), which is what post_sum runs.
//          Adding +0 is exact: for n <= P <= 64, P a power of two, the steps k >= P add zeros, and the tree over P leaves -- a group
//          of P lanes with k = P/2 .. 1, or one lane over P values -- gives the identical S.
// VALUE    p_h = x_h / S where S > 0, else 1 / n (a read whose weights are all 0 is spread evenly).  A p_h below 2^-56 is written
//          as 0: everything then lies on gfmt_decode_fast's 128-bit window and on gfmt_value_fast's exact powers of ten.
//          rec_h = gfmt_decode_fast(p_h), the six-digit record whose token is "%g" of p_h; f32_h = (float)gfmt_value(rec_h), the
//          float a BAM reader gets from that token.
// STATS    reads, reads_mapped (n >= 1), reads_multi (n >= 2), records, reads_flat (n >= 1 and S = 0), records_zero (p written
//          as 0), max_records: integers, independent of any order.
#pragma once
#include <cstdint>

#include "../../include/sfgpu.h"
#include "gfmt.h"

#if defined(__HIPCC__)
#define POST_HD __host__ __device__ __forceinline__
#else
#define POST_HD inline
#include <vector>
#endif

namespace sfgpu {

constexpr int kPostAcc = 64;                                          // the accumulators of post_sum
constexpr uint64_t kPostTinyBits = (uint64_t)(1023 - 960) << 52;      // 2^-960
constexpr uint64_t kPostHugeBits = (uint64_t)(1023 + 960) << 52;      // 2^960
constexpr uint64_t kPostFlushBits = (uint64_t)(1023 - 56) << 52;      // 2^-56

POST_HD bool post_weight_bad(double w) { return !(w >= 0.0) || w > gfmt_from_bits(kPostHugeBits); }
// a checked weight as it enters the sum
POST_HD double post_weight(double w) { return w < gfmt_from_bits(kPostTinyBits) ? 0.0 : w; }

// the halving tree over P = 2^m <= 64 values in a[0 .. P): -> a[0]
template <int P>
POST_HD double post_tree(double* a) {
    for (int k = P / 2; k > 0; k >>= 1)
        for (int j = 0; j < k; ++j) a[j] = a[j] + a[j + k];
    return a[0];
}
// S of x(0) .. x(n - 1)
template <typename X>
POST_HD double post_sum(uint64_t n, X x) {
    double a[kPostAcc];
    for (int j = 0; j < kPostAcc; ++j) a[j] = 0.0;
    for (uint64_t i = 0; i < n; ++i) a[i & (kPostAcc - 1)] = a[i & (kPostAcc - 1)] + x(i);
    return post_tree<kPostAcc>(a);
}
// the same for n <= 4 in registers: the tree over 4 leaves
POST_HD double post_sum4(double x0, double x1, double x2, double x3) { return (x0 + x2) + (x1 + x3); }

// what is written for one record
struct PostValue { double p; uint32_t rec; float f32; };
POST_HD PostValue post_value(double x, double S, uint64_t n) {
    PostValue v;
    v.p = S > 0.0 ? x / S : 1.0 / (double)n;
    if (v.p < gfmt_from_bits(kPostFlushBits)) v.p = 0.0;
    v.rec = gfmt_decode_fast(v.p);
    bool pending;
    v.f32 = (float)gfmt_value_fast(v.rec, &pending);                  // (never pending: the token's exponent is -22 .. 0)
    return v;
}

#if !defined(__HIPCC__)
// The whole pass, serially (host only).  -> 0; 1 + the lowest transcript with a bad weight; or -(1 + the lowest record whose tid
// is no transcript), the weights being checked first.  On an error nothing is written.
inline int64_t post_serial(const sfgpu_hit* hits, const uint32_t* hit_off, uint32_t n_reads, const double* w, uint64_t n_refs, double* p, uint32_t* rec,
                           float* f32, sfgpu_posterior_stats* st) {
    for (uint64_t t = 0; t < n_refs; ++t) if (post_weight_bad(w[t])) return (int64_t)(1 + t);
    const uint64_t n_rec = n_reads ? hit_off[n_reads] : 0;
    for (uint64_t h = 0; h < n_rec; ++h) if (hits[h].tid >= n_refs) return -(int64_t)(1 + h);
    *st = sfgpu_posterior_stats{};
    st->reads = n_reads; st->records = n_rec;
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint64_t b = hit_off[r], n = hit_off[r + 1] - b;
        if (!n) continue;
        st->reads_mapped++;
        if (n >= 2) st->reads_multi++;
        if (n > st->max_records) st->max_records = n;
        auto x = [&](uint64_t i) { return post_weight(w[hits[b + i].tid]); };
        const double S = post_sum(n, x);
        if (!(S > 0.0)) st->reads_flat++;
        for (uint64_t i = 0; i < n; ++i) {
            const PostValue v = post_value(x(i), S, n);
            p[b + i] = v.p; rec[b + i] = v.rec; f32[b + i] = v.f32;
            if (v.p == 0.0) st->records_zero++;
        }
    }
    return 0;
}
#endif

}  // namespace sfgpu
