// gibbsfmt.h -- the Gibbs sampler's multinomial chain and its two class visits, stated once.  Plain C++, host and device: gibbs.hip
// runs them inside its kernels (one lane per chain), tests/sampling_harness.cpp runs them alone -- the chain draw for draw, and a
// serial restatement of a whole sfgpu_gibbs_sample call -- and tests/test_gpu_rng.py holds the device to that restatement.
//
// STATE    chain-minor: count_map[nonzero][chain] (the reads of class c that member i holds), txp_count[transcript][chain].
// WEIGHTS  inv_len[t] = 1 / max(effLen_t, 1);  w_mass[t] = (prior + (prior + mass_t * numMapped)) * inv_len[t]   (k_gibbs_weights).
// INIT     class c, chain ch: k = 0 nothing; k = 1 the member takes all n; else one multinomial_chain over w_mass with
//          Philox(seed, ch, c); a class whose weights sum to nothing assigns nothing.
// ROUND    class c, chain ch, round r (0-based): Philox(seed, (r + 1) << 32 | ch, c); frac = 0.25 + 0.5 u; every member gives
//          round(frac * its reads) back, then the reads given back are drawn again over (prior + txp_count_t) * inv_len[t].
// CHAIN    multinomial(n; p) as k - 1 conditional binomials in member order, member `last` (the largest weight, first of equals)
//          skipped and given what is left.  LIGHT draws the binomials by inversion alone.
// KIND     per class (k_gibbs_plan): 1 wide (its ids span more than kWideSpan), else 2 heavy (k > 1 and more than kGibbsLightMax
//          reads), else 0 light.
#pragma once
#include "rng.h"

namespace sfgpu {

constexpr int kGibbsTile = 64;             // classes per tile
constexpr uint32_t kWideSpan = 2048;       // classes spanning more transcripts than this are "wide"
constexpr uint32_t kWideSerial = 64;       // up to this many wide classes are visited one after another by one launch
#if !defined(SFGPU_GIBBS_LIGHT_MAX)
#define SFGPU_GIBBS_LIGHT_MAX 1500
#endif
constexpr uint64_t kGibbsLightMax = SFGPU_GIBBS_LIGHT_MAX;   // classes of more reads than this are HEAVY: visited by the phase kernel that carries BTPE (see k_gibbs_phase)
constexpr double kGibbsPrior = 1e-8;       // priorAlpha (:215)
constexpr double kGibbsTiny = 4.9406564584124654e-324;

struct GibbsArgs {
    uint32_t n_chains; uint64_t C;
    const uint32_t* rowptr; const uint32_t* ids; const uint64_t* counts;
    const double* inv_len; const double* w_mass;        // 1/effLen_t ; (prior + mass_t)/effLen_t
    uint32_t* count_map; int32_t* txp_count;
    const uint8_t* wide;                                 // per class: visited in the wide phase
    const uint32_t* wide_list; uint32_t n_wide;
    uint64_t seed; uint32_t round;
};

// multinomial(n; p_0..p_{k-1}) as conditional binomials; calls put(i, r_i) for every member.  Member `last` gets what the others
// leave: a BINV walk costs its mean, so the chain costs n (1 - p_last) steps in all -- least when the LARGEST member is not sampled
// at all.  `last` is the same for every chain of the wavefront (the member with the largest EM weight: the chains live around the EM
// solution), so no lane idles; any order gives the same distribution.
template <bool LIGHT, typename ProbFn, typename PutFn>
SF_HD void multinomial_chain(Philox& g, uint32_t n, uint32_t k, double p_total, uint32_t last, ProbFn prob, PutFn put) {
    double p_rem = p_total;
    uint32_t n_rem = n;
    for (uint32_t i = 0; i < k; ++i) {
        if (i == last) continue;
        const double p = prob(i);
        const double ratio = (p_rem > 0.0) ? ratio_of(p, p_rem) : 0.0;
        const double pr = ratio < 1.0 ? ratio : 1.0;
        const uint32_t r = (n_rem == 0) ? 0u : (LIGHT ? binomial_by_inversion(g, n_rem, pr) : binomial(g, n_rem, pr));
        p_rem -= p; if (p_rem < 0.0) p_rem = 0.0;
        put(i, r);
        n_rem -= r;
    }
    put(last, n_rem);
}

// initCountMap_ (:45-92) for one class and one chain
template <bool LIGHT = false>
SF_HD void gibbs_init_class(const GibbsArgs& a, uint64_t c, uint32_t ch) {
    const uint32_t b = a.rowptr[c], k = a.rowptr[c + 1] - b;
    const uint32_t n = (uint32_t)a.counts[c];            // uint32 n in MultinomialSampler (:15)
    const uint32_t nch = a.n_chains;
    if (k == 0) return;
    if (k == 1) {                                        // :81-83
        a.count_map[(uint64_t)b * nch + ch] = n;
        a.txp_count[(uint64_t)a.ids[b] * nch + ch] += (int32_t)n;
        return;
    }
    double denom = 0.0, w_top = -1.0; uint32_t last = 0;
    for (uint32_t i = 0; i < k; ++i) { const double w = a.w_mass[a.ids[b + i]]; denom += w; if (w > w_top) { w_top = w; last = i; } }      // :58-63
    if (!(denom > kGibbsTiny)) {                                                      // :65 -- nothing assigned
        for (uint32_t i = 0; i < k; ++i) a.count_map[(uint64_t)(b + i) * nch + ch] = 0;
        return;
    }
    Philox g; g.init(a.seed, ch, c);
    multinomial_chain<LIGHT>(g, n, k, denom, last,
        [&](uint32_t i) { return a.w_mass[a.ids[b + i]]; },
        [&](uint32_t i, uint32_t r) {
            a.count_map[(uint64_t)(b + i) * nch + ch] = r;                            // :76-79
            a.txp_count[(uint64_t)a.ids[b + i] * nch + ch] += (int32_t)r;             // :86-89
        });
}

// sampleRound_ (:113-184) for one class and one chain
template <bool LIGHT = false>
SF_HD void gibbs_round_class(const GibbsArgs& a, uint64_t c, uint32_t ch) {
    const uint32_t b = a.rowptr[c], k = a.rowptr[c + 1] - b;
    if (k <= 1) return;                                     // singletons keep their full count (:128)
    const uint32_t nch = a.n_chains;
    Philox g; g.init(a.seed, ((uint64_t)(a.round + 1) << 32) | ch, c);
    const double frac = 0.25 + 0.5 * g.uniform();           // U(0.25, 0.75) per class (:106, :115)
    // pass 1: take round(frac * current) reads away from every member (:138-148)
    uint32_t n_res = 0, last = 0; double denom = 0.0, w_top = -1.0;
    for (uint32_t i = 0; i < k; ++i) {
        const uint64_t at = (uint64_t)(b + i) * nch + ch;
        const uint32_t t = a.ids[b + i];
        { const double w = a.w_mass[t]; if (w > w_top) { w_top = w; last = i; } }        // (wavefront-uniform: the member the chain does not sample)
        const uint32_t cur = a.count_map[at];
        const uint32_t r = (uint32_t)(frac * (double)cur + 0.5);                       // std::round, values >= 0 (:142)
        n_res += r;
        a.count_map[at] = cur - r;
        const int32_t tc = a.txp_count[(uint64_t)t * nch + ch] - (int32_t)r;
        a.txp_count[(uint64_t)t * nch + ch] = tc;
        denom += (kGibbsPrior + (double)tc) * a.inv_len[t];                            // :147
    }
    // pass 2: re-draw them from p_i ~ (prior + txpCount_i) * aux_i (:150-170).  denom >= k*1e-8/len > 0,
    // so the reference's "did not sample" branch (:172-179) cannot trigger for finite inputs.
    multinomial_chain<LIGHT>(g, n_res, k, denom, last,
        [&](uint32_t i) { const uint32_t t = a.ids[b + i]; return (kGibbsPrior + (double)a.txp_count[(uint64_t)t * nch + ch]) * a.inv_len[t]; },
        [&](uint32_t i, uint32_t r) {
            if (r) { a.count_map[(uint64_t)(b + i) * nch + ch] += r; a.txp_count[(uint64_t)a.ids[b + i] * nch + ch] += (int32_t)r; }
        });
}

}  // namespace sfgpu
