// test harness: compiles the product's sampler header (sailfish_amd/csrc/rng.h) as plain C++ so the
// CPU suite can check the samplers' distributions without a GPU
#include "../sailfish_amd/csrc/rng.h"
extern "C" {
void draw_binomial(uint64_t seed, uint32_t n, double p, uint32_t count, uint32_t* out) {
    for (uint32_t i = 0; i < count; ++i) {
        sfgpu::Philox g; g.init(seed, i, 0);
        out[i] = sfgpu::binomial(g, n, p);
    }
}
void draw_binomial_by_inversion(uint64_t seed, uint32_t n, double p, uint32_t count, uint32_t* out) {
    for (uint32_t i = 0; i < count; ++i) {
        sfgpu::Philox g; g.init(seed, i, 0);
        out[i] = sfgpu::binomial_by_inversion(g, n, p);
    }
}
void draw_uniform(uint64_t seed, uint64_t stream, uint32_t count, double* out) {
    sfgpu::Philox g; g.init(seed, stream, 0);
    for (uint32_t i = 0; i < count; ++i) out[i] = g.uniform();
}
void philox_block(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t* out) {
    sfgpu::Philox g; g.key[0] = k0; g.key[1] = k1; g.ctr[0] = c0; g.ctr[1] = c1; g.ctr[2] = c2; g.ctr[3] = c3; g.have = 0;
    g.block();
    for (int i = 0; i < 4; ++i) out[i] = g.out[i];
}
}

// the multinomial tree of csrc/sampling.hip (k_mn_level), node for node and stream for stream, on the host:
// prefix[0..C] = exclusive prefix sums of the class counts, out[0..C) = one resample of n_total reads
extern "C" void tree_multinomial(uint64_t seed, uint64_t draw, uint64_t C, const uint64_t* prefix, uint32_t n_total, uint32_t* out) {
    uint64_t W = 1; while (W < C) W <<= 1;
    int depth = 0; while (((uint64_t)1 << depth) < W) ++depth;
    uint32_t* cur = new uint32_t[W + 1]; uint32_t* nxt = new uint32_t[W + 1];
    cur[0] = n_total;
    for (int level = 0; level < depth; ++level) {
        const uint64_t width = W >> level;
        for (uint64_t i = 0; i < ((uint64_t)1 << level); ++i) {
            const uint32_t n = cur[i];
            const uint64_t lo = i * width, mid = lo + width / 2, hi = lo + width;
            const uint64_t pl = prefix[lo < C ? lo : C], pm = prefix[mid < C ? mid : C], ph = prefix[hi < C ? hi : C];
            const uint64_t s_left = pm - pl, s_all = ph - pl;
            uint32_t n_left;
            if (n == 0 || s_left == 0) n_left = 0;
            else if (s_left == s_all) n_left = n;
            else { sfgpu::Philox g; g.init(seed, ((uint64_t)1 << level) + i, draw); n_left = sfgpu::binomial(g, n, (double)s_left / (double)s_all); }
            nxt[2 * i] = n_left; nxt[2 * i + 1] = n - n_left;
        }
        uint32_t* t = cur; cur = nxt; nxt = t;
    }
    for (uint64_t c = 0; c < C; ++c) out[c] = cur[c];
    delete[] cur; delete[] nxt;
}
extern "C" void draw_uniform_sub(uint64_t seed, uint64_t stream, uint64_t substream, uint32_t count, double* out) {
    sfgpu::Philox g; g.init(seed, stream, substream);
    for (uint32_t i = 0; i < count; ++i) out[i] = g.uniform();
}
extern "C" void draw_words(uint64_t seed, uint64_t stream, uint64_t substream, uint32_t count, uint32_t* out) {
    sfgpu::Philox g; g.init(seed, stream, substream);
    for (uint32_t i = 0; i < count; ++i) out[i] = g.next32();
}

// ---- the Gibbs sampler's chain and class visits (sailfish_amd/csrc/gibbsfmt.h, the header the kernels of gibbs.hip call)
#include "../sailfish_amd/csrc/gibbsfmt.h"
#include <vector>

// sfgpu_chain_eval on the host: draw d of multinomial_chain<light> over the k weights from Philox(seed, d, 0), out[count][k]
extern "C" void draw_chain(int light, const double* w, uint32_t k, uint32_t n, uint32_t last, uint64_t seed, uint64_t count, uint32_t* out) {
    for (uint64_t d = 0; d < count; ++d) {
        double total = 0.0;
        for (uint32_t i = 0; i < k; ++i) total += w[i];
        sfgpu::Philox g; g.init(seed, d, 0);
        auto prob = [&](uint32_t i) { return w[i]; };
        auto put = [&](uint32_t i, uint32_t r) { out[d * k + i] = r; };
        if (light) sfgpu::multinomial_chain<true>(g, n, k, total, last, prob, put);
        else sfgpu::multinomial_chain<false>(g, n, k, total, last, prob, put);
    }
}

// sfgpu_gibbs_sample restated serially: the weights of k_gibbs_weights, then per sweep (the init sweep, then one per round) the
// device's order on classes that may share a transcript -- phase p = 0 .. K - 1: the light classes (kind 0) of the tiles = p (mod K),
// then their heavy ones (kind 2); then the wide classes (kind 1) in class order.  Chains do not see each other, so each is run on
// its own.  Only the plan with at most kWideSerial wide classes is restated (the coloured and thin-component orders are not):
// returns -1 beyond.  out[n_samples][M]: sample s = chain s % n_chains after s / n_chains + 1 rounds.
extern "C" int gibbs_serial(uint64_t M, uint64_t C, const uint32_t* rowptr, const uint32_t* ids, const uint64_t* counts, const double* len,
                            const double* mass, uint64_t num_mapped, uint32_t n_chains, uint64_t seed, uint32_t n_samples,
                            const uint8_t* kind, uint32_t K, int32_t* out) {
    using namespace sfgpu;
    std::vector<double> inv_len(M), w_mass(M);
    for (uint64_t t = 0; t < M; ++t) {
        double l = len[t]; if (l <= 1.0) l = 1.0;
        const double il = 1.0 / l;
        inv_len[t] = il;
        const double m = kGibbsPrior + mass[t] * (double)num_mapped;
        w_mass[t] = (kGibbsPrior + m) * il;
    }
    std::vector<uint32_t> wide_list;
    for (uint64_t c = 0; c < C; ++c) if (kind[c] == 1) wide_list.push_back((uint32_t)c);
    if (wide_list.size() > kWideSerial || K == 0) return -1;
    const uint64_t L = C ? rowptr[C] : 0;
    const uint64_t n_tiles = (C + kGibbsTile - 1) / kGibbsTile;
    // the kernels' chain-minor state; chains do not see each other, so each runs through all its sweeps on its own
    std::vector<uint32_t> count_map(L * n_chains + 1, 0u);
    std::vector<int32_t> txp((size_t)M * n_chains, 0);
    for (uint32_t ch = 0; ch < n_chains && ch < n_samples; ++ch) {
        GibbsArgs a{n_chains, C, rowptr, ids, counts, inv_len.data(), w_mass.data(), count_map.data(), txp.data(), kind,
                    wide_list.data(), (uint32_t)wide_list.size(), seed, 0u};
        auto sweep = [&](bool init) {
            for (uint64_t p = 0; p < K && p < n_tiles; ++p)
                for (int heavy = 0; heavy < 2; ++heavy)
                    for (uint64_t tile = p; tile < n_tiles; tile += K) {
                        const uint64_t c0 = tile * kGibbsTile, c1 = c0 + kGibbsTile < C ? c0 + kGibbsTile : C;
                        for (uint64_t c = c0; c < c1; ++c) {
                            if (kind[c] != (heavy ? 2 : 0)) continue;
                            if (heavy) { if (init) gibbs_init_class<false>(a, c, ch); else gibbs_round_class<false>(a, c, ch); }
                            else { if (init) gibbs_init_class<true>(a, c, ch); else gibbs_round_class<true>(a, c, ch); }
                        }
                    }
            for (uint32_t c : wide_list) { if (init) gibbs_init_class<false>(a, c, ch); else gibbs_round_class<false>(a, c, ch); }
        };
        sweep(true);
        for (uint64_t s = ch; s < n_samples; s += n_chains) {
            sweep(false);
            for (uint64_t t = 0; t < M; ++t) out[s * M + t] = txp[t * n_chains + ch];
            ++a.round;
        }
    }
    return 0;
}
