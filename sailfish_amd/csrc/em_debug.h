// em_debug.h -- developer dumps of the EM loops, included by em.hip behind the handle and the persistent loop's launch code.
// Each body is compiled under its macro only (tools/em_variants.sh name:"-DSFGPU_P_STAMP=1" ...) and the function is empty
// without it, so the driver calls them unconditionally, from one line each.  They print to stderr and change nothing a run computes.
#pragma once

// SFGPU_X_STAMP: the sweep kernels stamp their phases into em->dbg ([tile][16], 100 MHz clock)
static int em_dbg_stamps_begin(sfgpu_em* em) {
#ifdef SFGPU_X_STAMP
    if (!em->dbg) { SF_HIP(pool_malloc(&em->dbg, (size_t)em->n_tiles * 16 * 8)); }
    SF_HIP(hipMemsetAsync(em->dbg, 0, (size_t)em->n_tiles * 16 * 8, em->cur));
#endif
    return SFGPU_OK;
}
static void em_dbg_stamps_report(sfgpu_em* em) {
#ifdef SFGPU_X_STAMP
    if (em->dbg) {                                          // dev: phase stamps of the last launch that ran (100 MHz clock)
        std::vector<unsigned long long> h((size_t)em->n_tiles * 16);
        (void)hipMemcpy(h.data(), em->dbg, h.size() * 8, hipMemcpyDeviceToHost);
        unsigned long long t0min = ~0ull, tend = 0; double sum[16] = {0}; double ramp = 0; uint32_t n = 0;
        for (uint32_t b = 0; b < em->n_tiles; ++b) if (h[b * 16] && h[b * 16 + 10]) { t0min = std::min(t0min, h[b * 16]); tend = std::max(tend, h[b * 16 + 10]); }
        for (uint32_t b = 0; b < em->n_tiles; ++b) if (h[b * 16] && h[b * 16 + 10]) {
            ++n; ramp += (double)(h[b * 16] - t0min);
            for (int k = 1; k <= 10; ++k) sum[k] += h[b * 16 + k] ? (double)(h[b * 16 + k] - h[b * 16]) : 0.0;
        }
        fprintf(stderr, "stamps (%s, %u tiles; us after the tile's entry): entry %.2f after the first |", em->fused() ? "fused" : "unfused", n, ramp / n * 0.01);
        for (int k = 1; k <= 10; ++k) fprintf(stderr, " s%d %.2f", k, sum[k] / n * 0.01);
        fprintf(stderr, " | first entry -> last end %.2f us\n", (double)(tend - t0min) * 0.01);
        // the slowest tiles: duration of each phase for the five tiles with the latest end
        std::vector<uint32_t> order;
        for (uint32_t b = 0; b < em->n_tiles; ++b) if (h[b * 16] && h[b * 16 + 10]) order.push_back(b);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return h[x * 16 + 10] - h[x * 16] > h[y * 16 + 10] - h[y * 16]; });
        std::vector<TileDesc> htd(em->n_tiles);
        (void)hipMemcpy(htd.data(), em->td, htd.size() * sizeof(TileDesc), hipMemcpyDeviceToHost);
        for (size_t q = 0; q < order.size() && q < 5; ++q) {
            const uint32_t b = order[q];
            fprintf(stderr, "  slow tile %u (nc %u span %u n8 %u n_esc %u np %u nm %u nb %u; entry +%.2f):", b, htd[b].nc, htd[b].span, htd[b].n8, htd[b].n_esc, htd[b].np, htd[b].nm,
                    htd[b].nb_n, (double)(h[b * 16] - t0min) * 0.01);
            for (int k = 1; k <= 10; ++k) fprintf(stderr, " %.2f", h[b * 16 + k] ? (double)(h[b * 16 + k] - h[b * 16]) * 0.01 : 0.0);
            fprintf(stderr, "\n");
        }
        if (order.size() > 5) { const uint32_t b = order[order.size() / 2]; fprintf(stderr, "  median tile %u: total %.2f\n", b, (double)(h[b * 16 + 10] - h[b * 16]) * 0.01); }
    }
#endif
}

// SFGPU_P_PROGRESS: what every tile of a persistent launch that gave up had reached, and what it was waiting for
static void em_dbg_persist_progress(sfgpu_em* em) {
#ifdef SFGPU_P_PROGRESS
    std::vector<unsigned long long> h(em->n_tiles);
    (void)hipMemcpy(h.data(), em->dbg, h.size() * 8, hipMemcpyDeviceToHost);
    std::string line;
    for (uint32_t b = 0; b < em->n_tiles; ++b) { line += (char)('0' + (h[b] > 9 ? 9 : (int)h[b])); }
    fprintf(stderr, "persist progress (step + 1 per tile, 0 = never ran): %s\n", line.c_str());
    std::vector<unsigned long long> w(em->n_tiles);
    (void)hipMemcpy(w.data(), em->dbg + em->n_tiles, w.size() * 8, hipMemcpyDeviceToHost);
    fprintf(stderr, "persist waits at the give-up (tile: why * 1000 + step; tiles at steps < 2 only):");
    for (uint32_t b = 0; b < em->n_tiles; ++b) if (h[b] < 3) fprintf(stderr, " %u:%llu", b, w[b]);
    fprintf(stderr, "\n");
    {   // when and where every block started (100 MHz clock): the late ones, and a histogram of the waits' reasons
        std::vector<unsigned long long> t0(em->n_tiles), hw(em->n_tiles);
        (void)hipMemcpy(t0.data(), em->dbg + 2 * em->n_tiles, t0.size() * 8, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hw.data(), em->dbg + 3 * em->n_tiles, hw.size() * 8, hipMemcpyDeviceToHost);
        unsigned long long tmin = ~0ull; uint32_t never = 0;
        for (uint32_t b = 0; b < em->n_tiles; ++b) { if (!t0[b]) ++never; else tmin = std::min(tmin, t0[b]); }
        std::vector<uint32_t> ord(em->n_tiles);
        for (uint32_t b = 0; b < em->n_tiles; ++b) ord[b] = b;
        std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return t0[x] > t0[y]; });
        fprintf(stderr, "persist starts: %u blocks never started; the latest (tile: us after the first, xcc, hw_id):", never);
        for (uint32_t i = 0; i < 12 && i < em->n_tiles; ++i) { const uint32_t b = ord[i]; fprintf(stderr, " %u:%.1f,x%llu,%05llx", b, t0[b] ? (double)(t0[b] - tmin) * 0.01 : -1.0, hw[b] >> 32, hw[b] & 0xFFFFFull); }
        fprintf(stderr, "\n  why histogram (why * 1000 + step -> tiles):");
        std::map<unsigned long long, uint32_t> hist;
        for (uint32_t b = 0; b < em->n_tiles; ++b) ++hist[w[b]];
        for (auto& kv : hist) fprintf(stderr, " %llu->%u", kv.first, kv.second);
        fprintf(stderr, "\n  steps histogram (step + 1 -> tiles):");
        std::map<unsigned long long, uint32_t> hs;
        for (uint32_t b = 0; b < em->n_tiles; ++b) ++hs[h[b]];
        for (auto& kv : hs) fprintf(stderr, " %llu->%u", kv.first, kv.second);
        // the arrival counters as memory holds them now
        unsigned long long ctlw[4 * kShards];
        for (uint32_t k = 0; k < 4 * kShards; ++k) (void)hipMemcpy(&ctlw[k], em->xbuf + (size_t)(kCtlArrive + k) * kCtlStride * 8, 8, hipMemcpyDeviceToHost);
        fprintf(stderr, "\n  arrival counters [slot][shard] (low word):");
        for (uint32_t k = 0; k < 4 * kShards; ++k) fprintf(stderr, "%s%llu", (k % kShards) ? " " : " | ", ctlw[k] & 0xFFFFFFFFull);
        fprintf(stderr, "\n");
    }
    // the first stuck tile's view: what memory holds NOW where it polled (its neighbours' pieces, parity 1 = tags 1, 3, ...)
    for (uint32_t b = 0; b < em->n_tiles; ++b) if (h[b] == 2 && w[b] / 1000 == 2) {
        TileDesc t; (void)hipMemcpy(&t, em->td + b, sizeof(t), hipMemcpyDeviceToHost);
        auto up2 = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o1 = up2((size_t)kCtlWords * 8 + 64 + sizeof(PersistCold)) + up2((size_t)(em->P ? em->P : 1) * 16);
        fprintf(stderr, "tile %u (lo %u span %u nb %u): tags in memory of its neighbours' first / last overlapping slots (parity 1):", b, t.lo, t.span, t.nb_n);
        for (uint32_t j2 = 0; j2 < t.nb_n && j2 < 6; ++j2) {
            const uint32_t lo2 = t.e[j2].x, sp2 = t.e[j2].y, off2 = t.e[j2].z;
            const uint32_t p0 = std::max(lo2, t.lo), p1 = std::min(lo2 + sp2, t.lo + t.span) - 1;
            uint32_t g0[4], g1[4];
            (void)hipMemcpy(g0, em->xbuf + o1 + (size_t)(off2 + (p0 - lo2)) * 16, 16, hipMemcpyDeviceToHost);
            (void)hipMemcpy(g1, em->xbuf + o1 + (size_t)(off2 + (p1 - lo2)) * 16, 16, hipMemcpyDeviceToHost);
            fprintf(stderr, " [tile %u: %u/%u .. %u/%u]", t.e[j2].w, g0[1], g0[3], g1[1], g1[3]);
        }
        fprintf(stderr, "\n");
        break;
    }
#endif
}

// SFGPU_P_STAMP: where the steps of a persistent launch went
static void em_dbg_persist_stamps(sfgpu_em* em, uint32_t iters) {
#ifdef SFGPU_P_STAMP
    if (em->form == EmForm::persistent && em->dbg && iters > 2) {          // dev: where a persistent step goes, per tile (100 MHz clock)
        std::vector<unsigned long long> h((size_t)em->n_tiles * 8);
        (void)hipMemcpy(h.data(), em->dbg, h.size() * 8, hipMemcpyDeviceToHost);
        static const char* nm[7] = {"operands", "x+update", "barrier", "A", "B", "C", "D"};
        const double steps = (double)iters + 1.0;
        fprintf(stderr, "persist stamps (%s, %u tiles, %u steps; us per step and tile, mean / min / max over the tiles):", em->opts.use_vbem ? "VBEM" : "EM", em->n_tiles, iters + 1);
        for (int k = 0; k < 7; ++k) {
            double sum = 0, mn = 1e30, mx = 0;
            for (uint32_t b = 0; b < em->n_tiles; ++b) { const double v = (double)h[b * 8 + k] * 0.01 / steps; sum += v; mn = std::min(mn, v); mx = std::max(mx, v); }
            fprintf(stderr, " %s %.2f/%.2f/%.2f", nm[k], sum / em->n_tiles, mn, mx);
        }
        fprintf(stderr, "\n");
        // the tiles that wait least for their operands set the pace: what are they made of?
        std::vector<TileDesc> htd(em->n_tiles);
        (void)hipMemcpy(htd.data(), em->td, htd.size() * sizeof(TileDesc), hipMemcpyDeviceToHost);
        std::vector<uint32_t> order(em->n_tiles);
        for (uint32_t b = 0; b < em->n_tiles; ++b) order[b] = b;
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return h[x * 8] < h[y * 8]; });
        std::vector<TilePack> htp(em->n_tiles);
        (void)hipMemcpy(htp.data(), em->tp, htp.size() * sizeof(TilePack), hipMemcpyDeviceToHost);
        double mean_nc = 0, mean_np = 0, mean_nm = 0, mean_ov = 0, mean_n[4] = {0, 0, 0, 0};
        for (const TileDesc& t : htd) { mean_nc += t.nc; mean_np += t.np; mean_nm += t.nm; }
        for (const TilePack& t : htp) { mean_ov += t.n_ov; mean_n[0] += t.n1; mean_n[1] += t.n2; mean_n[2] += t.n3; mean_n[3] += t.n4; }
        fprintf(stderr, "  tile means: classes %.0f (records of 4 / 8 / 16 bytes / long: %.0f %.0f %.0f %.0f), pure chunks %.0f, mixed chunks %.0f, overflow chunks %.0f\n", mean_nc / em->n_tiles,
                mean_n[0] / em->n_tiles, mean_n[1] / em->n_tiles, mean_n[2] / em->n_tiles, mean_n[3] / em->n_tiles, mean_np / em->n_tiles, mean_nm / em->n_tiles, mean_ov / em->n_tiles);
        for (uint32_t i = 0; i < 6 && i < em->n_tiles; ++i) {
            const uint32_t b = order[i]; const TileDesc& t = htd[b];
            fprintf(stderr, "  tile %4u:", b);
            for (int k = 0; k < 7; ++k) fprintf(stderr, " %s %.2f", nm[k], (double)h[b * 8 + k] * 0.01 / steps);
            fprintf(stderr, " | span %u classes %u pure %u mixed %u overflow %u far members %u far slots %u neighbours %u\n", t.span, t.nc, t.np, t.nm, htp[b].n_ov, t.n_esc, t.nf, t.nb_n);
        }
    }
#endif
}
