// lgr_match_debug.cuh -- host-side diagnostics of a match call: the LGR_MATCH_DEBUG report of the pruned passes and the EXP_PROF read-out.
// Part of the brute-force FPFH matcher; included by lgr_match.hip behind the definition of MatchCall (the report reads the call's state).
// Nothing here is on the hot path: match_impl calls it only when the environment (or the EXP_PROF build) asks for it.
#pragma once

// LGR_MATCH_DEBUG >= 1, behind the statistics read-back of the pruned passes (hs: the passes' MaskStats, h_kept: the sweep's list length; both pinned host copies)
static int match_debug_report(const MatchCall& c, const MaskStats* hs, const unsigned long long* h_kept) {
    lgr_ctx* const ctx = c.ctx;
    const lgr_match_stats& st = c.st;
    const Side& B = c.B;
    const PruneWs& W = c.W;
    const int n_rb = c.n_rb, n_cc = c.n_cc, n_leaves = c.n_leaves, ma_pad = c.ma_pad, mb_pad = c.mb_pad;
    fprintf(stderr, "[lgr] stages per pass:");
    for (int k = 0; k <= n_beta; ++k) fprintf(stderr, " %llu", hs->stages[k]);
    fprintf(stderr, " of %.0f (n_rb %d n_cc %d item_rb %d leaves %d)\n", st.stages_all, n_rb, n_cc, c.item_rb, n_leaves);
    // what the schedule asks for at leaf granularity (the stages computed above also cover the neighbours' boundary tiles)
    std::vector<uint8_t> hd((size_t) n_rb * n_leaves), hsch((size_t) n_rb * n_leaves);
    LGR_HIP(ctx, hipMemcpy(hd.data(), W.done, hd.size(), hipMemcpyDeviceToHost));
    LGR_HIP(ctx, hipMemcpy(hsch.data(), W.sched, hsch.size(), hipMemcpyDeviceToHost));
    double need_cols = 0;
    for (int rb = 0; rb < n_rb; ++rb)
        for (int l = 0; l < n_leaves; ++l)
            if (hd[(size_t) rb * n_leaves + l] | hsch[(size_t) rb * n_leaves + l]) need_cols += B.h_leaf_start[l + 1] - B.h_leaf_start[l];
    fprintf(stderr, "[lgr] scheduled (row block, leaf) pairs cover %.4f of the tiles; computed stages %.4f\n",
            need_cols / ((double) n_rb * mb_pad), st.stages_done / st.stages_all);
    // which criterion asked for the final-pass tiles (hsch = the last pass): the block's rows, the leaf's columns, or both
    std::vector<float> hlb((size_t) n_rb * n_leaves), hurb(n_rb);
    std::vector<unsigned> hul(MAXLEAF);
    LGR_HIP(ctx, hipMemcpy(hlb.data(), W.LBsq, hlb.size() * 4, hipMemcpyDeviceToHost));
    LGR_HIP(ctx, hipMemcpy(hurb.data(), W.u_rb, hurb.size() * 4, hipMemcpyDeviceToHost));
    LGR_HIP(ctx, hipMemcpy(hul.data(), W.u_leaf, hul.size() * 4, hipMemcpyDeviceToHost));
    double by_rows = 0, by_cols = 0, by_both = 0;
    for (int rb = 0; rb < n_rb; ++rb)
        for (int l = 0; l < n_leaves; ++l) {
            if (!hsch[(size_t) rb * n_leaves + l]) continue;
            float lb = hlb[(size_t) rb * n_leaves + l], ug;
            memcpy(&ug, &hul[l], 4);
            bool r = hurb[rb] >= 0.f && lb <= hurb[rb] * 1.00001f + 1e-12f, cl = lb <= ug * 1.00001f + 1e-12f;
            double w = B.h_leaf_start[l + 1] - B.h_leaf_start[l];
            (r && cl ? by_both : r ? by_rows : by_cols) += w;
        }
    const double tot = (double) n_rb * mb_pad;
    fprintf(stderr, "[lgr] final pass by criterion: rows only %.4f, columns only %.4f, both %.4f of the tiles\n", by_rows / tot, by_cols / tot, by_both / tot);
    if (env_int("LGR_MATCH_DEBUG", 0) >= 2) {
        // how full are the sweep's VISITS?  A visit = one row block against one 128-tile column chunk: the stages its mask holds, of 32.  Every visit pays
        // the A fragments, the thresholds of its tile slots, the start of the DMA ring and two barriers before its first MFMA.
        std::vector<unsigned> hm((size_t) n_rb * n_cc);
        LGR_HIP(ctx, hipMemcpy(hm.data(), W.mask, hm.size() * 4, hipMemcpyDeviceToHost));
        double visits = 0, stages_ = 0, hist[6] = {0, 0, 0, 0, 0, 0}, runs = 0;   // visits holding 1-2, 3-4, 5-8, 9-16, 17-24, 25-32 stages
        for (unsigned m : hm) {
            if (!m) continue;
            const int n = __builtin_popcount(m);
            visits += 1; stages_ += n; runs += __builtin_popcount(m & ~(m << 1));
            hist[n <= 2 ? 0 : n <= 4 ? 1 : n <= 8 ? 2 : n <= 16 ? 3 : n <= 24 ? 4 : 5] += 1;
        }
        fprintf(stderr, "[lgr] last pass: %.0f visits (row block x chunk) of %zu, %.2f stages per visit in %.2f runs; visits by stages 1-2: %.3g, 3-4: %.3g, 5-8: %.3g, 9-16: %.3g, 17-24: %.3g, 25-32: %.3g\n",
                visits, hm.size(), stages_ / std::max(visits, 1.0), runs / std::max(visits, 1.0), hist[0], hist[1], hist[2], hist[3], hist[4], hist[5]);
    }
    if (c.split_used && env_int("LGR_MATCH_DEBUG", 0) >= 2 && h_kept[0] <= (unsigned long long) c.kept_cap) {
        // how are the tiles the sweep keeps distributed over the (row block, stage) pairs -- 32 tile slots each?  (Round 5, 900 k points, scene
        // seed 571: 16 M kept tiles, 78 % of them in pairs that keep more than half of their slots -- blobs of near-duplicate descriptors.
        // Flagging such stages from the list and giving them to the plain six-step kernel as a whole: 40.8 -> 38.0 ms for that scene, nothing
        // for the others; what those blobs needed was pass 0 taking every zero lower bound (near_kernel): 26.1 ms, 0.6 M kept tiles.)
        const size_t nk = (size_t) h_kept[0];
        std::vector<uint2> hk(nk);
        if (nk) LGR_HIP(ctx, hipMemcpy(hk.data(), c.kept, nk * sizeof(uint2), hipMemcpyDeviceToHost));
        std::vector<unsigned long long> key(nk);
        for (size_t i = 0; i < nk; ++i) key[i] = ((unsigned long long) (hk[i].x / (BLOCK_ROWS / TILE)) << 32) | (hk[i].y / STAGE_TILES);
        std::sort(key.begin(), key.end());
        double hist[6] = {0, 0, 0, 0, 0, 0}, pairs_ = 0;   // kept tiles in pairs holding 1-2, 3-4, 5-8, 9-16, 17-24, 25-32 of them
        for (size_t i = 0; i < nk;) {
            size_t j = i;
            while (j < nk && key[j] == key[i]) ++j;
            const size_t n = j - i;
            hist[n <= 2 ? 0 : n <= 4 ? 1 : n <= 8 ? 2 : n <= 16 ? 3 : n <= 24 ? 4 : 5] += (double) n;
            pairs_ += 1; i = j;
        }
        fprintf(stderr, "[lgr] kept tiles %zu in %.0f (row block, stage) pairs; tiles by the pair's count 1-2: %.3g, 3-4: %.3g, 5-8: %.3g, 9-16: %.3g, 17-24: %.3g, 25-32: %.3g\n",
                nk, pairs_, hist[0], hist[1], hist[2], hist[3], hist[4], hist[5]);
    }
    if (c.coarse && c.both && env_int("LGR_MATCH_DEBUG", 0) >= 2) {
        // What would homogeneous tiles be worth?  (Round 5, bench pair: scheduled pairs 1.57e8 tiles, tile maxima in the present order 1.03e8,
        // element level 6.8e7 -- rows and columns sorted by U would lose the radial shells, which take 88 M tile slots to 54 M tested, for at
        // most a third fewer; and the leaf's bound tested per tile inside the sweep took 54.4 M tested tiles to 47.4 M for 0.1 ms and four
        // spilled VGPRs: the (row block, leaf) bounds themselves are what limits the final pass, not the granularity of the upper bounds.)  32 x 32 tiles of the scheduled (row block, leaf) pairs that ANY element-level criterion
        // needs (LB^2 <= U^2 of the row or of the column), counted (i) per (row block, leaf) as scheduled, (ii) per tile with the present
        // row / column order (tile maxima), (iii) as if rows and columns were sorted by U inside their block / leaf (the fraction of
        // rows and of columns that need the pair).
        std::vector<float> hur(ma_pad), huc(mb_pad);
        LGR_HIP(ctx, hipMemcpy(hur.data(), W.u_row, hur.size() * 4, hipMemcpyDeviceToHost));
        LGR_HIP(ctx, hipMemcpy(huc.data(), W.u_colv, huc.size() * 4, hipMemcpyDeviceToHost));
        std::vector<std::vector<float>> rs(n_rb), cs(n_leaves), rts(n_rb), cts(n_leaves);
        for (int rb = 0; rb < n_rb; ++rb) {
            for (int r = 0; r < BLOCK_ROWS; ++r) rs[rb].push_back(std::max(hur[(size_t) rb * BLOCK_ROWS + r], 0.f));
            for (int t = 0; t < BLOCK_ROWS / TILE; ++t) rts[rb].push_back(*std::max_element(rs[rb].begin() + t * TILE, rs[rb].begin() + (t + 1) * TILE));
            std::sort(rs[rb].begin(), rs[rb].end()); std::sort(rts[rb].begin(), rts[rb].end());
        }
        for (int l = 0; l < n_leaves; ++l) {
            for (int col = B.h_leaf_start[l]; col < B.h_leaf_start[l + 1]; ++col) cs[l].push_back(std::max(huc[col], 0.f));
            for (size_t t = 0; t + TILE <= cs[l].size(); t += TILE) cts[l].push_back(*std::max_element(cs[l].begin() + t, cs[l].begin() + t + TILE));
            std::sort(cs[l].begin(), cs[l].end()); std::sort(cts[l].begin(), cts[l].end());
        }
        auto frac_ge = [](const std::vector<float>& v, float x) { return v.empty() ? 0.0 : (double) (v.end() - std::lower_bound(v.begin(), v.end(), x)) / (double) v.size(); };
        double t_sched = 0, t_tile = 0, t_ideal = 0, t_rows_ideal = 0, t_cols_ideal = 0;
        for (int rb = 0; rb < n_rb; ++rb)
            for (int l = 0; l < n_leaves; ++l) {
                if (!hsch[(size_t) rb * n_leaves + l]) continue;
                const float lb = hlb[(size_t) rb * n_leaves + l] / 1.00001f;
                const double tiles = 8.0 * (double) cts[l].size();
                const double pa = frac_ge(rs[rb], lb), pb = frac_ge(cs[l], lb), ta_ = frac_ge(rts[rb], lb), tb_ = frac_ge(cts[l], lb);
                t_sched += tiles;
                t_tile += tiles * (1.0 - (1.0 - ta_) * (1.0 - tb_));
                t_ideal += tiles * (1.0 - (1.0 - pa) * (1.0 - pb));
                t_rows_ideal += tiles * pa; t_cols_ideal += tiles * pb;
            }
        fprintf(stderr, "[lgr] final pass, 32 x 32 tiles by granularity of the criterion: scheduled pairs %.3g, tile maxima (present order) %.3g, element level (U-sorted tiles) %.3g "
                        "(rows alone %.3g, columns alone %.3g)\n", t_sched, t_tile, t_ideal, t_rows_ideal, t_cols_ideal);
    }
    if (c.coarse) {
        // how loose are the tile-level maxima the sweep's shell test uses?  quantiles of the rows' own bounds and of (tile max / tile median)
        std::vector<float> hu(ma_pad);
        LGR_HIP(ctx, hipMemcpy(hu.data(), W.u_row, hu.size() * 4, hipMemcpyDeviceToHost));
        std::vector<float> all, ratio;
        for (int t = 0; t < ma_pad / TILE; ++t) {
            std::vector<float> v;
            for (int r = 0; r < TILE; ++r) if (hu[(size_t) t * TILE + r] > 0.f) v.push_back(hu[(size_t) t * TILE + r]);
            if (v.size() < 8) continue;
            std::sort(v.begin(), v.end());
            ratio.push_back(v.back() / v[v.size() / 2]);
            all.insert(all.end(), v.begin(), v.end());
        }
        std::sort(all.begin(), all.end()); std::sort(ratio.begin(), ratio.end());
        auto q = [](const std::vector<float>& v, double f) { return v.empty() ? 0.f : v[(size_t) (f * (v.size() - 1))]; };
        fprintf(stderr, "[lgr] row bounds U^2: q10 %.3g q50 %.3g q90 %.3g q99 %.3g max %.3g; tile max / tile median: q10 %.2f q50 %.2f q90 %.2f q99 %.2f\n",
                q(all, 0.1), q(all, 0.5), q(all, 0.9), q(all, 0.99), q(all, 1.0), q(ratio, 0.1), q(ratio, 0.5), q(ratio, 0.9), q(ratio, 0.99));
    }
    return LGR_OK;
}

#ifdef EXP_PROF
// the EXP_PROF build: behind every MFMA launch group, the device's tick counters (g_prof, lgr_match_mfma.cuh) and the work list's split over the XCDs
static int match_prof_report(lgr_ctx* ctx, const int* xcd_start) {
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long hp[16];
    (void) hipMemcpyFromSymbol(hp, HIP_SYMBOL(g_prof), sizeof hp);
    int hx[9];
    (void) hipMemcpy(hx, xcd_start, sizeof hx, hipMemcpyDeviceToHost);
    fprintf(stderr, "[lgr] prof launch %d (10 ns ticks): prologue %llu stages %llu (barrier+dma wait %llu, - %llu) colflush %llu wg_total %llu | wgs %llu visits %llu rowflush %llu | items %d (per xcd %d %d %d %d %d %d %d %d)\n",
            ctx->mfma_timed - 1, hp[0], hp[1], hp[2], hp[5], hp[3], hp[4], hp[8], hp[9], hp[10], hx[8], hx[1] - hx[0], hx[2] - hx[1], hx[3] - hx[2],
            hx[4] - hx[3], hx[5] - hx[4], hx[6] - hx[5], hx[7] - hx[6], hx[8] - hx[7]);
    unsigned long long z[16] = {0};
    (void) hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z);
    return LGR_OK;
}
#endif
