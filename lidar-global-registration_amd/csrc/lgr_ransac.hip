// lgr_ransac.hip -- prerejective RANSAC on gfx950: on-device Philox sampling, polygon prerejection, 3-point Umeyama,
// batched hypothesis verification, uniformity / score metrics, adaptive bound, final SVD refit.
//
// Replaces src/sac_prerejective_omp.cpp:115-314 (SampleConsensusPrerejectiveOMP::align), src/metric.cpp:55-179,
// src/analysis.cpp:95-130 (uniformity), src/transformation.cpp:4-38 and the PCL pieces called from there
// (CorrespondenceRejectorPoly::thresholdPolygon, TransformationEstimationSVD -> umeyama).
//
// Schedule (deterministic, order-independent; the oracle's ORC_RNG_PHILOX mode states the same thing on the CPU):
//   iteration i draws Philox4x32-10(counter = i, key = seed); iterations are processed in batches; after a batch
//   the record inlier set (largest count, ties -> lowest i) tightens the bound through estimateMaxIterations and the
//   best hypothesis is the maximum metric (strict '>', ties -> lowest i).
// Float sequences restate the oracle op for op (oracle/src/orc_ransac.cpp); compiled with -ffp-contract=off.
// The loop itself runs from the device for all five metrics (RState, ransac_device_schedule below; rounds 4-5).  Uniformity / correspondences:
// the host enqueues two rounds and the final block blind and reads one record -- one synchronisation per alignment.  The plane metrics: the
// same rounds with the plane evaluation in them (a hypothesis's sparse subset is keyed by its iteration), then a host-driven final block
// (lgr_ransac_ex_dev) -- or, for the set of distinct hypotheses (lgr_ransac_multi_ex_dev), a final block per member that stays on the device.
// This file is the host side; the kernels are in lgr_ransac_common.cuh (sampling, hypotheses), lgr_ransac_count.cuh (packing, phase 1),
// lgr_ransac_metric.cuh (phase 2, refit) and lgr_ransac_schedule.cuh (the device-driven loop), all one translation unit.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <vector>

#include "lgr_host.h"
#include "lgr_internal.h"
#include "lgr_pointpass.cuh"
#include "lgr_ransac_schedule.cuh"

namespace {

// include/utils.h:34-43 calculateCombinationOrMax<int>
int comb_or_max(int n, int k) {
    double result = 1.0;
    for (int i = 0; i < k; ++i) { result *= n - i; result /= i + 1; }
    int mx = INT_MAX;
    return result > mx ? mx : (int) result;
}

// WS_RANSAC_MISC as every entry point of this file sees it (lgr_gror.hip keeps a list of its own in the slot during its own call).  One
// size for all of them, so the slot is never re-allocated under a pointer taken earlier in the same call.
struct RansacMisc {
    RState S;          // the device-driven schedule's state; S.best_T and S.Tn are the best and the refit transform of an alignment, plane metrics included
    float ev[8];       // evaluate_one_dev: [0..2] the evaluation in flight, [4..6] the guess's (rs_guess_kernel reads it)
    float out[4];      // a small result the host reads back: evaluate_one's (metric, n_inl bits, rmse), lgr_selfcheck_philox's block
    float T[16];       // a single transform the host uploaded (lgr_evaluate*_dev), lgr_refit_svd_dev's result
};
int ransac_misc(lgr_ctx* ctx, RansacMisc** out) { return lgr_ws_t(ctx, WS_RANSAC_MISC, 1, out); }

}  // namespace

int lgr_check_corr(lgr_ctx* ctx, const lgr_corr* d_corr, int c, int ns, int nt) {
    if (ctx->corr_trusted || c <= 0) return LGR_OK;
    int* d_bad;
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_STATS, 64, &d_bad));
    LGR_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, ctx->stream));
    corr_range_kernel<<<cdiv(c, 256), 256, 0, ctx->stream>>>(d_corr, c, ns, nt, d_bad);
    int* h;
    LGR_TRY(lgr_pinned(ctx, 64, (void**) &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h[0]) return lgr_fail(ctx, LGR_ERR_INVALID_ARG, "a correspondence index is outside its cloud (index_query in [0, ns), index_match in [0, nt))", __FILE__, __LINE__);
    return LGR_OK;
}

namespace {
int pack(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c, Packed* out) {
    LGR_TRY(lgr_check_corr(ctx, d_corr, c, ns, nt));
    const unsigned* bbk;
    LGR_TRY(lgr_bbox_launch(ctx, d_src, ns, &bbk));   // UniformityMetricEstimator::setSourceCloud (src/metric.cpp:167-170); stays on the device
    float4* P;
    const int cpad = (c + 63) & ~63;
    const size_t n4 = (size_t) c * 2 + (size_t) (c + 3) / 4 + 4;                     // P0, P1, sstar
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_PACK, n4 + (size_t) cpad * 2 + 8, &P));           // + PP (32 bytes per correspondence) + pstats
    out->P0 = P; out->P1 = P + c; out->sstar = (float*) (P + 2 * (size_t) c);
    float* PP = (float*) (P + n4);
    unsigned* pstats = (unsigned*) (P + n4 + (size_t) cpad * 2);
    out->PP = (const CPair*) PP; out->pstats = pstats;
    LGR_HIP(ctx, hipMemsetAsync(pstats, 0, 16, ctx->stream));
    if (c > 0)
        pack_kernel<<<std::min(cdiv(cpad, 256), 512), 256, 0, ctx->stream>>>(d_src, d_tgt, d_corr, c, bbk, out->P0, out->P1, out->sstar, PP, pstats, cpad);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// refit over the inliers flagged in d_mask (NULL: all pairs): compaction in correspondence order, then refit_kernel; the number of inliers
// stays on the device
int refit_launch(lgr_ctx* ctx, const Packed& pk, int c, const uint8_t* d_mask, float* d_Tout) {
    if (!d_mask || c == 0) {
        refit_kernel<<<1, 256, 0, ctx->stream>>>(pk.P0, pk.P1, c, d_Tout);
        LGR_HIP(ctx, hipGetLastError());
        return LGR_OK;
    }
    int* flags;
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_HIST, (size_t) 2 * c + 16 + 8 * ((size_t) c + 4), &flags));
    int* pos = flags + c;
    float4* Q0 = (float4*) (((uintptr_t) (flags + 2 * (size_t) c) + 15) & ~(uintptr_t) 15);
    float4* Q1 = Q0 + c;
    mask_flags_kernel<<<cdiv(c, 256), 256, 0, ctx->stream>>>(d_mask, c, flags);
    LGR_TRY(pp_scan_flags(ctx, flags, pos, (size_t) c));
    compact_pairs_kernel<<<cdiv(c, 256), 256, 0, ctx->stream>>>(pk.P0, pk.P1, flags, pos, c, Q0, Q1);
    refit_kernel<<<1, 256, 0, ctx->stream>>>(Q0, Q1, 0, d_Tout, pos + (c - 1), flags + (c - 1));
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// the workspace of a refit over c flagged pairs: the scan's positions, the compacted pairs and the scan's temporary storage
int refit_flagged_ws(lgr_ctx* ctx, int c, int** pos, float4** Q0, float4** Q1) {
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_HIST, (size_t) c + 16 + 8 * ((size_t) c + 4), pos));
    *Q0 = (float4*) (((uintptr_t) (*pos + (size_t) c) + 15) & ~(uintptr_t) 15);
    *Q1 = *Q0 + c;
    size_t tb = 0;
    void* tmp;
    LGR_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, *pos, *pos, 0, (size_t) c, rocprim::plus<int>(), ctx->stream));
    return lgr_ws(ctx, WS_GRID_TMP, tb, &tmp);   // what pp_scan_flags will ask for
}

size_t metric_smem() { return (size_t) (30000 + 64) * 4; }

int metric_launch(lgr_ctx* ctx, const float* Ts, const int* list2, int nh2, const Packed& pk, int c, int metric_id, int score_id,
                  float* metric_out, int* ninl_out, float* rmse_out, uint8_t* mask,
                  const unsigned* maskT = nullptr, const int* hpos = nullptr, int mask_nh = 0) {
    // per device, so not cached in a process-wide flag (a process may hold contexts on several GPUs); the call is a host-side table update
    LGR_HIP(ctx, hipFuncSetAttribute((const void*) metric_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) metric_smem()));
    bool need_list = metric_id != LGR_METRIC_UNIFORMITY || rmse_out;
    // hypotheses are processed in waves of at most `wave` workgroups so that the ordered inlier lists stay bounded
    int wave = need_list ? std::max(1, std::min(nh2, 512)) : std::max(1, nh2);   // without lists: all candidates in one launch
    float2* scratch = nullptr;
    if (need_list) LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_LIST, (size_t) wave * std::max(c, 1), &scratch));
    for (int h0 = 0; h0 < nh2; h0 += wave) {
        int nh = std::min(wave, nh2 - h0);
        metric_kernel<<<nh, MB, metric_smem(), ctx->stream>>>(Ts, list2 ? list2 + h0 : nullptr, nh, pk.P0, pk.P1, pk.sstar, c, metric_id,
                                                              score_id, metric_out + h0, ninl_out + h0,
                                                              rmse_out ? rmse_out + h0 : nullptr, mask, scratch, maskT, hpos ? hpos + h0 : nullptr, mask_nh);
    }
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

struct EvalOut { int n_inl; float rmse; float metric; };
// single transform (device pointer d_T to 16 floats): mask + stats, read back
int evaluate_one(lgr_ctx* ctx, const float* d_T, const Packed& pk, int c, int metric_id, int score_id, uint8_t* d_mask, EvalOut* out) {
    RansacMisc* M;
    LGR_TRY(ransac_misc(ctx, &M));
    float* d_metric = M->out; int* d_ninl = (int*) (M->out + 1); float* d_rmse = M->out + 2;
    LGR_TRY(metric_launch(ctx, d_T, nullptr, 1, pk, c, metric_id, score_id, d_metric, d_ninl, d_rmse, d_mask));
    float* h;
    LGR_TRY(lgr_pinned(ctx, 64, (void**) &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, d_metric, 12, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out->metric = h[0]; memcpy(&out->n_inl, &h[1], 4); out->rmse = h[2];
    return LGR_OK;
}

}  // namespace

int lgr_refit_flagged_reserve(lgr_ctx* ctx, int c) {
    int* pos;
    float4 *Q0, *Q1;
    return refit_flagged_ws(ctx, c, &pos, &Q0, &Q1);
}

int lgr_refit_flagged_launch(lgr_ctx* ctx, const float4* P0, const float4* P1, int c, int* d_flags, const int* d_n, float* d_Tout) {
    int* pos;
    float4 *Q0, *Q1;
    LGR_TRY(refit_flagged_ws(ctx, c, &pos, &Q0, &Q1));
    LGR_TRY(pp_scan_flags(ctx, d_flags, pos, (size_t) c));
    compact_pairs_kernel<<<cdiv(c, 256), 256, 0, ctx->stream>>>(P0, P1, d_flags, pos, c, Q0, Q1);
    refit_kernel<<<1, 256, 0, ctx->stream>>>(Q0, Q1, 0, d_Tout, d_n, d_n + 1);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// single transform under a plane metric: counter = 0xFFFFFFFE / 0xFFFFFFFF for the two evaluations of the final block.
// closest_plane: inliers / rmse / metric from the plane test, pairs (sorted by source index) returned for the refit.
int evaluate_one_plane(lgr_ctx* ctx, const float* d_T, const Packed& pk, int c, int metric_id, int score_id, uint8_t* d_mask,
                       const lgr_plane_dev& plane, unsigned counter, EvalOut* out, std::vector<int2>* pairs) {
    int* pl;
    LGR_TRY(lgr_ws_t(ctx, WS_PLANE_OUT, (size_t) 8 + 2 * (size_t) std::max(plane.n_sp, 1) + 8, &pl));
    int* d_cnt = pl; float* d_cp = (float*) (pl + 1); float* d_rm = (float*) (pl + 2); int* d_np = pl + 3;
    int2* d_pairs = (int2*) (pl + 8);
    const bool want_pairs = pairs != nullptr;
    LGR_TRY(lgr_plane_eval(ctx, plane, d_T, nullptr, 1, counter, score_id, d_cnt, d_cp, d_rm, want_pairs ? d_pairs : nullptr, d_np));
    int* h;
    LGR_TRY(lgr_pinned(ctx, 64 + (size_t) 8 * std::max(plane.n_sp, 1), (void**) &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, pl, 16, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int cnt = h[0];
    float cp, rm;
    memcpy(&cp, &h[1], 4); memcpy(&rm, &h[2], 4);
    if (want_pairs) {
        pairs->resize(cnt);
        if (cnt) {
            LGR_HIP(ctx, hipMemcpyAsync(h + 16, d_pairs, (size_t) cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
            LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
            memcpy(pairs->data(), h + 16, (size_t) cnt * 8);
            std::sort(pairs->begin(), pairs->end(), [](const int2& a, const int2& b) { return a.x < b.x; });   // source indices are distinct
        }
    }
    if (metric_id == LGR_METRIC_CLOSEST_PLANE || metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE) {
        if (d_mask) LGR_HIP(ctx, hipMemsetAsync(d_mask, 0, (size_t) c, ctx->stream));
        out->n_inl = cnt; out->rmse = rm; out->metric = cp;
        return LGR_OK;
    }
    EvalOut e;
    LGR_TRY(evaluate_one(ctx, d_T, pk, c, LGR_METRIC_CORRESPONDENCES, LGR_SCORE_CONSTANT, d_mask, &e));
    out->n_inl = e.n_inl; out->rmse = e.rmse; out->metric = e.metric * cp;
    return LGR_OK;
}

// one transform under the closest-plane metric, or (d_weights) the weighted one
static int evaluate_plane_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16], int score_id, uint64_t seed,
                              uint32_t counter, int metric_id, const float* d_weights, float weights_sum, int* n_inliers, float* rmse, float* metric,
                              float* threshold, int32_t* pairs, int* n_pairs) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    const bool weighted = metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE;
    LGR_CHECK(ctx, d_src && d_tgt && (d_weights || !weighted) && T16 && n_inliers && rmse && metric && ns > 0 && nt > 1 && score_id >= 0 && score_id <= 3,
              LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    lgr_plane_dev plane;
    LGR_TRY(lgr_plane_setup(ctx, d_src, ns, d_tgt, nt, seed, &plane));
    if (weighted) { plane.w = d_weights; plane.w_sum = weights_sum; plane.w_gate = 0.f; }   // (one transform: no gate)
    RansacMisc* M;
    LGR_TRY(ransac_misc(ctx, &M));
    LGR_HIP(ctx, hipMemcpyAsync(M->T, T16, 64, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    Packed none{nullptr, nullptr, nullptr};
    EvalOut e;
    std::vector<int2> pr;
    LGR_TRY(evaluate_one_plane(ctx, M->T, none, 0, metric_id, score_id, nullptr, plane, counter, &e, pairs ? &pr : nullptr));
    *n_inliers = e.n_inl; *rmse = e.rmse; *metric = e.metric;
    if (threshold) *threshold = plane.thr;
    if (pairs) {
        for (size_t i = 0; i < pr.size(); ++i) { pairs[2 * i] = pr[i].x; pairs[2 * i + 1] = pr[i].y; }
        if (n_pairs) *n_pairs = (int) pr.size();
    }
    return LGR_OK;
}
extern "C" int lgr_evaluate_plane_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16], int score_id,
                                      uint64_t seed, uint32_t counter, int* n_inliers, float* rmse, float* metric, float* threshold,
                                      int32_t* pairs, int* n_pairs) {
    return evaluate_plane_dev(ctx, d_src, ns, d_tgt, nt, T16, score_id, seed, counter, LGR_METRIC_CLOSEST_PLANE, nullptr, 0.f, n_inliers, rmse, metric,
                              threshold, pairs, n_pairs);
}
extern "C" int lgr_evaluate_plane_weighted_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16], int score_id,
                                               uint64_t seed, uint32_t counter, const float* d_weights, float weights_sum, int* n_inliers, float* rmse,
                                               float* metric, float* threshold, int32_t* pairs, int* n_pairs) {
    return evaluate_plane_dev(ctx, d_src, ns, d_tgt, nt, T16, score_id, seed, counter, LGR_METRIC_WEIGHTED_CLOSEST_PLANE, d_weights, weights_sum, n_inliers,
                              rmse, metric, threshold, pairs, n_pairs);
}

extern "C" int lgr_ransac_samples_n_dev(lgr_ctx* ctx, uint64_t seed, int first, int n, int n_corr, int n_samples, int32_t* d_tuples) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n_samples >= LGR_MIN_SAMPLES && n_samples <= LGR_MAX_SAMPLES, LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, n >= 0 && n_corr >= n_samples && (d_tuples || n == 0) && first >= 0, LGR_ERR_INVALID_ARG);
    if (n == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    LGR_NS_DISPATCH(n_samples, (samples_kernel<NS><<<cdiv(n, 256), 256, 0, ctx->stream>>>(seed, first, n, n_corr, d_tuples)));
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}
extern "C" int lgr_ransac_samples_dev(lgr_ctx* ctx, uint64_t seed, int first, int n, int n_corr, int32_t* d_triples) {
    return lgr_ransac_samples_n_dev(ctx, seed, first, n, n_corr, 3, d_triples);
}

// lgr.h: one Philox4x32-10 block through the device's generator (known-answer tests; philox_kernel, lgr_ransac_common.cuh)
extern "C" int lgr_selfcheck_philox(lgr_ctx* ctx, uint64_t key, const uint32_t counter4[4], uint32_t out4[4]) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, counter4 && out4, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    RansacMisc* M;
    LGR_TRY(ransac_misc(ctx, &M));
    unsigned* d = reinterpret_cast<unsigned*>(M->out);
    philox_kernel<<<1, 1, 0, ctx->stream>>>(key, counter4[0], counter4[1], counter4[2], counter4[3], d);
    LGR_HIP(ctx, hipGetLastError());
    LGR_HIP(ctx, hipMemcpyAsync(out4, d, 16, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_evaluate_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                                const float T16[16], int metric_id, int score_id,
                                uint8_t* d_mask, int* n_inliers, float* rmse, float* metric) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, d_src && d_tgt && (d_corr || c == 0) && T16 && c >= 0 && ns > 0 && nt > 0, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, metric_id == LGR_METRIC_UNIFORMITY || metric_id == LGR_METRIC_CORRESPONDENCES, LGR_ERR_UNSUPPORTED);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    Packed pk;
    LGR_TRY(pack(ctx, d_src, ns, d_tgt, nt, d_corr, c, &pk));
    RansacMisc* M;
    LGR_TRY(ransac_misc(ctx, &M));
    LGR_HIP(ctx, hipMemcpyAsync(M->T, T16, 64, hipMemcpyHostToDevice, ctx->stream));
    EvalOut e;
    LGR_TRY(evaluate_one(ctx, M->T, pk, c, metric_id, score_id, d_mask, &e));
    if (n_inliers) *n_inliers = e.n_inl;
    if (rmse) *rmse = e.rmse;
    if (metric) *metric = e.metric;
    return LGR_OK;
}

// The per-iteration arrays of a round of the device-driven schedule (and of lgr_ransac_replay_dev), nb iterations each.  `ok` (the
// prerejection flags hypotheses_kernel writes and compact_kernel scans) is used by lgr_ransac_replay_dev alone; the schedule appends its
// survivors to `list` itself and reuses `pos` as its posmap (iteration offset -> position in `list`).
struct BatchBuffers {
    float* Ts; int* ok; int* pos; int* list; int2* counts; int* list2; float* metric; int* ninl; int* hpos;
};
static int batch_buffers(lgr_ctx* ctx, int nb, BatchBuffers* b) {
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_T, (size_t) nb * 16, &b->Ts));
    int* s;
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_STATS, (size_t) nb * 9 + 64, &s));
    b->ok = s; b->pos = s + nb; b->list = s + 2 * (size_t) nb; b->counts = (int2*) (s + 3 * (size_t) nb);
    b->list2 = s + 5 * (size_t) nb; b->metric = (float*) (s + 6 * (size_t) nb); b->ninl = s + 7 * (size_t) nb; b->hpos = s + 8 * (size_t) nb;
    return LGR_OK;
}

// single-transform evaluation without a read-back: (metric, n_inl bits, rmse) -> d_out3 (device)
static int evaluate_one_dev(lgr_ctx* ctx, const float* d_T, const Packed& pk, int c, int metric_id, int score_id, uint8_t* d_mask, float* d_scratch3,
                            float* d_out3) {
    float* d_metric = d_scratch3; int* d_ninl = (int*) (d_scratch3 + 1); float* d_rmse = d_scratch3 + 2;
    LGR_HIP(ctx, hipMemsetAsync(d_rmse, 0, 4, ctx->stream));
    if (metric_id == LGR_METRIC_UNIFORMITY && c > 0) {
        int* ghist;
        LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_GHIST, (size_t) 30000 + 64, &ghist));
        LGR_HIP(ctx, hipMemsetAsync(ghist, 0, (30000 + 1) * 4, ctx->stream));
        LGR_HIP(ctx, hipFuncSetAttribute((const void*) metric_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) metric_smem()));
        inlier_hist_kernel<<<cdiv(c, 256), 256, 0, ctx->stream>>>(d_T, pk.P0, pk.P1, pk.sstar, c, d_mask, ghist);
        metric_kernel<<<1, MB, metric_smem(), ctx->stream>>>(d_T, nullptr, 1, pk.P0, pk.P1, pk.sstar, c, metric_id, score_id, d_metric, d_ninl, nullptr, nullptr,
                                                             nullptr, nullptr, nullptr, 0, ghist);
    } else {
        LGR_TRY(metric_launch(ctx, d_T, nullptr, 1, pk, c, metric_id, score_id, d_metric, d_ninl, nullptr, d_mask));
    }
    rs_store_eval_kernel<<<1, 64, 0, ctx->stream>>>(d_scratch3, d_out3);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// The working set of the device-driven loop -- and of the second pass over its iterations (lgr_ransac_multi_dev), which calls loop_buffers
// with the same arguments and so finds the same slots at the same sizes: nothing is reallocated under the loop's pointers.
struct LoopBuffers {
    BatchBuffers b;              // the per-iteration arrays of a round, nb_max iterations each
    int* posmap;                 // = b.pos: iteration offset in the round -> position in the survivors' list
    unsigned* maskT;             // uniformity: inlier bit masks [mask_cap][mask_pitch(c)], as many rows as 2 GB hold (more survivors: the metric
    int mask_cap;                //   kernel tests every correspondence again)
    float2* scratch;             // the other metrics: one ordered inlier list per workgroup of the metric grid
    int* pl_cnt; float* pl_cp;   // plane metrics: the plane test's inlier count and metric per evaluated hypothesis (closest_plane: every
                                 //   survivor, indexed like the survivors' list; combination: every candidate)
    int g_metric, g_count;       // grids: one 120 KB workgroup per CU; four times the resident single-wave workgroups (the tail evens out)
    int nb_max;                  // iterations of a full round
    RState* dS; float* d_ev;     // the loop's state; scratch of the single-transform evaluations
};
static int loop_buffers(lgr_ctx* ctx, const lgr_params* p, int c, int max_iterations, int batch, const lgr_plane_dev* plane, LoopBuffers* L) {
    const int nb_max = (int) std::min<long long>((long long) batch * MAX_ROUND_BATCHES, std::max(max_iterations, 1));
    L->nb_max = nb_max;
    LGR_TRY(batch_buffers(ctx, nb_max, &L->b));
    L->posmap = L->b.pos;
    RansacMisc* M;
    LGR_TRY(ransac_misc(ctx, &M));
    L->dS = &M->S; L->d_ev = M->ev;
    L->maskT = nullptr; L->mask_cap = 0;
    if (p->metric_id == LGR_METRIC_UNIFORMITY) {
        const size_t words = mask_pitch(c);
        L->mask_cap = (int) std::min<size_t>((size_t) nb_max, ((size_t) 2 << 30) / (words * 4));
        if (L->mask_cap > 0) LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_MASKT, words * (size_t) L->mask_cap, &L->maskT));
    }
    L->pl_cnt = nullptr; L->pl_cp = nullptr;
    if (plane) {
        LGR_TRY(lgr_ws_t(ctx, WS_PLANE_OUT, (size_t) 2 * nb_max + 16, &L->pl_cnt));
        L->pl_cp = (float*) (L->pl_cnt + nb_max);
    }
    L->g_metric = std::max(1, ctx->n_cu); L->g_count = 128 * std::max(1, ctx->n_cu);
    L->scratch = nullptr;
    if (p->metric_id != LGR_METRIC_UNIFORMITY) LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_LIST, (size_t) L->g_metric * std::max(c, 1), &L->scratch));
    return LGR_OK;
}

// the metric of the round's candidates (b.list2, their number in dS->n_cand): a fixed grid strides over them
static int metric_candidates(lgr_ctx* ctx, const LoopBuffers& L, const Packed& pk, int c, int metric_id, int score_id) {
    LGR_HIP(ctx, hipFuncSetAttribute((const void*) metric_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) metric_smem()));
    metric_kernel<<<L.g_metric, MB, metric_smem(), ctx->stream>>>(L.b.Ts, L.b.list2, 0, pk.P0, pk.P1, pk.sstar, c, metric_id, score_id, L.b.metric, L.b.ninl,
                                                                  nullptr, nullptr, L.scratch, L.maskT, L.b.hpos, L.mask_cap, nullptr, &L.dS->n_cand, &L.dS->n_ok);
    return LGR_OK;
}

// The front of a round, behind whatever set the round's range and gate in the RState (rs_begin in the loop, mh_begin in the second pass):
// hypotheses -> inlier counts -> candidates -> their metric in b.metric / b.ninl.  nb_up: an upper bound of the round's iterations.
// gated = false (the second pass of lgr_ransac_multi_ex_dev): the plane evaluation runs every subset to its end -- the values of an abandoned
// hypothesis are partial and timing dependent, and an item of the fold must be exact; dS->final_metric / dS->largest are not read then.
static int enqueue_round_front(lgr_ctx* ctx, const LoopBuffers& L, const Packed& pk, int c, const lgr_params* p, uint64_t seed, int nb_up,
                               const lgr_plane_dev* plane, bool gated = true) {
    const BatchBuffers& b = L.b;
    RState* const dS = L.dS;
    const bool closest = plane && (p->metric_id == LGR_METRIC_CLOSEST_PLANE || p->metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE);
    LGR_NS_DISPATCH(p->n_samples, (rs_hyp_kernel<NS><<<cdiv(nb_up, 128), 128, 0, ctx->stream>>>(pk.P0, pk.P1, c, seed, dS, p->edge_thr_coef, b.Ts, b.list,
                                                                                                 L.posmap, b.counts)));
    count_list_kernel<<<L.g_count, CB, 0, ctx->stream>>>(b.Ts, b.list, &dS->n_ok, pk.PP, pk.pstats, c, b.counts, L.maskT, L.mask_cap);
    if (closest) {
        // every survivor on its sparse subset; its plane inliers are "the inliers" (gate: the loop's best metric and record so far)
        const lgr_plane_dyn dyn{&dS->n_ok, &dS->round_first, gated ? &dS->final_metric : nullptr, gated ? &dS->largest : nullptr, gated ? &dS->n_gated : nullptr};
        LGR_TRY(lgr_plane_eval(ctx, *plane, b.Ts, b.list, nb_up, 0u, p->score_id, L.pl_cnt, L.pl_cp, nullptr, nullptr, nullptr, 0.f, gated ? 0 : 0x7fffffff, nullptr, &dyn));
        rs_plane_counts_kernel<<<64, 256, 0, ctx->stream>>>(dS, L.pl_cnt, b.counts);
    }
    rs_cand_kernel<<<64, 1024, 0, ctx->stream>>>(dS, b.counts, b.list, b.list2, b.hpos);
    if (closest) {
        rs_plane_pick_kernel<<<64, 256, 0, ctx->stream>>>(dS, b.hpos, L.pl_cnt, L.pl_cp, b.metric, b.ninl);
    } else if (plane) {   // combination: correspondences metric with the constant score (include/metric.h:191-192) x plane metric of the candidates
        LGR_TRY(metric_candidates(ctx, L, pk, c, LGR_METRIC_CORRESPONDENCES, LGR_SCORE_CONSTANT));
        const lgr_plane_dyn dyn{&dS->n_cand, &dS->round_first, gated ? &dS->final_metric : nullptr, gated ? &dS->int_max : nullptr, gated ? &dS->n_gated : nullptr};   // (records are correspondence counts here: only the metric gates)
        LGR_TRY(lgr_plane_eval(ctx, *plane, b.Ts, b.list2, nb_up, 0u, p->score_id, L.pl_cnt, L.pl_cp, nullptr, nullptr, nullptr, 0.f, 0x7fffffff, gated ? b.metric : nullptr, &dyn));
        rs_plane_mul_kernel<<<64, 256, 0, ctx->stream>>>(dS, b.metric, L.pl_cp);
    } else {
        LGR_TRY(metric_candidates(ctx, L, pk, c, p->metric_id, p->score_id));
    }
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// :265-296 the final re-estimation on the device: evaluation of d_T (-> d_e, inlier flags in d_mask), refit over its inliers (-> d_Tn),
// evaluation of the refit (-> d_e2); sized on the device, nothing is read back
static int enqueue_final_block(lgr_ctx* ctx, const Packed& pk, int c, const lgr_params* p, const float* d_T, uint8_t* d_mask, float* d_Tn, float* d_e,
                               float* d_e2) {
    RansacMisc* M;
    LGR_TRY(ransac_misc(ctx, &M));
    LGR_TRY(evaluate_one_dev(ctx, d_T, pk, c, p->metric_id, p->score_id, d_mask, M->ev, d_e));
    LGR_TRY(refit_launch(ctx, pk, c, d_mask, d_Tn));
    return evaluate_one_dev(ctx, d_Tn, pk, c, p->metric_id, p->score_id, d_mask, M->ev, d_e2);
}
// ... and its verdict, from the evaluation of the transform the block started from (:276-279); the least tolerable metric is 0.3 for
// uniformity (include/metric.h:97-99) and 0 for every other estimator (:73-75, :124-126, :198-200)
static bool final_converged(int e_ninl, float e_metric, int c, int metric_id) {
    const bool enough = e_ninl > MIN_NR_FINAL_INLIERS || (float) e_ninl > MIN_INLIER_RATE * (float) c;
    const float min_tol = metric_id == LGR_METRIC_UNIFORMITY ? 0.3f : 0.0f;
    return enough && e_metric > min_tol;
}
// the loop's state S and the outcome of a final block -> *res (Tn == nullptr: res->transformation stays)
static void fill_result(lgr_result* res, const RState& S, const float* Tn, bool converged, int n_inliers, float metric) {
    if (Tn) memcpy(res->transformation, Tn, 64);
    res->iterations = S.done;
    res->converged = converged ? 1 : 0;
    res->n_inliers = n_inliers;
    res->metric = metric;
    res->best_metric_before_refit = S.final_metric;
    res->best_iteration = S.best_iter;
    res->num_rejections = S.num_rejections;
    res->estimated_iters = S.bound;
}

// the whole loop as one launch (LGR_RANSAC_SCHEDULE_RESIDENT): the one place that lists the working set for rs_resident_kernel
static int launch_resident(lgr_ctx* ctx, const LoopBuffers& L, const float* d_src, const float* d_tgt, const lgr_corr* d_corr, int c, const Packed& pk,
                           const lgr_params* p, uint64_t seed, int max_iterations, int batch) {
    LGR_HIP(ctx, hipFuncSetAttribute((const void*) rs_resident_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) metric_smem()));
    int per_cu = 0;
    LGR_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*) rs_resident_kernel, MB, metric_smem()));
    LGR_CHECK(ctx, per_cu >= 1 && L.g_metric >= 1, LGR_ERR_HIP);   // (the grid must fit the device at once: one workgroup per CU)
    const BatchBuffers& b = L.b;
    ResidentArgs ra{};
    ra.c = c; ra.n_samples = p->n_samples; ra.seed = seed; ra.edge_thr = p->edge_thr_coef;
    ra.S = L.dS; ra.Ts = b.Ts; ra.list = b.list; ra.posmap = L.posmap; ra.counts = b.counts; ra.list2 = b.list2; ra.hpos = b.hpos;
    ra.metric = b.metric; ra.ninl = b.ninl;
    ra.maskT = L.maskT; ra.mask_cap = L.mask_cap; ra.scratch = L.scratch; ra.metric_id = p->metric_id; ra.score_id = p->score_id;
    ra.max_rounds = (int) std::min<long long>(((long long) max_iterations + batch - 1) / batch + 2, INT_MAX);
    rs_resident_kernel<<<L.g_metric, MB, metric_smem(), ctx->stream>>>(ra, d_src, d_tgt, d_corr, pk.PP, pk.pstats, pk.P0, pk.P1, pk.sstar);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// The device-driven schedule: see RState.  Runs the loop and returns the host copy of its state in *out; the best transform stays on the
// device in RansacMisc::S.best_T.  ONE host synchronisation per pair of rounds -- one per alignment whenever the loop ends within two
// rounds, i.e. for every max_iterations up to 17 batches and whenever a record inlier set brings the bound below that.
//   schedule        LGR_RANSAC_SCHEDULE_CHAIN: six launches per round; LGR_RANSAC_SCHEDULE_RESIDENT: one kernel for the whole loop (not with `plane`)
//   plane           the plane metrics (round 5): the same rounds with the plane evaluation in them; nullptr otherwise
//   initial_metric  the metric to beat from the start: a guess's under a plane metric (the caller evaluated it), otherwise 0 -- the
//                   guess of uniformity / correspondences is evaluated here
//   d_final_mask    not nullptr: the final block (enqueue_final_block on best_T) is enqueued blind in front of the read-back, its outcome
//                   is in out->Tn / e_* / e2_* and the inlier flags of the refit in d_final_mask.  The plane metrics' final block is the
//                   caller's: its refit needs the plane pairs sorted by source index on the host.
static int ransac_device_schedule(lgr_ctx* ctx, const float* d_src, const float* d_tgt, const lgr_corr* d_corr, int c, const Packed& pk, const lgr_params* p,
                                  uint64_t seed, int max_iterations, int batch, int schedule, const lgr_plane_dev* plane, float initial_metric,
                                  uint8_t* d_final_mask, RState* out) {
    LoopBuffers L;
    LGR_TRY(loop_buffers(ctx, p, c, max_iterations, batch, plane, &L));
    RState* const dS = L.dS;
    RState* hS;
    LGR_TRY(lgr_pinned(ctx, sizeof(RState), (void**) &hS));
    memset(hS, 0, sizeof(RState));
    hS->bound = max_iterations; hS->max_iterations = max_iterations; hS->batch = batch; hS->round_cap = MAX_ROUND_BATCHES;
    hS->best_iter = -1; hS->metric_id = p->metric_id; hS->c = c; hS->nr_samples = p->n_samples; hS->confidence = p->confidence;
    hS->int_max = INT_MAX; hS->final_metric = initial_metric;
    for (int i = 0; i < 16; ++i) hS->best_T[i] = p->has_guess ? p->guess[i] : ((i % 5 == 0) ? 1.f : 0.f);
    LGR_HIP(ctx, hipMemcpyAsync(dS, hS, sizeof(RState), hipMemcpyHostToDevice, ctx->stream));
    if (p->has_guess && !plane) {
        // src/sac_prerejective_omp.cpp:134-147: the guess is the hypothesis to beat (final_tn / final_metric)
        uint8_t* d_gm;
        LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_MASK, (size_t) c + 16, &d_gm));
        LGR_TRY(evaluate_one_dev(ctx, dS->best_T, pk, c, p->metric_id, p->score_id, d_gm, L.d_ev, L.d_ev + 4));
        rs_guess_kernel<<<1, 1, 0, ctx->stream>>>(dS, L.d_ev + 4);
    }
    const bool ransac_debug = getenv("LGR_RANSAC_DEBUG") != nullptr;
    const BatchBuffers& b = L.b;
    auto enqueue_round = [&](bool first) -> int {
        rs_begin_kernel<<<1, 64, 0, ctx->stream>>>(dS, first ? 1 : 0);
        LGR_TRY(enqueue_round_front(ctx, L, pk, c, p, seed, first ? std::min(batch, L.nb_max) : L.nb_max, plane));
        rs_replay_kernel<<<1, 1024, 0, ctx->stream>>>(dS, b.list, b.list2, b.metric, b.ninl, b.counts, L.posmap, b.Ts);
        LGR_HIP(ctx, hipGetLastError());
        return LGR_OK;
    };
    // :265-296 final re-estimation (enqueued blind: redone when the loop turns out not to have ended), then the one read-back
    auto final_block_and_state = [&]() -> int {
        if (d_final_mask) LGR_TRY(enqueue_final_block(ctx, pk, c, p, dS->best_T, d_final_mask, dS->Tn, &dS->e_metric, &dS->e2_metric));
        LGR_HIP(ctx, hipMemcpyAsync(hS, dS, sizeof(RState), hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return LGR_OK;
    };
    if (schedule == LGR_RANSAC_SCHEDULE_RESIDENT) {
        const int g_metric = L.g_metric;
        LGR_TRY(launch_resident(ctx, L, d_src, d_tgt, d_corr, c, pk, p, seed, max_iterations, batch));
        LGR_TRY(final_block_and_state());
        if (ransac_debug) fprintf(stderr, "[lgr] ransac (resident kernel, %d workgroups) after %d rounds: done %d bound %d largest %d best metric %.4f stop %d abort %d\n", g_metric,
                                  hS->rounds, hS->done, hS->bound, hS->largest, hS->final_metric, hS->stop, hS->abort);
        if (ransac_debug) fprintf(stderr, "[lgr]   %d survivors, %d candidates in all\n", hS->tot_ok, hS->tot_cand);
        if (ransac_debug) fprintf(stderr, "[lgr]   workgroup 0, us per phase incl. barrier: begin/replay %.1f hyp %.1f count %.1f cand %.1f metric %.1f\n", hS->phase_ticks[0] * 0.01,
                                  hS->phase_ticks[1] * 0.01, hS->phase_ticks[2] * 0.01, hS->phase_ticks[3] * 0.01, hS->phase_ticks[4] * 0.01);
        if (ransac_debug) fprintf(stderr, "[lgr]   own work per workgroup, us, max / mean: hyp %.1f / %.1f count %.1f / %.1f cand %.1f / %.1f metric %.1f / %.1f\n",
                                  hS->busy_max[1] * 0.01, hS->busy_sum[1] * 0.01 / g_metric, hS->busy_max[2] * 0.01, hS->busy_sum[2] * 0.01 / g_metric,
                                  hS->busy_max[3] * 0.01, hS->busy_sum[3] * 0.01 / g_metric, hS->busy_max[4] * 0.01, hS->busy_sum[4] * 0.01 / g_metric);
        if (hS->abort || !hS->stop) {
            ctx->err = "resident RANSAC kernel: a grid barrier timed out (a workgroup of the grid did not become resident) or the loop did not end";
            return LGR_ERR_HIP;
        }
    } else {
        bool first = true;
        do {
            LGR_TRY(enqueue_round(first));
            first = false;
            LGR_TRY(enqueue_round(false));
            LGR_TRY(final_block_and_state());
            if (ransac_debug) fprintf(stderr, "[lgr] ransac (device schedule) after %d rounds: done %d bound %d largest %d best metric %.4f stop %d (%d survivors, %d candidates in all, %d abandoned by the plane gate)\n",
                                      hS->rounds, hS->done, hS->bound, hS->largest, hS->final_metric, hS->stop, hS->tot_ok, hS->tot_cand, hS->n_gated);
        } while (!hS->stop);
    }
    *out = *hS;
    return LGR_OK;
}

static int check_params(lgr_ctx* ctx, const lgr_params* p) {
    LGR_CHECK(ctx, p != nullptr, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, p->n_samples >= LGR_MIN_SAMPLES && p->n_samples <= LGR_MAX_SAMPLES, LGR_ERR_UNSUPPORTED);   // (fewer than 3 pairs leave Umeyama's rotation open)
    LGR_CHECK(ctx, p->metric_id == LGR_METRIC_UNIFORMITY || p->metric_id == LGR_METRIC_CORRESPONDENCES ||
                       p->metric_id == LGR_METRIC_CLOSEST_PLANE || p->metric_id == LGR_METRIC_COMBINATION ||
                       p->metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE,
              LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, p->score_id >= 0 && p->score_id <= 3, LGR_ERR_INVALID_ARG);
    return LGR_OK;
}

extern "C" int lgr_ransac_replay_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                                     const lgr_params* p, const int32_t* d_triples, int n,
                                     uint8_t* d_ok, float* d_T16, int32_t* d_n_inliers, float* d_metric) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_TRY(check_params(ctx, p));
    LGR_CHECK(ctx, p->metric_id == LGR_METRIC_UNIFORMITY || p->metric_id == LGR_METRIC_CORRESPONDENCES, LGR_ERR_UNSUPPORTED);   // plane metrics: lgr_evaluate_plane_dev
    LGR_CHECK(ctx, d_src && d_tgt && d_corr && d_triples && d_ok && d_T16 && d_n_inliers && d_metric && c >= p->n_samples && n >= 0 && ns > 0 && nt > 0, LGR_ERR_INVALID_ARG);
    if (n == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    Packed pk;
    LGR_TRY(pack(ctx, d_src, ns, d_tgt, nt, d_corr, c, &pk));
    BatchBuffers b;
    LGR_TRY(batch_buffers(ctx, n, &b));
    int n_ok = 0;
    // every prerejection survivor gets its metric here (no MIN_NR_INLIERS gate): replay reports per hypothesis
    LGR_NS_DISPATCH(p->n_samples, (hypotheses_kernel<NS><<<cdiv(n, 128), 128, 0, ctx->stream>>>(d_src, d_tgt, d_corr, c, 0, 0, n, d_triples, p->edge_thr_coef, b.Ts, b.ok)));
    LGR_TRY(pp_scan_flags(ctx, b.ok, b.pos, (size_t) n));
    compact_kernel<<<cdiv(n, 256), 256, 0, ctx->stream>>>(b.ok, b.pos, n, nullptr, b.list);
    int* h;
    LGR_TRY(lgr_pinned(ctx, 64, (void**) &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, b.pos + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(h + 1, b.ok + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    n_ok = h[0] + h[1];
    LGR_HIP(ctx, hipMemsetAsync(d_n_inliers, 0, (size_t) n * 4, ctx->stream));
    LGR_HIP(ctx, hipMemsetAsync(d_metric, 0, (size_t) n * 4, ctx->stream));
    if (n_ok > 0) LGR_TRY(metric_launch(ctx, b.Ts, b.list, n_ok, pk, c, p->metric_id, p->score_id, b.metric, b.ninl, nullptr, nullptr));
    // scatter back to iteration order
    std::vector<int> hl(n_ok);
    std::vector<float> hm(n_ok);
    std::vector<int> hn(n_ok), hok(n);
    if (n_ok) {
        LGR_HIP(ctx, hipMemcpyAsync(hl.data(), b.list, (size_t) n_ok * 4, hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipMemcpyAsync(hm.data(), b.metric, (size_t) n_ok * 4, hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipMemcpyAsync(hn.data(), b.ninl, (size_t) n_ok * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    LGR_HIP(ctx, hipMemcpyAsync(hok.data(), b.ok, (size_t) n * 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float> fm(n, 0.f);
    std::vector<int> fn(n, 0);
    std::vector<uint8_t> fo(n);
    for (int i = 0; i < n; ++i) fo[i] = (uint8_t) hok[i];
    for (int j = 0; j < n_ok; ++j) { fm[hl[j]] = hm[j]; fn[hl[j]] = hn[j]; }
    LGR_HIP(ctx, hipMemcpyAsync(d_metric, fm.data(), (size_t) n * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(d_n_inliers, fn.data(), (size_t) n * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(d_ok, fo.data(), (size_t) n, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(d_T16, b.Ts, (size_t) n * 64, hipMemcpyDeviceToDevice, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_ransac_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                              const lgr_params* p, lgr_result* res, uint8_t* d_final_mask) {
    return lgr_ransac_ex_dev(ctx, d_src, ns, d_tgt, nt, d_corr, c, p, nullptr, res, d_final_mask);
}

extern "C" int lgr_ransac_ex_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                                 const lgr_params* p, const lgr_metric_params* mp, lgr_result* res, uint8_t* d_final_mask) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_TRY(check_params(ctx, p));
    const bool weighted = p->metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE;
    if (weighted && mp && !mp->weights) {   // refused before any work (lgr_weights.hip repeats the check)
        LGR_CHECK(ctx, mp->weight_id >= LGR_WEIGHT_CONSTANT && mp->weight_id <= LGR_WEIGHT_NSS, LGR_ERR_INVALID_ARG);
        LGR_CHECK(ctx, mp->weight_id != LGR_WEIGHT_HARRIS && mp->weight_id != LGR_WEIGHT_TOMASI, LGR_ERR_UNSUPPORTED);
    }
    LGR_CHECK(ctx, d_src && d_tgt && (d_corr || c == 0) && res && c >= 0 && ns > 0 && nt > 0, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    auto t_start = std::chrono::steady_clock::now();
    memset(res, 0, sizeof(*res));
    for (int i = 0; i < 16; ++i) res->transformation[i] = (i % 5 == 0) ? 1.f : 0.f;
    res->n_correspondences = c;
    ctx->plane_gate[0] = ctx->plane_gate[1] = 0;
    if (c < p->n_samples) return LGR_OK;   // selectCorrespondences refuses (src/sac_prerejective_omp.cpp:36-42); identity, not converged
    uint64_t seed = p->fix_seed ? 566ull : p->seed;
    Packed pk;
    LGR_TRY(pack(ctx, d_src, ns, d_tgt, nt, d_corr, c, &pk));
    int max_iterations = std::min(comb_or_max(c, p->n_samples), p->max_iterations);
    int batch = std::max(1, p->ransac_batch);
    const bool closest = p->metric_id == LGR_METRIC_CLOSEST_PLANE || weighted;   // (the plane pairs feed the refit)
    if (!closest && p->metric_id != LGR_METRIC_COMBINATION) {
        // the loop, the final evaluation and the refit driven from the device: one host synchronisation (ransac_device_schedule)
        uint8_t* d_mask = d_final_mask;
        if (!d_mask) LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_MASK, (size_t) c + 16, &d_mask));
        const int schedule = ctx->opt.ransac_schedule == LGR_RANSAC_SCHEDULE_RESIDENT ? LGR_RANSAC_SCHEDULE_RESIDENT : LGR_RANSAC_SCHEDULE_CHAIN;
        RState S;
        LGR_TRY(ransac_device_schedule(ctx, d_src, d_tgt, d_corr, c, pk, p, seed, max_iterations, batch, schedule, nullptr, 0.f, d_mask, &S));
        fill_result(res, S, S.Tn, final_converged(S.e_ninl, S.e_metric, c, p->metric_id), S.e2_ninl, S.e2_metric);
        res->time_te = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
        return LGR_OK;
    }
    // the plane metrics: the guess's evaluation, the loop on the device-driven schedule, then a host-driven final block
    RansacMisc* M;
    LGR_TRY(ransac_misc(ctx, &M));
    float* const d_best = M->S.best_T;   // where the schedule keeps the best transform so far
    float* const d_Tn = M->S.Tn;
    lgr_plane_dev plane;
    LGR_TRY(lgr_plane_setup(ctx, d_src, ns, d_tgt, nt, seed, &plane));
    if (weighted) {
        // WeightedClosestPlaneMetricEstimator::setSourceCloud: the weights and their sum, once per run
        auto t_w = std::chrono::steady_clock::now();
        LGR_TRY(lgr_weights_prepare(ctx, d_src, ns, mp, &plane.w, &plane.w_sum, &plane.w_gate));
        if (getenv("LGR_RANSAC_DEBUG"))
            fprintf(stderr, "[lgr] weights: %.3f ms, sum %.9g, gate %.9g\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_w).count(),
                    (double) plane.w_sum, (double) plane.w_gate);
    }
    float guess_metric = 0.f;
    if (p->has_guess) {
        // src/sac_prerejective_omp.cpp:134-147: the guess is the hypothesis to beat (final_tn / final_metric).  Its inliers only seed
        // the global largest_inlier_set, which the loop never reads (thread-local sets start empty, :177): the bound is unaffected.
        // (the schedule starts from the same transform: it uploads its RState with best_T = the guess)
        LGR_HIP(ctx, hipMemcpyAsync(d_best, p->guess, 64, hipMemcpyHostToDevice, ctx->stream));
        uint8_t* d_gm;
        LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_MASK, (size_t) c + 16, &d_gm));
        EvalOut eg;
        LGR_TRY(evaluate_one_plane(ctx, d_best, pk, c, p->metric_id, p->score_id, d_gm, plane, 0xFFFFFFFDu, &eg, nullptr));
        guess_metric = eg.metric;
    }
    // A round evaluates up to MAX_ROUND_BATCHES batches -- the sparse subset of a hypothesis is keyed by its ITERATION (Philox counter =
    // round_first + offset), so it does not matter which round or batch evaluates it; the gate uses the loop's state at the start of the
    // round (a looser gate than batch by batch: it still only abandons what can be neither the best nor a record).
    RState loop;
    LGR_TRY(ransac_device_schedule(ctx, d_src, d_tgt, d_corr, c, pk, p, seed, max_iterations, batch, LGR_RANSAC_SCHEDULE_CHAIN, &plane, guess_metric, nullptr, &loop));
    ctx->plane_gate[0] = (unsigned) (closest ? loop.tot_ok : loop.tot_cand);   // closest_plane scores every survivor on its subset, combination the candidates
    ctx->plane_gate[1] = (unsigned) loop.n_gated;
    // :265-296 final re-estimation
    uint8_t* d_mask = d_final_mask;
    if (!d_mask) LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_MASK, (size_t) c + 16, &d_mask));
    EvalOut e;
    std::vector<int2> plane_pairs;
    LGR_TRY(evaluate_one_plane(ctx, d_best, pk, c, p->metric_id, p->score_id, d_mask, plane, 0xFFFFFFFEu, &e, closest ? &plane_pairs : nullptr));
    const bool converged = final_converged(e.n_inl, e.metric, c, p->metric_id);
    if (closest) {
        // estimateOptimalRigidTransformation over the plane pairs (source point, nearest target point), ascending source index
        const int np = (int) plane_pairs.size();
        Packed pp;
        float4* P;
        LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_LIST, (size_t) 3 * std::max(np, 1) + 4, &P));
        pp.P0 = P; pp.P1 = P + std::max(np, 1); pp.sstar = nullptr; pp.PP = nullptr; pp.pstats = nullptr;
        int2* d_pairs = (int2*) (P + 2 * (size_t) std::max(np, 1));
        if (np) {
            LGR_HIP(ctx, hipMemcpyAsync(d_pairs, plane_pairs.data(), (size_t) np * 8, hipMemcpyHostToDevice, ctx->stream));
            plane_pack_kernel<<<cdiv(np, 256), 256, 0, ctx->stream>>>(d_src, d_tgt, d_pairs, np, pp.P0, pp.P1);
            LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        LGR_TRY(refit_launch(ctx, pp, np, nullptr, d_Tn));
    } else {
        LGR_TRY(refit_launch(ctx, pk, c, d_mask, d_Tn));
    }
    EvalOut e2;
    LGR_TRY(evaluate_one_plane(ctx, d_Tn, pk, c, p->metric_id, p->score_id, d_mask, plane, 0xFFFFFFFFu, &e2, nullptr));
    float* hT;
    LGR_TRY(lgr_pinned(ctx, 64, (void**) &hT));
    LGR_HIP(ctx, hipMemcpyAsync(hT, d_Tn, 64, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fill_result(res, loop, hT, converged, e2.n_inl, e2.metric);
    res->time_te = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    return LGR_OK;
}

// lgr.h: hypotheses of the last RANSAC call that were scored on a sparse plane subset, and how many of them the gate of plane_kernel abandoned
extern "C" int lgr_ransac_last_plane_gate(lgr_ctx* ctx, unsigned* out2) {
    if (!ctx || !out2) return LGR_ERR_INVALID_ARG;
    out2[0] = ctx->plane_gate[0]; out2[1] = ctx->plane_gate[1];
    return LGR_OK;
}

extern "C" int lgr_ransac(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                          const lgr_params* p, lgr_result* res, uint8_t* final_mask) {
    return lgr_ransac_ex(ctx, src, ns, tgt, nt, corr, c, p, nullptr, res, final_mask);
}

extern "C" int lgr_ransac_ex(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                             const lgr_params* p, const lgr_metric_params* mp, lgr_result* res, uint8_t* final_mask) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, src && tgt && (corr || c == 0) && res && ns > 0 && nt > 0 && c >= 0, LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_corr* dc;
    uint8_t* dm;
    lgr_metric_params mpd;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    LGR_TRY(hc.out((size_t) c, &dm, LGR_PAD_MASK));
    LGR_TRY(hc.weights(ns, &mp, &mpd));
    LGR_TRY(lgr_ransac_ex_dev(ctx, ds, ns, dt, nt, dc, c, p, mp, res, dm));
    if (final_mask && c >= p->n_samples) {
        LGR_TRY(hc.fetch(final_mask, dm, (size_t) c));
        LGR_TRY(hc.finish());
    } else if (final_mask && c > 0) memset(final_mask, 0, c);
    return LGR_OK;
}

extern "C" int lgr_refit_svd_dev(lgr_ctx* ctx, const float* d_src, const float* d_tgt, const lgr_corr* d_corr, int c,
                                 const uint8_t* d_mask, float T16[16]) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, d_src && d_tgt && (d_corr || c == 0) && T16 && c >= 0, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    float4* P;
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_PACK, (size_t) c * 2 + (size_t) (c + 3) / 4 + 4, &P));
    Packed pk{P, P + c, (float*) (P + 2 * (size_t) c), nullptr, nullptr};
    if (c > 0) pack_kernel<<<cdiv(c, 256), 256, 0, ctx->stream>>>(d_src, d_tgt, d_corr, c, nullptr, pk.P0, pk.P1, pk.sstar, nullptr, nullptr, c);
    RansacMisc* M;
    LGR_TRY(ransac_misc(ctx, &M));
    float* dT = M->T;
    LGR_TRY(refit_launch(ctx, pk, c, d_mask, dT));
    float* hT;
    LGR_TRY(lgr_pinned(ctx, 64, (void**) &hT));
    LGR_HIP(ctx, hipMemcpyAsync(hT, dT, 64, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(T16, hT, 64);
    return LGR_OK;
}

extern "C" int lgr_refit_svd(lgr_ctx* ctx, const float* src, const float* tgt, int ns, int nt, const lgr_corr* inliers, int n, float T16[16]) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, src && tgt && (inliers || n == 0) && T16 && ns > 0 && nt > 0 && n >= 0, LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_corr* dc;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(inliers, (size_t) n, &dc));
    LGR_TRY(lgr_check_corr(ctx, dc, n, ns, nt));   // the _dev form mirrors estimateOptimalRigidTransformation(src, tgt, inliers, T) and has no sizes to check against
    return lgr_refit_svd_dev(ctx, ds, dt, dc, n, nullptr, T16);
}

// src/hypotheses.cpp:50-129 chooseBestHypothesis (compiled out in the reference like updateHypotheses): the decision --
// the hypothesis whose correspondence inliers are spread most uniformly (strict >, identity when none is positive).  The
// hypotheses.csv side output of the reference (inlier / overlap areas) is not produced.
extern "C" int lgr_choose_best_hypothesis_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                                              const float* tns16, int n, float T_out16[16], int* best_index, float* uniformities) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, d_src && d_tgt && (d_corr || c == 0) && (tns16 || n == 0) && T_out16 && n >= 0 && c >= 0 && ns > 0 && nt > 0, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < 16; ++i) T_out16[i] = (i % 5 == 0) ? 1.f : 0.f;
    int best_i = -1;
    float best = 0.f;
    if (n > 0) {
        Packed pk;
        LGR_TRY(pack(ctx, d_src, ns, d_tgt, nt, d_corr, c, &pk));
        float* dT;
        LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_T, (size_t) n * 16, &dT));
        LGR_HIP(ctx, hipMemcpyAsync(dT, tns16, (size_t) n * 64, hipMemcpyHostToDevice, ctx->stream));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < n; ++i) {
            EvalOut e{0, 0.f, 0.f};
            if (c > 0) LGR_TRY(evaluate_one(ctx, dT + (size_t) i * 16, pk, c, LGR_METRIC_UNIFORMITY, LGR_SCORE_MSE, nullptr, &e));
            if (uniformities) uniformities[i] = e.metric;
            if (e.metric > best) { best = e.metric; best_i = i; memcpy(T_out16, tns16 + (size_t) i * 16, 64); }
        }
    }
    if (best_index) *best_index = best_i;
    return LGR_OK;
}

extern "C" int lgr_choose_best_hypothesis(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                                          const float* tns16, int n, float T_out16[16], int* best_index, float* uniformities) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, src && tgt && (corr || c == 0) && (tns16 || n == 0) && T_out16 && n >= 0 && c >= 0 && ns > 0 && nt > 0, LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_corr* dc;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    return lgr_choose_best_hypothesis_dev(ctx, ds, ns, dt, nt, dc, c, tns16, n, T_out16, best_index, uniformities);
}

// The scratch of the single-transform evaluations under a plane metric that stay on the device (the hypothesis set's guess and final
// blocks): a slot of its own, WS_PLANE_OUT being the loop's at another size (loop_buffers).
struct PlaneScratch {
    int* pl;            // the plane test's outputs: inlier count, metric, rmse, number of pairs
    float* guess;       // the guess's evaluation record (metric, inliers, rmse) and a word that stays 0
    int2* pairs;        // the plane pairs in arrival order, n_sp
    float4 *P0, *P1;    // ... and their points in ascending source index, n_sp each
};
static int plane_scratch(lgr_ctx* ctx, const lgr_plane_dev& plane, PlaneScratch* s) {
    const size_t n1 = (size_t) std::max(plane.n_sp, 1);
    float4* base;
    LGR_TRY(lgr_ws_t(ctx, WS_HYP_PLANE, 2 + (n1 + 1) / 2 + 2 * n1, &base));
    s->pl = (int*) base; s->guess = (float*) (base + 1); s->pairs = (int2*) (base + 2);
    s->P0 = base + 2 + (n1 + 1) / 2; s->P1 = s->P0 + n1;
    return LGR_OK;
}
// evaluate_one_plane without a read-back: (metric, n_inl bits, rmse) -> d_out3; the plane pairs stay in s.pairs, their number in s.pl[3]
static int evaluate_one_plane_dev(lgr_ctx* ctx, const float* d_T, const Packed& pk, int c, int metric_id, int score_id, uint8_t* d_mask,
                                  const lgr_plane_dev& plane, unsigned counter, bool want_pairs, const PlaneScratch& s, float* d_scratch3, float* d_out3) {
    LGR_TRY(lgr_plane_eval(ctx, plane, d_T, nullptr, 1, counter, score_id, s.pl, (float*) (s.pl + 1), (float*) (s.pl + 2), want_pairs ? s.pairs : nullptr, s.pl + 3));
    const bool combination = metric_id == LGR_METRIC_COMBINATION;
    if (combination) LGR_TRY(evaluate_one_dev(ctx, d_T, pk, c, LGR_METRIC_CORRESPONDENCES, LGR_SCORE_CONSTANT, d_mask, d_scratch3, d_out3));
    mh_plane_store_kernel<<<1, 64, 0, ctx->stream>>>(s.pl, d_out3, combination ? 1 : 0);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// the set of distinct hypotheses: the loop, then a second pass over its iterations (the mh_* kernels, lgr_ransac_schedule.cuh) and the fold
static int ransac_multi_impl(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                             const lgr_params* p, const lgr_metric_params* mp, int max_set, lgr_result* res, lgr_hypothesis* out, int* n_out,
                             int* best_index) {
    const bool weighted = p->metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE;
    if (weighted && mp && !mp->weights) {   // refused before any work, as lgr_ransac_ex_dev does
        LGR_CHECK(ctx, mp->weight_id >= LGR_WEIGHT_CONSTANT && mp->weight_id <= LGR_WEIGHT_NSS, LGR_ERR_INVALID_ARG);
        LGR_CHECK(ctx, mp->weight_id != LGR_WEIGHT_HARRIS && mp->weight_id != LGR_WEIGHT_TOMASI, LGR_ERR_UNSUPPORTED);
    }
    LGR_CHECK(ctx, p->alignment_id == LGR_ALIGN_RANSAC, LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, max_set >= 1 && max_set <= LGR_HYPOTHESES_MAX, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, d_src && d_tgt && (d_corr || c == 0) && res && out && n_out && best_index && c >= 0 && ns > 0 && nt > 0, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    auto t_start = std::chrono::steady_clock::now();
    memset(res, 0, sizeof(*res));
    for (int i = 0; i < 16; ++i) res->transformation[i] = (i % 5 == 0) ? 1.f : 0.f;
    res->n_correspondences = c;
    *n_out = 0; *best_index = -1;
    if (c < p->n_samples) return LGR_OK;   // selectCorrespondences refuses (src/sac_prerejective_omp.cpp:36-42); identity, empty set
    const uint64_t seed = p->fix_seed ? 566ull : p->seed;
    Packed pk;
    LGR_TRY(pack(ctx, d_src, ns, d_tgt, nt, d_corr, c, &pk));
    const int max_iterations = std::min(comb_or_max(c, p->n_samples), p->max_iterations);
    const int batch = std::max(1, p->ransac_batch);
    uint8_t* d_mask;
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_MASK, (size_t) c + 16, &d_mask));
    RansacMisc* M;
    LGR_TRY(ransac_misc(ctx, &M));
    const bool closest = p->metric_id == LGR_METRIC_CLOSEST_PLANE || weighted;   // (the plane pairs feed the refit)
    const bool planar = closest || p->metric_id == LGR_METRIC_COMBINATION;
    lgr_plane_dev plane;
    PlaneScratch ps{};
    // the hypothesis set is always built on the launch chain (as the plane metrics are); the loop's final block is enqueued and unused
    RState loop;
    if (planar) {
        // as lgr_ransac_ex_dev: the estimator's set-up, the guess's evaluation (it is the metric to beat, and the first item below), the loop
        ctx->plane_gate[0] = ctx->plane_gate[1] = 0;
        LGR_TRY(lgr_plane_setup(ctx, d_src, ns, d_tgt, nt, seed, &plane));
        if (weighted) LGR_TRY(lgr_weights_prepare(ctx, d_src, ns, mp, &plane.w, &plane.w_sum, &plane.w_gate));
        LGR_TRY(plane_scratch(ctx, plane, &ps));
        LGR_HIP(ctx, hipMemsetAsync(ps.pl, 0, 32, ctx->stream));
        float guess_metric = 0.f;
        if (p->has_guess) {
            LGR_HIP(ctx, hipMemcpyAsync(M->T, p->guess, 64, hipMemcpyHostToDevice, ctx->stream));
            LGR_TRY(evaluate_one_plane_dev(ctx, M->T, pk, c, p->metric_id, p->score_id, d_mask, plane, 0xFFFFFFFDu, false, ps, M->ev, ps.guess));
            float* hg;
            LGR_TRY(lgr_pinned(ctx, 64, (void**) &hg));
            LGR_HIP(ctx, hipMemcpyAsync(hg, ps.guess, 4, hipMemcpyDeviceToHost, ctx->stream));
            LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
            guess_metric = hg[0];
        }
        LGR_TRY(ransac_device_schedule(ctx, d_src, d_tgt, d_corr, c, pk, p, seed, max_iterations, batch, LGR_RANSAC_SCHEDULE_CHAIN, &plane, guess_metric, nullptr, &loop));
        ctx->plane_gate[0] = (unsigned) (closest ? loop.tot_ok : loop.tot_cand);   // the loop's numbers: the second pass is ungated and adds nothing
        ctx->plane_gate[1] = (unsigned) loop.n_gated;
    } else {
        LGR_TRY(ransac_device_schedule(ctx, d_src, d_tgt, d_corr, c, pk, p, seed, max_iterations, batch, LGR_RANSAC_SCHEDULE_CHAIN, nullptr, 0.f, d_mask, &loop));
    }
    fill_result(res, loop, nullptr, false, 0, 0.f);
    const int iterations = loop.done;
    const float m_star = loop.final_metric;

    // ---- second pass: the loop's own working set, the items of a round, the set
    LoopBuffers L;
    LGR_TRY(loop_buffers(ctx, p, c, max_iterations, batch, planar ? &plane : nullptr, &L));
    const BatchBuffers& b = L.b;
    const int nb_max = L.nb_max;
    RState* const dS = L.dS;
    float* item_T;
    LGR_TRY(lgr_ws_t(ctx, WS_HYP_ITEMS, (size_t) nb_max * 19 + 16, &item_T));
    float* item_m = item_T + (size_t) nb_max * 16;
    int32_t* item_it = (int32_t*) (item_m + nb_max);
    int* kslot = item_it + nb_max;
    int* d_n_items = kslot + nb_max;
    lgr_fold_set set;
    LGR_TRY(lgr_fold_begin(ctx, max_set, &set));
    if (p->has_guess && planar) {
        // :139-143 the guess is the first item, with the metric of its evaluation in front of the loop (counter 0xFFFFFFFD), no inlier gate
        LGR_TRY(lgr_fold_launch(ctx, set, M->T, ps.guess, nullptr, -1, 1, nullptr, p->distance_thr));
    } else if (p->has_guess) {
        // :139-143 the guess is the first item: the metric `evaluate` gives it, no inlier gate
        LGR_HIP(ctx, hipMemcpyAsync(M->T, p->guess, 64, hipMemcpyHostToDevice, ctx->stream));
        LGR_TRY(evaluate_one_dev(ctx, M->T, pk, c, p->metric_id, p->score_id, d_mask, L.d_ev, L.d_ev + 4));
        LGR_TRY(lgr_fold_launch(ctx, set, M->T, L.d_ev + 4, nullptr, -1, 1, nullptr, p->distance_thr));
    }
    const float gate_metric = (float) (0.1 * (double) m_star);   // (rs_gate_dev's own margin is four orders of magnitude above this rounding)
    for (int first = 0; first < iterations; first += nb_max) {
        const int nb = std::min(nb_max, iterations - first);
        mh_begin_kernel<<<1, 64, 0, ctx->stream>>>(dS, first, nb, gate_metric, p->metric_id, c);
        LGR_HIP(ctx, hipMemsetAsync(kslot, 0xff, (size_t) nb * 4, ctx->stream));
        LGR_TRY(enqueue_round_front(ctx, L, pk, c, p, seed, nb, planar ? &plane : nullptr, false));
        mh_keep_kernel<<<64, 256, 0, ctx->stream>>>(dS, b.list2, b.metric, m_star, kslot);
        mh_order_kernel<<<1, 1024, 0, ctx->stream>>>(dS, kslot, b.Ts, b.metric, item_T, item_m, item_it, d_n_items);
        LGR_HIP(ctx, hipGetLastError());
        LGR_TRY(lgr_fold_launch(ctx, set, item_T, item_m, item_it, 0, nb, d_n_items, p->distance_thr));
    }
    // ---- the set -> host
    const size_t set_bytes = sizeof(lgr_fold_state) + (size_t) max_set * 14 * 4;
    char* hs;
    LGR_TRY(lgr_pinned(ctx, 64 + set_bytes, (void**) &hs));
    LGR_HIP(ctx, hipMemcpyAsync(hs, set.state, sizeof(lgr_fold_state), hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(hs + 64, set.rt, (size_t) max_set * 14 * 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const lgr_fold_state fs = *(const lgr_fold_state*) hs;
    if (fs.overflow) return lgr_fail(ctx, LGR_ERR_UNSUPPORTED, "the set of hypotheses outgrew max_set during the fold (a truncated set is never returned)", __FILE__, __LINE__);
    const int n_set = fs.n;
    {
        const float* rt = (const float*) (hs + 64);
        const float* sm = rt + (size_t) 12 * max_set;
        const int32_t* si = (const int32_t*) (sm + max_set);
        for (int k = 0; k < n_set; ++k) {
            lgr_hypothesis& h = out[k];
            memset(&h, 0, sizeof(h));
            h.iteration = si[k]; h.loop_metric = sm[k];
            if (si[k] < 0) memcpy(h.loop_transformation, p->guess, 64);
            else {
                for (int col = 0; col < 4; ++col)
                    for (int r = 0; r < 3; ++r) h.loop_transformation[4 * col + r] = rt[(size_t) k * 12 + 3 * col + r];
                h.loop_transformation[15] = 1.f;   // (umeyama_n's fourth row)
            }
        }
    }
    // ---- :270-291 the final block per member, enqueued blind; then chooseBestHypothesis' criterion of the refit (:293)
    float* fin;
    LGR_TRY(lgr_ws_t(ctx, WS_HYP_FINAL, (size_t) std::max(n_set, 1) * 44, &fin));
    float* d_loopT = fin + (size_t) std::max(n_set, 1) * 12;
    float* d_Tn = d_loopT + (size_t) std::max(n_set, 1) * 16;
    for (int k = 0; k < n_set; ++k) {
        LGR_HIP(ctx, hipMemcpyAsync(d_loopT + (size_t) k * 16, out[k].loop_transformation, 64, hipMemcpyHostToDevice, ctx->stream));
        float* f = fin + (size_t) k * 12;
        float* Tn = d_Tn + (size_t) k * 16;
        if (planar) {
            // evaluation under counter 0xFFFFFFFE, refit, evaluation under 0xFFFFFFFF, as lgr_ransac_ex_dev's final block -- without its host
            const float* Tl = d_loopT + (size_t) k * 16;
            LGR_TRY(evaluate_one_plane_dev(ctx, Tl, pk, c, p->metric_id, p->score_id, d_mask, plane, 0xFFFFFFFEu, closest, ps, L.d_ev, f));
            if (closest) {
                // estimateOptimalRigidTransformation over the plane pairs in ascending source index, their number read on the device
                mh_plane_rank_pack_kernel<<<std::max(1, cdiv(plane.n_sp, 256)), 256, 0, ctx->stream>>>(d_src, d_tgt, ps.pairs, ps.pl + 3, ps.P0, ps.P1);
                refit_kernel<<<1, 256, 0, ctx->stream>>>(ps.P0, ps.P1, 0, Tn, ps.pl + 3, (const int*) (ps.guess + 3));
                LGR_HIP(ctx, hipGetLastError());
            } else {
                LGR_TRY(refit_launch(ctx, pk, c, d_mask, Tn));
            }
            LGR_TRY(evaluate_one_plane_dev(ctx, Tn, pk, c, p->metric_id, p->score_id, d_mask, plane, 0xFFFFFFFFu, false, ps, L.d_ev, f + 4));
        } else {
            LGR_TRY(enqueue_final_block(ctx, pk, c, p, d_loopT + (size_t) k * 16, d_mask, Tn, f, f + 4));
        }
        LGR_TRY(evaluate_one_dev(ctx, Tn, pk, c, LGR_METRIC_UNIFORMITY, LGR_SCORE_MSE, d_mask, L.d_ev, f + 8));
    }
    if (n_set) {
        std::vector<float> hf((size_t) n_set * 12), hT((size_t) n_set * 16);
        LGR_HIP(ctx, hipMemcpyAsync(hf.data(), fin, hf.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipMemcpyAsync(hT.data(), d_Tn, hT.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        float best = 0.f;
        for (int k = 0; k < n_set; ++k) {
            lgr_hypothesis& h = out[k];
            const float* f = hf.data() + (size_t) k * 12;
            int e_ninl, e2_ninl;
            memcpy(&e_ninl, &f[1], 4); memcpy(&e2_ninl, &f[5], 4);
            memcpy(h.transformation, hT.data() + (size_t) k * 16, 64);
            h.converged = final_converged(e_ninl, f[0], c, p->metric_id) ? 1 : 0;
            h.metric = f[4]; h.n_inliers = e2_ninl; h.uniformity = f[8];
            if (h.converged) res->converged = 1;
            if (h.uniformity > best) { best = h.uniformity; *best_index = k; }   // src/hypotheses.cpp:50-129: strict >, none positive -> identity
        }
        if (*best_index >= 0) {
            const lgr_hypothesis& h = out[*best_index];
            memcpy(res->transformation, h.transformation, 64);
            res->n_inliers = h.n_inliers; res->metric = h.metric;
        }
    }
    *n_out = n_set;
    res->time_te = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    return LGR_OK;
}

// the two metrics lgr_ransac_multi* has always taken; the _ex entries take all five
extern "C" int lgr_ransac_multi_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                                    const lgr_params* p, int max_set, lgr_result* res, lgr_hypothesis* out, int* n_out, int* best_index) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_TRY(check_params(ctx, p));
    LGR_CHECK(ctx, p->metric_id == LGR_METRIC_UNIFORMITY || p->metric_id == LGR_METRIC_CORRESPONDENCES, LGR_ERR_UNSUPPORTED);
    return ransac_multi_impl(ctx, d_src, ns, d_tgt, nt, d_corr, c, p, nullptr, max_set, res, out, n_out, best_index);
}
extern "C" int lgr_ransac_multi_ex_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                                       const lgr_params* p, const lgr_metric_params* mp, int max_set, lgr_result* res, lgr_hypothesis* out, int* n_out,
                                       int* best_index) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_TRY(check_params(ctx, p));
    return ransac_multi_impl(ctx, d_src, ns, d_tgt, nt, d_corr, c, p, mp, max_set, res, out, n_out, best_index);
}

extern "C" int lgr_ransac_multi(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                                const lgr_params* p, int max_set, lgr_result* res, lgr_hypothesis* out, int* n_out, int* best_index) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, max_set >= 1 && max_set <= LGR_HYPOTHESES_MAX, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, src && tgt && (corr || c == 0) && res && ns > 0 && nt > 0 && c >= 0, LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_corr* dc;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    return lgr_ransac_multi_dev(ctx, ds, ns, dt, nt, dc, c, p, max_set, res, out, n_out, best_index);
}
extern "C" int lgr_ransac_multi_ex(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                                   const lgr_params* p, const lgr_metric_params* mp, int max_set, lgr_result* res, lgr_hypothesis* out, int* n_out,
                                   int* best_index) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, max_set >= 1 && max_set <= LGR_HYPOTHESES_MAX, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, src && tgt && (corr || c == 0) && res && ns > 0 && nt > 0 && c >= 0, LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_corr* dc;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    lgr_metric_params mpd;
    LGR_TRY(hc.weights(ns, &mp, &mpd));
    return lgr_ransac_multi_ex_dev(ctx, ds, ns, dt, nt, dc, c, p, mp, max_set, res, out, n_out, best_index);
}
