// lgr_plane_dense.hip -- the closest-plane metric over EVERY source point, and the analysis layer's metric figures, for gfx950.
//
// Replaces ClosestPlaneMetricEstimator / WeightedClosestPlaneMetricEstimator::buildInliersAndEstimateMetric with sparse = false
// (reference src/metric.cpp:10-53, :55-81, :181-231), the form AlignmentAnalysis::start evaluates a finished alignment with
// (src/analysis.cpp:211, :223) and estimateTestMetric writes into metrics.csv (src/main.cpp:41-116): a serial loop over the source cloud
// with one kd-tree radius search per point there.  Here one thread per source point walks the 27 cells of a uniform grid over the target
// (lgr_grid.cuh, cell = 1.001 x radius) and writes its terms; the two float sums are then taken in the reference's loop order.
//
// Declared orders (shared with the CPU statement tests/cpp/plane_dense_ref.cpp).  The per-point rules -- move, nearest
// target, plane distance, inlier test, value -- are lgr_plane_point.cuh's, shared with plane_kernel (lgr_plane.hip).  This file's own:
//   * score and the squared-error sum are SEQUENTIAL f32 sums in ascending source index -- the reference's loop -- not the sparse
//     kernel's 2^-32 fixed-point sums.  Every point writes its two terms to a buffer first, a point that is no inlier writes +0: a
//     running f32 sum that started at +0 is never -0 (x + (-x) and (+0) + (-0) both round to +0), and adding +0 to anything but -0
//     returns it unchanged, whatever the signs of the other terms -- so the sum over all points is the sum over the inliers;
//   * rmse and metric are lgr_plane_figures (lgr_internal.h) with the denominator (float) ns, with weights weights_sum;
//   * the inlier list is {source index, nearest target index, dist, threshold} in ascending source index (flags -> exclusive scan).
#include <algorithm>

#include "lgr_grid.cuh"
#include "lgr_host.h"
#include "lgr_internal.h"
#include "lgr_math.cuh"
#include "lgr_plane_point.cuh"
#include "lgr_pointpass.cuh"

namespace {

struct PdT { float m[16]; };   // the transform, column-major, as a kernel argument

// pass 1: thread i handles source point i (plane_dense_point) and writes its nearest target, distance, terms and flag
template <bool W>
__global__ __launch_bounds__(PP_BLOCK) void plane_dense_kernel(GridDev g, const float4* __restrict__ src, int ns, PdT T, float thr, float r2, int score_id,
                                                              const float* __restrict__ w, int32_t* __restrict__ nn_out, float* __restrict__ dist_out,
                                                              float* __restrict__ term_val, float* __restrict__ term_sq, int* __restrict__ flags,
                                                              int* __restrict__ counter) {
    const int i = blockIdx.x * PP_BLOCK + threadIdx.x;
    bool inl = false;
    if (i < ns) {
        const PlanePoint p = plane_dense_point<W>(g, src[(size_t) i * 3], T.m, thr, r2, score_id, w, i);
        inl = p.inl;
        nn_out[i] = p.j;
        dist_out[i] = p.dist;
        term_val[i] = p.value;
        term_sq[i] = p.sq;
        flags[i] = inl ? 1 : 0;
    }
    wave_count(inl, counter);
}

__global__ __launch_bounds__(PP_BLOCK) void plane_dense_compact_kernel(const int* __restrict__ flags, const int* __restrict__ pos, const int32_t* __restrict__ nn,
                                                                      const float* __restrict__ dist, int ns, float thr, lgr_corr* __restrict__ out) {
    const int i = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (i >= ns || !flags[i]) return;
    out[pos[i]] = lgr_corr{i, nn[i], dist[i], thr};   // pos[i] < number of inliers <= ns
}

// everything between the argument checks and the final synchronisation of lgr_evaluate_plane_dense_dev
int dense_eval(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float* T16, int score_id, const lgr_metric_params* mp,
               float inlier_threshold, lgr_plane_dense_eval* out, lgr_corr* d_inliers, int32_t* d_nn) {
    const float* d_w = nullptr;
    float w_sum = 0.f, w_gate = 0.f;
    if (mp) LGR_TRY(lgr_weights_prepare(ctx, d_src, ns, mp, &d_w, &w_sum, &w_gate));   // harris / tomasi: LGR_ERR_UNSUPPORTED
    lgr_plane_target pt;
    LGR_TRY(lgr_plane_target_setup(ctx, d_tgt, nt, inlier_threshold, 2e18f, &pt));
    const float thr = pt.thr, radius = pt.radius;
    const GridDev& g = pt.g;
    const size_t nn = ((size_t) ns + 63) & ~(size_t) 63;
    int32_t* buf;
    char* misc;
    LGR_TRY(lgr_ws_t(ctx, WS_PD_TERMS, 6 * nn + 16, &buf));
    LGR_TRY(lgr_ws_t(ctx, WS_PD_MISC, 64, &misc));
    int32_t* nn_idx = d_nn ? d_nn : buf;
    float *dist = (float*) (buf + nn), *val = (float*) (buf + 2 * nn), *sq = (float*) (buf + 3 * nn);
    int *flags = buf + 4 * nn, *pos = buf + 5 * nn;
    int* counter = (int*) misc;          // [0] inliers
    float* sums = (float*) (misc + 16);  // [0] score, [1] squared distances
    LGR_HIP(ctx, hipMemsetAsync(misc, 0, 64, ctx->stream));
    PdT T;
    memcpy(T.m, T16, 64);
    if (d_w)
        plane_dense_kernel<true><<<cdiv(ns, PP_BLOCK), PP_BLOCK, 0, ctx->stream>>>(g, (const float4*) d_src, ns, T, thr, radius * radius, score_id, d_w, nn_idx, dist,
                                                                                  val, sq, flags, counter);
    else
        plane_dense_kernel<false><<<cdiv(ns, PP_BLOCK), PP_BLOCK, 0, ctx->stream>>>(g, (const float4*) d_src, ns, T, thr, radius * radius, score_id, nullptr, nn_idx,
                                                                                   dist, val, sq, flags, counter);
    GtSumJobs jobs{};
    jobs.p[0] = val; jobs.n[0] = ns; jobs.p[1] = sq; jobs.n[1] = ns;
    gt_seqsum_kernel<<<2, PP_BLOCK, 0, ctx->stream>>>(jobs, sums);
    LGR_HIP(ctx, hipGetLastError());
    if (d_inliers) {
        LGR_TRY(pp_scan_flags(ctx, flags, pos, (size_t) ns));
        plane_dense_compact_kernel<<<cdiv(ns, PP_BLOCK), PP_BLOCK, 0, ctx->stream>>>(flags, pos, nn_idx, dist, ns, thr, d_inliers);
        LGR_HIP(ctx, hipGetLastError());
    }
    char* h;
    LGR_TRY(lgr_pinned(ctx, 64, (void**) &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, misc, 32, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int n_inl;
    float s2[2];
    memcpy(&n_inl, h, 4);
    memcpy(s2, h + 16, 8);
    memset(out, 0, sizeof *out);
    out->n_inliers = n_inl;
    out->threshold = thr;
    out->score = s2[0];
    lgr_plane_figures(s2[0], s2[1], n_inl, d_w ? w_sum : (float) ns, &out->rmse, &out->metric);
    return LGR_OK;
}

}  // namespace

extern "C" int lgr_evaluate_plane_dense_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16], int score_id,
                                            const lgr_metric_params* mp, float inlier_threshold, lgr_plane_dense_eval* out, lgr_corr* d_inliers,
                                            int32_t* d_nn) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, d_src && d_tgt && T16 && out && ns > 0 && nt > 1 && score_id >= 0 && score_id <= 3 && aligned16(d_src) && aligned16(d_tgt), LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, !(inlier_threshold != inlier_threshold) && inlier_threshold <= 1e18f, LGR_ERR_INVALID_ARG);   // the squared radius stays finite
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    LGR_TRY(dense_eval(ctx, d_src, ns, d_tgt, nt, T16, score_id, mp, inlier_threshold, out, d_inliers, d_nn));
    return LGR_OK;
}

extern "C" int lgr_analysis_metric_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c, const float T16[16],
                                       const float* Tgt16, int metric_id, int score_id, const lgr_metric_params* mp, lgr_metric_eval* out,
                                       uint8_t* d_inlier_mask, lgr_corr* d_inliers) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, out && T16 && c >= 0 && (d_corr || c == 0) && metric_id >= LGR_METRIC_CORRESPONDENCES && metric_id <= LGR_METRIC_WEIGHTED_CLOSEST_PLANE,
              LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    memset(out, 0, sizeof *out);
    const bool plane = metric_id == LGR_METRIC_CLOSEST_PLANE || metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE;
    int n3[3] = {0, 0, 0};
    if (plane) {
        // the inliers ARE correspondences {source, nearest target, dist, threshold}: buildCorrectInliers is buildCorrectCorrespondences over them
        lgr_metric_params def;
        lgr_default_metric_params(&def);
        const lgr_metric_params* use = metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE ? (mp ? mp : &def) : nullptr;
        LGR_CHECK(ctx, ns > 0, LGR_ERR_INVALID_ARG);
        lgr_corr* d_inl = d_inliers;
        if (!d_inl) LGR_TRY(lgr_ws_t(ctx, WS_PD_INLIERS, (size_t) ns + 1, &d_inl));
        lgr_plane_dense_eval e;
        LGR_TRY(lgr_evaluate_plane_dense_dev(ctx, d_src, ns, d_tgt, nt, T16, score_id, use, 0.f, &e, d_inl, nullptr));
        out->metric = e.metric; out->rmse = e.rmse; out->n_inliers = e.n_inliers;
        if (Tgt16 && e.n_inliers > 0) {
            LGR_TRY(lgr_correct_correspondences_dev(ctx, d_src, ns, d_tgt, nt, d_inl, e.n_inliers, Tgt16, nullptr, nullptr, n3));
            out->n_correct_inliers = n3[0];
        }
        return LGR_OK;
    }
    // correspondences, uniformity and the correspondence half of combination (its own estimator: constant score, src/metric.cpp:233-250)
    const bool comb = metric_id == LGR_METRIC_COMBINATION;
    uint8_t* d_mask = d_inlier_mask;
    if (!d_mask) LGR_TRY(lgr_ws_t(ctx, WS_PD_MASK, (size_t) c + 16, &d_mask));
    LGR_TRY(lgr_evaluate_dev(ctx, d_src, ns, d_tgt, nt, d_corr, c, T16, comb ? (int) LGR_METRIC_CORRESPONDENCES : metric_id,
                             comb ? (int) LGR_SCORE_CONSTANT : score_id, d_mask, &out->n_inliers, &out->rmse, &out->metric));
    if (comb) {
        lgr_plane_dense_eval e;
        LGR_TRY(lgr_evaluate_plane_dense_dev(ctx, d_src, ns, d_tgt, nt, T16, score_id, nullptr, 0.f, &e, nullptr, nullptr));
        out->metric = out->metric * e.metric;   // metric = metric_cs * metric_cp
    }
    if (Tgt16 && c > 0) {
        LGR_TRY(lgr_correct_correspondences_dev(ctx, d_src, ns, d_tgt, nt, d_corr, c, Tgt16, d_mask, nullptr, n3));
        out->n_correct_inliers = n3[1];
    }
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_evaluate_plane_dense(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float T16[16], int score_id,
                                        const lgr_metric_params* mp, float inlier_threshold, lgr_plane_dense_eval* out, lgr_corr* inliers, int32_t* nn) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, src && tgt && out && ns > 0 && nt > 1, LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_corr* di = nullptr;
    int32_t* dn = nullptr;
    lgr_metric_params staged;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.weights(ns, &mp, &staged));
    if (inliers) LGR_TRY(hc.out((size_t) ns, &di));
    if (nn) LGR_TRY(hc.out((size_t) ns, &dn, 4));   // (slack kept from before; no reader past ns is known)
    LGR_TRY(lgr_evaluate_plane_dense_dev(ctx, ds, ns, dt, nt, T16, score_id, mp, inlier_threshold, out, di, dn));
    LGR_TRY(hc.fetch(inliers, di, (size_t) out->n_inliers));
    LGR_TRY(hc.fetch(nn, dn, (size_t) ns));
    return hc.finish();
}

extern "C" int lgr_analysis_metric(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c, const float T16[16],
                                   const float* Tgt16, int metric_id, int score_id, const lgr_metric_params* mp, lgr_metric_eval* out, uint8_t* inlier_mask,
                                   lgr_corr* inliers) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, src && tgt && out && ns > 0 && nt > 0 && c >= 0 && (corr || c == 0), LGR_ERR_INVALID_ARG);
    const bool plane = metric_id == LGR_METRIC_CLOSEST_PLANE || metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE;
    float *ds, *dt;
    lgr_corr *dc, *di = nullptr;
    uint8_t* dm = nullptr;
    lgr_metric_params staged;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    LGR_TRY(hc.weights(ns, &mp, &staged));
    if (inlier_mask && !plane && c) LGR_TRY(hc.out((size_t) c, &dm, LGR_PAD_MASK));
    if (inliers && plane) LGR_TRY(hc.out((size_t) ns, &di));
    LGR_TRY(lgr_analysis_metric_dev(ctx, ds, ns, dt, nt, c ? dc : nullptr, c, T16, Tgt16, metric_id, score_id, mp, out, dm, di));
    if (dm) LGR_TRY(hc.fetch(inlier_mask, dm, (size_t) c));
    if (di) LGR_TRY(hc.fetch(inliers, di, (size_t) out->n_inliers));
    return hc.finish();
}
