// lgr_plane_point.cuh -- what the closest-plane metric does with ONE source point, written once for its device users: the sparse RANSAC
// evaluation (plane_kernel, lgr_plane.hip), the dense evaluation (plane_dense_kernel, lgr_plane_dense.hip), the refinement loop
// (refine_dense_kernel, lgr_refine.hip).  Device only, in an unnamed namespace like lgr_pointpass.cuh -- which it does not include: that
// header's kernels would be emitted into lgr_plane.hip's object.  metric_kernel (lgr_ransac_metric.cuh) keeps a copy of plane_score's
// expressions.  The CPU statements (tests/cpp/plane_dense_ref.cpp, tests/*_ref_lib.py) restate these rules on their own and do not include
// this file.
//
// Declared orders (reference src/metric.cpp:10-53, :55-81) -- a point gets the same bits from every user:
//   * the moved point is ((c0 x + c1 y) + c2 z) + c3 per row; a non-finite moved point is skipped;
//   * the nearest target within r = 2 x threshold: strict d2 < r * r with lgr_dist2, the smallest squared distance, then the lowest
//     index; non-finite target points never answer;
//   * dist = |(N.x (Q.x - px) + N.y (Q.y - py)) + N.z (Q.z - pz)|, an inlier iff dist < threshold (a NaN distance is none);
//   * the value of an inlier is plane_score (lgr_expf for EXP), times w[i] in f32 under weights (calculateScore: value *=
//     weights[inlier.index_query]); its squared-error term is dist * dist.
#pragma once
#include "lgr_grid.cuh"
#include "lgr_internal.h"
#include "lgr_math.cuh"

namespace {

// Eigen Matrix4f * Vector4f on SSE, T column-major: ((c0 x + c1 y) + c2 z) + c3
__device__ __forceinline__ void plane_move(const float* T, float x, float y, float z, float& px, float& py, float& pz) {
    px = ((T[0] * x + T[4] * y) + T[8] * z) + T[12];
    py = ((T[1] * x + T[5] * y) + T[9] * z) + T[13];
    pz = ((T[2] * x + T[6] * y) + T[10] * z) + T[14];
}

// distance of the moved point p to the tangent plane of the target point Q with normal N
__device__ __forceinline__ float plane_dist(const float4& Q, const float4& N, float px, float py, float pz) {
    return fabsf((N.x * (Q.x - px) + N.y * (Q.y - py)) + N.z * (Q.z - pz));
}

// the score of an inlier at distance dist under threshold thr (ScoreFunction, src/metric.cpp:55-81)
__device__ __forceinline__ float plane_score(float dist, float thr, int score_id) {
    float value = 1.f;
    if (score_id == LGR_SCORE_MAE) value = fabsf(dist - thr) / thr;
    else if (score_id == LGR_SCORE_MSE) value = (dist - thr) * (dist - thr) / (thr * thr);
    else if (score_id == LGR_SCORE_EXP) value = lgr_expf(-dist * dist / (2 * thr * thr));
    return value;
}

// What the dense users compute for source point i.  t: the nearest target's sorted position (-1: none within the radius, or the moved
// point is not finite), j: its index (-1), Q: the grid's copy of it (zeros), dist: 0 without a target; value and sq: 0 unless inl.
struct PlanePoint { int t, j; float dist, value, sq; bool inl; float4 Q; };

// No branch inside the candidate loop (nearest_within, lgr_grid.cuh); what follows the walk is a handful of selects, so the lanes
// of a wave only differ in how many candidates their cells hold.
template <bool W>
__device__ __forceinline__ PlanePoint plane_dense_point(const GridDev& g, const float4& P, const float* T, float thr, float r2, int score_id,
                                                        const float* __restrict__ w, int i) {
    PlanePoint o;
    float px, py, pz, d2;
    plane_move(T, P.x, P.y, P.z, px, py, pz);
    o.t = nearest_within(g, px, py, pz, r2, d2, o.j);   // (a non-finite moved point walks nothing: -1)
    float value = 0.f, sq = 0.f;
    o.dist = 0.f;
    o.inl = false;
    o.Q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (o.t >= 0) {
        o.Q = g.pxyz[o.t];
        const float4 N = g.pnrm[o.t];
        o.dist = plane_dist(o.Q, N, px, py, pz);
        o.inl = o.dist < thr;
        if (o.inl) {
            value = plane_score(o.dist, thr, score_id);
            if constexpr (W) value *= w[i];
            sq = o.dist * o.dist;
        }
    }
    o.value = o.inl ? value : 0.f;
    o.sq = o.inl ? sq : 0.f;
    return o;
}

}  // namespace
