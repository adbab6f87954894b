// CPU statement of the dense closest-plane evaluation of a transform (include/lgr.h lgr_evaluate_plane_dense*; reference
// src/metric.cpp:10-53 buildClosestPlaneInliers with sparse = false, :55-81 calculateScore, :193-215 the two metric expressions), written
// from the declared orders of DESIGN.md section 4:
//   * the moved point is ((c0 x + c1 y) + c2 z) + c3 per row (Eigen Matrix4f * Vector4f); a non-finite moved point is skipped;
//   * its nearest target within r = 2 x threshold: strict d2 < r * r, d2 = ((dx dx) + dy dy) + dz dz, the smallest d2, then the lowest
//     index; non-finite target points never answer;
//   * dist = |(N.x (Q.x - px) + N.y (Q.y - py)) + N.z (Q.z - pz)|; an inlier iff dist < threshold (a NaN distance is none);
//   * rmse and score are the reference's own loops: plain serial f32 sums over the inliers in ascending source index;
//   * metric = score / ((sparse_ ? SPARSE_POINTS_FRACTION : 1.f) * (float) src.size()) read literally: SPARSE_POINTS_FRACTION is the double
//     macro 0.01, so the ternary has type double, the product and the division are in double and the result is rounded to float once;
//     with weights the second factor is weights_sum (the serial f32 sum of all source weights).
// Everything is brute force.  The EXP score's exponential is the project's own polynomial (csrc/lgr_math.cuh lgr_expf, the oracle's c_expf),
// restated here as tests/cpp/weights_ref.cpp restates it: a dense and a sparse evaluation of a point then agree in every bit.  No host
// libm routine beyond sqrt / fabs / floor is called.
// Build: g++ -O2 -ffp-contract=off -fopenmp -fPIC -shared (tests/plane_dense_ref_lib.py).
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

namespace {

struct Corr { int32_t query, match; float distance, threshold; };

bool finite3(float a, float b, float c) { return std::isfinite(a) && std::isfinite(b) && std::isfinite(c); }

// Cephes polynomial, argument clamped to [-87, 88]
float score_expf(float x) {
    if (x < -87.0f) x = -87.0f;
    if (x > 88.0f) x = 88.0f;
    float fn = std::floor(x * 1.44269504089f + 0.5f);
    float r = x - fn * 0.693359375f;
    r = r - fn * (-2.12194440e-4f);
    float z = r * r;
    float p = 1.9875691500e-4f * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    p = p * z + r + 1.0f;
    int n = (int) fn;
    uint32_t b = (uint32_t) (n + 127) << 23;
    float s;
    memcpy(&s, &b, 4);
    return p * s;
}

}  // namespace

extern "C" {

// returns the number of inliers.  w: ns weights or NULL.  inliers: room for ns (or NULL); nn: ns ints (or NULL), -1 = none in range.
int pdref_evaluate(const float* src, int ns, const float* tgt, int nt, const float* T, int score_id, const float* w, float thr, float* rmse_out,
                   float* metric_out, float* score_out, Corr* inliers, int32_t* nn_out) {
    const float radius = 2 * thr;   // DIST_TO_PLANE_COEFFICIENT * inlier_threshold
    const float r2 = radius * radius;
    std::vector<int> nn(ns);
    std::vector<float> dist(ns);
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < ns; ++i) {
        const float* s = src + (size_t) i * 12;
        const float px = ((T[0] * s[0] + T[4] * s[1]) + T[8] * s[2]) + T[12];
        const float py = ((T[1] * s[0] + T[5] * s[1]) + T[9] * s[2]) + T[13];
        const float pz = ((T[2] * s[0] + T[6] * s[1]) + T[10] * s[2]) + T[14];
        int best = -1;
        float bd = 0.f;
        if (finite3(px, py, pz))
            for (int j = 0; j < nt; ++j) {
                const float* q = tgt + (size_t) j * 12;
                if (!finite3(q[0], q[1], q[2])) continue;
                const float dx = px - q[0], dy = py - q[1], dz = pz - q[2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 < r2)) continue;
                if (best < 0 || d2 < bd) { best = j; bd = d2; }   // ascending j: an equal distance keeps the lower index
            }
        nn[i] = best;
        dist[i] = 0.f;
        if (best >= 0) {
            const float* Q = tgt + (size_t) best * 12;
            dist[i] = std::fabs((Q[4] * (Q[0] - px) + Q[5] * (Q[1] - py)) + Q[6] * (Q[2] - pz));
        }
    }
    // buildClosestPlaneInliers' loop (sparse = false: idx = i) and calculateScore's, both serial
    int n_inl = 0;
    float rmse = 0.f, score = 0.f;
    for (int i = 0; i < ns; ++i) {
        if (nn_out) nn_out[i] = nn[i];
        if (nn[i] < 0) continue;
        const float d = dist[i];
        if (!(d < thr)) continue;
        if (inliers) inliers[n_inl] = Corr{i, nn[i], d, thr};
        ++n_inl;
        rmse += d * d;
        float value = 1.f;
        if (score_id == 1) value = std::fabs(d - thr) / thr;
        else if (score_id == 2) value = (d - thr) * (d - thr) / (thr * thr);
        else if (score_id == 3) value = score_expf(-d * d / (2 * thr * thr));
        if (w) value *= w[i];
        score += value;
    }
    rmse = n_inl ? std::sqrt(rmse / static_cast<float>(n_inl)) : FLT_MAX;
    float denom = (float) ns;
    if (w) {
        denom = 0.f;
        for (int i = 0; i < ns; ++i) denom += w[i];   // WeightedClosestPlaneMetricEstimator::setSourceCloud
    }
    const bool sparse = false;
    *metric_out = score / ((sparse ? 0.01 : 1.f) * denom);
    *rmse_out = rmse;
    *score_out = score;
    return n_inl;
}

}  // extern "C"
