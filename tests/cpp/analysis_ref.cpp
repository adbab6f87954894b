// CPU statement of the ground-truth evaluation of an alignment (include/lgr.h lgr_evaluate_gt*; reference src/analysis.cpp:19-24, 30-43,
// 45-88, 141-185, 187-206, 218-246 and mergeOverlaps, src/common.cpp:558-591), written from the declared orders of DESIGN.md section 4:
//   * a point moves as x * c0 + (y * c1 + (z * c2 + c3)), a normal the same without c3;
//   * "nearest target within r": strict d2 < r * r, d2 = ((dx dx) + dy dy) + dz dz, the smallest d2, then the lowest index; non-finite
//     points neither ask nor answer;  "nearest target": the same order over the whole cloud;
//   * float sums over points: sequential, ascending index, over per-point terms;
//   * the median of the normal differences: rank n / 2 of the ascending values, NaN values dropped.
// Everything is brute force.  The correspondence uniformity is not restated here: tests/analysis_ref_lib.py takes it from the oracle's
// orc_evaluate over the correct correspondences.  acosf is the host libm's (pinned against the device's restatement by
// tests/test_oracle_libm.py and tests/test_gpu_pcl_arith.py).
// Build: g++ -O2 -ffp-contract=off -fopenmp -fPIC -shared (tests/analysis_ref_lib.py).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace {

struct Corr { int32_t query, match; float distance, threshold; };

bool finite3(float a, float b, float c) { return std::isfinite(a) && std::isfinite(b) && std::isfinite(c); }
float sq3(float x, float y, float z) { return (x * x + y * y) + z * z; }
float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
float dist2(const float* a, const float* b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}
void se3(const float* M, const float* p, float* o) {
    for (int r = 0; r < 3; ++r) o[r] = M[r] * p[0] + (M[4 + r] * p[1] + (M[8 + r] * p[2] + M[12 + r]));
}
void so3(const float* M, const float* p, float* o) {
    for (int r = 0; r < 3; ++r) o[r] = M[r] * p[0] + (M[4 + r] * p[1] + M[8 + r] * p[2]);
}

// nearest point of pts (12-float rows) to q under (d2, index); r2 < 0: no radius.  -1 when there is none.
int nearest(const float* q, const float* pts, int n, float r2, float* d2_out) {
    int best = -1;
    float bd = 0.f;
    if (!finite3(q[0], q[1], q[2])) return -1;
    for (int j = 0; j < n; ++j) {
        const float* p = pts + 12 * (size_t) j;
        if (!finite3(p[0], p[1], p[2])) continue;
        const float d2 = dist2(q, p);
        if (r2 >= 0.f && !(d2 < r2)) continue;
        if (best < 0 || d2 < bd) { best = j; bd = d2; }   // ascending j: an equal distance keeps the lower index
    }
    if (d2_out) *d2_out = bd;
    return best;
}

// Gauss-Jordan with partial pivoting in double, rounded to float (the library's lgr_inverse4)
void inverse4(const float* m16, float* out16) {
    double a[4][8];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { a[r][c] = m16[4 * c + r]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r) if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (piv != col) for (int c = 0; c < 8; ++c) std::swap(a[piv][c], a[col][c]);
        const double d = a[col][col];
        for (int c = 0; c < 8; ++c) a[col][c] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
            for (int c = 0; c < 8; ++c) a[r][c] -= f * a[col][c];
        }
    }
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out16[4 * c + r] = (float) a[r][4 + c];
}

// calculateSmoothedDensities (src/common.cpp:531-547) as the library computes it: k nearest finite points in (d2, index) order, the point
// itself included; NaN where there are fewer than k; the second neighbour is the point itself where there is none
void smoothed_densities(const float* pts, int n, int k, float* out) {
    std::vector<float> dk(n);
    std::vector<int> nn1(n);
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < n; ++i) {
        const float* q = pts + 12 * (size_t) i;
        std::vector<std::pair<float, int>> best;   // ascending, at most k
        if (finite3(q[0], q[1], q[2]))
            for (int j = 0; j < n; ++j) {
                const float* p = pts + 12 * (size_t) j;
                if (!finite3(p[0], p[1], p[2])) continue;
                const std::pair<float, int> e(dist2(q, p), j);
                if ((int) best.size() == k && !(e < best.back())) continue;
                best.insert(std::upper_bound(best.begin(), best.end(), e), e);
                if ((int) best.size() > k) best.pop_back();
            }
        dk[i] = (int) best.size() >= k ? std::sqrt(best[k - 1].first) : std::numeric_limits<float>::quiet_NaN();
        nn1[i] = best.size() >= 2 ? best[1].second : i;
    }
    for (int i = 0; i < n; ++i) {
        const float a = dk[i], b = dk[nn1[i]];
        out[i] = (b < a) ? b : a;   // std::min(a, b)
    }
}

float sum_sq(const std::vector<float>& d) {
    float s = 0.f;
    for (float v : d) s += v * v;
    return s;
}

}  // namespace

extern "C" {

struct aref_eval {
    float r_err, t_err, pcd_err, overlap_rmse;
    int32_t overlap_size;
    float normal_diff;
    int32_t n_normal_overlap, n_overlap_src, n_overlap_tgt, n_overlap;
    float overlap, overlap_area;
    int32_t n_correspondences, n_correct_correspondences, n_inliers, n_correct_inliers;
    int32_t converged, converged_and_overlap_ok;
};

// src/analysis.cpp:19-24: angle of R1^T R2 from its unit quaternion and |t1 - t2|, in double, rounded once (as the oracle's orc_rot_trans_diff)
void aref_rot_trans_diff(const float* T1, const float* T2, float* angle, float* tdist) {
    double R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += (double) T1[4 * i + k] * (double) T2[4 * j + k];
            R[3 * i + j] = s;
        }
    const double tr = R[0] + R[4] + R[8];
    const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
    const double sn = 0.5 * std::sqrt(vx * vx + vy * vy + vz * vz), cs = 0.5 * (tr - 1.0);
    *angle = (float) std::atan2(sn, cs);
    const double dx = (double) T1[12] - T2[12], dy = (double) T1[13] - T2[13], dz = (double) T1[14] - T2[14];
    *tdist = (float) std::sqrt(dx * dx + dy * dy + dz * dz);
}

// D = T^-1 * G: every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 in f32
void aref_diff_matrix(const float* T, const float* G, float* D) {
    float inv[16];
    inverse4(T, inv);
    for (int col = 0; col < 4; ++col)
        for (int r = 0; r < 4; ++r)
            D[4 * col + r] = ((inv[r] * G[4 * col] + inv[4 + r] * G[4 * col + 1]) + inv[8 + r] * G[4 * col + 2]) + inv[12 + r] * G[4 * col + 3];
}

// quantities 2 and 3.  Per-point outputs (each optional): term_pcd, term_ov (0 where skipped), idx (-1 where skipped)
void aref_overlap_rmse(const float* src, int ns, const float* tgt, int nt, const float* T, const float* G, float thr, float* pcd_err,
                       float* overlap_rmse, int* overlap_size, float* term_pcd, float* term_ov, int32_t* idx) {
    float D[16];
    aref_diff_matrix(T, G, D);
    const float radius = 2 * thr, r2 = radius * radius;
    std::vector<float> tp(ns), to(ns, 0.f);
    std::vector<int32_t> nn(ns, -1);
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < ns; ++i) {
        const float* p = src + 12 * (size_t) i;
        float g[3], a[3], b[3];
        se3(G, p, g); se3(T, p, a); se3(D, p, b);
        tp[i] = sq3(p[0] - b[0], p[1] - b[1], p[2] - b[2]);
        const int j = nearest(g, tgt, nt, r2, nullptr);
        if (j < 0) continue;
        const float* q = tgt + 12 * (size_t) j;
        if (!finite3(q[4], q[5], q[6])) continue;
        const float s = dot3(g[0] - q[0], g[1] - q[1], g[2] - q[2], q[4], q[5], q[6]);
        const float px = g[0] - s * q[4], py = g[1] - s * q[5], pz = g[2] - s * q[6];
        if (std::sqrt(sq3(g[0] - px, g[1] - py, g[2] - pz)) > thr) continue;
        const float d = std::sqrt(sq3(a[0] - px, a[1] - py, a[2] - pz));
        to[i] = d * d;
        nn[i] = j;
    }
    float s_pcd = 0.f, s_ov = 0.f;
    int cnt = 0;
    for (int i = 0; i < ns; ++i) {
        s_pcd += tp[i];
        if (nn[i] >= 0) { s_ov += to[i]; ++cnt; }
    }
    *pcd_err = std::sqrt(s_pcd / (float) ns);
    *overlap_size = cnt;
    *overlap_rmse = cnt ? std::sqrt(s_ov / (float) cnt) : std::numeric_limits<float>::quiet_NaN();
    if (term_pcd) memcpy(term_pcd, tp.data(), (size_t) ns * 4);
    if (term_ov) memcpy(term_ov, to.data(), (size_t) ns * 4);
    if (idx) memcpy(idx, nn.data(), (size_t) ns * 4);
}

// the ground-truth-aligned source (points and normals moved, the third quad copied)
void aref_align(const float* src, int ns, const float* G, float* out) {
    for (int i = 0; i < ns; ++i) {
        const float* p = src + 12 * (size_t) i;
        float* o = out + 12 * (size_t) i;
        memcpy(o, p, 48);
        se3(G, p, o); so3(G, p + 4, o + 4);
        o[3] = 1.f; o[7] = 0.f;
    }
}

// quantity 4.  values (optional, ns floats): the per-point difference, -1 where the point does not count
void aref_normal_difference(const float* src, int ns, const float* tgt, int nt, const float* G, float thr, float* normal_diff, int* n_overlap,
                            float* values) {
    std::vector<float> al((size_t) 12 * std::max(ns, 1)), v(ns, -1.f);
    aref_align(src, ns, G, al.data());
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < ns; ++i) {
        const float* a = al.data() + 12 * (size_t) i;
        float d2 = 0.f;
        const int j = nearest(a, tgt, nt, -1.f, &d2);
        if (j < 0) continue;
        const float* t = tgt + 12 * (size_t) j;
        if (!(std::sqrt(d2) < thr) || !std::isfinite(a[4]) || !std::isfinite(t[4])) continue;
        float cs = dot3(a[4], a[5], a[6], t[4], t[5], t[6]);
        cs = cs < -1.f ? -1.f : (1.f < cs ? 1.f : cs);
        const float d = std::fabs(acosf(cs));
        if (d >= 0.f) v[i] = d;
    }
    std::vector<float> f;
    for (float d : v) if (d >= 0.f) f.push_back(d);
    *n_overlap = (int) f.size();
    if (values) memcpy(values, v.data(), (size_t) ns * 4);
    if (f.empty()) { *normal_diff = (float) M_PI; return; }
    std::sort(f.begin(), f.end());
    *normal_diff = f[f.size() / 2];
}

// one pass of mergeOverlaps: mask of the compared cloud against the reference cloud; returns the count
static int overlap_pass(const float* cmp, int n, const float* ref, int nr, float thr, uint8_t* mask) {
    const float radius = 2 * thr, r2 = radius * radius;
    int cnt = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : cnt)
    for (int i = 0; i < n; ++i) {
        const float* p = cmp + 12 * (size_t) i;
        float d2 = 0.f;
        const int j = nearest(p, ref, nr, r2, &d2);
        mask[i] = 0;
        if (j < 0) continue;
        const float* q = ref + 12 * (size_t) j;
        float dp = std::fabs(dot3(q[4], q[5], q[6], q[0] - p[0], q[1] - p[1], q[2] - p[2]));
        dp = std::isfinite(dp) ? dp : d2;
        if (dp < thr) { mask[i] = 1; ++cnt; }
    }
    return cnt;
}

// quantity 5.  mask_src / mask_tgt: ns / nt bytes (required)
void aref_merge_overlaps(const float* src, int ns, const float* tgt, int nt, const float* G, float thr, uint8_t* mask_src, uint8_t* mask_tgt,
                         int* n2, float* overlap, float* overlap_area) {
    std::vector<float> al((size_t) 12 * std::max(ns, 1));
    aref_align(src, ns, G, al.data());
    n2[0] = overlap_pass(al.data(), ns, tgt, nt, thr, mask_src);
    n2[1] = overlap_pass(tgt, nt, al.data(), ns, thr, mask_tgt);
    const int no = n2[0] + n2[1];
    *overlap = (float) no / (float) (ns + nt);
    *overlap_area = std::numeric_limits<float>::quiet_NaN();
    if (no < 2 || ns < 2) return;
    std::vector<float> ov((size_t) 12 * no);
    size_t w = 0;
    for (int i = 0; i < ns; ++i) if (mask_src[i]) { memcpy(&ov[12 * w], &al[12 * (size_t) i], 48); ++w; }
    for (int i = 0; i < nt; ++i) if (mask_tgt[i]) { memcpy(&ov[12 * w], tgt + 12 * (size_t) i, 48); ++w; }
    std::vector<float> d_ov(no), d_src(ns);
    smoothed_densities(ov.data(), no, 2, d_ov.data());
    smoothed_densities(src, ns, 2, d_src.data());
    *overlap_area = sum_sq(d_ov) / sum_sq(d_src);
}

// quantities 6 and 7.  correct: c bytes (required); inlier_mask optional.  out3 = {correct, inliers, correct inliers}
void aref_correct_correspondences(const float* src, const float* tgt, const Corr* corr, int c, const float* G, const uint8_t* inlier_mask,
                                  uint8_t* correct, int* out3) {
    out3[0] = out3[1] = out3[2] = 0;
    for (int i = 0; i < c; ++i) {
        float g[3];
        se3(G, src + 12 * (size_t) corr[i].query, g);
        const float* q = tgt + 12 * (size_t) corr[i].match;
        const float e = std::sqrt(sq3(g[0] - q[0], g[1] - q[1], g[2] - q[2]));
        correct[i] = e < corr[i].threshold ? 1 : 0;
        const bool inl = inlier_mask && inlier_mask[i];
        out3[0] += correct[i];
        out3[1] += inl ? 1 : 0;
        out3[2] += (inl && correct[i]) ? 1 : 0;
    }
}

// everything but the correspondence uniformity
void aref_evaluate(const float* src, int ns, const float* tgt, int nt, const Corr* corr, int c, const float* T, const float* G, float thr,
                   int converged, const uint8_t* inlier_mask, aref_eval* out, uint8_t* correct /* c bytes */) {
    memset(out, 0, sizeof *out);
    aref_rot_trans_diff(T, G, &out->r_err, &out->t_err);
    aref_overlap_rmse(src, ns, tgt, nt, T, G, thr, &out->pcd_err, &out->overlap_rmse, &out->overlap_size, nullptr, nullptr, nullptr);
    aref_normal_difference(src, ns, tgt, nt, G, thr, &out->normal_diff, &out->n_normal_overlap, nullptr);
    std::vector<uint8_t> ms(std::max(ns, 1)), mt(std::max(nt, 1));
    int n2[2];
    aref_merge_overlaps(src, ns, tgt, nt, G, thr, ms.data(), mt.data(), n2, &out->overlap, &out->overlap_area);
    out->n_overlap_src = n2[0]; out->n_overlap_tgt = n2[1]; out->n_overlap = n2[0] + n2[1];
    int o3[3];
    aref_correct_correspondences(src, tgt, corr, c, G, inlier_mask, correct, o3);
    out->n_correspondences = c; out->n_correct_correspondences = o3[0]; out->n_inliers = o3[1]; out->n_correct_inliers = o3[2];
    out->converged = converged ? 1 : 0;
    out->converged_and_overlap_ok = (converged && out->overlap_rmse < thr) ? 1 : 0;
}

}  // extern "C"
