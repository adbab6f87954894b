// CPU statement of the temperature maps, the hypothesis overlap comparison and the colour passes (include/lgr.h lgr_temperature_map*,
// lgr_temperature_maps*, lgr_compare_overlaps*, lgr_nearest_dev, lgr_color_*; reference src/common.cpp:771-850, 859-963 and
// src/main.cpp:152-205), written from the declared orders of DESIGN.md section 4:
//   * a point moves as x * c0 + (y * c1 + (z * c2 + c3)), a normal the same without c3;
//   * "nearest within r": strict d2 < r * r, d2 = ((dx dx) + dy dy) + dz dz, the smallest d2, then the lowest index; "nearest": the same
//     order over the whole cloud; non-finite points neither ask nor answer;
//   * getColor with std::min / std::max themselves, plain float arithmetic;
//   * weighted_count: sequential f32 sum of density^2 in index order over {moved source rows, target rows}; 0 below 2 points.
// Everything is brute force over all points.  acosf is the host libm's.
// Build: g++ -O2 -ffp-contract=off -fopenmp -fPIC -shared (tests/debug_ref_lib.py).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cstdint>
#include <cmath>
#include <limits>
#include <vector>

namespace {

struct Corr { int32_t query, match; float distance, threshold; };

bool finite3(float a, float b, float c) { return std::isfinite(a) && std::isfinite(b) && std::isfinite(c); }
float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
float dist2(const float* a, const float* b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
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

// |n_q . (q - p)| against the neighbour q of p, the squared distance where that is not finite
float plane_distance(const float* p, const float* q, float d2) {
    const float dp = std::fabs(dot3(q[4], q[5], q[6], q[0] - p[0], q[1] - p[1], q[2] - p[2]));
    return std::isfinite(dp) ? dp : d2;
}

// calculateSmoothedDensities (src/common.cpp:531-547): k nearest finite points in (d2, index) order, the point itself included; NaN where
// there are fewer than k; the second neighbour is the point itself where there is none
void smoothed_densities(const float* pts, int n, int k, float* out) {
    std::vector<float> dk(n);
    std::vector<int> nn1(n);
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < n; ++i) {
        const float* q = pts + 12 * (size_t) i;
        std::vector<std::pair<float, int>> best;
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
    for (int i = 0; i < n; ++i) out[i] = std::min(dk[i], dk[nn1[i]]);
}

// one pass of compareOverlaps: mask of the compared cloud against its NEAREST reference point; returns the count
int overlap_pass(const float* cmp, int n, const float* ref, int nr, float thr, uint8_t* mask) {
    int cnt = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : cnt)
    for (int i = 0; i < n; ++i) {
        const float* p = cmp + 12 * (size_t) i;
        float d2 = 0.f;
        const int j = nearest(p, ref, nr, -1.f, &d2);
        mask[i] = 0;
        if (j < 0) continue;
        if (plane_distance(p, ref + 12 * (size_t) j, d2) < thr) { mask[i] = 1; ++cnt; }
    }
    return cnt;
}

}  // namespace

extern "C" {

// src/common.cpp:818-835, as written there
int dref_get_color(float v, float vmin, float vmax) {
    float r = 1.f, g = 1.f, b = 1.f;
    float dv = vmax - vmin;
    v = std::max(vmin, std::min(v, vmax));
    if (v < (vmin + dv / 3.f)) {
        b = 1.f - 3.f * (v - vmin) / dv;
    } else if (v < (vmin + 2.f * dv / 3.f)) {
        b = 0.f;
        g = 2.f - 3.f * (v - vmin) / dv;
    } else {
        b = 0.f;
        g = 0.f;
        r = 3.f - 3.f * (v - vmin) / dv;
    }
    // (std::uint8_t) (255.f * c) for a product in (-1, 256); a NaN product (vmin == vmax) is declared 0
    auto c8 = [](float c) { const float x = 255.f * c; return std::isnan(x) ? 0 : (int) (std::uint8_t) x; };
    return (c8(r) << 16) + (c8(g) << 8) + c8(b);
}

// src/common.cpp:1155-1159 applied `times` times
int dref_mix_color(int color, int mix, int times) {
    uint8_t r = (color >> 16) & 0xff, g = (color >> 8) & 0xff, b = color & 0xff;
    for (int k = 0; k < times; ++k) {
        r = r / 2 + ((mix >> 16) & 0xff) / 2;
        g = g / 2 + ((mix >> 8) & 0xff) / 2;
        b = b / 2 + ((mix >> 0) & 0xff) / 2;
    }
    return (r << 16) + (g << 8) + b;
}

// include/utils.h:45-66 quantile<float>
float dref_quantile(double q, const float* values, int n) {
    if (q < 0.0 || q > 1.0 || n == 0) return std::numeric_limits<float>::quiet_NaN();
    if (n == 1) return values[0];
    std::size_t N = n;
    std::size_t i = std::floor(q * (double) (N - 1));
    std::size_t j = std::min(i + 1, N - 1);
    std::vector<float> v(values, values + n);
    std::nth_element(v.begin(), v.begin() + i, v.end());
    float ith = v[i];
    if (i < j) {
        std::nth_element(v.begin(), v.begin() + j, v.end());
        float jth = v[j];
        return ith * ((double) N * q - (double) i) + jth * ((double) j - (double) N * q);
    }
    return ith;
}

void dref_color_map(const float* values, int n, float vmin, float vmax, int32_t* colors) {
    for (int i = 0; i < n; ++i) colors[i] = dref_get_color(values[i], vmin, vmax);
}

// src/common.cpp:837-850
void dref_color_weights(const float* w, int n, int32_t* colors, float* range2) {
    range2[0] = dref_quantile(0.01, w, n);
    range2[1] = dref_quantile(0.99, w, n);
    dref_color_map(w, n, range2[0], range2[1], colors);
}

// src/common.cpp:781-812 in its own order (the lists are walked one after the other)
void dref_color_correspondences(int n, const int32_t* kp, int n_kp, int with_kp, const Corr* corr, int c, const Corr* correct, int n_correct, const Corr* inl,
                                int n_inl, int is_source, int32_t* colors) {
    for (int i = 0; i < n; ++i) colors[i] = with_kp ? 0x03c04a : 0xf8c471;
    for (int i = 0; i < n_kp; ++i) colors[kp[i]] = 0xf8c471;
    for (int i = 0; i < c; ++i) colors[is_source ? corr[i].query : corr[i].match] = 0xff0000;
    for (int i = 0; i < n_inl; ++i) colors[is_source ? inl[i].query : inl[i].match] = 0x0000ff;
    for (int i = 0; i < n_correct; ++i) {
        int32_t& col = colors[is_source ? correct[i].query : correct[i].match];
        col = dref_mix_color(col, 0xffffff, 1);
    }
}

void dref_move(const float* src, int ns, const float* M, float* out) {
    for (int i = 0; i < ns; ++i) {
        const float* p = src + 12 * (size_t) i;
        float* o = out + 12 * (size_t) i;
        memcpy(o, p, 48);
        for (int r = 0; r < 3; ++r) {
            o[r] = M[r] * p[0] + (M[4 + r] * p[1] + (M[8 + r] * p[2] + M[12 + r]));
            o[4 + r] = M[r] * p[4] + (M[4 + r] * p[5] + M[8 + r] * p[6]);
        }
        o[3] = 1.f; o[7] = 0.f;
    }
}

// the unbounded nearest neighbour of every query (rows of 12 floats): index (-1: none) and squared distance (+inf: none)
void dref_nearest(const float* q, int nq, const float* pts, int n, int32_t* idx, float* d2) {
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < nq; ++i) {
        float d = 0.f;
        idx[i] = nearest(q + 12 * (size_t) i, pts, n, -1.f, &d);
        d2[i] = idx[i] >= 0 ? d : std::numeric_limits<float>::infinity();
    }
}

// src/common.cpp:859-906 for both temperature types; every output required (n entries each)
void dref_temperature_map(const float* cmp, int n, const float* ref, int nr, float dmax, float* td, float* tn, int32_t* cd, int32_t* cn, int32_t* nn,
                          int* n_below) {
    const float radius = 2 * dmax, r2 = radius * radius;
    const float tmax = M_PI / 2;
    int cnt = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : cnt)
    for (int i = 0; i < n; ++i) {
        const float* p = cmp + 12 * (size_t) i;
        float d2 = 0.f;
        const int j = nearest(p, ref, nr, r2, &d2);
        float dist_to_plane = dmax;
        const float* q = nullptr;
        if (j >= 0) {
            q = ref + 12 * (size_t) j;
            dist_to_plane = plane_distance(p, q, d2);
        }
        nn[i] = j;
        if (dist_to_plane < dmax) {
            float cos_normal_diff = dot3(q[4], q[5], q[6], p[4], p[5], p[6]);
            float normal_diff = std::fabs(acosf(std::max(std::min(cos_normal_diff, 1.f), -1.f)));
            normal_diff = std::min(normal_diff, tmax);
            normal_diff = std::isfinite(normal_diff) ? normal_diff : tmax;
            td[i] = dist_to_plane; tn[i] = normal_diff;
            ++cnt;
        } else {
            td[i] = dmax; tn[i] = tmax;
        }
        cd[i] = dref_get_color(td[i], 0.f, dmax);
        cn[i] = dref_get_color(tn[i], 0.f, tmax);
    }
    *n_below = cnt;
}

// src/common.cpp:908-963 without the files: outs of the source side, then of the target side; moved: ns rows
void dref_temperature_maps(const float* src, int ns, const float* tgt, int nt, const float* T, float thr, float* td_s, float* tn_s, int32_t* cd_s,
                           int32_t* cn_s, int32_t* nn_s, float* td_t, float* tn_t, int32_t* cd_t, int32_t* cn_t, int32_t* nn_t, float* moved, int* n_below2) {
    dref_move(src, ns, T, moved);
    dref_temperature_map(moved, ns, tgt, nt, thr, td_s, tn_s, cd_s, cn_s, nn_s, n_below2 + 0);
    dref_temperature_map(tgt, nt, moved, ns, thr, td_t, tn_t, cd_t, cn_t, nn_t, n_below2 + 1);
}

// src/main.cpp:152-205 for n transformations; mask_src: n x ns bytes, mask_tgt: n x nt bytes (required)
void dref_compare_overlaps(const float* src, int ns, const float* tgt, int nt, const float* tns, int n, float thr, int32_t* counts, float* weighted,
                           int32_t* counts2, uint8_t* mask_src, uint8_t* mask_tgt) {
    std::vector<float> al((size_t) 12 * std::max(ns, 1));
    for (int k = 0; k < n; ++k) {
        uint8_t *ms = mask_src + (size_t) k * ns, *mt = mask_tgt + (size_t) k * nt;
        counts[k] = 0; weighted[k] = 0.f; counts2[2 * k] = counts2[2 * k + 1] = 0;
        if (ns == 0 || nt == 0) continue;
        dref_move(src, ns, tns + 16 * (size_t) k, al.data());
        counts2[2 * k] = overlap_pass(al.data(), ns, tgt, nt, thr, ms);
        counts2[2 * k + 1] = overlap_pass(tgt, nt, al.data(), ns, thr, mt);
        const int no = counts2[2 * k] + counts2[2 * k + 1];
        counts[k] = no;
        if (no < 2) continue;
        std::vector<float> ov((size_t) 12 * no), dens(no);
        size_t w = 0;
        for (int i = 0; i < ns; ++i) if (ms[i]) { memcpy(&ov[12 * w], &al[12 * (size_t) i], 48); ++w; }
        for (int i = 0; i < nt; ++i) if (mt[i]) { memcpy(&ov[12 * w], tgt + 12 * (size_t) i, 48); ++w; }
        smoothed_densities(ov.data(), no, 2, dens.data());
        float s = 0.f;
        for (int i = 0; i < no; ++i) s += dens[i] * dens[i];
        weighted[k] = s;
    }
}

}  // extern "C"
