// rops_ref.cpp -- CPU statement of the gravity frames, the RoPS135 rows on given frames and the 135-d brute-force matcher, written
// from the algorithm description (src/common.cpp:713-750; ROPSEstimationWithLocalReferenceFrames with 5 bins, 3 rotations, support
// radius = search radius; OpenCV 4.5.1's normL2Sqr; include/matching.h matchBF) with the canonical orders of DESIGN.md section 4.
// Test infrastructure: the tests compile it with g++ -O2 -ffp-contract=off -fopenmp -shared and compare the device bit for bit.
// It calls the host's own acosf, cosf, sinf and logf and states static_cast<unsigned> as the compiler does it, so device == this
// pins the device's restatements (lgr_libm.cuh, lgr_rops_math.h) against the running libm.  Gravity frames that fail the angle
// test are filled in by the caller from tests/shot_ref_lib.py (SHOT frames).
//   points: 12 floats {x, y, z, 1, nx, ny, nz, 0, intensity, curvature, pad, pad}; frames 9 floats (x, y, z axes); rows 135 floats.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../lidar-global-registration_amd/csrc/lgr_rops_math.h"   // (only for the checks of rops_logf / rops_bin against the host)

namespace {

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// Eigen's unvectorized 3-term reduction: a0 b0 + (a1 b1 + a2 b2)
inline float dot3(const float* a, const float* b) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }
inline void cross(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
inline void mat_vec(const float* M, const float* v, float* o) {   // row-major M (rows = frame axes / rotation rows)
    for (int i = 0; i < 3; ++i) o[i] = dot3(M + 3 * i, v);
}

// one distribution matrix's moments, the reference's loops verbatim (std::log, std::pow with the constant exponents 1 and 2)
void central_moments(const float mat[5][5], float out[5]) {
    float mean_i = 0.0f, mean_j = 0.0f;
    for (unsigned i = 0; i < 5; i++)
        for (unsigned j = 0; j < 5; j++) {
            const float m = mat[i][j];
            mean_i += static_cast<float>(i + 1) * m;
            mean_j += static_cast<float>(j + 1) * m;
        }
    float moments[4] = {0.f, 0.f, 0.f, 0.f}, entropy = 0.0f;
    for (unsigned i = 0; i < 5; i++) {
        const float i_factor = static_cast<float>(i + 1) - mean_i;
        for (unsigned j = 0; j < 5; j++) {
            const float j_factor = static_cast<float>(j + 1) - mean_j;
            const float m = mat[i][j];
            if (m > 0.0f) entropy -= m * std::log(m);
            // the exponents of power[][] as constants: GCC folds std::pow(t, 1.f) to t and std::pow(t, 2.f) to t * t
            moments[0] += std::pow(i_factor, 1.0f) * std::pow(j_factor, 1.0f) * m;
            moments[1] += std::pow(i_factor, 2.0f) * std::pow(j_factor, 1.0f) * m;
            moments[2] += std::pow(i_factor, 1.0f) * std::pow(j_factor, 2.0f) * m;
            moments[3] += std::pow(i_factor, 2.0f) * std::pow(j_factor, 2.0f) * m;
        }
    }
    for (int k = 0; k < 4; ++k) out[k] = moments[k];
    out[4] = entropy;
}

// one row.  pts: the transformed support (3 floats each)
void rops_row(const std::vector<float>& pts, float* row) {
    const size_t n = pts.size() / 3;
    float feature[135];
    int nf = 0;
    const float rad = M_PI / 180.0f;
    for (int axis = 0; axis < 3; ++axis) {
        const float ax = axis == 0 ? 1.f : 0.f, ay = axis == 1 ? 1.f : 0.f, az = axis == 2 ? 1.f : 0.f;
        float theta = 90.0f / static_cast<float>(3 + 1);
        const float step = theta;
        do {
            volatile float arg = theta * rad;   // (the host's cosf / sinf at run time, not the compiler's folded constants)
            const float cosine = std::cos((float) arg), sine = std::sin((float) arg);
            const float R[9] = {cosine + (1 - cosine) * ax * ax,   (1 - cosine) * ax * ay - sine * az, (1 - cosine) * ax * az + sine * ay,
                                (1 - cosine) * ay * ax + sine * az, cosine + (1 - cosine) * ay * ay,   (1 - cosine) * ay * az - sine * ax,
                                (1 - cosine) * az * ax - sine * ay, (1 - cosine) * az * ay + sine * ax, cosine + (1 - cosine) * az * az};
            std::vector<float> rot(3 * n);
            float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
            for (size_t q = 0; q < n; ++q) {
                mat_vec(R, &pts[3 * q], &rot[3 * q]);
                for (int c = 0; c < 3; ++c) { mn[c] = std::min(mn[c], rot[3 * q + c]); mx[c] = std::max(mx[c], rot[3 * q + c]); }
            }
            const unsigned coord[3][2] = {{0, 1}, {0, 2}, {1, 2}};
            for (int pr = 0; pr < 3; ++pr) {
                float mat[5][5] = {};
                float* flat = &mat[0][0];   // the reference's matrix is column-major: cell (row, col) at row + 5 col
                const unsigned cu = coord[pr][0], cv = coord[pr][1];
                const float u_bl = (mx[cu] - mn[cu]) / 5u, v_bl = (mx[cv] - mn[cv]) / 5u;
                for (size_t q = 0; q < n; ++q) {
                    const float u_ratio = (rot[3 * q + cu] - mn[cu]) / u_bl, v_ratio = (rot[3 * q + cv] - mn[cv]) / v_bl;
                    // static_cast<unsigned int>(float) on x86-64 g++: cvttss2si to 64 bits, low half (NaN, inf -> 0)
                    const int64_t ri = (u_ratio > -0x1p63f && u_ratio < 0x1p63f) ? (int64_t) u_ratio : INT64_MIN;
                    const int64_t ci = (v_ratio > -0x1p63f && v_ratio < 0x1p63f) ? (int64_t) v_ratio : INT64_MIN;
                    unsigned r = (unsigned) (uint64_t) ri, c = (unsigned) (uint64_t) ci;
                    if (r == 5) r--;
                    if (c == 5) c--;
                    const uint64_t lin = (uint64_t) r + 5ull * c;
                    if (lin < 25) flat[lin] += 1.0f;   // (>= 25: outside the reference's matrix; dropped)
                }
                float cm[5][5];   // [i][j] = matrix(i, j) / max(1, n)
                for (int i = 0; i < 5; ++i)
                    for (int j = 0; j < 5; ++j) cm[i][j] = flat[i + 5 * j] / std::max<float>(1, (float) n);
                central_moments(cm, feature + nf);
                nf += 5;
            }
            theta += step;
        } while (theta < 90.0f);
    }
    float norm = 0.f;
    for (int j = 0; j < 135; ++j) norm = norm + std::abs(feature[j]);
    const float inv = norm < std::numeric_limits<float>::epsilon() ? 1.0f : 1.0f / norm;
    for (int j = 0; j < 135; ++j) row[j] = feature[j] * inv;
}

// normL2Sqr, n = 135: 8 blocks of 16 (acc[k][lane] += t * t for element 16 b + 4 k + lane; s = ((acc0 + acc1) + acc2) + acc3;
// (s0 + s2) + (s1 + s3)), then d += t * t over elements 128..134
float l2sqr135(const float* a, const float* b) {
    float acc[4][4] = {};
    for (int blk = 0; blk < 8; ++blk)
        for (int k = 0; k < 4; ++k)
            for (int l = 0; l < 4; ++l) {
                const float t = a[16 * blk + 4 * k + l] - b[16 * blk + 4 * k + l];
                acc[k][l] = t * t + acc[k][l];
            }
    float s[4];
    for (int l = 0; l < 4; ++l) s[l] = ((acc[0][l] + acc[1][l]) + acc[2][l]) + acc[3][l];
    float d = (s[0] + s[2]) + (s[1] + s[3]);
    for (int j = 128; j < 135; ++j) {
        const float t = a[j] - b[j];
        d += t * t;
    }
    return d;
}

}  // namespace

extern "C" {

// gravity frames; fail[i] = 1 where the angle test fails (the caller supplies the SHOT frame there; the row is left NaN)
void rops_ref_gravity(const float* kps, int m, float* out9, int* fail) {
    const float g[3] = {0.f, 0.f, 1.f};
    for (int i = 0; i < m; ++i) {
        const float* p = kps + 12 * (size_t) i;
        const float z[3] = {p[4], p[5], p[6]};
        float* o = out9 + 9 * (size_t) i;
        if (std::acos(std::abs(std::clamp(dot3(z, g), -1.0f, 1.0f))) > 0.04f) {
            float y[3], x[3];
            cross(g, z, y);
            cross(y, z, x);
            for (int d = 0; d < 3; ++d) { o[d] = x[d]; o[3 + d] = y[d]; o[6 + d] = z[d]; }
            fail[i] = 0;
        } else {
            for (int d = 0; d < 9; ++d) o[d] = std::numeric_limits<float>::quiet_NaN();
            fail[i] = 1;
        }
    }
}

// RoPS rows on the given frames; support: surface points with d2 < r * r, d2 = ((dx dx) + dy dy) + dz dz
void rops_ref(const float* kps, int m, const float* surf, int n, float radius, const float* lrf, float* out135) {
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < m; ++i) {
        const float* p = kps + 12 * (size_t) i;
        const float* F = lrf + 9 * (size_t) i;
        std::vector<float> pts;
        if (finite3(p)) {
            const float r2 = radius * radius;
            for (int k = 0; k < n; ++k) {
                const float* q = surf + 12 * (size_t) k;
                const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
                if (!((dx * dx + dy * dy) + dz * dz < r2)) continue;
                const float d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
                float t[3];
                mat_vec(F, d, t);
                pts.insert(pts.end(), t, t + 3);
            }
        }
        rops_row(pts, out135 + 135 * (size_t) i);
    }
}

// one row from an explicit transformed support (3 floats per point): the hand-worked tests
void rops_ref_row(const float* pts, int n, float* out135) {
    std::vector<float> v(pts, pts + 3 * (size_t) n);
    rops_row(v, out135);
}

// host logf against lgr_rops_math.h's rops_logf on every float with bit pattern in [lo, hi]: the count of differing results
long long rops_ref_count_logf(unsigned lo, unsigned hi) {
    long long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static, 1 << 16)
    for (long long u = lo; u <= (long long) hi; ++u) {
        float x;
        const uint32_t b = (uint32_t) u;
        std::memcpy(&x, &b, 4);
        const float a = std::log(x), c = rops_logf(x);
        if (std::memcmp(&a, &c, 4)) ++bad;
    }
    return bad;
}

// static_cast<unsigned int> as the compiler emits it (kept out of line so that no constant folding applies)
__attribute__((noinline)) unsigned rops_ref_cast_u32(float r) { return static_cast<unsigned>(r); }
unsigned rops_ref_bin(float r) { return rops_bin(r); }

float rops_ref_l2sqr(const float* a, const float* b) { return l2sqr135(a, b); }

// matchBF: per train block the first minimum of sqrt(d2) (strict '<' from FLT_MAX), a later block wins ties; -1 / 0 for no match
void rops_ref_match(const float* q, int mq, const float* t, int mt, int block, int* idx, float* dist) {
#pragma omp parallel for schedule(dynamic, 8)
    for (int i = 0; i < mq; ++i) {
        int best = -1;
        float bd = 0.f;
        for (int j0 = 0; j0 < mt; j0 += block) {
            const int j1 = std::min(mt, j0 + block);
            int bi = -1;
            float bbd = FLT_MAX;
            for (int j = j0; j < j1; ++j) {
                const float d = std::sqrt(l2sqr135(q + 135 * (size_t) i, t + 135 * (size_t) j));
                if (d < bbd) { bbd = d; bi = j; }
            }
            if (bi >= 0 && (best < 0 || !(bd < bbd))) { best = bi; bd = bbd; }
        }
        idx[i] = best;
        dist[i] = best >= 0 ? bd : 0.f;
    }
}

}  // extern "C"
