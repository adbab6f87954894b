// lgr_icp_math.h -- the f64 arithmetic of one point-to-plane ICP step ("Point-to-plane ICP"), stated once for the
// device (icp_step_kernel, lgr_icp.hip) and the CPU statement of the tests (tests/cpp/icp_ref.cpp), so that device == statement is a
// bit-for-bit claim:
//   icp_tri        position of A(a, b), a <= b, among the 21 upper-triangle sums (row by row);
//   icp_solve      A xi = -b by LDL^T without pivoting, one fixed operation order, with the pivot rule of the statement;
//   icp_rotation   R from the unit quaternion (1, w / 2) / |(1, w / 2)|: nine polynomial expressions, no trigonometry;
//   icp_compose    T' = [R | (c - R c) + t] o T, every entry formed in f64 and rounded to f32 once;
//   icp_norm3, icp_rmse, icp_next_dist   the scalars of the stop rule, the report and the next iteration's distance;
//   icp_inv_sym3, icp_robust_weight      lgr_icp_ex*: the inverse of plane-to-plane's 3 x 3 covariance sum, the M-estimators' weights;
//   icp_trim_key, icp_trim_k, icp_trim_median_rank, icp_trim_scale, icp_trim_weight   lgr_icp_trim*: the key that orders the pairs, K from
//                  keep and P, the median's rank, k of the iteration and the weight under it.
// Every operation is one IEEE binary64 + - * / sqrt (binary32 where a float is named); compile with -ffp-contract=off on both sides (the
// Makefile and the tests do).  The pairing, the 28 terms of a point and the balanced tree that sums them are NOT here: the kernels
// (icp_terms_kernel, icp_tree_kernel) and the statements each write them on their own.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ICP_HD __host__ __device__ __forceinline__
#define ICP_UNROLL _Pragma("unroll")   // every loop below has constant bounds: unrolled, the small matrices live in registers
#else
#define ICP_HD inline
#define ICP_UNROLL
#endif

enum { ICP_TERMS = 28, ICP_STOP_MAX_ITERATIONS = 0, ICP_STOP_CONVERGED = 1, ICP_STOP_NO_PAIRS = 2, ICP_STOP_DEGENERATE = 3, ICP_MIN_PAIRS = 6 };
// layout of the 28 sums: [0, 21) A's upper triangle, [21, 27) b = sum g r, [27] sum r r

ICP_HD int icp_tri(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }   // a <= b

ICP_HD bool icp_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }

// ---- the variants of lgr_icp_ex* ("ICP variants"): the two pieces both sides share; the pairing, the gate and the
// term products are written once in icp_terms_kernel and once in tests/cpp/icp_ex_ref.cpp
enum { ICP_POINT_TO_PLANE = 0, ICP_POINT_TO_POINT = 1, ICP_PLANE_TO_PLANE = 2, ICP_ROBUST_NONE = 0, ICP_ROBUST_HUBER = 1, ICP_ROBUST_CAUCHY = 2, ICP_ROBUST_TUKEY = 3 };

// M = S^-1 of the symmetric S = (xx, xy, xz, yy, yz, zz), in the same packing: the adjugate's six entries, each a b - c d, the determinant
// (xx c00 + xy c01) + xz c02 along the first row, six divisions.  false: the determinant is not finite or not > 0 (M is not written).
ICP_HD bool icp_inv_sym3(const double* S, double* M) {
    const double xx = S[0], xy = S[1], xz = S[2], yy = S[3], yz = S[4], zz = S[5];
    const double c00 = yy * zz - yz * yz, c01 = xz * yz - xy * zz, c02 = xy * yz - xz * yy;
    const double det = (xx * c00 + xy * c01) + xz * c02;
    if (!icp_finite(det) || !(det > 0.0)) return false;
    const double c11 = xx * zz - xz * xz, c12 = xy * xz - xx * yz, c22 = xx * yy - xy * xy;
    M[0] = c00 / det; M[1] = c01 / det; M[2] = c02 / det;
    M[3] = c11 / det; M[4] = c12 / det; M[5] = c22 / det;
    return true;
}

// w(rho, k) of a residual rho >= 0 under the scale k > 0; q = (rho rho) / (k k).  A NaN rho gives a weight that is not > 0 (NONE excepted).
//   HUBER  rho <= k ? 1 : k / rho        CAUCHY  1 / (1 + q)        TUKEY  rho < k ? (1 - q) (1 - q) : 0
ICP_HD double icp_robust_weight(int kind, double rho, double k) {
    if (kind == ICP_ROBUST_HUBER) return rho <= k ? 1.0 : k / rho;
    if (kind == ICP_ROBUST_CAUCHY) return 1.0 / (1.0 + (rho * rho) / (k * k));
    if (kind == ICP_ROBUST_TUKEY) {
        if (!(rho < k)) return 0.0;
        const double t = 1.0 - (rho * rho) / (k * k);
        return t * t;
    }
    return 1.0;
}

// ---- trimmed ICP (lgr_icp_trim*; DESIGN.md section 4, "Trimmed ICP"): the scalar pieces the device and tests/cpp/icp_trim_ref.cpp share.
// How the ranks are found is NOT here: the device selects by radix (lgr_rank_select.cuh), the statement sorts.

// key = (float) rho as its bit pattern.  true: the key is finite and carries no sign bit, so that its bits order as a uint32 the way the
// values order as floats -- the point is a candidate.  (A finite rho of this loop stays far below FLT_MAX: max_dist <= 1e18.)
ICP_HD bool icp_trim_key(double rho, uint32_t* bits) {
    const float key = (float) rho;
    uint32_t b;
    __builtin_memcpy(&b, &key, 4);
    *bits = b;
    return b <= 0x7f7fffffu;
}

ICP_HD float icp_trim_key_value(uint32_t bits) {
    float key;
    __builtin_memcpy(&key, &bits, 4);
    return key;
}

// what orders the candidates: (key, i)
ICP_HD unsigned long long icp_trim_composite(uint32_t key_bits, uint32_t i) { return ((unsigned long long) key_bits << 32) | i; }

// K = floor(keep P) of P candidates, keep in (0, 1]
ICP_HD long long icp_trim_k(float keep, long long P) { return (long long) __builtin_floor((double) keep * (double) P); }

// rank of the median among P >= 1 candidates (the lower one of an even count)
ICP_HD long long icp_trim_median_rank(long long P) { return (P - 1) / 2; }

// k of the iteration: scale_from_median x the median key (0 without a candidate) where scale_from_median > 0, else the caller's scale
ICP_HD double icp_trim_scale(float scale_from_median, float key_median, float robust_scale) {
    return scale_from_median > 0.f ? (double) scale_from_median * (double) key_median : (double) robust_scale;
}

// w of a kept candidate: a k that is not finite or not > 0 (a median key of 0) weighs every pair 1
ICP_HD double icp_trim_weight(int kind, double rho, double k) { return icp_finite(k) && k > 0.0 ? icp_robust_weight(kind, rho, k) : 1.0; }

// xi = -A^-1 b.  A = L D L^T with unit lower L: for column j, v_k = L(j, k) D(k) (k < j), D(j) = A(j, j) - sum_k L(j, k) v_k and
// L(i, j) = (A(i, j) - sum_k L(i, k) v_k) / D(j), the sums subtracted one by one in ascending k.  Then L y = -b downwards, z = y / D,
// L^T xi = z upwards, again one subtraction per k in ascending (downwards) / descending-row ascending-k (upwards) order as written.
// false: a pivot is not finite or not > 1e-12 x the largest diagonal entry of A (a single plane, collinear normals, NaN sums).
ICP_HD bool icp_solve(const double* s, double* xi) {
    double L[6][6], D[6], v[6], y[6];
    double dmax = s[icp_tri(0, 0)];
    ICP_UNROLL
    for (int j = 1; j < 6; ++j) {
        const double a = s[icp_tri(j, j)];
        dmax = a > dmax ? a : dmax;
    }
    const double floor_ = 1e-12 * dmax;
    ICP_UNROLL
    for (int j = 0; j < 6; ++j) {
        double d = s[icp_tri(j, j)];
        ICP_UNROLL
        for (int k = 0; k < j; ++k) {
            v[k] = L[j][k] * D[k];
            d = d - L[j][k] * v[k];
        }
        if (!icp_finite(d) || !(d > floor_)) return false;
        D[j] = d;
        ICP_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double a = s[icp_tri(j, i)];
            ICP_UNROLL
            for (int k = 0; k < j; ++k) a = a - L[i][k] * v[k];
            L[i][j] = a / d;
        }
    }
    ICP_UNROLL
    for (int i = 0; i < 6; ++i) {
        double a = -s[21 + i];
        ICP_UNROLL
        for (int k = 0; k < i; ++k) a = a - L[i][k] * y[k];
        y[i] = a;
    }
    ICP_UNROLL
    for (int i = 5; i >= 0; --i) {
        double a = y[i] / D[i];
        ICP_UNROLL
        for (int k = i + 1; k < 6; ++k) a = a - L[k][i] * xi[k];
        xi[i] = a;
    }
    return true;
}

// R (row-major 3 x 3) of the unit quaternion (w, x, y, z) = (1, wx / 2, wy / 2, wz / 2) / n, n = sqrt(((1 + hx hx) + hy hy) + hz hz)
ICP_HD void icp_rotation(const double* w3, double* R) {
    const double hx = w3[0] * 0.5, hy = w3[1] * 0.5, hz = w3[2] * 0.5;
    const double n = __builtin_sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    const double w = 1.0 / n, x = hx / n, y = hy / n, z = hz / n;
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// T and out column-major 4 x 4 floats (out may not alias T); c the centre (floats), t3 the step's translation
ICP_HD void icp_compose(const double* R, const double* t3, const float* c, const float* T, float* out) {
    const double c0 = (double) c[0], c1 = (double) c[1], c2 = (double) c[2];
    ICP_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double r0 = R[3 * i], r1 = R[3 * i + 1], r2 = R[3 * i + 2];
        const double tt = ((double) c[i] - ((r0 * c0 + r1 * c1) + r2 * c2)) + t3[i];
        ICP_UNROLL
        for (int j = 0; j < 3; ++j)
            out[4 * j + i] = (float) ((r0 * (double) T[4 * j] + r1 * (double) T[4 * j + 1]) + r2 * (double) T[4 * j + 2]);
        out[12 + i] = (float) (((r0 * (double) T[12] + r1 * (double) T[13]) + r2 * (double) T[14]) + tt);
    }
    out[3] = 0.f; out[7] = 0.f; out[11] = 0.f; out[15] = 1.f;
}

ICP_HD double icp_norm3(const double* v) { return __builtin_sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// (float) sqrt(sum r r / pairs); FLT_MAX without a pair, as the library's other rmse figures
ICP_HD float icp_rmse(double rr, long long pairs) { return pairs > 0 ? (float) __builtin_sqrt(rr / (double) pairs) : 3.4028234663852886e38f; }

// d_{k+1} = max(min_dist, d_k * shrink) in f32
ICP_HD float icp_next_dist(float d, float shrink, float min_dist) {
    const float n = d * shrink;
    return min_dist > n ? min_dist : n;
}

// What one iteration decides from its 28 sums and its pair count.  T: T_k; Tn: T_{k+1} (written when the step is taken).
// returns the stop code, or -1 to go on; rot / trans: |w| and |t| of the step as floats (0 when no step is taken).
ICP_HD int icp_step(const double* s, long long pairs, const float* c, const float* T, int k, int max_iterations, float rot_eps, float trans_eps,
                    float* Tn, bool* stepped, float* rot, float* trans) {
    *stepped = false;
    *rot = 0.f; *trans = 0.f;
    if (pairs < ICP_MIN_PAIRS) return ICP_STOP_NO_PAIRS;
    double xi[6], R[9];
    if (!icp_solve(s, xi)) return ICP_STOP_DEGENERATE;
    icp_rotation(xi, R);
    icp_compose(R, xi + 3, c, T, Tn);
    *stepped = true;
    const double nw = icp_norm3(xi), nt = icp_norm3(xi + 3);
    *rot = (float) nw; *trans = (float) nt;
    if (nw < (double) rot_eps && nt < (double) trans_eps) return ICP_STOP_CONVERGED;
    if (k + 1 >= max_iterations) return ICP_STOP_MAX_ITERATIONS;
    return -1;
}
