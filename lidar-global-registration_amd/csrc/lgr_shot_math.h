// lgr_shot_math.h -- the double-precision arithmetic of the SHOT stage that has no IEEE-exact definition, stated once for the device
// kernels (lgr_shot.hip) and the CPU reference of the tests (tests/cpp/shot_ref.cpp), so that device == reference is a bit-for-bit
// statement:
//   shot_acos, shot_atan2   fdlibm 5.3's __ieee754_acos / atan / __ieee754_atan2 (Sun Microsystems, freely distributable) restated
//                           op for op: only IEEE + - * / sqrt and bit tests.  What the reference's std::acos / std::atan2 return
//                           (the host's libm) differs from them by at most 1 ulp; tests/test_shot_ref.py measures it;
//   shot_eigen3             the symmetric 3 x 3 eigen-decomposition of SHOTLocalReferenceFrameEstimation (Eigen's
//                           SelfAdjointEigenSolver<Matrix3d> in the reference) as cyclic Jacobi with a fixed schedule: a declared
//                           deviation, like lgr_svd3.
// Compile with -ffp-contract=off on both sides (the Makefile and the tests do).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SHOT_HD __host__ __device__ __forceinline__
#define SHOT_UNROLL _Pragma("unroll")
#else
#define SHOT_HD inline
#define SHOT_UNROLL
#endif

SHOT_HD int32_t shot_hi(double x) { uint64_t b; __builtin_memcpy(&b, &x, 8); return (int32_t) (uint32_t) (b >> 32); }
SHOT_HD uint32_t shot_lo(double x) { uint64_t b; __builtin_memcpy(&b, &x, 8); return (uint32_t) b; }
SHOT_HD double shot_with_lo(double x, uint32_t lo) {
    uint64_t b; __builtin_memcpy(&b, &x, 8);
    b = (b & 0xffffffff00000000ull) | lo;
    double r; __builtin_memcpy(&r, &b, 8); return r;
}
SHOT_HD double shot_fabs(double x) { return x < 0.0 ? -x : (x == 0.0 ? 0.0 : x); }
SHOT_HD double shot_sqrt(double x) { return __builtin_sqrt(x); }

// fdlibm e_acos.c
SHOT_HD double shot_acos(double x) {
    const double one = 1.0, pi = 3.14159265358979311600e+00, pio2_hi = 1.57079632679489655800e+00,
                 pio2_lo = 6.12323399573676603587e-17, pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01,
                 pS2 = 2.01212532134862925881e-01, pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04,
                 pS5 = 3.47933107596021167570e-05, qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00,
                 qS3 = -6.88283971605453293030e-01, qS4 = 7.70381505559019352791e-02;
    const int32_t hx = shot_hi(x), ix = hx & 0x7fffffff;
    if (ix >= 0x3ff00000) {                                   // |x| >= 1
        if (((ix - 0x3ff00000) | (int32_t) shot_lo(x)) == 0) return hx > 0 ? 0.0 : pi + 2.0 * pio2_lo;
        return (x - x) / (x - x);                              // NaN
    }
    if (ix < 0x3fe00000) {                                    // |x| < 0.5
        if (ix <= 0x3c600000) return pio2_hi + pio2_lo;
        const double z = x * x;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double r = p / q;
        return pio2_hi - (x - (pio2_lo - x * r));
    } else if (hx < 0) {                                      // x < -0.5
        const double z = (one + x) * 0.5;
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double s = shot_sqrt(z);
        const double r = p / q;
        const double w = r * s - pio2_lo;
        return pi - 2.0 * (s + w);
    } else {                                                  // x > 0.5
        const double z = (one - x) * 0.5;
        const double s = shot_sqrt(z);
        const double df = shot_with_lo(s, 0u);
        const double c = (z - df * df) / (s + df);
        const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const double q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const double r = p / q;
        const double w = r * s + c;
        return 2.0 * (df + w);
    }
}

// fdlibm s_atan.c
SHOT_HD double shot_atan(double x) {
    const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
    const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
    const double aT0 = 3.33333333333329318027e-01, aT1 = -1.99999999998764832476e-01, aT2 = 1.42857142725034663711e-01,
                 aT3 = -1.11111104054623557880e-01, aT4 = 9.09088713343650656196e-02, aT5 = -7.69187620504482999495e-02,
                 aT6 = 6.66107313738753120669e-02, aT7 = -5.83357013379057348645e-02, aT8 = 4.97687799461593236017e-02,
                 aT9 = -3.65315727442169155270e-02, aT10 = 1.62858201153657823623e-02;
    const double one = 1.0;
    const int32_t hx = shot_hi(x), ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x44100000) {                                   // |x| >= 2^66
        if (ix > 0x7ff00000 || (ix == 0x7ff00000 && shot_lo(x) != 0)) return x + x;
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3fdc0000) {                                    // |x| < 0.4375
        if (ix < 0x3e200000) return x;                        // |x| < 2^-29
        id = -1;
    } else {
        x = shot_fabs(x);
        if (ix < 0x3ff30000) {                                // |x| < 1.1875
            if (ix < 0x3fe60000) { id = 0; x = (2.0 * x - one) / (2.0 + x); }
            else { id = 1; x = (x - one) / (x + one); }
        } else {
            if (ix < 0x40038000) { id = 2; x = (x - 1.5) / (one + 1.5 * x); }
            else { id = 3; x = -1.0 / x; }
        }
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
    const double s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
    if (id < 0) return x - x * (s1 + s2);
    // (selects rather than a run-time index: a device array indexed at run time lives in scratch memory)
    const double ahi = id == 0 ? atanhi[0] : (id == 1 ? atanhi[1] : (id == 2 ? atanhi[2] : atanhi[3]));
    const double alo = id == 0 ? atanlo[0] : (id == 1 ? atanlo[1] : (id == 2 ? atanlo[2] : atanlo[3]));
    const double zz = ahi - ((x * (s1 + s2) - alo) - x);
    return hx < 0 ? -zz : zz;
}

// fdlibm e_atan2.c
SHOT_HD double shot_atan2(double y, double x) {
    const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900e-01, pi_o_2 = 1.5707963267948965580e+00,
                 pi = 3.1415926535897931160e+00, pi_lo = 1.2246467991473531772e-16;
    const int32_t hx = shot_hi(x), ix = hx & 0x7fffffff, hy = shot_hi(y), iy = hy & 0x7fffffff;
    const uint32_t lx = shot_lo(x), ly = shot_lo(y);
    if (((uint32_t) ix | ((lx | (0u - lx)) >> 31)) > 0x7ff00000u || ((uint32_t) iy | ((ly | (0u - ly)) >> 31)) > 0x7ff00000u) return x + y;
    if (((hx - 0x3ff00000) | (int32_t) lx) == 0) return shot_atan(y);   // x = 1.0
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);                   // 2 * sign(x) + sign(y)
    if ((iy | (int32_t) ly) == 0) {                                      // y = 0
        switch (m) {
            case 0: case 1: return y;
            case 2: return pi + tiny;
            default: return -pi - tiny;
        }
    }
    if ((ix | (int32_t) lx) == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;   // x = 0
    if (ix == 0x7ff00000) {                                              // x = inf
        if (iy == 0x7ff00000) {
            switch (m) {
                case 0: return pi_o_4 + tiny;
                case 1: return -pi_o_4 - tiny;
                case 2: return 3.0 * pi_o_4 + tiny;
                default: return -3.0 * pi_o_4 - tiny;
            }
        } else {
            switch (m) {
                case 0: return 0.0;
                case 1: return -0.0;
                case 2: return pi + tiny;
                default: return -pi - tiny;
            }
        }
    }
    if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;   // y = inf
    const int k = (iy - ix) >> 20;
    double z;
    if (k > 60) z = pi_o_2 + 0.5 * pi_lo;                                // |y / x| > 2^60
    else if (hx < 0 && k < -60) z = 0.0;                                 // |y| / x < -2^60
    else z = shot_atan(shot_fabs(y / x));
    switch (m) {
        case 0: return z;
        case 1: return -z;
        case 2: return pi - (z - pi_lo);
        default: return (z - pi_lo) - pi;
    }
}

// Symmetric 3 x 3 eigen-decomposition by cyclic Jacobi: SHOT_JACOBI_SWEEPS sweeps over (0,1), (0,2), (1,2), a rotation skipped only when its
// off-diagonal entry is exactly 0 (Rutishauser's formulas: t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c).
// a: row-major, symmetric, destroyed.  On return w[k] = a[k][k] and column k of v (row-major v[3 * r + k]) is its eigenvector.
#define SHOT_JACOBI_SWEEPS 8
SHOT_HD void shot_eigen3(double a[9], double w[3], double v[9]) {
    for (int i = 0; i < 9; ++i) v[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SHOT_JACOBI_SWEEPS; ++sweep) {
        SHOT_UNROLL
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = a[3 * p + q];
            if (apq == 0.0) continue;
            const double theta = (a[3 * q + q] - a[3 * p + p]) / (2.0 * apq);
            double t;
            if (shot_fabs(theta) > 1e150) t = 0.5 / theta;
            else {
                t = 1.0 / (shot_fabs(theta) + shot_sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
            }
            const double c = 1.0 / shot_sqrt(t * t + 1.0), s = t * c;
            SHOT_UNROLL
            for (int k = 0; k < 3; ++k) {                 // A J (columns p, q)
                const double akp = a[3 * k + p], akq = a[3 * k + q];
                a[3 * k + p] = c * akp - s * akq;
                a[3 * k + q] = s * akp + c * akq;
            }
            SHOT_UNROLL
            for (int k = 0; k < 3; ++k) {                 // J^T (A J) (rows p, q)
                const double apk = a[3 * p + k], aqk = a[3 * q + k];
                a[3 * p + k] = c * apk - s * aqk;
                a[3 * q + k] = s * apk + c * aqk;
            }
            SHOT_UNROLL
            for (int k = 0; k < 3; ++k) {                 // V J
                const double vkp = v[3 * k + p], vkq = v[3 * k + q];
                v[3 * k + p] = c * vkp - s * vkq;
                v[3 * k + q] = s * vkp + c * vkq;
            }
        }
    }
    for (int k = 0; k < 3; ++k) w[k] = a[4 * k];
}

// columns of the smallest and the largest eigenvalue (ties: the lower column for the smallest, the higher for the largest)
SHOT_HD void shot_extremes(const double w[3], int* lo, int* hi) {
    int a = 0, b = 0;
    for (int k = 1; k < 3; ++k) {
        if (w[k] < w[a]) a = k;
        if (!(w[k] < w[b])) b = k;
    }
    *lo = a; *hi = b;
}
