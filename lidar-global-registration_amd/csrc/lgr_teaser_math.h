// lgr_teaser_math.h -- the float arithmetic of the TEASER alignment ("TEASER"), stated once for the device kernels
// (lgr_teaser.hip) and the CPU statement of the tests (tests/cpp/teaser_ref.cpp), so that device == statement is a bit-for-bit claim:
//   teaser_edge        the compatibility test of two nodes, | |T_u T_v| - |S_u S_v| | <= 2 beta, false for a non-finite operand;
//   teaser_e2, teaser_residual, teaser_mu0, teaser_weight     the GNC-TLS rotation's scalars;
//   teaser_rotation    R from H = sum (w a) b^T by the library's 3x3 SVD and the refit's reflection fix (no centring).  The SVD is a
//                      parameter: lgr_svd3 (lgr_math.cuh) on the device, c_svd3 (oracle/src/orc_math.h, op for op the same) on the host;
//   teaser_end_key, teaser_key_value, teaser_tls_term         the per-axis TLS shift's sort key and cost term.
// Every operation is one IEEE binary32 + - * / sqrt; compile with -ffp-contract=off on both sides (the Makefile and the tests do).
//
// Edge cases the statement leaves open, decided here:
//   H == 0 (all TIMs 0): the SVD returns U = V = I, so R = I.
//   "All weights 0 keeps the last R" is a stop rule: an iteration whose new weights hold no w_k > 0 is the last one (checked after the
//       cost rule), so no solve ever sees an all-zero weight list.
//   max_k r_k is taken with "r > m ? r : m" from m = 0: a NaN residual never becomes the maximum.
//   rotation_cost is the last cost formed, 0 when the loop stopped at mu <= 0 before forming one.
//   End points that compare equal as floats (-0 == +0) sort as equal: the key canonicalises -0 to +0, and the centres are formed from
//       the keys' values.  A NaN end point sorts above every number; a centre next to it is NaN and has an empty consensus.
//   An axis without any non-empty consensus (only NaN or overflowing members): shift 0, cost = the member count.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TEASER_HD __host__ __device__ __forceinline__
#define TEASER_UNROLL _Pragma("unroll")
#else
#define TEASER_HD inline
#define TEASER_UNROLL
#endif

enum { TEASER_NODES_MAX = 2048 };   // == LGR_TEASER_NODES_MAX (include/lgr.h)

TEASER_HD uint32_t teaser_asuint(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
TEASER_HD float teaser_asfloat(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }

// len(v) = sqrtf((x*x + y*y) + z*z), correctly rounded (edge_len of lgr_gror_nodes.cuh)
TEASER_HD float teaser_len(float x, float y, float z) { return __builtin_sqrtf((x * x + y * y) + z * z); }

// A(u, v) for u != v; two_beta = 2.f * beta, formed once by the caller.  NaN <= x is false, inf - inf is NaN.
TEASER_HD bool teaser_edge(float sux, float suy, float suz, float tux, float tuy, float tuz, float svx, float svy, float svz, float tvx, float tvy,
                           float tvz, float two_beta) {
    const float lt = teaser_len(tux - tvx, tuy - tvy, tuz - tvz), ls = teaser_len(sux - svx, suy - svy, suz - svz);
    return __builtin_fabsf(lt - ls) <= two_beta;
}

TEASER_HD float teaser_e2(float two_beta) {
    const float e2 = two_beta * two_beta;
    return e2 < 1e-16f ? 1e-2f : e2;
}

// R row-major; (R a)_i = (R_i0 a0 + R_i1 a1) + R_i2 a2
TEASER_HD float teaser_rot_row(const float* R, int i, float a0, float a1, float a2) { return (R[3 * i] * a0 + R[3 * i + 1] * a1) + R[3 * i + 2] * a2; }

TEASER_HD float teaser_residual(const float* R, float a0, float a1, float a2, float b0, float b1, float b2) {
    const float d0 = b0 - teaser_rot_row(R, 0, a0, a1, a2), d1 = b1 - teaser_rot_row(R, 1, a0, a1, a2), d2 = b2 - teaser_rot_row(R, 2, a0, a1, a2);
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

TEASER_HD float teaser_max(float m, float r) { return r > m ? r : m; }

// mu of the first iteration; the caller stops when !(mu > 0)
TEASER_HD float teaser_mu0(float max_r, float e2) { return 1.f / ((2.f * max_r) / e2 - 1.f); }

TEASER_HD float teaser_weight(float r, float mu, float e2) {
    const float th1 = ((mu + 1.f) / mu) * e2, th2 = (mu / (mu + 1.f)) * e2;
    if (r >= th1) return 0.f;
    if (r <= th2) return 1.f;
    return __builtin_sqrtf(((e2 * mu) * (mu + 1.f)) / r) - mu;
}

TEASER_HD float teaser_det3(const float* M) {   // lgr_det3 / c_det3
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// H[3 r + s] = sum (w a[r]) b[s] -> R (row-major) with b ~ R a: H = U S V^T, R = V U^T, and with det R < 0 the third column of V
// negated (refit_kernel, src/transformation.cpp:27-33).  svd(A, U, S, V) is the library's 3x3 SVD.
template <class Svd>
TEASER_HD void teaser_rotation(const float* H, float* R, Svd svd) {
    float U[9], Sg[3], V[9];
    svd(H, U, Sg, V);
    TEASER_UNROLL for (int i = 0; i < 3; ++i)
        TEASER_UNROLL for (int j = 0; j < 3; ++j) R[3 * i + j] = (V[3 * i + 0] * U[3 * j + 0] + V[3 * i + 1] * U[3 * j + 1]) + V[3 * i + 2] * U[3 * j + 2];
    if (teaser_det3(R) < 0.f) {
        V[2] = -V[2]; V[5] = -V[5]; V[8] = -V[8];
        TEASER_UNROLL for (int i = 0; i < 3; ++i)
            TEASER_UNROLL for (int j = 0; j < 3; ++j) R[3 * i + j] = (V[3 * i + 0] * U[3 * j + 0] + V[3 * i + 1] * U[3 * j + 1]) + V[3 * i + 2] * U[3 * j + 2];
    }
}

// sort key of an interval end: (value ascending, lower end (kind 0) before upper end (kind 1), member k ascending)
TEASER_HD uint64_t teaser_end_key(float v, int kind, int k) {
    uint32_t b = teaser_asuint(v + 0.f);                        // -0 -> +0
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);             // order-preserving; NaNs (sign clear) above +inf
    return ((uint64_t) b << 32) | ((uint64_t) (kind & 1) << 16) | (uint64_t) (uint32_t) (k & 0xffff);
}
TEASER_HD float teaser_key_value(uint64_t key) {
    const uint32_t b = (uint32_t) (key >> 32);
    return teaser_asfloat((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}

TEASER_HD bool teaser_in_consensus(float x, float centre, float beta) { return __builtin_fabsf(x - centre) <= beta; }

// fminf(((x - xhat) / beta)^2, 1.f)
TEASER_HD float teaser_tls_term(float x, float xhat, float beta) {
    const float d = (x - xhat) / beta, q = d * d;
    return q < 1.f ? q : 1.f;
}
