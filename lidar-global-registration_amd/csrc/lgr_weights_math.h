// lgr_weights_math.h -- the scalar pieces of the point-weight functions behind weighted_closest_plane (reference src/weights.cpp),
// stated once for the device kernels (lgr_weights.hip) and the CPU statement of the tests (tests/cpp/weights_ref.cpp), so that the
// declared choices of DESIGN.md section 4 are one text:
//   wt_expf     GNU libc 2.35's expf (sysdeps/ieee754/flt-32/e_expf.c, from ARM's optimized-routines: a 32-entry 2^(i/32) table and a
//               degree-3 double polynomial) as the x86-64 build runs it on a CPU with FMA (the e_expf-fma ifunc variant: GCC fuses
//               InvLn2N * x into BOTH of its uses, kd = fma(InvLn2N, x, SHIFT) and r = fma(InvLn2N, x, -kd), and every a * b + c of
//               the polynomial).  Underflow goes through the same path down to x = -0x1.9fe368p6 (subnormal results rounded once
//               from double), below that 0.  tests/test_weights_ref.py compares it with the host's expf on every float <= 0;
//   wt_nss_bin  findBin (src/weights.cpp:145-157) with the comparisons against the double M_PI kept as written (never true for a float),
//               into 251 bins (floor(theta * 8) * 8 + floor(phi * 8) reaches 25 * 8 + 50); a NaN polar angle (|nz| > 1) gives -1: the
//               point is not counted and weighs 0.  acosf / atan2f are the caller's (the device's restatement or the host libm);
//   wt_quantile utils.h quantile<float>(0.8, v) from its i-th and j-th smallest values: ith (n q - i) + jth (j - n q) in double.
// logf is rops_logf (lgr_rops_math.h).  Compile with -ffp-contract=off on both sides; fused operations are explicit.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define WT_HD __host__ __device__ __forceinline__
#else
#define WT_HD inline
#endif

// e_exp2f_data.c: tab[i] = bits(2^(i/32)) - (i << 47) (a switch, not an indexed local array: that would live in scratch on the device)
WT_HD uint64_t wt_exp2f_tab(int i) {
    switch (i) {
        case 0: return 0x3ff0000000000000ull; case 1: return 0x3fefd9b0d3158574ull; case 2: return 0x3fefb5586cf9890full; case 3: return 0x3fef9301d0125b51ull;
        case 4: return 0x3fef72b83c7d517bull; case 5: return 0x3fef54873168b9aaull; case 6: return 0x3fef387a6e756238ull; case 7: return 0x3fef1e9df51fdee1ull;
        case 8: return 0x3fef06fe0a31b715ull; case 9: return 0x3feef1a7373aa9cbull; case 10: return 0x3feedea64c123422ull; case 11: return 0x3feece086061892dull;
        case 12: return 0x3feebfdad5362a27ull; case 13: return 0x3feeb42b569d4f82ull; case 14: return 0x3feeab07dd485429ull; case 15: return 0x3feea47eb03a5585ull;
        case 16: return 0x3feea09e667f3bcdull; case 17: return 0x3fee9f75e8ec5f74ull; case 18: return 0x3feea11473eb0187ull; case 19: return 0x3feea589994cce13ull;
        case 20: return 0x3feeace5422aa0dbull; case 21: return 0x3feeb737b0cdc5e5ull; case 22: return 0x3feec49182a3f090ull; case 23: return 0x3feed503b23e255dull;
        case 24: return 0x3feee89f995ad3adull; case 25: return 0x3feeff76f2fb5e47ull; case 26: return 0x3fef199bdd85529cull; case 27: return 0x3fef3720dcef9069ull;
        case 28: return 0x3fef5818dcfba487ull; case 29: return 0x3fef7c97337b9b5full; case 30: return 0x3fefa4afa2a490daull; default: return 0x3fefd0765b6e4540ull;
    }
}
// e_expf.c (WANT_ERRNO_UFLOW 0, TOINT_INTRINSICS 0)
WT_HD float wt_expf(float x) {
    uint32_t ux;
    __builtin_memcpy(&ux, &x, 4);
    const uint32_t abstop = (ux >> 20) & 0x7ffu;
    if (abstop >= 0x42bu) {                       // |x| >= 88 (top12(88.0f)) or NaN
        if (ux == 0xff800000u) return 0.f;        // -inf
        if (abstop >= 0x7f8u) return x + x;       // +inf, NaN
        if (x > 0x1.62e42ep6f) return 0x1p97f * 0x1p97f;     // __math_oflowf: +inf
        if (x < -0x1.9fe368p6f) return 0x1p-95f * 0x1p-95f;  // __math_uflowf: +0
    }
    const double InvLn2N = 0x1.71547652b82fep+0 * 32.0, SHIFT = 0x1.8p+52;
    const double C0 = 0x1.c6af84b912394p-5 / 32.0 / 32.0 / 32.0, C1 = 0x1.ebfce50fac4f3p-3 / 32.0 / 32.0, C2 = 0x1.62e42ff0c52d6p-1 / 32.0;
    const double xd = (double) x;
    double kd = __builtin_fma(InvLn2N, xd, SHIFT);
    uint64_t ki;
    __builtin_memcpy(&ki, &kd, 8);
    kd -= SHIFT;
    const double r = __builtin_fma(InvLn2N, xd, -kd);
    uint64_t t = wt_exp2f_tab((int) (ki % 32u));
    t += ki << (52 - 5);
    double s;
    __builtin_memcpy(&s, &t, 8);
    const double z = __builtin_fma(C0, r, C1);
    const double r2 = r * r;
    double y = __builtin_fma(C2, r, 1.0);
    y = __builtin_fma(z, r2, y);
    y = y * s;
    return (float) y;
}

constexpr int WT_NSS_BINS = 251;

// theta = acosf(nz), at = atan2f(ny, nx) of a finite normal
WT_HD int wt_nss_bin(float theta, float at) {
    const double PI = 3.14159265358979323846;
    float phi = (float) fmod((double) at + 2.f * PI, 2.f * PI);
    const float PI_F = (float) PI, TWO_PI_F = (float) (2.f * PI);
    theta = theta < 0.f ? 0.f : theta;            // std::max(theta, 0.f)
    theta = PI_F < theta ? PI_F : theta;          // std::min(., (float) M_PI)
    phi = phi < 0.f ? 0.f : phi;
    phi = TWO_PI_F < phi ? TWO_PI_F : phi;
    if ((double) theta == PI) theta = 0.f;        // (never true for a float)
    if ((double) phi == 2.f * PI) phi = 0.f;      // (never true for a float)
    if (theta != theta) return -1;                // |nz| > 1: acosf is NaN (declared: not counted, weight 0)
    return (int) (floorf(theta * 8.f) * 8.f + floorf(phi * 8.f));
}

// order-preserving bits of a float (ascending keys <-> ascending values; -0 below +0, NaNs at the two ends) and back
WT_HD uint32_t wt_key(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
WT_HD float wt_unkey(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// utils.h quantile<float>(q, v) for any q in [0, 1] (saveColorizedWeights takes 0.01 and 0.99), same ranks and same formula
WT_HD void wt_quantile_ranks_q(double q, long long n, long long* i, long long* j) {
    *i = (long long) floor(q * (double) (n - 1));
    *j = *i + 1 < n - 1 ? *i + 1 : n - 1;
}
WT_HD float wt_quantile_q(double q, long long n, long long i, long long j, float ith, float jth) {
    if (n == 1) return ith;
    if (i < j) return (float) ((double) ith * ((double) n * q - (double) i) + (double) jth * ((double) j - (double) n * q));
    return ith;
}

// quantile(0.8, v) of n >= 1 values from the i-th and j-th smallest (i = floor(0.8 (n - 1)), j = min(i + 1, n - 1))
WT_HD void wt_quantile_ranks(long long n, long long* i, long long* j) {
    *i = (long long) floor(0.8 * (double) (n - 1));
    *j = *i + 1 < n - 1 ? *i + 1 : n - 1;
}
WT_HD float wt_quantile(long long n, long long i, long long j, float ith, float jth) {
    if (n == 1) return ith;
    if (i < j) return (float) ((double) ith * ((double) n * 0.8 - (double) i) + (double) jth * ((double) j - (double) n * 0.8));
    return ith;
}
