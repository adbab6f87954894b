// lgr_rops_math.h -- the float arithmetic of the RoPS stage that has no IEEE-exact definition or that C++ leaves to the platform,
// stated once for the device kernels (lgr_rops.hip) and the CPU reference of the tests (tests/cpp/rops_ref.cpp), so that
// device == reference is a bit-for-bit statement:
//   rops_logf   GNU libc 2.35's logf (sysdeps/ieee754/flt-32/e_logf.c, from ARM's optimized-routines: a 16-entry {1/c, log c}
//               table and a degree-3 double polynomial) as the x86-64 build runs it on a CPU with FMA (the e_logf-fma ifunc
//               variant: GCC contracts every a * b + c of the source into one fused operation).  tests/test_rops_ref.py compares it
//               with the host's logf on every float of (0, 1];
//   rops_bin    static_cast<unsigned int>(float) as g++ compiles it on x86-64: cvttss2si into a 64-bit register, then the low 32 bits.
//               NaN and |r| >= 2^63 give the "integer indefinite" 0x8000000000000000, i.e. 0; otherwise trunc(r) modulo 2^32;
//   rops_dot3   Eigen's unvectorized 3-term reduction (Vector3f::dot, one row of Matrix3f * Vector3f): a0 b0 + (a1 b1 + a2 b2);
//   rops_cross  Eigen's generic cross product: (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), not normalized.
// std::pow(t, 1.f) and std::pow(t, 2.f) of computeCentralMoments are t and t * t (GCC folds a constant exponent that way).
// Compile with -ffp-contract=off on both sides (the Makefile and the tests do); fused operations are explicit (__builtin_fma).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ROPS_HD __host__ __device__ __forceinline__
#else
#define ROPS_HD inline
#endif

ROPS_HD uint32_t rops_asuint(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
ROPS_HD float rops_asfloat(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }

// logf_data.c: {invc, logc} of the 16 subintervals of [OFF, 2 OFF) (a switch, not an indexed local array: that would live in
// scratch memory on the device)
ROPS_HD void rops_logf_tab(int i, double* invc, double* logc) {
    switch (i) {
        case 0: *invc = 0x1.661ec79f8f3bep+0; *logc = -0x1.57bf7808caadep-2; return;
        case 1: *invc = 0x1.571ed4aaf883dp+0; *logc = -0x1.2bef0a7c06ddbp-2; return;
        case 2: *invc = 0x1.49539f0f010bp+0; *logc = -0x1.01eae7f513a67p-2; return;
        case 3: *invc = 0x1.3c995b0b80385p+0; *logc = -0x1.b31d8a68224e9p-3; return;
        case 4: *invc = 0x1.30d190c8864a5p+0; *logc = -0x1.6574f0ac07758p-3; return;
        case 5: *invc = 0x1.25e227b0b8eap+0; *logc = -0x1.1aa2bc79c81p-3; return;
        case 6: *invc = 0x1.1bb4a4a1a343fp+0; *logc = -0x1.a4e76ce8c0e5ep-4; return;
        case 7: *invc = 0x1.12358f08ae5bap+0; *logc = -0x1.1973c5a611cccp-4; return;
        case 8: *invc = 0x1.0953f419900a7p+0; *logc = -0x1.252f438e10c1ep-5; return;
        case 9: *invc = 0x1p+0; *logc = 0x0p+0; return;
        case 10: *invc = 0x1.e608cfd9a47acp-1; *logc = 0x1.aa5aa5df25984p-5; return;
        case 11: *invc = 0x1.ca4b31f026aap-1; *logc = 0x1.c5e53aa362eb4p-4; return;
        case 12: *invc = 0x1.b2036576afce6p-1; *logc = 0x1.526e57720db08p-3; return;
        case 13: *invc = 0x1.9c2d163a1aa2dp-1; *logc = 0x1.bc2860d22477p-3; return;
        case 14: *invc = 0x1.886e6037841edp-1; *logc = 0x1.1058bc8a07ee1p-2; return;
        default: *invc = 0x1.767dcf5534862p-1; *logc = 0x1.4043057b6ee09p-2; return;
    }
}

// e_logf.c for finite x > 0 (the only arguments RoPS passes: counts / N in (0, 1]); x <= 0, inf and NaN are not handled
ROPS_HD float rops_logf(float x) {
    // logf_data.c: ln 2 and the polynomial A[0..2]
    const double Ln2 = 0x1.62e42fefa39efp-1, A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
    const uint32_t OFF = 0x3f330000u;
    uint32_t ix = rops_asuint(x);
    if (ix == 0x3f800000u) return 0.f;
    if (ix < 0x00800000u) {                     // subnormal: normalize
        ix = rops_asuint(x * 0x1p23f);
        ix -= 23u << 23;
    }
    const uint32_t tmp = ix - OFF;
    const int i = (int) ((tmp >> (23 - 4)) % 16u);
    const int k = (int32_t) tmp >> 23;          // arithmetic shift
    const uint32_t iz = ix - (tmp & (0x1ffu << 23));
    double invc, logc;
    rops_logf_tab(i, &invc, &logc);
    const double z = (double) rops_asfloat(iz);
    const double r = __builtin_fma(z, invc, -1.0);
    const double y0 = __builtin_fma((double) k, Ln2, logc);
    const double r2 = r * r;
    double y = __builtin_fma(A1, r, A2);
    y = __builtin_fma(A0, r2, y);
    y = __builtin_fma(y, r2, y0 + r);
    return (float) y;
}

// static_cast<unsigned int>(r), x86-64 g++ (cvttss2si r64 + low half)
ROPS_HD uint32_t rops_bin(float r) {
    if (!(r > -0x1p63f && r < 0x1p63f)) return 0u;   // NaN, +-inf, out of the int64 range: 0x8000000000000000 -> 0
    return (uint32_t) (uint64_t) (int64_t) r;
}

ROPS_HD float rops_dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return a0 * b0 + (a1 * b1 + a2 * b2); }

ROPS_HD void rops_cross(const float a[3], const float b[3], float out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// rotateCloud's matrix about the unit axis e_axis (axis 0, 1, 2) by the angle with the given cosine / sine, entry for entry as
// the reference writes it (row-major out[9])
ROPS_HD void rops_rotation(int axis, float cosine, float sine, float out[9]) {
    const float x = axis == 0 ? 1.f : 0.f, y = axis == 1 ? 1.f : 0.f, z = axis == 2 ? 1.f : 0.f;
    out[0] = cosine + (1 - cosine) * x * x;     out[1] = (1 - cosine) * x * y - sine * z; out[2] = (1 - cosine) * x * z + sine * y;
    out[3] = (1 - cosine) * y * x + sine * z;   out[4] = cosine + (1 - cosine) * y * y;   out[5] = (1 - cosine) * y * z - sine * x;
    out[6] = (1 - cosine) * z * x - sine * y;   out[7] = (1 - cosine) * z * y + sine * x; out[8] = cosine + (1 - cosine) * z * z;
}

// the cell of one projected point: getDistributionMatrix's (row, col) with 'row == bins -> bins - 1', as the linear index into the
// column-major 5 x 5 matrix (row + 5 col); >= 25 only for boxes whose bin length underflows to a subnormal (the reference then writes
// outside its matrix); the callers drop such points
ROPS_HD uint64_t rops_cell(float u_ratio, float v_ratio) {
    uint32_t row = rops_bin(u_ratio), col = rops_bin(v_ratio);
    if (row == 5u) row--;
    if (col == 5u) col--;
    return (uint64_t) row + 5ull * (uint64_t) col;
}

// computeCentralMoments of one 5 x 5 distribution matrix given as counts (column-major, cnt[i + 5 j]) of n points:
// m = cnt / max(1, n); mean_i, mean_j; the moments (1,1), (2,1), (1,2), (2,2) and the entropy, in the reference's (i, j) order
ROPS_HD void rops_moments(const uint32_t* cnt, uint32_t n, float out5[5]) {
    const float div = n > 1u ? (float) n : 1.f;
    float mean_i = 0.f, mean_j = 0.f;
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) {
            const float m = (float) cnt[i + 5 * j] / div;
            mean_i += (float) (i + 1) * m;
            mean_j += (float) (j + 1) * m;
        }
    float m11 = 0.f, m21 = 0.f, m12 = 0.f, m22 = 0.f, entropy = 0.f;
    for (int i = 0; i < 5; ++i) {
        const float fi = (float) (i + 1) - mean_i;
        for (int j = 0; j < 5; ++j) {
            const float fj = (float) (j + 1) - mean_j;
            const float m = (float) cnt[i + 5 * j] / div;
            if (m > 0.f) entropy -= m * rops_logf(m);
            m11 += fi * fj * m;
            m21 += (fi * fi) * fj * m;
            m12 += fi * (fj * fj) * m;
            m22 += (fi * fi) * (fj * fj) * m;
        }
    }
    out5[0] = m11; out5[1] = m21; out5[2] = m12; out5[3] = m22; out5[4] = entropy;
}
