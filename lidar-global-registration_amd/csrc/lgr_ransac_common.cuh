// lgr_ransac_common.cuh -- constants, small types and the hypothesis generator of the prerejective RANSAC (included by lgr_ransac.hip):
// the on-device Philox sampler (draws_n, select_n), the polygon prerejection, the NS-point Umeyama transform, the kernels that run them
// stand-alone (samples_kernel, hypotheses_kernel), the n_samples dispatch, LGR_APPLY and the packed-correspondence formats.
// Part of lgr_ransac.hip's one translation unit; see its header for the schedule and DESIGN.md section 5.
#pragma once
#include <climits>

#include "lgr_internal.h"
#include "lgr_math.cuh"

namespace {

constexpr int MIN_NR_INLIERS = 10;         // src/sac_prerejective_omp.cpp:8
constexpr int MIN_NR_FINAL_INLIERS = 20;   // :9
constexpr double MIN_INLIER_RATE = 0.15;   // :10

// ---------------------------------------------------------------------------------------------------- sampling
// src/sac_prerejective_omp.cpp:33-77 selectCorrespondences (control flow kept literally), NS = AlignmentParameters::n_samples
// The reference's loops (for i < NS: draw, for j < i: bump / wrap / insert-and-break) unrolled at compile time so that sample[] stays in
// registers (with run-time indices it lived in scratch memory).  `step` is one pass of the j loop's body at position j for the value x
// being placed: returns true for `continue` (x was bumped and stays the candidate for the next j), false for "insert x at j".
template <int NS>
__device__ __forceinline__ void select_n(const int (&r)[NS], int n_corr, int (&sample)[NS]) {
    auto step = [&](int& x, int sj) {
        if (x >= sj) {
            if (x < n_corr - 1) { x++; return true; }
            else if (sj == 0) { x = 1; return true; }
            else { x = 0; }
        }
        return false;
    };
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        int x = r[i] % n_corr;
        bool placed = false;
#pragma unroll
        for (int j = 0; j < i; ++j) {
            if (!placed && !step(x, sample[j])) {
#pragma unroll
                for (int k = i; k > j; --k) sample[k] = sample[k - 1];
                sample[j] = x;
                placed = true;
            }
        }
        if (!placed) sample[i] = x;
    }
}

// the raw draws of iteration `iter`: draw j = word j % 4 of Philox(seed; counter (iter, j / 4, 0, 0)), top 31 bits
template <int NS>
__device__ __forceinline__ void draws_n(unsigned long long seed, unsigned iter, int (&r)[NS]) {
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        if ((j & 3) == 0) lgr_philox4(seed, iter, (unsigned) (j >> 2), 0u, 0u, w);
        r[j] = (int) (w[j & 3] >> 1);
    }
}

template <int NS>
__global__ void samples_kernel(unsigned long long seed, int first, int n, int n_corr, int32_t* __restrict__ tuples) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    int r[NS], s[NS];
    draws_n<NS>(seed, (unsigned) (first + b), r);
    select_n<NS>(r, n_corr, s);
#pragma unroll
    for (int j = 0; j < NS; ++j) tuples[(size_t) NS * b + j] = s[j];
}

// ---------------------------------------------------------------------------------------------------- hypotheses
struct P3 { float x, y, z; };
__device__ __forceinline__ P3 ldp(const float* pts, int i) { const float* p = pts + (size_t) i * 12; return P3{p[0], p[1], p[2]}; }
__device__ __forceinline__ float p3c(const P3& p, int a) { return a == 0 ? p.x : (a == 1 ? p.y : p.z); }

// pcl::registration::CorrespondenceRejectorPoly::thresholdPolygon: every edge i -> (i + 1) % NS
template <int NS>
__device__ __forceinline__ bool poly_ok(const P3 (&s)[NS], const P3 (&t)[NS], float thr2) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int j = (i + 1) % NS;
        float dx = s[i].x - s[j].x, dy = s[i].y - s[j].y, dz = s[i].z - s[j].z;
        float ds = dx * dx + dy * dy + dz * dz;
        dx = t[i].x - t[j].x; dy = t[i].y - t[j].y; dz = t[i].z - t[j].z;
        float dt = dx * dx + dy * dy + dz * dz;
        float sim = ds < dt ? ds / dt : dt / ds;
        if (!(sim >= thr2)) return false;
    }
    return true;
}

// pcl::umeyama (no scaling) on NS pairs; T column-major.  Means and the entries of sigma are left-to-right sums over the points.
template <int NS>
__device__ __forceinline__ void umeyama_n(const P3 (&s)[NS], const P3 (&d)[NS], float* T) {
    const float one_over_n = 1.0f / (float) NS;
    float sm[3], dm[3], S[3][NS], D[3][NS];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float ss = p3c(s[0], a), ds = p3c(d[0], a);
#pragma unroll
        for (int j = 1; j < NS; ++j) { ss += p3c(s[j], a); ds += p3c(d[j], a); }
        sm[a] = ss * one_over_n;
        dm[a] = ds * one_over_n;
#pragma unroll
        for (int j = 0; j < NS; ++j) { S[a][j] = p3c(s[j], a) - sm[a]; D[a][j] = p3c(d[j], a) - dm[a]; }
    }
    float sigma[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float acc = D[i][0] * S[j][0];
#pragma unroll
            for (int k = 1; k < NS; ++k) acc += D[i][k] * S[j][k];
            sigma[3 * i + j] = one_over_n * acc;
        }
    float U[9], Sg[3], V[9];
    lgr_svd3(sigma, U, Sg, V);
    float sgn = (lgr_det3(U) * lgr_det3(V) < 0.f) ? -1.f : 1.f;
    float R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = (U[3 * i + 0] * V[3 * j + 0] + U[3 * i + 1] * V[3 * j + 1]) + (U[3 * i + 2] * sgn) * V[3 * j + 2];
    float t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = dm[i] - ((R[3 * i + 0] * sm[0] + R[3 * i + 1] * sm[1]) + R[3 * i + 2] * sm[2]);
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) T[4 * j + i] = R[3 * i + j];
        T[12 + i] = t[i];
    }
    T[15] = 1.f;
}

// one thread per iteration of the batch: sample (or replay a given tuple) -> prerejection -> NS-point transform
template <int NS>
__global__ void hypotheses_kernel(const float* __restrict__ src, const float* __restrict__ tgt, const lgr_corr* __restrict__ corr,
                                  int c, unsigned long long seed, int first, int n, const int32_t* __restrict__ tuples,
                                  float edge_thr, float* __restrict__ Ts, int* __restrict__ ok) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    int smp[NS];
    if (tuples) {
#pragma unroll
        for (int j = 0; j < NS; ++j) smp[j] = tuples[(size_t) NS * b + j];
    } else {
        int r[NS];
        draws_n<NS>(seed, (unsigned) (first + b), r);
        select_n<NS>(r, c, smp);
    }
    P3 s[NS], t[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) { lgr_corr cr = corr[smp[j]]; s[j] = ldp(src, cr.index_query); t[j] = ldp(tgt, cr.index_match); }   // buildIndices :17-31
    bool good = poly_ok<NS>(s, t, edge_thr * edge_thr);
    float T[16];
    if (good) umeyama_n<NS>(s, t, T);
    else {
#pragma unroll
        for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.f : 0.f;
    }
    float4* o = reinterpret_cast<float4*>(Ts + (size_t) b * 16);
    o[0] = make_float4(T[0], T[1], T[2], T[3]); o[1] = make_float4(T[4], T[5], T[6], T[7]);
    o[2] = make_float4(T[8], T[9], T[10], T[11]); o[3] = make_float4(T[12], T[13], T[14], T[15]);
    ok[b] = good ? 1 : 0;
}

// n_samples the kernels are instantiated for (the reference's sampler, polygon test and Umeyama are generic in it; every shipped config uses 3)
constexpr int LGR_MIN_SAMPLES = 3, LGR_MAX_SAMPLES = 8;
#define LGR_NS_DISPATCH(ns, CALL)                                                                                      \
    switch (ns) {                                                                                                      \
        case 3: { constexpr int NS = 3; CALL; break; }                                                                 \
        case 4: { constexpr int NS = 4; CALL; break; }                                                                 \
        case 5: { constexpr int NS = 5; CALL; break; }                                                                 \
        case 6: { constexpr int NS = 6; CALL; break; }                                                                 \
        case 7: { constexpr int NS = 7; CALL; break; }                                                                 \
        default: { constexpr int NS = 8; CALL; break; }                                                                \
    }

// T (column-major) applied as Eigen's Matrix4f * Vector4f on SSE: ((c0*x + c1*y) + c2*z) + c3
#define LGR_APPLY(T, sx, sy, sz, ox, oy, oz)                       \
    float ox = ((T[0] * sx + T[4] * sy) + T[8] * sz) + T[12];      \
    float oy = ((T[1] * sx + T[5] * sy) + T[9] * sz) + T[13];      \
    float oz = ((T[2] * sx + T[6] * sy) + T[10] * sz) + T[14];

// ---------------------------------------------------------------------------------------------------- packed correspondences
// PP (count_item's operand): one 64-byte record per TWO correspondences, {sx sy sz | qx qy qz | s* | band slope} as 2-vectors, padded
// with never-inlier fillers to a multiple of 64 correspondences; pstats = bit patterns of max |source coordinate|, max |target
// coordinate|, max finite s* (float max through integer atomics: all values >= 0).
constexpr int CP_FLOATS = 16;
typedef float v2f_c __attribute__((ext_vector_type(2)));
struct CPair { v2f_c sx, sy, sz, qx, qy, qz, ss, rs; };
static_assert(sizeof(CPair) == CP_FLOATS * 4, "pack_kernel writes this layout");

// what pack() leaves on the device: pack_kernel's P0 / P1 / sstar per correspondence, the pair records and their statistics
struct Packed { float4* P0; float4* P1; float* sstar; const CPair* PP; const unsigned* pstats; };

}  // namespace

// lgr_selfcheck_philox: one Philox4x32-10 block through the device's generator (known-answer tests)
__global__ void philox_kernel(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned* __restrict__ out) {
    unsigned w[4];
    lgr_philox4(seed, c0, c1, c2, c3, w);
    out[0] = w[0]; out[1] = w[1]; out[2] = w[2]; out[3] = w[3];
}
