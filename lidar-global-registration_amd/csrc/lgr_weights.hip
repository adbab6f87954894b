// lgr_weights.hip -- the point weights of the weighted_closest_plane metric (reference src/weights.cpp, src/metric.cpp:202-231) for gfx950.
//
//   WeightedClosestPlaneMetricEstimator::setSourceCloud: weights = getWeightFunction(weight_id)(NORMAL_NR_POINTS = 30, src),
//   weights_sum = sequential f32 sum in index order.  Built: constant, curvature (HarrisKeypoint3D CURVATURE without non-maximum
//   suppression = the normals' curvature field, non-finite -> 0), exp_curvature and curvedness (pcl::PrincipalCurvaturesEstimation
//   with setKSearch(30) on the cloud itself), nss (normal-space histogram).  harris / tomasi: LGR_ERR_UNSUPPORTED.
//
// Canonical choices: the k nearest neighbours in (distance, index) order (lgr_knn_lists, as the normals
// stage), PCL 1.12.1 computePointPrincipalCurvatures op for op with pcl::eigen33's scaled computeRoots of lgr_libm.cuh; the
// scalar functions of lgr_weights_math.h (glibc expf, findBin into 251 bins, the quantile formula) and glibc logf (lgr_rops_math.h).
//
// Kernels: principal curvatures (one thread per point over its neighbour list), the 0.8 quantile (the radix sort of lgr_sort.hip on
// the order-preserving bits of max(pc1, pc2), one thread for the double formula), the NSS histogram (integer atomics), the per-point
// maps, and the sum (one workgroup: tiles staged in LDS, one lane adds them in index order; every lane folds a max).
#include <algorithm>
#include <cmath>

#include "lgr_grid.cuh"
#include "lgr_host.h"
#include "lgr_internal.h"
#include "lgr_libm.cuh"
#include "lgr_seqsum.h"
#include "lgr_rops_math.h"
#include "lgr_weights_math.h"

namespace {

constexpr int WB = 256;
constexpr int NORMAL_NR_POINTS = 30;   // include/common.h: the macro setSourceCloud passes (not AlignmentParameters::normal_nr_points)

__device__ __forceinline__ float wt_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return a0 * b0 + (a1 * b1 + a2 * b2);   // Eigen's unvectorized 3-term reduction (one row of Matrix3f * Vector3f)
}

// PCL 1.12.1 PrincipalCurvaturesEstimation::computePointPrincipalCurvatures for point i over its neighbour list nbr[i * k ..] (-1 past the
// end: fewer than k points in the cloud).  A non-finite query point or an empty list gives NaN (computeFeature's rule).
__global__ __launch_bounds__(WB) void pc_kernel(const float* __restrict__ pts, int n, const int* __restrict__ nbr, int k,
                                                float* __restrict__ pc1_out, float* __restrict__ pc2_out) {
    const int i = blockIdx.x * WB + threadIdx.x;
    if (i >= n) return;
    const float* q = pts + (size_t) i * 12;
    const int* L = nbr + (size_t) i * k;
    int m = 0;
    while (m < k && L[m] >= 0) ++m;
    if (!lgr_finite3(q[0], q[1], q[2]) || m == 0) { pc1_out[i] = __uint_as_float(0x7fc00000u); pc2_out[i] = __uint_as_float(0x7fc00000u); return; }
    const float n0 = q[4], n1 = q[5], n2 = q[6];
    // M = I - n n^T (row-major; symmetric)
    const float M00 = 1.f - n0 * n0, M01 = 0.f - n0 * n1, M02 = 0.f - n0 * n2;
    const float M10 = 0.f - n1 * n0, M11 = 1.f - n1 * n1, M12 = 0.f - n1 * n2;
    const float M20 = 0.f - n2 * n0, M21 = 0.f - n2 * n1, M22 = 1.f - n2 * n2;
    auto project = [&](int j, float& p0, float& p1, float& p2) {
        const float* v = pts + (size_t) L[j] * 12 + 4;
        const float v0 = v[0], v1 = v[1], v2 = v[2];
        p0 = wt_dot3(M00, M01, M02, v0, v1, v2);
        p1 = wt_dot3(M10, M11, M12, v0, v1, v2);
        p2 = wt_dot3(M20, M21, M22, v0, v1, v2);
    };
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    for (int j = 0; j < m; ++j) {
        float p0, p1, p2;
        project(j, p0, p1, p2);
        c0 += p0; c1 += p1; c2 += p2;
    }
    const float fm = (float) m;
    c0 /= fm; c1 /= fm; c2 /= fm;
    float C00 = 0.f, C01 = 0.f, C02 = 0.f, C11 = 0.f, C12 = 0.f, C22 = 0.f;
    for (int j = 0; j < m; ++j) {   // (the projections again: the same operations give the same values)
        float p0, p1, p2;
        project(j, p0, p1, p2);
        const float d0 = p0 - c0, d1 = p1 - c1, d2 = p2 - c2;
        C00 += d0 * d0; C01 += d0 * d1; C02 += d0 * d2;   // (float) (double) (d0 * d1) is d0 * d1
        C11 += d1 * d1; C12 += d1 * d2; C22 += d2 * d2;
    }
    // pcl::eigen33(covariance, eigenvalues): scale by the largest |entry|, computeRoots, scale back
    const float C[9] = {C00, C01, C02, C01, C11, C12, C02, C12, C22};
    float scale = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) scale = fmaxf(scale, fabsf(C[t]));
    if (scale <= 1.17549435e-38f) scale = 1.f;
    float s[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) s[t] = C[t] / scale;
    float r0, r1, r2;
    lgr_pcl_roots3(s, r0, r1, r2);
    (void) r0;
    const float inv = 1.0f / fm;   // indices_size
    pc1_out[i] = (r2 * scale) * inv;
    pc2_out[i] = (r1 * scale) * inv;
}

__device__ __forceinline__ float wt_max_pc(float pc1, float pc2) {
    const bool fin = isfinite(pc1) && isfinite(pc2);
    return fin ? (pc1 < pc2 ? pc2 : pc1) : 0.f;   // std::max(pc1, pc2)
}
// (wt_key / wt_unkey, the order-preserving bits of a float, are in lgr_weights_math.h)

__global__ __launch_bounds__(WB) void maxpc_key_kernel(const float* __restrict__ pc1, const float* __restrict__ pc2, int n, unsigned* __restrict__ keys) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) keys[i] = wt_key(wt_max_pc(pc1[i], pc2[i]));
}

// lambda = logf(1.05f) * quantile(0.8, max_pcs), from the sorted keys
__global__ void lambda_kernel(const unsigned* __restrict__ sorted, int n, float* __restrict__ lambda) {
    long long i, j;
    wt_quantile_ranks(n, &i, &j);
    const float q = wt_quantile(n, i, j, wt_unkey(sorted[i]), wt_unkey(sorted[j]));
    *lambda = rops_logf(1.05f) * q;
}

__device__ __forceinline__ bool wt_normal_finite(const float* p) { return isfinite(p[4]) && isfinite(p[5]) && isfinite(p[6]); }
__device__ __forceinline__ int wt_bin_of(const float* p) {
    return wt_nss_bin(lgr_glibc::acosf_(p[6]), lgr_glibc::atan2f_(p[5], p[4]));
}

__global__ __launch_bounds__(WB) void nss_hist_kernel(const float* __restrict__ pts, int n, int* __restrict__ hist, int* __restrict__ bins) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float* p = pts + (size_t) i * 12;
        int b = -1;
        if (wt_normal_finite(p)) b = wt_bin_of(p);
        bins[i] = b;
        if (b >= 0) atomicAdd(&hist[b], 1);
    }
}

__global__ __launch_bounds__(WB) void weights_map_kernel(int weight_id, const float* __restrict__ pts, int n, const float* __restrict__ pc1, const float* __restrict__ pc2,
                                   const float* __restrict__ lambda, const int* __restrict__ hist, const int* __restrict__ bins, float* __restrict__ w) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float v;
        if (weight_id == LGR_WEIGHT_CONSTANT) {
            v = 1.f;
        } else if (weight_id == LGR_WEIGHT_CURVATURE) {
            const float c = pts[(size_t) i * 12 + 9];
            v = isfinite(c) ? c : 0.f;
        } else if (weight_id == LGR_WEIGHT_EXP_CURVATURE) {
            const float mp = wt_max_pc(pc1[i], pc2[i]);
            v = mp == 0.f ? 0.f : wt_expf(-*lambda / mp);
        } else if (weight_id == LGR_WEIGHT_CURVEDNESS) {
            const float a = pc1[i], b = pc2[i];
            v = (isfinite(a) && isfinite(b)) ? rops_logf(__builtin_sqrtf((a * a + b * b) / 2.f) + 1.f) : 0.f;
        } else {   // nss
            const int b = bins[i];
            v = b >= 0 ? 1.f / (float) hist[b] / 64.f : 0.f;
        }
        w[i] = v;
    }
}

// out[0] = sequential f32 sum in index order, out[1] = max (NaN ignored), out[2] = number of non-finite weights (as a float).
// One workgroup, tiles double-buffered in LDS: lane 0 adds tile k in index order (float4 reads, the adds one dependent chain) while
// waves 1-3 stage tile k + 1 and fold the max / count of what they load.
constexpr int SUM_TILE = 4096;
__global__ __launch_bounds__(WB) void seq_sum_kernel(const float* __restrict__ w, int n, float* __restrict__ out) {
    __shared__ float4 tile[2][SUM_TILE / 4];
    __shared__ float s_max[WB / 64];
    __shared__ int s_bad[WB / 64];
    float sum = 0.f, mx = -INFINITY;
    int bad = 0;
    auto stage = [&](int b, int k, int t0, int stride) {
        float* dst = (float*) tile[k];
        const int len = min(SUM_TILE, n - b);
        for (int t = t0; t < len; t += stride) {
            const float v = w[b + t];
            dst[t] = v;
            mx = fmaxf(mx, v);
            bad += isfinite(v) ? 0 : 1;
        }
    };
    stage(0, 0, threadIdx.x, WB);
    __syncthreads();
    int k = 0;
    for (int b = 0; b < n; b += SUM_TILE, k ^= 1) {
        if (threadIdx.x >= 64) {
            if (b + SUM_TILE < n) stage(b + SUM_TILE, k ^ 1, threadIdx.x - 64, WB - 64);
        } else if (threadIdx.x == 0) {
            const int len = min(SUM_TILE, n - b), n4 = len >> 2;
            const float4* t = tile[k];
#pragma unroll 8
            for (int q = 0; q < n4; ++q) {
                const float4 v = t[q];
                sum += v.x; sum += v.y; sum += v.z; sum += v.w;
            }
            for (int r = 4 * n4; r < len; ++r) sum += ((const float*) t)[r];
        }
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o)); bad += __shfl_xor(bad, o); }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = mx; s_bad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < WB / 64; ++t) { mx = fmaxf(mx, s_max[t]); bad += s_bad[t]; }
        out[0] = sum; out[1] = mx; out[2] = (float) bad;
    }
}

int check_weight_id(lgr_ctx* ctx, int weight_id) {
    LGR_CHECK(ctx, weight_id >= LGR_WEIGHT_CONSTANT && weight_id <= LGR_WEIGHT_NSS, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, weight_id != LGR_WEIGHT_HARRIS && weight_id != LGR_WEIGHT_TOMASI, LGR_ERR_UNSUPPORTED);
    return LGR_OK;
}

int pcs_launch(lgr_ctx* ctx, const float* d_pts, int n, int k, float* d_pc1, float* d_pc2) {
    LGR_CHECK(ctx, k >= 1, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, k <= 128, LGR_ERR_UNSUPPORTED);   // (the k-NN lists' limit)
    int* nbr;
    LGR_TRY(lgr_ws_t(ctx, WS_WEIGHTS_KNN, (size_t) n * k + 1, &nbr));
    LGR_TRY(lgr_knn_lists(ctx, d_pts, n, d_pts, n, k, nbr, nullptr));
    pc_kernel<<<cdiv(n, WB), WB, 0, ctx->stream>>>(d_pts, n, nbr, k, d_pc1, d_pc2);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

}  // namespace

// the weight map of weight_id into d_w (n floats), on ctx->stream
int lgr_weights_map(lgr_ctx* ctx, const float* d_pts, int n, int weight_id, int nr_points, float* d_w) {
    LGR_TRY(check_weight_id(ctx, weight_id));
    LGR_CHECK(ctx, n > 0 && d_pts && d_w, LGR_ERR_INVALID_ARG);
    const int grid = std::min(cdiv(n, WB), 8 * std::max(1, ctx->n_cu));
    float* pc1 = nullptr;
    float* pc2 = nullptr;
    float* lambda = nullptr;
    int* hist = nullptr;
    int* bins = nullptr;
    char* tmp;
    const size_t nn = ((size_t) n + 63) & ~(size_t) 63;
    LGR_TRY(lgr_ws_t(ctx, WS_WEIGHTS_TMP, 4 * nn * 4 + 4096, &tmp));
    if (weight_id == LGR_WEIGHT_EXP_CURVATURE || weight_id == LGR_WEIGHT_CURVEDNESS) {
        pc1 = (float*) tmp; pc2 = pc1 + nn;
        LGR_TRY(pcs_launch(ctx, d_pts, n, nr_points, pc1, pc2));
        if (weight_id == LGR_WEIGHT_EXP_CURVATURE) {
            unsigned* keys = (unsigned*) (pc2 + nn);
            unsigned* sorted = keys + nn;
            int* vals;
            LGR_TRY(lgr_ws_t(ctx, WS_WEIGHTS_VALS, 2 * nn + 64, &vals));
            lambda = (float*) (vals + 2 * nn);
            maxpc_key_kernel<<<grid, WB, 0, ctx->stream>>>(pc1, pc2, n, keys);
            LGR_TRY(lgr_sort_pairs_u32(ctx, keys, sorted, vals, vals + nn, (size_t) n, 0, 32));
            lambda_kernel<<<1, 1, 0, ctx->stream>>>(sorted, n, lambda);
        }
    } else if (weight_id == LGR_WEIGHT_NSS) {
        bins = (int*) tmp;
        hist = bins + nn;
        LGR_HIP(ctx, hipMemsetAsync(hist, 0, WT_NSS_BINS * 4, ctx->stream));
        nss_hist_kernel<<<grid, WB, 0, ctx->stream>>>(d_pts, n, hist, bins);
    }
    weights_map_kernel<<<grid, WB, 0, ctx->stream>>>(weight_id, d_pts, n, pc1, pc2, lambda, hist, bins, d_w);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// weights_sum (sequential f32 sum in index order), the largest weight and the number of non-finite weights of d_w; synchronises
int lgr_weights_sum(lgr_ctx* ctx, const float* d_w, int n, float* sum, float* w_max, int* n_bad) {
    float* d_out;
    LGR_TRY(lgr_ws_t(ctx, WS_WEIGHTS_SUM, 16, &d_out));
    seq_sum_kernel<<<1, WB, 0, ctx->stream>>>(d_w, n, d_out);
    LGR_HIP(ctx, hipGetLastError());
    float* h;
    LGR_TRY(lgr_pinned(ctx, 64, (void**) &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, d_out, 12, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *sum = h[0]; *w_max = h[1]; *n_bad = (int) h[2];
    return LGR_OK;
}

// the weights of a RANSAC run under weighted_closest_plane (mp NULL: the defaults = constant); d_w stays valid until the next call
int lgr_weights_prepare(lgr_ctx* ctx, const float* d_src, int ns, const lgr_metric_params* mp, const float** d_w, float* w_sum, float* w_gate) {
    lgr_metric_params def;
    lgr_default_metric_params(&def);
    if (!mp) mp = &def;
    float* w = nullptr;
    if (mp->weights) {
        w = const_cast<float*>(mp->weights);
    } else {
        LGR_TRY(check_weight_id(ctx, mp->weight_id));
        LGR_TRY(lgr_ws_t(ctx, WS_WEIGHTS, (size_t) ns + 64, &w));
        if (mp->weight_id == LGR_WEIGHT_CONSTANT) {   // all ones: the sum without the chain of adds (lgr_seqsum.h)
            LGR_TRY(lgr_weights_map(ctx, d_src, ns, LGR_WEIGHT_CONSTANT, NORMAL_NR_POINTS, w));
            *d_w = w; *w_sum = lgr_seqsum(1.0f, ns); *w_gate = 1.f;
            return LGR_OK;
        }
        LGR_TRY(lgr_weights_map(ctx, d_src, ns, mp->weight_id, NORMAL_NR_POINTS, w));
    }
    float mx;
    int bad;
    LGR_TRY(lgr_weights_sum(ctx, w, ns, w_sum, &mx, &bad));
    LGR_CHECK(ctx, bad == 0, LGR_ERR_INVALID_ARG);   // caller weights must be finite (the built maps always are)
    *d_w = w;
    *w_gate = std::max(mx, 0.f);
    return LGR_OK;
}

extern "C" void lgr_default_metric_params(lgr_metric_params* m) {
    if (!m) return;
    memset(m, 0, sizeof(*m));
    m->weight_id = LGR_WEIGHT_CONSTANT;   // include/common.h:150
    m->weights = nullptr;
}

extern "C" int lgr_principal_curvatures_dev(lgr_ctx* ctx, const float* d_pts, int n, int k, float* d_pc1, float* d_pc2) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && (d_pts || n == 0) && (d_pc1 || n == 0) && (d_pc2 || n == 0), LGR_ERR_INVALID_ARG);
    if (n == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    LGR_TRY(pcs_launch(ctx, d_pts, n, k, d_pc1, d_pc2));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_principal_curvatures(lgr_ctx* ctx, const float* pts, int n, int k, float* pc1, float* pc2) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && (pts || n == 0) && (pc1 || n == 0) && (pc2 || n == 0), LGR_ERR_INVALID_ARG);
    if (n == 0) return LGR_OK;
    float *dp, *d1, *d2;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(pts, (size_t) n * 12, &dp));
    LGR_TRY(hc.out((size_t) n, &d1));
    LGR_TRY(hc.out((size_t) n, &d2));
    LGR_TRY(lgr_principal_curvatures_dev(ctx, dp, n, k, d1, d2));
    LGR_TRY(hc.fetch(pc1, d1, (size_t) n));
    LGR_TRY(hc.fetch(pc2, d2, (size_t) n));
    return hc.finish();
}

extern "C" int lgr_weights_dev(lgr_ctx* ctx, const float* d_pts, int n, int weight_id, int nr_points, float* d_out, float* weights_sum) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_TRY(check_weight_id(ctx, weight_id));
    LGR_CHECK(ctx, n >= 0 && (d_pts || n == 0) && (d_out || n == 0), LGR_ERR_INVALID_ARG);
    if (n == 0) {
        if (weights_sum) *weights_sum = 0.f;
        return LGR_OK;
    }
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    LGR_TRY(lgr_weights_map(ctx, d_pts, n, weight_id, nr_points, d_out));
    if (weights_sum) {
        float mx;
        int bad;
        LGR_TRY(lgr_weights_sum(ctx, d_out, n, weights_sum, &mx, &bad));
    }
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_weights(lgr_ctx* ctx, const float* pts, int n, int weight_id, int nr_points, float* out, float* weights_sum) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_TRY(check_weight_id(ctx, weight_id));
    LGR_CHECK(ctx, n >= 0 && (pts || n == 0) && (out || n == 0), LGR_ERR_INVALID_ARG);
    if (n == 0) {
        if (weights_sum) *weights_sum = 0.f;
        return LGR_OK;
    }
    float *dp, *dw;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(pts, (size_t) n * 12, &dp));
    LGR_TRY(hc.out((size_t) n, &dw));
    LGR_TRY(lgr_weights_dev(ctx, dp, n, weight_id, nr_points, dw, weights_sum));
    LGR_TRY(hc.fetch(out, dw, (size_t) n));
    return hc.finish();
}

// lgr.h: the expf / logf restatements element-wise on the device (lgr_selfcheck_libm fn 5 / 6)
__global__ __launch_bounds__(256) void wt_libm_kernel(int fn, const float* __restrict__ a, long long n, float* __restrict__ out) {
    for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
        out[i] = fn == 5 ? wt_expf(a[i]) : rops_logf(a[i]);
}
int lgr_weights_libm_launch(lgr_ctx* ctx, int fn, const float* d_a, long long n, float* d_out) {
    wt_libm_kernel<<<8 * std::max(1, ctx->n_cu), 256, 0, ctx->stream>>>(fn, d_a, n, d_out);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}
