// lgr_pointpass.cuh -- what the thread-per-point passes of lgr_analysis.hip, lgr_plane_dense.hip and lgr_debug.hip share: PCL's point
// moves, the wave-aggregated counter, the sequential f32 sum jobs, the move of a whole cloud and
// the compaction of an overlap cloud (flags, their exclusive scan, the kept rows).  Its host helpers are the read-back of a few words
// (read_words) and the scan of 0 / 1 flags (pp_scan_flags); host arrays are staged by lgr_host.h, not here.  Everything here sits in an
// unnamed namespace: each translation unit gets its own copy of the kernels.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "lgr_grid.cuh"
#include "lgr_internal.h"

namespace {

constexpr int PP_BLOCK = 256;

// pcl::detail::Transformer::se3 / so3
__device__ __forceinline__ void se3(const float* __restrict__ M, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = M[0] * x + (M[4] * y + (M[8] * z + M[12]));
    oy = M[1] * x + (M[5] * y + (M[9] * z + M[13]));
    oz = M[2] * x + (M[6] * y + (M[10] * z + M[14]));
}
__device__ __forceinline__ void so3(const float* __restrict__ M, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = M[0] * x + (M[4] * y + M[8] * z);
    oy = M[1] * x + (M[5] * y + M[9] * z);
    oz = M[2] * x + (M[6] * y + M[10] * z);
}
__device__ __forceinline__ float sq3(float x, float y, float z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
__device__ __forceinline__ bool fin(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

__device__ __forceinline__ void wave_count(bool f, int* counter) {
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, __popcll(m));
}

// Sequential f32 sums in index order, one workgroup per job: lane 0 adds tile k (one dependent chain, float4 reads from LDS) while waves
// 1-3 stage tile k + 1.  sq: the term is v * v (the squared smoothed densities of src/analysis.cpp:232).
constexpr int GT_SUM_TILE = 4096, GT_SUM_JOBS = 4, GT_SUM_JOBS_WIDE = 16;
struct GtSumJobs { const float* p[GT_SUM_JOBS]; int n[GT_SUM_JOBS]; int sq[GT_SUM_JOBS]; };
// the jobs of one chunk of a batched evaluation (lgr_evaluate_gt_batch_dev: two sums per transform), every one over n terms
struct GtSumJobsWide { const float* p[GT_SUM_JOBS_WIDE]; int n; };
// one job, by the whole workgroup; the sum is lane 0's return value
__device__ __forceinline__ float gt_seqsum_job(const float* __restrict__ w, const int n, const bool sq) {
    __shared__ float4 tile[2][GT_SUM_TILE / 4];
    float sum = 0.f;
    auto stage = [&](int b, int k, int t0, int stride) {
        float* dst = (float*) tile[k];
        const int len = min(GT_SUM_TILE, n - b);
        for (int t = t0; t < len; t += stride) {
            const float v = w[b + t];
            dst[t] = sq ? v * v : v;
        }
    };
    stage(0, 0, threadIdx.x, PP_BLOCK);
    __syncthreads();
    int k = 0;
    for (int b = 0; b < n; b += GT_SUM_TILE, k ^= 1) {
        if (threadIdx.x >= 64) {
            if (b + GT_SUM_TILE < n) stage(b + GT_SUM_TILE, k ^ 1, threadIdx.x - 64, PP_BLOCK - 64);
        } else if (threadIdx.x == 0) {
            const int len = min(GT_SUM_TILE, n - b), n4 = len >> 2;
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
    return sum;
}
[[maybe_unused]] __global__ __launch_bounds__(PP_BLOCK) void gt_seqsum_kernel(GtSumJobs jobs, float* __restrict__ out) {
    const float sum = gt_seqsum_job(jobs.p[blockIdx.x], jobs.n[blockIdx.x], jobs.sq[blockIdx.x] != 0);
    if (threadIdx.x == 0) out[blockIdx.x] = sum;
}
[[maybe_unused]] __global__ __launch_bounds__(PP_BLOCK) void gt_seqsum_wide_kernel(GtSumJobsWide jobs, float* __restrict__ out) {
    const float sum = gt_seqsum_job(jobs.p[blockIdx.x], jobs.n, false);
    if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// a cloud moved by the column-major 4x4 M16 (device memory): rows {M p, 1 | M n, 0 | third quad copied} (pcl::transformPointCloudWithNormals)
[[maybe_unused]] __global__ __launch_bounds__(PP_BLOCK) void pp_move_kernel(const float4* __restrict__ src, int ns, const float* __restrict__ M16, float4* __restrict__ out) {
    __shared__ float G[16];
    if (threadIdx.x < 16) G[threadIdx.x] = M16[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (i >= ns) return;
    const float4 P = src[(size_t) i * 3], N = src[(size_t) i * 3 + 1];
    float4 p, n;
    se3(G, P.x, P.y, P.z, p.x, p.y, p.z);
    so3(G, N.x, N.y, N.z, n.x, n.y, n.z);
    p.w = 1.f; n.w = 0.f;
    out[(size_t) i * 3] = p;
    out[(size_t) i * 3 + 1] = n;
    out[(size_t) i * 3 + 2] = src[(size_t) i * 3 + 2];
}

// compaction of an overlap cloud: flags of [first cloud | second cloud] in index order, then the kept rows
[[maybe_unused]] __global__ __launch_bounds__(PP_BLOCK) void pp_flags_kernel(const uint8_t* __restrict__ ma, int na, const uint8_t* __restrict__ mb, int nb, int* __restrict__ flags) {
    const int i = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (i < na + nb) flags[i] = (i < na ? ma[i] : mb[i - na]) ? 1 : 0;
}
[[maybe_unused]] __global__ __launch_bounds__(PP_BLOCK) void pp_compact_rows_kernel(const float4* __restrict__ a, int na, const float4* __restrict__ b, int nb,
                                                                   const int* __restrict__ flags, const int* __restrict__ pos, float4* __restrict__ out) {
    const int i = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (i >= na + nb || !flags[i]) return;
    const float4* r = i < na ? a + (size_t) i * 3 : b + (size_t) (i - na) * 3;
    float4* o = out + (size_t) pos[i] * 3;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}

inline bool aligned16(const void* p) { return ((uintptr_t) p & 15) == 0; }

// n <= 16 words of a device array -> host (through the pinned scratch; synchronises)
inline int read_words(lgr_ctx* ctx, const void* d, int n, void* out) {
    void* h;
    LGR_TRY(lgr_pinned(ctx, 64, &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, d, (size_t) n * 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out, h, (size_t) n * 4);
    return LGR_OK;
}

// pos[i] = number of set flags before i (flags are 0 / 1 ints), on ctx->stream; the scan's temporary storage is the WS_GRID_TMP slot
inline int pp_scan_flags(lgr_ctx* ctx, int* flags, int* pos, size_t n) {
    size_t tb = 0;
    LGR_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, flags, pos, 0, n, rocprim::plus<int>(), ctx->stream));
    void* tmp;
    LGR_TRY(lgr_ws(ctx, WS_GRID_TMP, tb, &tmp));
    LGR_HIP(ctx, rocprim::exclusive_scan(tmp, tb, flags, pos, 0, n, rocprim::plus<int>(), ctx->stream));
    return LGR_OK;
}

}  // namespace
