// lgr_pointpass.cuh -- what the thread-per-point passes of lgr_analysis.hip and lgr_plane_dense.hip share: the branch-free
// nearest-within-r walk, the wave-aggregated counter, the sequential f32 sum jobs and the exclusive scan of a flag array (the first half
// of a compaction).  Everything here sits in an unnamed namespace: each translation unit gets its own copy of the kernels.
#pragma once
#include <rocprim/device/device_scan.hpp>

#include "lgr_grid.cuh"
#include "lgr_internal.h"

namespace {

constexpr int PP_BLOCK = 256;

// nearest grid point within r2 of p: sorted position or -1.  The candidate loop has no branch on the candidate: every lane offers every
// candidate of its cells and keeps the better one by selects, so a wave never serialises on which lanes found something.
__device__ __forceinline__ int nearest_within(const GridDev& g, float px, float py, float pz, float r2, float& best_d2, int& best_idx) {
    int nn = -1, nn_t = -1;
    float best = 0.f;
    if (g.n > 0 && lgr_finite3(px, py, pz))
        lgr_visit27(g, px, py, pz, [&](int t, const float4& Q) {
            const float d2 = lgr_dist2(px, py, pz, Q.x, Q.y, Q.z);
            const int qi = __float_as_int(Q.w);
            const bool take = (d2 < r2) && (nn < 0 || d2 < best || (d2 == best && qi < nn));
            nn = take ? qi : nn;
            nn_t = take ? t : nn_t;
            best = take ? d2 : best;
        });
    best_d2 = best;
    best_idx = nn;
    return nn_t;
}

__device__ __forceinline__ void wave_count(bool f, int* counter) {
    const unsigned long long m = __ballot(f);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, __popcll(m));
}

// Sequential f32 sums in index order, one workgroup per job: lane 0 adds tile k (one dependent chain, float4 reads from LDS) while waves
// 1-3 stage tile k + 1.  sq: the term is v * v (the squared smoothed densities of src/analysis.cpp:232).
constexpr int GT_SUM_TILE = 4096, GT_SUM_JOBS = 4;
struct GtSumJobs { const float* p[GT_SUM_JOBS]; int n[GT_SUM_JOBS]; int sq[GT_SUM_JOBS]; };
__global__ __launch_bounds__(PP_BLOCK) void gt_seqsum_kernel(GtSumJobs jobs, float* __restrict__ out) {
    __shared__ float4 tile[2][GT_SUM_TILE / 4];
    const float* __restrict__ w = jobs.p[blockIdx.x];
    const int n = jobs.n[blockIdx.x];
    const bool sq = jobs.sq[blockIdx.x] != 0;
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
    if (threadIdx.x == 0) out[blockIdx.x] = sum;
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
