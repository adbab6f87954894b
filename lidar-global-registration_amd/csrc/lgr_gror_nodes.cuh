// lgr_gror_nodes.cuh -- GROR's node stage (include/gror/ia_gror.hpp:126-170): the correspondences packed as point pairs, every node's
// reliability degree over all C^2 pairs, the ranking keys (degree descending, index ascending) and the gather of the K best.  Shared by
// lgr_gror.hip and lgr_teaser.hip (TEASER selects its nodes by GROR's rule).  Everything here sits in an unnamed
// namespace: each translation unit gets its own copy of the kernels.
#pragma once
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "lgr_internal.h"

namespace {

// bad == nullptr: the caller has range-checked the correspondences (lgr_check_corr).  Otherwise the check happens here: a pair with an
// index outside [0, ns) x [0, nt) sets *bad and is packed as NaNs instead of being gathered, and the caller reads *bad back later.
__global__ void gror_pack_kernel(const float* __restrict__ src, const float* __restrict__ tgt, const lgr_corr* __restrict__ corr, int c,
                                 float4* __restrict__ S, float4* __restrict__ T, int ns = 0, int nt = 0, int* __restrict__ bad = nullptr) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c) return;
    lgr_corr cr = corr[i];
    if (bad && ((unsigned) cr.index_query >= (unsigned) ns || (unsigned) cr.index_match >= (unsigned) nt)) {
        const float q = __uint_as_float(0x7fc00000u);
        S[i] = make_float4(q, q, q, 0.f);
        T[i] = make_float4(q, q, q, 0.f);
        *bad = 1;
        return;
    }
    const float* s = src + 12 * (size_t) cr.index_query;
    const float* t = tgt + 12 * (size_t) cr.index_match;
    S[i] = make_float4(s[0], s[1], s[2], 0.f);
    T[i] = make_float4(t[0], t[1], t[2], 0.f);
}

__device__ __forceinline__ float edge_len(float4 a, float4 b) {   // pcl::geometry::distance
    float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
}

constexpr int DEG_THREADS = 256;
constexpr int DEG_TILE = 512;
// degree[i] += #{ j in this block's slice, j != i : | |s_i s_j| - |t_i t_j| | < 2 * resolution }
__global__ __launch_bounds__(DEG_THREADS) void gror_degree_kernel(const float4* __restrict__ S, const float4* __restrict__ T, int c, int slice,
                                                                  float two_res, int* __restrict__ degree) {
    __shared__ float4 Ss[DEG_TILE], Ts[DEG_TILE];
    int i = blockIdx.x * DEG_THREADS + threadIdx.x;
    bool live = i < c;
    float4 si = live ? S[i] : make_float4(0, 0, 0, 0), ti = live ? T[i] : make_float4(0, 0, 0, 0);
    int j0 = blockIdx.y * slice, j1 = min(c, j0 + slice);
    int cnt = 0;
    for (int base = j0; base < j1; base += DEG_TILE) {
        int m = min(DEG_TILE, j1 - base);
        __syncthreads();
        for (int k = threadIdx.x; k < m; k += DEG_THREADS) { Ss[k] = S[base + k]; Ts[k] = T[base + k]; }
        __syncthreads();
        // The decision |  |s_i s_j| - |t_i t_j|  | < 2 r with the hardware's one-instruction square root (1 ulp) wherever that decides it -- the two
        // lengths are within 1.5 ulp of the correctly rounded ones, so the difference is within 4 ulp of the larger length of the reference's: a pair
        // goes through edge_len's correctly rounded square roots (a dozen instructions each) only when it lies within 1e-6 of the larger length of the
        // threshold, which some lane of a wave does for ~1e-4 of the steps (round 5: 3.3 -> ~2 ms for 50 000 correspondences; dead lanes take part:
        // their points are the origin).
        for (int k = 0; k < m; ++k) {
            const float4 sj = Ss[k], tj = Ts[k];
            const float ax = si.x - sj.x, ay = si.y - sj.y, az = si.z - sj.z, bx = ti.x - tj.x, by = ti.y - tj.y, bz = ti.z - tj.z;
            const float la = __builtin_amdgcn_sqrtf((ax * ax + ay * ay) + az * az), lb = __builtin_amdgcn_sqrtf((bx * bx + by * by) + bz * bz);
            const float d = fabsf(la - lb);
            bool in = d < two_res;
            if (__any(!(fabsf(d - two_res) > 1e-6f * fmaxf(la, lb) + 1e-30f)))   // (NaN: taken)
                in = fabsf(edge_len(si, sj) - edge_len(ti, tj)) < two_res;
            cnt += (in && live && base + k != i) ? 1 : 0;
        }
    }
    if (live && cnt) atomicAdd(&degree[i], cnt);
}

__global__ void gror_keys_kernel(const int* __restrict__ degree, int c, unsigned long long* __restrict__ keys) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < c) keys[i] = ((unsigned long long) (0xffffffffu - (unsigned) degree[i]) << 32) | (unsigned) i;
}

__global__ void gror_gather_kernel(const unsigned long long* __restrict__ keys, int K, int use_keys, const float4* __restrict__ S,
                                   const float4* __restrict__ T, float4* __restrict__ out) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    int i = use_keys ? (int) (keys[k] & 0xffffffffu) : k;
    float4 s = S[i], t = T[i];
    s.w = __int_as_float(i);
    out[2 * k] = s;
    out[2 * k + 1] = t;
}

struct GrorBuffers { float4 *S, *T; int* degree; };

[[maybe_unused]] int gror_pack(lgr_ctx* ctx, const float* d_src, const float* d_tgt, const lgr_corr* d_corr, int c, GrorBuffers* b, int ns = 0, int nt = 0,
                               int* d_bad = nullptr) {
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_PACK, (size_t) 2 * c + 4, &b->S));
    b->T = b->S + c;
    gror_pack_kernel<<<cdiv(c, 256), 256, 0, ctx->stream>>>(d_src, d_tgt, d_corr, c, b->S, b->T, ns, nt, d_bad);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

[[maybe_unused]] int gror_degrees(lgr_ctx* ctx, const GrorBuffers& b, int c, float resolution, int* d_degree) {
    LGR_HIP(ctx, hipMemsetAsync(d_degree, 0, (size_t) c * 4, ctx->stream));
    int iblocks = cdiv(c, DEG_THREADS);
    // enough workgroups for 256 CUs: split the j range when there are few i blocks
    int want = std::max(1, (8 * ctx->n_cu) / iblocks);
    int nsplit = std::min(want, cdiv(c, DEG_TILE));
    int slice = cdiv(cdiv(c, nsplit), DEG_TILE) * DEG_TILE;
    nsplit = cdiv(c, slice);
    gror_degree_kernel<<<dim3(iblocks, nsplit), DEG_THREADS, 0, ctx->stream>>>(b.S, b.T, c, slice, 2.0f * resolution, d_degree);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// keys2[0 .. c) = the correspondences by (degree descending, index ascending), the index in the low word; keys / keys2: c words each
[[maybe_unused]] int gror_rank(lgr_ctx* ctx, const int* d_degree, int c, unsigned long long* keys, unsigned long long* keys2) {
    gror_keys_kernel<<<cdiv(c, 256), 256, 0, ctx->stream>>>(d_degree, c, keys);
    size_t tb = 0;
    LGR_HIP(ctx, rocprim::radix_sort_keys(nullptr, tb, keys, keys2, (size_t) c, 0, 64, ctx->stream));
    void* tmp;
    LGR_TRY(lgr_ws(ctx, WS_GRID_TMP, tb, &tmp));
    LGR_HIP(ctx, rocprim::radix_sort_keys(tmp, tb, keys, keys2, (size_t) c, 0, 64, ctx->stream));
    return LGR_OK;
}

}  // namespace
