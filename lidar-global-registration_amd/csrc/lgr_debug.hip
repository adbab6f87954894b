// lgr_debug.hip -- temperature maps, hypothesis overlap comparison and the colour passes of the debug files for gfx950.
//
// Replaces what the reference's `debug` command and `compare` test type compute (src/main.cpp:152-205 compareOverlaps, :207-227
// compareHypotheses, :229-284 generateDebugFiles; src/common.cpp:771-816 savePointCloudWithCorrespondences, :818-835 getColor, :837-850
// saveColorizedWeights, :859-906 calculateTemperatureMap, :908-963 saveTemperatureMaps): full-cloud kd-tree passes on the CPU there, a
// thread per point over a uniform grid here.  The files themselves are the caller's (lgr_amd/formats.py, host/lgr_io.hpp).
//
// Declared orders (shared with the CPU statement tests/cpp/debug_ref.cpp):
//   * a cloud moves as in lgr_analysis.hip (se3 / so3, lgr_pointpass.cuh);
//   * "nearest within r" is nearest_within (strict d2 < r * r, smallest squared distance, then lowest index; grid cell 1.001 r);
//   * "nearest" is lgr_nearest_far (lgr_grid.cuh): the minimum under (squared distance, index) over all finite points, which is what
//     lgr_knn_lists gives with k = 1; a non-finite query has no neighbour;
//   * getColor is plain f32 with IEEE division, std::min / std::max as the C++ library defines them (a NaN value takes vmin's colour);
//     a channel is (int) (255.f * c) & 255, 0 for a NaN product (vmin == vmax);
//   * mixPointColor is applied once per correct correspondence that touches a point, from an integer count per point (c -> c / 2 + 127
//     has reached its fixed point after 8 steps from any start, so min(count, 8) steps are count steps);
//   * weighted_count is the sequential f32 sum of density^2 in index order over the overlap cloud {moved source rows, target rows}.
#include <algorithm>
#include <cmath>
#include <limits>

#include "lgr_grid.cuh"
#include "lgr_internal.h"
#include "lgr_libm.cuh"
#include "lgr_host.h"
#include "lgr_pointpass.cuh"
#include "lgr_weights_math.h"

namespace {

constexpr int DB = PP_BLOCK;
constexpr int FAR_BLOCK = 128;
constexpr float DBG_HALF_PI = 1.57079637050628662f;   // (float) M_PI / 2

// src/common.cpp:818-835
__device__ __forceinline__ int channel8(float c) {
    const float x = 255.f * c;
    return (x == x) ? ((int) x & 255) : 0;
}
__device__ __forceinline__ int get_color(float v, float vmin, float vmax) {
    float r = 1.f, g = 1.f, b = 1.f;
    const float dv = vmax - vmin;
    const float m = (vmax < v) ? vmax : v;   // std::min(v, vmax)
    v = (vmin < m) ? m : vmin;               // std::max(vmin, m)
    if (v < (vmin + dv / 3.f)) {
        b = 1.f - 3.f * (v - vmin) / dv;
    } else if (v < (vmin + 2.f * dv / 3.f)) {
        b = 0.f;
        g = 2.f - 3.f * (v - vmin) / dv;
    } else {
        b = 0.f;
        g = 0.f;
        r = 3.f - 3.f * (v - vmin) / dv;
    }
    return (channel8(r) << 16) + (channel8(g) << 8) + channel8(b);
}

struct TempOut { float* td; float* tn; int32_t* cd; int32_t* cn; int32_t* nn; };

// calculateTemperatureMap for both temperature types: thread i handles compared point i
__global__ __launch_bounds__(DB) void temperature_kernel(GridDev ref, const float4* __restrict__ cmp, int n, float dmax, float r2, TempOut o,
                                                         int* __restrict__ counter) {
    const int i = blockIdx.x * DB + threadIdx.x;
    bool below = false;
    if (i < n) {
        const float4 P = cmp[(size_t) i * 3], PN = cmp[(size_t) i * 3 + 1];
        float d2;
        int j;
        const int t = nearest_within(ref, P.x, P.y, P.z, r2, d2, j);
        float dp = dmax, tn = DBG_HALF_PI;
        if (t >= 0) {
            const float4 Q = ref.pxyz[t], N = ref.pnrm[t];
            dp = fabsf(dot3(N.x, N.y, N.z, Q.x - P.x, Q.y - P.y, Q.z - P.z));
            dp = fin(dp) ? dp : d2;   // "normal can be invalid"
            below = dp < dmax;
            if (below) {
                float cs = dot3(N.x, N.y, N.z, PN.x, PN.y, PN.z);
                cs = (1.f < cs) ? 1.f : cs;     // std::min(cs, 1.f)
                cs = (cs < -1.f) ? -1.f : cs;   // std::max(., -1.f)
                float nd = fabsf(lgr_glibc::acosf_(cs));
                nd = (DBG_HALF_PI < nd) ? DBG_HALF_PI : nd;   // std::min(nd, temperature_max): a NaN stays
                tn = fin(nd) ? nd : DBG_HALF_PI;
            }
        }
        const float td = below ? dp : dmax;
        if (o.td) o.td[i] = td;
        if (o.tn) o.tn[i] = tn;
        if (o.cd) o.cd[i] = get_color(td, 0.f, dmax);
        if (o.cn) o.cn[i] = get_color(tn, 0.f, DBG_HALF_PI);
        if (o.nn) o.nn[i] = j;
    }
    wave_count(below, counter);
}

// the unbounded nearest neighbour of every query row (12 floats); mask != nullptr: compareOverlaps' test against that neighbour's plane
__global__ __launch_bounds__(FAR_BLOCK) void nearest_far_kernel(GridDev ref, const float4* __restrict__ q, int nq, float thr, int32_t* __restrict__ idx,
                                                                float* __restrict__ d2_out, uint8_t* __restrict__ mask, int* __restrict__ counter) {
    __shared__ int st_lo[LGR_FAR_STACK * FAR_BLOCK], st_hi[LGR_FAR_STACK * FAR_BLOCK];
    __shared__ float st_b[LGR_FAR_STACK * FAR_BLOCK];
    const int i = blockIdx.x * FAR_BLOCK + threadIdx.x;
    bool in = false;
    if (i < nq) {
        const float4 P = q[(size_t) i * 3];
        float d2 = 0.f;
        int j = -1, t = -1;
        if (lgr_finite3(P.x, P.y, P.z))
            t = lgr_nearest_far<FAR_BLOCK>(ref, P.x, P.y, P.z, st_lo + threadIdx.x, st_hi + threadIdx.x, st_b + threadIdx.x, d2, j);
        if (idx) idx[i] = j;
        if (d2_out) d2_out[i] = t >= 0 ? d2 : __uint_as_float(0x7f800000u);
        if (mask) {
            if (t >= 0) {
                const float4 Q = ref.pxyz[t], N = ref.pnrm[t];
                float dp = fabsf(dot3(N.x, N.y, N.z, Q.x - P.x, Q.y - P.y, Q.z - P.z));
                dp = fin(dp) ? dp : d2;
                in = dp < thr;
            }
            mask[i] = in ? 1 : 0;
        }
    }
    if (counter) wave_count(in, counter);
}

__global__ __launch_bounds__(DB) void color_map_kernel(const float* __restrict__ v, int n, const float* __restrict__ range2, float vmin, float vmax,
                                                       int32_t* __restrict__ colors) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (range2) { vmin = range2[0]; vmax = range2[1]; }
    if (i < n) colors[i] = get_color(v[i], vmin, vmax);
}
__global__ __launch_bounds__(DB) void order_keys_kernel(const float* __restrict__ v, int n, unsigned* __restrict__ keys) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (i < n) keys[i] = wt_key(v[i]);
}
// quantile(0.01, v) and quantile(0.99, v) from the ascending keys -> range2
__global__ void quantile_range_kernel(const unsigned* __restrict__ sorted, int n, float* __restrict__ range2) {
    const double qs[2] = {0.01, 0.99};
    for (int k = 0; k < 2; ++k) {
        long long i, j;
        wt_quantile_ranks_q(qs[k], n, &i, &j);
        range2[k] = wt_quantile_q(qs[k], n, i, j, wt_unkey(sorted[i]), wt_unkey(sorted[j]));
    }
}

// savePointCloudWithCorrespondences: state bits 1 = key point, 2 = in a correspondence, 4 = in an inlier; mixes = correct correspondences
constexpr int CC_KP = 1, CC_CORR = 2, CC_INL = 4;
__global__ __launch_bounds__(DB) void cc_mark_kp_kernel(const int32_t* __restrict__ kp, int n_kp, int n, int* __restrict__ state, int* __restrict__ bad) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (i >= n_kp) return;
    const int p = kp[i];
    if ((unsigned) p < (unsigned) n) atomicOr(&state[p], CC_KP); else atomicAdd(bad, 1);
}
__global__ __launch_bounds__(DB) void cc_mark_corr_kernel(const lgr_corr* __restrict__ corr, int c, int is_source, int n, int bit, int* __restrict__ state,
                                                          int* __restrict__ mixes, int* __restrict__ bad) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (i >= c) return;
    const int p = is_source ? corr[i].index_query : corr[i].index_match;
    if ((unsigned) p >= (unsigned) n) { atomicAdd(bad, 1); return; }
    if (bit) atomicOr(&state[p], bit); else atomicAdd(&mixes[p], 1);
}
__global__ __launch_bounds__(DB) void cc_color_kernel(const int* __restrict__ state, const int* __restrict__ mixes, int n, int with_kp, int32_t* __restrict__ colors) {
    const int i = blockIdx.x * DB + threadIdx.x;
    if (i >= n) return;
    const int s = state[i];
    int col = with_kp ? LGR_COLOR_PARAKEET : LGR_COLOR_BEIGE;
    if (s & CC_KP) col = LGR_COLOR_BEIGE;
    if (s & CC_CORR) col = LGR_COLOR_RED;
    if (s & CC_INL) col = LGR_COLOR_BLUE;
    int r = (col >> 16) & 255, g = (col >> 8) & 255, b = col & 255;
    const int m = min(mixes[i], 8);   // mixPointColor with white: c / 2 + 0xff / 2, at its fixed point after 8 steps
    for (int k = 0; k < m; ++k) { r = r / 2 + 127; g = g / 2 + 127; b = b / 2 + 127; }
    colors[i] = (r << 16) + (g << 8) + b;
}

// ---------------------------------------------------------------------------------------------------- host side
#define DBG_CHECK_DISTANCE(ctx, d) LGR_CHECK(ctx, (d) > 0.f && (d) <= 1e18f, LGR_ERR_INVALID_ARG)

TempOut temp_out(const lgr_temperature_out* o) {
    return o ? TempOut{o->temp_distance, o->temp_normal, o->color_distance, o->color_normal, o->nn} : TempOut{nullptr, nullptr, nullptr, nullptr, nullptr};
}

// 16 zeroed counter words of WS_DBG_MISC, then room for `extra` floats
int misc(lgr_ctx* ctx, size_t extra, int** counters, float** rest) {
    char* d;
    LGR_TRY(lgr_ws_t(ctx, WS_DBG_MISC, 64 + 4 * extra + 64, &d));
    LGR_HIP(ctx, hipMemsetAsync(d, 0, 64, ctx->stream));
    *counters = (int*) d;
    *rest = (float*) (d + 64);
    return LGR_OK;
}

// one temperature map: compared cloud against the grid of the reference cloud
void launch_temperature(lgr_ctx* ctx, const GridDev& ref, const float* d_cmp, int n, float dmax, const lgr_temperature_out* out, int* counter) {
    const float radius = 2 * dmax;   // DIST_TO_PLANE_COEFFICIENT * distance_max
    if (n > 0) temperature_kernel<<<cdiv(n, DB), DB, 0, ctx->stream>>>(ref, (const float4*) d_cmp, n, dmax, radius * radius, temp_out(out), counter);
}

int upload(lgr_ctx* ctx, float* d, const float* h, size_t n_floats) {
    LGR_HIP(ctx, hipMemcpyAsync(d, h, n_floats * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // h may be a stack buffer
    return LGR_OK;
}

// host twin plumbing for a lgr_temperature_out: the arrays the caller asked for, n entries each, in one staged buffer; copied back afterwards
int temp_out_dev(lgr_host_call& hc, const lgr_temperature_out* host, int n, lgr_temperature_out* dev) {
    *dev = lgr_temperature_out{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!host || n == 0) return LGR_OK;
    int32_t* d;
    LGR_TRY(hc.out((size_t) 5 * n, &d, 16));   // (slack kept from before; no reader past 5 n is known)
    if (host->temp_distance) dev->temp_distance = (float*) d;
    if (host->temp_normal) dev->temp_normal = (float*) d + n;
    if (host->color_distance) dev->color_distance = d + 2 * (size_t) n;
    if (host->color_normal) dev->color_normal = d + 3 * (size_t) n;
    if (host->nn) dev->nn = d + 4 * (size_t) n;
    return LGR_OK;
}
int temp_out_fetch(lgr_host_call& hc, const lgr_temperature_out* host, int n, const lgr_temperature_out& dev) {
    if (!host || n == 0) return LGR_OK;
    LGR_TRY(hc.fetch(host->temp_distance, dev.temp_distance, (size_t) n));
    LGR_TRY(hc.fetch(host->temp_normal, dev.temp_normal, (size_t) n));
    LGR_TRY(hc.fetch(host->color_distance, dev.color_distance, (size_t) n));
    LGR_TRY(hc.fetch(host->color_normal, dev.color_normal, (size_t) n));
    return hc.fetch(host->nn, dev.nn, (size_t) n);
}

}  // namespace

extern "C" int lgr_temperature_map_dev(lgr_ctx* ctx, const float* d_cmp, int n, const float* d_ref, int nr, float distance_max,
                                       const lgr_temperature_out* out, int* n_below) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && nr >= 0 && (d_cmp || n == 0) && (d_ref || nr == 0) && aligned16(d_cmp) && aligned16(d_ref) && n_below, LGR_ERR_INVALID_ARG);
    DBG_CHECK_DISTANCE(ctx, distance_max);
    *n_below = 0;
    if (n == 0 || nr == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    int* counters;
    float* rest;
    LGR_TRY(misc(ctx, 0, &counters, &rest));
    GridDev g{};
    LGR_TRY(lgr_grid_build(ctx, WS_GRID_C, d_ref, nr, 2 * distance_max * 1.001f, 0.f, &g));
    launch_temperature(ctx, g, d_cmp, n, distance_max, out, counters);
    LGR_HIP(ctx, hipGetLastError());
    return read_words(ctx, counters, 1, n_below);
}

extern "C" int lgr_temperature_maps_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16], float distance_thr,
                                        const lgr_temperature_out* src_out, const lgr_temperature_out* tgt_out, float* d_moved, int n_below2[2]) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, ns >= 0 && nt >= 0 && (d_src || ns == 0) && (d_tgt || nt == 0) && aligned16(d_src) && aligned16(d_tgt) && aligned16(d_moved) && T16 &&
                       n_below2, LGR_ERR_INVALID_ARG);
    DBG_CHECK_DISTANCE(ctx, distance_thr);
    n_below2[0] = n_below2[1] = 0;
    if (ns == 0 || nt == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    int* counters;
    float* d_T;
    LGR_TRY(misc(ctx, 16, &counters, &d_T));
    LGR_TRY(upload(ctx, d_T, T16, 16));
    if (!d_moved) LGR_TRY(lgr_ws_t(ctx, WS_DBG_MOVED, (size_t) 12 * ns + 16, &d_moved));
    pp_move_kernel<<<cdiv(ns, DB), DB, 0, ctx->stream>>>((const float4*) d_src, ns, d_T, (float4*) d_moved);
    const float cell = 2 * distance_thr * 1.001f;
    GridDev gt{}, gs{};
    LGR_TRY(lgr_grid_build(ctx, WS_GRID_C, d_tgt, nt, cell, 0.f, &gt));
    launch_temperature(ctx, gt, d_moved, ns, distance_thr, src_out, counters + 0);
    LGR_TRY(lgr_grid_build(ctx, WS_GRID_B, d_moved, ns, cell, 0.f, &gs));
    launch_temperature(ctx, gs, d_tgt, nt, distance_thr, tgt_out, counters + 1);
    LGR_HIP(ctx, hipGetLastError());
    return read_words(ctx, counters, 2, n_below2);
}

extern "C" int lgr_nearest_dev(lgr_ctx* ctx, const float* d_q, int nq, const float* d_pts, int n, int32_t* d_idx, float* d_d2) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, nq >= 0 && n >= 0 && (d_q || nq == 0) && (d_pts || n == 0) && (d_idx || nq == 0) && aligned16(d_q) && aligned16(d_pts), LGR_ERR_INVALID_ARG);
    if (nq == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    GridDev g{};
    LGR_TRY(lgr_grid_build(ctx, WS_GRID_C, d_pts, n, 0.f, 4.f, &g));
    nearest_far_kernel<<<cdiv(nq, FAR_BLOCK), FAR_BLOCK, 0, ctx->stream>>>(g, (const float4*) d_q, nq, 0.f, d_idx, d_d2, nullptr, nullptr);
    LGR_HIP(ctx, hipGetLastError());
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_nearest(lgr_ctx* ctx, const float* q, int nq, const float* pts, int n, int32_t* idx, float* d2) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, nq >= 0 && n >= 0 && (q || nq == 0) && (pts || n == 0) && (idx || nq == 0), LGR_ERR_INVALID_ARG);
    if (nq == 0) return LGR_OK;
    float *dq, *dp, *dd;
    int32_t* di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(q, (size_t) nq * 12, &dq));
    LGR_TRY(hc.in(pts, (size_t) n * 12, &dp));
    LGR_TRY(hc.out((size_t) nq, &di));
    LGR_TRY(hc.out((size_t) nq, &dd));
    LGR_TRY(lgr_nearest_dev(ctx, dq, nq, dp, n, di, dd));
    LGR_TRY(hc.fetch(idx, di, (size_t) nq));
    LGR_TRY(hc.fetch(d2, dd, (size_t) nq));
    return hc.finish();
}

extern "C" int lgr_compare_overlaps_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float* tns16, int n, float distance_thr,
                                        int32_t* counts, float* weighted_counts, int32_t* counts2, uint8_t* d_mask_src, uint8_t* d_mask_tgt) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, ns >= 0 && nt >= 0 && n >= 0 && n <= 4096 && (d_src || ns == 0) && (d_tgt || nt == 0) && aligned16(d_src) && aligned16(d_tgt) &&
                       (n == 0 || (tns16 && counts && weighted_counts)), LGR_ERR_INVALID_ARG);
    DBG_CHECK_DISTANCE(ctx, distance_thr);
    for (int k = 0; k < n; ++k) {
        counts[k] = 0; weighted_counts[k] = 0.f;
        if (counts2) counts2[2 * k] = counts2[2 * k + 1] = 0;
    }
    if (n == 0 || ns == 0 || nt == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t) ns + nt;
    int* flags;
    float *d_moved, *d_T;
    LGR_TRY(lgr_ws_t(ctx, WS_DBG_MISC, (size_t) 16 * n + 16, &d_T));
    LGR_TRY(upload(ctx, d_T, tns16, (size_t) 16 * n));
    LGR_TRY(lgr_ws_t(ctx, WS_DBG_MOVED, (size_t) 12 * ns + 16, &d_moved));
    // flags, their scan, the two masks of a caller that passes none, then 2 counter words and the sum
    LGR_TRY(lgr_ws_t(ctx, WS_DBG_FLAGS, 2 * np + (np + 3) / 4 + 32, &flags));
    int* pos = flags + np;
    uint8_t* own = (uint8_t*) (pos + np);
    int* counters = (int*) (own + ((np + 3) / 4) * 4);
    float* d_sum = (float*) (counters + 2);
    GridDev gt{};
    LGR_TRY(lgr_grid_build(ctx, WS_GRID_C, d_tgt, nt, 0.f, 4.f, &gt));   // once for all n transformations
    for (int k = 0; k < n; ++k) {
        uint8_t* ms = d_mask_src ? d_mask_src + (size_t) k * ns : own;
        uint8_t* mt = d_mask_tgt ? d_mask_tgt + (size_t) k * nt : own + ns;
        LGR_HIP(ctx, hipMemsetAsync(counters, 0, 16, ctx->stream));
        pp_move_kernel<<<cdiv(ns, DB), DB, 0, ctx->stream>>>((const float4*) d_src, ns, d_T + 16 * (size_t) k, (float4*) d_moved);
        nearest_far_kernel<<<cdiv(ns, FAR_BLOCK), FAR_BLOCK, 0, ctx->stream>>>(gt, (const float4*) d_moved, ns, distance_thr, nullptr, nullptr, ms, counters + 0);
        GridDev gs{};
        LGR_TRY(lgr_grid_build(ctx, WS_GRID_B, d_moved, ns, 0.f, 4.f, &gs));
        nearest_far_kernel<<<cdiv(nt, FAR_BLOCK), FAR_BLOCK, 0, ctx->stream>>>(gs, (const float4*) d_tgt, nt, distance_thr, nullptr, nullptr, mt, counters + 1);
        LGR_HIP(ctx, hipGetLastError());
        int n2[2];
        LGR_TRY(read_words(ctx, counters, 2, n2));
        const int no = n2[0] + n2[1];
        counts[k] = no;
        if (counts2) { counts2[2 * k] = n2[0]; counts2[2 * k + 1] = n2[1]; }
        if (no < 2) continue;   // calculateSmoothedDensities would rassert (src/common.cpp:532): declared 0
        pp_flags_kernel<<<cdiv((long long) np, DB), DB, 0, ctx->stream>>>(ms, ns, mt, nt, flags);
        LGR_TRY(pp_scan_flags(ctx, flags, pos, np));
        float *d_ov, *d_dens;
        LGR_TRY(lgr_ws_t(ctx, WS_DBG_OVERLAP, (size_t) 12 * no + 16, &d_ov));
        LGR_TRY(lgr_ws_t(ctx, WS_DBG_DENS, (size_t) no + 16, &d_dens));
        pp_compact_rows_kernel<<<cdiv((long long) np, DB), DB, 0, ctx->stream>>>((const float4*) d_moved, ns, (const float4*) d_tgt, nt, flags, pos, (float4*) d_ov);
        LGR_HIP(ctx, hipGetLastError());
        LGR_TRY(lgr_smoothed_densities_dev(ctx, d_ov, no, 2, d_dens));
        GtSumJobs jobs{};
        jobs.p[0] = d_dens; jobs.n[0] = no; jobs.sq[0] = 1;
        gt_seqsum_kernel<<<1, DB, 0, ctx->stream>>>(jobs, d_sum);
        LGR_HIP(ctx, hipGetLastError());
        LGR_TRY(read_words(ctx, d_sum, 1, &weighted_counts[k]));
    }
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_color_map_dev(lgr_ctx* ctx, const float* d_values, int n, float vmin, float vmax, int32_t* d_colors) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && ((d_values && d_colors) || n == 0), LGR_ERR_INVALID_ARG);
    if (n == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    color_map_kernel<<<cdiv(n, DB), DB, 0, ctx->stream>>>(d_values, n, nullptr, vmin, vmax, d_colors);
    LGR_HIP(ctx, hipGetLastError());
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_color_weights_dev(lgr_ctx* ctx, const float* d_weights, int n, int32_t* d_colors, float range2[2]) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && ((d_weights && d_colors) || n == 0), LGR_ERR_INVALID_ARG);
    if (range2) range2[0] = range2[1] = std::numeric_limits<float>::quiet_NaN();   // quantile of an empty vector
    if (n == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = ((size_t) n + 63) & ~(size_t) 63;
    unsigned* keys;
    LGR_TRY(lgr_ws_t(ctx, WS_DBG_SORT, 4 * nn + 64, &keys));
    unsigned* sorted = keys + nn;
    int* vals = (int*) (sorted + nn);
    float* d_range = (float*) (vals + 2 * nn);
    order_keys_kernel<<<cdiv(n, DB), DB, 0, ctx->stream>>>(d_weights, n, keys);
    LGR_TRY(lgr_sort_pairs_u32(ctx, keys, sorted, vals, vals + nn, (size_t) n, 0, 32));
    quantile_range_kernel<<<1, 1, 0, ctx->stream>>>(sorted, n, d_range);
    color_map_kernel<<<cdiv(n, DB), DB, 0, ctx->stream>>>(d_weights, n, d_range, 0.f, 0.f, d_colors);
    LGR_HIP(ctx, hipGetLastError());
    if (range2) return read_words(ctx, d_range, 2, range2);
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_color_correspondences_dev(lgr_ctx* ctx, int n, const int32_t* d_kp, int n_kp, const lgr_corr* d_corr, int c, const lgr_corr* d_correct,
                                             int n_correct, const lgr_corr* d_inl, int n_inl, int is_source, int32_t* d_colors) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && n_kp >= 0 && c >= 0 && n_correct >= 0 && n_inl >= 0 && (d_kp || n_kp == 0) && (d_corr || c == 0) && (d_correct || n_correct == 0) &&
                       (d_inl || n_inl == 0) && (d_colors || n == 0), LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    int* state;
    LGR_TRY(lgr_ws_t(ctx, WS_DBG_FLAGS, 2 * (size_t) n + 16, &state));
    LGR_HIP(ctx, hipMemsetAsync(state, 0, (2 * (size_t) n + 16) * 4, ctx->stream));
    int *mixes = state + n, *bad = state + 2 * (size_t) n;
    if (n_kp) cc_mark_kp_kernel<<<cdiv(n_kp, DB), DB, 0, ctx->stream>>>(d_kp, n_kp, n, state, bad);
    if (c) cc_mark_corr_kernel<<<cdiv(c, DB), DB, 0, ctx->stream>>>(d_corr, c, is_source, n, CC_CORR, state, mixes, bad);
    if (n_inl) cc_mark_corr_kernel<<<cdiv(n_inl, DB), DB, 0, ctx->stream>>>(d_inl, n_inl, is_source, n, CC_INL, state, mixes, bad);
    if (n_correct) cc_mark_corr_kernel<<<cdiv(n_correct, DB), DB, 0, ctx->stream>>>(d_correct, n_correct, is_source, n, 0, state, mixes, bad);
    if (n) cc_color_kernel<<<cdiv(n, DB), DB, 0, ctx->stream>>>(state, mixes, n, d_kp != nullptr, d_colors);
    LGR_HIP(ctx, hipGetLastError());
    int n_bad = 0;
    LGR_TRY(read_words(ctx, bad, 1, &n_bad));
    LGR_CHECK(ctx, n_bad == 0, LGR_ERR_INVALID_ARG);   // an index outside [0, n)
    return LGR_OK;
}

// ---------------------------------------------------------------------------------------------------- host twins
extern "C" int lgr_temperature_map(lgr_ctx* ctx, const float* cmp, int n, const float* ref, int nr, float distance_max, const lgr_temperature_out* out,
                                   int* n_below) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && nr >= 0 && (cmp || n == 0) && (ref || nr == 0), LGR_ERR_INVALID_ARG);
    float *dc, *dr;
    lgr_temperature_out st;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(cmp, n, ref, nr, &dc, &dr));
    LGR_TRY(temp_out_dev(hc, out, nr ? n : 0, &st));
    LGR_TRY(lgr_temperature_map_dev(ctx, dc, n, dr, nr, distance_max, out ? &st : nullptr, n_below));
    LGR_TRY(temp_out_fetch(hc, out, nr ? n : 0, st));
    return hc.finish();
}

extern "C" int lgr_temperature_maps(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float T16[16], float distance_thr,
                                    const lgr_temperature_out* src_out, const lgr_temperature_out* tgt_out, float* moved, int n_below2[2]) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, ns >= 0 && nt >= 0 && (src || ns == 0) && (tgt || nt == 0), LGR_ERR_INVALID_ARG);
    float *ds, *dt, *dm = nullptr;
    lgr_temperature_out ss, tt;
    const bool any = ns > 0 && nt > 0;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(temp_out_dev(hc, src_out, any ? ns : 0, &ss));
    LGR_TRY(temp_out_dev(hc, tgt_out, any ? nt : 0, &tt));
    if (moved && any) LGR_TRY(lgr_ws_t(ctx, WS_DBG_MOVED, (size_t) 12 * ns + 16, &dm));   // the twin's own slot for the moved source
    LGR_TRY(lgr_temperature_maps_dev(ctx, ds, ns, dt, nt, T16, distance_thr, src_out ? &ss : nullptr, tgt_out ? &tt : nullptr, dm, n_below2));
    LGR_TRY(temp_out_fetch(hc, src_out, any ? ns : 0, ss));
    LGR_TRY(temp_out_fetch(hc, tgt_out, any ? nt : 0, tt));
    if (dm) LGR_TRY(hc.fetch(moved, dm, (size_t) ns * 12));
    return hc.finish();
}

extern "C" int lgr_compare_overlaps(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float* tns16, int n, float distance_thr,
                                    int32_t* counts, float* weighted_counts, int32_t* counts2, uint8_t* mask_src, uint8_t* mask_tgt) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, ns >= 0 && nt >= 0 && n >= 0 && n <= 4096 && (src || ns == 0) && (tgt || nt == 0), LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    uint8_t *dms = nullptr, *dmt = nullptr;
    const bool any = ns > 0 && nt > 0 && n > 0;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    if (mask_src && any) LGR_TRY(hc.out((size_t) n * ns, &dms, LGR_PAD_MASK));
    if (mask_tgt && any) LGR_TRY(hc.out((size_t) n * nt, &dmt, LGR_PAD_MASK));
    LGR_TRY(lgr_compare_overlaps_dev(ctx, ds, ns, dt, nt, tns16, n, distance_thr, counts, weighted_counts, counts2, dms, dmt));
    if (dms) LGR_TRY(hc.fetch(mask_src, dms, (size_t) n * ns));
    if (dmt) LGR_TRY(hc.fetch(mask_tgt, dmt, (size_t) n * nt));
    return hc.finish();
}

namespace {
// n values up, n colours back
template <class F>
int colors_of_values(lgr_ctx* ctx, const float* values, int n, int32_t* colors, F&& run) {
    LGR_CHECK(ctx, n >= 0 && ((values && colors) || n == 0), LGR_ERR_INVALID_ARG);
    float* dv;
    int32_t* dc;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(values, (size_t) n, &dv));
    LGR_TRY(hc.out((size_t) n, &dc));
    LGR_TRY(run(dv, dc));
    LGR_TRY(hc.fetch(colors, dc, (size_t) n));
    return hc.finish();
}
}  // namespace

extern "C" int lgr_color_map(lgr_ctx* ctx, const float* values, int n, float vmin, float vmax, int32_t* colors) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return colors_of_values(ctx, values, n, colors, [&](const float* dv, int32_t* dc) { return lgr_color_map_dev(ctx, dv, n, vmin, vmax, dc); });
}

extern "C" int lgr_color_weights(lgr_ctx* ctx, const float* weights, int n, int32_t* colors, float range2[2]) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return colors_of_values(ctx, weights, n, colors, [&](const float* dv, int32_t* dc) { return lgr_color_weights_dev(ctx, dv, n, dc, range2); });
}

extern "C" int lgr_color_correspondences(lgr_ctx* ctx, int n, const int32_t* kp, int n_kp, const lgr_corr* corr, int c, const lgr_corr* correct, int n_correct,
                                         const lgr_corr* inl, int n_inl, int is_source, int32_t* colors) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && n_kp >= 0 && c >= 0 && n_correct >= 0 && n_inl >= 0 && (kp || n_kp == 0) && (corr || c == 0) && (correct || n_correct == 0) &&
                       (inl || n_inl == 0) && (colors || n == 0), LGR_ERR_INVALID_ARG);
    int32_t *d, *dkp;
    lgr_corr *dc, *dok, *di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.out((size_t) n, &d));
    LGR_TRY(hc.in(kp, (size_t) n_kp, &dkp));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    LGR_TRY(hc.in(correct, (size_t) n_correct, &dok));
    LGR_TRY(hc.in(inl, (size_t) n_inl, &di));
    // key points given, none found: the twin still gets a pointer (it colours by "were key points given"); the lists are null when empty
    LGR_TRY(lgr_color_correspondences_dev(ctx, n, kp ? dkp : nullptr, n_kp, c ? dc : nullptr, c, n_correct ? dok : nullptr, n_correct, n_inl ? di : nullptr,
                                          n_inl, is_source, d));
    LGR_TRY(hc.fetch(colors, d, (size_t) n));
    return hc.finish();
}
