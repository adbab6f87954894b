// lgr_analysis.hip -- ground-truth evaluation of an alignment for gfx950.
//
// Replaces what AlignmentAnalysis::start computes when a ground truth is known (reference src/analysis.cpp:19-24, :30-43, :45-88, :141-185,
// :187-206, :218-246 and mergeOverlaps, src/common.cpp:558-591): several full-cloud kd-tree passes on the CPU there, one query per point,
// each independent of the others.  Here every pass is a kernel with a thread per point over a uniform grid (lgr_grid.cuh).
// lgr_evaluate_gt_batch* judges n estimates against one ground truth: what the ground truth alone decides runs once, the rest per
// chunk of LGR_GT_BATCH_CHUNK estimates (gt_foot_kernel, gt_batch_kernel, run_points_batch).
//
// Declared orders (shared with the CPU statement tests/cpp/analysis_ref.cpp):
//   * a point moves in PCL's se3 order x * c0 + (y * c1 + (z * c2 + c3)), a normal the same without c3; no contraction;
//   * "nearest target within r" is the closest-plane metric's rule (lgr_plane.hip): strict d2 < r * r, the smallest squared distance
//     (lgr_dist2), then the lowest index; non-finite points neither ask nor answer; grid cell = 1.001 r;
//   * "nearest target" is lgr_knn_lists with k = 1: ascending (squared distance, index);
//   * a float sum over points is the sequential f32 sum in ascending index of per-point terms that were written to a buffer first
//     (a skipped point's term is +0, which leaves a sum of non-negative terms unchanged); counts are integers (order free);
//   * the median of the normal differences is the element of rank n / 2 of the ascending values (a radix sort of their bit patterns:
//     all of them are >= 0); a NaN difference does not count (the reference's `diff >= 0.f` filter drops it too).
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "lgr_grid.cuh"
#include "lgr_internal.h"
#include "lgr_libm.cuh"
#include "lgr_host.h"
#include "lgr_pointpass.cuh"

namespace {

constexpr int AB = PP_BLOCK;
constexpr float GT_PI = 3.14159274101257324f;   // (float) M_PI

struct GtMats { float T[16], G[16], D[16]; };   // estimate, ground truth, D = T^-1 * G (column-major)

// Quantities 2, 3 and 6 in one launch: thread i handles source point i (its point-cloud term, its overlap term after ONE grid walk) and
// correspondence i.  counters: [0] overlap_size, [1] correct correspondences, [2] correct inliers, [3] inliers.
__global__ __launch_bounds__(AB) void gt_point_kernel(GridDev g, const float4* __restrict__ src, int ns, const float4* __restrict__ tgt,
                                                      const lgr_corr* __restrict__ corr, int c, const GtMats* __restrict__ mats, float thr, float r2,
                                                      float* __restrict__ term_pcd, float* __restrict__ term_ov, int32_t* __restrict__ nn_out,
                                                      const uint8_t* __restrict__ inl_mask, uint8_t* __restrict__ correct_out, int* __restrict__ counters) {
    __shared__ GtMats M;
    for (int k = threadIdx.x; k < 48; k += AB) ((float*) &M)[k] = ((const float*) mats)[k];
    __syncthreads();
    const int i = blockIdx.x * AB + threadIdx.x;
    bool counted = false;
    if (i < ns) {
        const float4 P = src[(size_t) i * 3];
        float gx, gy, gz, ax, ay, az, bx, by, bz;
        se3(M.G, P.x, P.y, P.z, gx, gy, gz);
        se3(M.T, P.x, P.y, P.z, ax, ay, az);
        se3(M.D, P.x, P.y, P.z, bx, by, bz);
        term_pcd[i] = sq3(P.x - bx, P.y - by, P.z - bz);   // dist2(p, D p), src/analysis.cpp:26-28
        float d2;
        int j;
        const int t = nearest_within(g, gx, gy, gz, r2, d2, j);
        float term = 0.f;
        if (t >= 0) {
            const float4 Q = g.pxyz[t], N = g.pnrm[t];
            if (lgr_finite3(N.x, N.y, N.z)) {
                const float s = dot3(gx - Q.x, gy - Q.y, gz - Q.z, N.x, N.y, N.z);
                const float qx = gx - s * N.x, qy = gy - s * N.y, qz = gz - s * N.z;   // point_on_plane
                if (!(__builtin_sqrtf(sq3(gx - qx, gy - qy, gz - qz)) > thr)) {
                    const float d = __builtin_sqrtf(sq3(ax - qx, ay - qy, az - qz));
                    term = d * d;
                    counted = true;
                }
            }
        }
        term_ov[i] = term;
        if (nn_out) nn_out[i] = counted ? j : -1;
    }
    wave_count(counted, counters + 0);
    bool correct = false, inl = false;
    if (i < c) {
        const lgr_corr cr = corr[i];
        const float4 P = src[(size_t) cr.index_query * 3], Q = tgt[(size_t) cr.index_match * 3];
        float gx, gy, gz;
        se3(M.G, P.x, P.y, P.z, gx, gy, gz);
        const float e = __builtin_sqrtf(sq3(gx - Q.x, gy - Q.y, gz - Q.z));   // pcl::L2_Norm(source_point.data, target_point.data, 3)
        correct = e < cr.threshold;
        inl = inl_mask && inl_mask[i];
        if (correct_out) correct_out[i] = correct ? 1 : 0;
    }
    wave_count(correct, counters + 1);
    wave_count(correct && inl, counters + 2);
    wave_count(inl, counters + 3);
}

// ---- n estimates against one ground truth (lgr_evaluate_gt_batch_dev): gt_point_kernel split where the estimate enters ----
constexpr int GTB_CHUNK = LGR_GT_BATCH_CHUNK;
static_assert(2 * GTB_CHUNK <= GT_SUM_JOBS_WIDE, "two sum jobs per transform of a chunk");
struct GtBatchMats { float T[16], D[16]; };   // one estimate and its D = T^-1 * G (column-major)

// What gt_point_kernel computes from the ground truth alone, once per batch.  Thread i walks the target's grid for source point i and
// keeps the foot point on the tangent plane (src/analysis.cpp:69-76) as foot[i] = (q, 1), or (0, 0, 0, 0) where the point is skipped;
// for correspondence i it writes the correct flag.  counters: [0] overlap_size, [1] correct correspondences.
__global__ __launch_bounds__(AB) void gt_foot_kernel(GridDev g, const float4* __restrict__ src, int ns, const float4* __restrict__ tgt,
                                                     const lgr_corr* __restrict__ corr, int c, const GtMats* __restrict__ mats, float thr, float r2,
                                                     float4* __restrict__ foot, uint8_t* __restrict__ correct_out, int* __restrict__ counters) {
    __shared__ float G[16];
    if (threadIdx.x < 16) G[threadIdx.x] = mats->G[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * AB + threadIdx.x;
    bool counted = false;
    if (i < ns) {
        const float4 P = src[(size_t) i * 3];
        float gx, gy, gz;
        se3(G, P.x, P.y, P.z, gx, gy, gz);
        float d2;
        int j;
        const int t = nearest_within(g, gx, gy, gz, r2, d2, j);
        float4 F = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0) {
            const float4 Q = g.pxyz[t], N = g.pnrm[t];
            if (lgr_finite3(N.x, N.y, N.z)) {
                const float s = dot3(gx - Q.x, gy - Q.y, gz - Q.z, N.x, N.y, N.z);
                const float qx = gx - s * N.x, qy = gy - s * N.y, qz = gz - s * N.z;   // point_on_plane
                if (!(__builtin_sqrtf(sq3(gx - qx, gy - qy, gz - qz)) > thr)) {
                    F = make_float4(qx, qy, qz, 1.f);
                    counted = true;
                }
            }
        }
        foot[i] = F;
    }
    wave_count(counted, counters + 0);
    bool correct = false;
    if (i < c) {
        const lgr_corr cr = corr[i];
        const float4 P = src[(size_t) cr.index_query * 3], Q = tgt[(size_t) cr.index_match * 3];
        float gx, gy, gz;
        se3(G, P.x, P.y, P.z, gx, gy, gz);
        const float e = __builtin_sqrtf(sq3(gx - Q.x, gy - Q.y, gz - Q.z));
        correct = e < cr.threshold;
        correct_out[i] = correct ? 1 : 0;
    }
    wave_count(correct, counters + 1);
}

// ... and what depends on the estimate, for the m <= GTB_CHUNK estimates of a chunk in one launch: thread i reads source point i and its
// foot point once and writes, per estimate s, the point-cloud term to terms[(2 s) ns + i] and the overlap term to terms[(2 s + 1) ns + i]
// (+0 for a skipped point); no grid walk.  With inlier masks (m x c bytes) it counts per s the inliers -> counters[2 s] and the correct
// inliers -> counters[2 s + 1].
__global__ __launch_bounds__(AB) void gt_batch_kernel(const float4* __restrict__ src, int ns, const float4* __restrict__ foot,
                                                      const GtBatchMats* __restrict__ mats, int m, float* __restrict__ terms,
                                                      const uint8_t* __restrict__ correct, const uint8_t* __restrict__ inl_masks, int c,
                                                      int* __restrict__ counters) {
    __shared__ GtBatchMats M[GTB_CHUNK];
    for (int k = threadIdx.x; k < 32 * m; k += AB) ((float*) M)[k] = ((const float*) mats)[k];
    __syncthreads();
    const int i = blockIdx.x * AB + threadIdx.x;
    if (i < ns) {
        const float4 P = src[(size_t) i * 3], Q = foot[i];
        const bool counted = Q.w != 0.f;
        for (int s = 0; s < m; ++s) {
            float bx, by, bz;
            se3(M[s].D, P.x, P.y, P.z, bx, by, bz);
            terms[(size_t) (2 * s) * ns + i] = sq3(P.x - bx, P.y - by, P.z - bz);   // dist2(p, D p), src/analysis.cpp:26-28
            float term = 0.f;
            if (counted) {
                float ax, ay, az;
                se3(M[s].T, P.x, P.y, P.z, ax, ay, az);
                const float d = __builtin_sqrtf(sq3(ax - Q.x, ay - Q.y, az - Q.z));   // src/analysis.cpp:77
                term = d * d;
            }
            terms[(size_t) (2 * s + 1) * ns + i] = term;
        }
    }
    if (!inl_masks) return;   // (uniform)
    const bool correct_i = i < c && correct[i];
    for (int s = 0; s < m; ++s) {
        const bool inl = i < c && inl_masks[(size_t) s * c + i];
        wave_count(inl, counters + 2 * s);
        wave_count(inl && correct_i, counters + 2 * s + 1);
    }
}

// one pass of mergeOverlaps (src/common.cpp:563-584): compared point i is in the overlap when its nearest reference point within the
// radius lies closer than thr to it along that point's normal (the squared distance stands in for a non-finite plane distance)
__global__ __launch_bounds__(AB) void gt_overlap_mask_kernel(GridDev ref, const float4* __restrict__ cmp, int n, float thr, float r2,
                                                             uint8_t* __restrict__ mask, int* __restrict__ counter) {
    const int i = blockIdx.x * AB + threadIdx.x;
    bool in = false;
    if (i < n) {
        const float4 P = cmp[(size_t) i * 3];
        float d2;
        int j;
        const int t = nearest_within(ref, P.x, P.y, P.z, r2, d2, j);
        if (t >= 0) {
            const float4 Q = ref.pxyz[t], N = ref.pnrm[t];
            float dp = fabsf(dot3(N.x, N.y, N.z, Q.x - P.x, Q.y - P.y, Q.z - P.z));
            dp = fin(dp) ? dp : d2;   // "normal can be invalid"
            in = dp < thr;
        }
        mask[i] = in ? 1 : 0;
    }
    wave_count(in, counter);
}

// calculateNormalDifference's per-point value (src/analysis.cpp:158-167) as a sort key: its bit pattern, or ~0 where the point does not count
__global__ __launch_bounds__(AB) void gt_normal_diff_kernel(const float4* __restrict__ aligned, int ns, const float4* __restrict__ tgt,
                                                            const int32_t* __restrict__ nn, const float* __restrict__ nn_d2, float thr,
                                                            unsigned* __restrict__ keys, int* __restrict__ counter) {
    const int i = blockIdx.x * AB + threadIdx.x;
    bool counted = false;
    if (i < ns) {
        unsigned key = 0xffffffffu;
        const int j = nn[i];
        if (j >= 0 && __builtin_sqrtf(nn_d2[i]) < thr) {
            const float4 A = aligned[(size_t) i * 3 + 1], B = tgt[(size_t) j * 3 + 1];
            if (fin(A.x) && fin(B.x)) {
                float cs = dot3(A.x, A.y, A.z, B.x, B.y, B.z);
                cs = cs < -1.f ? -1.f : (1.f < cs ? 1.f : cs);   // std::clamp
                const float v = fabsf(lgr_glibc::acosf_(cs));
                if (v >= 0.f) { key = __float_as_uint(v); counted = true; }
            }
        }
        keys[i] = key;
    }
    wave_count(counted, counter);
}

// (se3 / so3, the cloud move, the sequential f32 sum jobs and the overlap compaction are in lgr_pointpass.cuh)

// the correct correspondences with an infinite threshold (order free: the uniformity histogram counts a set)
__global__ __launch_bounds__(AB) void gt_compact_corr_kernel(const lgr_corr* __restrict__ corr, const uint8_t* __restrict__ correct, int c,
                                                             lgr_corr* __restrict__ out, int* __restrict__ n_out) {
    const int i = blockIdx.x * AB + threadIdx.x;
    if (i >= c || !correct[i]) return;
    lgr_corr cr = corr[i];
    cr.threshold = __uint_as_float(0x7f800000u);
    out[atomicAdd(n_out, 1)] = cr;
}

// ---------------------------------------------------------------------------------------------------- host side
// src/analysis.cpp:19-24 as the oracle states it (orc_rot_trans_diff): the angle of R1^T R2 from its unit quaternion, in double
void rot_trans_diff(const float* T1, const float* T2, float* angle, float* tdist) {
    double R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += (double) T1[4 * i + k] * (double) T2[4 * j + k];
            R[3 * i + j] = s;
        }
    const double tr = R[0] + R[4] + R[8];
    const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
    const double sn = 0.5 * std::sqrt(vx * vx + vy * vy + vz * vz), cs = 0.5 * (tr - 1.0);
    *angle = (float) std::atan2(sn, cs);
    const double dx = (double) T1[12] - T2[12], dy = (double) T1[13] - T2[13], dz = (double) T1[14] - T2[14];
    *tdist = (float) std::sqrt(dx * dx + dy * dy + dz * dz);
}

// T, G and D = T^-1 * G (the inverse by lgr_inverse4, the product in f32, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3) -> device
void form_D(const float* T, const float* G, float* D) {
    float inv[16];
    lgr_inverse4(T, inv);
    for (int col = 0; col < 4; ++col)
        for (int r = 0; r < 4; ++r)
            D[4 * col + r] = ((inv[r] * G[4 * col] + inv[4 + r] * G[4 * col + 1]) + inv[8 + r] * G[4 * col + 2]) + inv[12 + r] * G[4 * col + 3];
}

int upload_mats(lgr_ctx* ctx, const float* T16, const float* G16, const GtMats** d_mats, int** d_counters, float** d_sums) {
    GtMats m;
    memcpy(m.T, T16 ? T16 : G16, 64);
    memcpy(m.G, G16, 64);
    form_D(m.T, m.G, m.D);
    char* d;
    LGR_TRY(lgr_ws_t(ctx, WS_GT_MISC, 512, &d));
    LGR_HIP(ctx, hipMemsetAsync(d + 192, 0, 320, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(d, &m, sizeof m, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // m is a stack buffer
    *d_mats = (const GtMats*) d;
    *d_counters = (int*) (d + 192);    // 16 ints
    *d_sums = (float*) (d + 256);      // 8 floats
    return LGR_OK;
}

struct GtState {
    const GtMats* mats;
    int* counters;     // [0..3] gt_point_kernel, [4] overlap mask of the source, [5] of the target, [6] normal overlap, [7] correct correspondences compacted
    float* sums;       // [0] point-cloud terms, [1] overlap terms, [2] squared densities of the overlap cloud, [3] of the source
    float thr, r2;
};

// the target on a grid of cell 1.001 * (2 thr), built once per call: run_points and the first pass of run_merge walk the same one (nothing
// between them writes the WS_GRID_C slots: the k-nn pass builds in WS_GRID_A, the aligned source's grid goes to WS_GRID_B)
int target_grid(lgr_ctx* ctx, const GtState& st, const float* d_tgt, int nt, GridDev* g) {
    return lgr_grid_build(ctx, WS_GRID_C, d_tgt, nt, 2 * st.thr * 1.001f, 0.f, g);
}

struct PointsOut { float pcd_err, overlap_rmse; int overlap_size, n_correct, n_correct_inl, n_inl; };

// quantities 2, 3, 6 (and 7's count)
int run_points(lgr_ctx* ctx, const GtState& st, const GridDev& g, const float* d_src, int ns, const float* d_tgt, const lgr_corr* d_corr, int c,
               const uint8_t* d_inl, uint8_t* d_correct, int32_t* d_idx, PointsOut* out) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    *out = PointsOut{nan, nan, 0, 0, 0, 0};
    if (ns == 0) return LGR_OK;   // (no source point: no correspondence either)
    float* terms;
    LGR_TRY(lgr_ws_t(ctx, WS_GT_TERMS, (size_t) 2 * ns + 8, &terms));
    gt_point_kernel<<<cdiv(std::max(ns, c), AB), AB, 0, ctx->stream>>>(g, (const float4*) d_src, ns, (const float4*) d_tgt, d_corr, c, st.mats, st.thr, st.r2,
                                                                     terms, terms + ns, d_idx, d_inl, d_correct, st.counters);
    GtSumJobs jobs{};
    jobs.p[0] = terms; jobs.n[0] = ns; jobs.p[1] = terms + ns; jobs.n[1] = ns;
    gt_seqsum_kernel<<<2, AB, 0, ctx->stream>>>(jobs, st.sums);
    LGR_HIP(ctx, hipGetLastError());
    int cnt[4];
    float sums[2];
    LGR_TRY(read_words(ctx, st.counters, 4, cnt));
    LGR_TRY(read_words(ctx, st.sums, 2, sums));
    out->pcd_err = std::sqrt(sums[0] / (float) ns);
    out->overlap_size = cnt[0]; out->n_correct = cnt[1]; out->n_correct_inl = cnt[2]; out->n_inl = cnt[3];
    out->overlap_rmse = cnt[0] ? std::sqrt(sums[1] / (float) cnt[0]) : nan;
    return LGR_OK;
}

// quantities 6 and 7 alone: the correspondence half of gt_point_kernel (no source point: no grid walk, no term).  out3: correct, correct
// inliers, inliers
int run_correct(lgr_ctx* ctx, const GtState& st, const float* d_src, const float* d_tgt, const lgr_corr* d_corr, int c, const uint8_t* d_inl,
                uint8_t* d_correct, int out3[3]) {
    out3[0] = out3[1] = out3[2] = 0;
    if (c == 0) return LGR_OK;
    gt_point_kernel<<<cdiv(c, AB), AB, 0, ctx->stream>>>(GridDev{}, (const float4*) d_src, 0, (const float4*) d_tgt, d_corr, c, st.mats, st.thr, st.r2, nullptr,
                                                        nullptr, nullptr, d_inl, d_correct, st.counters);
    LGR_HIP(ctx, hipGetLastError());
    return read_words(ctx, st.counters + 1, 3, out3);
}

// run_points for n estimates (quantities 2, 3, 6 and 7's count): ONE grid walk and ONE correct-correspondence pass (gt_foot_kernel), then
// per chunk of GTB_CHUNK estimates one gt_batch_kernel and one launch of sum jobs; one upload before and one read-back after all chunks.
// shared: overlap_size and n_correct of every member.  d_inls: n x c bytes or nullptr.
struct BatchPoints { float pcd_err, overlap_rmse; int n_correct_inl, n_inl; };
int run_points_batch(lgr_ctx* ctx, const GtState& st, const GridDev& g, const float* d_src, int ns, const float* d_tgt, const lgr_corr* d_corr, int c,
                     const float* T16s, int n, const float* G16, const uint8_t* d_inls, uint8_t* d_correct, int shared[2], BatchPoints* out) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    shared[0] = shared[1] = 0;
    for (int s = 0; s < n; ++s) out[s] = BatchPoints{nan, nan, 0, 0};
    if (ns == 0) return LGR_OK;   // (no source point: no correspondence either)
    // WS_GTB_MISC: the n estimates' matrices, then 4 + 4 n result words: overlap_size, correct correspondences, two unused, per estimate
    // (inliers, correct inliers), then per estimate (sum of point-cloud terms, sum of overlap terms)
    std::vector<GtBatchMats> hm((size_t) n);
    for (int s = 0; s < n; ++s) {
        memcpy(hm[s].T, T16s + 16 * s, 64);
        form_D(hm[s].T, G16, hm[s].D);
    }
    char* d_misc;
    const size_t mats_bytes = (size_t) n * sizeof(GtBatchMats), res_words = 4 + 4 * (size_t) n;
    LGR_TRY(lgr_ws_t(ctx, WS_GTB_MISC, mats_bytes + res_words * 4, &d_misc));
    const GtBatchMats* d_mats = (const GtBatchMats*) d_misc;
    int* d_res = (int*) (d_misc + mats_bytes);
    int* d_cnt = d_res + 4;
    float* d_sums = (float*) (d_res + 4 + 2 * n);
    float4* foot;
    float* terms;
    LGR_TRY(lgr_ws_t(ctx, WS_GTB_FOOT, (size_t) ns + 1, &foot));
    LGR_TRY(lgr_ws_t(ctx, WS_GTB_TERMS, (size_t) 2 * GTB_CHUNK * ns + 8, &terms));
    LGR_HIP(ctx, hipMemsetAsync(d_res, 0, res_words * 4, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(d_misc, hm.data(), mats_bytes, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // hm is pageable memory of this frame
    const int blocks = cdiv(std::max(ns, c), AB);
    gt_foot_kernel<<<blocks, AB, 0, ctx->stream>>>(g, (const float4*) d_src, ns, (const float4*) d_tgt, d_corr, c, st.mats, st.thr, st.r2, foot, d_correct, d_res);
    for (int s0 = 0; s0 < n; s0 += GTB_CHUNK) {
        const int m = std::min(GTB_CHUNK, n - s0);
        gt_batch_kernel<<<blocks, AB, 0, ctx->stream>>>((const float4*) d_src, ns, foot, d_mats + s0, m, terms, d_correct,
                                                       d_inls ? d_inls + (size_t) s0 * c : nullptr, c, d_cnt + 2 * s0);
        GtSumJobsWide jobs{};
        for (int j = 0; j < 2 * m; ++j) jobs.p[j] = terms + (size_t) j * ns;
        jobs.n = ns;
        gt_seqsum_wide_kernel<<<2 * m, AB, 0, ctx->stream>>>(jobs, d_sums + 2 * s0);   // (the next chunk's terms wait for these sums: one stream)
    }
    LGR_HIP(ctx, hipGetLastError());
    void* h;
    LGR_TRY(lgr_pinned(ctx, res_words * 4, &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, d_res, res_words * 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int* hi = (const int*) h;
    const float* hs = (const float*) (hi + 4 + 2 * n);
    shared[0] = hi[0]; shared[1] = hi[1];
    for (int s = 0; s < n; ++s) {
        out[s].pcd_err = std::sqrt(hs[2 * s] / (float) ns);
        out[s].overlap_rmse = hi[0] ? std::sqrt(hs[2 * s + 1] / (float) hi[0]) : nan;
        out[s].n_inl = hi[4 + 2 * s]; out[s].n_correct_inl = hi[4 + 2 * s + 1];
    }
    return LGR_OK;
}

int align_source(lgr_ctx* ctx, const GtState& st, const float* d_src, int ns, float** d_aligned) {
    LGR_TRY(lgr_ws_t(ctx, WS_GT_ALIGNED, (size_t) 12 * ns + 16, d_aligned));
    if (ns > 0) pp_move_kernel<<<cdiv(ns, AB), AB, 0, ctx->stream>>>((const float4*) d_src, ns, st.mats->G, (float4*) *d_aligned);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// sum of the squared smoothed densities (k = 2, the default of include/common.h:290) of a cloud -> st.sums[slot]
int density_sq_sum(lgr_ctx* ctx, const GtState& st, const float* d_pts, int n, float* d_dens, int slot) {
    LGR_TRY(lgr_smoothed_densities_dev(ctx, d_pts, n, 2, d_dens));
    GtSumJobs jobs{};
    jobs.p[0] = d_dens; jobs.n[0] = n; jobs.sq[0] = 1;
    gt_seqsum_kernel<<<1, AB, 0, ctx->stream>>>(jobs, st.sums + slot);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// quantity 5 (gt: the target's grid, unused when either cloud is empty; overlap_area == nullptr: masks, counts and overlap only, without
// the two density passes)
int run_merge(lgr_ctx* ctx, const GtState& st, const GridDev& gt, const float* d_src, const float* d_aligned, int ns, const float* d_tgt, int nt,
              uint8_t* d_mask_src, uint8_t* d_mask_tgt, int n2[2], float* overlap, float* overlap_area) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    n2[0] = n2[1] = 0;
    *overlap = 0.f / (float) (ns + nt);
    if (overlap_area) *overlap_area = nan;
    if (ns == 0 || nt == 0) {
        if (d_mask_src && ns) LGR_HIP(ctx, hipMemsetAsync(d_mask_src, 0, (size_t) ns, ctx->stream));
        if (d_mask_tgt && nt) LGR_HIP(ctx, hipMemsetAsync(d_mask_tgt, 0, (size_t) nt, ctx->stream));
        return LGR_OK;
    }
    const size_t n = (size_t) ns + nt;
    int* flags;
    LGR_TRY(lgr_ws_t(ctx, WS_GT_FLAGS, 2 * n + (n + 3) / 4 + 16, &flags));
    int* pos = flags + n;
    uint8_t* own = (uint8_t*) (pos + n);
    if (!d_mask_src) d_mask_src = own;
    if (!d_mask_tgt) d_mask_tgt = own + ns;
    GridDev gs{};
    gt_overlap_mask_kernel<<<cdiv(ns, AB), AB, 0, ctx->stream>>>(gt, (const float4*) d_aligned, ns, st.thr, st.r2, d_mask_src, st.counters + 4);
    LGR_TRY(lgr_grid_build(ctx, WS_GRID_B, d_aligned, ns, 2 * st.thr * 1.001f, 0.f, &gs));   // the aligned source's own grid
    gt_overlap_mask_kernel<<<cdiv(nt, AB), AB, 0, ctx->stream>>>(gs, (const float4*) d_tgt, nt, st.thr, st.r2, d_mask_tgt, st.counters + 5);
    LGR_HIP(ctx, hipGetLastError());
    LGR_TRY(read_words(ctx, st.counters + 4, 2, n2));
    const int no = n2[0] + n2[1];
    *overlap = (float) no / (float) (ns + nt);
    if (!overlap_area || no < 2 || ns < 2) return LGR_OK;   // calculateSmoothedDensities would rassert (src/common.cpp:532)
    pp_flags_kernel<<<cdiv((long long) n, AB), AB, 0, ctx->stream>>>(d_mask_src, ns, d_mask_tgt, nt, flags);
    LGR_TRY(pp_scan_flags(ctx, flags, pos, n));
    float *d_ov, *d_dens;
    LGR_TRY(lgr_ws_t(ctx, WS_GT_OVERLAP, (size_t) 12 * no + 16, &d_ov));
    LGR_TRY(lgr_ws_t(ctx, WS_GT_DENS, (size_t) std::max(no, ns) + 16, &d_dens));
    pp_compact_rows_kernel<<<cdiv((long long) n, AB), AB, 0, ctx->stream>>>((const float4*) d_aligned, ns, (const float4*) d_tgt, nt, flags, pos, (float4*) d_ov);
    LGR_HIP(ctx, hipGetLastError());
    LGR_TRY(density_sq_sum(ctx, st, d_ov, no, d_dens, 2));
    LGR_TRY(density_sq_sum(ctx, st, d_src, ns, d_dens, 3));
    float s[2];
    LGR_TRY(read_words(ctx, st.sums + 2, 2, s));
    *overlap_area = s[0] / s[1];
    return LGR_OK;
}

// quantity 4
int run_normal_diff(lgr_ctx* ctx, const GtState& st, const float* d_aligned, int ns, const float* d_tgt, int nt, float* normal_diff, int* n_overlap) {
    *normal_diff = GT_PI;
    *n_overlap = 0;
    if (ns == 0 || nt == 0) return LGR_OK;
    const size_t nn = ((size_t) ns + 63) & ~(size_t) 63;
    int32_t* buf;
    LGR_TRY(lgr_ws_t(ctx, WS_GT_KNN, 6 * nn + 16, &buf));
    int32_t* idx = buf;
    float* d2 = (float*) (buf + nn);
    unsigned *keys = (unsigned*) (buf + 2 * nn), *keys2 = keys + nn;
    int *vals = (int*) (keys2 + nn), *vals2 = vals + nn;
    LGR_TRY(lgr_knn_lists(ctx, d_aligned, ns, d_tgt, nt, 1, idx, d2));   // nearestKSearch(..., 1): ascending (d2, index)
    gt_normal_diff_kernel<<<cdiv(ns, AB), AB, 0, ctx->stream>>>((const float4*) d_aligned, ns, (const float4*) d_tgt, idx, d2, st.thr, keys, st.counters + 6);
    LGR_HIP(ctx, hipGetLastError());
    LGR_TRY(lgr_sort_pairs_u32(ctx, keys, keys2, vals, vals2, (size_t) ns, 0, 32));
    LGR_TRY(read_words(ctx, st.counters + 6, 1, n_overlap));
    if (*n_overlap > 0) LGR_TRY(read_words(ctx, keys2 + *n_overlap / 2, 1, normal_diff));
    return LGR_OK;
}

// quantity 8: the uniformity the RANSAC metric evaluates (lgr_evaluate_dev, LGR_METRIC_UNIFORMITY) over the correct correspondences -- each
// handed over with an infinite threshold, so that the inlier set of that evaluation IS the set (the points of a correct correspondence
// are finite); the bounding box is the source cloud's, as calculateCorrespondenceUniformity(src, correct) takes it
int run_uniformity(lgr_ctx* ctx, const GtState& st, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                   const uint8_t* d_correct, lgr_corr* cc, int n_correct, const float* G16, float* uniformity) {
    *uniformity = 0.f;
    if (n_correct == 0) return LGR_OK;
    gt_compact_corr_kernel<<<cdiv(c, AB), AB, 0, ctx->stream>>>(d_corr, d_correct, c, cc, st.counters + 7);
    LGR_HIP(ctx, hipGetLastError());
    int n_inl = 0;
    float rmse = 0.f;
    LGR_TRY(lgr_evaluate_dev(ctx, d_src, ns, d_tgt, nt, cc, n_correct, G16, LGR_METRIC_UNIFORMITY, LGR_SCORE_MSE, nullptr, &n_inl, &rmse, uniformity));
    return LGR_OK;
}

// WS_GT_CORR, requested once per call: room for the c compacted correct correspondences, then the c bytes of the correct mask for a
// caller that passes none
int corr_storage(lgr_ctx* ctx, int c, lgr_corr** cc, uint8_t** own_mask) {
    LGR_TRY(lgr_ws_t(ctx, WS_GT_CORR, (size_t) c + (size_t) (c + 15) / 16 + 16, cc));
    *own_mask = (uint8_t*) (*cc + c);
    return LGR_OK;
}

int begin(lgr_ctx* ctx, const float* T16, const float* G16, float thr, GtState* st) {
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    LGR_TRY(upload_mats(ctx, T16, G16, &st->mats, &st->counters, &st->sums));
    st->thr = thr;
    const float radius = 2 * thr;   // DIST_TO_PLANE_COEFFICIENT * distance_thr
    st->r2 = radius * radius;
    return LGR_OK;
}

#define GT_CHECK_CLOUDS(ctx)                                                                                                          \
    LGR_CHECK(ctx, ns >= 0 && nt >= 0 && (d_src || ns == 0) && (d_tgt || nt == 0) && aligned16(d_src) && aligned16(d_tgt) && distance_thr > 0.f && \
                   distance_thr <= 1e18f, LGR_ERR_INVALID_ARG)

}  // namespace

extern "C" int lgr_overlap_rmse_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16], const float Tgt16[16],
                                    float distance_thr, float* overlap_rmse, int* overlap_size, float* pcd_err, int32_t* d_idx) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    GT_CHECK_CLOUDS(ctx);
    LGR_CHECK(ctx, T16 && Tgt16 && overlap_rmse && overlap_size, LGR_ERR_INVALID_ARG);
    GtState st;
    LGR_TRY(begin(ctx, T16, Tgt16, distance_thr, &st));
    GridDev g{};
    if (ns > 0) LGR_TRY(target_grid(ctx, st, d_tgt, nt, &g));
    PointsOut po;
    LGR_TRY(run_points(ctx, st, g, d_src, ns, d_tgt, nullptr, 0, nullptr, nullptr, d_idx, &po));
    *overlap_rmse = po.overlap_rmse; *overlap_size = po.overlap_size;
    if (pcd_err) *pcd_err = po.pcd_err;
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_merge_overlaps_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float Tgt16[16], float distance_thr,
                                      uint8_t* d_mask_src, uint8_t* d_mask_tgt, int n_overlap2[2], float* overlap, float* overlap_area) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    GT_CHECK_CLOUDS(ctx);
    LGR_CHECK(ctx, Tgt16 && n_overlap2 && overlap, LGR_ERR_INVALID_ARG);
    GtState st;
    LGR_TRY(begin(ctx, nullptr, Tgt16, distance_thr, &st));
    float* d_aligned;
    LGR_TRY(align_source(ctx, st, d_src, ns, &d_aligned));
    GridDev g{};
    if (ns > 0 && nt > 0) LGR_TRY(target_grid(ctx, st, d_tgt, nt, &g));
    LGR_TRY(run_merge(ctx, st, g, d_src, d_aligned, ns, d_tgt, nt, d_mask_src, d_mask_tgt, n_overlap2, overlap, overlap_area));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_normal_difference_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float Tgt16[16], float distance_thr,
                                         float* normal_diff, int* n_normal_overlap) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    GT_CHECK_CLOUDS(ctx);
    LGR_CHECK(ctx, Tgt16 && normal_diff && n_normal_overlap, LGR_ERR_INVALID_ARG);
    GtState st;
    LGR_TRY(begin(ctx, nullptr, Tgt16, distance_thr, &st));
    float* d_aligned;
    LGR_TRY(align_source(ctx, st, d_src, ns, &d_aligned));
    LGR_TRY(run_normal_diff(ctx, st, d_aligned, ns, d_tgt, nt, normal_diff, n_normal_overlap));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_correct_correspondences_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                                               const float Tgt16[16], const uint8_t* d_inlier_mask, uint8_t* d_correct_mask, int n3[3]) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, ns >= 0 && nt >= 0 && c >= 0 && (d_src || ns == 0) && (d_tgt || nt == 0) && (d_corr || c == 0) && aligned16(d_src) && aligned16(d_tgt) &&
                       Tgt16 && n3 && (c == 0 || (ns > 0 && nt > 0)), LGR_ERR_INVALID_ARG);
    GtState st;
    LGR_TRY(begin(ctx, nullptr, Tgt16, 1.f, &st));
    LGR_TRY(lgr_check_corr(ctx, d_corr, c, ns, nt));   // before the kernel gathers points through the indices
    LGR_TRY(run_correct(ctx, st, d_src, d_tgt, d_corr, c, d_inlier_mask, d_correct_mask, n3));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_evaluate_gt_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c, const float T16[16],
                                   const float Tgt16[16], float distance_thr, int converged, const uint8_t* d_inlier_mask, lgr_gt_eval* out,
                                   uint8_t* d_correct_mask) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    GT_CHECK_CLOUDS(ctx);
    LGR_CHECK(ctx, T16 && Tgt16 && out && c >= 0 && (d_corr || c == 0), LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, c == 0 || (ns > 0 && nt > 0), LGR_ERR_INVALID_ARG);   // a correspondence needs a point on either side
    GtState st;
    LGR_TRY(begin(ctx, T16, Tgt16, distance_thr, &st));
    LGR_TRY(lgr_check_corr(ctx, d_corr, c, ns, nt));   // before any kernel gathers points through the indices
    memset(out, 0, sizeof *out);
    rot_trans_diff(T16, Tgt16, &out->r_err, &out->t_err);
    lgr_corr* d_cc = nullptr;
    uint8_t *d_correct = d_correct_mask, *d_own = nullptr;
    if (c > 0) LGR_TRY(corr_storage(ctx, c, &d_cc, &d_own));
    if (!d_correct) d_correct = d_own;
    GridDev g{};
    if (ns > 0) LGR_TRY(target_grid(ctx, st, d_tgt, nt, &g));
    PointsOut po;
    LGR_TRY(run_points(ctx, st, g, d_src, ns, d_tgt, d_corr, c, d_inlier_mask, d_correct, nullptr, &po));
    out->pcd_err = po.pcd_err; out->overlap_rmse = po.overlap_rmse; out->overlap_size = po.overlap_size;
    out->n_correspondences = c; out->n_correct_correspondences = po.n_correct; out->n_inliers = po.n_inl; out->n_correct_inliers = po.n_correct_inl;
    float* d_aligned;
    LGR_TRY(align_source(ctx, st, d_src, ns, &d_aligned));
    LGR_TRY(run_normal_diff(ctx, st, d_aligned, ns, d_tgt, nt, &out->normal_diff, &out->n_normal_overlap));
    int n2[2];
    LGR_TRY(run_merge(ctx, st, g, d_src, d_aligned, ns, d_tgt, nt, nullptr, nullptr, n2, &out->overlap, &out->overlap_area));
    out->n_overlap_src = n2[0]; out->n_overlap_tgt = n2[1]; out->n_overlap = n2[0] + n2[1];
    LGR_TRY(run_uniformity(ctx, st, d_src, ns, d_tgt, nt, d_corr, c, d_correct, d_cc, po.n_correct, Tgt16, &out->corr_uniformity));
    out->converged = converged ? 1 : 0;
    out->converged_and_overlap_ok = (converged && out->overlap_rmse < distance_thr) ? 1 : 0;
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

// n estimates against one ground truth.  What AlignmentAnalysis::start computes from the ground truth alone -- the overlap set of
// calculateOverlapRmse (src/analysis.cpp:69-76), the correct correspondences and their uniformity, the normal difference, mergeOverlaps
// with its two density passes -- runs once; only the last distance of the overlap error (:77), the point-cloud error and the counts
// of an inlier mask run per estimate, GTB_CHUNK estimates to a launch (run_points_batch).
extern "C" int lgr_evaluate_gt_batch_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c, const float* T16s,
                                         int n, const float Tgt16[16], float distance_thr, const int32_t* converged, const uint8_t* d_inlier_masks,
                                         lgr_gt_eval* out, uint8_t* d_correct_mask) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, n <= LGR_GT_BATCH_MAX, LGR_ERR_UNSUPPORTED);
    GT_CHECK_CLOUDS(ctx);
    LGR_CHECK(ctx, Tgt16 && c >= 0 && (d_corr || c == 0) && (n == 0 || (T16s && converged && out)), LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, c == 0 || (ns > 0 && nt > 0), LGR_ERR_INVALID_ARG);   // a correspondence needs a point on either side
    if (n == 0) return LGR_OK;
    GtState st;
    LGR_TRY(begin(ctx, nullptr, Tgt16, distance_thr, &st));   // (the state's own estimate is the ground truth: nothing below reads it)
    LGR_TRY(lgr_check_corr(ctx, d_corr, c, ns, nt));   // before any kernel gathers points through the indices
    lgr_corr* d_cc = nullptr;
    uint8_t *d_correct = d_correct_mask, *d_own = nullptr;
    if (c > 0) LGR_TRY(corr_storage(ctx, c, &d_cc, &d_own));
    if (!d_correct) d_correct = d_own;
    GridDev g{};
    if (ns > 0) LGR_TRY(target_grid(ctx, st, d_tgt, nt, &g));
    int shared[2];
    BatchPoints bp[LGR_GT_BATCH_MAX];
    LGR_TRY(run_points_batch(ctx, st, g, d_src, ns, d_tgt, d_corr, c, T16s, n, Tgt16, c > 0 ? d_inlier_masks : nullptr, d_correct, shared, bp));
    lgr_gt_eval e;   // the fields every member shares
    memset(&e, 0, sizeof e);
    e.overlap_size = shared[0];
    e.n_correspondences = c; e.n_correct_correspondences = shared[1];
    float* d_aligned;
    LGR_TRY(align_source(ctx, st, d_src, ns, &d_aligned));
    LGR_TRY(run_normal_diff(ctx, st, d_aligned, ns, d_tgt, nt, &e.normal_diff, &e.n_normal_overlap));
    int n2[2];
    LGR_TRY(run_merge(ctx, st, g, d_src, d_aligned, ns, d_tgt, nt, nullptr, nullptr, n2, &e.overlap, &e.overlap_area));
    e.n_overlap_src = n2[0]; e.n_overlap_tgt = n2[1]; e.n_overlap = n2[0] + n2[1];
    LGR_TRY(run_uniformity(ctx, st, d_src, ns, d_tgt, nt, d_corr, c, d_correct, d_cc, shared[1], Tgt16, &e.corr_uniformity));
    for (int s = 0; s < n; ++s) {
        out[s] = e;
        rot_trans_diff(T16s + 16 * s, Tgt16, &out[s].r_err, &out[s].t_err);
        out[s].pcd_err = bp[s].pcd_err; out[s].overlap_rmse = bp[s].overlap_rmse;
        out[s].n_inliers = bp[s].n_inl; out[s].n_correct_inliers = bp[s].n_correct_inl;
        out[s].converged = converged[s] ? 1 : 0;
        out[s].converged_and_overlap_ok = (converged[s] && out[s].overlap_rmse < distance_thr) ? 1 : 0;
    }
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

namespace {
// (the host twins stage their arrays through lgr_host_call, lgr_host.h; two masks of one call share a staged buffer)
#define GT_CHECK_HOST_CLOUDS(ctx) LGR_CHECK(ctx, ns >= 0 && nt >= 0 && (src || ns == 0) && (tgt || nt == 0), LGR_ERR_INVALID_ARG)
}  // namespace

extern "C" int lgr_overlap_rmse(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float T16[16], const float Tgt16[16],
                                float distance_thr, float* overlap_rmse, int* overlap_size, float* pcd_err, int32_t* idx) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    GT_CHECK_HOST_CLOUDS(ctx);
    float *ds, *dt;
    int32_t* di = nullptr;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    if (idx && ns) LGR_TRY(hc.out((size_t) ns, &di, 4));   // (slack kept from before; no reader past ns is known)
    LGR_TRY(lgr_overlap_rmse_dev(ctx, ds, ns, dt, nt, T16, Tgt16, distance_thr, overlap_rmse, overlap_size, pcd_err, di));
    if (di) LGR_TRY(hc.fetch(idx, di, (size_t) ns));
    return hc.finish();
}

extern "C" int lgr_merge_overlaps(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float Tgt16[16], float distance_thr,
                                  uint8_t* mask_src, uint8_t* mask_tgt, int n_overlap2[2], float* overlap, float* overlap_area) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    GT_CHECK_HOST_CLOUDS(ctx);
    float *ds, *dt;
    uint8_t* dm;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.out((size_t) ns + (size_t) nt, &dm, LGR_PAD_MASK));   // both masks in one buffer
    LGR_TRY(lgr_merge_overlaps_dev(ctx, ds, ns, dt, nt, Tgt16, distance_thr, dm, dm + ns, n_overlap2, overlap, overlap_area));
    LGR_TRY(hc.fetch(mask_src, dm, (size_t) ns));
    LGR_TRY(hc.fetch(mask_tgt, dm + ns, (size_t) nt));
    return hc.finish();
}

extern "C" int lgr_normal_difference(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float Tgt16[16], float distance_thr,
                                     float* normal_diff, int* n_normal_overlap) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    GT_CHECK_HOST_CLOUDS(ctx);
    float *ds, *dt;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    return lgr_normal_difference_dev(ctx, ds, ns, dt, nt, Tgt16, distance_thr, normal_diff, n_normal_overlap);
}

extern "C" int lgr_correct_correspondences(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                                           const float Tgt16[16], const uint8_t* inlier_mask, uint8_t* correct_mask, int n3[3]) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    GT_CHECK_HOST_CLOUDS(ctx);
    LGR_CHECK(ctx, c >= 0 && (corr || c == 0), LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_corr* dc;
    uint8_t* dm;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    LGR_TRY(hc.in(inlier_mask, (size_t) c, &dm, (size_t) c + LGR_PAD_MASK));   // the inlier mask, then the correct mask
    LGR_TRY(lgr_correct_correspondences_dev(ctx, ds, ns, dt, nt, c ? dc : nullptr, c, Tgt16, (c && inlier_mask) ? dm : nullptr,
                                            (c && correct_mask) ? dm + c : nullptr, n3));
    LGR_TRY(hc.fetch(correct_mask, dm + c, (size_t) c));
    return hc.finish();
}

extern "C" int lgr_evaluate_gt_batch(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c, const float* T16s, int n,
                                     const float Tgt16[16], float distance_thr, const int32_t* converged, const uint8_t* inlier_masks, lgr_gt_eval* out,
                                     uint8_t* correct_mask) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, ns >= 0 && nt >= 0 && c >= 0 && n >= 0 && (src || ns == 0) && (tgt || nt == 0) && (corr || c == 0) && Tgt16, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, n <= LGR_GT_BATCH_MAX, LGR_ERR_UNSUPPORTED);
    float *ds, *dt;
    lgr_corr* dc;
    uint8_t* dm;   // the correct mask, then the n inlier masks
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    LGR_TRY(hc.out((size_t) (n + 1) * c, &dm, LGR_PAD_MASK));
    const bool masks = c && n && inlier_masks;
    if (masks) LGR_HIP(ctx, hipMemcpyAsync(dm + c, inlier_masks, (size_t) n * c, hipMemcpyHostToDevice, ctx->stream));   // behind the correct mask
    LGR_TRY(lgr_evaluate_gt_batch_dev(ctx, ds, ns, dt, nt, c ? dc : nullptr, c, T16s, n, Tgt16, distance_thr, converged, masks ? dm + c : nullptr, out,
                                      (c && correct_mask) ? dm : nullptr));
    if (n) LGR_TRY(hc.fetch(correct_mask, dm, (size_t) c));
    return hc.finish();
}

extern "C" int lgr_evaluate_gt(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c, const float T16[16],
                               const float Tgt16[16], float distance_thr, int converged, const uint8_t* inlier_mask, lgr_gt_eval* out,
                               uint8_t* correct_mask) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, ns >= 0 && nt >= 0 && c >= 0 && (src || ns == 0) && (tgt || nt == 0) && (corr || c == 0) && T16 && Tgt16 && out, LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_corr* dc;
    uint8_t* dm;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    LGR_TRY(hc.in(inlier_mask, (size_t) c, &dm, (size_t) c + LGR_PAD_MASK));   // the inlier mask, then the correct mask
    LGR_TRY(lgr_evaluate_gt_dev(ctx, ds, ns, dt, nt, c ? dc : nullptr, c, T16, Tgt16, distance_thr, converged,
                                (c && inlier_mask) ? dm : nullptr, out, (c && correct_mask) ? dm + c : nullptr));
    LGR_TRY(hc.fetch(correct_mask, dm + c, (size_t) c));
    return hc.finish();
}
