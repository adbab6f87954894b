// lgr_align.hip -- match filters (OneSided / LeftToRight / Cluster / Ratio), correspondence search and alignPointClouds.
//
//   include/matching.h:395-411, 428-453, 492-550  -> lgr_filter_dev
//   src/correspondence_search.cpp:4-15 + include/matching.h:148-262 (keypoint 'any', single scale) -> lgr_correspondences*
//   src/alignment.cpp:72-109 (RANSAC branch; CSV side effects dropped)                          -> lgr_align*
//   include/matching.h:132-146, 164-262 (one Storage per cloud, filled once)                    -> lgr_cloud_fill, lgr_*_prepared*
#include <rocprim/device/device_scan.hpp>

#include <chrono>
#include <cmath>

#include <climits>

#include "lgr_cloud.h"
#include "lgr_host.h"

namespace {

// threshold = std::min(std::max(thr_s[i], thr_t[j]), distance_thr)
__device__ __forceinline__ float corr_threshold(float a, float b, float dthr) {
    float m = (a < b) ? b : a;          // std::max(a, b)
    return (dthr < m) ? dthr : m;       // std::min(m, dthr)
}

// calculateCorrespondenceDistance (include/matching.h:524-550) with randomness = 1: of the k spatial neighbours of i that
// have a match, the share whose match is NOT among the k spatial neighbours of j.  The neighbour list of j is read once
// into registers (KMAX ints), so the k x k membership test touches no memory (it was 1600 dependent global loads per
// correspondence and direction: 44 ms at 1M in the cluster mode).
template <int KMAX>
__device__ __forceinline__ float cluster_distance(int i, int j, int k, const int32_t* __restrict__ knn_a, const int32_t* __restrict__ knn_b,
                                                   const int32_t* __restrict__ ab_idx) {
    int nb[KMAX];
#pragma unroll
    for (int b = 0; b < KMAX; ++b) nb[b] = b < k ? knn_b[(size_t) j * k + b] : -2;   // -2 never equals a match index
    int consistent = 0, pairs = 0;
    // eight neighbours per round: their indices, then their matches, are requested together (index -> match is a dependent gather; one
    // neighbour per round was 2 k memory round trips in a row per correspondence and direction: 2.5 ms at 1M, k = 40)
    for (int a0 = 0; a0 < k; a0 += 8) {
        int in[8], mt[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) in[u] = a0 + u < k ? knn_a[(size_t) i * k + a0 + u] : -1;
#pragma unroll
        for (int u = 0; u < 8; ++u) mt[u] = in[u] >= 0 ? ab_idx[in[u]] : -1;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (mt[u] < 0) continue;
            bool hit = false;
#pragma unroll
            for (int b = 0; b < KMAX; ++b) hit = hit || (nb[b] == mt[u]);
            consistent += hit ? 1 : 0;
            pairs++;
        }
    }
    if (pairs == 0) return 0.f;
    return 1.f - (float) consistent / (float) pairs;
}

template <int KMAX>
__global__ void filter_flags(int matching_id, int ns, const int32_t* __restrict__ ij, const float* __restrict__ dij,
                             const int32_t* __restrict__ ji, const float* __restrict__ dji,
                             const int32_t* __restrict__ knn_s, const int32_t* __restrict__ knn_t, int k,
                             int* __restrict__ flags, float* __restrict__ dist) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    int j = ij[i];
    int keep = 0;
    float d = 0.f;
    if (j >= 0) {
        if (matching_id == LGR_MATCH_ONE_SIDED) { keep = 1; d = dij[i]; }
        else if (matching_id == LGR_MATCH_LR) { keep = ji[j] == i ? 1 : 0; d = dji[j]; }   // reverse-direction distance (:444)
        else {
            float di = cluster_distance<KMAX>(i, j, k, knn_s, knn_t, ij);
            float dj = cluster_distance<KMAX>(j, i, k, knn_t, knn_s, ji);
            keep = (di < 0.95f && dj < 0.95f) ? 1 : 0;      // MATCHING_CLUSTER_THRESHOLD include/common.h:52
            d = (di < dj) ? dj : di;                         // std::max(distance_i, distance_j)
        }
    }
    flags[i] = keep; dist[i] = d;
}

__global__ void filter_emit(int ns, const int32_t* __restrict__ ij, const int* __restrict__ flags, const int* __restrict__ pos,
                            const float* __restrict__ dist, const float* __restrict__ thr_s, const float* __restrict__ thr_t,
                            float distance_thr, lgr_corr* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns || !flags[i]) return;
    int j = ij[i];
    lgr_corr c;
    c.index_query = i; c.index_match = j; c.distance = dist[i];
    c.threshold = corr_threshold(thr_s[i], thr_t[j], distance_thr);
    out[pos[i]] = c;
}

}  // namespace

// the filter's per-cloud tables: smoothed densities (thresholds) of both key-point clouds and, for the cluster filter, their
// k-NN lists.  They depend on the clouds only, not on the matches.
struct FilterTables { float *thr_s = nullptr, *thr_t = nullptr; int32_t *knn_s = nullptr, *knn_t = nullptr; };
static int filter_tables_alloc(lgr_ctx* ctx, int matching_id, int ns, int nt, int cluster_k, FilterTables* ft) {
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_MISC, (size_t) ns + nt + 16, &ft->thr_s));
    ft->thr_t = ft->thr_s + ns;
    if (matching_id == LGR_MATCH_CLUSTER) {
        LGR_TRY(lgr_ws_t(ctx, WS_PIPE_KNN_S, (size_t) ns * cluster_k, &ft->knn_s));
        LGR_TRY(lgr_ws_t(ctx, WS_PIPE_KNN_T, (size_t) nt * cluster_k, &ft->knn_t));
    }
    return LGR_OK;
}
static int filter_cloud_tables(lgr_ctx* cx, const float* pts, int n, int cluster_k, float* thr, int32_t* knn) {
    LGR_TRY(lgr_smoothed_densities_dev(cx, pts, n, 2, thr));   // calculateSmoothedDensities(kps) (include/matching.h:396-397 etc.)
    if (knn) {
        LGR_TRY(lgr_knn_lists(cx, pts, n, pts, n, cluster_k, knn, nullptr));   // (membership tests only: no distance table)
    }
    return LGR_OK;
}
static int filter_core(lgr_ctx* ctx, int matching_id, int ns, const int32_t* d_ij_idx, const float* d_ij_dist, const int32_t* d_ji_idx, const float* d_ji_dist,
                       float distance_thr, int cluster_k, const FilterTables& ft, lgr_corr* d_out, int* n_out);

extern "C" int lgr_filter_dev(lgr_ctx* ctx, int matching_id, const float* d_src, int ns, const float* d_tgt, int nt,
                              const int32_t* d_ij_idx, const float* d_ij_dist, const int32_t* d_ji_idx, const float* d_ji_dist,
                              float distance_thr, int cluster_k, lgr_corr* d_out, int* n_out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, d_src && d_tgt && d_ij_idx && d_ij_dist && d_out && n_out && ns > 1 && nt > 1, LGR_ERR_INVALID_ARG);
    if (matching_id == LGR_MATCH_RATIO) matching_id = LGR_MATCH_ONE_SIDED;   // OneSidedMatcher's loop over the entries the ratio test left
    LGR_CHECK(ctx, matching_id == LGR_MATCH_LR || matching_id == LGR_MATCH_ONE_SIDED || matching_id == LGR_MATCH_CLUSTER, LGR_ERR_INVALID_ARG);
    if (matching_id != LGR_MATCH_ONE_SIDED) LGR_CHECK(ctx, d_ji_idx && d_ji_dist, LGR_ERR_INVALID_ARG);
    if (matching_id == LGR_MATCH_CLUSTER) LGR_CHECK(ctx, cluster_k >= 1 && cluster_k <= 64, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    *n_out = 0;
    FilterTables ft;
    LGR_TRY(filter_tables_alloc(ctx, matching_id, ns, nt, cluster_k, &ft));
    // the two clouds' tables side by side on the two contexts
    LGR_TRY(lgr_run_pair(ctx, [&](lgr_ctx* cx) { return filter_cloud_tables(cx, d_src, ns, cluster_k, ft.thr_s, ft.knn_s); },
                         [&](lgr_ctx* cx) { return filter_cloud_tables(cx, d_tgt, nt, cluster_k, ft.thr_t, ft.knn_t); }));
    return filter_core(ctx, matching_id, ns, d_ij_idx, d_ij_dist, d_ji_idx, d_ji_dist, distance_thr, cluster_k, ft, d_out, n_out);
}

static int filter_core(lgr_ctx* ctx, int matching_id, int ns, const int32_t* d_ij_idx, const float* d_ij_dist, const int32_t* d_ji_idx, const float* d_ji_dist,
                       float distance_thr, int cluster_k, const FilterTables& ft, lgr_corr* d_out, int* n_out) {
    float *thr_s = ft.thr_s, *thr_t = ft.thr_t;
    int32_t *knn_s = ft.knn_s, *knn_t = ft.knn_t;
    *n_out = 0;
    int *flags, *pos;
    float* dist;
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_FLAGS, (size_t) ns * 3 + 16, &flags));
    pos = flags + ns; dist = (float*) (pos + ns);
    if (matching_id != LGR_MATCH_CLUSTER) filter_flags<1><<<cdiv(ns, 128), 128, 0, ctx->stream>>>(matching_id, ns, d_ij_idx, d_ij_dist, d_ji_idx, d_ji_dist, knn_s, knn_t, cluster_k, flags, dist);
    else if (cluster_k <= 40) filter_flags<40><<<cdiv(ns, 128), 128, 0, ctx->stream>>>(matching_id, ns, d_ij_idx, d_ij_dist, d_ji_idx, d_ji_dist, knn_s, knn_t, cluster_k, flags, dist);
    else filter_flags<64><<<cdiv(ns, 128), 128, 0, ctx->stream>>>(matching_id, ns, d_ij_idx, d_ij_dist, d_ji_idx, d_ji_dist, knn_s, knn_t, cluster_k, flags, dist);
    size_t tb = 0;
    LGR_HIP(ctx, rocprim::exclusive_scan(nullptr, tb, flags, pos, 0, (size_t) ns, rocprim::plus<int>(), ctx->stream));
    void* tmp;
    LGR_TRY(lgr_ws(ctx, WS_GRID_TMP, tb, &tmp));
    LGR_HIP(ctx, rocprim::exclusive_scan(tmp, tb, flags, pos, 0, (size_t) ns, rocprim::plus<int>(), ctx->stream));
    filter_emit<<<cdiv(ns, 256), 256, 0, ctx->stream>>>(ns, d_ij_idx, flags, pos, dist, thr_s, thr_t, distance_thr, d_out);
    int* h;
    LGR_TRY(lgr_pinned(ctx, 64, (void**) &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, pos + (ns - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(h + 1, flags + (ns - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = h[0] + h[1];
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

static void tick(lgr_ctx* ctx, int i) { (void) hipEventRecord(ctx->ev[i], ctx->stream); }

// rows of 12 floats picked by index: the key-point cloud pcd[kps_indices] (pcl::copyPointCloud, include/matching.h:167) and the
// per-level key-point sub-clouds of the multi-scale path
__global__ void gather_rows12_kernel(const float* __restrict__ pts, const int32_t* __restrict__ idx, int m, float* __restrict__ out) {
    size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t) m * 12) return;
    out[e] = pts[(size_t) idx[e / 12] * 12 + e % 12];
}
static void gather_rows12(lgr_ctx* ctx, const float* pts, const int32_t* idx, int m, float* out) {
    gather_rows12_kernel<<<cdiv((long long) m * 12, 256), 256, 0, ctx->stream>>>(pts, idx, m, out);
}
// finalize (include/matching.h:150-160): local key-point indices -> indices of the clouds
__global__ void finalize_kernel(lgr_corr* __restrict__ corr, int n, const int32_t* __restrict__ ks, const int32_t* __restrict__ kt) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    corr[i].index_query = ks[corr[i].index_query];
    corr[i].index_match = kt[corr[i].index_match];
}

// ---- the descriptors of the correspondence search (lgr_feature_params), one table entry each
typedef int (*FeatureStage)(lgr_ctx* ctx, const float* kps, int m, const float* surf, int n, float radius, float* out, const lgr_params* p, const float* vp);
struct Descriptor {
    int len;              // floats per row
    FeatureStage stage;   // rows of m > 0 key points on a level's surface
    bool dense;           // matched by lgr_match_dense (brute force only); FPFH has the guess / FLANN / brute-force dispatch and lgr_match_prepare
    int lrf;              // the one lrf_id that is built (FPFH never reads lrf_id, include/common.h:366,407)
};
static int fpfh_stage(lgr_ctx* ctx, const float* kps, int m, const float* surf, int n, float radius, float* out, const lgr_params*, const float*) { return lgr_fpfh_dev(ctx, kps, m, surf, n, radius, out); }
static int shot_stage(lgr_ctx* ctx, const float* kps, int m, const float* surf, int n, float radius, float* out, const lgr_params*, const float*) { return lgr_shot_dev(ctx, kps, m, surf, n, radius, nullptr, out, nullptr); }
static int rops_stage(lgr_ctx* ctx, const float* kps, int m, const float* surf, int n, float radius, float* out, const lgr_params* p, const float* vp) {
    // include/matching.h:243-246 (reestimate_frames, true by default: lgr_params has no field for it): the key-point copy's normals
    // are re-estimated on the level's surface, estimateNormalsPoints(normal_nr_points, kps, surface, viewpoint, true).  FPFH and SHOT
    // never read them (so their stages skip the step); the gravity frames do (z = the key point's normal).
    float* kn;
    LGR_TRY(lgr_ws_t(ctx, WS_ROPS_KPS, (size_t) m * 12, &kn));
    LGR_HIP(ctx, hipMemcpyAsync(kn, kps, (size_t) m * 48, hipMemcpyDeviceToDevice, ctx->stream));
    LGR_TRY(lgr_normals_knn_dev(ctx, kn, m, surf, n, p->normal_nr_points, vp, 1));
    // estimateFeatures<RoPS135> estimates its frames on every call, so per scale level too
    return lgr_rops_gravity_dev(ctx, kn, m, surf, n, radius, out);
}
static const Descriptor DESCRIPTORS[] = {
    /* LGR_DESCRIPTOR_FPFH */ {33, fpfh_stage, false, LGR_LRF_DEFAULT},
    // the reference's other SHOT frames (gravity, gt) replace getLocalRF and are not built
    /* LGR_DESCRIPTOR_SHOT */ {352, shot_stage, true, LGR_LRF_DEFAULT},
    // default: estimateFeatures<RoPS135> triangulates the cloud (GreedyProjectionTriangulation) and takes RoPS's own frames;
    // gt: the reference reads parameters.ground_truth, for which lgr_feature_params has no channel
    /* LGR_DESCRIPTOR_ROPS */ {135, rops_stage, true, LGR_LRF_GRAVITY},
};
static_assert(LGR_DESCRIPTOR_FPFH == 0 && LGR_DESCRIPTOR_SHOT == 1 && LGR_DESCRIPTOR_ROPS == 2, "DESCRIPTORS is indexed by descriptor_id");

extern "C" void lgr_default_feature_params(lgr_feature_params* f) {
    if (!f) return;
    memset(f, 0, sizeof(*f));
    f->descriptor_id = LGR_DESCRIPTOR_FPFH;
    f->lrf_id = LGR_LRF_DEFAULT;
}

// the descriptor a feature-parameter struct selects, checked against the rest of the configuration (NULL: FPFH)
static int feature_descriptor(lgr_ctx* ctx, const lgr_params* p, const lgr_feature_params* f, const Descriptor** out) {
    *out = &DESCRIPTORS[LGR_DESCRIPTOR_FPFH];
    if (!f) return LGR_OK;
    LGR_CHECK(ctx, f->descriptor_id >= 0 && f->descriptor_id < (int) (sizeof DESCRIPTORS / sizeof *DESCRIPTORS), LGR_ERR_UNSUPPORTED);
    const Descriptor& d = DESCRIPTORS[f->descriptor_id];
    if (d.dense) {
        LGR_CHECK(ctx, f->lrf_id == LGR_LRF_DEFAULT || f->lrf_id == LGR_LRF_GRAVITY || f->lrf_id == LGR_LRF_GT, LGR_ERR_INVALID_ARG);
        LGR_CHECK(ctx, f->lrf_id == d.lrf, LGR_ERR_UNSUPPORTED);
        LGR_CHECK(ctx, p->use_bfmatcher && !p->has_guess, LGR_ERR_UNSUPPORTED);     // matchFLANN / matchLocal are built for FPFH only
        LGR_CHECK(ctx, ctx->opt.arithmetic != LGR_ARITH_PCL, LGR_ERR_UNSUPPORTED);  // the arithmetic modes are FPFH weightings
    }
    *out = &d;
    return LGR_OK;
}

// ---- One correspondence search (lgr_correspondences_ex_dev, at the end of this section, is the list of its stages): what the stages
// share.  Streams: the filter tables run on aux2 (start_tables), posted before the feature stages; the source cloud's features run on
// the caller's context with lgr_match_prepare right behind them, the target cloud's on aux (lgr_run_pair); finish joins aux2.
struct CorrCall {
    lgr_ctx* ctx;
    const lgr_params* p;
    const Descriptor* d = nullptr;
    const float *clouds[2], *kclouds[2];     // the clouds; the key-point clouds (the clouds themselves, or the ISS detections
    int sizes[2], ksizes[2];                 // with their index lists)
    int32_t* kidx[2] = {nullptr, nullptr};
    lgr_cloud* own[2] = {nullptr, nullptr};  // lgr_cloud_prepare*: the object that side's results go into (NULL: workspace)
    MsSide mss[2];                           // multi-scale: initialize() of both clouds
    lgr_corr* d_out;
    int* n_out;
    bool empty = false;                      // a cloud without two points: nothing to match
    float *feat[2], *surf[2], *dij, *dji;    // workspace: rows and down-sampled surfaces per cloud, the matches of both directions
    int32_t *ij, *ji;
    FilterTables ftab;
    int ratio_k = 0;                         // LGR_MATCH_RATIO: the list length of the ratio test (check)
    float ms[3] = {0, 0, 0};
    // lgr_aux_job keeps a REFERENCE to its callable, so `tables` has to outlive the posted job: it is declared in front of the guard
    // that waits for the job, members are destroyed in reverse order, and so every exit of the entry point waits first.  The
    // prepare-cancel guard comes last: it runs first, as it did when all three were locals of one function.
    struct Tables {
        CorrCall* c;
        int operator()(lgr_ctx* cx) const {
            LGR_TRY(filter_cloud_tables(cx, c->kclouds[0], c->ksizes[0], c->p->cluster_k, c->ftab.thr_s, c->ftab.knn_s));
            return filter_cloud_tables(cx, c->kclouds[1], c->ksizes[1], c->p->cluster_k, c->ftab.thr_t, c->ftab.knn_t);
        }
    } tables{this};
    lgr_helper_guard tables_guard;   // every exit path waits for the helper (which always drains its stream)
    struct PrepGuard { lgr_ctx* c; ~PrepGuard() { lgr_match_prepare_cancel(c); } } prep_guard;

    CorrCall(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params* p, lgr_corr* d_out, int* n_out)
        : ctx(ctx), p(p), clouds{d_src, d_tgt}, kclouds{d_src, d_tgt}, sizes{ns, nt}, ksizes{ns, nt}, d_out(d_out), n_out(n_out), prep_guard{ctx} {}
    CorrCall(const CorrCall&) = delete;
    const float* vp(int side) const { return side == 0 ? (p->has_vp_src ? p->vp_src : nullptr) : (p->has_vp_tgt ? p->vp_tgt : nullptr); }
    float iss_radius(int side) const { return side == 0 ? p->iss_radius_src : p->iss_radius_tgt; }
    bool ratio() const { return p->matching_id == LGR_MATCH_RATIO; }
    bool both_dirs() const { return p->matching_id != LGR_MATCH_ONE_SIDED && !ratio(); }
    // a per-cloud result whose size a stage finds out itself: the side's object, or the workspace slot of the existing entry points
    template <class T>
    int result(int side, int slot, size_t count, T** out) const { return own[side] ? lgr_cloud_alloc_t(ctx, own[side], count, out) : lgr_ws_t(ctx, slot, count, out); }
};

// One level of one cloud (include/matching.h:234-248; the single-scale search has one level): down-sample `in` into `surf`, normals,
// descriptors of m key points -- kps[d_list[0..m)] gathered into `sub`, or kps[0..m) when d_list is NULL -- into `out`.  The three
// stage times are added to ms; *nd is the down-sampled size.
static int level_features(lgr_ctx* cx, const CorrCall& c, int side, const float* in, int n_in, float voxel, float radius, float* surf,
                          const float* kps, int m, const int32_t* d_list, float* sub, float* out, float* ms, int* nd) {
    const lgr_params* p = c.p;
    tick(cx, 0);
    LGR_TRY(lgr_downsample_dev(cx, in, n_in, voxel, surf, nd));
    tick(cx, 1);
    LGR_TRY(lgr_normals_knn_dev(cx, surf, *nd, nullptr, 0, p->normal_nr_points, c.vp(side), p->normals_available));
    tick(cx, 2);
    if (m) {
        if (d_list) { gather_rows12(cx, kps, d_list, m, sub); kps = sub; }
        LGR_TRY(c.d->stage(cx, kps, m, surf, *nd, radius, out, p, c.vp(side)));
    }
    tick(cx, 3);
    LGR_HIP(cx, hipEventSynchronize(cx->ev[3]));
    float t;
    for (int s = 0; s < 3; ++s) { (void) hipEventElapsedTime(&t, cx->ev[s], cx->ev[s + 1]); ms[s] += t; }
    return LGR_OK;
}

// ---- multi-scale matching (feature_radius unset): include/matching.h:176-262 (initialize) and :264-352
// (match_multiscale).  The heavy stages (5-NN, down-sampling chain, normals, descriptors, brute-force matching per level, the merge
// of the levels' matches and the proximity vote) run on the device; the per-key-point level assignment (log2f/sqrtf of the
// reference's host arithmetic, level pruning) runs on the host in initialize.
static int ms_initialize(CorrCall& c, int side, MsSide& st) {
    lgr_ctx* ctx = c.ctx;
    const lgr_params* p = c.p;
    const int D = c.d->len, n = c.sizes[side], n_kps = c.ksizes[side];
    const float *d_pcd = c.clouds[side], *d_kps = c.kclouds[side];
    const int k = 5;
    LGR_CHECK(ctx, n >= k, LGR_ERR_INVALID_ARG);
    // :180-188 density of every key point = distance to its 4th neighbour in the full cloud
    int32_t* d_nn;
    float* d_d2;
    LGR_TRY(lgr_ws_t(ctx, WS_MS_KNN_I, (size_t) n_kps * k, &d_nn));
    LGR_TRY(lgr_ws_t(ctx, WS_MS_KNN_D, (size_t) n_kps * k, &d_d2));
    LGR_TRY(lgr_knn_dev(ctx, d_kps, n_kps, d_pcd, n, k, d_nn, d_d2));
    std::vector<float> d2((size_t) n_kps * k);
    LGR_HIP(ctx, hipMemcpyAsync(d2.data(), d_d2, d2.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> level(n_kps);
    for (int i = 0; i < n_kps; ++i) {
        float density = sqrtf(d2[(size_t) i * k + (k - 1)]);
        float feature_radius = sqrtf((float) p->feature_nr_points * density * density / M_PI);
        level[i] = (int) std::floor(std::log2(feature_radius) / std::log2(p->scale_factor));
        st.min_l2 = std::min(level[i], st.min_l2);
        st.max_l2 = std::max(level[i], st.max_l2);
    }
    // :189-208 levels with too few points are dropped, key points clamped into the remaining range
    LGR_CHECK(ctx, (long long) st.max_l2 - st.min_l2 < 64, LGR_ERR_INVALID_ARG);   // non-finite densities (duplicate-only clouds)
    std::vector<int> count(st.max_l2 - st.min_l2 + 1, 0);
    for (int v : level) count[v - st.min_l2]++;
    const int max_nr = *std::max_element(count.begin(), count.end());
    size_t front = 0, back = count.size();
    while (10 * count[front] < max_nr) { ++front; st.min_l2++; }
    while (1000 * count[back - 1] < max_nr) { --back; st.max_l2--; }
    for (int& v : level) v = std::min(std::max(v, st.min_l2), st.max_l2);
    const int nr_scales = st.max_l2 - st.min_l2 + 1;
    std::vector<std::vector<int>> lists(nr_scales);   // per scale: key-point indices
    for (int i = 0; i < n_kps; ++i)
        for (int j = level[i]; j <= st.max_l2; ++j) lists[j - st.min_l2].push_back(i);
    st.levels.assign(nr_scales, lgr_cloud_lvl{});
    size_t rows = 0;
    for (int i = 0; i < nr_scales; ++i) {
        lgr_cloud_lvl& l = st.levels[i];
        l.log2_radius = st.min_l2 + i;
        l.radius = powf(p->scale_factor, (float) l.log2_radius);
        l.voxel = sqrtf(M_PI * l.radius * l.radius / (float) p->feature_nr_points);
        l.rows = (int) lists[i].size();
        l.off = rows;
        rows += lists[i].size();
    }
    LGR_TRY(c.result(side, side == 0 ? WS_MS_FEAT_S : WS_MS_FEAT_T, rows * D + 1, &st.feat));
    LGR_TRY(c.result(side, side == 0 ? WS_MS_LIST_S : WS_MS_LIST_T, rows + 1, &st.d_lists));
    for (int i = 0; i < nr_scales; ++i)
        if (!lists[i].empty())
            LGR_HIP(ctx, hipMemcpyAsync(st.d_lists + st.levels[i].off, lists[i].data(), lists[i].size() * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // :228-261 per scale: down-sample the previous level's cloud, normals, descriptors of the level's key points
    float *bufA, *bufB, *sub;
    LGR_TRY(lgr_ws_t(ctx, side == 0 ? WS_PIPE_SURF_S : WS_PIPE_SURF_T, (size_t) n * 12, &bufA));
    LGR_TRY(lgr_ws_t(ctx, WS_MS_SURF2, (size_t) n * 12, &bufB));
    LGR_TRY(lgr_ws_t(ctx, WS_MS_SUB, (size_t) std::max(n_kps, 1) * 12, &sub));
    const float* in = d_pcd;
    int n_in = n;
    for (int i = 0; i < nr_scales; ++i) {
        lgr_cloud_lvl& l = st.levels[i];
        float* out = (i & 1) ? bufB : bufA;
        LGR_TRY(level_features(ctx, c, side, in, n_in, l.voxel, l.radius, out, d_kps, l.rows, st.d_lists + l.off, sub, st.feat + l.off * D, c.ms, &l.surface));
        in = out; n_in = l.surface;
    }
    return LGR_OK;
}

// inverse of a column-major 4x4 by Gauss-Jordan with partial pivoting in double, rounded to float: the canonical stand-in for
// Eigen's Matrix4f::inverse() (include/matching.h:296), same as the oracle's orc_inverse4
void lgr_inverse4(const float* m16, float* out16) {
    double a[4][8];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { a[r][c] = m16[4 * c + r]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r) if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (piv != col) for (int c = 0; c < 8; ++c) std::swap(a[piv][c], a[col][c]);
        double d = a[col][col];
        for (int c = 0; c < 8; ++c) a[col][c] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            double f = a[r][col];
            for (int c = 0; c < 8; ++c) a[r][c] -= f * a[col][c];
        }
    }
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out16[4 * c + r] = (float) a[r][4 + c];
}

// the matcher dispatch of match_multiscale (include/matching.h:294-312): guess -> matchLocal in both directions (the inverse guess
// for train -> query, :296), else bf -> matchBF (one MFMA pass serves both directions), else matchFLANN.  The long descriptors
// run the exact dense matcher (checked on entry: brute force only).
static int match_dispatch(const CorrCall& c, const float* a_pts, const float* fa, int ma, const float* b_pts, const float* fb, int mb,
                          int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d) {
    lgr_ctx* ctx = c.ctx;
    const lgr_params* p = c.p;
    const bool need_ba = c.both_dirs();
    if (c.d->dense) return lgr_match_dense(ctx, c.d->len, fa, ma, fb, mb, p->bf_block_size, ab_i, ab_d, need_ba ? ba_i : nullptr, need_ba ? ba_d : nullptr);
    if (p->has_guess) {
        LGR_TRY(lgr_match_local_dev(ctx, a_pts, ma, b_pts, mb, fa, fb, p->guess, p->match_search_radius, ab_i, ab_d));
        if (need_ba) {
            float inv[16];
            lgr_inverse4(p->guess, inv);
            LGR_TRY(lgr_match_local_dev(ctx, b_pts, mb, a_pts, ma, fb, fa, inv, p->match_search_radius, ba_i, ba_d));
        }
    } else if (p->use_bfmatcher) {
        if (need_ba) LGR_TRY(lgr_match_bf2_dev(ctx, fa, ma, fb, mb, p->bf_block_size, ab_i, ab_d, ba_i, ba_d));
        else LGR_TRY(lgr_match_bf_dev(ctx, fa, ma, fb, mb, p->bf_block_size, ab_i, ab_d));
    } else {
        LGR_TRY(lgr_match_flann_dev(ctx, fa, ma, fb, mb, ab_i, ab_d));
        if (need_ba) LGR_TRY(lgr_match_flann_dev(ctx, fb, mb, fa, ma, ba_i, ba_d));
    }
    return LGR_OK;
}

// randomness = k > 1, single scale: the k nearest rows of both directions, then the vote per direction -- ij on the target key
// points with their radius, ji on the source key points (include/matching.h:327-352 with one level)
static int match_knn_vote(const CorrCall& c) {
    lgr_ctx* ctx = c.ctx;
    const lgr_params* p = c.p;
    const int k = p->randomness, ns = c.ksizes[0], nt = c.ksizes[1];
    const bool need_ji = c.both_dirs();
    int32_t *cij, *cji = nullptr;
    LGR_TRY(lgr_ws_t(ctx, WS_KNN_CAND_IJ, (size_t) 2 * ns * k, &cij));
    if (need_ji) LGR_TRY(lgr_ws_t(ctx, WS_KNN_CAND_JI, (size_t) 2 * nt * k, &cji));
    float *dij = (float*) (cij + (size_t) ns * k), *dji = need_ji ? (float*) (cji + (size_t) nt * k) : nullptr;
    LGR_TRY(lgr_match_knn_core(ctx, c.d->len, c.feat[0], ns, c.feat[1], nt, p->bf_block_size, k, cij, dij, cji, dji));
    LGR_TRY(lgr_vote_matches_core(ctx, cij, dij, ns, k, c.kclouds[1], nt, p->iss_radius_tgt, c.ij, c.dij));
    if (need_ji) LGR_TRY(lgr_vote_matches_core(ctx, cji, dji, nt, k, c.kclouds[0], ns, p->iss_radius_src, c.ji, c.dji));
    return LGR_OK;
}

// matching ratio: a level's candidate per source key point, from the k-nearest sweep of the one direction
static int match_ratio(const CorrCall& c, const float* fa, int ma, const float* fb, int mb, int32_t* ab_i, float* ab_d) {
    return lgr_match_ratio_core(c.ctx, c.d->len, fa, ma, fb, mb, c.p->bf_block_size, c.ratio_k, LGR_MATCHING_RATIO_THRESHOLD, ab_i, ab_d);
}

// A level's matches into the per-key-point candidate tables (include/matching.h:300-315): one thread per (row, slot) of the level's
// result arrays, both directions in one launch.  Row i of direction a -> b is key point la[i]; its slot e lands at column
// col0 + e of that key point's table row, so the levels' order is the slot order; a match lb[.] is a key-point index too.  Unmatched
// slots (-1) keep the table's -1 fill.
__global__ void ms_merge_kernel(int ma, int mb, int kr, int width, int col0, const int32_t* __restrict__ la, const int32_t* __restrict__ lb,
                                const int32_t* __restrict__ ab_i, const float* __restrict__ ab_d, const int32_t* __restrict__ ba_i, const float* __restrict__ ba_d,
                                int32_t* __restrict__ cij, float* __restrict__ dij, int32_t* __restrict__ cji, float* __restrict__ dji) {
    const long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    const long long na = (long long) ma * kr, nb = cji ? (long long) mb * kr : 0;
    if (e < na) {
        const int v = ab_i[e];
        if (v >= 0 && v < mb) {
            const size_t at = (size_t) la[e / kr] * width + col0 + (int) (e % kr);
            cij[at] = lb[v]; dij[at] = ab_d[e];
        }
    } else if (e < na + nb) {
        const long long f = e - na;
        const int v = ba_i[f];
        if (v >= 0 && v < ma) {
            const size_t at = (size_t) lb[f / kr] * width + col0 + (int) (f % kr);
            cji[at] = la[v]; dji[at] = ba_d[f];
        }
    }
}

// match_multiscale over two initialized clouds: per common level the matcher, the level's matches into the candidate tables, then the
// vote per direction -- ij on the target key points with their radius, ji on the source key points.  Nothing is read back.
static int ms_match(CorrCall& c) {
    lgr_ctx* ctx = c.ctx;
    const int D = c.d->len;
    const MsSide* st = c.mss;
    const bool need_ji = c.both_dirs();
    const int ns = c.ksizes[0], nt = c.ksizes[1], kr = c.p->randomness;
    const int lo = std::max(st[0].min_l2, st[1].min_l2), hi = std::min(st[0].max_l2, st[1].max_l2);
    if (lo > hi) {   // no level in common: no key point has a candidate
        LGR_HIP(ctx, hipMemsetAsync(c.ij, 0xff, (size_t) ns * 4, ctx->stream));
        LGR_HIP(ctx, hipMemsetAsync(c.dij, 0, (size_t) ns * 4, ctx->stream));
        if (need_ji) {
            LGR_HIP(ctx, hipMemsetAsync(c.ji, 0xff, (size_t) nt * 4, ctx->stream));
            LGR_HIP(ctx, hipMemsetAsync(c.dji, 0, (size_t) nt * 4, ctx->stream));
        }
        return LGR_OK;
    }
    const int width = (hi - lo + 1) * kr;
    int32_t *cij, *cji = nullptr;
    LGR_TRY(lgr_ws_t(ctx, WS_KNN_CAND_IJ, (size_t) 2 * ns * width, &cij));
    if (need_ji) LGR_TRY(lgr_ws_t(ctx, WS_KNN_CAND_JI, (size_t) 2 * nt * width, &cji));
    float *dij = (float*) (cij + (size_t) ns * width), *dji = need_ji ? (float*) (cji + (size_t) nt * width) : nullptr;
    LGR_HIP(ctx, hipMemsetAsync(cij, 0xff, (size_t) ns * width * 4, ctx->stream));
    if (need_ji) LGR_HIP(ctx, hipMemsetAsync(cji, 0xff, (size_t) nt * width * 4, ctx->stream));
    // the level buffers at the size of the largest level (a key point takes part in every level from its own up): growing one would
    // wait for the stream
    int32_t* r;
    float* sub = nullptr;
    const lgr_cloud_lvl &top_a = st[0].levels[hi - st[0].min_l2], &top_b = st[1].levels[hi - st[1].min_l2];
    LGR_TRY(lgr_ws_t(ctx, WS_MS_RES, (size_t) 2 * (top_a.rows + top_b.rows) * kr + 4, &r));
    if (c.p->has_guess) LGR_TRY(lgr_ws_t(ctx, WS_MS_SUB, (size_t) (top_a.rows + top_b.rows) * 12 + 4, &sub));
    for (int level = lo; level <= hi; ++level) {
        const lgr_cloud_lvl &a = st[0].levels[level - st[0].min_l2], &b = st[1].levels[level - st[1].min_l2];
        const int ma = a.rows, mb = b.rows;
        if (ma == 0 || mb == 0) continue;
        int32_t *ab_i = r, *ba_i = r + (size_t) ma * kr;
        float *ab_d = (float*) (r + (size_t) (ma + mb) * kr), *ba_d = ab_d + (size_t) ma * kr;
        const float* fa = st[0].feat + a.off * D;
        const float* fb = st[1].feat + b.off * D;
        const int32_t *la = st[0].d_lists + a.off, *lb = st[1].d_lists + b.off;
        const float *pa = nullptr, *pb = nullptr;
        if (c.p->has_guess) {   // matchLocal works on the level's key-point sub-clouds (kps_multiscale, include/matching.h:243)
            gather_rows12(ctx, c.kclouds[0], la, ma, sub);
            gather_rows12(ctx, c.kclouds[1], lb, mb, sub + (size_t) ma * 12);
            pa = sub; pb = sub + (size_t) ma * 12;
        }
        // randomness > 1: the level's kr matches per key point, in list order (checked on entry: brute force, no guess)
        if (c.ratio()) LGR_TRY(match_ratio(c, fa, ma, fb, mb, ab_i, ab_d));   // (checked on entry: kr = 1, brute force, no guess)
        else if (kr > 1) LGR_TRY(lgr_match_knn_core(ctx, D, fa, ma, fb, mb, c.p->bf_block_size, kr, ab_i, ab_d, need_ji ? ba_i : nullptr, need_ji ? ba_d : nullptr));
        else LGR_TRY(match_dispatch(c, pa, fa, ma, pb, fb, mb, ab_i, ab_d, ba_i, ba_d));
        const long long items = (long long) (ma + (need_ji ? mb : 0)) * kr;
        ms_merge_kernel<<<cdiv(items, 256), 256, 0, ctx->stream>>>(ma, mb, kr, width, (level - lo) * kr, la, lb, ab_i, ab_d, ba_i, ba_d, cij, dij, cji, dji);
    }
    LGR_HIP(ctx, hipGetLastError());
    LGR_TRY(lgr_vote_matches_launch(ctx, cij, dij, ns, width, c.kclouds[1], nt, c.p->iss_radius_tgt, c.ij, c.dij));
    if (need_ji) LGR_TRY(lgr_vote_matches_launch(ctx, cji, dji, nt, width, c.kclouds[0], ns, c.p->iss_radius_src, c.ji, c.dji));
    return LGR_OK;
}

static int ms_match_tables(CorrCall& c) {
    for (int s = 0; s < 2; ++s) LGR_TRY(ms_initialize(c, s, c.mss[s]));
    tick(c.ctx, 4);
    return ms_match(c);
}

// ---- the stages of lgr_correspondences_ex_dev, in the order they run
static int check(CorrCall& c, const lgr_feature_params* fp) {
    lgr_ctx* ctx = c.ctx;
    const lgr_params* p = c.p;
    LGR_CHECK(ctx, (c.clouds[0] || c.sizes[0] == 0) && (c.clouds[1] || c.sizes[1] == 0) && p && c.n_out && c.sizes[0] >= 0 && c.sizes[1] >= 0, LGR_ERR_INVALID_ARG);
    LGR_TRY(feature_descriptor(ctx, p, fp, &c.d));
    if (c.sizes[0] < 2 || c.sizes[1] < 2) { *c.n_out = 0; c.empty = true; return LGR_OK; }   // the reference ends with an empty correspondence list
    LGR_CHECK(ctx, c.d_out != nullptr, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, p->randomness >= 1 && p->randomness <= LGR_RANDOMNESS_MAX, LGR_ERR_UNSUPPORTED);
    if (c.ratio()) {   // the ratio test reads one k-nearest list per key point and level: the brute-force matcher, one direction
        LGR_CHECK(ctx, p->randomness == 1 && p->use_bfmatcher && !p->has_guess, LGR_ERR_UNSUPPORTED);
        c.ratio_k = fp && fp->ratio_k ? fp->ratio_k : 2;   // MATCHING_RATIO_K include/common.h:51
        LGR_CHECK(ctx, c.ratio_k >= 2 && c.ratio_k <= LGR_RANDOMNESS_MAX, LGR_ERR_UNSUPPORTED);
    }
    if (p->randomness > 1) {   // the k-nearest matcher is the brute-force one (include/matching.h:612-625); the vote needs the voted side's radius
        LGR_CHECK(ctx, p->use_bfmatcher && !p->has_guess, LGR_ERR_UNSUPPORTED);
        LGR_CHECK(ctx, std::isfinite(p->iss_radius_tgt) && p->iss_radius_tgt > 0.f, LGR_ERR_INVALID_ARG);
        LGR_CHECK(ctx, !c.both_dirs() || (std::isfinite(p->iss_radius_src) && p->iss_radius_src > 0.f), LGR_ERR_INVALID_ARG);
    }
    LGR_CHECK(ctx, p->feature_nr_points > 0 && p->normal_nr_points >= 1 && p->normal_nr_points <= 64 && p->bf_block_size > 0 && p->scale_factor > 1.f,
              LGR_ERR_INVALID_ARG);
    // checked before any stage runs (this entry point builds the filter tables itself, so lgr_filter_dev's checks do not cover it):
    // the cluster filter keeps at most 64 spatial neighbours per point (filter_flags<64>)
    LGR_CHECK(ctx, p->matching_id == LGR_MATCH_LR || p->matching_id == LGR_MATCH_ONE_SIDED || p->matching_id == LGR_MATCH_CLUSTER || c.ratio(),
              LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, p->matching_id != LGR_MATCH_CLUSTER || (p->cluster_k >= 1 && p->cluster_k <= 64), LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    *c.n_out = 0;
    LGR_CHECK(ctx, p->keypoint_id == LGR_KEYPOINT_ANY || p->keypoint_id == LGR_KEYPOINT_ISS, LGR_ERR_UNSUPPORTED);
    return LGR_OK;
}

// key points (src/correspondence_search.cpp:8-11): every point, or the ISS detections.  kps = pcd[kps_indices]
// (include/matching.h:167); every later stage works on the key-point clouds and the indices are mapped back at the
// end (finalize, include/matching.h:150-160).
static int keypoints(CorrCall& c, int s) {
    lgr_ctx* ctx = c.ctx;
    if (c.p->keypoint_id != LGR_KEYPOINT_ISS) return LGR_OK;
    float* kp;
    LGR_TRY(lgr_ws_t(ctx, s == 0 ? WS_PIPE_KIDX_S : WS_PIPE_KIDX_T, (size_t) c.sizes[s] + 1, &c.kidx[s]));
    int m = 0;
    LGR_TRY(lgr_iss_keypoints_dev(ctx, c.clouds[s], c.sizes[s], c.iss_radius(s), 0.975f, 0.975f, 4, c.kidx[s], &m));
    if (c.own[s]) {   // the detector writes into a list as long as the cloud: the object keeps the m indices it found
        int32_t* kept;
        LGR_TRY(lgr_cloud_alloc_t(ctx, c.own[s], (size_t) std::max(m, 1), &kept));
        LGR_HIP(ctx, hipMemcpyAsync(kept, c.kidx[s], (size_t) m * 4, hipMemcpyDeviceToDevice, ctx->stream));
        c.kidx[s] = kept;
    }
    LGR_TRY(c.result(s, s == 0 ? WS_PIPE_KPS_S : WS_PIPE_KPS_T, (size_t) std::max(m, 1) * 12, &kp));
    if (m) gather_rows12(ctx, c.clouds[s], c.kidx[s], m, kp);
    c.kclouds[s] = kp; c.ksizes[s] = m;
    return LGR_OK;
}

// the matches of both directions (the pair's own buffers)
static int alloc_matches(CorrCall& c) {
    lgr_ctx* ctx = c.ctx;
    const int ns = c.ksizes[0], nt = c.ksizes[1];
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_IJ, (size_t) ns, &c.ij));
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_JI, (size_t) nt, &c.ji));
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_DIJ, (size_t) ns, &c.dij));
    return lgr_ws_t(ctx, WS_PIPE_DJI, (size_t) nt, &c.dji);
}

static int alloc(CorrCall& c) {
    lgr_ctx* ctx = c.ctx;
    const int ns = c.ksizes[0], nt = c.ksizes[1];
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_FEAT_S, (size_t) ns * c.d->len, &c.feat[0]));
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_FEAT_T, (size_t) nt * c.d->len, &c.feat[1]));
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_SURF_S, (size_t) c.sizes[0] * 12, &c.surf[0]));
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_SURF_T, (size_t) c.sizes[1] * 12, &c.surf[1]));
    LGR_TRY(alloc_matches(c));
    LGR_TRY(filter_tables_alloc(ctx, c.p->matching_id, ns, nt, c.p->cluster_k, &c.ftab));
    return lgr_ctx_aux2(ctx);
}

// The filter's per-cloud tables do not depend on the matches: a third context computes them from a host thread of its own
// while the feature stages and the matcher run (their sorts and k-NN kernels fill the matcher's low-occupancy phases).
static int start_tables(CorrCall& c) {
    lgr_ctx* ctx = c.ctx;
    c.tables_guard.aux = ctx->aux2;
    if (ctx->opt.helper_contexts) {
        LGR_HIP(ctx, hipEventRecord(ctx->aux2_ev, ctx->stream));
        LGR_HIP(ctx, hipStreamWaitEvent(ctx->aux2->stream, ctx->aux2_ev, 0));
        LGR_TRY(lgr_helper_post(ctx, ctx->aux2, lgr_aux_job(ctx->aux2, c.tables)));
        c.tables_guard.armed = true;
    } else {
        const int rc = c.tables(ctx->aux2);            // same stream, this thread
        if (rc != LGR_OK) { ctx->err = ctx->aux2->err; return rc; }
    }
    return LGR_OK;
}

// include/matching.h:172,230-231: radius quantised to a power of scale_factor; voxel from feature_nr_points
static lgr_cloud_lvl single_level(const lgr_params* p) {
    lgr_cloud_lvl l{};
    l.log2_radius = (int) std::floor(std::log2(p->feature_radius) / std::log2(p->scale_factor));
    l.radius = powf(p->scale_factor, (float) l.log2_radius);
    l.voxel = sqrtf(M_PI * l.radius * l.radius / (float) p->feature_nr_points);
    return l;
}

// the matcher of the single-scale search on both clouds' rows
static int match_single(CorrCall& c) {
    if (c.ratio()) return match_ratio(c, c.feat[0], c.ksizes[0], c.feat[1], c.ksizes[1], c.ij, c.dij);   // one level: the vote is the identity
    if (c.p->randomness > 1) return match_knn_vote(c);
    return match_dispatch(c, c.kclouds[0], c.feat[0], c.ksizes[0], c.kclouds[1], c.feat[1], c.ksizes[1], c.ij, c.dij, c.ji, c.dji);
}

// The two clouds' feature stages are independent until the matcher: the source cloud runs on this context, the target cloud
// on a second context (own stream and workspace) driven by a second host thread, so that the ~20 host read-backs per cloud
// (voxel counts, grid extents) and the short sort / scan launches of one cloud hide behind the other cloud's kernels.
// Results cannot depend on it (disjoint outputs; every kernel is deterministic).
static int features_and_match_single(CorrCall& c) {
    lgr_ctx* ctx = c.ctx;
    const lgr_params* p = c.p;
    const lgr_cloud_lvl l = single_level(p);
    auto cloud_features = [&](lgr_ctx* cx, int s, float* ms) -> int {
        LGR_HIP(cx, hipSetDevice(cx->device));
        int nd;
        return level_features(cx, c, s, c.clouds[s], c.sizes[s], l.voxel, l.radius, c.surf[s], c.kclouds[s], c.ksizes[s], nullptr, nullptr, c.feat[s], ms, &nd);
    };
    float ms_t[3] = {0, 0, 0};
    const auto t_feat0 = std::chrono::steady_clock::now();
    // The source cloud is done first (this thread): the matcher's query-side half (clustering, assignment, sort) runs right behind
    // its features, under the target cloud's feature kernels on the second context.
    const bool prepare_query = p->use_bfmatcher && !p->has_guess && !c.d->dense && p->randomness == 1 && !c.ratio();   // match_dispatch: the FPFH brute-force matcher will be called
    LGR_TRY(lgr_run_pair(ctx,
        [&](lgr_ctx* cx) {
            LGR_TRY(cloud_features(cx, 0, c.ms));
            return prepare_query ? lgr_match_prepare(cx, c.feat[0], c.ksizes[0], c.ksizes[1], c.both_dirs()) : (int) LGR_OK;
        },
        [&](lgr_ctx* cx) { return cloud_features(cx, 1, ms_t); }));
    // the two clouds overlap in wall time: report the wall time of the feature stages, split in proportion to the stage times
    // the two streams measured (each of which includes the other stream's interleaved kernels)
    const float wall = 1e3f * std::chrono::duration<float>(std::chrono::steady_clock::now() - t_feat0).count();
    float sum = 0.f;
    for (int s = 0; s < 3; ++s) { c.ms[s] += ms_t[s]; sum += c.ms[s]; }
    if (sum > 0.f) for (int s = 0; s < 3; ++s) c.ms[s] *= wall / sum;
    tick(ctx, 4);
    return match_single(c);
}

// wait for the tables, filter, map key-point indices back (finalize), stage times
static int finish(CorrCall& c) {
    lgr_ctx* ctx = c.ctx;
    const lgr_params* p = c.p;
    tick(ctx, 5);
    if (c.tables_guard.armed) {
        const int rc_tab = c.tables_guard.wait();
        (void) hipSetDevice(ctx->device);
        if (rc_tab != LGR_OK) { ctx->err = ctx->aux2->err; return rc_tab; }
    }
    LGR_TRY(filter_core(ctx, c.ratio() ? (int) LGR_MATCH_ONE_SIDED : p->matching_id, c.ksizes[0], c.ij, c.dij, c.ji, c.dji, p->distance_thr, p->cluster_k, c.ftab, c.d_out, c.n_out));
    if (c.kidx[0] && *c.n_out) finalize_kernel<<<cdiv(*c.n_out, 256), 256, 0, ctx->stream>>>(c.d_out, *c.n_out, c.kidx[0], c.kidx[1]);
    tick(ctx, 6);
    LGR_HIP(ctx, hipEventSynchronize(ctx->ev[6]));
    float t;
    ctx->stage_ms[0] = c.ms[0]; ctx->stage_ms[1] = c.ms[1]; ctx->stage_ms[2] = c.ms[2];
    (void) hipEventElapsedTime(&t, ctx->ev[4], ctx->ev[5]); ctx->stage_ms[3] = t;
    (void) hipEventElapsedTime(&t, ctx->ev[5], ctx->ev[6]); ctx->stage_ms[4] = t;
    return LGR_OK;
}

extern "C" int lgr_correspondences_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params* p,
                                       lgr_corr* d_out, int* n_out) {
    return lgr_correspondences_ex_dev(ctx, d_src, ns, d_tgt, nt, p, nullptr, d_out, n_out);
}

extern "C" int lgr_correspondences_ex_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params* p,
                                          const lgr_feature_params* fp, lgr_corr* d_out, int* n_out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    CorrCall c(ctx, d_src, ns, d_tgt, nt, p, d_out, n_out);   // its guards act on every return below
    LGR_TRY(check(c, fp));
    if (c.empty) return LGR_OK;
    for (int s = 0; s < 2; ++s) LGR_TRY(keypoints(c, s));
    if (c.ksizes[0] == 0 || c.ksizes[1] == 0) return LGR_OK;   // ISS found nothing on a side: no job has been posted yet
    LGR_TRY(alloc(c));
    LGR_TRY(start_tables(c));                                  // aux2, under everything up to finish
    // (feature_radius unset, i.e. <= 0 here: the multi-scale path, include/matching.h:176-208)
    LGR_TRY(p->feature_radius > 0.f ? features_and_match_single(c) : ms_match_tables(c));
    return finish(c);
}

extern "C" int lgr_correspondences(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_params* p, lgr_corr* out, int* n_out) {
    return lgr_correspondences_ex(ctx, src, ns, tgt, nt, p, nullptr, out, n_out);
}

// (the host entry points stage their arrays through lgr_host_call, lgr_host.h, on ctx->stream)
extern "C" int lgr_correspondences_ex(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_params* p, const lgr_feature_params* fp,
                                      lgr_corr* out, int* n_out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (src || ns == 0) && (tgt || nt == 0) && p && n_out && ns >= 0 && nt >= 0, LGR_ERR_INVALID_ARG);
    if (ns < 2 || nt < 2) { *n_out = 0; return LGR_OK; }
    LGR_CHECK(ctx, out != nullptr, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    float *ds, *dt;
    lgr_corr* dc;
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_CORR, (size_t) ns + 1, &dc));   // the pipeline's own slot, as in lgr_measure_dev: not a staged array
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(lgr_correspondences_ex_dev(ctx, ds, ns, dt, nt, p, fp, dc, n_out));
    LGR_TRY(hc.fetch(out, dc, (size_t) *n_out));
    return hc.finish();
}


// ---- prepared clouds (lgr_cloud.h): the per-cloud stages above, run once per cloud into an object; a pair call starts at the matcher
static uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int lgr_cloud_key_of(lgr_ctx* ctx, const lgr_params* p, const lgr_feature_params* fp, int side, lgr_cloud_key* out) {
    lgr_cloud_key k;
    memset(&k, 0, sizeof k);
    k.feature_nr_points = p->feature_nr_points; k.normal_nr_points = p->normal_nr_points; k.normals_available = p->normals_available;
    k.keypoint_id = p->keypoint_id;
    k.has_vp = side == 0 ? p->has_vp_src : p->has_vp_tgt;
    k.cluster_k = p->matching_id == LGR_MATCH_CLUSTER ? p->cluster_k : 0;   // the other filters read the densities only
    k.descriptor_id = fp ? fp->descriptor_id : (int) LGR_DESCRIPTOR_FPFH;
    k.lrf_id = fp ? fp->lrf_id : (int) LGR_LRF_DEFAULT;
    k.arithmetic = ctx->opt.arithmetic;
    k.feature_radius = p->feature_radius > 0.f ? float_bits(p->feature_radius) : 0u;   // unset, however it is written: multi-scale
    k.scale_factor = float_bits(p->scale_factor);
    k.iss_radius = float_bits(side == 0 ? p->iss_radius_src : p->iss_radius_tgt);
    if (k.has_vp) for (int a = 0; a < 3; ++a) k.vp[a] = float_bits((side == 0 ? p->vp_src : p->vp_tgt)[a]);
    *out = k;
    return LGR_OK;
}

int lgr_cloud_fill(lgr_ctx* ctx, lgr_cloud* cl, int side, const lgr_params* p, const lgr_feature_params* fp) {
    int n0 = 0;
    lgr_corr none;   // check only asks for an output pointer; nothing is written through it
    CorrCall c(ctx, cl->pts, cl->n, cl->pts, cl->n, p, &none, &n0);
    LGR_TRY(check(c, fp));
    LGR_TRY(lgr_cloud_key_of(ctx, p, fp, side, &cl->key));
    cl->row_len = c.d->len;
    cl->multiscale = !(p->feature_radius > 0.f);
    cl->kps = cl->pts; cl->m = cl->n;
    if (c.empty) { cl->empty = true; return LGR_OK; }
    c.own[side] = cl;
    LGR_TRY(keypoints(c, side));
    cl->kps = c.kclouds[side]; cl->m = c.ksizes[side]; cl->kidx = c.kidx[side];
    if (cl->m == 0) return LGR_OK;   // ISS found nothing: a pair with this cloud has no correspondences
    if (!cl->multiscale) {
        float* surf;
        cl->single = single_level(p);
        cl->single.rows = cl->m;
        LGR_TRY(lgr_cloud_alloc_t(ctx, cl, (size_t) cl->m * cl->row_len, &cl->feat));
        LGR_TRY(lgr_ws_t(ctx, side == 0 ? WS_PIPE_SURF_S : WS_PIPE_SURF_T, (size_t) cl->n * 12, &surf));
        LGR_TRY(level_features(ctx, c, side, cl->pts, cl->n, cl->single.voxel, cl->single.radius, surf, cl->kps, cl->m, nullptr, nullptr, cl->feat, c.ms, &cl->single.surface));
    } else {
        LGR_TRY(ms_initialize(c, side, cl->ms));
    }
    LGR_TRY(lgr_cloud_alloc_t(ctx, cl, (size_t) cl->m + 16, &cl->thr));
    if (cl->key.cluster_k) LGR_TRY(lgr_cloud_alloc_t(ctx, cl, (size_t) cl->m * cl->key.cluster_k, &cl->knn));
    LGR_TRY(filter_cloud_tables(ctx, cl->kps, cl->m, cl->key.cluster_k, cl->thr, cl->knn));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

extern "C" int lgr_correspondences_prepared_dev(lgr_ctx* ctx, const lgr_cloud* src, const lgr_cloud* tgt, const lgr_params* p, const lgr_feature_params* fp,
                                                lgr_corr* d_out, int* n_out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, src && tgt && p && n_out, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, src->device == ctx->device && tgt->device == ctx->device, LGR_ERR_INVALID_ARG);
    const lgr_cloud* cl[2] = {src, tgt};
    CorrCall c(ctx, src->pts, src->n, tgt->pts, tgt->n, p, d_out, n_out);
    LGR_TRY(check(c, fp));
    for (int s = 0; s < 2; ++s) {
        lgr_cloud_key k;
        LGR_TRY(lgr_cloud_key_of(ctx, p, fp, s, &k));
        LGR_CHECK(ctx, memcmp(&k, &cl[s]->key, sizeof k) == 0 /* the cloud was prepared for other parameters */, LGR_ERR_INVALID_ARG);
    }
    for (int s = 0; s < 3; ++s) ctx->stage_ms[s] = 0.f;
    if (c.empty) return LGR_OK;
    for (int s = 0; s < 2; ++s) {
        c.kclouds[s] = cl[s]->kps; c.ksizes[s] = cl[s]->m; c.kidx[s] = cl[s]->kidx;
        c.feat[s] = cl[s]->feat; c.mss[s] = cl[s]->ms;
    }
    if (c.ksizes[0] == 0 || c.ksizes[1] == 0) return LGR_OK;
    c.ftab.thr_s = src->thr; c.ftab.knn_s = src->knn;
    c.ftab.thr_t = tgt->thr; c.ftab.knn_t = tgt->knn;
    LGR_TRY(alloc_matches(c));
    tick(ctx, 4);
    LGR_TRY(src->multiscale ? ms_match(c) : match_single(c));
    return finish(c);
}

extern "C" int lgr_correspondences_prepared(lgr_ctx* ctx, const lgr_cloud* src, const lgr_cloud* tgt, const lgr_params* p, const lgr_feature_params* fp,
                                            lgr_corr* out, int* n_out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, src && tgt && p && n_out, LGR_ERR_INVALID_ARG);
    lgr_corr* dc = nullptr;
    if (src->n >= 2 && tgt->n >= 2) {
        LGR_CHECK(ctx, out != nullptr, LGR_ERR_INVALID_ARG);
        LGR_HIP(ctx, hipSetDevice(ctx->device));
        LGR_TRY(lgr_ws_t(ctx, WS_PIPE_CORR, (size_t) src->n + 1, &dc));
    }
    LGR_TRY(lgr_correspondences_prepared_dev(ctx, src, tgt, p, fp, dc, n_out));
    if (*n_out) LGR_HIP(ctx, hipMemcpyAsync(out, dc, (size_t) *n_out * 16, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}


extern "C" int lgr_align_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params* p, lgr_result* res) {
    return lgr_align_ex_dev(ctx, d_src, ns, d_tgt, nt, p, nullptr, res);
}

extern "C" int lgr_align_ex_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params* p, const lgr_feature_params* fp,
                                lgr_result* res) {
    return lgr_align_ex2_dev(ctx, d_src, ns, d_tgt, nt, p, fp, nullptr, res);
}

static int align_estimate(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params* p, const lgr_metric_params* mp,
                          const lgr_corr* dc, int c, std::chrono::steady_clock::time_point t0, lgr_result* res);
// what lgr_align* checks before the search, and its answer for a cloud without two points
static int align_check(lgr_ctx* ctx, const lgr_params* p, const lgr_feature_params* fp) {
    // alignTeaser throws in the reference (src/alignment.cpp:40)
    LGR_CHECK(ctx, p->alignment_id == LGR_ALIGN_RANSAC || p->alignment_id == LGR_ALIGN_GROR, LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, p->n_samples >= 3 && p->n_samples <= 8, LGR_ERR_UNSUPPORTED);   // (lgr_ransac.hip instantiates its kernels for 3..8)
    const Descriptor* descriptor;
    return feature_descriptor(ctx, p, fp, &descriptor);
}
static void align_identity(lgr_result* res) {
    // a cloud without two points gives no correspondences; the reference then leaves the identity, not converged
    // (selectCorrespondences refuses fewer than n_samples, src/sac_prerejective_omp.cpp:36-42)
    memset(res, 0, sizeof(*res));
    for (int i = 0; i < 16; ++i) res->transformation[i] = (i % 5 == 0) ? 1.f : 0.f;
}

extern "C" int lgr_align_prepared(lgr_ctx* ctx, const lgr_cloud* src, const lgr_cloud* tgt, const lgr_params* p, const lgr_feature_params* fp,
                                  const lgr_metric_params* mp, lgr_result* res) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, src && tgt && p && res, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, src->device == ctx->device && tgt->device == ctx->device, LGR_ERR_INVALID_ARG);
    LGR_TRY(align_check(ctx, p, fp));
    if (src->n < 2 || tgt->n < 2) { align_identity(res); return LGR_OK; }
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    auto t0 = std::chrono::steady_clock::now();
    lgr_corr* dc;
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_CORR, (size_t) src->n + 1, &dc));
    int c = 0;
    LGR_TRY(lgr_correspondences_prepared_dev(ctx, src, tgt, p, fp, dc, &c));
    return align_estimate(ctx, src->pts, src->n, tgt->pts, tgt->n, p, mp, dc, c, t0, res);
}

extern "C" int lgr_align_ex2_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params* p, const lgr_feature_params* fp,
                                 const lgr_metric_params* mp, lgr_result* res) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (d_src || ns == 0) && (d_tgt || nt == 0) && p && res && ns >= 0 && nt >= 0, LGR_ERR_INVALID_ARG);
    LGR_TRY(align_check(ctx, p, fp));
    if (ns < 2 || nt < 2) { align_identity(res); return LGR_OK; }
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    auto t0 = std::chrono::steady_clock::now();
    lgr_corr* dc;
    LGR_TRY(lgr_ws_t(ctx, WS_PIPE_CORR, (size_t) ns + 1, &dc));
    int c = 0;
    LGR_TRY(lgr_correspondences_ex_dev(ctx, d_src, ns, d_tgt, nt, p, fp, dc, &c));
    return align_estimate(ctx, d_src, ns, d_tgt, nt, p, mp, dc, c, t0, res);
}

// the transform estimation behind a finished search (src/alignment.cpp:72-109), for lgr_align_ex2_dev and lgr_align_prepared
static int align_estimate(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params* p, const lgr_metric_params* mp,
                          const lgr_corr* dc, int c, std::chrono::steady_clock::time_point t0, lgr_result* res) {
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double time_cs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    tick(ctx, 7);
    ctx->corr_trusted = true;                  // dc was produced by lgr_correspondences_dev: no range check (lgr_check_corr)
    int rc_te;
    if (p->alignment_id == LGR_ALIGN_GROR) {   // src/alignment.cpp:21-35: resolution = distance_thr, K_optimal = 800
        rc_te = lgr_gror_dev(ctx, d_src, ns, d_tgt, nt, dc, c, p->distance_thr, 800, res, nullptr);
    } else {
        rc_te = lgr_ransac_ex_dev(ctx, d_src, ns, d_tgt, nt, dc, c, p, mp, res, nullptr);
    }
    ctx->corr_trusted = false;
    LGR_TRY(rc_te);
    tick(ctx, 8);
    LGR_HIP(ctx, hipEventSynchronize(ctx->ev[8]));
    float t;
    (void) hipEventElapsedTime(&t, ctx->ev[7], ctx->ev[8]);
    ctx->stage_ms[5] = t;
    res->time_cs = time_cs;
    res->n_correspondences = c;
    for (int i = 0; i < 12; ++i) res->stage_ms[i] = ctx->stage_ms[i];
    return LGR_OK;
}

extern "C" int lgr_align(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_params* p, lgr_result* res) {
    return lgr_align_ex(ctx, src, ns, tgt, nt, p, nullptr, res);
}

extern "C" int lgr_align_ex(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_params* p, const lgr_feature_params* fp,
                            lgr_result* res) {
    return lgr_align_ex2(ctx, src, ns, tgt, nt, p, fp, nullptr, res);
}

extern "C" int lgr_align_ex2(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_params* p, const lgr_feature_params* fp,
                             const lgr_metric_params* mp, lgr_result* res) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (src || ns == 0) && (tgt || nt == 0) && p && res && ns >= 0 && nt >= 0, LGR_ERR_INVALID_ARG);
    if (ns < 2 || nt < 2) return lgr_align_ex2_dev(ctx, nullptr, 0, nullptr, 0, p, fp, mp, res);   // identity, not converged
    float *ds, *dt;
    lgr_metric_params mpd;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.weights(ns, &mp, &mpd));
    return lgr_align_ex2_dev(ctx, ds, ns, dt, nt, p, fp, mp, res);
}

// ---- the `measure` test type (measureTestResults, src/main.cpp:312-382) ----
// include/utils.h:68-74 calculateMean<float>: std::accumulate from the double 0.0, divided by (float) size, returned as float
extern "C" float lgr_measure_mean(const float* x, int n) {
    if (n <= 0 || !x) return std::numeric_limits<float>::quiet_NaN();
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum = sum + x[i];
    return (float) (sum / (float) n);
}

// include/utils.h:76-88 calculateStandardDeviation<float>: the float sum of the squared differences in order, the population form
extern "C" float lgr_measure_deviation(const float* x, int n, float mean) {
    if (n <= 0 || !x) return std::numeric_limits<float>::quiet_NaN();
    float deviation = 0.f;
    for (int i = 0; i < n; ++i) deviation += (x[i] - mean) * (x[i] - mean);
    return std::sqrt(deviation / (float) n);
}

// src/main.cpp:345-380 over the finished runs
static void measure_aggregate(const lgr_measure_run* runs, int n, lgr_measurement* out) {
    std::vector<float> r, t, o, time;
    for (int i = 0; i < n; ++i) {
        if (runs[i].eval.converged_and_overlap_ok) {
            r.push_back(runs[i].eval.r_err); t.push_back(runs[i].eval.t_err); o.push_back(runs[i].eval.overlap_rmse);
        }
        time.push_back((float) (runs[i].result.time_cs + runs[i].result.time_te));
    }
    memset(out, 0, sizeof *out);
    out->n_times = n; out->n_success = (int) r.size();
    out->success_rate = (float) out->n_success / (float) n;
    auto both = [](const std::vector<float>& v, float* mean, float* dev) {
        *mean = lgr_measure_mean(v.data(), (int) v.size());
        *dev = lgr_measure_deviation(v.data(), (int) v.size(), *mean);
    };
    both(r, &out->mae, &out->sae); both(t, &out->mte, &out->ste); both(o, &out->mrmse, &out->srmse); both(time, &out->mtime, &out->stime);
}

extern "C" int lgr_measure_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params* p, const lgr_feature_params* fp,
                               const lgr_metric_params* mp, const float Tgt16[16], const uint64_t* seeds, int n_times, lgr_measure_run* runs,
                               lgr_measurement* out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    // lgr_align_ex2_dev's own checks, in its order
    LGR_CHECK(ctx, (d_src || ns == 0) && (d_tgt || nt == 0) && p && ns >= 0 && nt >= 0, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, p->alignment_id == LGR_ALIGN_RANSAC || p->alignment_id == LGR_ALIGN_GROR, LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, p->n_samples >= 3 && p->n_samples <= 8, LGR_ERR_UNSUPPORTED);
    const Descriptor* descriptor;
    LGR_TRY(feature_descriptor(ctx, p, fp, &descriptor));
    LGR_CHECK(ctx, Tgt16 && runs && out && n_times >= 1 && n_times <= LGR_GT_BATCH_MAX, LGR_ERR_INVALID_ARG);
    const bool ransac = p->alignment_id == LGR_ALIGN_RANSAC;
    const int n = ransac ? n_times : 1;   // src/main.cpp:350
    const bool empty = ns < 2 || nt < 2;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    lgr_corr* dc = nullptr;
    if (!empty) {
        // ... and the checks of its two stages, before either runs: the search's (check) and the loop's, which a call without
        // correspondences makes and then returns from (lgr_ransac_ex_dev: identity, no launch)
        {
            int n0 = 0;
            lgr_corr none;   // check only asks for an output pointer; nothing is written through it
            CorrCall probe(ctx, d_src, ns, d_tgt, nt, p, &none, &n0);
            LGR_TRY(check(probe, fp));
        }
        lgr_result r0;
        if (ransac) LGR_TRY(lgr_ransac_ex_dev(ctx, d_src, ns, d_tgt, nt, nullptr, 0, p, mp, &r0, nullptr));
    }
    // the evaluation's own bound (include/lgr.h), after everything lgr_align_ex2_dev would have refused; still before any work
    LGR_CHECK(ctx, p->distance_thr > 0.f && p->distance_thr <= 1e18f, LGR_ERR_INVALID_ARG);
    if (!empty) LGR_TRY(lgr_ws_t(ctx, WS_PIPE_CORR, (size_t) ns + 1, &dc));
    for (int i = 0; i < n; ++i) {
        memset(&runs[i], 0, sizeof runs[i]);
        runs[i].seed = seeds ? seeds[i] : p->seed + (uint64_t) i;
        for (int k = 0; k < 16; ++k) runs[i].result.transformation[k] = (k % 5 == 0) ? 1.f : 0.f;   // a cloud without two points: identity, not converged
    }
    int c = 0;
    uint8_t* d_masks = nullptr;
    if (!empty) {
        auto t0 = std::chrono::steady_clock::now();
        LGR_TRY(lgr_correspondences_ex_dev(ctx, d_src, ns, d_tgt, nt, p, fp, dc, &c));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const double time_cs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        float search_ms[12];
        for (int k = 0; k < 12; ++k) search_ms[k] = ctx->stage_ms[k];
        LGR_TRY(lgr_ws_t(ctx, WS_MEASURE_MASKS, (size_t) n * c + 16, &d_masks));
        LGR_HIP(ctx, hipMemsetAsync(d_masks, 0, (size_t) n * c + 16, ctx->stream));   // (a run with c < n_samples writes no mask)
        // WeightedClosestPlaneMetricEstimator::setSourceCloud once for all runs: lgr_weights_prepare sums a caller's weights with the kernel
        // it sums its own map with, so handing the map over is bit-identical to letting each run compute it.  The constant map is not
        // handed over: its sum is a closed form there (lgr_seqsum.h) and the map costs one fill.
        lgr_metric_params mp_shared;
        const lgr_metric_params* mp_run = mp;
        if (ransac && p->metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE && mp && !mp->weights && mp->weight_id != LGR_WEIGHT_CONSTANT && c >= p->n_samples) {
            float* d_w;
            LGR_TRY(lgr_ws_t(ctx, WS_MEASURE_W, (size_t) ns + 64, &d_w));
            LGR_TRY(lgr_weights_map(ctx, d_src, ns, mp->weight_id, 30, d_w));   // NORMAL_NR_POINTS (lgr_weights.hip)
            mp_shared = *mp; mp_shared.weights = d_w; mp_run = &mp_shared;
        }
        lgr_params pr = *p;
        pr.fix_seed = 0;   // src/main.cpp:339
        for (int i = 0; i < n; ++i) {
            pr.seed = runs[i].seed;
            lgr_result* res = &runs[i].result;
            tick(ctx, 7);
            ctx->corr_trusted = true;   // dc was produced by the search above (lgr_check_corr)
            const int rc = ransac ? lgr_ransac_ex_dev(ctx, d_src, ns, d_tgt, nt, dc, c, &pr, mp_run, res, d_masks + (size_t) i * c)
                                  : lgr_gror_dev(ctx, d_src, ns, d_tgt, nt, dc, c, p->distance_thr, 800, res, d_masks + (size_t) i * c);
            ctx->corr_trusted = false;
            LGR_TRY(rc);
            tick(ctx, 8);
            LGR_HIP(ctx, hipEventSynchronize(ctx->ev[8]));
            float t;
            (void) hipEventElapsedTime(&t, ctx->ev[7], ctx->ev[8]);
            res->time_cs = time_cs;
            res->n_correspondences = c;
            for (int k = 0; k < 12; ++k) res->stage_ms[k] = search_ms[k];
            res->stage_ms[5] = t;
        }
    }
    float T16s[LGR_GT_BATCH_MAX * 16];
    int32_t conv[LGR_GT_BATCH_MAX];
    lgr_gt_eval evals[LGR_GT_BATCH_MAX];
    for (int i = 0; i < n; ++i) {
        memcpy(T16s + 16 * i, runs[i].result.transformation, 64);
        conv[i] = runs[i].result.converged;
    }
    LGR_TRY(lgr_evaluate_gt_batch_dev(ctx, d_src, ns, d_tgt, nt, dc, c, T16s, n, Tgt16, p->distance_thr, conv, c ? d_masks : nullptr, evals, nullptr));
    for (int i = 0; i < n; ++i) runs[i].eval = evals[i];
    measure_aggregate(runs, n, out);
    return LGR_OK;
}

extern "C" int lgr_measure(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_params* p, const lgr_feature_params* fp,
                           const lgr_metric_params* mp, const float Tgt16[16], const uint64_t* seeds, int n_times, lgr_measure_run* runs,
                           lgr_measurement* out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (src || ns == 0) && (tgt || nt == 0) && p && ns >= 0 && nt >= 0, LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_metric_params mpd;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.weights(ns, &mp, &mpd));
    return lgr_measure_dev(ctx, ds, ns, dt, nt, p, fp, mp, Tgt16, seeds, n_times, runs, out);
}
