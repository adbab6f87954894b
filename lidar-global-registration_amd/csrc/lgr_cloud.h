// lgr_cloud.h -- the prepared cloud (include/lgr.h: lgr_cloud), the reference's per-cloud Storage (include/matching.h:132-146) on the
// device.  lgr_cloud.hip owns the object and its memory; the per-cloud stages that fill it are the ones of the correspondence search
// (lgr_align.hip), which write into workspace for the unprepared entry points and into the object's memory for lgr_cloud_prepare*.
#pragma once
#include <climits>
#include <new>

#include "lgr_internal.h"

// one level of one cloud: rows descriptor rows of the key points list[0..rows) (indices into the key points) on a surface of
// `surface` points; `off` is the level's row offset into the cloud's row table and list table
struct lgr_cloud_lvl { int log2_radius; float radius, voxel; int rows, surface; size_t off; };

// initialize() of one cloud in multi-scale mode (include/matching.h:176-262): the clamped level range after the pruning, per level the
// key-point list and rows
struct MsSide {
    int min_l2 = INT_MAX, max_l2 = INT_MIN;
    std::vector<lgr_cloud_lvl> levels;
    float* feat = nullptr;                 // device, sum(rows) x D (D = the descriptor's row length)
    int32_t* d_lists = nullptr;            // device, the levels' lists concatenated like the rows
};

// everything the state depends on (floats by their bits): two clouds serve a pair call when theirs equal the two sides of its lgr_params
struct lgr_cloud_key {
    int32_t feature_nr_points, normal_nr_points, normals_available, keypoint_id, has_vp, cluster_k /* 0: no cluster tables */;
    int32_t descriptor_id, lrf_id, arithmetic;
    uint32_t feature_radius, scale_factor, iss_radius, vp[3];
};

struct lgr_cloud {
    int device = 0;
    lgr_cloud_key key{};
    int row_len = 0;
    bool empty = false;                    // fewer than two points: pairs with it have no correspondences
    float* pts = nullptr; int n = 0;       // the cloud
    const float* kps = nullptr; int m = 0; // the key-point cloud (pts itself under keypoint any) ...
    int32_t* kidx = nullptr;               // ... and its indices into the cloud (NULL: 0..n-1)
    bool multiscale = false;
    lgr_cloud_lvl single{};                // single scale: the one level (its list is 0..m-1), rows in `feat`
    float* feat = nullptr;
    MsSide ms;                             // multi-scale
    float* thr = nullptr;                  // the filter's tables (filter_cloud_tables): smoothed densities, cluster k-NN lists
    int32_t* knn = nullptr;
    std::vector<void*> blocks;             // every hipMalloc of the object
    size_t bytes = 0;
};

// memory of the object (hipMalloc, freed by lgr_cloud_destroy); errors are reported on cx
int lgr_cloud_alloc(lgr_ctx* cx, lgr_cloud* c, size_t bytes, void** out);
template <class T>
static inline int lgr_cloud_alloc_t(lgr_ctx* cx, lgr_cloud* c, size_t count, T** out) {
    void* p = nullptr;
    int rc = lgr_cloud_alloc(cx, c, count * sizeof(T), &p);
    *out = (T*) p;
    return rc;
}
// lgr_align.hip: the key of one side of (p, fp) on ctx; the per-cloud stages of one side into a fresh object (checks already made)
int lgr_cloud_key_of(lgr_ctx* ctx, const lgr_params* p, const lgr_feature_params* fp, int side, lgr_cloud_key* out);
int lgr_cloud_fill(lgr_ctx* ctx, lgr_cloud* c, int side, const lgr_params* p, const lgr_feature_params* fp);
// lgr_match_knn.hip: the vote kernel on ctx->stream, nothing read back (the candidates are the pipeline's own, so none is out of range)
int lgr_vote_matches_launch(lgr_ctx* ctx, const int32_t* d_cand_idx, const float* d_cand_dist, int mq, int width, const float* d_train_pts, int mt,
                            float iss_radius, int32_t* d_idx, float* d_dist);
