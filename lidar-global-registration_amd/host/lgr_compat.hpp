// lgr_compat.hpp -- header-only C++ shim that re-exposes the reference's call surface on top of the C ABI (lgr.h).
//
// Mirrors (same names, argument meaning and error behaviour) of:
//   include/alignment.h:6-19              alignPointClouds / alignRansac / alignGror / alignTeaser
//   include/correspondence_search.h:9-28  CorrespondenceSearch, FeatureBasedCorrespondenceSearch
//   include/sac_prerejective_omp.h:21-56  SampleConsensusPrerejectiveOMP
//   include/downsample.h:32               downsamplePointCloud
//   include/common.h:322-332, 360-370     estimateFeatures<FPFH>, estimateFeatures<SHOT>, estimateFeatures<RoPS135> (gravity frames)
//   include/matching.h:373-376            matchBF<FPFH>, matchBF<SHOT>, matchBF<RoPS135>
//   include/transformation.h:6-7          estimateOptimalRigidTransformation
//   include/hypotheses.h:10-16            updateHypotheses, chooseBestHypothesis (the decision; no hypotheses.csv side output)
//   src/common.cpp:531-547, 644-655       calculateSmoothedDensities, estimateNormalsPoints
//   include/analysis.h:14-34, 36-98       calculatePointCloudRmse, calculateOverlapRmse, calculateNormalDifference,
//                                         buildCorrectCorrespondences, AlignmentAnalysis (start without its file side effects)
//   include/common.h:294                  mergeOverlaps
//
// The reference passes pcl::PointCloud<pcl::PointXYZINormal> / pcl::FPFHSignature33 / Eigen::Matrix4f.  Neither PCL
// nor Eigen exists in this image, so the shim is written against three tiny layout-compatible types (lgr::PointN is
// the 48-byte PointXYZINormal, lgr::FPFH the 132-byte signature, lgr::SHOT the 1444-byte pcl::SHOT352, lgr::RoPS135 the 540-byte
// RoPS135, lgr::Matrix4f a column-major 4x4).  A maintainer of the reference defines LGR_COMPAT_POINT_T / LGR_COMPAT_FPFH_T /
// LGR_COMPAT_SHOT_T / LGR_COMPAT_ROPS_T / LGR_COMPAT_MATRIX4F_T to the real types before
// including this header: every access below is either `.points`, `.size()`, `.data()` or a
// reinterpret of the contiguous storage, which the real types provide with the same layout.
#pragma once
#include <algorithm>
#include <array>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lgr.h"

namespace lgr {

#ifndef LGR_COMPAT_POINT_T
struct alignas(16) PointN {   // pcl::PointXYZINormal
    float x = 0, y = 0, z = 0, _pad0 = 1.f;
    float normal_x = 0, normal_y = 0, normal_z = 0, _pad1 = 0;
    float intensity = 0, curvature = 0, _pad2 = 0, _pad3 = 0;
    PointN() = default;
    PointN(float x_, float y_, float z_, float intensity_ = 0.f, float nx = 0.f, float ny = 0.f, float nz = 0.f)
        : x(x_), y(y_), z(z_), normal_x(nx), normal_y(ny), normal_z(nz), intensity(intensity_) {}
};
#else
using PointN = LGR_COMPAT_POINT_T;
#endif
static_assert(sizeof(PointN) == 48, "PointN must be the 48-byte pcl::PointXYZINormal layout");

#ifndef LGR_COMPAT_COLORED_POINT_T
struct alignas(16) PointColoredN {   // pcl::PointXYZRGBNormal (include/common.h: PointColoredN)
    float x = 0, y = 0, z = 0, _pad0 = 1.f;
    float normal_x = 0, normal_y = 0, normal_z = 0, _pad1 = 0;
    std::uint8_t b = 0, g = 0, r = 0, a = 255;
    float curvature = 0, _pad2 = 0, _pad3 = 0;
};
#else
using PointColoredN = LGR_COMPAT_COLORED_POINT_T;
#endif
static_assert(sizeof(PointColoredN) == 48, "PointColoredN must be the 48-byte pcl::PointXYZRGBNormal layout");

#ifndef LGR_COMPAT_FPFH_T
struct FPFH { float histogram[33]; };   // pcl::FPFHSignature33
#else
using FPFH = LGR_COMPAT_FPFH_T;
#endif
static_assert(sizeof(FPFH) == 132, "FPFH must be 33 floats");

#ifndef LGR_COMPAT_SHOT_T
struct SHOT { float descriptor[352]; float rf[9]; };   // pcl::SHOT352
#else
using SHOT = LGR_COMPAT_SHOT_T;
#endif
static_assert(sizeof(SHOT) == 1444, "SHOT must be the 1444-byte pcl::SHOT352 layout (352 + 9 floats)");

#ifndef LGR_COMPAT_ROPS_T
struct RoPS135 { float histogram[135]; };   // pcl::Histogram<135> (include/common.h)
#else
using RoPS135 = LGR_COMPAT_ROPS_T;
#endif
static_assert(sizeof(RoPS135) == 540, "RoPS135 must be the 540-byte pcl::Histogram<135> layout");

#ifndef LGR_COMPAT_MATRIX4F_T
struct Matrix4f {   // column-major like Eigen::Matrix4f
    float m[16];
    static Matrix4f Identity() { Matrix4f r{}; for (int i = 0; i < 16; ++i) r.m[i] = (i % 5 == 0) ? 1.f : 0.f; return r; }
    float& operator()(int row, int col) { return m[4 * col + row]; }
    float operator()(int row, int col) const { return m[4 * col + row]; }
    float* data() { return m; }
    const float* data() const { return m; }
};
#else
using Matrix4f = LGR_COMPAT_MATRIX4F_T;
#endif

template <class T> struct Cloud {   // the subset of pcl::PointCloud<T> the path touches
    using Ptr = std::shared_ptr<Cloud<T>>;
    using ConstPtr = std::shared_ptr<const Cloud<T>>;
    std::vector<T> points;
    unsigned width = 0, height = 1;
    bool is_dense = true;
    std::size_t size() const { return points.size(); }
    bool empty() const { return points.empty(); }
};
using PointNCloud = Cloud<PointN>;
using PointColoredNCloud = Cloud<PointColoredN>;
using FPFHCloud = Cloud<FPFH>;
using SHOTCloud = Cloud<SHOT>;
using RoPS135Cloud = Cloud<RoPS135>;

// include/common.h:120-127
struct Correspondence {
    int index_query = 0, index_match = -1;
    float distance = 3.4028235e38f, threshold = 0.f;
    Correspondence() = default;
    Correspondence(int q, int m, float d, float thr) : index_query(q), index_match(m), distance(d), threshold(thr) {}
};
static_assert(sizeof(Correspondence) == sizeof(lgr_corr), "Correspondence must match lgr_corr");
using Correspondences = std::vector<Correspondence>;
using CorrespondencesPtr = std::shared_ptr<Correspondences>;
using CorrespondencesConstPtr = std::shared_ptr<const Correspondences>;

// include/common.h:192-195
struct MultivaluedCorrespondence { std::vector<int> match_indices; std::vector<float> distances; };

// include/common.h:135-163 (string ids kept; translated to the ABI enums in to_abi)
struct AlignmentParameters {
    bool reestimate_frames{true};
    int feature_nr_points{352}, normal_nr_points{30};
    float edge_thr_coef{0.95f};
    float distance_thr{0.f}, iss_radius_src{0.f}, iss_radius_tgt{0.f};
    std::optional<float> feature_radius;
    float scale_factor{2.0f};
    float confidence{0.999f};
    bool use_bfmatcher{true};
    int bf_block_size{10000};
    int ratio_k{2}, cluster_k{40};
    int randomness{1}, n_samples{3};
    std::string alignment_id{"ransac"}, descriptor_id{"shot"}, keypoint_id{"iss"};
    std::string metric_id{"combination"}, matching_id{"cluster"}, lrf_id{"default"};
    std::string weight_id{"constant"}, score_id{"mse"};
    int max_iterations{0};
    bool save_features{false};
    std::string testname;
    std::optional<Matrix4f> ground_truth;
    bool fix_seed = true, normals_available = false;
    float match_search_radius = 0;
    std::optional<Matrix4f> guess;
    std::string dir_path;
    std::optional<std::array<float, 3>> vp_src, vp_tgt;
};

// include/common.h:165-174
struct AlignmentResult {
    PointNCloud::ConstPtr src, tgt;
    Matrix4f transformation;
    CorrespondencesConstPtr correspondences;
    int iterations = 0;
    bool converged = false;
    double time_te = 0.0, time_cs = 0.0;
};

// ---- context: one per host thread, created lazily on device 0 (override with set_device before the first call)
inline int& device_ordinal() { static int d = 0; return d; }
inline void set_device(int d) { device_ordinal() = d; }
inline lgr_ctx* context() {
    static thread_local lgr_ctx* ctx = nullptr;
    // a liblgr_hip.so of another ABI revision would read lgr_params with another layout (include/lgr.h LGR_VERSION)
    if (!ctx && lgr_version() != LGR_VERSION)
        throw std::runtime_error("lgr: liblgr_hip.so has ABI revision " + std::to_string(lgr_version()) + ", this header is revision " + std::to_string(LGR_VERSION));
    if (!ctx && lgr_ctx_create(device_ordinal(), LGR_STREAM_OWN, &ctx) != LGR_OK)
        throw std::runtime_error("lgr: no MI355X device / context creation failed (there is no CPU fallback)");
    return ctx;
}
inline void check(int rc, const char* what) {
    if (rc != LGR_OK) throw std::runtime_error(std::string("lgr: ") + what + ": " + lgr_last_error(context()));
}

// the reference falls back instead of failing on unknown ids (src/alignment.cpp:96-100, src/matching.cpp:60-64,
// src/metric.cpp:296-300): unknown matching -> lr, unknown metric -> correspondences, unknown alignment -> ransac
inline lgr_params to_abi(const AlignmentParameters& p) {
    lgr_params a;
    lgr_default_params(&a);
    a.feature_nr_points = p.feature_nr_points; a.normal_nr_points = p.normal_nr_points;
    a.edge_thr_coef = p.edge_thr_coef; a.distance_thr = p.distance_thr;
    a.feature_radius = p.feature_radius.value_or(0.f);   // unset -> 0 -> multi-scale matching (include/matching.h:176-208)
    a.scale_factor = p.scale_factor; a.confidence = p.confidence; a.bf_block_size = p.bf_block_size;
    a.cluster_k = p.cluster_k; a.randomness = p.randomness; a.n_samples = p.n_samples;
    a.alignment_id = p.alignment_id == "gror" ? LGR_ALIGN_GROR : LGR_ALIGN_RANSAC;
    // detectKeyPoints (src/common.cpp:657-691): "iss" -> ISS, anything else -> every point (with a warning there)
    a.keypoint_id = p.keypoint_id == "iss" ? LGR_KEYPOINT_ISS : LGR_KEYPOINT_ANY;
    a.iss_radius_src = p.iss_radius_src; a.iss_radius_tgt = p.iss_radius_tgt;
    a.matching_id = p.matching_id == "cluster" ? LGR_MATCH_CLUSTER : (p.matching_id == "one_sided" ? LGR_MATCH_ONE_SIDED :
                    (p.matching_id == "ratio" ? LGR_MATCH_RATIO : LGR_MATCH_LR));   // ratio: ratio_k travels in lgr_feature_params (to_feature_abi)
    a.metric_id = p.metric_id == "uniformity" ? LGR_METRIC_UNIFORMITY : p.metric_id == "closest_plane" ? LGR_METRIC_CLOSEST_PLANE
                  : p.metric_id == "combination" ? LGR_METRIC_COMBINATION
                  : p.metric_id == "weighted_closest_plane" ? LGR_METRIC_WEIGHTED_CLOSEST_PLANE : LGR_METRIC_CORRESPONDENCES;
    a.score_id = p.score_id == "mae" ? LGR_SCORE_MAE : (p.score_id == "mse" ? LGR_SCORE_MSE : (p.score_id == "exp" ? LGR_SCORE_EXP : LGR_SCORE_CONSTANT));
    a.max_iterations = p.max_iterations; a.normals_available = p.normals_available; a.fix_seed = p.fix_seed;
    if (p.vp_src) { a.has_vp_src = 1; std::memcpy(a.vp_src, p.vp_src->data(), 12); }
    if (p.vp_tgt) { a.has_vp_tgt = 1; std::memcpy(a.vp_tgt, p.vp_tgt->data(), 12); }
    a.use_bfmatcher = p.use_bfmatcher ? 1 : 0;
    a.match_search_radius = p.match_search_radius;
    if (p.guess) { a.has_guess = 1; std::memcpy(a.guess, p.guess->data(), 64); }
    return a;
}
// weight_id -> the weights of weighted_closest_plane; unknown names fall back to constant, as getWeightFunction does (src/weights.cpp:27-44,
// with a warning there).  harris / tomasi are passed on and refused by the library (LGR_ERR_UNSUPPORTED).
inline lgr_metric_params to_metric_abi(const AlignmentParameters& p) {
    lgr_metric_params m;
    lgr_default_metric_params(&m);
    const std::string& w = p.weight_id;
    m.weight_id = w == "exp_curvature" ? LGR_WEIGHT_EXP_CURVATURE : w == "curvedness" ? LGR_WEIGHT_CURVEDNESS : w == "harris" ? LGR_WEIGHT_HARRIS
                  : w == "tomasi" ? LGR_WEIGHT_TOMASI : w == "curvature" ? LGR_WEIGHT_CURVATURE : w == "nss" ? LGR_WEIGHT_NSS : LGR_WEIGHT_CONSTANT;
    return m;
}
inline const float* raw(const PointNCloud& c) { return reinterpret_cast<const float*>(c.points.data()); }

// ---- include/downsample.h:32 (pcd_down may alias pcd_fullsize, src/common.cpp:455-456; reference output order)
inline void downsamplePointCloud(const PointNCloud::ConstPtr& pcd_fullsize, PointNCloud::Ptr& pcd_down, float voxel_size) {
    std::vector<PointN> out(pcd_fullsize->size());
    int n_out = 0;
    check(lgr_downsample(context(), raw(*pcd_fullsize), (int) pcd_fullsize->size(), voxel_size, LGR_ORDER_REFERENCE,
                         reinterpret_cast<float*>(out.data()), &n_out), "downsamplePointCloud");
    out.resize(n_out);
    pcd_down->points = std::move(out);
    pcd_down->width = n_out; pcd_down->height = 1; pcd_down->is_dense = true;
}

// ---- src/common.cpp:644-655
inline void estimateNormalsPoints(int k_points, PointNCloud::Ptr& pcd, const PointNCloud::ConstPtr& surface,
                                  const std::optional<std::array<float, 3>>& vp, bool normals_available) {
    check(lgr_normals_knn(context(), reinterpret_cast<float*>(pcd->points.data()), (int) pcd->size(),
                          surface ? raw(*surface) : nullptr, surface ? (int) surface->size() : 0, k_points,
                          vp ? vp->data() : nullptr, normals_available), "estimateNormalsPoints");
}

// ---- include/common.h:322-332 (only the FPFH specialisation exists on this path; the primary template throws, :318-320)
template <class FeatureT>
inline void estimateFeatures(const PointNCloud::ConstPtr&, const PointNCloud::ConstPtr&, typename Cloud<FeatureT>::Ptr&, float, const AlignmentParameters&) {
    throw std::runtime_error("Feature with proposed reference frame isn't supported!");
}
template <>
inline void estimateFeatures<FPFH>(const PointNCloud::ConstPtr& pcd, const PointNCloud::ConstPtr& surface, FPFHCloud::Ptr& features,
                                   float radius_search, const AlignmentParameters&) {
    features->points.resize(pcd->size());
    check(lgr_fpfh(context(), raw(*pcd), (int) pcd->size(), raw(*surface), (int) surface->size(), radius_search,
                   reinterpret_cast<float*>(features->points.data())), "estimateFeatures<FPFH>");
    features->width = (unsigned) pcd->size();
}

// SHOT frames (src/common.cpp:693-755 estimateReferenceFrames, lrf_id compared in lower case): "gt" and "gravity" are not built on the
// device path; any other id is the default frame, as in the reference (which warns and falls back)
inline bool lrf_is_default(std::string id) {
    for (char& c : id) c = (char) std::tolower((unsigned char) c);
    return id != "gt" && id != "gravity";
}
// include/common.h:360-370 estimateFeatures<SHOT>: SHOTEstimationOMP with the frames of estimateReferenceFrames
template <>
inline void estimateFeatures<SHOT>(const PointNCloud::ConstPtr& pcd, const PointNCloud::ConstPtr& surface, SHOTCloud::Ptr& features,
                                   float radius_search, const AlignmentParameters& parameters) {
    if (!lrf_is_default(parameters.lrf_id)) throw std::runtime_error("lgr: lrf '" + parameters.lrf_id + "' is not built on the device path");
    const int m = (int) pcd->size();
    std::vector<float> rows((size_t) m * 352), frames((size_t) m * 9);
    check(lgr_shot(context(), raw(*pcd), m, raw(*surface), (int) surface->size(), radius_search, nullptr, rows.data(), frames.data()),
          "estimateFeatures<SHOT>");
    features->points.resize(m);
    for (int i = 0; i < m; ++i) {
        std::memcpy(features->points[i].descriptor, rows.data() + (size_t) i * 352, 352 * sizeof(float));
        std::memcpy(features->points[i].rf, frames.data() + (size_t) i * 9, 9 * sizeof(float));
    }
    features->width = (unsigned) m;
}

// RoPS frames: "gravity" (compared in lower case) is built; the default frames need GreedyProjectionTriangulation and "gt" the ground
// truth, neither of which the device path has
inline bool lrf_is_gravity(std::string id) {
    for (char& c : id) c = (char) std::tolower((unsigned char) c);
    return id == "gravity";
}
// include/common.h estimateFeatures<RoPS135>: estimateReferenceFrames (gravity), then ROPSEstimationWithLocalReferenceFrames on them
template <>
inline void estimateFeatures<RoPS135>(const PointNCloud::ConstPtr& pcd, const PointNCloud::ConstPtr& surface, RoPS135Cloud::Ptr& features,
                                      float radius_search, const AlignmentParameters& parameters) {
    if (!lrf_is_gravity(parameters.lrf_id))
        throw std::runtime_error("lgr: RoPS is built on gravity frames only (lrf '" + parameters.lrf_id + "' needs a triangulation or the ground truth)");
    const int m = (int) pcd->size();
    std::vector<float> frames((size_t) m * 9);
    check(lgr_gravity_lrf(context(), raw(*pcd), m, raw(*surface), (int) surface->size(), radius_search, frames.data()), "estimateReferenceFrames");
    features->points.resize(m);
    check(lgr_rops(context(), raw(*pcd), m, raw(*surface), (int) surface->size(), radius_search, frames.data(),
                   reinterpret_cast<float*>(features->points.data())), "estimateFeatures<RoPS135>");
    features->width = (unsigned) m;
}

// ---- include/matching.h:373-376, :594-634: every query's list of randomness matches (randomness = 1: the one-match entry points)
template <class FeatureT>
inline std::vector<MultivaluedCorrespondence> matchBF(const typename Cloud<FeatureT>::ConstPtr& query_features,
                                                      const typename Cloud<FeatureT>::ConstPtr& train_features,
                                                      const AlignmentParameters& parameters) {
    static_assert(sizeof(FeatureT) == 132 || sizeof(FeatureT) == 1444 || sizeof(FeatureT) == 540, "only FPFH, SHOT and RoPS135 are built on this path");
    const int k = parameters.randomness;
    if (k < 1 || k > LGR_RANDOMNESS_MAX) throw std::runtime_error("lgr: randomness outside 1..LGR_RANDOMNESS_MAX is not supported");
    int mq = (int) query_features->size(), mt = (int) train_features->size();
    std::vector<int32_t> idx((std::size_t) mq * k);
    std::vector<float> dist((std::size_t) mq * k);
    // SHOT352: the 352 descriptor floats of every row, without the frame; RoPS135 and FPFH rows are contiguous
    auto shot_rows = [](const Cloud<FeatureT>& c) {
        std::vector<float> r(sizeof(FeatureT) == 1444 ? c.size() * 352 : 0);
        if (sizeof(FeatureT) == 1444)
            for (std::size_t i = 0; i < c.size(); ++i) std::memcpy(r.data() + i * 352, &c.points[i], 352 * sizeof(float));
        return r;
    };
    const std::vector<float> q352 = shot_rows(*query_features), t352 = shot_rows(*train_features);
    const float* q = sizeof(FeatureT) == 1444 ? q352.data() : reinterpret_cast<const float*>(query_features->points.data());
    const float* t = sizeof(FeatureT) == 1444 ? t352.data() : reinterpret_cast<const float*>(train_features->points.data());
    if (k > 1) {
        constexpr int row_len = sizeof(FeatureT) == 540 ? 135 : sizeof(FeatureT) == 1444 ? 352 : 33;
        check(lgr_match_knn(context(), row_len, q, mq, t, mt, parameters.bf_block_size, k, idx.data(), dist.data()), "matchBF");
    } else if constexpr (sizeof(FeatureT) == 540) {
        check(lgr_match_rops(context(), q, mq, t, mt, parameters.bf_block_size, idx.data(), dist.data()), "matchBF");
    } else if constexpr (sizeof(FeatureT) == 1444) {
        check(lgr_match_shot(context(), q, mq, t, mt, parameters.bf_block_size, idx.data(), dist.data()), "matchBF");
    } else {
        check(lgr_match_bf(context(), q, mq, t, mt, parameters.bf_block_size, idx.data(), dist.data()), "matchBF");
    }
    std::vector<MultivaluedCorrespondence> out(mq);
    for (int i = 0; i < mq; ++i)
        for (int e = 0; e < k; ++e)
            if (idx[(std::size_t) i * k + e] >= 0) {
                out[i].match_indices.push_back(idx[(std::size_t) i * k + e]);
                out[i].distances.push_back(dist[(std::size_t) i * k + e]);
            }
    return out;
}

namespace detail {
template <class FeatureT>
constexpr int row_len() { return sizeof(FeatureT) == 540 ? 135 : sizeof(FeatureT) == 1444 ? 352 : 33; }
// SHOT352: the 352 descriptor floats of every row, without the frame (as matchBF strips them); empty for the other descriptors
template <class FeatureT>
inline std::vector<float> shot_rows(const Cloud<FeatureT>& c) {
    std::vector<float> r(sizeof(FeatureT) == 1444 ? c.size() * 352 : 0);
    if (sizeof(FeatureT) == 1444)
        for (std::size_t i = 0; i < c.size(); ++i) std::memcpy(r.data() + i * 352, &c.points[i], 352 * sizeof(float));
    return r;
}
// the rows an entry point reads: the stripped copy for SHOT, the cloud's own (contiguous) rows otherwise
template <class FeatureT>
inline const float* rows(const Cloud<FeatureT>& c, const std::vector<float>& stripped) {
    return sizeof(FeatureT) == 1444 ? stripped.data() : reinterpret_cast<const float*>(c.points.data());
}
}  // namespace detail

// ---- include/matching.h:367-370 (randomness = 1; exact search, so the rows matchBF finds -- tests/flann_bf_matcher.h:82-83)
template <class FeatureT>
inline std::vector<MultivaluedCorrespondence> matchFLANN(const typename Cloud<FeatureT>::ConstPtr& query_features,
                                                         const typename Cloud<FeatureT>::ConstPtr& train_features,
                                                         const AlignmentParameters& parameters) {
    static_assert(sizeof(FeatureT) == 132 || sizeof(FeatureT) == 1444 || sizeof(FeatureT) == 540, "only FPFH, SHOT and RoPS135 are built on this path");
    if (parameters.randomness != 1) throw std::runtime_error("lgr: randomness > 1 is not built for matchFLANN (the reference leaves its tie order unspecified)");
    int mq = (int) query_features->size(), mt = (int) train_features->size();
    std::vector<int32_t> idx(mq);
    std::vector<float> dist(mq);
    if constexpr (sizeof(FeatureT) == 132) {
        check(lgr_match_flann(context(), reinterpret_cast<const float*>(query_features->points.data()), mq,
                              reinterpret_cast<const float*>(train_features->points.data()), mt, idx.data(), dist.data()), "matchFLANN");
    } else {
        const std::vector<float> q352 = detail::shot_rows(*query_features), t352 = detail::shot_rows(*train_features);
        check(lgr_match_flann_rows(context(), detail::row_len<FeatureT>(), detail::rows(*query_features, q352), mq, detail::rows(*train_features, t352), mt,
                                   idx.data(), dist.data()), "matchFLANN");
    }
    std::vector<MultivaluedCorrespondence> out(mq);
    for (int i = 0; i < mq; ++i)
        if (idx[i] >= 0) { out[i].match_indices.push_back(idx[i]); out[i].distances.push_back(dist[i]); }
    return out;
}

// ---- include/matching.h:378-382: the reference takes the train cloud as a pcl::search::KdTree; here it is the cloud itself
template <class FeatureT>
inline std::vector<MultivaluedCorrespondence> matchLocal(const PointNCloud::ConstPtr& query_pcd, const PointNCloud::ConstPtr& train_pcd,
                                                         const typename Cloud<FeatureT>::ConstPtr& query_features,
                                                         const typename Cloud<FeatureT>::ConstPtr& train_features,
                                                         const AlignmentParameters& parameters, const Matrix4f& guess) {
    static_assert(sizeof(FeatureT) == 132 || sizeof(FeatureT) == 1444 || sizeof(FeatureT) == 540, "only FPFH, SHOT and RoPS135 are built on this path");
    const int k = parameters.randomness;
    if (k < 1 || k > LGR_RANDOMNESS_MAX) throw std::runtime_error("lgr: randomness outside 1..LGR_RANDOMNESS_MAX is not supported");
    int mq = (int) query_features->size(), mt = (int) train_features->size();
    if ((int) query_pcd->size() != mq || (int) train_pcd->size() != mt) throw std::runtime_error("lgr: matchLocal: clouds and feature clouds differ in size");
    std::vector<int32_t> idx((std::size_t) mq * k);
    std::vector<float> dist((std::size_t) mq * k);
    if (sizeof(FeatureT) == 132 && k == 1) {
        check(lgr_match_local(context(), raw(*query_pcd), mq, raw(*train_pcd), mt, reinterpret_cast<const float*>(query_features->points.data()),
                              reinterpret_cast<const float*>(train_features->points.data()), guess.data(), parameters.match_search_radius,
                              idx.data(), dist.data()), "matchLocal");
    } else {
        const std::vector<float> q352 = detail::shot_rows(*query_features), t352 = detail::shot_rows(*train_features);
        check(lgr_match_local_knn(context(), detail::row_len<FeatureT>(), raw(*query_pcd), mq, raw(*train_pcd), mt, detail::rows(*query_features, q352),
                                  detail::rows(*train_features, t352), guess.data(), parameters.match_search_radius, k, idx.data(), dist.data()), "matchLocal");
    }
    std::vector<MultivaluedCorrespondence> out(mq);
    for (int i = 0; i < mq; ++i)
        for (int e = 0; e < k; ++e)
            if (idx[(std::size_t) i * k + e] >= 0) {
                out[i].match_indices.push_back(idx[(std::size_t) i * k + e]);
                out[i].distances.push_back(dist[(std::size_t) i * k + e]);
            }
    return out;
}

// ---- src/common.cpp:531-547
inline std::vector<float> calculateSmoothedDensities(const PointNCloud::ConstPtr& pcd, int k = 2) {
    if (!(pcd->size() > 1 && k >= 2)) throw std::runtime_error("Assertion 3458240390587502 failed!");   // rassert
    std::vector<float> out(pcd->size());
    check(lgr_smoothed_densities(context(), raw(*pcd), (int) pcd->size(), k, out.data()), "calculateSmoothedDensities");
    return out;
}

// ---- include/transformation.h:6-7
inline void estimateOptimalRigidTransformation(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt,
                                               const Correspondences& inliers, Matrix4f& transformation) {
    check(lgr_refit_svd(context(), raw(*src), raw(*tgt), (int) src->size(), (int) tgt->size(),
                        reinterpret_cast<const lgr_corr*>(inliers.data()), (int) inliers.size(), transformation.data()),
          "estimateOptimalRigidTransformation");
}

// ---- not in the reference: its final block's closest-plane step (src/sac_prerejective_omp.cpp:270-291) in the dense form, repeated while
// the metric rises (lgr_refine_plane).  parameters.score_id scores the inliers; metric_id "weighted_closest_plane" evaluates with the
// weights of parameters.weight_id, anything else with closest_plane.  The threshold is the target's density.
inline Matrix4f refineTransformation(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& tn,
                                     const AlignmentParameters& parameters, int max_steps, lgr_refine_result& result) {
    lgr_refine_params rp;
    lgr_default_refine_params(&rp);
    rp.score_id = to_abi(parameters).score_id;
    rp.max_steps = max_steps;
    const lgr_metric_params mp = to_metric_abi(parameters);
    check(lgr_refine_plane(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(), tn.data(), &rp,
                           parameters.metric_id == "weighted_closest_plane" ? &mp : nullptr, &result, nullptr, nullptr),
          "refineTransformation");
    Matrix4f out;
    std::memcpy(out.data(), result.transformation, 64);
    return out;
}
inline Matrix4f refineTransformation(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& tn,
                                     const AlignmentParameters& parameters, int max_steps) {
    lgr_refine_result result;
    return refineTransformation(src, tgt, tn, parameters, max_steps, result);
}

// ---- not in the reference: point-to-plane ICP from tn (lgr_icp_plane_host).  max_dist <= 0: 4 x the target's
// density; the other parameters are lgr_default_icp_params' (the overload with `params` takes them all from the caller).
inline Matrix4f icpPointToPlane(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& tn, const lgr_icp_params& params,
                                lgr_icp_result& result) {
    check(lgr_icp_plane_host(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(), tn.data(), &params, &result, nullptr, nullptr),
          "icpPointToPlane");
    Matrix4f out;
    std::memcpy(out.data(), result.transformation, 64);
    return out;
}
inline Matrix4f icpPointToPlane(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& tn, float max_dist, int max_iterations,
                                lgr_icp_result& result) {
    lgr_icp_params ip;
    lgr_default_icp_params(&ip);
    ip.max_dist = max_dist;
    ip.max_iterations = max_iterations;
    return icpPointToPlane(src, tgt, tn, ip, result);
}
inline Matrix4f icpPointToPlane(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& tn, float max_dist, int max_iterations) {
    lgr_icp_result result;
    return icpPointToPlane(src, tgt, tn, max_dist, max_iterations, result);
}

// ---- not in the reference: the ICP variants from tn (lgr_icp_ex_host; DESIGN.md section 4, "ICP variants").  `options` is the ABI's
// struct, filled by lgr_default_icp_ex_params and then by the caller: variant, robust kernel and scale, normal gate, plane_eps, per-point
// weights (host floats, one per source point, or null) and the base parameters of icpPointToPlane.
inline Matrix4f icpRegistration(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& tn, const lgr_icp_ex_params& options,
                                lgr_icp_result& result) {
    check(lgr_icp_ex_host(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(), tn.data(), &options, &result, nullptr, nullptr),
          "icpRegistration");
    Matrix4f out;
    std::memcpy(out.data(), result.transformation, 64);
    return out;
}
inline Matrix4f icpRegistration(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& tn, const lgr_icp_ex_params& options) {
    lgr_icp_result result;
    return icpRegistration(src, tgt, tn, options, result);
}

// ---- not in the reference: trimmed ICP from tn (lgr_icp_trim_host; DESIGN.md section 4, "Trimmed ICP").  `options` as icpRegistration's;
// keep in (0, 1]: the fraction of each iteration's pairs, smallest residuals first, that contributes; scale_from_median > 0: the robust
// kernel's scale is that multiple of the iteration's median residual (1.4826: the MAD rule) and options.robust_scale is not read.
// keep 1 and scale_from_median 0 is icpRegistration.  info, when given, receives one record per evaluated iteration.
inline Matrix4f icpRegistrationTrimmed(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& tn, const lgr_icp_ex_params& options,
                                       float keep, float scale_from_median, lgr_icp_result& result, std::vector<lgr_icp_trim_step>* info = nullptr) {
    lgr_icp_trim_params tp;
    lgr_default_icp_trim_params(&tp);
    tp.ex = options; tp.keep = keep; tp.scale_from_median = scale_from_median;
    int n = 0;
    const int room = options.base.max_iterations < 1 ? 1 : options.base.max_iterations > LGR_ICP_MAX_ITERATIONS ? LGR_ICP_MAX_ITERATIONS : options.base.max_iterations;
    if (info) info->assign((size_t) room, lgr_icp_trim_step{});   // (a count outside [0, LGR_ICP_MAX_ITERATIONS] is refused by the call)
    check(lgr_icp_trim_host(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(), tn.data(), &tp, &result, nullptr, info ? info->data() : nullptr, &n),
          "icpRegistrationTrimmed");
    if (info) info->resize((size_t) n);
    Matrix4f out;
    std::memcpy(out.data(), result.transformation, 64);
    return out;
}
inline Matrix4f icpRegistrationTrimmed(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& tn, const lgr_icp_ex_params& options,
                                       float keep, float scale_from_median) {
    lgr_icp_result result;
    return icpRegistrationTrimmed(src, tgt, tn, options, keep, scale_from_median, result);
}

// ---- include/hypotheses.h:10-12
inline void updateHypotheses(std::vector<Matrix4f>& transformations, std::vector<float>& metrics, const Matrix4f& new_transformation,
                             float new_metric, const AlignmentParameters& parameters) {
    if (transformations.size() != metrics.size()) throw std::runtime_error("Assertion 45832351834023 failed!");
    int n = (int) metrics.size(), cap = n + 1;
    std::vector<float> buf((size_t) cap * 16), met(cap);
    for (int i = 0; i < n; ++i) { std::memcpy(&buf[16 * (size_t) i], transformations[i].data(), 64); met[i] = metrics[i]; }
    int m = lgr_update_hypotheses(buf.data(), met.data(), n, cap, new_transformation.data(), new_metric, parameters.distance_thr);
    if (m < 0) throw std::runtime_error("lgr: updateHypotheses failed");
    transformations.resize(m); metrics.resize(m);
    for (int i = 0; i < m; ++i) { std::memcpy(transformations[i].data(), &buf[16 * (size_t) i], 64); metrics[i] = met[i]; }
}

// ---- include/hypotheses.h:14-16 (src/hypotheses.cpp:50-129): the hypothesis whose correspondence inliers are spread most uniformly,
// identity when none has a positive uniformity
inline Matrix4f chooseBestHypothesis(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const CorrespondencesConstPtr& correspondences,
                                     const AlignmentParameters& params, std::vector<Matrix4f>& tns) {
    (void) params;
    std::vector<float> buf(std::max<size_t>(tns.size(), 1) * 16);
    for (size_t i = 0; i < tns.size(); ++i) std::memcpy(&buf[16 * i], tns[i].data(), 64);
    Matrix4f out;
    int best = -1;
    check(lgr_choose_best_hypothesis(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(),
                                     reinterpret_cast<const lgr_corr*>(correspondences->data()), (int) correspondences->size(), buf.data(), (int) tns.size(),
                                     out.data(), &best, nullptr),
          "chooseBestHypothesis");
    return out;
}

// descriptor_id / lrf_id -> lgr_feature_params: "fpfh" or "shot" (the struct default, include/common.h:148) or "rops".  The frames matter to
// SHOT and RoPS only (FPFH never reads lrf_id, include/common.h:366,407)
inline lgr_feature_params to_feature_abi(const AlignmentParameters& parameters_) {
    lgr_feature_params f;
    lgr_default_feature_params(&f);
    f.ratio_k = parameters_.ratio_k;   // read under matching_id "ratio" only (include/common.h:146)
    if (parameters_.descriptor_id == "shot") {
        f.descriptor_id = LGR_DESCRIPTOR_SHOT;
        if (!lrf_is_default(parameters_.lrf_id)) f.lrf_id = LGR_LRF_GRAVITY;
    } else if (parameters_.descriptor_id == "rops") {   // gravity frames only (estimateFeatures<RoPS135> above)
        if (!lrf_is_gravity(parameters_.lrf_id))
            throw std::runtime_error("lgr: RoPS is built on gravity frames only (lrf '" + parameters_.lrf_id + "' needs a triangulation or the ground truth)");
        f.descriptor_id = LGR_DESCRIPTOR_ROPS;
        f.lrf_id = LGR_LRF_GRAVITY;
    } else if (parameters_.descriptor_id != "fpfh") {
        throw std::runtime_error("lgr: only descriptors 'fpfh', 'shot' and 'rops' are built on the device path");
    }
    return f;
}

// ---- include/correspondence_search.h:9-28
class CorrespondenceSearch {
public:
    virtual CorrespondencesPtr calculateCorrespondences() = 0;
    virtual ~CorrespondenceSearch() = default;
};
// one lgr_cloud for the duration of a scope (include/lgr.h: prepared clouds), the reference's per-cloud Storage (include/matching.h:132-146)
class PreparedCloud {
public:
    PreparedCloud(const PointNCloud& cloud, int side, const lgr_params& a, const lgr_feature_params& f) {
        check(lgr_cloud_prepare(context(), reinterpret_cast<const float*>(cloud.points.data()), (int) cloud.size(), side, &a, &f, &cloud_), "lgr_cloud_prepare");
    }
    ~PreparedCloud() { lgr_cloud_destroy(cloud_); }
    PreparedCloud(const PreparedCloud&) = delete;
    PreparedCloud& operator=(const PreparedCloud&) = delete;
    const lgr_cloud* get() const { return cloud_; }
private:
    lgr_cloud* cloud_ = nullptr;
};
// AlignmentParameters::save_features: the writer of one level's descriptor table lives with the other file formats in lgr_io.hpp
// (saveFeatures, include/feature_analysis.h:11-27), which registers it here when it is included; a caller that never sets save_features
// needs neither.
using FeatureSaver = void (*)(const AlignmentParameters& parameters, bool is_source, const std::optional<int>& log2_radius, const float* rows, std::size_t n,
                              std::size_t row_len);
inline FeatureSaver& feature_saver() { static FeatureSaver saver = nullptr; return saver; }

class FeatureBasedCorrespondenceSearch : CorrespondenceSearch {
public:
    FeatureBasedCorrespondenceSearch() = delete;
    FeatureBasedCorrespondenceSearch(PointNCloud::ConstPtr src, PointNCloud::ConstPtr tgt, AlignmentParameters parameters)
        : src_(std::move(src)), tgt_(std::move(tgt)), parameters_(std::move(parameters)) {}
    CorrespondencesPtr calculateCorrespondences() override {
        // key points: "iss" or every point (src/common.cpp:657-691; other ids fall back to every point there too)
        // descriptor: "fpfh" or "shot" (the struct default, include/common.h:148).  The frames matter to SHOT only (FPFH never reads lrf_id,
        // include/common.h:366,407): "gt" / "gravity" give LGR_ERR_UNSUPPORTED there, every other id is the default frame.
        lgr_feature_params f = to_feature_abi(parameters_);
        lgr_params a = to_abi(parameters_);
        auto out = std::make_shared<Correspondences>(src_->size());
        int n = 0;
        // initialize() per cloud (include/matching.h:164-262), then the pair: the bytes lgr_correspondences_ex returns
        PreparedCloud src(*src_, 0, a, f), tgt(*tgt_, 1, a, f);
        check(lgr_correspondences_prepared(context(), src.get(), tgt.get(), &a, &f, reinterpret_cast<lgr_corr*>(out->data()), &n), "calculateCorrespondences");
        out->resize(n);
        if (parameters_.save_features) saveFeatures(src.get(), tgt.get());
        return out;
    }
protected:
    // include/matching.h:273-279: the tables of every level the two clouds share, source -> target only (!inverse_tn)
    void saveFeatures(const lgr_cloud* src, const lgr_cloud* tgt) const {
        if (!feature_saver()) throw std::runtime_error("lgr: save_features needs lgr_io.hpp (saveFeatures) in the program");
        const lgr_cloud* clouds[2] = {src, tgt};
        struct lgr_cloud_info info[2];
        for (int s = 0; s < 2; ++s) check(lgr_cloud_info(clouds[s], &info[s]), "lgr_cloud_info");
        if (!info[0].levels || !info[1].levels) return;
        const int lo = std::max(info[0].first_log2_radius, info[1].first_log2_radius);
        const int hi = std::min(info[0].first_log2_radius + info[0].levels, info[1].first_log2_radius + info[1].levels) - 1;
        std::vector<float> rows;
        for (int log2_radius = lo; log2_radius <= hi; ++log2_radius)
            for (int s = 0; s < 2; ++s) {
                lgr_cloud_level_info li;
                const int level = log2_radius - info[s].first_log2_radius;
                check(lgr_cloud_level(clouds[s], level, &li, nullptr, nullptr), "lgr_cloud_level");
                rows.resize((std::size_t) li.rows * (std::size_t) info[s].row_len);
                check(lgr_cloud_level(clouds[s], level, nullptr, nullptr, rows.data()), "lgr_cloud_level");
                feature_saver()(parameters_, s == 0, info[s].multiscale ? std::optional<int>(log2_radius) : std::nullopt, rows.data(), (std::size_t) li.rows,
                                (std::size_t) info[s].row_len);
            }
    }
    PointNCloud::ConstPtr src_, tgt_;
    AlignmentParameters parameters_;
};

// ---- include/sac_prerejective_omp.h:21-56
#ifndef LGR_SAVE_MULTIPLE_HYPOTHESES_MAX
#define LGR_SAVE_MULTIPLE_HYPOTHESES_MAX 64   // members the set may hold under LGR_SAVE_MULTIPLE_HYPOTHESES (at most LGR_HYPOTHESES_MAX)
#endif
class SampleConsensusPrerejectiveOMP {
public:
    SampleConsensusPrerejectiveOMP() = delete;
    SampleConsensusPrerejectiveOMP(PointNCloud::ConstPtr src, PointNCloud::ConstPtr tgt, CorrespondencesConstPtr correspondences,
                                   AlignmentParameters parameters)
        : src_(std::move(src)), tgt_(std::move(tgt)), correspondences_(std::move(correspondences)), parameters_(std::move(parameters)) {}
    // A translation unit that defines LGR_SAVE_MULTIPLE_HYPOTHESES before this header gets the reference's SAVE_MULTIPLE_HYPOTHESES mode
    // (src/sac_prerejective_omp.cpp:11): the set of distinct hypotheses, the final block on every member, chooseBestHypothesis' pick.
    AlignmentResult align() {
        lgr_params a = to_abi(parameters_);
        lgr_result r;
#ifdef LGR_SAVE_MULTIPLE_HYPOTHESES
        hypotheses_.assign(LGR_SAVE_MULTIPLE_HYPOTHESES_MAX, lgr_hypothesis{});
        int n = 0;
        best_hypothesis_ = -1;
        lgr_metric_params m = to_metric_abi(parameters_);   // (every metric_id; weight_id is read under weighted_closest_plane)
        const int rc = lgr_ransac_multi_ex(context(), raw(*src_), (int) src_->size(), raw(*tgt_), (int) tgt_->size(),
                                           reinterpret_cast<const lgr_corr*>(correspondences_->data()), (int) correspondences_->size(), &a, &m,
                                           LGR_SAVE_MULTIPLE_HYPOTHESES_MAX, &r, hypotheses_.data(), &n, &best_hypothesis_);
        hypotheses_.resize(rc == LGR_OK ? n : 0);
        check(rc, "SampleConsensusPrerejectiveOMP::align (multiple hypotheses)");
#else
        lgr_metric_params m = to_metric_abi(parameters_);
        check(lgr_ransac_ex(context(), raw(*src_), (int) src_->size(), raw(*tgt_), (int) tgt_->size(),
                            reinterpret_cast<const lgr_corr*>(correspondences_->data()), (int) correspondences_->size(), &a, &m, &r, nullptr),
              "SampleConsensusPrerejectiveOMP::align");
#endif
        AlignmentResult out;
        out.src = src_; out.tgt = tgt_; out.correspondences = correspondences_;
        std::memcpy(out.transformation.data(), r.transformation, 64);
        out.iterations = r.iterations; out.converged = r.converged != 0; out.time_te = r.time_te;
        return out;
    }
    inline std::string getClassName() const { return "SampleConsensusPrerejectiveOMP"; }
    // the set the last align() kept, in set order, and the index chooseBestHypothesis picked (-1: none; always empty / -1 without
    // LGR_SAVE_MULTIPLE_HYPOTHESES)
    inline const std::vector<lgr_hypothesis>& getHypotheses() const { return hypotheses_; }
    inline int getBestHypothesisIndex() const { return best_hypothesis_; }
protected:
    PointNCloud::ConstPtr src_, tgt_;
    CorrespondencesConstPtr correspondences_;
    AlignmentParameters parameters_;
    std::vector<lgr_hypothesis> hypotheses_;
    int best_hypothesis_ = -1;
};

// ---- include/alignment.h:6-19
inline AlignmentResult alignRansac(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt,
                                   const CorrespondencesPtr& correspondences, const AlignmentParameters& parameters) {
    SampleConsensusPrerejectiveOMP ransac(src, tgt, correspondences, parameters);
    return ransac.align();
}
// src/alignment.cpp:21-35: resolution = distance_thr, K_optimal = 800, iterations = 1, converged = true
inline AlignmentResult alignGror(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const CorrespondencesPtr& correspondences,
                                 const AlignmentParameters& parameters) {
    lgr_result r;
    check(lgr_gror(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(),
                   reinterpret_cast<const lgr_corr*>(correspondences->data()), (int) correspondences->size(), parameters.distance_thr, 800, &r, nullptr),
          "alignGror");
    AlignmentResult out;
    out.src = src; out.tgt = tgt; out.correspondences = correspondences;
    std::memcpy(out.transformation.data(), r.transformation, 64);
    out.iterations = 1; out.converged = true; out.time_te = r.time_te;
    return out;
}
// src/alignment.cpp:37-69: the reference throws "Not implemented: support TEASER" (:40); its commented-out body (:41-69) names the
// estimator and its parameters -- noise_bound = distance_thr, cbar2 = 1, no scale, GNC-TLS rotation with 100 iterations, factor 1.4 and cost
// threshold 0.005 -- and reports iterations = 1.  Here it is carried out by lgr_teaser (include/lgr.h; the statement: DESIGN.md section 4).
// converged = a solution was found (a clique of at least three correspondences); without one the transformation is the identity.
inline AlignmentResult alignTeaser(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const CorrespondencesPtr& correspondences,
                                   const AlignmentParameters& parameters, lgr_teaser_info* info_out = nullptr) {
    lgr_teaser_params tp;
    lgr_default_teaser_params(&tp, parameters.distance_thr);
    lgr_result r;
    lgr_teaser_info info;
    check(lgr_teaser(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(),
                     reinterpret_cast<const lgr_corr*>(correspondences->data()), (int) correspondences->size(), &tp, &r, &info, nullptr, nullptr),
          "alignTeaser");
    if (info_out) *info_out = info;
    AlignmentResult out;
    out.src = src; out.tgt = tgt; out.correspondences = correspondences;
    std::memcpy(out.transformation.data(), r.transformation, 64);
    out.iterations = 1; out.converged = info.valid != 0; out.time_te = r.time_te;
    return out;
}
// src/alignment.cpp:72-109 without the two CSV side effects (correspondences csv, transformations.csv)
inline AlignmentResult alignPointClouds(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const AlignmentParameters& params) {
    FeatureBasedCorrespondenceSearch corr_search(src, tgt, params);
    CorrespondencesPtr correspondences = corr_search.calculateCorrespondences();
    AlignmentResult result;
    if (params.alignment_id == "gror") result = alignGror(src, tgt, correspondences, params);
    else if (params.alignment_id == "teaser") result = alignTeaser(src, tgt, correspondences, params);
    else result = alignRansac(src, tgt, correspondences, params);   // unknown ids fall back to RANSAC (:96-100)
    return result;
}


// ---- include/utils.h:68-88: the two aggregates of the measure test type, under the reference's names and in its arithmetic (the mean is a
//      double sum divided by (T) size; the deviation a T sum of squared differences, the population form; quiet NaN for an empty list)
template <typename T>
T calculateMean(const std::vector<T>& values) {
    if (values.empty()) return (T) std::numeric_limits<float>::quiet_NaN();
    double sum = 0.0;
    for (const T& x : values) sum += x;
    return (T) (sum / (T) values.size());
}
template <typename T>
T calculateStandardDeviation(const std::vector<T>& values) {
    if (values.empty()) return (T) std::numeric_limits<float>::quiet_NaN();
    const T mean = calculateMean(values);
    T squares = 0;
    for (const T& x : values) {
        const T d = x - mean;
        squares += d * d;
    }
    return std::sqrt(squares / (T) values.size());
}

// ---- the loop of measureTestResults (src/main.cpp:338-380) for one parameter set: n_times alignments that differ in the RANSAC seed only
//      (seeds empty: the ABI's default seed + i), one correspondence search, every run judged against the ground truth (lgr_measure).
//      No file side effects: the test_measurements.csv row is the caller's (its columns are the measurement's fields in order).
struct MeasurementResult {
    lgr_measurement measurement;          // success_rate, mae, sae, mte, ste, mrmse, srmse, mtime, stime
    std::vector<lgr_measure_run> runs;    // the runs made, in order: seed, lgr_result, lgr_gt_eval
};
inline MeasurementResult measureAlignment(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const AlignmentParameters& parameters,
                                          const Matrix4f& transformation_gt, int n_times = 10, const std::vector<uint64_t>& seeds = {}) {
    if (parameters.alignment_id == "teaser") throw std::runtime_error("Not implemented: support TEASER");   // src/alignment.cpp:40
    if (!seeds.empty() && (int) seeds.size() != n_times) throw std::invalid_argument("lgr: measureAlignment takes one seed per run");
    lgr_params a = to_abi(parameters);
    a.fix_seed = 0;   // src/main.cpp:339
    lgr_feature_params f = to_feature_abi(parameters);
    lgr_metric_params m = to_metric_abi(parameters);
    MeasurementResult out;
    out.runs.assign(n_times > 0 ? (size_t) n_times : 1, lgr_measure_run{});
    check(lgr_measure(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(), &a, &f, &m, transformation_gt.data(),
                      seeds.empty() ? nullptr : seeds.data(), n_times, out.runs.data(), &out.measurement), "measureAlignment");
    out.runs.resize((size_t) out.measurement.n_times);
    return out;
}

// ---- include/analysis.h, include/common.h:294: the ground-truth analysis on the device (declared orders: DESIGN.md section 4).  Each free
//      function runs its own pass only (the host building blocks of lgr.h); AlignmentAnalysis runs the whole evaluation once.
inline lgr_gt_eval evaluateGroundTruth(const PointNCloud& src, const PointNCloud& tgt, const Correspondences& correspondences,
                                       const Matrix4f& transformation, const Matrix4f& transformation_gt, float distance_thr, bool converged,
                                       std::vector<uint8_t>* correct = nullptr) {
    lgr_gt_eval e;
    if (correct) correct->assign(correspondences.size(), 0);
    check(lgr_evaluate_gt(context(), raw(src), (int) src.size(), raw(tgt), (int) tgt.size(), reinterpret_cast<const lgr_corr*>(correspondences.data()),
                          (int) correspondences.size(), transformation.data(), transformation_gt.data(), distance_thr, converged ? 1 : 0, nullptr, &e,
                          correct && !correct->empty() ? correct->data() : nullptr), "evaluateGroundTruth");
    return e;
}
// src/analysis.cpp:30-43 (the point pass against an empty target: no neighbour is found; the threshold only has to be valid)
inline float calculatePointCloudRmse(const PointNCloud::ConstPtr& pcd, const Matrix4f& transformation, const Matrix4f& transformation_gt) {
    float rmse = 0.f, pcd_err = 0.f;
    int n = 0;
    check(lgr_overlap_rmse(context(), raw(*pcd), (int) pcd->size(), nullptr, 0, transformation.data(), transformation_gt.data(), 1.f, &rmse, &n,
                           &pcd_err, nullptr), "calculatePointCloudRmse");
    return pcd_err;
}
// src/analysis.cpp:45-88
inline float calculateOverlapRmse(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& transformation,
                                  const Matrix4f& transformation_gt, float inlier_threshold) {
    float rmse = 0.f;
    int n = 0;
    check(lgr_overlap_rmse(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(), transformation.data(), transformation_gt.data(),
                           inlier_threshold, &rmse, &n, nullptr, nullptr), "calculateOverlapRmse");
    return rmse;
}
// src/analysis.cpp:141-185 (without checkNormals' assert)
inline float calculateNormalDifference(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, float distance_thr,
                                       const Matrix4f& transformation_gt) {
    float diff = 0.f;
    int n = 0;
    check(lgr_normal_difference(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(), transformation_gt.data(), distance_thr, &diff, &n),
          "calculateNormalDifference");
    return diff;
}
// src/analysis.cpp:187-206
inline void buildCorrectCorrespondences(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Correspondences& correspondences,
                                        Correspondences& correct_correspondences, const Matrix4f& transformation_gt) {
    std::vector<uint8_t> correct(correspondences.size(), 0);
    int n3[3];
    check(lgr_correct_correspondences(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(),
                                      reinterpret_cast<const lgr_corr*>(correspondences.data()), (int) correspondences.size(), transformation_gt.data(),
                                      nullptr, correct.empty() ? nullptr : correct.data(), n3), "buildCorrectCorrespondences");
    correct_correspondences.clear();
    correct_correspondences.reserve((size_t) n3[0]);
    for (size_t i = 0; i < correspondences.size(); ++i)
        if (correct[i]) correct_correspondences.push_back(correspondences[i]);
}
// src/common.cpp:558-591 (include/common.h:294): pcd1 is compared as it is (the caller has moved it already), so the ABI's ground truth is
// the identity, which moves no finite point; dst = the kept rows of pcd1, then of pcd2, each in index order
inline void mergeOverlaps(const PointNCloud::ConstPtr& pcd1, const PointNCloud::ConstPtr& pcd2, PointNCloud::Ptr& dst, float distance_thr) {
    std::vector<uint8_t> m1(pcd1->size() + 1, 0), m2(pcd2->size() + 1, 0);
    int n2[2];
    float overlap = 0.f;
    const Matrix4f I = Matrix4f::Identity();
    check(lgr_merge_overlaps(context(), raw(*pcd1), (int) pcd1->size(), raw(*pcd2), (int) pcd2->size(), I.data(), distance_thr, m1.data(), m2.data(), n2,
                             &overlap, nullptr), "mergeOverlaps");
    dst->points.clear();
    dst->points.reserve((size_t) n2[0] + (size_t) n2[1]);
    for (size_t i = 0; i < pcd1->size(); ++i)
        if (m1[i]) dst->points.push_back(pcd1->points[i]);
    for (size_t i = 0; i < pcd2->size(); ++i)
        if (m2[i]) dst->points.push_back(pcd2->points[i]);
    dst->width = (unsigned) dst->points.size(); dst->height = 1;
}

// ---- the debug layer (src/common.cpp:818-835, 859-906, 1149-1159; src/main.cpp:152-205) on the device: declared orders in DESIGN.md
//      section 4.  The functions that write files (saveTemperatureMaps, savePointCloudWithCorrespondences, ...) are in lgr_io.hpp.
constexpr int COLOR_BEIGE = LGR_COLOR_BEIGE, COLOR_RED = LGR_COLOR_RED, COLOR_PARAKEET = LGR_COLOR_PARAKEET, COLOR_BLUE = LGR_COLOR_BLUE,
              COLOR_WHITE = LGR_COLOR_WHITE;
enum class TemperatureType { Distance, NormalDifference };

// src/common.cpp:818-835 (the library's kernels compute the same expression; compile without floating-point contraction to get their bits)
inline int getColor(float v, float vmin, float vmax) {
    float r = 1.f, g = 1.f, b = 1.f;
    float dv = vmax - vmin;
    v = std::max(vmin, std::min(v, vmax));
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
    auto c8 = [](float c) { const float x = 255.f * c; return x == x ? ((int) x & 255) : 0; };   // a NaN channel (vmin == vmax) is 0
    return (c8(r) << 16) + (c8(g) << 8) + c8(b);
}
// src/common.cpp:1149-1159
inline void setPointColor(PointColoredN& point, int color) {
    point.r = (color >> 16) & 0xff;
    point.g = (color >> 8) & 0xff;
    point.b = (color >> 0) & 0xff;
}
inline void mixPointColor(PointColoredN& point, int color) {
    point.r = point.r / 2 + ((color >> 16) & 0xff) / 2;
    point.g = point.g / 2 + ((color >> 8) & 0xff) / 2;
    point.b = point.b / 2 + ((color >> 0) & 0xff) / 2;
}
inline void setPointColor(PointColoredN& point, std::uint8_t red, std::uint8_t green, std::uint8_t blue) { point.r = red; point.g = green; point.b = blue; }
inline const float* raw(const PointColoredNCloud& c) { return reinterpret_cast<const float*>(c.points.data()); }
// pcl::copyPoint PointN -> PointColoredN: the fields both have (x y z, the normal, curvature)
inline void copyPoint(const PointN& in, PointColoredN& out) {
    out.x = in.x; out.y = in.y; out.z = in.z;
    out.normal_x = in.normal_x; out.normal_y = in.normal_y; out.normal_z = in.normal_z;
    out.curvature = in.curvature;
}

// pcl::transformPointCloudWithNormals on the host, in the order the library moves a cloud: x c0 + (y c1 + (z c2 + c3)),
// a normal the same without c3; the other fields are copied.  in and out may be the same cloud.
template <class PointT>
inline void transformPointCloudWithNormals(const Cloud<PointT>& in, Cloud<PointT>& out, const Matrix4f& T) {
    const float* M = T.data();
    if (&in != &out) out = in;
    for (PointT& p : out.points) {
        const float x = p.x, y = p.y, z = p.z, nx = p.normal_x, ny = p.normal_y, nz = p.normal_z;
        p.x = M[0] * x + (M[4] * y + (M[8] * z + M[12]));
        p.y = M[1] * x + (M[5] * y + (M[9] * z + M[13]));
        p.z = M[2] * x + (M[6] * y + (M[10] * z + M[14]));
        p.normal_x = M[0] * nx + (M[4] * ny + M[8] * nz);
        p.normal_y = M[1] * nx + (M[5] * ny + M[9] * nz);
        p.normal_z = M[2] * nx + (M[6] * ny + M[10] * nz);
    }
}

// src/common.cpp:859-906: colours `compared` and fills `temperatures`.  The library reads rows of 12 floats whose first two quads are the
// point and the normal: the layout of PointColoredN as well.  Returns the number of temperatures below distance_max.
inline int calculateTemperatureMap(PointColoredNCloud::Ptr& compared, PointColoredNCloud::Ptr& reference, TemperatureType type,
                                   std::vector<float>& temperatures, float /* temperature_min: 0 in every caller */, float /* temperature_max */,
                                   float distance_max) {
    const int n = (int) compared->size();
    temperatures.assign((size_t) n, type == TemperatureType::Distance ? distance_max : (float) M_PI / 2);
    std::vector<std::int32_t> colors((size_t) n + 1, getColor(1.f, 0.f, 1.f));
    lgr_temperature_out out{};
    int n_below = 0;
    if (type == TemperatureType::Distance) { out.temp_distance = temperatures.data(); out.color_distance = colors.data(); }
    else { out.temp_normal = temperatures.data(); out.color_normal = colors.data(); }
    check(lgr_temperature_map(context(), raw(*compared), n, raw(*reference), (int) reference->size(), distance_max, n ? &out : nullptr, &n_below),
          "calculateTemperatureMap");
    for (int i = 0; i < n; ++i) setPointColor(compared->points[(size_t) i], colors[(size_t) i]);
    return n_below;
}

// src/main.cpp:152-205: the two printed lines, and the numbers beside them
struct OverlapComparison { int count[2]; float weighted_count[2]; };
inline OverlapComparison compareOverlaps(const PointNCloud::ConstPtr& src, const PointNCloud::ConstPtr& tgt, const Matrix4f& transformation,
                                         const Matrix4f& transformation_gt, const AlignmentParameters& parameters) {
    float tns[32];
    std::memcpy(tns, transformation.data(), 64);
    std::memcpy(tns + 16, transformation_gt.data(), 64);
    OverlapComparison r{};
    std::int32_t counts[2] = {0, 0};
    check(lgr_compare_overlaps(context(), raw(*src), (int) src->size(), raw(*tgt), (int) tgt->size(), tns, 2, parameters.distance_thr, counts,
                               r.weighted_count, nullptr, nullptr, nullptr), "compareOverlaps");
    r.count[0] = counts[0]; r.count[1] = counts[1];
    std::cerr << "\tincorrect hypothesis: " << r.count[0] << " points, " << r.weighted_count[0] << "weighted points\n";
    std::cerr << "\t  correct hypothesis: " << r.count[1] << " points, " << r.weighted_count[1] << "weighted points\n";
    return r;
}

// ---- include/utils.h:13-25, include/metric.h: the metric estimators in their DENSE form (sparse = false), the form AlignmentAnalysis and
//      estimateTestMetric use.  The dense evaluations draw no random numbers: `rand` is accepted and never called.
class UniformRandIntGenerator {
public:
    UniformRandIntGenerator(const int min, const int max, std::mt19937::result_type seed = std::random_device{}()) : dist_(min, max), gen_(seed) {}
    int operator()() { return dist_(gen_); }
private:
    std::uniform_int_distribution<int> dist_;
    std::mt19937 gen_;
};

enum ScoreFunction { Constant, MAE, MSE, EXP };

inline int weight_abi(const std::string& w) {   // unknown names fall back to constant, as getWeightFunction does (src/weights.cpp:27-44)
    return w == "exp_curvature" ? LGR_WEIGHT_EXP_CURVATURE : w == "curvedness" ? LGR_WEIGHT_CURVEDNESS : w == "harris" ? LGR_WEIGHT_HARRIS
           : w == "tomasi" ? LGR_WEIGHT_TOMASI : w == "curvature" ? LGR_WEIGHT_CURVATURE : w == "nss" ? LGR_WEIGHT_NSS : LGR_WEIGHT_CONSTANT;
}

class MetricEstimator {
public:
    using Ptr = std::shared_ptr<MetricEstimator>;
    using ConstPtr = std::shared_ptr<const MetricEstimator>;
    explicit MetricEstimator(ScoreFunction score_function = ScoreFunction::Constant) : score_function_(score_function) {}
    virtual ~MetricEstimator() = default;
    virtual float getInitialMetric() const { return 0.0f; }
    virtual float getMinTolerableMetric() const { return 0.0f; }
    virtual void buildInliersAndEstimateMetric(const Matrix4f& transformation, Correspondences& inliers, float& rmse, float& metric,
                                               UniformRandIntGenerator& rand) const = 0;
    // src/metric.cpp:83-101: the same test as buildCorrectCorrespondences (src/analysis.cpp:187-206), over the inliers
    virtual void buildCorrectInliers(const Correspondences& inliers, Correspondences& correct_inliers, const Matrix4f& transformation_gt) const {
        buildCorrectCorrespondences(src_, tgt_, inliers, correct_inliers, transformation_gt);
    }
    virtual inline void setCorrespondences(const CorrespondencesConstPtr& correspondences) { correspondences_ = correspondences; }
    virtual inline void setSourceCloud(const PointNCloud::ConstPtr& src) { src_ = src; }
    virtual inline void setTargetCloud(const PointNCloud::ConstPtr& tgt) { tgt_ = tgt; }
    virtual std::string getClassName() const = 0;

protected:
    // lgr_analysis_metric under metric_id for this estimator's clouds, correspondences and score.  The inliers of the plane metrics are the
    // device's list; those of the correspondence estimator are the correspondences the device's mask marks, their distance recomputed here
    // in f32 as |T p - q| (the device reports the mask, the count and the sums, not the distances)
    void evaluate(int metric_id, int score_id, const lgr_metric_params* mp, const Matrix4f& transformation, Correspondences& inliers, float& rmse,
                  float& metric) const {
        if (!src_ || !tgt_) throw std::runtime_error("lgr: MetricEstimator: setSourceCloud / setTargetCloud first");
        static const Correspondences none;
        const Correspondences& corr = correspondences_ ? *correspondences_ : none;
        const bool plane = metric_id == LGR_METRIC_CLOSEST_PLANE || metric_id == LGR_METRIC_WEIGHTED_CLOSEST_PLANE;
        std::vector<uint8_t> mask(corr.size() + 1, 0);
        std::vector<lgr_corr> list(plane ? src_->size() + 1 : 1);
        lgr_metric_eval e;
        check(lgr_analysis_metric(context(), raw(*src_), (int) src_->size(), raw(*tgt_), (int) tgt_->size(), reinterpret_cast<const lgr_corr*>(corr.data()),
                                  (int) corr.size(), transformation.data(), nullptr, metric_id, score_id, mp, &e, plane ? nullptr : mask.data(),
                                  plane ? list.data() : nullptr), getClassName().c_str());
        rmse = e.rmse;
        metric = e.metric;
        inliers.clear();
        inliers.reserve((size_t) e.n_inliers);
        if (plane) {
            for (int i = 0; i < e.n_inliers; ++i) inliers.emplace_back(list[i].index_query, list[i].index_match, list[i].distance, list[i].threshold);
            return;
        }
        const float* T = transformation.data();
        for (size_t i = 0; i < corr.size(); ++i) {
            if (!mask[i]) continue;
            const float* p = raw(*src_) + 12 * (size_t) corr[i].index_query;
            const float* q = raw(*tgt_) + 12 * (size_t) corr[i].index_match;
            float d[3];
            for (int r = 0; r < 3; ++r) d[r] = (((T[r] * p[0] + T[4 + r] * p[1]) + T[8 + r] * p[2]) + T[12 + r]) - q[r];
            inliers.emplace_back(corr[i].index_query, corr[i].index_match, std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), corr[i].threshold);
        }
    }
    int score_abi() const {
        return score_function_ == MAE ? LGR_SCORE_MAE : score_function_ == MSE ? LGR_SCORE_MSE : score_function_ == EXP ? LGR_SCORE_EXP : LGR_SCORE_CONSTANT;
    }
    static void refuse_sparse(bool sparse) {
        // the sparse 1 % subset of this path is defined by Philox and a per-hypothesis counter, which this signature cannot carry
        if (sparse) throw std::invalid_argument("lgr: the sparse closest-plane estimator takes a Philox counter: call lgr_evaluate_plane_dev "
                                                "(lgr_evaluate_plane_weighted_dev) instead");
    }
    CorrespondencesConstPtr correspondences_;
    PointNCloud::ConstPtr src_, tgt_;
    ScoreFunction score_function_;
};

class CorrespondencesMetricEstimator : public MetricEstimator {
public:
    explicit CorrespondencesMetricEstimator(ScoreFunction score_function = ScoreFunction::Constant) : MetricEstimator(score_function) {}
    void buildInliersAndEstimateMetric(const Matrix4f& transformation, Correspondences& inliers, float& rmse, float& metric,
                                       UniformRandIntGenerator&) const override {
        evaluate(LGR_METRIC_CORRESPONDENCES, score_abi(), nullptr, transformation, inliers, rmse, metric);
    }
    inline std::string getClassName() const override { return "CorrespondencesMetricEstimator"; }
};

class UniformityMetricEstimator : public CorrespondencesMetricEstimator {
public:
    UniformityMetricEstimator() : CorrespondencesMetricEstimator(ScoreFunction::Constant) {}
    inline float getMinTolerableMetric() const override { return 0.3f; }
    void buildInliersAndEstimateMetric(const Matrix4f& transformation, Correspondences& inliers, float& rmse, float& metric,
                                       UniformRandIntGenerator&) const override {
        evaluate(LGR_METRIC_UNIFORMITY, score_abi(), nullptr, transformation, inliers, rmse, metric);
    }
};

class ClosestPlaneMetricEstimator : public MetricEstimator {
public:
    explicit ClosestPlaneMetricEstimator(bool sparse = false, ScoreFunction score_function = ScoreFunction::Constant) : MetricEstimator(score_function) {
        refuse_sparse(sparse);
    }
    void buildInliersAndEstimateMetric(const Matrix4f& transformation, Correspondences& inliers, float& rmse, float& metric,
                                       UniformRandIntGenerator&) const override {
        evaluate(LGR_METRIC_CLOSEST_PLANE, score_abi(), nullptr, transformation, inliers, rmse, metric);
    }
    inline std::string getClassName() const override { return "ClosestPlaneMetricEstimator"; }
};

class WeightedClosestPlaneMetricEstimator : public MetricEstimator {
public:
    WeightedClosestPlaneMetricEstimator() = delete;
    // nr_points: the library computes the weights with k = 30 neighbours, the reference's NORMAL_NR_POINTS -- the only value it is ever called with
    WeightedClosestPlaneMetricEstimator(std::string weight_id, int nr_points, bool sparse = false, ScoreFunction score_function = ScoreFunction::Constant)
        : MetricEstimator(score_function), weight_id_(std::move(weight_id)) {
        refuse_sparse(sparse);
        if (nr_points != 30) throw std::invalid_argument("lgr: WeightedClosestPlaneMetricEstimator: nr_points must be 30 (NORMAL_NR_POINTS)");
    }
    void buildInliersAndEstimateMetric(const Matrix4f& transformation, Correspondences& inliers, float& rmse, float& metric,
                                       UniformRandIntGenerator&) const override {
        lgr_metric_params m;
        lgr_default_metric_params(&m);
        m.weight_id = weight_abi(weight_id_);
        evaluate(LGR_METRIC_WEIGHTED_CLOSEST_PLANE, score_abi(), &m, transformation, inliers, rmse, metric);
    }
    inline std::string getClassName() const override { return "WeightedClosestPlaneMetricEstimator"; }
protected:
    std::string weight_id_;
};

class CombinationMetricEstimator : public MetricEstimator {
public:
    explicit CombinationMetricEstimator(bool sparse = false, ScoreFunction score_function = ScoreFunction::Constant) : MetricEstimator(score_function) {
        refuse_sparse(sparse);
    }
    // inliers and rmse of the correspondence estimator (constant score), metric = metric_cs * metric_cp (src/metric.cpp:239-250)
    void buildInliersAndEstimateMetric(const Matrix4f& transformation, Correspondences& inliers, float& rmse, float& metric,
                                       UniformRandIntGenerator&) const override {
        evaluate(LGR_METRIC_COMBINATION, score_abi(), nullptr, transformation, inliers, rmse, metric);
    }
    inline std::string getClassName() const override { return "CombinationMetricEstimator"; }
};

// src/metric.cpp:270-301.  sparse = true throws (std::invalid_argument, naming lgr_evaluate_plane_dev) for the plane-based estimators
inline MetricEstimator::Ptr getMetricEstimatorFromParameters(const AlignmentParameters& parameters, bool sparse = false) {
    const std::string& s = parameters.score_id;
    const ScoreFunction score_function = s == "mae" ? ScoreFunction::MAE : s == "mse" ? ScoreFunction::MSE : s == "exp" ? ScoreFunction::EXP : ScoreFunction::Constant;
    if (parameters.metric_id == "uniformity") return std::make_shared<UniformityMetricEstimator>();
    if (parameters.metric_id == "closest_plane") return std::make_shared<ClosestPlaneMetricEstimator>(sparse, score_function);
    if (parameters.metric_id == "weighted_closest_plane")
        return std::make_shared<WeightedClosestPlaneMetricEstimator>(parameters.weight_id, 30 /* NORMAL_NR_POINTS */, sparse, score_function);
    if (parameters.metric_id == "combination") return std::make_shared<CombinationMetricEstimator>(sparse, score_function);
    return std::make_shared<CorrespondencesMetricEstimator>(score_function);   // unknown ids too (with a warning in the reference)
}

// include/analysis.h:36-98.  start() prints nothing and writes no results.csv (the reference's print() / save()): the figures are read
// through the getters, evaluation() and its neighbours metric(), rmse(), inliers(), correctInliers().
class AlignmentAnalysis {
public:
    AlignmentAnalysis() {}
    // src/analysis.cpp:208-216: the estimator is the dense one of the parameters' metric
    AlignmentAnalysis(AlignmentResult result, AlignmentParameters parameters) : parameters_(std::move(parameters)), result_(std::move(result)) {
        metric_estimator_ = getMetricEstimatorFromParameters(parameters_);
        metric_estimator_->setSourceCloud(result_.src);
        metric_estimator_->setTargetCloud(result_.tgt);
        metric_estimator_->setCorrespondences(result_.correspondences);
    }
    void start(const std::optional<Matrix4f>& transformation_gt, const std::string& testname) {
        testname_ = testname;
        has_gt_ = transformation_gt.has_value();
        // :222-223, with or without a ground truth (clouds the dense plane evaluation cannot take -- none, an empty source, fewer than two
        // target points -- leave metric 0, rmse FLT_MAX and no inliers)
        inliers_.clear(); correct_inliers_.clear();
        metric_ = 0.f; rmse_ = std::numeric_limits<float>::max();
        if (metric_estimator_ && result_.src && result_.tgt && result_.src->size() > 0 && result_.tgt->size() > 1) {
            UniformRandIntGenerator rand(0, std::numeric_limits<int>::max(), 566 /* SEED */);
            metric_estimator_->buildInliersAndEstimateMetric(result_.transformation, inliers_, rmse_, metric_, rand);
            if (has_gt_) metric_estimator_->buildCorrectInliers(inliers_, correct_inliers_, transformation_gt.value());   // :236
        }
        if (!has_gt_) return;
        static const Correspondences none;
        eval_ = evaluateGroundTruth(*result_.src, *result_.tgt, result_.correspondences ? *result_.correspondences : none, result_.transformation,
                                    transformation_gt.value(), parameters_.distance_thr, result_.converged);
    }
    inline bool alignmentHasConverged() const { return result_.converged; }
    inline Matrix4f getTransformation() const { return result_.transformation; }
    inline float getRotationError() const { return has_gt_ ? eval_.r_err : nan_(); }
    inline float getTranslationError() const { return has_gt_ ? eval_.t_err : nan_(); }
    inline float getOverlapError() const { return has_gt_ ? eval_.overlap_rmse : nan_(); }
    inline float getPointCloudError() const { return has_gt_ ? eval_.pcd_err : nan_(); }
    inline float getRunningTime() const { return (float) (result_.time_cs + result_.time_te); }
    inline MetricEstimator::Ptr getMetricEstimator() { return metric_estimator_; }
    inline const lgr_gt_eval& evaluation() const { return eval_; }   // every figure of start(), src/main.cpp:356's verdict included
    // start()'s first statement and buildCorrectInliers.  The reference keeps these four private and only streams them (print, results.csv)
    inline float metric() const { return metric_; }
    inline float rmse() const { return rmse_; }
    inline const Correspondences& inliers() const { return inliers_; }
    inline const Correspondences& correctInliers() const { return correct_inliers_; }
private:
    static float nan_() { return std::numeric_limits<float>::quiet_NaN(); }
    AlignmentParameters parameters_;
    AlignmentResult result_;
    lgr_gt_eval eval_{};
    MetricEstimator::Ptr metric_estimator_;
    Correspondences inliers_, correct_inliers_;
    float metric_ = 0.f, rmse_ = std::numeric_limits<float>::max();
    bool has_gt_ = false;
    std::string testname_;
};

}  // namespace lgr
