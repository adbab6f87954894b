/*
 * lgr.h -- C ABI of the MI355X-native global-registration hot path (liblgr_hip.so).
 *
 * Drop-in boundary for aleksandrina-streltsova/lidar-global-registration.  The reference has no FFI layer: its
 * boundary is the C++ header surface include/alignment.h:6-19, include/correspondence_search.h:9-28,
 * include/sac_prerejective_omp.h:21-56 plus the free functions named below.  Each entry point cites the reference
 * interface it replaces; lidar-global-registration_amd/host/ holds the header-only C++ shim that re-exposes the
 * reference names on top of this ABI, and INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.  Every call returns an int status (LGR_OK == 0, negative =
 *     error); nothing throws across the ABI.  "not converged" is NOT an error: see lgr_result.converged.
 *   - point  : 12 floats, pcl::PointXYZINormal layout {x,y,z,1 | nx,ny,nz,0 | intensity,curvature,pad,pad} (48 B)
 *   - fpfh   : 33 floats (pcl::FPFHSignature33, 132 B, row-major M x 33)
 *   - shot   : 352 floats (pcl::SHOT352::descriptor, 1408 B, row-major M x 352); frames 9 floats (pcl::ReferenceFrame)
 *   - rops   : 135 floats (RoPS135::histogram, 540 B, row-major M x 135)
 *   - corr   : lgr_corr (include/common.h:120-127 Correspondence), 16 B
 *   - T      : 16 floats COLUMN-major (Eigen::Matrix4f default)
 *   - host entry points (no suffix) borrow caller memory for the duration of the call, upload, run the device
 *     path and download.  *_dev entry points take DEVICE pointers (HIP), enqueue on the context stream and are
 *     asynchronous unless stated; outputs are caller-allocated device buffers.
 *   - one lgr_ctx per host thread / GPU.  A ctx owns its workspace (grown on demand, never inside a timed launch
 *     once warmed up) and is not re-entrant.  Several contexts on ONE device are allowed, but by default they take turns call
 *     by call (lgr_ctx_options.concurrent_contexts): results are then bit-identical to a serial run by construction.
 *   - the HIP extension is mandatory: there is no CPU fallback anywhere behind this ABI.
 */
#ifndef LGR_H
#define LGR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision.  Still 5 with trimmed ICP: lgr_icp_trim_params, lgr_icp_trim_step, lgr_default_icp_trim_params, lgr_icp_trim_dev,
 * lgr_icp_trim_host, lgr_rank_select_dev and lgr_rank_select_host are additions; lgr_icp_ex*, lgr_icp_plane* and their structs did not
 * change.  Still 5 with the ICP variants: lgr_icp_ex_params, LGR_ICP_POINT_TO_* / LGR_ICP_PLANE_TO_PLANE, LGR_ICP_ROBUST_*,
 * lgr_default_icp_ex_params, lgr_icp_ex_dev and lgr_icp_ex_host are additions; lgr_icp_plane* and its structs did not change.  Still 5 with point-to-plane ICP: lgr_icp_params, lgr_icp_step, lgr_icp_result, LGR_ICP_*, lgr_default_icp_params,
 * lgr_icp_plane_dev and lgr_icp_plane_host are additions; no struct or entry point that existed changed.  Still 5 with the reference point order on the device: lgr_hash_order_dev, lgr_downsample_order_dev, lgr_dedupe_order_dev,
 * lgr_preprocess_order_dev and lgr_selfcheck_hash_order are additions; no struct or entry point that existed changed.  Still 5 with the prepared clouds: lgr_cloud, struct lgr_cloud_info, lgr_cloud_level_info, lgr_cloud_prepare*, lgr_cloud_destroy,
 * lgr_cloud_info, lgr_cloud_keypoints*, lgr_cloud_level*, lgr_correspondences_prepared*, lgr_align_prepared and the host twin lgr_nearest are
 * additions; no struct or entry point that existed changed.  Still 5 with the ratio matcher: lgr_feature_params.ratio_k takes the first of that struct's reserved words (a host that
 * zeroes them gets k = 2, MATCHING_RATIO_K, and the word is read under LGR_MATCH_RATIO only), LGR_MATCH_RATIO and the lgr_ratio_test* /
 * lgr_match_ratio* entry points are additions.  5 (round 5): lgr_ctx_options.arithmetic / pcl_neighbour_cap and lgr_match_options.auto_dense / irregular_rows (former reserved words: a host that zeroes
 * them keeps the default arithmetic and switches auto_dense and the irregular-row lane off), lgr_match_last_lbstats, lgr_match_last_irregular, lgr_selfcheck_philox,
 * lgr_selfcheck_libm added; the DEFAULT arithmetic of the normals and pair features changed to PCL's own sequences (results differ from
 * revision 4 at rounding level).  4 (round 4): lgr_match_options.split_sweep / kept_cap and lgr_ctx_options.concurrent_contexts (former reserved words: a host that
 * zeroes them switches the split off and keeps the contexts exclusive), lgr_match_last_issued, lgr_selfcheck_rcp added.  3 (round 3): lgr_match_options.shell_bound (one of the reserved words: a host that zeroes them would switch the shell
 * bound off), lgr_match_last_shell added.  2 (round 3): lgr_match_last_* take the context, lgr_ctx_options / lgr_ctx_host_threads added;
 * lgr_params grew in revision 1 -> 2 as well (use_bfmatcher, has_guess, match_search_radius, guess).  A host built against another revision must not
 * call in: check lgr_version() == LGR_VERSION once after loading (lgr_amd/capi.py and host/lgr_compat.hpp do). */
#define LGR_VERSION 5

enum {
    LGR_OK = 0,
    LGR_ERR_INVALID_ARG = -1,
    LGR_ERR_NO_DEVICE = -2,
    LGR_ERR_OOM = -3,
    LGR_ERR_HIP = -4,          /* a HIP runtime call failed; see lgr_last_error */
    LGR_ERR_UNSUPPORTED = -5,  /* e.g. n_samples outside 3..8, randomness outside 1..LGR_RANDOMNESS_MAX (or > 1 with FLANN / a guess), alignment teaser
                                  through lgr_align* (TEASER is the stand-alone lgr_teaser*), a k_select outside 3..LGR_TEASER_NODES_MAX,
                                  LGR_MATCH_RATIO with ratio_k outside 2..LGR_RANDOMNESS_MAX, randomness > 1, FLANN or a guess */
    LGR_ERR_VOXEL_TOO_SMALL = -6
};

enum { LGR_RANDOMNESS_MAX = 8 };                                               /* the longest match list per key point */
enum { LGR_MATCH_LR = 0, LGR_MATCH_ONE_SIDED = 1, LGR_MATCH_CLUSTER = 2, LGR_MATCH_RATIO = 3 };   /* src/matching.cpp:21-75 */
#define LGR_MATCHING_RATIO_THRESHOLD 1.1f   /* MATCHING_RATIO_THRESHOLD include/common.h:50: what the pipeline uses under LGR_MATCH_RATIO */
enum { LGR_METRIC_CORRESPONDENCES = 0, LGR_METRIC_UNIFORMITY = 1, LGR_METRIC_CLOSEST_PLANE = 2, LGR_METRIC_COMBINATION = 3,
       LGR_METRIC_WEIGHTED_CLOSEST_PLANE = 4 };   /* src/metric.cpp:272-301 */
enum { LGR_SCORE_CONSTANT = 0, LGR_SCORE_MAE = 1, LGR_SCORE_MSE = 2, LGR_SCORE_EXP = 3 };
enum { LGR_ALIGN_RANSAC = 0, LGR_ALIGN_GROR = 1 };                              /* src/alignment.cpp:92-101 */
enum { LGR_KEYPOINT_ANY = 0, LGR_KEYPOINT_ISS = 1 };                            /* src/common.cpp:657-691 */
enum { LGR_ORDER_REFERENCE = 0, LGR_ORDER_CANONICAL = 1 };                      /* downsample output order */

typedef struct { int32_t index_query, index_match; float distance, threshold; } lgr_corr;

/* mirrors AlignmentParameters (include/common.h:135-163); string ids become enums; optionals become has_* flags */
typedef struct {
    int32_t feature_nr_points;   /* 352 */
    int32_t normal_nr_points;    /* 30 */
    float   edge_thr_coef;       /* 0.95 */
    float   distance_thr;
    float   feature_radius;      /* > 0: single scale; <= 0 = unset: multi-scale (include/matching.h:176-262) */
    float   scale_factor;        /* 2.0 */
    float   confidence;          /* 0.999 */
    int32_t bf_block_size;       /* ALIGNMENT_BLOCK_SIZE (lgr_default_params: 10000); every shipped YAML sets 200000 (data/test.yaml:12) */
    int32_t cluster_k;           /* 40 */
    int32_t randomness;          /* matches per key point and level before the vote, 1..LGR_RANDOMNESS_MAX (data/test.yaml:14 ships 1).
                                    > 1: the brute-force matcher only (use_bfmatcher = 1, no guess, else LGR_ERR_UNSUPPORTED), and the
                                    iss_radius_* of a side whose key points are voted on must be finite and > 0 (LGR_ERR_INVALID_ARG) */
    int32_t n_samples;           /* 3 (every shipped config); 3..8 accepted: sampler, polygon test and Umeyama are generic in it,
                                    src/sac_prerejective_omp.cpp:33-77,105-108,220 */
    int32_t alignment_id, matching_id, metric_id, score_id;
    int32_t max_iterations;
    int32_t normals_available;
    int32_t fix_seed;            /* 1: seed = 566 (SEED include/common.h:25); 0: seed field below */
    int32_t has_vp_src, has_vp_tgt;
    float   vp_src[3], vp_tgt[3];
    int32_t ransac_batch;        /* iterations per device batch (deterministic schedule), default 65536 */
    uint64_t seed;
    int32_t keypoint_id;         /* LGR_KEYPOINT_ANY (every point, BASELINE configs) or LGR_KEYPOINT_ISS */
    float   iss_radius_src, iss_radius_tgt;   /* include/common.h:139; salient = non-maxima radius */
    int32_t use_bfmatcher;       /* 1 (ALIGNMENT_USE_BFMATCHER include/common.h:41); 0: matchFLANN (include/matching.h:309) */
    /* include/common.h:158-160: "cannot be set in config, set before alignment steps" */
    int32_t has_guess;           /* 1: matching is matchLocal around guess * p (include/matching.h:294-299) and the guess is the
                                  *    hypothesis RANSAC has to beat (src/sac_prerejective_omp.cpp:134-147) */
    float   match_search_radius;
    float   guess[16];           /* column-major */
} lgr_params;

/* mirrors AlignmentResult (include/common.h:165-174) + diagnostics */
typedef struct {
    float   transformation[16];  /* column-major */
    int32_t iterations;
    int32_t converged;
    int32_t n_inliers;
    float   metric;
    float   best_metric_before_refit;
    int32_t best_iteration;
    int32_t num_rejections;
    int32_t estimated_iters;
    int32_t n_correspondences;
    double  time_cs, time_te;    /* seconds, device-synchronised wall time */
    float   stage_ms[12];        /* 0 downsample 1 normals 2 fpfh (the descriptor stage: FPFH or SHOT) 3 match 4 filter 5 ransac 6 refit (hipEvent) */
} lgr_result;

typedef struct lgr_ctx lgr_ctx;

/* How a context uses the HOST and the device queue (never what it returns).  Independent pieces of the path -- the two clouds'
 * feature stages, the two sides / directions of the matcher, the match filter's per-cloud tables -- run side by side on up to two
 * internal contexts, each with a stream of its own and ONE persistent helper host thread (started on first use, parked on a
 * condition variable between calls).  helper_contexts = 0 turns that off: every piece runs on the context's own stream from the
 * calling thread (no extra threads, no extra streams; the internal contexts remain as workspaces only) -- for hosts that give a
 * rank fewer cores than 3, at the price of the overlap (about +20 % per 1M-point pair). */
typedef struct {
    int32_t helper_contexts;      /* 1 (default) / 0 */
    int32_t concurrent_contexts;  /* 0 (default): the contexts of one device take turns call by call -- the device never executes two
                                   * contexts' work side by side (a context's own helper streams are not affected).  1 (EXPERIMENTAL): this
                                   * context does not wait its turn.  Several pairs in flight per GPU bought +5 % throughput at best
                                   * (DESIGN.md section 10).  Every kernel is deterministic and contexts share no state, so results must not
                                   * depend on it, and the -m gpu suite asserts exactly that (tests/test_gpu_concurrent_contexts.py: three
                                   * overlapping contexts bit-equal to the serial run); but in round 3 the builder's MI355X boxes returned
                                   * normals that differed at rounding level between runs when 2-3 contexts worked at once, and rounds 4-5
                                   * could not reproduce that on the units they were given -- not even with the round-3 binary -- so the
                                   * cause is not established.  Do not enable it where bit-reproducibility is a requirement.  One process per
                                   * GPU (the multi-GPU layout) never has two contexts on a device. */
    int32_t arithmetic;           /* LGR_ARITH_FAST (0, default) / LGR_ARITH_PCL (1): see below */
    int32_t pcl_neighbour_cap;    /* LGR_ARITH_PCL: neighbours of a key point sorted at once; 0 default (512), 1024, 64 (tests: drives the shell path).  Never changes results */
    int32_t ransac_schedule;      /* how the RANSAC loop (uniformity / correspondences metrics) is driven; never changes results.
                                   * LGR_RANSAC_SCHEDULE_DEFAULT (0) = LGR_RANSAC_SCHEDULE_CHAIN (1): device-driven chain of launches, six per round;
                                   * LGR_RANSAC_SCHEDULE_RESIDENT (2): ONE resident kernel for the whole loop (a workgroup per CU, phases handed over
                                   * at grid barriers).  The plane metrics always use the chain. */
    int32_t reserved[3];
} lgr_ctx_options;
enum { LGR_RANSAC_SCHEDULE_DEFAULT = 0, LGR_RANSAC_SCHEDULE_CHAIN = 1, LGR_RANSAC_SCHEDULE_RESIDENT = 2 };
/* Arithmetic of the third-party pieces (normals, pair features, FPFH weighting: PCL 1.12.1 behind include/common.h:322-332 and
 * src/common.cpp:644-655).  In BOTH modes the normals are pcl::eigen33's closed form and the pair features use the acosf swap test and the
 * atan2f of the named libm (GNU libc 2.35's float routines restated op for op: csrc/lgr_libm.cuh, pinned against the running libm by
 * tests/test_oracle_libm.py) -- PCL's own sequences since round 5.  The modes differ in the FPFH weighting only:
 *   LGR_ARITH_FAST  one fused multiply-add chain per bin over the neighbours in grid order (what v_mfma_f32_16x16x4_f32 computes), block
 *                   normaliser from the finished bins: rounding-level deviation from PCL (measured: profiles/r5_pcl_order_by_piece_1M.json);
 *   LGR_ARITH_PCL   pcl::FPFHEstimation::weightPointSPFHSignature as written: neighbours by ascending (squared distance, index),
 *                   val = hist * w rounded, float adds, double block sums of the vals (a sort per key point: several ms per 1M-point cloud).
 * Each mode is bit-identical to the oracle's mode of the same name (ORC_ARITH_CANONICAL / ORC_ARITH_PCL). */
enum { LGR_ARITH_FAST = 0, LGR_ARITH_PCL = 1 };

/* How the brute-force matcher runs (NEVER what it returns: every setting gives the same matches and distance bits).  The
 * defaults are the production schedule; the other values exist so that tests can drive every path at small sizes and so that
 * profiles can switch single mechanisms off.  Held by the context: lgr_ctx_set_match_options. */
typedef struct {
    int32_t prune;            /* exact bound-based tile skipping: -1 auto (on from 65536 x 65536 pairs), 0 off (dense), 1 on */
    int32_t leaves;           /* second-level k-means leaves per cluster: 0 auto (about 1024 rows per leaf), else 1 .. 64 */
    int32_t near;             /* pass-0 width: nearest leaves per row block / row blocks per leaf; 0 = default (40) */
    int32_t operand_format;   /* -1 auto (f16 two-term splits, rotated to 30 coordinates when the rows allow it), 0 f32, 1 f16, 2 f16 rotated */
    int32_t box_bounds;       /* bounding-box lower bounds beside the ball bounds: 1 PCA basis (default), 2 raw coordinates, 0 off */
    int32_t column_stage;     /* per-stage column criterion in the final schedule: 1 (default) / 0 */
    int32_t coarse_rejection; /* two-step coarse test in the final MFMA pass: 1 (default: unless the pass schedules more than half of all tiles --
                               * descriptors the bounds cannot separate --, then the plain six-step kernel), 2 (always), 0 (never) */
    int32_t rerank_refilter;  /* MFMA re-filter of the rerank's candidate groups: 1 (default) / 0 (whole-group exact scan) */
    int32_t pair_cap;         /* pairs per rerank item the re-filter may emit before falling back to the group scan: -1 default (8) */
    int32_t poison_tables;    /* diagnostics: fill never-computed minimum-table entries with 0 (nothing may read them) */
    int32_t self_check;       /* diagnostics: device check of the proven filter bound (lgr_match_last_check, lgr_match_last_check_cover):
                               * 1 every 37th query, 2 every query (test sizes), 0 off */
    int32_t shell_bound;      /* radial shell bound per (row block, column stage) in the passes that have upper bounds: 1 (default) / 0 */
    int32_t split_sweep;      /* final pass of the rotated format as two kernels -- the coarse sweep appends the tiles it keeps to a list, a second
                               * kernel finishes them: 1 (default) / 0 (one fused kernel, round 3) */
    int32_t kept_cap;         /* capacity of that list in tiles: 0 default (16 M); a pass that keeps more is repeated on the fused kernel (tests: force it) */
    int32_t auto_dense;       /* 1 (default): when the bounds can separate (almost) nothing -- >= 90 % of the (row block, leaf) lower bounds are zero:
                               * descriptors without cluster structure -- pass 0 computes everything and the final pass finds an empty schedule, decided on
                               * the device (lgr_match_last_lbstats reports the counts).  0: never */
    int32_t irregular_rows;   /* 1 (default): the few finite rows whose three 11-bin block sums differ from the consensus of the sets (FPFH: an all-zero row of an
                               * isolated point among rows whose blocks sum to 100) are kept out of the MFMA filter -- one of them would cost both sets the
                               * rotated 30-coordinate format -- and matched by an exact side scan instead (lgr_match_last_irregular reports the counts; at
                               * most 1024 per side, else they stay in the filter as before).  0: never */
} lgr_match_options;

/* ---- context ---- */
int  lgr_version(void);
/* device: HIP ordinal.  stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream; NULL is HIP's null
 * stream, which is what torch uses by default) or LGR_STREAM_OWN -> the ctx creates and owns a non-blocking stream */
#define LGR_STREAM_OWN ((void*) (intptr_t) -1)
int  lgr_ctx_create(int device, void* stream, lgr_ctx** out);
int  lgr_ctx_destroy(lgr_ctx* ctx);
int  lgr_ctx_sync(lgr_ctx* ctx);
const char* lgr_last_error(lgr_ctx* ctx);
void lgr_default_params(lgr_params* p);                      /* defaults of src/common.cpp:216-223,335-413 */
/* on-device stage timers of the last lgr_align*/
int  lgr_ctx_stage_ms(lgr_ctx* ctx, float* out12);
void lgr_match_default_options(lgr_match_options* opt);
/* opt == NULL restores the defaults.  Applies to every later matcher call of this context, stand-alone or inside lgr_align*. */
int  lgr_ctx_set_match_options(lgr_ctx* ctx, const lgr_match_options* opt);
int  lgr_ctx_get_match_options(lgr_ctx* ctx, lgr_match_options* opt);
/* device bytes the context's workspace currently holds (the sum of its grown-on-demand buffers): what a caller sizes its own
 * HBM budget against when it pushes many pairs of different sizes through one context (src/main.cpp:384-407 loops pairs in
 * one process) */
int  lgr_ctx_workspace_bytes(lgr_ctx* ctx, uint64_t* bytes);
void lgr_ctx_default_options(lgr_ctx_options* opt);
/* opt == NULL restores the defaults.  Waits for the context's queued work; call it between alignments, not during one. */
int  lgr_ctx_set_options(lgr_ctx* ctx, const lgr_ctx_options* opt);
int  lgr_ctx_get_options(lgr_ctx* ctx, lgr_ctx_options* opt);
/* host threads this context drives the device from: 1 (the caller's) + the helper threads it has started so far (at most 2) */
int  lgr_ctx_host_threads(lgr_ctx* ctx, int* n);

/* ---- building block under every grid / voxel / placement step (the reference has no counterpart: its containers are hash maps and
 *      kd-trees): stable LSD radix sort of (key, 32-bit value) pairs on the context's stream, out of place (in != out, input kept).
 *      u32: key bits [begin_bit, end_bit).  u64: bit ranges (shift, width), least significant first; bits outside the ranges must be
 *      equal in all keys.  Exported for tests and for callers that build their own orderings on the device. ---- */
int lgr_sort_pairs_u32_dev(lgr_ctx*, const uint32_t* d_keys_in, uint32_t* d_keys_out, const int32_t* d_vals_in, int32_t* d_vals_out,
                           size_t n, int begin_bit, int end_bit);
int lgr_sort_pairs_u64_dev(lgr_ctx*, const uint64_t* d_keys_in, uint64_t* d_keys_out, const int32_t* d_vals_in, int32_t* d_vals_out,
                           size_t n, const int* shifts, const int* widths, int n_ranges);

/* ---- include/common.h:266-280 calculateBoundingBox ---- */
int lgr_bbox_dev(lgr_ctx*, const float* d_pts, int n, float* d_min3_max3 /* 6 floats */);

/* ---- loader preprocessing: the steps of loadPointClouds (src/common.cpp:429-470) after the PLY reader:
 *      filterDuplicatePoints (:417-427), intensity = 1, voxel grid at 2 x calculatePointCloudDensity (:453-456,
 *      include/common.h:288), estimateNormalsPoints(30).  out holds n points, out != pts.  vp3 NULL -> origin.
 *      order (host entry): LGR_ORDER_REFERENCE reproduces the libstdc++ unordered_set / unordered_map output order
 *      (lgr_preprocess_order_dev below). ---- */
int lgr_preprocess(lgr_ctx*, const float* pts, int n, const float* vp3, int normals_available, int order, float* out, int* n_out, float* voxel_out);
int lgr_preprocess_dev(lgr_ctx*, const float* d_pts, int n, const float* vp3 /* host */, int normals_available, float* d_out, int* n_out /* host */,
                       float* voxel_out /* host, or NULL */);
/* src/common.cpp:417-427 filterDuplicatePoints (first occurrence of every exact xyz, input order; intensity := 1 as :446-451) */
int lgr_dedupe_dev(lgr_ctx*, const float* d_pts, int n, float* d_out, int* n_out /* host */);
/* src/common.cpp:202-208 calculatePointCloudDensity(pcd, quantile) */
int lgr_cloud_density_dev(lgr_ctx*, const float* d_pts, int n, float quantile, float* out /* host */);

/* ---- include/common.h:304-310 detectKeyPoints(pcd, parameters, iss_radius) with keypoint_id = iss
 *      (src/common.cpp:657-691: pcl::ISSKeypoint3D, salient = non-max radius = iss_radius, thresholds 0.975,
 *      min_neighbors 4; the reference passes gamma/min_neighbors as constants, they are arguments here).
 *      idx must hold n entries; ascending point indices. ---- */
int lgr_iss_keypoints(lgr_ctx*, const float* pts, int n, float radius, float gamma21, float gamma32, int min_neighbors,
                      int32_t* idx, int* n_out);
int lgr_iss_keypoints_dev(lgr_ctx*, const float* d_pts, int n, float radius, float gamma21, float gamma32, int min_neighbors,
                          int32_t* d_idx, int* n_out /* host */);

/* ---- include/downsample.h:32 downsamplePointCloud(pcd, pcd_down, voxel_size)  (src/downsample.cpp:5-41) ----
 * out may alias the input (the reference passes the same cloud, src/common.cpp:455-456).  n_out <= n.
 * order: LGR_ORDER_REFERENCE reproduces the libstdc++ unordered_map iteration order (on the device: lgr_downsample_order_dev),
 *        LGR_ORDER_CANONICAL = voxels sorted by (iz,iy,ix). */
int lgr_downsample(lgr_ctx*, const float* pts, int n, float voxel, int order, float* out, int* n_out);
int lgr_downsample_dev(lgr_ctx*, const float* d_pts, int n, float voxel, float* d_out, int* n_out /* host */);

/* ---- the reference's point ORDER on the device ----
 * The reference numbers its points by the iteration order of two libstdc++ hash containers: the std::unordered_set of
 * filterDuplicatePoints (src/common.cpp:417-427, after reserve(n)) and the std::unordered_map of downsamplePointCloud
 * (src/downsample.cpp:20,32-34); every index it writes afterwards (correspondence CSVs, extracted point ids, inlier lists) is in that
 * order.  csrc/lgr_stdhash.h states the rule (bucket schedule from the runtime's rehash policy object, per bucket count one sort by
 * (earliest time of the bucket descending, time descending)) and the two hashes; csrc/lgr_hash_order.hip runs it as kernels.
 *
 * lgr_hash_order_dev: the elements of a container are its distinct keys, numbered 0..n-1 by first insertion, d_hash[e] the hash code of
 * element e; d_order (n entries) receives the element ids in iteration order.  reserve: 0 (the container grew by itself) or the argument
 * of a reserve() before the first insertion, >= n; anything else is LGR_ERR_INVALID_ARG.  n == 0: LGR_OK, nothing written.  Asynchronous,
 * no host synchronisation, no allocation beyond the context's workspace. */
int lgr_hash_order_dev(lgr_ctx*, const uint64_t* d_hash, int n, long long reserve, int32_t* d_order);
/* lgr_downsample_dev with the output order as an argument: LGR_ORDER_CANONICAL gives its bytes, LGR_ORDER_REFERENCE the voxels in the map's
 * iteration order (elements = the voxels by first input index; invalid points are skipped as there).  d_out may alias d_pts. */
int lgr_downsample_order_dev(lgr_ctx*, const float* d_pts, int n, float voxel, int order, float* d_out, int* n_out /* host */);
/* lgr_dedupe_dev likewise: LGR_ORDER_REFERENCE is the set's iteration order under reserve(n) (points with a NaN coordinate never compare
 * equal and are all kept; the first occurrence's payload is kept, intensity := 1).  d_out != d_pts. */
int lgr_dedupe_order_dev(lgr_ctx*, const float* d_pts, int n, int order, float* d_out, int* n_out /* host */);
/* lgr_preprocess_dev likewise, the whole loader chain on the device: duplicates out in set order, density, the voxel grid over THAT order
 * (so every voxel accumulates in it), map order, normals.  What lgr_preprocess (host entry) runs. */
int lgr_preprocess_order_dev(lgr_ctx*, const float* d_pts, int n, const float* vp3 /* host */, int normals_available, int order, float* d_out,
                             int* n_out /* host */, float* voxel_out /* host, or NULL */);
/* Guard for a host whose libstdc++ orders differently: n voxel keys drawn on the host (coordinates in [0, spread), generator seeded with
 * seed) go through a real std::unordered_map (reserve(reserve) first when reserve > 0; 0 or >= n) and through lgr_hash_order_dev;
 * *mismatches = positions at which the device order, or the host restatement of the rule, differs from the container's iteration order,
 * plus elements whose restated hash differs from the library's.  Must be 0. */
int lgr_selfcheck_hash_order(lgr_ctx*, int n, int spread, uint64_t seed, long long reserve, long long* mismatches);

/* ---- src/common.cpp:644-655 estimateNormalsPoints(k, pcd, surface, vp, normals_available) ----
 * writes normal_x/y/z + curvature of pts in place; surf NULL -> pts is its own surface; vp NULL -> origin */
int lgr_normals_knn(lgr_ctx*, float* pts, int n, const float* surf, int ns, int k, const float* vp3, int normals_available);
int lgr_normals_knn_dev(lgr_ctx*, float* d_pts, int n, const float* d_surf, int ns, int k, const float* vp3 /* host */, int normals_available);

/* ---- include/common.h:322-332 estimateFeatures<FPFH>(kps, surface, features, radius, params) ----
 * LGR_ERR_UNSUPPORTED for radius > 1e18 (the weighting kernel's reciprocal is checked for squared distances up to 1e36) and for
 * more than 2^32 / 48 - 2 surface points (32-bit row offsets into the SPFH table). */
int lgr_fpfh(lgr_ctx*, const float* kps, int m, const float* surf, int n, float radius, float* out_m_x_33);
int lgr_fpfh_dev(lgr_ctx*, const float* d_kps, int m, const float* d_surf, int n, float radius, float* d_out);
/* ---- SHOT352 (include/common.h estimateFeatures<SHOT>: pcl::SHOTEstimationOMP<PointXYZINormal, PointXYZINormal, SHOT352> with
 *      pcl::SHOTLocalReferenceFrameEstimation at the same radius on the same surface) ----
 * lrf rows: 9 floats per key point, x, y, z axes (pcl::ReferenceFrame); NaN rows where no frame exists (fewer than 5 neighbours that
 * differ from the key point, a non-finite key point).  shot rows: 352 floats (pcl::SHOT352::descriptor); NaN rows for a NaN frame,
 * fewer than 5 neighbours (the key point itself counted) or a non-finite key point.  lrf == NULL: the frames are estimated, else
 * the given frames are used; out_lrf (optional) receives the frames used.  Neighbours in ascending (squared distance, index) order,
 * the eigen-decomposition and acos / atan2 are the canonical ones of DESIGN.md section 4 (csrc/lgr_shot_math.h). */
int lgr_shot_lrf(lgr_ctx*, const float* kps, int m, const float* surf, int n, float radius, float* out_m_x_9);
int lgr_shot_lrf_dev(lgr_ctx*, const float* d_kps, int m, const float* d_surf, int n, float radius, float* d_out_m_x_9);
int lgr_shot(lgr_ctx*, const float* kps, int m, const float* surf, int n, float radius, const float* lrf_or_null,
             float* out_m_x_352, float* out_lrf_or_null);
int lgr_shot_dev(lgr_ctx*, const float* d_kps, int m, const float* d_surf, int n, float radius, const float* d_lrf_or_null,
                 float* d_out_m_x_352, float* d_out_lrf_or_null);
/* ---- gravity frames (src/common.cpp:693-755 estimateReferenceFrames with lrf_id "gravity", g = (0, 0, 1)) ----
 * z = the key point's normal (floats 4..6 of its row).  acos(|clamp(z . g, -1, 1)|) > 0.04 (RF_MIN_ANGLE_RAD): y = g x z, x = y x z
 * (not normalized); otherwise -- a near-vertical or NaN normal -- the SHOT frame of lgr_shot_lrf on the same surface and radius
 * (NaN where that has none).  9 floats per key point as lgr_shot_lrf.  The dot and cross products follow DESIGN.md section 4. */
int lgr_gravity_lrf(lgr_ctx*, const float* kps, int m, const float* surf, int n, float radius, float* out_m_x_9);
int lgr_gravity_lrf_dev(lgr_ctx*, const float* d_kps, int m, const float* d_surf, int n, float radius, float* d_out_m_x_9);
/* ---- RoPS135 on given frames (include/common.h estimateFeatures<RoPS135> after estimateReferenceFrames:
 *      ROPSEstimationWithLocalReferenceFrames, include/pcl/impl/rops_custom_lrf.hpp:96-186 and :364-518; 5 bins, 3 rotations,
 *      support radius = radius) ----
 * The support is the surface points with squared distance < radius^2 (as lgr_shot), transformed by the frame (lrf: m x 9, required).
 * Per axis x, y, z and angle 22.5, 45, 67.5 degrees: the rotated support's box, then for the projections XY, XZ, YZ the 5 x 5
 * distribution matrix, its central moments (1,1), (2,1), (1,2), (2,2) and its entropy; the row divided by its L1 norm (unchanged
 * below FLT_EPSILON).  An empty support (or a non-finite key point) gives the zero row; one support point or a NaN frame gives the
 * zero row too (every point falls in cell (0, 0)).  logf, the bin index cast and Eigen's orders are those of DESIGN.md section 4
 * (csrc/lgr_rops_math.h). */
int lgr_rops(lgr_ctx*, const float* kps, int m, const float* surf, int n, float radius, const float* lrf, float* out_m_x_135);
int lgr_rops_dev(lgr_ctx*, const float* d_kps, int m, const float* d_surf, int n, float radius, const float* d_lrf, float* d_out_m_x_135);
/* Device self-check of the FPFH weighting kernel's reciprocal (v_rcp_f32 + one Newton step in place of the IEEE division sequence;
 * include/common.h:322-332 -> pcl::FPFHEstimation::weightPointSPFHSignature's 1.0f / dists[idx]): every float whose bit pattern lies in
 * [lo_bits, hi_bits] goes through both; out2[0] = values where they differ (must be 0 on [1e-36, 1e36], the range the kernel uses it on),
 * out2[1] = values tested. */
int lgr_selfcheck_rcp(lgr_ctx*, unsigned lo_bits, unsigned hi_bits, unsigned long long* out2);
/* the named libm's float routines as the device evaluates them (csrc/lgr_libm.cuh: GNU libc 2.35's acosf / atanf / atan2f / sinf / cosf restated op
 * for op), element-wise on host arrays: fn 0 acosf(a), 1 atanf(a), 2 atan2f(a, b), 3 sinf(a), 4 cosf(a) (sinf / cosf: |a| < 120).  A host
 * can compare them with its own libm (tests/test_gpu_pcl_arith.py compares with the oracle's restatement, which is pinned against glibc). */
int lgr_selfcheck_libm(lgr_ctx*, int fn, const float* a, const float* b, long long n, float* out);
/* fn 5: expf(a) (glibc 2.35's e_expf.c as its FMA build computes it, csrc/lgr_weights_math.h: every float, subnormal and zero results
 * included), fn 6: logf(a) for finite a > 0 (e_logf.c, csrc/lgr_rops_math.h) -- the two the point weights of weighted_closest_plane use. */

/* ---- include/matching.h:373-376 matchBF<FPFH>(query, train, params), randomness = 1 ----
 * idx[i] = matched train row or -1 (invalid / NaN query), dist[i] = L2 distance (sqrt) */
int lgr_match_bf(lgr_ctx*, const float* q33, int mq, const float* t33, int mt, int block, int32_t* idx, float* dist);
int lgr_match_bf_dev(lgr_ctx*, const float* d_q33, int mq, const float* d_t33, int mt, int block, int32_t* d_idx, float* d_dist);
/* both directions in one MFMA pass (what LeftToRight/Cluster matchers need, include/matching.h:431-432,495-496) */
int lgr_match_bf2_dev(lgr_ctx*, const float* d_a33, int ma, const float* d_b33, int mb, int block,
                      int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist);
/* ---- include/matching.h:373-376 matchBF<SHOT>(query, train, params): the contract of lgr_match_bf on M x 352 rows (OpenCV 4.5.1's
 *      normL2Sqr lane order for n = 352: 22 blocks of 16, no tail; ties: the later bf block, then the lower index; NaN rows never
 *      match).  The result is defined by the exact dense scan on the canonical distances; lgr_ctx_set_dense_filter chooses between that
 *      scan and an MFMA filter that runs the same selection on a proven superset of the rows it depends on: the same bytes either way. ---- */
int lgr_match_shot(lgr_ctx*, const float* q352, int mq, const float* t352, int mt, int block, int32_t* idx, float* dist);
int lgr_match_shot_dev(lgr_ctx*, const float* d_q352, int mq, const float* d_t352, int mt, int block, int32_t* d_idx, float* d_dist);
/* both directions from one pass over the (a, b) distances */
int lgr_match2_shot_dev(lgr_ctx*, const float* d_a352, int ma, const float* d_b352, int mb, int block,
                        int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist);
/* ---- include/matching.h:373-376 matchBF<RoPS135>(query, train, params): the contract of lgr_match_shot on M x 135 rows (OpenCV 4.5.1's
 *      normL2Sqr for n = 135: 8 blocks of 16 in the lane order of lgr_match_shot, then d2 += t * t over elements 128..134 in order) ---- */
int lgr_match_rops(lgr_ctx*, const float* q135, int mq, const float* t135, int mt, int block, int32_t* idx, float* dist);
int lgr_match_rops_dev(lgr_ctx*, const float* d_q135, int mq, const float* d_t135, int mt, int block, int32_t* d_idx, float* d_dist);
int lgr_match2_rops_dev(lgr_ctx*, const float* d_a135, int ma, const float* d_b135, int mb, int block,
                        int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist);
/* How the six entry points above, and SHOT / RoPS matching at randomness 1 inside lgr_correspondences* / lgr_align* / prepared and
 * multi-scale calls, sweep their rows; never what they return.  mode: -1 auto (filtered from the measured crossover size), 0 exact scan,
 * 1 filtered at any size.  self_check: 0 / 1 (test sizes): on the device, every pair of regular rows against the proven bound of the
 * filter and every query's candidates against an exact scan; a violation fails the call with LGR_ERR_HIP.  Values outside these:
 * LGR_ERR_INVALID_ARG, the setting unchanged.  lgr_ctx_set_knn_filter and the k-nearest / ratio paths are independent of this switch.
 * ABI: additions only (these four entry points); no struct changed, lgr_version() stays 5. */
int lgr_ctx_set_dense_filter(lgr_ctx*, int mode, int self_check);
int lgr_ctx_get_dense_filter(lgr_ctx*, int* mode, int* self_check);
/* last one-match call of this context on 135 / 352-float rows: the slots of lgr_match_knn_last -- [0] 1 filtered / 0 exact scan, [1] (query,
 * train) pairs whose canonical distance was computed, [2] query rows answered from candidates, [3] query rows answered by the exact scan,
 * [4] train rows offered to every query, [5] per-row candidate capacity, [6] self-check violations (~0 = not run), [7] reason code when
 * [0] == 0 under mode 1 (1: more than 1024 finite rows the operands cannot carry, 2: more than half of a direction's rows on the fallback
 * scan, 3: an empty side) */
int lgr_match_dense_last(lgr_ctx*, unsigned long long* out8);
int lgr_match_dense_last_check(lgr_ctx*, double* worst_ratio /* max |f - d2| / e over checked pairs, -1 = not run */);
/* ---- include/matching.h:612-625 matchBF with randomness = k > 1, on rows of row_len 33 (FPFH), 135 (RoPS135) or 352 (SHOT), other
 *      lengths and k outside 1..LGR_RANDOMNESS_MAX: LGR_ERR_UNSUPPORTED.  idx / dist are m x k: row i holds query i's matches in list
 *      order, then -1 / 0.f.  The distances are those of lgr_match_bf / lgr_match_rops / lgr_match_shot.  Per bf block
 *      cv::batchDistance's K-list: the first min(k, entries) rows in ascending (distance, index); the blocks' lists, ascending, go
 *      entry by entry through updateMultivaluedCorrespondence (src/common.cpp:517-529: insert in front of the first entry whose
 *      distance is not smaller, truncate to k), which leaves the first k of their union in (distance ascending, index DESCENDING)
 *      (DESIGN.md section 4).  k = 1 is the one-match entry points' result.  Every row length: an exact dense scan, or --
 *      lgr_ctx_set_knn_filter -- an MFMA filter (f32 operands for 33 floats, f16-split operands for 135 and 352) that offers every query
 *      a proven superset of the rows its list depends on and runs the same selection on the canonical distances of those rows only: the
 *      same bytes either way. ---- */
int lgr_match_knn(lgr_ctx*, int row_len, const float* q, int mq, const float* t, int mt, int block, int k, int32_t* idx, float* dist);
int lgr_match_knn_dev(lgr_ctx*, int row_len, const float* d_q, int mq, const float* d_t, int mt, int block, int k, int32_t* d_idx, float* d_dist);
/* both directions; the rows are packed once, each direction sweeps the distances itself */
int lgr_match_knn2_dev(lgr_ctx*, int row_len, const float* d_a, int ma, const float* d_b, int mb, int block, int k,
                       int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist);
/* How lgr_match_knn* / lgr_match_ratio* and randomness > 1 / matching ratio inside lgr_correspondences* / lgr_align* / prepared and
 * multi-scale calls sweep rows of 33, 135 and 352 floats; never what they return.  mode: -1 auto (filtered from the measured crossover size), 0 exact scan (the path of
 * revision 5), 1 filtered at any size.  self_check: 0 / 1 (test sizes): on the device, every pair of regular rows against the proven
 * bound of the filter and every query's candidates against an exact scan; a violation fails the call with LGR_ERR_HIP.  Values outside
 * these: LGR_ERR_INVALID_ARG.  Every row length honours the mode, each with its own measured crossover; lgr_ctx_set_dense_filter and the
 * one-match entry points are independent of this switch.
 * ABI: additions only (these four entry points); no struct changed, lgr_version() stays 5. */
int lgr_ctx_set_knn_filter(lgr_ctx*, int mode, int self_check);
int lgr_ctx_get_knn_filter(lgr_ctx*, int* mode, int* self_check);
/* last k-nearest call of this context, of any row length (every call writes all slots, an exact scan too: [0] = 0, [1] = all pairs,
 * [3] = all rows): [0] 1 filtered / 0 exact scan, [1] (query, train) pairs whose canonical distance
 * was computed, [2] query rows answered from candidates, [3] query rows answered by the fallback scan, [4] train rows offered to every
 * query, [5] per-row candidate capacity, [6] self-check violations (~0 = not run), [7] reason code when [0] == 0 under mode 1
 * (1: more than 1024 rows the operands cannot carry, 2: more than half of a direction's rows on the fallback scan, 3: an empty side) */
int lgr_match_knn_last(lgr_ctx*, unsigned long long* out8);
int lgr_match_knn_last_check(lgr_ctx*, double* worst_ratio /* max |a - d2| / e over checked pairs, -1 = not run */);
/* ---- include/matching.h:327-352 the vote among a query's candidates: cand_idx / cand_dist are mq x width (1..64), entries < 0 are
 *      skipped, an entry >= mt returns LGR_ERR_INVALID_ARG (the call synchronises to report it); train_pts: mt rows of 12 floats.
 *      cnt(m1) = float sum over m2 >= m1, in list order, of r / max(dl, r) where dl = sqrtf((dx*dx + dy*dy) + dz*dz) < 32 * r,
 *      r = iss_radius (finite, > 0); the largest cnt wins, then the smaller distance, strict compares from {0, 0}.
 *      idx[i] / dist[i] = the winner's entry, or -1 / 0.f. ---- */
int lgr_vote_matches(lgr_ctx*, const int32_t* cand_idx, const float* cand_dist, int mq, int width, const float* train_pts, int mt,
                     float iss_radius, int32_t* idx, float* dist);
int lgr_vote_matches_dev(lgr_ctx*, const int32_t* d_cand_idx, const float* d_cand_dist, int mq, int width, const float* d_train_pts, int mt,
                         float iss_radius, int32_t* d_idx, float* d_dist);
/* ---- include/matching.h:470-473 RatioMatcher::match_impl is a TODO in the reference; DESIGN.md section 4 states what is built: Lowe's
 *      ratio test on a query's list of lgr_match_knn*.  knn_idx / knn_dist are mq x k, a row in list order, then -1 / 0.f.  idx[i] /
 *      dist[i] = the row's first entry iff the row has k entries and dist[first] * threshold < dist[k-th] (one f32 multiply, a strict
 *      compare: equal distances never pass, a list shorter than k is dropped), else -1 / 0.f.  k outside 2..LGR_RANDOMNESS_MAX:
 *      LGR_ERR_UNSUPPORTED; a threshold that is not finite and > 0: LGR_ERR_INVALID_ARG.  mq = 0 writes nothing. ---- */
int lgr_ratio_test(lgr_ctx*, const int32_t* knn_idx, const float* knn_dist, int mq, int k, float threshold, int32_t* idx, float* dist);
int lgr_ratio_test_dev(lgr_ctx*, const int32_t* d_knn_idx, const float* d_knn_dist, int mq, int k, float threshold, int32_t* d_idx, float* d_dist);
/* the fused form: lgr_match_knn_dev's sweep of one direction with the test where its lists are decoded (the mq x k table is never
 * written).  Bit-equal to lgr_match_knn_dev followed by lgr_ratio_test_dev; idx / dist hold mq entries.  Arguments as lgr_match_knn*. */
int lgr_match_ratio(lgr_ctx*, int row_len, const float* q, int mq, const float* t, int mt, int block, int k, float threshold, int32_t* idx, float* dist);
int lgr_match_ratio_dev(lgr_ctx*, int row_len, const float* d_q, int mq, const float* d_t, int mt, int block, int k, float threshold,
                        int32_t* d_idx, float* d_dist);
/* ---- include/matching.h:373-376 matchFLANN<FPFH>(query_features, train_features, parameters), randomness 1 (:565-592):
 *      pcl::KdTreeFLANN is an exact search, so the nearest row is the one matchBF finds (the reference's own test asserts that,
 *      tests/flann_bf_matcher.h:82-83); what differs is the reported distance: sqrt of FLANN's L2_Simple (sequential sum of
 *      squares) instead of OpenCV's lane-ordered norm.  idx = -1 for invalid query rows. ---- */
int lgr_match_flann(lgr_ctx*, const float* q33, int mq, const float* t33, int mt, int32_t* idx, float* dist);
int lgr_match_flann_dev(lgr_ctx*, const float* d_q33, int mq, const float* d_t33, int mt, int32_t* d_idx, float* d_dist);
/* ---- include/matching.h:383-387 matchLocal<FPFH>(query_pcd, train_tree, query_features, train_features, parameters, guess)
 *      (:637-678): for every valid query row, the train row with the nearest descriptor (pcl::L2_Norm: sequential sum, sqrtf)
 *      among the train POINTS within match_search_radius of guess * query point (strict d2 < r*r; FLT_MAX radius = all points);
 *      equal descriptor distances: the spatially nearer point, then the lower index (KNNResult keeps the first, radiusSearch
 *      visits by ascending distance).  guess16: column-major, host. ---- */
int lgr_match_local(lgr_ctx*, const float* query_pts, int mq, const float* train_pts, int mt, const float* q33, const float* t33,
                    const float guess16[16], float match_search_radius, int32_t* idx, float* dist);
int lgr_match_local_dev(lgr_ctx*, const float* d_query_pts, int mq, const float* d_train_pts, int mt, const float* d_q33, const float* d_t33,
                        const float guess16[16] /* host */, float match_search_radius, int32_t* d_idx, float* d_dist);
/* ---- matchLocal<FeatureT> with parameters.randomness = k (:637-678, KNNResult :44-94) on rows of row_len 33 (FPFH), 135 (RoPS135) or
 *      352 (SHOT: the descriptor floats without the frame, as lgr_match_shot takes them); other lengths and k outside
 *      1..LGR_RANDOMNESS_MAX: LGR_ERR_UNSUPPORTED.  The moved query point is x*c0 + (y*c1 + (z*c2 + c3)) per coordinate.  A query row is
 *      valid when all row_len floats are finite; a non-finite moved point has no candidates; a candidate is a finite train point whose
 *      s = ((dx*dx + dy*dy) + dz*dz) to the moved point satisfies strict s < r*r and whose row is all finite.  Descriptor distance:
 *      pcl::L2_Norm -- sum = 0; for j ascending: d = q[j] - t[j]; sum += d*d (no contraction); sqrtf.  idx / dist are mq x k: row i
 *      holds the first k candidates in ascending (distance, s, train index), then -1 / 0.f (KNNResult puts a later equal distance
 *      behind an earlier one, radiusSearch visits by ascending spatial distance, the index stands for FLANN's unspecified order).
 *      A radius whose square is not finite (FLT_MAX): every finite train point with a finite s; radius 0: no candidate.  NULL pointers
 *      with non-zero counts, negative counts, a negative or NaN radius: LGR_ERR_INVALID_ARG, before any work.  mq = 0 writes nothing,
 *      mt = 0 fills -1 / 0.f.  (row_len 33, k 1) equals lgr_match_local* bit for bit.  guess16: column-major, host. ---- */
int lgr_match_local_knn(lgr_ctx*, int row_len, const float* query_pts, int mq, const float* train_pts, int mt, const float* q, const float* t,
                        const float guess16[16], float match_search_radius, int k, int32_t* idx /* mq x k */, float* dist /* mq x k */);
int lgr_match_local_knn_dev(lgr_ctx*, int row_len, const float* d_query_pts, int mq, const float* d_train_pts, int mt, const float* d_q, const float* d_t,
                            const float guess16[16] /* host */, float match_search_radius, int k, int32_t* d_idx, float* d_dist);
/* ---- matchFLANN<FeatureT>, randomness 1 (:562-592), on rows of row_len 33, 135 or 352 (others: LGR_ERR_UNSUPPORTED): lgr_match_flann's
 *      declared choice for every row length.  idx[i] = the row lgr_match_bf / lgr_match_rops / lgr_match_shot finds with a single train
 *      block (the argmin under OpenCV's lane order, the lowest index at equal distance); dist[i] = sqrtf of the sequential sum above
 *      (FLANN's L2_Simple); -1 / 0.f for an invalid query.  mq = 0 writes nothing, mt = 0 fills -1 / 0.f.  (33) equals lgr_match_flann*
 *      bit for bit.  randomness > 1 under FLANN is not built: the reference leaves its tie order unspecified. ---- */
int lgr_match_flann_rows(lgr_ctx*, int row_len, const float* q, int mq, const float* t, int mt, int32_t* idx, float* dist);
int lgr_match_flann_rows_dev(lgr_ctx*, int row_len, const float* d_q, int mq, const float* d_t, int mt, int32_t* d_idx, float* d_dist);

/* diagnostics of the context's last match call (stand-alone or inside lgr_align*), kept in the context:
 * [items_ab, dense_ab, items_ba, dense_ba, sub_cols, rg_rows] and the duration of
 * its MFMA filter kernel (hipEvents on the ctx stream) -- what bench.py's roofline object is computed from */
int lgr_match_last_stats(lgr_ctx*, unsigned* out6);
int lgr_match_last_kernel_ms(lgr_ctx*, float* ms);
/* fraction of the (256-row block x 128-column stage) tiles the MFMA passes of the last match call computed; the exact
 * bound-based skipping leaves the rest out.  1.0 = dense.  Every (row block, stage) counts once, so the figure is
 * never above 1; lgr_match_last_issued sums the passes (a stage that straddles two leaves may be computed by two passes): the work
 * that was issued, >= the executed fraction. */
int lgr_match_last_work(lgr_ctx*, double* executed_fraction);
int lgr_match_last_issued(lgr_ctx*, double* out2 /* [0] issued fraction, [1] issued (row, column) element pairs of the padded operands */);
/* coarse rejection inside the MFMA filter kernel (rotated format only; lgr_match_options.coarse_rejection = 0 turns it off): 32 x 32 tiles
 * tested after their first two MFMA steps in the last match call, and tiles abandoned there. */
int lgr_match_last_coarse(lgr_ctx*, double* out2);
/* shell test inside the same sweep (lgr_match_options.shell_bound): 32 x 32 tiles of the swept stages a wave left out before any MFMA step,
 * because the radial shells of its rows and of the tile's columns about their cluster centre are farther apart than every upper bound */
int lgr_match_last_shell(lgr_ctx*, double* tiles_skipped);
/* exact rerank (f16 operand formats; lgr_match_options.rerank_refilter = 0 turns it off): (query, train row) pairs the MFMA re-filter of
 * the candidate groups passed on to the exact distance in the last match call, query->train and train->query direction; a
 * count above the pair buffer (8 per candidate group) means that direction fell back to the exact scan of whole groups. */
int lgr_match_last_pairs(lgr_ctx*, unsigned* out2);
/* MFMA operand format of the last match call: 1 = two-term f16 splits on v_mfma_f32_32x32x16_f16, K = 112; 2 = the same on
 * 30 Helmert coordinates, K = 96 (chosen when every 11-bin block of all rows has the same sum, as FPFH rows do); 0 = f32
 * operands on v_mfma_f32_32x32x2_f32 (lgr_match_options.operand_format selects one explicitly).  Results do not depend on it. */
int lgr_match_last_format(lgr_ctx*, int* f16);
/* (row block, leaf) pairs whose lower bound is zero / finite in the last pruned match call (lgr_match_options.auto_dense) */
int lgr_match_last_lbstats(lgr_ctx*, double* out2);
/* irregular rows of the last match call (lgr_match_options.irregular_rows): [0] query side, [1] train side: rows that were matched by the
 * exact side scan instead of the MFMA filter (0 when the lane was off, found no consensus among the block sums, or gave up); [2] = 1 when it
 * gave up (more than 1024 such rows on a side: the call was rebuilt with every finite row in the filter). */
int lgr_match_last_irregular(lgr_ctx*, unsigned* out3);
/* self-check of the matcher's filter bound (lgr_match_options.self_check = 1 or 2, test sizes): worst |filtered - exact| / eps over
 * sampled table entries of the last match call, rows then columns; -1 = not run.  Must be <= 1. */
int lgr_match_last_check(lgr_ctx*, double* out2);
/* what that check covered, rows [0..3] then columns [4..7]: entries checked, entries whose upper side was tested, entries whose upper
 * side was waived (the exact minimum lies above the coarse rejection's U^2), entries with a row that counts as computed only through the
 * per-stage column criterion (columns; 0 for rows).  ~0 (-1) = not run: all eight, or a direction's four when it was not matched. */
int lgr_match_last_check_cover(lgr_ctx*, unsigned long long* out8);
/* the same option also packs the MFMA operands a second time with the reference packing kernel and compares on the device, bit for bit:
 * out2[0] = pieces compared (16-byte pieces of fragments and norms, tile shells) over the call's packing launches, out2[1] = pieces that
 * differed (any: the call fails).  ~0 (-1) = not run (self_check off, or the f32 operand format). */
int lgr_match_last_pack_check(lgr_ctx*, unsigned long long* out2);
/* ---- src/common.cpp:531-547 calculateSmoothedDensities(pcd, k) / :202-208 calculatePointCloudDensity ---- */
int lgr_smoothed_densities(lgr_ctx*, const float* pts, int n, int k, float* out);
int lgr_smoothed_densities_dev(lgr_ctx*, const float* d_pts, int n, int k, float* d_out);
int lgr_knn_dev(lgr_ctx*, const float* d_q, int nq, const float* d_pts, int n, int k, int32_t* d_idx, float* d_d2);

/* ---- include/matching.h:395-411 / 428-453 / 492-550 match_impl of OneSided / LeftToRight / Cluster matcher.  LGR_MATCH_RATIO is
 *      LGR_MATCH_ONE_SIDED over the table it is given (the ratio test has already dropped entries: ij_idx < 0 is skipped) ---- */
int lgr_filter_dev(lgr_ctx*, int matching_id, const float* d_src, int ns, const float* d_tgt, int nt,
                   const int32_t* d_ij_idx, const float* d_ij_dist, const int32_t* d_ji_idx, const float* d_ji_dist,
                   float distance_thr, int cluster_k, lgr_corr* d_out, int* n_out /* host */);

/* ---- include/correspondence_search.h:14-28 FeatureBasedCorrespondenceSearch::calculateCorrespondences (keypoint any) ---- */
int lgr_correspondences(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_params*, lgr_corr* out, int* n_out);
int lgr_correspondences_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params*, lgr_corr* d_out, int* n_out /* host */);

/* ---- the descriptor of the correspondence search (AlignmentParameters.descriptor_id / lrf_id, include/common.h:148) ----
 * A struct of its own so that lgr_params keeps its revision-5 layout.  NULL = FPFH: lgr_correspondences_ex*(..., NULL) and
 * lgr_align_ex*(..., NULL) are lgr_correspondences* and lgr_align*.  SHOT is built for the brute-force matcher only: SHOT with
 * use_bfmatcher = 0, with has_guess, or on a context whose arithmetic is LGR_ARITH_PCL returns LGR_ERR_UNSUPPORTED (the
 * arithmetic modes differ in the FPFH weighting only and mean nothing for SHOT; the SHOT stage has one arithmetic).  lrf_id
 * matters to SHOT and RoPS only (FPFH never reads it, as in the reference).  SHOT: LGR_LRF_DEFAULT is built, the reference's
 * 'gravity' and 'gt' frames (src/common.cpp:693-755) return LGR_ERR_UNSUPPORTED, other values LGR_ERR_INVALID_ARG.
 * RoPS (LGR_DESCRIPTOR_ROPS, include/common.h estimateFeatures<RoPS135>): LGR_LRF_GRAVITY is built (lgr_gravity_lrf, then lgr_rops,
 * per call and per scale level, on key points whose normals are first re-estimated on the level's surface as include/matching.h:243-246
 * does); LGR_LRF_DEFAULT returns LGR_ERR_UNSUPPORTED (the reference triangulates the cloud with
 * GreedyProjectionTriangulation for it), LGR_LRF_GT too (this struct has no ground-truth channel), other values
 * LGR_ERR_INVALID_ARG; use_bfmatcher = 0, has_guess and LGR_ARITH_PCL are refused as for SHOT.
 * lgr_result.stage_ms[2] ("fpfh") carries the descriptor stage, whichever descriptor ran (for RoPS: frames and rows).
 * matching_id = LGR_MATCH_RATIO (every descriptor; lgr_correspondences*, lgr_align*, lgr_measure*): only source -> target is matched;
 * per level the candidate of lgr_match_ratio_dev(bf_block_size, ratio_k, LGR_MATCHING_RATIO_THRESHOLD), the levels' candidates through
 * the vote of the multi-scale path, then the one-sided output.  It needs randomness = 1 and the brute-force matcher without a guess,
 * else LGR_ERR_UNSUPPORTED, checked before any stage runs. */
enum { LGR_DESCRIPTOR_FPFH = 0, LGR_DESCRIPTOR_SHOT = 1, LGR_DESCRIPTOR_ROPS = 2 };
enum { LGR_LRF_DEFAULT = 0, LGR_LRF_GRAVITY = 1, LGR_LRF_GT = 2 };   /* SHOT: default only; RoPS: gravity only */
typedef struct {
    int32_t descriptor_id;   /* LGR_DESCRIPTOR_FPFH / LGR_DESCRIPTOR_SHOT / LGR_DESCRIPTOR_ROPS */
    int32_t lrf_id;          /* LGR_LRF_DEFAULT (SHOT) / LGR_LRF_GRAVITY (RoPS) */
    int32_t ratio_k;         /* LGR_MATCH_RATIO only (AlignmentParameters::ratio_k, include/common.h:146): the list length of the ratio test,
                                2..LGR_RANDOMNESS_MAX; 0 = 2 (MATCHING_RATIO_K, include/common.h:51); anything else LGR_ERR_UNSUPPORTED.
                                The first of the former reserved words; other matchers do not read it.  A NULL struct means 2. */
    int32_t reserved[5];     /* 0 */
} lgr_feature_params;
void lgr_default_feature_params(lgr_feature_params* f);      /* FPFH, default frames */
int lgr_correspondences_ex(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_params*, const lgr_feature_params*,
                           lgr_corr* out, int* n_out);
int lgr_correspondences_ex_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params*, const lgr_feature_params*,
                               lgr_corr* d_out, int* n_out /* host */);

/* ---- include/sac_prerejective_omp.h:21-56 SampleConsensusPrerejectiveOMP(src,tgt,corrs,params).align() ----
 * final_mask (optional): c bytes, inlier mask of the refit transform */
int lgr_ransac(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
               const lgr_params*, lgr_result*, uint8_t* final_mask);
int lgr_ransac_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                   const lgr_params*, lgr_result* /* host */, uint8_t* d_final_mask);
/* replay mode (SURVEY section 7 "RANSAC RNG"): evaluate n caller-supplied sample tuples (params.n_samples correspondence indices each) */
int lgr_ransac_replay_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                          const lgr_params*, const int32_t* d_triples, int n,
                          uint8_t* d_ok, float* d_T16, int32_t* d_n_inliers, float* d_metric);
/* the on-device sampler alone: triples of iterations [first, first+n) (Philox4x32-10 + selectCorrespondences :33-77) */
int lgr_ransac_samples_dev(lgr_ctx*, uint64_t seed, int first, int n, int n_corr, int32_t* d_triples);
/* ... for any n_samples in 3..8: draw j of an iteration is word j % 4 of Philox(key = seed, counter = (iteration, j / 4, 0, 0)) >> 1 */
int lgr_ransac_samples_n_dev(lgr_ctx*, uint64_t seed, int first, int n, int n_corr, int n_samples, int32_t* d_tuples);
/* one Philox4x32-10 block from the device's generator (the sampler above uses counter = (iteration, 0, 0, 0), key = seed; the closest-plane
 * metric's subsets the full counter): key = (k0 | k1 << 32).  For Random123's known-answer vectors. */
int lgr_selfcheck_philox(lgr_ctx*, uint64_t key, const uint32_t counter4[4], uint32_t out4[4]);
/* src/metric.cpp:125-179 buildInliersAndEstimateMetric for one transform */
int lgr_evaluate_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                     const float T16[16] /* host */, int metric_id, int score_id,
                     uint8_t* d_mask, int* n_inliers, float* rmse, float* metric /* host outs */);

/* ---- ClosestPlaneMetricEstimator::buildInliersAndEstimateMetric (src/metric.cpp:10-53,181-199) of one transform on the
 *      sparse 1 % subset RANSAC uses (src/sac_prerejective_omp.cpp:109); the subset of hypothesis `counter` is defined by
 *      Philox.  threshold = calculatePointCloudDensity(tgt).  pairs (optional, 2 ints per inlier, room for
 *      0.01 * ns pairs): (source index, nearest target index), ascending source index.  In lgr_ransac / lgr_align:
 *      params.metric_id = LGR_METRIC_CLOSEST_PLANE or LGR_METRIC_COMBINATION. ---- */
int lgr_evaluate_plane_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16] /* host */, int score_id,
                           uint64_t seed, uint32_t counter, int* n_inliers, float* rmse, float* metric, float* threshold /* or NULL */,
                           int32_t* pairs /* host, or NULL */, int* n_pairs);

/* ---- weighted_closest_plane (WeightedClosestPlaneMetricEstimator, src/metric.cpp:202-231) and its point weights (src/weights.cpp) ----
 * The metric is closest_plane's (same sparse subset, inliers, rmse and final block) with the score of an inlier multiplied in f32 by the
 * weight of its source point, and metric = score / (0.01 * weights_sum), in double, weights_sum = the sequential f32 sum of all source
 * weights in index order.  The weights are computed once per source cloud, with k = 30 neighbours (the reference's NORMAL_NR_POINTS
 * macro, not lgr_params.normal_nr_points).  weight_id in the order of src/common.cpp:49-55; harris and tomasi return
 * LGR_ERR_UNSUPPORTED, other unknown ids LGR_ERR_INVALID_ARG.  nss counts into 251 bins.
 * lgr_ransac* / lgr_align* with metric_id = LGR_METRIC_WEIGHTED_CLOSEST_PLANE use constant weights (the reference's default
 * weight_id); the _ex / _ex2 entries take lgr_metric_params (NULL: the defaults).  Plane metrics always run on the launch chain. */
enum { LGR_WEIGHT_CONSTANT = 0, LGR_WEIGHT_EXP_CURVATURE = 1, LGR_WEIGHT_CURVEDNESS = 2, LGR_WEIGHT_HARRIS = 3, LGR_WEIGHT_TOMASI = 4,
       LGR_WEIGHT_CURVATURE = 5, LGR_WEIGHT_NSS = 6 };
typedef struct {
    int32_t weight_id;       /* LGR_WEIGHT_* (ignored when weights != NULL) */
    int32_t reserved[5];     /* 0 */
    const float* weights;    /* NULL, or ns caller-supplied finite per-source-point weights used instead of weight_id: a host pointer for the
                              * host entries, a device pointer for the _dev entries */
} lgr_metric_params;
void lgr_default_metric_params(lgr_metric_params* m);   /* constant weights */
int lgr_ransac_ex(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                  const lgr_params*, const lgr_metric_params*, lgr_result*, uint8_t* final_mask);
int lgr_ransac_ex_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                      const lgr_params*, const lgr_metric_params*, lgr_result* /* host */, uint8_t* d_final_mask);
/* the plane metrics' early-out gate in the last lgr_ransac* call of this context (closest_plane, combination, weighted_closest_plane; 0, 0
 * after any other metric): out2[0] hypotheses scored on their sparse plane subset, out2[1] those of them abandoned part-way through it
 * because they could be neither the best nor a record.  Which ones are abandoned may differ between runs; the results never do. */
int lgr_ransac_last_plane_gate(lgr_ctx*, unsigned* out2);
/* the weight map of weight_id (out: n floats) and, when weights_sum != NULL, its sequential f32 sum.  nr_points: the neighbours of the
 * principal curvatures (exp_curvature, curvedness; 1..128, more returns LGR_ERR_UNSUPPORTED); the other maps ignore it. */
int lgr_weights(lgr_ctx*, const float* pts, int n, int weight_id, int nr_points, float* out, float* weights_sum /* or NULL */);
int lgr_weights_dev(lgr_ctx*, const float* d_pts, int n, int weight_id, int nr_points, float* d_out, float* weights_sum /* host, or NULL */);
/* pcl::PrincipalCurvaturesEstimation over the k nearest neighbours of each point in the cloud itself ((distance, index) order, the
 * point included; fewer when the cloud has fewer than k points): pc1 >= pc2, NaN for a non-finite point */
int lgr_principal_curvatures(lgr_ctx*, const float* pts, int n, int k, float* pc1, float* pc2);
int lgr_principal_curvatures_dev(lgr_ctx*, const float* d_pts, int n, int k, float* d_pc1, float* d_pc2);
/* lgr_evaluate_plane_dev under weighted_closest_plane: d_weights = ns device floats, weights_sum = the metric's denominator */
int lgr_evaluate_plane_weighted_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16] /* host */, int score_id,
                                    uint64_t seed, uint32_t counter, const float* d_weights, float weights_sum,
                                    int* n_inliers, float* rmse, float* metric, float* threshold /* or NULL */,
                                    int32_t* pairs /* host, or NULL */, int* n_pairs);

/* ---- include/transformation.h:6-7 estimateOptimalRigidTransformation(src, tgt, inliers, T) ---- */
int lgr_refit_svd(lgr_ctx*, const float* src, const float* tgt, int ns, int nt, const lgr_corr* inliers, int n, float T16[16]);
int lgr_refit_svd_dev(lgr_ctx*, const float* d_src, const float* d_tgt, const lgr_corr* d_corr, int c,
                      const uint8_t* d_mask /* NULL: all */, float T16[16] /* host */);

/* ---- include/alignment.h:18-19 alignPointClouds(src, tgt, params) (src/alignment.cpp:72-109, no CSV side effects);
 *      alignRansac (:14-19) is lgr_ransac; alignGror (:21-35) via params.alignment_id ---- */
int lgr_align(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_params*, lgr_result*);
int lgr_align_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params*, lgr_result* /* host */);

/* lgr_align with the descriptor of lgr_feature_params (NULL: FPFH, i.e. lgr_align) */
int lgr_align_ex(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_params*, const lgr_feature_params*, lgr_result*);
int lgr_align_ex_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params*, const lgr_feature_params*,
                     lgr_result* /* host */);

/* lgr_align_ex with the metric parameters of weighted_closest_plane (NULL: the defaults, i.e. lgr_align_ex) */
int lgr_align_ex2(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_params*, const lgr_feature_params*,
                  const lgr_metric_params*, lgr_result*);
int lgr_align_ex2_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params*, const lgr_feature_params*,
                      const lgr_metric_params*, lgr_result* /* host */);

/* ---- alignGror(src, tgt, correspondences, parameters) (src/alignment.cpp:21-35) =
 *      pcl::registration::GRORInitialAlignment::computeTransformation (include/gror/ia_gror.hpp:367-415) with
 *      setResolution(distance_thr), setOptimalSelectionNumber(800).  Result: transformation, iterations = 1,
 *      converged = 1 (as alignGror reports), n_inliers = inliers of the refinement (:261-293), metric = size of the
 *      maximum consistent set (best_count_), best_iteration = rows that reached the tight-constraint stage,
 *      estimated_iters = K.  inlier_mask (c bytes) optional.  Tie orders of the three std::sort calls: DESIGN.md. ---- */
int lgr_gror(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
             float resolution, int k_optimal, lgr_result* res, uint8_t* inlier_mask /* host, or NULL */);
int lgr_gror_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                 float resolution, int k_optimal, lgr_result* res /* host */, uint8_t* d_inlier_mask /* or NULL */);
/* node degrees of optimalSelectionBasedOnNodeReliability (include/gror/ia_gror.hpp:126-170), c int32 on the device */
int lgr_gror_node_degree_dev(lgr_ctx*, const float* d_src, const float* d_tgt, const lgr_corr* d_corr, int c,
                             float resolution, int32_t* d_degree);

/* ---- alignTeaser(src, tgt, correspondences, parameters) (src/alignment.cpp:37-69).  The reference throws ("Not implemented: support
 *      TEASER", :40); its commented-out body (:41-69) fixes the estimator's parameters, and the statement computed here is this
 *      project's own ("TEASER"): the k_select correspondences of highest GROR node degree, their compatibility
 *      graph, its maximum core, a greedy clique in it, the rotation by GNC-TLS over the clique's open chain of TIMs, the shift by
 *      per-axis TLS over the clique's members.  No scale estimation (:50).
 *      lgr_params.alignment_id has no value for it: lgr_align* / lgr_measure* keep returning LGR_ERR_UNSUPPORTED for "teaser". ---- */
enum { LGR_TEASER_NODES_MAX = 2048 };
typedef struct {
    float   noise_bound;               /* beta = distance_thr (:48); finite, in (0, 1e18], else LGR_ERR_INVALID_ARG (cbar2 = 1, :49) */
    int32_t k_select;                  /* nodes kept: 0 = 1024, else 3..LGR_TEASER_NODES_MAX; anything else LGR_ERR_UNSUPPORTED */
    int32_t rotation_max_iterations;   /* 100 (:53); 1..1000, else LGR_ERR_INVALID_ARG */
    float   rotation_gnc_factor;       /* 1.4 (:54); finite and > 1, else LGR_ERR_INVALID_ARG */
    float   rotation_cost_threshold;   /* 0.005 (:55); finite and >= 0, else LGR_ERR_INVALID_ARG */
    int32_t reserved[3];
} lgr_teaser_params;
typedef struct {
    int32_t valid;                     /* 1: a clique of >= 3 nodes was found and the transform is a solution */
    int32_t n_nodes;                   /* K = min(c, k_select) */
    int32_t max_core, n_core;          /* K* and |V*| */
    int32_t n_clique;
    int32_t rotation_iterations;       /* SVD solves */
    int32_t n_rotation_inliers;        /* TIMs with weight >= 0.5 */
    int32_t n_translation_inliers;     /* clique members inside all three axes' consensus sets */
    float   rotation_cost;             /* the last GNC cost formed (0: the loop stopped at mu <= 0) */
    float   translation_cost[3];       /* the TLS cost of each axis's shift */
    int32_t reserved[4];
} lgr_teaser_info;
/* the reference's commented values (:48-55) with noise_bound = distance_thr */
void lgr_default_teaser_params(lgr_teaser_params*, float distance_thr);
/* Result: transformation (the identity without a solution), iterations = rotation_iterations, converged = valid, n_inliers = set bytes
 * of the mask (|T_i - (R S_i + t)| <= beta on every axis, over all c), metric = n_clique, best_iteration = K*, estimated_iters = K,
 * n_correspondences = c, time_te, stage_ms[0..5] = nodes, adjacency, clique, rotation, translation, mask.  c < 3: LGR_OK, no solution,
 * nothing is read from the correspondences.  An index outside its cloud: LGR_ERR_INVALID_ARG (checked on the device, reported with
 * the call's one read-back).  clique (optional): 2 * LGR_TEASER_NODES_MAX int32 -- [0, n_clique) the clique's correspondence indices
 * in node order, [LGR_TEASER_NODES_MAX, + n_nodes) the nodes' (degree descending, index ascending), every other entry -1.
 * inlier_mask (optional): c bytes. */
int lgr_teaser(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c, const lgr_teaser_params*,
               lgr_result* res, lgr_teaser_info* info /* or NULL */, int32_t* clique /* host, or NULL */, uint8_t* inlier_mask /* host, or NULL */);
int lgr_teaser_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c, const lgr_teaser_params*,
                   lgr_result* res /* host */, lgr_teaser_info* info /* host, or NULL */, int32_t* d_clique /* or NULL */,
                   uint8_t* d_inlier_mask /* or NULL */);

/* ---- include/hypotheses.h:10-16 (host bookkeeping; compiled out in the reference, SAVE_MULTIPLE_HYPOTHESES false) ---- */
/* include/hypotheses.h:14-16 chooseBestHypothesis(src, tgt, correspondences, params, tns) (src/hypotheses.cpp:50-129), the
 * decision only: the hypothesis with the largest inlier uniformity (identity / index -1 when none is positive) */
int lgr_choose_best_hypothesis_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                                   const float* tns16 /* host, n x 16 */, int n, float T_out16[16], int* best_index, float* uniformities /* host, n, or NULL */);
int lgr_update_hypotheses(float* tns16, float* metrics, int n, int cap, const float* new_T16, float new_metric, float distance_thr);
/* host twin of lgr_choose_best_hypothesis_dev: clouds and correspondences in host memory */
int lgr_choose_best_hypothesis(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                               const float* tns16 /* n x 16 */, int n, float T_out16[16], int* best_index, float* uniformities /* n, or NULL */);

/* ---- the loop with SAVE_MULTIPLE_HYPOTHESES set (src/sac_prerejective_omp.cpp:11): the set of distinct hypotheses ----
 * The fold alone: src/hypotheses.cpp:14-48 updateHypotheses applied to n (transform, metric) items in the caller's order, starting from
 * the empty set (the reference's call sites src/sac_prerejective_omp.cpp:143, :230, :261 fold the loop's hypotheses one by one).
 * Returns the members in set order: their transforms (column-major, the items' own 16 floats), metrics and positions in the item list.
 * 1 <= max_set <= LGR_HYPOTHESES_MAX, anything else is LGR_ERR_INVALID_ARG; a set that outgrows max_set at the end of any step is
 * LGR_ERR_UNSUPPORTED (never a truncated set).  Transforms are read as R|t: an item's fourth row does not enter a decision. */
#define LGR_HYPOTHESES_MAX 2048
int lgr_fold_hypotheses_dev(lgr_ctx*, const float* d_tns16 /* n x 16 */, const float* d_metrics, int n, float distance_thr, int max_set,
                            float* d_set_tns16 /* max_set x 16 */, float* d_set_metrics, int32_t* d_set_index, int* n_out /* host */);
int lgr_fold_hypotheses(lgr_ctx*, const float* tns16, const float* metrics, int n, float distance_thr, int max_set,
                        float* set_tns16, float* set_metrics, int32_t* set_index, int* n_out);

/* One member of the set after the final block (src/sac_prerejective_omp.cpp:270-291 per member) */
typedef struct {
    float   loop_transformation[16];   /* column-major, as the loop produced it (the guess: as given) */
    float   transformation[16];        /* after the refit over its inliers (:282) */
    int32_t iteration;                 /* the iteration that produced it; -1: the guess (:139-143) */
    float   loop_metric, metric;       /* in the loop (:230) / of the refit (:290) */
    int32_t n_inliers, converged;      /* of the refit / enough inliers and a metric above the estimator's minimum (:277-281) */
    float   uniformity;                /* chooseBestHypothesis' criterion of the refit (src/hypotheses.cpp:50-129) */
} lgr_hypothesis;

/* SampleConsensusPrerejectiveOMP::align with SAVE_MULTIPLE_HYPOTHESES: the loop of lgr_ransac_dev, every accepted hypothesis folded
 * through updateHypotheses with params->distance_thr (:143 the guess, which passes no inlier gate; :230 / :261 every iteration that
 * survives prerejection with >= MIN_NR_INLIERS inliers), the final block on every member (:270-291) and chooseBestHypothesis over the
 * refit transforms (:293).  Declared order: one stream, the guess first, then the iterations ascending (the
 * reference folds per OpenMP thread and merges the threads' sets in thread order).
 * res: iterations, num_rejections, estimated_iters, best_iteration and best_metric_before_refit are lgr_ransac_dev's on the same input;
 * converged = any member converged; transformation, n_inliers and metric are the chosen member's (identity, 0, 0 when none has a
 * positive uniformity: *best_index = -1).  out receives *n_out <= max_set members in set order.
 * Metrics uniformity and correspondences; the plane metrics, combination and alignment_id = gror return LGR_ERR_UNSUPPORTED, and so does
 * a set that outgrows max_set (1 <= max_set <= LGR_HYPOTHESES_MAX, else LGR_ERR_INVALID_ARG).  c < n_samples: LGR_OK, empty set,
 * identity, as lgr_ransac_ex_dev.  Always driven as a chain of launches (lgr_ctx_options.ransac_schedule does not apply). */
int lgr_ransac_multi_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                         const lgr_params*, int max_set, lgr_result* res, lgr_hypothesis* out /* host, max_set */, int* n_out, int* best_index);
int lgr_ransac_multi(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                     const lgr_params*, int max_set, lgr_result* res, lgr_hypothesis* out, int* n_out, int* best_index);
/* lgr_ransac_multi* for all five metrics, with the metric parameters of weighted_closest_plane where lgr_ransac_ex* takes them (NULL: the
 * defaults; read under that metric only, harris and tomasi LGR_ERR_UNSUPPORTED before any work; host weights for the host entry, device
 * weights for the _dev one).  uniformity / correspondences: lgr_ransac_multi*'s bytes.  Under a plane metric the fields of a member mean
 * what lgr_result's mean after lgr_ransac_ex*: n_inliers = plane inliers (closest_plane, weighted_closest_plane) or correspondence inliers
 * (combination), loop_metric / metric = the estimator's metric; an item of the fold is an iteration that survives prerejection with >=
 * MIN_NR_INLIERS of those inliers, scored on the sparse subset its iteration keys (never abandoned part-way: the second pass runs without
 * the loop's gate), the guess is scored under counter 0xFFFFFFFD, and the final block of a member is lgr_ransac_ex_dev's (counters
 * 0xFFFFFFFE / 0xFFFFFFFF, the refit over the plane pairs in ascending source index or, combination, over the correspondence inliers),
 * run on the device for every member with one read-back for all.  lgr_ransac_last_plane_gate reports the loop's numbers.  alignment_id =
 * gror stays LGR_ERR_UNSUPPORTED. */
int lgr_ransac_multi_ex_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                            const lgr_params*, const lgr_metric_params*, int max_set, lgr_result* res, lgr_hypothesis* out /* host, max_set */,
                            int* n_out, int* best_index);
int lgr_ransac_multi_ex(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c,
                        const lgr_params*, const lgr_metric_params*, int max_set, lgr_result* res, lgr_hypothesis* out, int* n_out, int* best_index);

/* ---- include/analysis.h:36-98 AlignmentAnalysis::start(transformation_gt, testname) (src/analysis.cpp:218-246): a transformation judged
 *      against a known ground truth.  What the reference leaves unordered (OpenMP reductions, kd-tree ties) has the declared orders of
 *      points move in PCL's se3 order, "nearest within r" is the closest-plane metric's rule (strict d2 < r * r,
 *      smallest squared distance, then the lowest index; non-finite points never match), every float sum over points is the sequential
 *      f32 sum in ascending index over per-point terms.  No file side effects (AlignmentAnalysis::save is the caller's business:
 *      tools/register_ply.py --ground-truth).  Point rows must be 16-byte aligned.  0 < distance_thr <= 1e18, so that the squared search
 *      radius (2 distance_thr)^2 and the grid cell stay finite in f32; anything else is LGR_ERR_INVALID_ARG. ---- */
typedef struct {
    float   r_err, t_err;                /* src/analysis.cpp:19-24 calculateRotationAndTranslationDifferences (radians, length) */
    float   pcd_err;                     /* :30-43 calculatePointCloudRmse; NaN for an empty source */
    float   overlap_rmse;                /* :45-88 calculateOverlapRmse; quiet NaN when overlap_size == 0 */
    int32_t overlap_size;
    float   normal_diff;                 /* :141-185 calculateNormalDifference (radians; pi when nothing counts) */
    int32_t n_normal_overlap;
    int32_t n_overlap_src, n_overlap_tgt, n_overlap;   /* src/common.cpp:558-591 mergeOverlaps at the ground truth; n_overlap = the sum */
    float   overlap;                     /* src/analysis.cpp:229 n_overlap / (float) (ns + nt) */
    float   overlap_area;                /* :230-234; NaN when either cloud of the ratio has fewer than 2 points */
    int32_t n_correspondences;           /* c */
    int32_t n_correct_correspondences;   /* :187-206 buildCorrectCorrespondences */
    int32_t n_inliers;                   /* set bytes of the inlier mask (0 without one) */
    int32_t n_correct_inliers;           /* mask && correct: buildCorrectInliers' test for the correspondence metrics (src/metric.cpp) */
    float   corr_uniformity;             /* :90-130 over the correct correspondences; 0 when there is none (the reference divides 0 by 0) */
    int32_t converged;                   /* as passed in */
    int32_t converged_and_overlap_ok;    /* converged && overlap_rmse < distance_thr (src/main.cpp:356; NaN compares false) */
    int32_t reserved[5];                 /* 0 */
} lgr_gt_eval;
/* inlier_mask (optional): c bytes, e.g. final_mask of lgr_ransac*.  correct_mask (optional): receives c bytes, 1 = correct correspondence.
 * ns == 0 or nt == 0 is not an error: counts 0, overlap_rmse NaN, normal_diff pi. */
int lgr_evaluate_gt(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c, const float T16[16],
                    const float Tgt16[16], float distance_thr, int converged, const uint8_t* inlier_mask_or_null, lgr_gt_eval* out,
                    uint8_t* correct_mask_or_null);
int lgr_evaluate_gt_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c, const float T16[16] /* host */,
                        const float Tgt16[16] /* host */, float distance_thr, int converged, const uint8_t* d_inlier_mask_or_null,
                        lgr_gt_eval* out /* host */, uint8_t* d_correct_mask_or_null);
/* n transforms judged against ONE ground truth: out[s] is, field for field and bit for bit, what lgr_evaluate_gt_dev returns for
 * (T16s + 16 s, converged[s], inlier mask s) -- NaN and empty-cloud conventions and the declared orders included.  What
 * AlignmentAnalysis::start computes from the ground truth alone runs once per call: the target's grid, the overlap set of
 * calculateOverlapRmse (found at the ground truth, src/analysis.cpp:69-76: only the last distance, :77, uses the estimate), the correct
 * correspondences and their uniformity, the normal difference and mergeOverlaps.  The transforms are taken LGR_GT_BATCH_CHUNK to a
 * launch.  T16s: n x 16 column-major; d_inlier_masks: n x c bytes, mask s at offset s * c; the correct mask (c bytes) is the same for
 * every member.  n == 0: LGR_OK, nothing written; n > LGR_GT_BATCH_MAX: LGR_ERR_UNSUPPORTED; otherwise the checks of lgr_evaluate_gt_dev. */
enum { LGR_GT_BATCH_MAX = 64, LGR_GT_BATCH_CHUNK = 8 };
int lgr_evaluate_gt_batch(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c, const float* T16s /* n x 16 */, int n,
                          const float Tgt16[16], float distance_thr, const int32_t* converged /* n */, const uint8_t* inlier_masks_or_null /* n x c */,
                          lgr_gt_eval* out /* n */, uint8_t* correct_mask_or_null /* c */);
int lgr_evaluate_gt_batch_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                              const float* T16s /* host, n x 16 */, int n, const float Tgt16[16] /* host */, float distance_thr,
                              const int32_t* converged /* host, n */, const uint8_t* d_inlier_masks_or_null /* n x c bytes */,
                              lgr_gt_eval* out /* host, n */, uint8_t* d_correct_mask_or_null /* c bytes */);

/* ---- the `measure` test type (measureTestResults, src/main.cpp:312-382): n_times alignments of one pair that differ in the RANSAC
 *      seed only, each judged against the ground truth, and the test_measurements.csv row over them.  The correspondence search does
 *      not depend on the seed and runs once; the runs are lgr_ransac_ex_dev with fix_seed = 0 and seed = seeds[i] (seeds == NULL:
 *      params->seed + i; the reference's std::random_device seeding is the caller's business); all runs are judged by one
 *      lgr_evaluate_gt_batch_dev call with distance_thr = params->distance_thr and each run's final inlier mask.
 *      runs[i].result is what lgr_align_ex2_dev returns for that seed, except time_cs and stage_ms[0..4]: the shared search's, the same
 *      in every run.  1 <= n_times <= LGR_GT_BATCH_MAX, else LGR_ERR_INVALID_ARG; alignment_id = gror has no seed: one run
 *      (src/main.cpp:350), out->n_times reports the runs made.  Whatever lgr_align_ex2_dev refuses is refused with its code before the
 *      search starts; after those checks a distance_thr outside (0, 1e18] is LGR_ERR_INVALID_ARG (the evaluation's bound).  Aggregates, on the host as the reference states them (src/main.cpp:345-380, include/utils.h:68-88): a run
 *      succeeds when eval.converged_and_overlap_ok; mae / sae, mte / ste and mrmse / srmse are mean and deviation of r_err, t_err and
 *      overlap_rmse over the successful runs in run order, mtime / stime of (float) (time_cs + time_te) over all runs; the mean is the
 *      sequential double sum from 0.0 divided by (float) size, the deviation std::sqrt of the sequential float sum of
 *      (x - mean) * (x - mean) divided by (float) size (the population form); an empty list gives quiet NaN for both. ---- */
typedef struct { uint64_t seed; lgr_result result; lgr_gt_eval eval; } lgr_measure_run;
typedef struct {
    int32_t n_times, n_success;
    float   success_rate, mae, sae, mte, ste, mrmse, srmse, mtime, stime;   /* the columns of src/main.cpp:324 */
    int32_t reserved[5];   /* 0 */
} lgr_measurement;
int lgr_measure(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_params*, const lgr_feature_params* /* or NULL */,
                const lgr_metric_params* /* or NULL */, const float Tgt16[16], const uint64_t* seeds_or_null, int n_times,
                lgr_measure_run* runs /* n_times */, lgr_measurement* out);
int lgr_measure_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_params*, const lgr_feature_params* /* or NULL */,
                    const lgr_metric_params* /* or NULL */, const float Tgt16[16] /* host */, const uint64_t* seeds_or_null /* host */, int n_times,
                    lgr_measure_run* runs /* host, n_times */, lgr_measurement* out /* host */);
/* the two aggregates alone, on host lists (include/utils.h:68-88 calculateMean / calculateStandardDeviation for float) */
float lgr_measure_mean(const float* x, int n);
float lgr_measure_deviation(const float* x, int n, float mean);

/* ---- prepared clouds: include/matching.h:132-146 Storage, filled once per cloud by FeatureBasedMatcherImpl::initialize (:164-262) ----
 * The correspondence search does everything up to the matcher per cloud: key points, the down-sampling chain, normals, descriptor rows
 * (one level under feature_radius > 0, the pruned level range otherwise) and the match filter's per-cloud tables.  lgr_cloud_prepare*
 * runs those stages once into an object that owns its device memory (hipMalloc; nothing of it lives in the context's workspace, so it
 * outlives any number of calls and may be used from any context of its device); lgr_correspondences_prepared* / lgr_align_prepared
 * start at the matcher.  A host that registers N scans pairwise prepares each scan once.
 *   - side (0 / 1) selects which of vp_* / has_vp_* / iss_radius_* of lgr_params the cloud is prepared with; the rest is read as in a pair
 *     call, and lgr_params is checked as lgr_correspondences_ex_dev checks it, with the same codes.
 *   - the object records what its state depends on: feature_nr_points, normal_nr_points, feature_radius (every value <= 0 counts as
 *     "unset"), scale_factor, normals_available, keypoint_id, the side's view point and ISS radius, cluster_k under LGR_MATCH_CLUSTER
 *     (0 otherwise: the other filters read the densities only), descriptor_id, lrf_id and the context's arithmetic; floats by their
 *     bits.  A pair call whose lgr_params (source-side fields for src, target-side fields for tgt) differ from that record returns
 *     LGR_ERR_INVALID_ARG; so do clouds of another device than the context's.  A cloud prepared as side 0 serves as a target when the
 *     fields agree.
 *   - the pair calls never write to a cloud: one cloud may appear in any number of pairs, on both sides, and as both arguments of a call.
 *   - lgr_correspondences_prepared* returns the bytes lgr_correspondences_ex* returns for the same clouds and parameters, and
 *     lgr_align_prepared the lgr_result of lgr_align_ex2* apart from the time fields; stage_ms[0..2] are 0 in a prepared call.  Whatever
 *     the unprepared entry points refuse is refused with the same code by lgr_cloud_prepare* or by the pair call.
 *   - a cloud of fewer than 2 points is a valid object: pairs with it have no correspondences, lgr_align_prepared gives the identity, not
 *     converged.
 * Getters: lgr_cloud_keypoints* gives the key points as indices into the cloud, lgr_cloud_level* one level's key-point list (indices into
 * the key points) and descriptor rows (rows x row_len).  The _dev forms hand out the object's own pointers, read-only and valid until
 * lgr_cloud_destroy; a NULL list means 0..count-1 (keypoint any; the one level of the single-scale form).  The host forms copy into caller
 * arrays (either may be NULL) and synchronise. */
typedef struct lgr_cloud lgr_cloud;
struct lgr_cloud_info {           /* a tag, not a typedef: the getter carries the same name (as stat(2) does) */
    int32_t  n, keypoints, row_len;
    int32_t  levels;              /* levels that hold rows: 1 in the single-scale form, 0 without key points or without two points */
    int32_t  first_log2_radius;   /* log2_radius of level 0 (levels follow in steps of 1) */
    int32_t  multiscale;          /* 1: prepared with feature_radius unset */
    uint64_t bytes;               /* device memory the object holds */
    int32_t  reserved[4];         /* 0 */
};
typedef struct {
    int32_t log2_radius;
    float   radius, voxel;        /* powf(scale_factor, log2_radius) and the voxel of include/matching.h:230-231 */
    int32_t rows, surface;        /* key points of the level; size of the level's down-sampled surface */
    int32_t reserved[3];          /* 0 */
} lgr_cloud_level_info;
int lgr_cloud_prepare(lgr_ctx*, const float* pts, int n, int side, const lgr_params*, const lgr_feature_params* /* or NULL */, lgr_cloud** out);
int lgr_cloud_prepare_dev(lgr_ctx*, const float* d_pts, int n, int side, const lgr_params*, const lgr_feature_params* /* or NULL */, lgr_cloud** out);
int lgr_cloud_destroy(lgr_cloud*);   /* NULL: LGR_OK */
int lgr_cloud_info(const lgr_cloud*, struct lgr_cloud_info* out);
int lgr_cloud_keypoints(const lgr_cloud*, int32_t* out_or_null /* keypoints */, int* m);
int lgr_cloud_keypoints_dev(const lgr_cloud*, const int32_t** d_idx /* NULL: 0..n-1 */, int* m);
int lgr_cloud_level(const lgr_cloud*, int level, lgr_cloud_level_info* info_or_null, int32_t* list_out_or_null, float* rows_out_or_null);
int lgr_cloud_level_dev(const lgr_cloud*, int level, lgr_cloud_level_info* info_or_null, const int32_t** d_list_or_null, const float** d_rows_or_null);
int lgr_correspondences_prepared(lgr_ctx*, const lgr_cloud* src, const lgr_cloud* tgt, const lgr_params*, const lgr_feature_params* /* or NULL */,
                                 lgr_corr* out, int* n_out);
int lgr_correspondences_prepared_dev(lgr_ctx*, const lgr_cloud* src, const lgr_cloud* tgt, const lgr_params*, const lgr_feature_params* /* or NULL */,
                                     lgr_corr* d_out, int* n_out /* host */);
int lgr_align_prepared(lgr_ctx*, const lgr_cloud* src, const lgr_cloud* tgt, const lgr_params*, const lgr_feature_params* /* or NULL */,
                       const lgr_metric_params* /* or NULL; weights: a DEVICE array */, lgr_result*);

/* src/analysis.cpp:45-88 calculateOverlapRmse (and :30-43 calculatePointCloudRmse, computed by the same pass; pcd_err may be NULL).
 * d_idx (optional, ns ints): the target point whose tangent plane source point i was measured against, -1 where the point was skipped. */
int lgr_overlap_rmse_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16] /* host */, const float Tgt16[16] /* host */,
                         float distance_thr, float* overlap_rmse, int* overlap_size, float* pcd_err /* host outs */, int32_t* d_idx_or_null);
int lgr_overlap_rmse(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float T16[16], const float Tgt16[16], float distance_thr,
                     float* overlap_rmse, int* overlap_size, float* pcd_err_or_null, int32_t* idx_or_null);   /* host twin */
/* src/common.cpp:558-591 mergeOverlaps(Tgt * src, tgt, dst, distance_thr) as two byte masks (optional: ns and nt bytes) + src/analysis.cpp:229-234:
 * n_overlap2 = {source points, target points} in the overlap, overlap, overlap_area (calculateSmoothedDensities with its default k = 2).
 * overlap_area may be NULL: the two density passes it costs are then not run.  dst of the reference = the source rows whose mask byte is
 * set (moved by Tgt), then the target rows whose byte is set, each in index order. */
int lgr_merge_overlaps_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float Tgt16[16] /* host */, float distance_thr,
                           uint8_t* d_mask_src_or_null, uint8_t* d_mask_tgt_or_null, int n_overlap2[2], float* overlap,
                           float* overlap_area_or_null /* host outs */);
int lgr_merge_overlaps(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float Tgt16[16], float distance_thr,
                       uint8_t* mask_src_or_null, uint8_t* mask_tgt_or_null, int n_overlap2[2], float* overlap,
                       float* overlap_area_or_null);   /* host twin */
/* src/analysis.cpp:187-206 buildCorrectCorrespondences alone: correct_mask (optional, c bytes), n3 = {correct correspondences, correct
 * inliers, inliers} (the last two 0 without an inlier mask).  Correspondence indices are checked against ns and nt. */
int lgr_correct_correspondences_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                                    const float Tgt16[16] /* host */, const uint8_t* d_inlier_mask_or_null, uint8_t* d_correct_mask_or_null,
                                    int n3[3] /* host */);
int lgr_correct_correspondences(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c, const float Tgt16[16],
                                const uint8_t* inlier_mask_or_null, uint8_t* correct_mask_or_null, int n3[3]);   /* host twin */
/* src/analysis.cpp:141-185 calculateNormalDifference (without checkNormals' assert): the element of rank n / 2 of the ascending differences */
int lgr_normal_difference_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float Tgt16[16] /* host */, float distance_thr,
                              float* normal_diff, int* n_normal_overlap /* host outs */);
int lgr_normal_difference(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float Tgt16[16], float distance_thr,
                          float* normal_diff, int* n_normal_overlap);   /* host twin */

/* ---- ClosestPlaneMetricEstimator / WeightedClosestPlaneMetricEstimator::buildInliersAndEstimateMetric in their DENSE form, sparse = false
 *      (src/metric.cpp:10-53,181-231 with calculateScore :55-81): every source point, in index order -- what AlignmentAnalysis::start
 *      evaluates a finished alignment with (src/analysis.cpp:211,223) and estimateTestMetric writes to metrics.csv (src/main.cpp:41-116).
 *      Per point the expressions are those of lgr_evaluate_plane_dev (the same point gets the same nearest target, distance and value
 *      from either); score and the squared-error sum are the reference's serial f32 loops in ascending source index.
 *      mp == NULL: closest_plane.  mp != NULL: weighted_closest_plane with the weights of mp (weight_id, or mp->weights: ns finite floats,
 *      a device pointer for the _dev entry, a host pointer for the host twin); harris / tomasi return LGR_ERR_UNSUPPORTED.
 *      inlier_threshold <= 0: calculatePointCloudDensity(tgt), as setTargetCloud does; > 0: used as given, so that a caller that evaluates
 *      several transforms against one target pays for the density once (out->threshold of the first call).  NaN or > 1e18: LGR_ERR_INVALID_ARG.
 *      ns == 0 or nt < 2: LGR_ERR_INVALID_ARG.  Point rows must be 16-byte aligned.
 *      d_inliers (optional, room for ns): the reference's `inliers` vector, {source index, nearest target index, dist, threshold} in
 *      ascending source index; out->n_inliers entries are written.  d_nn (optional, ns ints): the nearest target within 2 x threshold of
 *      every moved source point, -1 where there is none (or the moved point is not finite) -- whether or not the point is an inlier. ---- */
typedef struct {
    int32_t n_inliers;
    float   rmse;          /* sqrtf(sum dist^2 / n_inliers); FLT_MAX when there is no inlier (src/metric.cpp:49-52) */
    float   metric;        /* score / ns, or score / weights_sum with weights (src/metric.cpp:199,214): the division in double */
    float   threshold;     /* the inlier threshold used */
    float   score;         /* calculateScore's sum, before the division */
    int32_t reserved[3];   /* 0 */
} lgr_plane_dense_eval;
int lgr_evaluate_plane_dense_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16] /* host */, int score_id,
                                 const lgr_metric_params* mp_or_null, float inlier_threshold, lgr_plane_dense_eval* out /* host */,
                                 lgr_corr* d_inliers_or_null, int32_t* d_nn_or_null);
int lgr_evaluate_plane_dense(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float T16[16], int score_id,
                             const lgr_metric_params* mp_or_null, float inlier_threshold, lgr_plane_dense_eval* out,
                             lgr_corr* inliers_or_null, int32_t* nn_or_null);   /* host twin */

/* ---- the first statement of AlignmentAnalysis::start plus buildCorrectInliers (src/analysis.cpp:211,223-224, src/metric.cpp:83-101) for
 *      any metric_id: metric_estimator_->buildInliersAndEstimateMetric(T, inliers, rmse, metric, rand) with the DENSE estimator of
 *      getMetricEstimatorFromParameters(parameters, false), then the inliers that are correct under the ground truth.
 *        correspondences, uniformity       lgr_evaluate_dev; correct inliers = inlier mask && buildCorrectCorrespondences
 *        closest_plane, weighted_...       lgr_evaluate_plane_dense_dev (mp: the weights, NULL = constant); correct inliers =
 *                                          lgr_correct_correspondences_dev over the dense inlier list (each carries the plane threshold)
 *        combination                       inliers and rmse of the correspondence estimator (constant score: CombinationMetricEstimator
 *                                          default-constructs it); metric = metric_cs * metric_cp in f32, metric_cp the dense closest-plane
 *                                          metric under score_id (src/metric.cpp:239-250); correct inliers as for correspondences
 *      Tgt16 == NULL: no ground truth, n_correct_inliers = 0.
 *      inlier_mask (optional, c bytes): the inlier mask of the correspondence estimator (correspondences, uniformity, combination; not written
 *      under the plane metrics).  inliers (optional, room for ns): the dense inlier list of the plane metrics, n_inliers entries (not written
 *      under the other metrics). ---- */
typedef struct {
    float   metric, rmse;
    int32_t n_inliers, n_correct_inliers;
    int32_t reserved[4];   /* 0 */
} lgr_metric_eval;
int lgr_analysis_metric_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c, const float T16[16] /* host */,
                            const float* Tgt16_or_null /* host */, int metric_id, int score_id, const lgr_metric_params* mp_or_null,
                            lgr_metric_eval* out /* host */, uint8_t* d_inlier_mask_or_null, lgr_corr* d_inliers_or_null);
int lgr_analysis_metric(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c, const float T16[16],
                        const float* Tgt16_or_null, int metric_id, int score_id, const lgr_metric_params* mp_or_null, lgr_metric_eval* out,
                        uint8_t* inlier_mask_or_null, lgr_corr* inliers_or_null);   /* host twin */

/* ---- the `debug` command and the `compare` test type: generateDebugFiles, compareHypotheses and compareOverlaps (src/main.cpp:152-284)
 *      without their files.  Colours are 0x00RRGGBB in an int32, as setPointColor takes them (src/common.cpp:1149-1153).  Declared orders:
 *      DESIGN.md section 4.  Point rows must be 16-byte aligned; 0 < distance <= 1e18, anything else is LGR_ERR_INVALID_ARG; an empty
 *      cloud is not an error: counts are 0 and nothing is written. ---- */
#define LGR_COLOR_BEIGE    0xf8c471   /* include/common.h:26-34 */
#define LGR_COLOR_RED      0xff0000
#define LGR_COLOR_PARAKEET 0x03c04a
#define LGR_COLOR_BLUE     0x0000ff
#define LGR_COLOR_WHITE    0xffffff
/* per-point outputs of one temperature map, each NULL or an array of one entry per compared point (device memory for the _dev entries,
 * host memory for the host twins) */
typedef struct {
    float*   temp_distance;   /* TemperatureType::Distance: the plane distance, distance_max where there is no neighbour or it is not below */
    float*   temp_normal;     /* TemperatureType::NormalDifference: radians, (float) M_PI / 2 at most and where the distance one is at its maximum */
    int32_t* color_distance;  /* getColor(temp_distance, 0, distance_max) */
    int32_t* color_normal;    /* getColor(temp_normal, 0, (float) M_PI / 2) */
    int32_t* nn;              /* the reference point the temperatures were taken against, -1 when there is none within 2 distance_max */
} lgr_temperature_out;
/* src/common.cpp:859-906 calculateTemperatureMap(compared, reference, type, ...) for both types after ONE search (the reference searches
 * once per type and finds the same neighbour): nearest reference point within DIST_TO_PLANE_COEFFICIENT * distance_max under the rule of
 * lgr_merge_overlaps; dist_to_plane = |n_q . (q - p)|, the squared distance where that is not finite.  *n_below = temperatures < distance_max,
 * the rows the reference keeps for its *_distances_*.csv (src/common.cpp:932-937). */
int lgr_temperature_map_dev(lgr_ctx*, const float* d_compared, int n, const float* d_reference, int nr, float distance_max,
                            const lgr_temperature_out* out_or_null, int* n_below /* host */);
int lgr_temperature_map(lgr_ctx*, const float* compared, int n, const float* reference, int nr, float distance_max,
                        const lgr_temperature_out* out_or_null, int* n_below);   /* host twin */
/* src/common.cpp:908-963 saveTemperatureMaps(src, tgt, name, params, distance_thr, transformation) with normals available: the source moved
 * by T (pcl::transformPointCloudWithNormals), then one map per direction, source against target and target against the moved source.
 * moved_or_null: room for ns rows, receives the moved source (what the reference writes to its PLY files).  n_below2 = {source, target}. */
int lgr_temperature_maps_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float T16[16] /* host */, float distance_thr,
                             const lgr_temperature_out* src_out_or_null, const lgr_temperature_out* tgt_out_or_null, float* d_moved_or_null,
                             int n_below2[2] /* host */);
int lgr_temperature_maps(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float T16[16], float distance_thr,
                         const lgr_temperature_out* src_out_or_null, const lgr_temperature_out* tgt_out_or_null, float* moved_or_null,
                         int n_below2[2]);   /* host twin */
/* src/main.cpp:152-205 compareOverlaps for n transformations (the reference passes two: the found one and the ground truth): per
 * transformation the source moved by it, the moved source points whose NEAREST target (no radius) lies closer than distance_thr along that
 * target's normal, the target points likewise against the moved source; counts[k] = size of that overlap, weighted_counts[k] = sequential
 * f32 sum of the squared smoothed densities (k = 2) of the overlap cloud {moved source rows, then target rows, each in index order}; 0
 * where the overlap has fewer than 2 points (declared: calculateSmoothedDensities would rassert).  counts2 (optional, 2 n): {source,
 * target} points per transformation.  Masks (optional): n x ns and n x nt bytes.  A non-finite point is in no overlap. */
int lgr_compare_overlaps_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float* tns16 /* host, n x 16 */, int n,
                             float distance_thr, int32_t* counts /* host, n */, float* weighted_counts /* host, n */,
                             int32_t* counts2_or_null /* host */, uint8_t* d_mask_src_or_null, uint8_t* d_mask_tgt_or_null);
int lgr_compare_overlaps(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float* tns16, int n, float distance_thr,
                         int32_t* counts, float* weighted_counts, int32_t* counts2_or_null, uint8_t* mask_src_or_null,
                         uint8_t* mask_tgt_or_null);   /* host twin */
/* the search behind lgr_compare_overlaps: nearest point of d_pts for every query (rows of 12 floats both), under the order of lgr_knn_dev
 * with k = 1 (squared distance, then index), at a cost that does not depend on how far a query lies from the cloud.  -1 / +inf where the
 * query is not finite or the cloud has no finite point. */
int lgr_nearest_dev(lgr_ctx*, const float* d_q, int nq, const float* d_pts, int n, int32_t* d_idx, float* d_d2_or_null);
int lgr_nearest(lgr_ctx*, const float* q, int nq, const float* pts, int n, int32_t* idx, float* d2_or_null);   /* host twin */
/* src/common.cpp:818-835 getColor(v, vmin, vmax) per value */
int lgr_color_map_dev(lgr_ctx*, const float* d_values, int n, float vmin, float vmax, int32_t* d_colors);
int lgr_color_map(lgr_ctx*, const float* values, int n, float vmin, float vmax, int32_t* colors);   /* host twin */
/* src/common.cpp:837-850 saveColorizedWeights: getColor between quantile(0.01, weights) and quantile(0.99, weights) (include/utils.h:45-66);
 * range2 (optional) receives the two quantiles */
int lgr_color_weights_dev(lgr_ctx*, const float* d_weights, int n, int32_t* d_colors, float range2_or_null[2] /* host */);
int lgr_color_weights(lgr_ctx*, const float* weights, int n, int32_t* colors, float range2_or_null[2]);   /* host twin */
/* src/common.cpp:771-816 savePointCloudWithCorrespondences, the colours of its n points: parakeet with key points (beige without), key
 * points beige, the points of `corr` red, of `inliers` blue, then mixPointColor with white once per entry of `correct` that touches the
 * point (is_source: index_query, else index_match).  An index outside [0, n) is LGR_ERR_INVALID_ARG. */
int lgr_color_correspondences_dev(lgr_ctx*, int n, const int32_t* d_kp_idx_or_null, int n_kp, const lgr_corr* d_corr, int c,
                                  const lgr_corr* d_correct, int n_correct, const lgr_corr* d_inliers, int n_inliers, int is_source,
                                  int32_t* d_colors);
int lgr_color_correspondences(lgr_ctx*, int n, const int32_t* kp_idx_or_null, int n_kp, const lgr_corr* corr, int c, const lgr_corr* correct,
                              int n_correct, const lgr_corr* inliers, int n_inliers, int is_source, int32_t* colors);   /* host twin */

/* ---- iterated closest-plane refinement of a transform: the step of the reference's final block (src/sac_prerejective_omp.cpp:270-291 --
 *      closest-plane inliers of the transform, estimateOptimalRigidTransformation over those pairs, evaluation of the result) in its DENSE
 *      form, repeated while the metric rises.  Declared order:
 *        thr = params.threshold > 0 ? params.threshold : calculatePointCloudDensity(tgt)          (once)
 *        E = dense_eval(T0); T = T0; steps = 0                                                    (lgr_evaluate_plane_dense's values)
 *        while steps < max_steps:
 *            E.n_inliers < 3                   -> stop = NO_PAIRS
 *            T' = refit over E's inlier pairs (source i, nearest target of i), ascending i        (lgr_refit_svd's arithmetic)
 *            E' = dense_eval(T');  !(E'.metric > E.metric) -> stop = NO_GAIN, T stays             (a NaN or zero metric never wins)
 *            T, E = T', E'; steps += 1
 *        else stop = MAX_STEPS
 *      Every float of every evaluated transform equals that statement bit for bit.  mp == NULL: closest_plane; mp != NULL: the weighted
 *      estimator evaluates (harris / tomasi: LGR_ERR_UNSUPPORTED), the refit ignores weights as the reference's does.  An empty source is
 *      LGR_OK with steps = 0, stop = NO_PAIRS and T0 returned (metric 0, rmse FLT_MAX).  nt < 2, max_steps outside
 *      [0, LGR_REFINE_MAX_STEPS], score_id outside [0, 3], a NaN threshold or one above 1e18 and non-zero reserved words:
 *      LGR_ERR_INVALID_ARG, before any work.  Point rows must be 16-byte aligned.
 *      trace (optional, host, room for max_steps + 2 entries): every evaluated transform in order -- T0, each candidate, the rejected one
 *      last; *n_trace receives the number written (steps + 1, one more with a rejected candidate).
 *      The device path builds the target grid, the threshold and the weights once, then enqueues the steps in groups of LGR_REFINE_GROUP
 *      and reads one small record per group: the transform, the counts and the inlier flags never pass through the host. ---- */
#define LGR_REFINE_MAX_STEPS 1024
#define LGR_REFINE_GROUP 4
enum { LGR_REFINE_STOP_MAX_STEPS = 0, LGR_REFINE_STOP_NO_GAIN = 1, LGR_REFINE_STOP_NO_PAIRS = 2 };
typedef struct {
    int32_t score_id;      /* LGR_SCORE_* */
    int32_t max_steps;     /* 0 .. LGR_REFINE_MAX_STEPS */
    float   threshold;     /* <= 0: the target's density */
    int32_t reserved[5];   /* 0 */
} lgr_refine_params;
void lgr_default_refine_params(lgr_refine_params* p);   /* MSE score, 10 steps, threshold 0 */
typedef struct {
    float   transformation[16];   /* column-major */
    float   metric, rmse, score;  /* as lgr_plane_dense_eval */
    int32_t n_inliers;
} lgr_refine_step;
typedef struct {
    float   transformation[16];   /* the last accepted step (T0 when steps == 0) */
    float   metric, rmse, score;
    int32_t n_inliers;
    float   threshold;            /* the inlier threshold used */
    int32_t steps;                /* accepted steps */
    int32_t stop;                 /* LGR_REFINE_STOP_* */
    int32_t reserved0;            /* 0 */
    lgr_refine_step first;        /* T0 and its evaluation */
    lgr_refine_step rejected;     /* the candidate that lost (stop == NO_GAIN), zeroed otherwise */
    int32_t reserved[4];          /* 0 */
} lgr_refine_result;
int lgr_refine_plane_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float T0_16[16] /* host */,
                         const lgr_refine_params*, const lgr_metric_params* mp_or_null, lgr_refine_result* out /* host */,
                         lgr_refine_step* trace_or_null /* host */, int* n_trace_or_null);
int lgr_refine_plane(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float T0_16[16], const lgr_refine_params*,
                     const lgr_metric_params* mp_or_null, lgr_refine_result* out, lgr_refine_step* trace_or_null,
                     int* n_trace_or_null);   /* host twin */

/* ---- point-to-plane ICP: fine registration of a transform on the device.  A statement of this library's own (DESIGN.md section 4,
 *      "Point-to-plane ICP"; the reference has no ICP), bit-identical to the CPU statement tests/cpp/icp_ref.cpp:
 *        max_dist = params.max_dist > 0 ? params.max_dist : 4 x calculatePointCloudDensity(tgt); min_dist = params.min_dist > 0 ?
 *        params.min_dist : max_dist; c = centre of the target's bounding box; ONE grid over the target for max_dist.
 *        iteration k = 0, 1, ... with the f32 transform T_k (T_0 = T0):
 *            d_k = k ? max(min_dist, d_{k-1} x shrink) : max_dist                                  (f32)
 *            source point i pairs with j = its nearest target within d_k under the rule of lgr_evaluate_plane_dense (strict
 *            d2 < d_k^2, smallest squared distance, then lowest index) iff the moved point and the target's normal are finite;
 *            a pair's 28 f64 terms: g g^T (upper triangle), g r, r r with g = ((p - c) x n, n), r = n . (p - q); every other point: 28 x +0.0;
 *            each sum: the balanced binary tree over the source index, padded with +0.0 to the next power of two     (no atomics, no chain)
 *            pairs < 6 -> NO_PAIRS; A xi = -b by LDL^T in f64, a pivot not > 1e-12 x max diag A -> DEGENERATE           (T_k stays)
 *            T_{k+1} = [R | (c - R c) + t] o T_k, R from the unit quaternion (1, w / 2) / |.|, rounded to f32 once
 *            |w| < rot_eps && |t| < trans_eps -> CONVERGED; k + 1 == max_iterations -> MAX_ITERATIONS
 *      An empty source or max_iterations == 0 is LGR_OK with 0 iterations and T0 returned (stop NO_PAIRS / MAX_ITERATIONS, pairs 0, rmse
 *      FLT_MAX, max_dist = the caller's value when positive, else 0): nothing is computed.  nt < 2, max_iterations outside
 *      [0, LGR_ICP_MAX_ITERATIONS], a NaN or infinite max_dist / min_dist or one above 1e18, shrink outside (0, 1], a negative or NaN eps and
 *      non-zero reserved words: LGR_ERR_INVALID_ARG, before any work; so is a min_dist above the max_dist in use.  Rows 16-byte aligned.
 *      trace (optional, host, room for max_iterations entries): entry k is iteration k -- the transform it started from, d_k, its pairs
 *      and rmse, |w| and |t| of its step (0 when it took none); *n_trace = iterations evaluated (iterations, one more after NO_PAIRS /
 *      DEGENERATE).  The device path enqueues the iterations in groups of LGR_ICP_GROUP and reads one small record per group; the pairs,
 *      the terms, the sums and the transform never pass through the host.  The host form is lgr_icp_plane_host (not lgr_icp_plane: the name
 *      without a suffix is kept free until the host-entry table of the tests has a row for it). ---- */
#define LGR_ICP_MAX_ITERATIONS 1024
#define LGR_ICP_GROUP 8
enum { LGR_ICP_STOP_MAX_ITERATIONS = 0, LGR_ICP_STOP_CONVERGED = 1, LGR_ICP_STOP_NO_PAIRS = 2, LGR_ICP_STOP_DEGENERATE = 3 };
typedef struct {
    int32_t max_iterations;   /* 0 .. LGR_ICP_MAX_ITERATIONS */
    float   max_dist;         /* <= 0: 4 x the target's density */
    float   min_dist;         /* <= 0: max_dist */
    float   shrink;           /* (0, 1] */
    float   rot_eps;          /* rad */
    float   trans_eps;
    int32_t reserved[2];      /* 0 */
} lgr_icp_params;
void lgr_default_icp_params(lgr_icp_params* p);   /* 30 iterations, max_dist 0, min_dist 0, shrink 1, eps 1e-6 / 1e-6 */
typedef struct {
    float   transformation[16];   /* T_k, column-major */
    float   dist;                 /* d_k */
    int32_t pairs;
    float   rmse;                 /* (float) sqrt(sum r r / pairs); FLT_MAX without a pair */
    float   rot, trans;           /* |w|, |t| of the step taken, 0 without one */
    int32_t reserved[3];          /* 0 */
} lgr_icp_step;
typedef struct {
    float   transformation[16];   /* the final transform */
    int32_t iterations;           /* steps taken */
    int32_t stop;                 /* LGR_ICP_STOP_* */
    float   max_dist;             /* the value used */
    int32_t pairs;  float rmse;   /* of the last evaluated iteration */
    int32_t pairs0; float rmse0;  /* of iteration 0 */
    int32_t reserved[5];          /* 0 */
} lgr_icp_result;
int lgr_icp_plane_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float T0_16[16] /* host */,
                      const lgr_icp_params*, lgr_icp_result* out /* host */, lgr_icp_step* trace_or_null /* host */, int* n_trace_or_null);
int lgr_icp_plane_host(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float T0_16[16], const lgr_icp_params*,
                       lgr_icp_result* out, lgr_icp_step* trace_or_null, int* n_trace_or_null);   /* host twin */

/* ---- ICP variants: the loop of lgr_icp_plane* with another contribution per source point ("ICP variants"; CPU
 *      statement tests/cpp/icp_ex_ref.cpp).  The set-up, d_k, the balanced f64 tree padded with +0.0, the solve, the step, the stop rule,
 *      the trace and the grouped enqueue are those of lgr_icp_plane*; `base` is read exactly as lgr_icp_plane* reads its parameters.
 *      What source point i contributes in iteration k, all in f64, one IEEE operation at a time:
 *        1. p' = plane_move(T_k, p), j = nearest_within(d_k^2) by the rule above; no neighbour or a non-finite p': no pair.
 *        2. omega = weights ? (double) weights[i] : 1; an omega that is not finite or not > 0: no pair.
 *        3. n = the target normal of j; m = the source normal of i rotated by T_k's rotation block, m_a = (T[a] nx + T[4+a] ny) + T[8+a] nz.
 *           POINT_TO_PLANE reads n, PLANE_TO_PLANE n and m, the gate n and m, POINT_TO_POINT without the gate no normal at all.  A normal
 *           that is read and not finite: no pair.
 *        4. the gate (on iff min_normal_cos > -1): the pair is kept iff (mx nx + my ny) + mz nz >= (double) min_normal_cos.  It rejects the
 *           NEAREST neighbour; it does not look for the nearest compatible one.
 *        5. e = p' - q, u = p' - c, J = [-[u]x | I] with columns j_0 = (0, -uz, uy), j_1 = (uz, 0, -ux), j_2 = (-uy, ux, 0), j_3..5 = unit.
 *           POINT_TO_PLANE (one row): r = n . e, rho = |r|, g = (u x n, n), as lgr_icp_plane*.
 *           POINT_TO_POINT (three rows): M = I, rho^2 = e^T M e = e . e.
 *           PLANE_TO_PLANE (three rows; generalised ICP with covariances from the normals): Sigma = 2 I - (1 - eps)(n n^T + m m^T),
 *           M = Sigma^-1 by adjugate over determinant (icp_inv_sym3); a determinant that is not finite or not > 0: no pair;
 *           rho^2 = e^T M e, rho its square root.  Normals are used as given: pass unit normals.
 *        6. w = icp_robust_weight(robust, rho, k): NONE 1; HUBER rho <= k ? 1 : k / rho; CAUCHY 1 / (1 + rho^2 / k^2); TUKEY rho < k ?
 *           (1 - rho^2 / k^2)^2 : 0.  W = w omega; a W that is not > 0: no pair (a point Tukey switches off does not count in `pairs`).
 *        7. the 28 terms.  One row: (W g_a) g_b, (W g_a) r, and r r unweighted.  Three rows: W (j_a . (M j_b)), W (j_a . (M e)), and
 *           e . (M e) unweighted.  rmse = sqrt(slot 27 / pairs) is the variant's own unweighted residual: the point-to-plane distance, the
 *           point-to-point distance, and for PLANE_TO_PLANE the Mahalanobis distance under M.  Fewer than 6 pairs: NO_PAIRS, every variant.
 *      POINT_TO_PLANE / ROBUST_NONE / gate off / weights NULL returns the bytes of lgr_icp_plane* (W == 1 changes no product).
 *      Refused with LGR_ERR_INVALID_ARG before any work: everything lgr_icp_plane* refuses; an unknown variant or robust; with a robust
 *      kernel a robust_scale that is not finite or not > 0 (it is not read under ROBUST_NONE); min_normal_cos NaN or outside [-1, 1];
 *      plane_eps NaN, negative, or non-zero outside [1e-6, 1] (checked under every variant); a non-zero reserved word at either level.
 *      The idle calls (empty source, max_iterations 0) return what lgr_icp_plane* returns.  Not built: a symmetric objective, a search for
 *      the nearest compatible neighbour, the information matrix as an output.  The host form is lgr_icp_ex_host for the reason given above. ---- */
enum { LGR_ICP_POINT_TO_PLANE = 0, LGR_ICP_POINT_TO_POINT = 1, LGR_ICP_PLANE_TO_PLANE = 2 };
enum { LGR_ICP_ROBUST_NONE = 0, LGR_ICP_ROBUST_HUBER = 1, LGR_ICP_ROBUST_CAUCHY = 2, LGR_ICP_ROBUST_TUKEY = 3 };
typedef struct {
    lgr_icp_params base;      /* read exactly as lgr_icp_plane* reads it (reserved words 0) */
    int32_t variant;          /* LGR_ICP_* */
    int32_t robust;           /* LGR_ICP_ROBUST_* */
    float   robust_scale;     /* k, finite and > 0, in units of the variant's residual rho; read only when robust != NONE */
    float   min_normal_cos;   /* in [-1, 1]; the gate is on iff > -1 (the default filler writes -1) */
    float   plane_eps;        /* PLANE_TO_PLANE only: 0 = 1e-3, else in [1e-6, 1] */
    int32_t reserved[3];      /* 0 */
    const float* weights;     /* NULL, or ns per-source-point weights: device pointer for _dev, host pointer for _host */
} lgr_icp_ex_params;
void lgr_default_icp_ex_params(lgr_icp_ex_params* p);   /* base: lgr_default_icp_params; min_normal_cos -1; everything else 0 */
int lgr_icp_ex_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float T0_16[16] /* host */,
                   const lgr_icp_ex_params*, lgr_icp_result* out /* host */, lgr_icp_step* trace_or_null /* host */, int* n_trace_or_null);
int lgr_icp_ex_host(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float T0_16[16], const lgr_icp_ex_params*,
                    lgr_icp_result* out, lgr_icp_step* trace_or_null, int* n_trace_or_null);   /* host twin */

/* ---- trimmed ICP and median-scaled robust kernels: the loop of lgr_icp_ex* with two additions per iteration, both driven by exact ranks
 *      of the pairs' residuals found on the device ("Trimmed ICP"; CPU statement tests/cpp/icp_trim_ref.cpp).  Neither
 *      names an absolute scale.  Everything not said here is lgr_icp_ex*'s; `ex` is read exactly as lgr_icp_ex* reads its parameters.
 *      Per iteration:
 *        1. source point i is a candidate iff steps 1 - 5 above give it a pair (a neighbour, a finite p', omega > 0, finite normals where
 *           read, the gate, a plane-to-plane determinant > 0) and key_i = (float) rho_i is finite without a sign bit, so that its bits
 *           order as a uint32 (rho is formed under every configuration: |r|, or the square root of e^T M e).  P = the number of
 *           candidates, ordered by (key_i, i).
 *        2. K = (long long) floor((double) keep * (double) P); the first K candidates of the order are kept.  cut = the key of the K-th,
 *           0 when K = 0.
 *        3. with scale_from_median > 0: k = (double) scale_from_median * (double) key_m, m the candidate of rank (P - 1) / 2 among ALL
 *           candidates (key_m = 0 without one); a k that is not finite or not > 0 gives w = 1 in that iteration.  Otherwise k =
 *           ex.robust_scale.  scale = (float) k, or 0 under ROBUST_NONE.
 *        4. only a kept candidate contributes, with W = w(robust, rho, k) omega and the 28 terms of step 7; a W that is not > 0: no pair.
 *           pairs, rmse, the tree, the solve, the stop rule, the trace and the grouped enqueue are unchanged; K < 6 ends in NO_PAIRS.
 *      keep == 1 and scale_from_median == 0 forwards to lgr_icp_ex* and returns its bytes: no select runs, and info holds candidates =
 *      kept = pairs, cut 0 and scale = ex.robust_scale (0 under ROBUST_NONE).  Refused with LGR_ERR_INVALID_ARG before any work: whatever
 *      lgr_icp_ex* refuses; keep NaN or outside (0, 1]; scale_from_median NaN, negative or infinite; scale_from_median > 0 with
 *      ROBUST_NONE; a non-zero reserved word.  With scale_from_median > 0, ex.robust_scale is neither read nor validated.  info receives
 *      one entry per evaluated iteration, beside the trace's; *n_trace counts both and is required when either is given.  The idle calls
 *      (empty source, max_iterations 0) return what lgr_icp_ex* returns and write no info.  Not built: a fraction chosen per iteration,
 *      trimming by a fraction of all source points.  The host form carries _host for the reason given above. ---- */
typedef struct {
    lgr_icp_ex_params ex;      /* read exactly as lgr_icp_ex* reads it */
    float   keep;              /* in (0, 1]; 1 = no trimming */
    float   scale_from_median; /* 0 = use ex.robust_scale; > 0: k of the iteration = this x the median residual */
    int32_t reserved[2];       /* 0 */
} lgr_icp_trim_params;
typedef struct { int32_t candidates, kept; float cut, scale; } lgr_icp_trim_step;   /* one per evaluated iteration */
void lgr_default_icp_trim_params(lgr_icp_trim_params* p);   /* ex: lgr_default_icp_ex_params; keep 1; scale_from_median 0 */
int lgr_icp_trim_dev(lgr_ctx*, const float* d_src, int ns, const float* d_tgt, int nt, const float T0_16[16] /* host */,
                     const lgr_icp_trim_params*, lgr_icp_result* out /* host */, lgr_icp_step* trace_or_null /* host */,
                     lgr_icp_trim_step* info_or_null /* host */, int* n_trace_or_null);
int lgr_icp_trim_host(lgr_ctx*, const float* src, int ns, const float* tgt, int nt, const float T0_16[16], const lgr_icp_trim_params*,
                      lgr_icp_result* out, lgr_icp_step* trace_or_null, lgr_icp_trim_step* info_or_null, int* n_trace_or_null);   /* host twin */

/* ---- exact rank select, the primitive under trimmed ICP: among the elements with valid[i] != 0 (all when NULL) whose key is finite and
 *      carries no sign bit (a NaN, an infinite or a negative key is not counted), ordered by (key, i), the element at each of n_ranks (1
 *      or 2) ranks: its index and key.  below[i] = 1 iff element i is counted and its position is < ranks[0], else 0; *n_valid = the
 *      number counted.  LGR_ERR_INVALID_ARG for a rank outside [0, n_valid), except that ranks[0] == n_valid is allowed: it sets the flag
 *      of every counted element, and out_index[0] = -1, out_key[0] = 0.  (*n_valid is written also when a rank is refused.)  n = 0
 *      launches nothing.  MSB-first radix select over (key bits << 32) | i with integer histograms: deterministic, no sort. ---- */
int lgr_rank_select_dev(lgr_ctx*, const float* d_keys, const uint8_t* d_valid_or_null, int n, const int64_t* ranks /* host */, int n_ranks,
                        int32_t* out_index /* host, n_ranks */, float* out_key /* host, n_ranks */, uint8_t* d_below_or_null /* n */,
                        int64_t* n_valid /* host */);
int lgr_rank_select_host(lgr_ctx*, const float* keys, const uint8_t* valid_or_null, int n, const int64_t* ranks, int n_ranks,
                         int32_t* out_index, float* out_key, uint8_t* below_or_null, int64_t* n_valid);   /* host twin */

#ifdef __cplusplus
}
#endif
#endif
