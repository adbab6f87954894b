"""ctypes binding of liblgr_hip.so (the C ABI declared in include/lgr.h).

The HIP extension is mandatory: importing this module raises if the shared library is missing; nothing here (or
anywhere in the product) falls back to a CPU path.
"""
import ctypes as C
import os

import numpy as np

try:   # torch ships its own HIP runtime: it must be loaded BEFORE liblgr_hip.so pulls in libamdhip64
    import torch as _torch  # noqa: F401
except ImportError:  # pragma: no cover
    _torch = None

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
# LGR_HIP_LIB: another build of the same sources (A/B experiments of tools/: e.g. a library built with `make EXP=-D...`); never a fallback
LIB_PATH = os.environ.get("LGR_HIP_LIB") or os.path.join(_CSRC, "liblgr_hip.so")

MATCH_LR, MATCH_ONE_SIDED, MATCH_CLUSTER, MATCH_RATIO = 0, 1, 2, 3
MATCHING_RATIO_THRESHOLD = 1.1     # LGR_MATCHING_RATIO_THRESHOLD: what the pipeline uses under MATCH_RATIO
METRIC_CORRESPONDENCES, METRIC_UNIFORMITY, METRIC_CLOSEST_PLANE, METRIC_COMBINATION, METRIC_WEIGHTED_CLOSEST_PLANE = 0, 1, 2, 3, 4
WEIGHT_CONSTANT, WEIGHT_EXP_CURVATURE, WEIGHT_CURVEDNESS, WEIGHT_HARRIS, WEIGHT_TOMASI, WEIGHT_CURVATURE, WEIGHT_NSS = 0, 1, 2, 3, 4, 5, 6
WEIGHT_IDS = {"constant": 0, "exp_curvature": 1, "curvedness": 2, "harris": 3, "tomasi": 4, "curvature": 5, "nss": 6}
KEYPOINT_ANY, KEYPOINT_ISS = 0, 1
SCORE_CONSTANT, SCORE_MAE, SCORE_MSE, SCORE_EXP = 0, 1, 2, 3
ALIGN_RANSAC, ALIGN_GROR = 0, 1
ORDER_REFERENCE, ORDER_CANONICAL = 0, 1
DESCRIPTOR_FPFH, DESCRIPTOR_SHOT, DESCRIPTOR_ROPS = 0, 1, 2
LRF_DEFAULT, LRF_GRAVITY, LRF_GT = 0, 1, 2
ERR_UNSUPPORTED = -5
ERR_INVALID_ARG = -1

CORR_DTYPE = np.dtype([("index_query", "<i4"), ("index_match", "<i4"), ("distance", "<f4"), ("threshold", "<f4")])


class Params(C.Structure):
    _fields_ = [
        ("feature_nr_points", C.c_int32), ("normal_nr_points", C.c_int32), ("edge_thr_coef", C.c_float),
        ("distance_thr", C.c_float), ("feature_radius", C.c_float), ("scale_factor", C.c_float),
        ("confidence", C.c_float), ("bf_block_size", C.c_int32), ("cluster_k", C.c_int32),
        ("randomness", C.c_int32), ("n_samples", C.c_int32),
        ("alignment_id", C.c_int32), ("matching_id", C.c_int32), ("metric_id", C.c_int32), ("score_id", C.c_int32),
        ("max_iterations", C.c_int32), ("normals_available", C.c_int32), ("fix_seed", C.c_int32),
        ("has_vp_src", C.c_int32), ("has_vp_tgt", C.c_int32), ("vp_src", C.c_float * 3), ("vp_tgt", C.c_float * 3),
        ("ransac_batch", C.c_int32), ("seed", C.c_uint64),
        ("keypoint_id", C.c_int32), ("iss_radius_src", C.c_float), ("iss_radius_tgt", C.c_float), ("use_bfmatcher", C.c_int32),
        ("has_guess", C.c_int32), ("match_search_radius", C.c_float), ("guess", C.c_float * 16),
    ]


class Result(C.Structure):
    _fields_ = [
        ("transformation", C.c_float * 16), ("iterations", C.c_int32), ("converged", C.c_int32),
        ("n_inliers", C.c_int32), ("metric", C.c_float), ("best_metric_before_refit", C.c_float),
        ("best_iteration", C.c_int32), ("num_rejections", C.c_int32), ("estimated_iters", C.c_int32),
        ("n_correspondences", C.c_int32), ("time_cs", C.c_double), ("time_te", C.c_double),
        ("stage_ms", C.c_float * 12),
    ]

    def matrix(self):
        return np.array(self.transformation, dtype=np.float32).reshape(4, 4).T.copy()


TEASER_NODES_MAX = 2048   # LGR_TEASER_NODES_MAX


class TeaserParams(C.Structure):
    """lgr_teaser_params (include/lgr.h): the values of the reference's commented-out alignTeaser body (src/alignment.cpp:41-69)."""
    _fields_ = [("noise_bound", C.c_float), ("k_select", C.c_int32), ("rotation_max_iterations", C.c_int32), ("rotation_gnc_factor", C.c_float),
                ("rotation_cost_threshold", C.c_float), ("reserved", C.c_int32 * 3)]


class TeaserInfo(C.Structure):
    """lgr_teaser_info (include/lgr.h)."""
    _fields_ = [("valid", C.c_int32), ("n_nodes", C.c_int32), ("max_core", C.c_int32), ("n_core", C.c_int32), ("n_clique", C.c_int32),
                ("rotation_iterations", C.c_int32), ("n_rotation_inliers", C.c_int32), ("n_translation_inliers", C.c_int32),
                ("rotation_cost", C.c_float), ("translation_cost", C.c_float * 3), ("reserved", C.c_int32 * 4)]


def default_teaser_params(distance_thr, **kw):
    """lgr_default_teaser_params + overrides"""
    p = TeaserParams()
    _lib.lgr_default_teaser_params(C.byref(p), C.c_float(distance_thr))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


class MatchOptions(C.Structure):
    """lgr_match_options (include/lgr.h): how the matcher runs, never what it returns."""
    _fields_ = [("prune", C.c_int32), ("leaves", C.c_int32), ("near", C.c_int32), ("operand_format", C.c_int32), ("box_bounds", C.c_int32),
                ("column_stage", C.c_int32), ("coarse_rejection", C.c_int32), ("rerank_refilter", C.c_int32), ("pair_cap", C.c_int32),
                ("poison_tables", C.c_int32), ("self_check", C.c_int32), ("shell_bound", C.c_int32), ("split_sweep", C.c_int32), ("kept_cap", C.c_int32), ("auto_dense", C.c_int32),
                ("irregular_rows", C.c_int32)]


class CtxOptions(C.Structure):
    """lgr_ctx_options (include/lgr.h): how the context uses host threads and streams, never what it returns."""
    _fields_ = [("helper_contexts", C.c_int32), ("concurrent_contexts", C.c_int32), ("arithmetic", C.c_int32), ("pcl_neighbour_cap", C.c_int32),
                ("ransac_schedule", C.c_int32), ("reserved", C.c_int32 * 3)]


RANSAC_SCHEDULE_DEFAULT, RANSAC_SCHEDULE_CHAIN, RANSAC_SCHEDULE_RESIDENT = 0, 1, 2   # lgr_ctx_options.ransac_schedule
ARITH_FAST, ARITH_PCL = 0, 1   # lgr_ctx_options.arithmetic (include/lgr.h): the FPFH weighting as one fused chain in grid order / exactly as PCL writes it
LIBM_ACOSF, LIBM_ATANF, LIBM_ATAN2F, LIBM_SINF, LIBM_COSF = 0, 1, 2, 3, 4


FORMAT_AUTO, FORMAT_F32, FORMAT_F16, FORMAT_F16R = -1, 0, 1, 2


class FeatureParams(C.Structure):
    """lgr_feature_params: the descriptor of the correspondence search (AlignmentParameters.descriptor_id / lrf_id) and ratio_k."""
    _fields_ = [("descriptor_id", C.c_int32), ("lrf_id", C.c_int32), ("ratio_k", C.c_int32), ("reserved", C.c_int32 * 5)]


def feature_params(descriptor="fpfh", lrf_id=None, ratio_k=None):
    """descriptor: 'fpfh' / 'shot' / 'rops' (or the LGR_DESCRIPTOR_* value).  lrf_id None: the frames built for the descriptor
    (LRF_GRAVITY for RoPS, LRF_DEFAULT otherwise).  ratio_k (MATCH_RATIO only): the list length of the ratio test, None = 2."""
    f = FeatureParams()
    _lib.lgr_default_feature_params(C.byref(f))
    f.descriptor_id = {"fpfh": DESCRIPTOR_FPFH, "shot": DESCRIPTOR_SHOT, "rops": DESCRIPTOR_ROPS}.get(descriptor, descriptor)
    if lrf_id is None:
        lrf_id = LRF_GRAVITY if f.descriptor_id == DESCRIPTOR_ROPS else LRF_DEFAULT
    f.lrf_id = int(lrf_id)
    if ratio_k is not None:
        f.ratio_k = int(ratio_k)
    return f


class MetricParams(C.Structure):
    _fields_ = [("weight_id", C.c_int32), ("reserved", C.c_int32 * 5), ("weights", C.c_void_p)]


def metric_params(weight="constant", weights=None):
    """weighted_closest_plane's point weights: weight = 'constant' / 'exp_curvature' / 'curvedness' / 'curvature' / 'nss' (or the
    LGR_WEIGHT_* value); weights = caller-supplied per-source-point weights (numpy for the host entries, a cuda tensor for the _dev
    entries: keep it alive for the call) used instead."""
    m = MetricParams()
    _lib.lgr_default_metric_params(C.byref(m))
    m.weight_id = WEIGHT_IDS.get(weight, weight) if isinstance(weight, str) else int(weight)
    if weights is not None:
        m.weights = _ptr(weights).value
    return m


class GtEval(C.Structure):
    """lgr_gt_eval (include/lgr.h): an alignment judged against its ground truth.  Angles in radians."""
    _fields_ = [("r_err", C.c_float), ("t_err", C.c_float), ("pcd_err", C.c_float), ("overlap_rmse", C.c_float), ("overlap_size", C.c_int32),
                ("normal_diff", C.c_float), ("n_normal_overlap", C.c_int32), ("n_overlap_src", C.c_int32), ("n_overlap_tgt", C.c_int32),
                ("n_overlap", C.c_int32), ("overlap", C.c_float), ("overlap_area", C.c_float), ("n_correspondences", C.c_int32),
                ("n_correct_correspondences", C.c_int32), ("n_inliers", C.c_int32), ("n_correct_inliers", C.c_int32),
                ("corr_uniformity", C.c_float), ("converged", C.c_int32), ("converged_and_overlap_ok", C.c_int32), ("reserved", C.c_int32 * 5)]
    correct_mask = None   # numpy uint8 [c], set by Context.evaluate_gt*

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class PlaneDenseEval(C.Structure):
    """lgr_plane_dense_eval (include/lgr.h): the dense closest-plane evaluation of one transform."""
    _fields_ = [("n_inliers", C.c_int32), ("rmse", C.c_float), ("metric", C.c_float), ("threshold", C.c_float), ("score", C.c_float),
                ("reserved", C.c_int32 * 3)]
    inliers = None   # numpy CORR_DTYPE [n_inliers] (with_inliers), set by Context.evaluate_plane_dense*
    nn = None        # numpy int32 [ns] (with_nn)


class MetricEval(C.Structure):
    """lgr_metric_eval (include/lgr.h): metric, rmse, inliers and correct inliers of an alignment under any metric_id."""
    _fields_ = [("metric", C.c_float), ("rmse", C.c_float), ("n_inliers", C.c_int32), ("n_correct_inliers", C.c_int32), ("reserved", C.c_int32 * 4)]


REFINE_MAX_STEPS, REFINE_GROUP = 1024, 4   # LGR_REFINE_MAX_STEPS, LGR_REFINE_GROUP
REFINE_STOP_MAX_STEPS, REFINE_STOP_NO_GAIN, REFINE_STOP_NO_PAIRS = 0, 1, 2
REFINE_STOP_NAMES = ("max_steps", "no_gain", "no_pairs")


class RefineParams(C.Structure):
    """lgr_refine_params (include/lgr.h)"""
    _fields_ = [("score_id", C.c_int32), ("max_steps", C.c_int32), ("threshold", C.c_float), ("reserved", C.c_int32 * 5)]


class RefineStep(C.Structure):
    """lgr_refine_step (include/lgr.h): one evaluated transform of a refinement"""
    _fields_ = [("transformation", C.c_float * 16), ("metric", C.c_float), ("rmse", C.c_float), ("score", C.c_float), ("n_inliers", C.c_int32)]

    def matrix(self):
        return np.array(self.transformation, dtype=np.float32).reshape(4, 4).T.copy()


class RefineResult(C.Structure):
    """lgr_refine_result (include/lgr.h): the last accepted step, why the loop ended, T0's evaluation and the candidate that lost"""
    _fields_ = [("transformation", C.c_float * 16), ("metric", C.c_float), ("rmse", C.c_float), ("score", C.c_float), ("n_inliers", C.c_int32),
                ("threshold", C.c_float), ("steps", C.c_int32), ("stop", C.c_int32), ("reserved0", C.c_int32), ("first", RefineStep),
                ("rejected", RefineStep), ("reserved", C.c_int32 * 4)]
    trace = None   # list of RefineStep (trace=True), set by Context.refine_plane*

    def matrix(self):
        return np.array(self.transformation, dtype=np.float32).reshape(4, 4).T.copy()


def refine_params(score_id=None, max_steps=None, threshold=None):
    p = RefineParams()
    _lib.lgr_default_refine_params(C.byref(p))
    if score_id is not None:
        p.score_id = int(score_id)
    if max_steps is not None:
        p.max_steps = int(max_steps)
    if threshold is not None:
        p.threshold = float(threshold)
    return p


ICP_MAX_ITERATIONS, ICP_GROUP = 1024, 8   # LGR_ICP_MAX_ITERATIONS, LGR_ICP_GROUP
ICP_STOP_MAX_ITERATIONS, ICP_STOP_CONVERGED, ICP_STOP_NO_PAIRS, ICP_STOP_DEGENERATE = 0, 1, 2, 3
ICP_STOP_NAMES = ("max_iterations", "converged", "no_pairs", "degenerate")


class IcpParams(C.Structure):
    """lgr_icp_params (include/lgr.h)"""
    _fields_ = [("max_iterations", C.c_int32), ("max_dist", C.c_float), ("min_dist", C.c_float), ("shrink", C.c_float), ("rot_eps", C.c_float),
                ("trans_eps", C.c_float), ("reserved", C.c_int32 * 2)]


class IcpStep(C.Structure):
    """lgr_icp_step (include/lgr.h): one evaluated iteration of a point-to-plane ICP"""
    _fields_ = [("transformation", C.c_float * 16), ("dist", C.c_float), ("pairs", C.c_int32), ("rmse", C.c_float), ("rot", C.c_float), ("trans", C.c_float),
                ("reserved", C.c_int32 * 3)]

    def matrix(self):
        return np.array(self.transformation, dtype=np.float32).reshape(4, 4).T.copy()


class IcpResult(C.Structure):
    """lgr_icp_result (include/lgr.h): the final transform, why the loop ended, the pairs and rmse of the last and the first iteration"""
    _fields_ = [("transformation", C.c_float * 16), ("iterations", C.c_int32), ("stop", C.c_int32), ("max_dist", C.c_float), ("pairs", C.c_int32),
                ("rmse", C.c_float), ("pairs0", C.c_int32), ("rmse0", C.c_float), ("reserved", C.c_int32 * 5)]
    trace = None   # list of IcpStep (trace=True), set by Context.icp_plane*
    info = None    # list of IcpTrimStep, set by Context.icp_trim*

    def matrix(self):
        return np.array(self.transformation, dtype=np.float32).reshape(4, 4).T.copy()


def icp_params(max_iterations=None, max_dist=None, min_dist=None, shrink=None, rot_eps=None, trans_eps=None):
    p = IcpParams()
    _lib.lgr_default_icp_params(C.byref(p))
    if max_iterations is not None:
        p.max_iterations = int(max_iterations)
    for name, v in (("max_dist", max_dist), ("min_dist", min_dist), ("shrink", shrink), ("rot_eps", rot_eps), ("trans_eps", trans_eps)):
        if v is not None:
            setattr(p, name, float(v))
    return p


ICP_POINT_TO_PLANE, ICP_POINT_TO_POINT, ICP_PLANE_TO_PLANE = 0, 1, 2        # LGR_ICP_*
ICP_ROBUST_NONE, ICP_ROBUST_HUBER, ICP_ROBUST_CAUCHY, ICP_ROBUST_TUKEY = 0, 1, 2, 3   # LGR_ICP_ROBUST_*
ICP_VARIANT_IDS = {"plane": 0, "point": 1, "plane2plane": 2}
ICP_ROBUST_IDS = {"none": 0, "huber": 1, "cauchy": 2, "tukey": 3}


class IcpExParams(C.Structure):
    """lgr_icp_ex_params (include/lgr.h)"""
    _fields_ = [("base", IcpParams), ("variant", C.c_int32), ("robust", C.c_int32), ("robust_scale", C.c_float), ("min_normal_cos", C.c_float),
                ("plane_eps", C.c_float), ("reserved", C.c_int32 * 3), ("weights", C.c_void_p)]


def icp_ex_params(variant=None, robust=None, robust_scale=None, min_normal_cos=None, plane_eps=None, weights=None, **base_kw):
    """lgr_default_icp_ex_params, then the given fields.  variant / robust: the LGR_ICP_* value or its name ('plane', 'point', 'plane2plane';
    'none', 'huber', 'cauchy', 'tukey'); weights: per-source-point weights (a cuda tensor for the _dev entry, numpy for the host entry:
    keep it alive for the call); base_kw: the keywords of icp_params."""
    p = IcpExParams()
    _lib.lgr_default_icp_ex_params(C.byref(p))
    p.base = icp_params(**base_kw)
    if variant is not None:
        p.variant = ICP_VARIANT_IDS[variant] if isinstance(variant, str) else int(variant)
    if robust is not None:
        p.robust = ICP_ROBUST_IDS[robust] if isinstance(robust, str) else int(robust)
    for name, v in (("robust_scale", robust_scale), ("min_normal_cos", min_normal_cos), ("plane_eps", plane_eps)):
        if v is not None:
            setattr(p, name, float(v))
    if weights is not None:
        p.weights = _ptr(weights).value
    return p


class IcpTrimParams(C.Structure):
    """lgr_icp_trim_params (include/lgr.h)"""
    _fields_ = [("ex", IcpExParams), ("keep", C.c_float), ("scale_from_median", C.c_float), ("reserved", C.c_int32 * 2)]


class IcpTrimStep(C.Structure):
    """lgr_icp_trim_step (include/lgr.h): the candidates, the kept ones, the cut and the robust scale of one evaluated iteration"""
    _fields_ = [("candidates", C.c_int32), ("kept", C.c_int32), ("cut", C.c_float), ("scale", C.c_float)]


def icp_trim_params(keep=None, scale_from_median=None, **ex_and_base):
    """lgr_default_icp_trim_params, then the given fields; ex_and_base: the keywords of icp_ex_params"""
    p = IcpTrimParams()
    _lib.lgr_default_icp_trim_params(C.byref(p))
    p.ex = icp_ex_params(**ex_and_base)
    if keep is not None:
        p.keep = float(keep)
    if scale_from_median is not None:
        p.scale_from_median = float(scale_from_median)
    return p


class TemperatureOut(C.Structure):
    """lgr_temperature_out (include/lgr.h): five optional per-point arrays of one temperature map."""
    _fields_ = [("temp_distance", C.c_void_p), ("temp_normal", C.c_void_p), ("color_distance", C.c_void_p), ("color_normal", C.c_void_p), ("nn", C.c_void_p)]


TEMP_FIELDS = ("temp_distance", "temp_normal", "color_distance", "color_normal", "nn")
COLOR_BEIGE, COLOR_RED, COLOR_PARAKEET, COLOR_BLUE, COLOR_WHITE = 0xf8c471, 0xff0000, 0x03c04a, 0x0000ff, 0xffffff


HYPOTHESES_MAX = 2048   # LGR_HYPOTHESES_MAX


class Hypothesis(C.Structure):
    """lgr_hypothesis (include/lgr.h): one member of the set of distinct hypotheses after the final block."""
    _fields_ = [("loop_transformation", C.c_float * 16), ("transformation", C.c_float * 16), ("iteration", C.c_int32),
                ("loop_metric", C.c_float), ("metric", C.c_float), ("n_inliers", C.c_int32), ("converged", C.c_int32),
                ("uniformity", C.c_float)]

    def loop_matrix(self):
        return np.array(self.loop_transformation, dtype=np.float32).reshape(4, 4).T.copy()

    def matrix(self):
        return np.array(self.transformation, dtype=np.float32).reshape(4, 4).T.copy()


GT_BATCH_MAX, GT_BATCH_CHUNK = 64, 8   # LGR_GT_BATCH_MAX, LGR_GT_BATCH_CHUNK


class MeasureRun(C.Structure):
    """lgr_measure_run (include/lgr.h): one seeded run of Context.measure*: its seed, its alignment and its ground-truth evaluation."""
    _fields_ = [("seed", C.c_uint64), ("result", Result), ("eval", GtEval)]


class Measurement(C.Structure):
    """lgr_measurement (include/lgr.h): the test_measurements.csv columns over the runs (src/main.cpp:324)."""
    _fields_ = [("n_times", C.c_int32), ("n_success", C.c_int32), ("success_rate", C.c_float), ("mae", C.c_float), ("sae", C.c_float),
                ("mte", C.c_float), ("ste", C.c_float), ("mrmse", C.c_float), ("srmse", C.c_float), ("mtime", C.c_float), ("stime", C.c_float),
                ("reserved", C.c_int32 * 5)]


class CloudInfo(C.Structure):
    """struct lgr_cloud_info (include/lgr.h)."""
    _fields_ = [("n", C.c_int32), ("keypoints", C.c_int32), ("row_len", C.c_int32), ("levels", C.c_int32), ("first_log2_radius", C.c_int32),
                ("multiscale", C.c_int32), ("bytes", C.c_uint64), ("reserved", C.c_int32 * 4)]


class CloudLevelInfo(C.Structure):
    """lgr_cloud_level_info (include/lgr.h)."""
    _fields_ = [("log2_radius", C.c_int32), ("radius", C.c_float), ("voxel", C.c_float), ("rows", C.c_int32), ("surface", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class LgrError(RuntimeError):
    pass


def load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C {_CSRC}` (or __graft_entry__.build()). "
            "The MI355X HIP extension is mandatory; there is no CPU fallback.")
    return C.CDLL(LIB_PATH)


ABI_VERSION = 5      # LGR_VERSION of the include/lgr.h these structures mirror

_lib = load()
_lib.lgr_last_error.restype = C.c_char_p
_lib.lgr_last_error.argtypes = [C.c_void_p]
_lib.lgr_measure_mean.restype = C.c_float
_lib.lgr_measure_mean.argtypes = [C.c_void_p, C.c_int]
_lib.lgr_measure_deviation.restype = C.c_float
_lib.lgr_measure_deviation.argtypes = [C.c_void_p, C.c_int, C.c_float]
_lib.lgr_cloud_destroy.argtypes = [C.c_void_p]
_lib.lgr_cloud_info.argtypes = [C.c_void_p, C.c_void_p]
_lib.lgr_cloud_keypoints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
_lib.lgr_cloud_level.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
if _lib.lgr_version() != ABI_VERSION:     # a stale liblgr_hip.so would read lgr_params / call lgr_match_last_* with another layout
    raise ImportError(f"{LIB_PATH} has ABI revision {_lib.lgr_version()}, this binding needs {ABI_VERSION}: rebuild it (make -C {_CSRC})")


def lib():
    return _lib


def default_params(**kw):
    p = Params()
    _lib.lgr_default_params(C.byref(p))
    for k, v in kw.items():
        if k in ("vp_src", "vp_tgt"):
            setattr(p, k, (C.c_float * 3)(*[float(x) for x in v]))
            setattr(p, "has_" + k, 1)
        elif k == "guess":      # 4x4, row/col indexed normally -> column-major 16
            p.guess = (C.c_float * 16)(*np.asarray(v, np.float32).T.reshape(16).tolist())
            p.has_guess = 1
        else:
            assert hasattr(p, k), k
            setattr(p, k, v)
    return p


def _ptr(t):
    """device (torch tensor) or host (numpy) pointer as void*."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data_as(C.c_void_p)
    return C.c_void_p(t.data_ptr())


class PreparedCloud:
    """One lgr_cloud (Context.prepare_cloud): key points, per-level descriptor rows and the filter's tables of one cloud, in device
    memory of its own.  Read-only for every pair call; close() (or the with block) frees it."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if self.h:
            _lib.lgr_cloud_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def _ok(rc):
        if rc != 0:
            raise LgrError(f"rc={rc}")

    def info(self):
        out = CloudInfo()
        self._ok(_lib.lgr_cloud_info(self.h, C.byref(out)))
        return out

    def keypoints(self):
        """indices of the key points into the cloud, int32 [m]"""
        out = np.empty(self.info().keypoints, np.int32)
        m = C.c_int(0)
        self._ok(_lib.lgr_cloud_keypoints(self.h, _ptr(out), C.byref(m)))
        return out[: m.value]

    def levels(self):
        """the CloudLevelInfo of every level"""
        out = []
        for i in range(self.info().levels):
            li = CloudLevelInfo()
            self._ok(_lib.lgr_cloud_level(self.h, i, C.byref(li), None, None))
            out.append(li)
        return out

    def level(self, i):
        """(CloudLevelInfo, list int32 [rows] of indices into the key points, rows float32 [rows, row_len])"""
        li = CloudLevelInfo()
        self._ok(_lib.lgr_cloud_level(self.h, int(i), C.byref(li), None, None))
        lst = np.empty(li.rows, np.int32)
        rows = np.empty((li.rows, self.info().row_len), np.float32)
        self._ok(_lib.lgr_cloud_level(self.h, int(i), C.byref(li), _ptr(lst), _ptr(rows)))
        return li, lst, rows


class Context:
    """One lgr_ctx bound to a torch device + (by default) torch's current stream on it.  stream=-1 (LGR_STREAM_OWN): the context
    creates a non-blocking stream of its own -- torch's stream does not wait for it, so device outputs of the *_dev wrappers below
    must be consumed after ctx.sync() (the wrappers that read results back through torch do that themselves: _join)."""

    def __init__(self, device=0, stream=None):
        import torch
        self.torch = torch
        self.device = int(device)
        self.foreign_stream = stream is not None and stream != torch.cuda.current_stream(self.device).cuda_stream
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        h = C.c_void_p()
        rc = _lib.lgr_ctx_create(self.device, C.c_void_p(stream), C.byref(h))
        if rc != 0:
            raise LgrError(f"lgr_ctx_create failed: {rc}")
        self.h = h

    def close(self):
        if self.h:
            _lib.lgr_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            raise LgrError(f"rc={rc}: {_lib.lgr_last_error(self.h).decode()}")

    def sync(self):
        self.check(_lib.lgr_ctx_sync(self.h))

    def _join(self):
        """before torch reads a buffer the library wrote: nothing to do on torch's own stream, a stream sync otherwise"""
        if self.foreign_stream:
            self.sync()

    def set_match_options(self, **kw):
        """defaults + overrides (no arguments: back to the defaults); returns the options now in force"""
        o = MatchOptions()
        _lib.lgr_match_default_options(C.byref(o))
        for k, v in kw.items():
            assert hasattr(o, k), k
            setattr(o, k, int(v))
        self.check(_lib.lgr_ctx_set_match_options(self.h, C.byref(o)))
        return o

    def match_options(self):
        o = MatchOptions()
        self.check(_lib.lgr_ctx_get_match_options(self.h, C.byref(o)))
        return o

    def set_options(self, **kw):
        """lgr_ctx_options: defaults + overrides (helper_contexts=0: one host thread, one stream); returns the options now in force"""
        o = CtxOptions()
        _lib.lgr_ctx_default_options(C.byref(o))
        for k, v in kw.items():
            assert hasattr(o, k), k
            setattr(o, k, int(v))
        self.check(_lib.lgr_ctx_set_options(self.h, C.byref(o)))
        return o

    def host_threads(self):
        """1 + the helper host threads this context has started (at most 2)"""
        n = C.c_int(0)
        self.check(_lib.lgr_ctx_host_threads(self.h, C.byref(n)))
        return n.value

    def workspace_bytes(self):
        out = C.c_uint64(0)
        self.check(_lib.lgr_ctx_workspace_bytes(self.h, C.byref(out)))
        return int(out.value)

    def _dev(self):
        return self.torch.device("cuda", self.device)

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self._dev())

    # ---- matching -------------------------------------------------------------------------------------------
    def match_bf(self, q, t, block=10000):
        """q, t: cuda float32 [m,33].  returns (idx int32 [mq], dist float32 [mq])."""
        torch = self.torch
        q = q.contiguous(); t = t.contiguous()
        idx = self.empty((q.shape[0],), torch.int32)
        dist = self.empty((q.shape[0],), torch.float32)
        self.check(_lib.lgr_match_bf_dev(self.h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_bf2(self, a, b, block=10000):
        torch = self.torch
        a = a.contiguous(); b = b.contiguous()
        ab_i = self.empty((a.shape[0],), torch.int32); ab_d = self.empty((a.shape[0],), torch.float32)
        ba_i = self.empty((b.shape[0],), torch.int32); ba_d = self.empty((b.shape[0],), torch.float32)
        self.check(_lib.lgr_match_bf2_dev(self.h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], int(block),
                                          _ptr(ab_i), _ptr(ab_d), _ptr(ba_i), _ptr(ba_d)))
        return ab_i, ab_d, ba_i, ba_d

    def sort_pairs_u32(self, keys, vals, begin_bit=0, end_bit=32):
        """lgr_sort_pairs_u32_dev: cuda int32 keys (bit patterns of the uint32 keys) and int32 values -> (keys, values) stably sorted
        by the key bits [begin_bit, end_bit)"""
        torch = self.torch
        keys = keys.contiguous(); vals = vals.contiguous()
        ko = self.empty((keys.shape[0],), torch.int32); vo = self.empty((keys.shape[0],), torch.int32)
        self.check(_lib.lgr_sort_pairs_u32_dev(self.h, _ptr(keys), _ptr(ko), _ptr(vals), _ptr(vo), C.c_size_t(keys.shape[0]), int(begin_bit), int(end_bit)))
        return ko, vo

    def sort_pairs_u64(self, keys, vals, ranges):
        """lgr_sort_pairs_u64_dev: cuda int64 keys (bit patterns), int32 values, ranges = [(shift, width), ...] least significant first"""
        torch = self.torch
        keys = keys.contiguous(); vals = vals.contiguous()
        ko = self.empty((keys.shape[0],), torch.int64); vo = self.empty((keys.shape[0],), torch.int32)
        sh = (C.c_int * max(1, len(ranges)))(*[r[0] for r in ranges]); wd = (C.c_int * max(1, len(ranges)))(*[r[1] for r in ranges])
        self.check(_lib.lgr_sort_pairs_u64_dev(self.h, _ptr(keys), _ptr(ko), _ptr(vals), _ptr(vo), C.c_size_t(keys.shape[0]), sh, wd, len(ranges)))
        return ko, vo

    def match_flann(self, q, t):
        """matchFLANN<FPFH> (include/matching.h:565-592): cuda float32 [m,33] -> (idx, dist)"""
        torch = self.torch
        q = q.contiguous(); t = t.contiguous()
        idx = self.empty((q.shape[0],), torch.int32)
        dist = self.empty((q.shape[0],), torch.float32)
        self.check(_lib.lgr_match_flann_dev(self.h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_local(self, qpts, tpts, qf, tf, guess, radius):
        """matchLocal<FPFH> (include/matching.h:637-678): points [m,12], descriptors [m,33] on the device; guess 4x4 (numpy)"""
        torch = self.torch
        g = (C.c_float * 16)(*np.asarray(guess, np.float32).T.reshape(16).tolist())
        idx = self.empty((qpts.shape[0],), torch.int32)
        dist = self.empty((qpts.shape[0],), torch.float32)
        self.check(_lib.lgr_match_local_dev(self.h, _ptr(qpts), qpts.shape[0], _ptr(tpts), tpts.shape[0], _ptr(qf.contiguous()), _ptr(tf.contiguous()),
                                            g, C.c_float(radius), _ptr(idx), _ptr(dist)))
        return idx, dist

    # ---- matchLocal with a k-list and matchFLANN on FPFH / RoPS135 / SHOT rows (the row length is the descriptors' second dimension) ----
    def match_local_knn(self, qpts, tpts, qf, tf, guess, radius, k=1):
        """matchLocal<FeatureT> with randomness = k: cuda points [m, 12], descriptors [m, 33 | 135 | 352]; guess 4x4 (numpy).
        (idx int32 [mq, k], dist float32 [mq, k]): a query's candidates in ascending (distance, spatial distance, index), then -1 / 0."""
        torch = self.torch
        g = (C.c_float * 16)(*np.asarray(guess, np.float32).T.reshape(16).tolist())
        qpts = qpts.contiguous(); tpts = tpts.contiguous(); qf = qf.contiguous(); tf = tf.contiguous()
        idx = self.empty((qf.shape[0], max(int(k), 0)), torch.int32)
        dist = self.empty((qf.shape[0], max(int(k), 0)), torch.float32)
        self.check(_lib.lgr_match_local_knn_dev(self.h, int(qf.shape[1]), _ptr(qpts), qf.shape[0], _ptr(tpts), tf.shape[0], _ptr(qf), _ptr(tf),
                                                g, C.c_float(radius), int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_local_knn_host(self, qpts, tpts, qf, tf, guess, radius, k=1):
        g = (C.c_float * 16)(*np.asarray(guess, np.float32).T.reshape(16).tolist())
        qpts = np.ascontiguousarray(qpts, np.float32); tpts = np.ascontiguousarray(tpts, np.float32)
        qf = np.ascontiguousarray(qf, np.float32); tf = np.ascontiguousarray(tf, np.float32)
        idx = np.zeros((qf.shape[0], max(int(k), 0)), np.int32); dist = np.zeros((qf.shape[0], max(int(k), 0)), np.float32)
        self.check(_lib.lgr_match_local_knn(self.h, int(qf.shape[1]), _ptr(qpts), qf.shape[0], _ptr(tpts), tf.shape[0], _ptr(qf), _ptr(tf),
                                            g, C.c_float(radius), int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_flann_rows(self, q, t):
        """matchFLANN<FeatureT>, randomness 1: cuda float32 [m, 33 | 135 | 352] -> (idx int32 [mq], dist float32 [mq]); the row the
        brute-force matcher finds with one train block, the distance in FLANN's sequential order."""
        torch = self.torch
        q = q.contiguous(); t = t.contiguous()
        idx = self.empty((q.shape[0],), torch.int32); dist = self.empty((q.shape[0],), torch.float32)
        self.check(_lib.lgr_match_flann_rows_dev(self.h, int(q.shape[1]), _ptr(q), q.shape[0], _ptr(t), t.shape[0], _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_flann_rows_host(self, q, t):
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        idx = np.zeros(q.shape[0], np.int32); dist = np.zeros(q.shape[0], np.float32)
        self.check(_lib.lgr_match_flann_rows(self.h, int(q.shape[1]), _ptr(q), q.shape[0], _ptr(t), t.shape[0], _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_bf_host(self, q, t, block=10000):
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        idx = np.zeros(q.shape[0], np.int32); dist = np.zeros(q.shape[0], np.float32)
        self.check(_lib.lgr_match_bf(self.h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_stats(self):
        out = (C.c_uint * 6)()
        self.check(_lib.lgr_match_last_stats(self.h, out))
        return dict(items_ab=out[0], dense_ab=out[1], items_ba=out[2], dense_ba=out[3], sub_cols=out[4], rg_rows=out[5])

    def match_work(self):
        """fraction of the (row block x column stage) tiles the MFMA passes of the last match call computed"""
        f = C.c_double(1.0)
        self.check(_lib.lgr_match_last_work(self.h, C.byref(f)))
        return f.value

    def selfcheck_rcp(self, lo, hi):
        """(differing, tested) over every float in [lo, hi]: the FPFH weighting kernel's reciprocal against the IEEE division"""
        out = (C.c_ulonglong * 2)()
        lo_b, hi_b = (int(np.float32(v).view(np.uint32)) for v in (lo, hi))
        self.check(_lib.lgr_selfcheck_rcp(self.h, C.c_uint(lo_b), C.c_uint(hi_b), out))
        return int(out[0]), int(out[1])

    def match_lbstats(self):
        """(zero, finite) lower bounds among the (row block, leaf) pairs of the last pruned match call: what lgr_match_options.auto_dense decides on"""
        out = (C.c_double * 2)()
        self.check(_lib.lgr_match_last_lbstats(self.h, out))
        return out[0], out[1]

    def match_irregular(self):
        """(query side, train side, gave up) of the last match call: rows that went through the exact side scan (lgr_match_options.irregular_rows)"""
        out = (C.c_uint * 3)()
        self.check(_lib.lgr_match_last_irregular(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def selfcheck_philox(self, key, counter4):
        """one Philox4x32-10 block from the device's generator (full counter; key = k0 | k1 << 32)"""
        c = (C.c_uint32 * 4)(*[int(x) for x in counter4])
        out = (C.c_uint32 * 4)()
        self.check(_lib.lgr_selfcheck_philox(self.h, C.c_uint64(key), c, out))
        return list(out)

    def selfcheck_libm(self, fn, a, b=None):
        """csrc/lgr_libm.cuh (glibc 2.35's float acosf / atanf / atan2f / sinf / cosf restated) evaluated on the device, element-wise"""
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(a if b is None else b, np.float32)
        out = np.empty_like(a)
        self.check(_lib.lgr_selfcheck_libm(self.h, int(fn), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.c_longlong(a.size), out.ctypes.data_as(C.c_void_p)))
        return out

    def match_issued(self):
        """the same with the stages of every pass summed (>= match_work): the MFMA work that was issued"""
        out = (C.c_double * 2)()
        self.check(_lib.lgr_match_last_issued(self.h, out))
        return out[0]

    def match_issued_pairs(self):
        """(row, column) element pairs of the padded operands in the stages the passes of the last match call issued"""
        out = (C.c_double * 2)()
        self.check(_lib.lgr_match_last_issued(self.h, out))
        return out[1]

    def match_pairs(self):
        """(query->train, train->query) pairs the MFMA re-filter of the rerank handed to the exact distance in the last match call"""
        out = (C.c_uint * 2)()
        self.check(_lib.lgr_match_last_pairs(self.h, out))
        return out[0], out[1]

    def match_coarse(self):
        """(tiles tested, tiles abandoned) by the coarse rejection inside the MFMA filter kernel in the last match call"""
        out = (C.c_double * 2)()
        self.check(_lib.lgr_match_last_coarse(self.h, out))
        return out[0], out[1]

    def match_shell(self):
        """tiles of the swept stages the shell test left out before any MFMA step in the last match call"""
        out = C.c_double()
        self.check(_lib.lgr_match_last_shell(self.h, C.byref(out)))
        return out.value

    def match_format(self):
        """'f16' (split operands on the f16 MFMA, K = 112), 'f16r' (the same on 30 rotated coordinates, K = 96) or 'f32'
        for the last match call"""
        v = C.c_int(0)
        self.check(_lib.lgr_match_last_format(self.h, C.byref(v)))
        return {0: "f32", 1: "f16", 2: "f16r"}[v.value]

    def match_check(self):
        """(rows, cols) worst |filtered - exact| / eps of the last match call run under set_match_options(self_check=1), or -1"""
        out = (C.c_double * 2)()
        self.check(_lib.lgr_match_last_check(self.h, out))
        return out[0], out[1]

    def match_check_cover(self):
        """what the self-check of the last match call covered, per direction: {"rows": {...}, "cols": {...}} with the counts of
        "entries" checked, "upper" (upper side tested), "waived" (upper side waived by the coarse rejection) and "colstage" (a row
        guaranteed only through the per-stage column criterion); -1 when that direction was not checked"""
        out = (C.c_ulonglong * 8)()
        self.check(_lib.lgr_match_last_check_cover(self.h, out))
        keys = ("entries", "upper", "waived", "colstage")
        return {d: {k: (-1 if out[4 * j + n] == 0xFFFFFFFFFFFFFFFF else int(out[4 * j + n])) for n, k in enumerate(keys)}
                for j, d in enumerate(("rows", "cols"))}

    def match_pack_check(self):
        """(compared, differing) pieces of the packing kernel's output against the reference packing kernel's in the last match call run
        under set_match_options(self_check=...): 16-byte pieces of fragments and norms and tile shells; (-1, -1) when it did not run"""
        out = (C.c_ulonglong * 2)()
        self.check(_lib.lgr_match_last_pack_check(self.h, out))
        return tuple(-1 if v == 0xFFFFFFFFFFFFFFFF else int(v) for v in out)

    def match_kernel_ms(self):
        ms = C.c_float(0)
        self.check(_lib.lgr_match_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    # ---- geometry stages ------------------------------------------------------------------------------------
    def bbox(self, pts):
        out = self.empty((6,), self.torch.float32)
        self.check(_lib.lgr_bbox_dev(self.h, _ptr(pts), pts.shape[0], _ptr(out)))
        return out

    def knn(self, q, pts, k):
        torch = self.torch
        idx = self.empty((q.shape[0], k), torch.int32); d2 = self.empty((q.shape[0], k), torch.float32)
        self.check(_lib.lgr_knn_dev(self.h, _ptr(q), q.shape[0], _ptr(pts), pts.shape[0], int(k), _ptr(idx), _ptr(d2)))
        return idx, d2

    def smoothed_densities(self, pts, k=2):
        out = self.empty((pts.shape[0],), self.torch.float32)
        self.check(_lib.lgr_smoothed_densities_dev(self.h, _ptr(pts), pts.shape[0], int(k), _ptr(out)))
        return out

    def hash_order(self, hashes, reserve=0):
        """iteration order of a libstdc++ hash container whose element e (numbered by first insertion) has hash code hashes[e] (cuda
        uint64 / int64 tensor): int32 element ids.  reserve: 0, or the argument (>= n) of a reserve() before the first insertion."""
        n = int(hashes.shape[0])
        out = self.empty((n,), self.torch.int32)
        self.check(_lib.lgr_hash_order_dev(self.h, _ptr(hashes) if n else None, n, C.c_longlong(int(reserve)), _ptr(out) if n else None))
        return out

    def selfcheck_hash_order(self, n, spread=2000, seed=1, reserve=0):
        """mismatches (must be 0) between a real std::unordered_map of n drawn voxel keys and the device order (include/lgr.h)"""
        out = C.c_longlong(-1)
        self.check(_lib.lgr_selfcheck_hash_order(self.h, int(n), int(spread), C.c_uint64(int(seed)), C.c_longlong(int(reserve)), C.byref(out)))
        return out.value

    def preprocess(self, pts, vp=None, normals_available=False, order=ORDER_CANONICAL):
        """order = ORDER_REFERENCE: the reference's unordered_set / unordered_map numbering (lgr_preprocess_order_dev)"""
        out = self.empty((pts.shape[0], 12), self.torch.float32)
        n = C.c_int(0)
        voxel = C.c_float(0)
        v = (C.c_float * 3)(*[float(x) for x in vp]) if vp is not None else None
        if order == ORDER_CANONICAL:
            self.check(_lib.lgr_preprocess_dev(self.h, _ptr(pts), pts.shape[0], v, int(normals_available), _ptr(out), C.byref(n), C.byref(voxel)))
        else:
            self.check(_lib.lgr_preprocess_order_dev(self.h, _ptr(pts), pts.shape[0], v, int(normals_available), int(order), _ptr(out), C.byref(n),
                                                     C.byref(voxel)))
        return out[: n.value], voxel.value

    def preprocess_host(self, pts, vp=None, normals_available=False, order=ORDER_CANONICAL):
        pts = np.ascontiguousarray(pts, np.float32)
        out = np.zeros_like(pts)
        n = C.c_int(0)
        voxel = C.c_float(0)
        v = (C.c_float * 3)(*[float(x) for x in vp]) if vp is not None else None
        self.check(_lib.lgr_preprocess(self.h, _ptr(pts), pts.shape[0], v, int(normals_available), int(order), _ptr(out), C.byref(n), C.byref(voxel)))
        return out[: n.value].copy(), voxel.value

    def dedupe(self, pts, order=ORDER_CANONICAL):
        out = self.empty((max(pts.shape[0], 1), 12), self.torch.float32)
        n = C.c_int(0)
        if order == ORDER_CANONICAL:
            self.check(_lib.lgr_dedupe_dev(self.h, _ptr(pts), pts.shape[0], _ptr(out), C.byref(n)))
        else:
            self.check(_lib.lgr_dedupe_order_dev(self.h, _ptr(pts), pts.shape[0], int(order), _ptr(out), C.byref(n)))
        return out[: n.value]

    def cloud_density(self, pts, quantile=0.8):
        v = C.c_float(0)
        self.check(_lib.lgr_cloud_density_dev(self.h, _ptr(pts), pts.shape[0], C.c_float(quantile), C.byref(v)))
        return v.value

    def iss_keypoints(self, pts, radius, gamma21=0.975, gamma32=0.975, min_neighbors=4):
        idx = self.empty((max(pts.shape[0], 1),), self.torch.int32)
        n = C.c_int(0)
        self.check(_lib.lgr_iss_keypoints_dev(self.h, _ptr(pts), pts.shape[0], C.c_float(radius), C.c_float(gamma21), C.c_float(gamma32),
                                              int(min_neighbors), _ptr(idx), C.byref(n)))
        return idx[: n.value]

    def downsample(self, pts, voxel, order=ORDER_CANONICAL, out=None):
        """order = ORDER_REFERENCE: the voxels in the reference's unordered_map order; out (optional) may be pts itself"""
        if out is None:
            out = self.empty((pts.shape[0], 12), self.torch.float32)
        n = C.c_int(0)
        if order == ORDER_CANONICAL:
            self.check(_lib.lgr_downsample_dev(self.h, _ptr(pts), pts.shape[0], C.c_float(voxel), _ptr(out), C.byref(n)))
        else:
            self.check(_lib.lgr_downsample_order_dev(self.h, _ptr(pts), pts.shape[0], C.c_float(voxel), int(order), _ptr(out), C.byref(n)))
        return out[: n.value]

    def downsample_host(self, pts, voxel, order=ORDER_CANONICAL):
        pts = np.ascontiguousarray(pts, np.float32)
        out = np.zeros_like(pts)
        n = C.c_int(0)
        self.check(_lib.lgr_downsample(self.h, _ptr(pts), pts.shape[0], C.c_float(voxel), int(order), _ptr(out), C.byref(n)))
        return out[: n.value].copy()

    def normals_knn(self, pts, k=30, surf=None, vp=None):
        """in place on the cuda tensor pts"""
        v = (C.c_float * 3)(*[float(x) for x in vp]) if vp is not None else None
        self.check(_lib.lgr_normals_knn_dev(self.h, _ptr(pts), pts.shape[0], _ptr(surf), 0 if surf is None else surf.shape[0],
                                            int(k), v, 0))
        return pts

    def fpfh(self, kps, surf, radius):
        out = self.empty((kps.shape[0], 33), self.torch.float32)
        self.check(_lib.lgr_fpfh_dev(self.h, _ptr(kps), kps.shape[0], _ptr(surf), surf.shape[0], C.c_float(radius), _ptr(out)))
        return out

    def shot_lrf(self, kps, surf, radius):
        """SHOT local reference frames: cuda float32 [m, 9] (x, y, z axes; NaN rows where no frame exists)."""
        out = self.empty((kps.shape[0], 9), self.torch.float32)
        self.check(_lib.lgr_shot_lrf_dev(self.h, _ptr(kps), kps.shape[0], _ptr(surf), surf.shape[0], C.c_float(radius), _ptr(out)))
        return out

    def shot(self, kps, surf, radius, lrf=None, with_lrf=False):
        """SHOT352 rows: cuda float32 [m, 352]; lrf (cuda [m, 9]) = given frames, None = estimated.  with_lrf: also the frames used."""
        out = self.empty((kps.shape[0], 352), self.torch.float32)
        lo = self.empty((kps.shape[0], 9), self.torch.float32) if with_lrf else None
        self.check(_lib.lgr_shot_dev(self.h, _ptr(kps), kps.shape[0], _ptr(surf), surf.shape[0], C.c_float(radius),
                                     _ptr(None if lrf is None else lrf.contiguous()), _ptr(out), _ptr(lo)))
        return (out, lo) if with_lrf else out

    def shot_host(self, kps, surf, radius, lrf=None):
        kps = np.ascontiguousarray(kps, np.float32); surf = np.ascontiguousarray(surf, np.float32)
        out = np.zeros((kps.shape[0], 352), np.float32)
        lo = np.zeros((kps.shape[0], 9), np.float32)
        lrf = None if lrf is None else np.ascontiguousarray(lrf, np.float32)
        self.check(_lib.lgr_shot(self.h, _ptr(kps), kps.shape[0], _ptr(surf), surf.shape[0], C.c_float(radius), _ptr(lrf), _ptr(out), _ptr(lo)))
        return out, lo

    def match_shot(self, q, t, block=10000):
        """exact matchBF on [m, 352] rows: (idx int32 [mq], dist float32 [mq])."""
        torch = self.torch
        q = q.contiguous(); t = t.contiguous()
        idx = self.empty((q.shape[0],), torch.int32)
        dist = self.empty((q.shape[0],), torch.float32)
        self.check(_lib.lgr_match_shot_dev(self.h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), _ptr(idx), _ptr(dist)))
        return idx, dist

    def match2_shot(self, a, b, block=10000):
        torch = self.torch
        a = a.contiguous(); b = b.contiguous()
        ab_i = self.empty((a.shape[0],), torch.int32); ab_d = self.empty((a.shape[0],), torch.float32)
        ba_i = self.empty((b.shape[0],), torch.int32); ba_d = self.empty((b.shape[0],), torch.float32)
        self.check(_lib.lgr_match2_shot_dev(self.h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], int(block),
                                            _ptr(ab_i), _ptr(ab_d), _ptr(ba_i), _ptr(ba_d)))
        return ab_i, ab_d, ba_i, ba_d

    def match_shot_host(self, q, t, block=10000):
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        idx = np.zeros(q.shape[0], np.int32); dist = np.zeros(q.shape[0], np.float32)
        self.check(_lib.lgr_match_shot(self.h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), _ptr(idx), _ptr(dist)))
        return idx, dist

    # ---- randomness > 1: the k nearest rows (row length 33, 135 or 352) and the vote among a query's candidates ----------------------
    def match_knn(self, q, t, block=10000, k=2):
        """exact matchBF with randomness = k on cuda float32 [m, 33 | 135 | 352] rows: (idx int32 [mq, k], dist float32 [mq, k]),
        a query's matches in list order, then -1 / 0.  set_knn_filter chooses how every row length is swept, never the result."""
        torch = self.torch
        q = q.contiguous(); t = t.contiguous()
        idx = self.empty((q.shape[0], max(int(k), 0)), torch.int32)
        dist = self.empty((q.shape[0], max(int(k), 0)), torch.float32)
        self.check(_lib.lgr_match_knn_dev(self.h, int(q.shape[1]), _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_knn2(self, a, b, block=10000, k=2):
        """match_knn in both directions, the rows packed once (under set_knn_filter: one centre and scale for the call):
        (ab_idx, ab_dist, ba_idx, ba_dist)"""
        torch = self.torch
        a = a.contiguous(); b = b.contiguous()
        kk = max(int(k), 0)
        ab_i = self.empty((a.shape[0], kk), torch.int32); ab_d = self.empty((a.shape[0], kk), torch.float32)
        ba_i = self.empty((b.shape[0], kk), torch.int32); ba_d = self.empty((b.shape[0], kk), torch.float32)
        self.check(_lib.lgr_match_knn2_dev(self.h, int(a.shape[1]), _ptr(a), a.shape[0], _ptr(b), b.shape[0], int(block), int(k),
                                           _ptr(ab_i), _ptr(ab_d), _ptr(ba_i), _ptr(ba_d)))
        return ab_i, ab_d, ba_i, ba_d

    # ---- how the k-nearest matcher sweeps rows of 33, 135 and 352 floats (never what it returns) -----------------------------------------
    def set_knn_filter(self, mode=-1, self_check=0):
        """mode -1 auto (filtered from the row length's crossover size), 0 exact scan, 1 filtered at any size; self_check 0 / 1 (test
        sizes).  Holds for match_knn* / match_ratio* and randomness > 1 / matching ratio in the pipeline, on FPFH, SHOT and RoPS rows;
        set_dense_filter (the one-match matchers) is a separate switch."""
        self.check(_lib.lgr_ctx_set_knn_filter(self.h, int(mode), int(self_check)))

    def knn_filter(self):
        """(mode, self_check) now in force"""
        m, c = C.c_int(0), C.c_int(0)
        self.check(_lib.lgr_ctx_get_knn_filter(self.h, C.byref(m), C.byref(c)))
        return m.value, c.value

    def match_knn_last(self):
        """the eight counters of lgr_match_knn_last for the last k-nearest call of any row length, exact scans included ([6]: -1 when the
        self-check did not run)"""
        out = (C.c_ulonglong * 8)()
        self.check(_lib.lgr_match_knn_last(self.h, out))
        return [-1 if v == 0xFFFFFFFFFFFFFFFF else int(v) for v in out]

    def match_knn_last_check(self):
        """worst |filtered - canonical d2| / bound over the pairs the self-check of the last k-nearest call covered, or -1"""
        out = C.c_double(-1)
        self.check(_lib.lgr_match_knn_last_check(self.h, C.byref(out)))
        return out.value

    # ---- how 135 / 352-float rows are swept by the one-match matcher (never what it returns) ---------------------------------------------
    def set_dense_filter(self, mode=-1, self_check=0):
        """mode -1 auto (filtered from the crossover size), 0 exact scan, 1 filtered at any size; self_check 0 / 1 (test sizes)"""
        self.check(_lib.lgr_ctx_set_dense_filter(self.h, int(mode), int(self_check)))

    def dense_filter(self):
        """(mode, self_check) now in force"""
        m, c = C.c_int(0), C.c_int(0)
        self.check(_lib.lgr_ctx_get_dense_filter(self.h, C.byref(m), C.byref(c)))
        return m.value, c.value

    def match_dense_last(self):
        """the eight counters of lgr_match_dense_last for the last one-match call on 135 / 352-float rows ([6]: -1 when the self-check did not run)"""
        out = (C.c_ulonglong * 8)()
        self.check(_lib.lgr_match_dense_last(self.h, out))
        return [-1 if v == 0xFFFFFFFFFFFFFFFF else int(v) for v in out]

    def match_dense_last_check(self):
        """worst |filtered - canonical d2| / bound over the pairs the self-check of the last one-match call on long rows covered, or -1"""
        out = C.c_double(-1)
        self.check(_lib.lgr_match_dense_last_check(self.h, C.byref(out)))
        return out.value

    def match_knn_host(self, q, t, block=10000, k=2):
        """match_knn on numpy rows of 33, 135 or 352 floats (uploaded, matched under set_knn_filter, downloaded)"""
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        idx = np.zeros((q.shape[0], max(int(k), 0)), np.int32); dist = np.zeros((q.shape[0], max(int(k), 0)), np.float32)
        self.check(_lib.lgr_match_knn(self.h, int(q.shape[1]), _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    # ---- the ratio test on a query's k-nearest list (MATCH_RATIO): on a table, and fused into the sweep ------------------------------
    def ratio_test(self, knn_idx, knn_dist, threshold=MATCHING_RATIO_THRESHOLD):
        """cuda int32 / float32 [mq, k] lists of match_knn -> (idx int32 [mq], dist float32 [mq]): a list's first entry iff the list
        has k entries and dist[0] * threshold < dist[k - 1] (f32, strict), else -1 / 0."""
        torch = self.torch
        ki = knn_idx.contiguous(); kd = knn_dist.contiguous()
        idx = self.empty((ki.shape[0],), torch.int32); dist = self.empty((ki.shape[0],), torch.float32)
        self.check(_lib.lgr_ratio_test_dev(self.h, _ptr(ki), _ptr(kd), ki.shape[0], int(ki.shape[1]), C.c_float(threshold), _ptr(idx), _ptr(dist)))
        return idx, dist

    def ratio_test_host(self, knn_idx, knn_dist, threshold=MATCHING_RATIO_THRESHOLD):
        ki = np.ascontiguousarray(knn_idx, np.int32); kd = np.ascontiguousarray(knn_dist, np.float32)
        idx = np.zeros(ki.shape[0], np.int32); dist = np.zeros(ki.shape[0], np.float32)
        self.check(_lib.lgr_ratio_test(self.h, _ptr(ki), _ptr(kd), ki.shape[0], int(ki.shape[1]), C.c_float(threshold), _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_ratio(self, q, t, block=10000, k=2, threshold=MATCHING_RATIO_THRESHOLD):
        """match_knn and ratio_test in one sweep (the [mq, k] table is never written): (idx int32 [mq], dist float32 [mq]); rows of 33,
        135 or 352 floats, swept as set_knn_filter says"""
        torch = self.torch
        q = q.contiguous(); t = t.contiguous()
        idx = self.empty((q.shape[0],), torch.int32); dist = self.empty((q.shape[0],), torch.float32)
        self.check(_lib.lgr_match_ratio_dev(self.h, int(q.shape[1]), _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), int(k), C.c_float(threshold),
                                            _ptr(idx), _ptr(dist)))
        return idx, dist

    def match_ratio_host(self, q, t, block=10000, k=2, threshold=MATCHING_RATIO_THRESHOLD):
        """match_ratio on numpy rows of 33, 135 or 352 floats"""
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        idx = np.zeros(q.shape[0], np.int32); dist = np.zeros(q.shape[0], np.float32)
        self.check(_lib.lgr_match_ratio(self.h, int(q.shape[1]), _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), int(k), C.c_float(threshold),
                                        _ptr(idx), _ptr(dist)))
        return idx, dist

    def vote_matches(self, cand_idx, cand_dist, train_pts, iss_radius):
        """the vote of include/matching.h:327-352: cuda int32 / float32 [mq, width] candidates (entries < 0 skipped), cuda float32
        [mt, 12] train key points -> (idx int32 [mq], dist float32 [mq])"""
        torch = self.torch
        ci = cand_idx.contiguous(); cd = cand_dist.contiguous(); tp = train_pts.contiguous()
        idx = self.empty((ci.shape[0],), torch.int32); dist = self.empty((ci.shape[0],), torch.float32)
        self.check(_lib.lgr_vote_matches_dev(self.h, _ptr(ci), _ptr(cd), ci.shape[0], int(ci.shape[1]), _ptr(tp), tp.shape[0], C.c_float(iss_radius),
                                             _ptr(idx), _ptr(dist)))
        return idx, dist

    def vote_matches_host(self, cand_idx, cand_dist, train_pts, iss_radius):
        ci = np.ascontiguousarray(cand_idx, np.int32); cd = np.ascontiguousarray(cand_dist, np.float32)
        tp = np.ascontiguousarray(train_pts, np.float32)
        idx = np.zeros(ci.shape[0], np.int32); dist = np.zeros(ci.shape[0], np.float32)
        self.check(_lib.lgr_vote_matches(self.h, _ptr(ci), _ptr(cd), ci.shape[0], int(ci.shape[1]), _ptr(tp), tp.shape[0], C.c_float(iss_radius),
                                         _ptr(idx), _ptr(dist)))
        return idx, dist

    def gravity_lrf(self, kps, surf, radius):
        """gravity-aligned frames: cuda float32 [m, 9]; SHOT frames where the normal is within 0.04 rad of the vertical (or NaN)."""
        out = self.empty((kps.shape[0], 9), self.torch.float32)
        self.check(_lib.lgr_gravity_lrf_dev(self.h, _ptr(kps), kps.shape[0], _ptr(surf), surf.shape[0], C.c_float(radius), _ptr(out)))
        return out

    def gravity_lrf_host(self, kps, surf, radius):
        kps = np.ascontiguousarray(kps, np.float32); surf = np.ascontiguousarray(surf, np.float32)
        out = np.zeros((kps.shape[0], 9), np.float32)
        self.check(_lib.lgr_gravity_lrf(self.h, _ptr(kps), kps.shape[0], _ptr(surf), surf.shape[0], C.c_float(radius), _ptr(out)))
        return out

    def rops(self, kps, surf, radius, lrf):
        """RoPS135 rows on the given frames (cuda [m, 9]): cuda float32 [m, 135]."""
        out = self.empty((kps.shape[0], 135), self.torch.float32)
        self.check(_lib.lgr_rops_dev(self.h, _ptr(kps), kps.shape[0], _ptr(surf), surf.shape[0], C.c_float(radius), _ptr(lrf.contiguous()),
                                     _ptr(out)))
        return out

    def rops_host(self, kps, surf, radius, lrf):
        kps = np.ascontiguousarray(kps, np.float32); surf = np.ascontiguousarray(surf, np.float32)
        lrf = np.ascontiguousarray(lrf, np.float32)
        out = np.zeros((kps.shape[0], 135), np.float32)
        self.check(_lib.lgr_rops(self.h, _ptr(kps), kps.shape[0], _ptr(surf), surf.shape[0], C.c_float(radius), _ptr(lrf), _ptr(out)))
        return out

    def match_rops(self, q, t, block=10000):
        """exact matchBF on [m, 135] rows: (idx int32 [mq], dist float32 [mq])."""
        torch = self.torch
        q = q.contiguous(); t = t.contiguous()
        idx = self.empty((q.shape[0],), torch.int32)
        dist = self.empty((q.shape[0],), torch.float32)
        self.check(_lib.lgr_match_rops_dev(self.h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), _ptr(idx), _ptr(dist)))
        return idx, dist

    def match2_rops(self, a, b, block=10000):
        torch = self.torch
        a = a.contiguous(); b = b.contiguous()
        ab_i = self.empty((a.shape[0],), torch.int32); ab_d = self.empty((a.shape[0],), torch.float32)
        ba_i = self.empty((b.shape[0],), torch.int32); ba_d = self.empty((b.shape[0],), torch.float32)
        self.check(_lib.lgr_match2_rops_dev(self.h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], int(block),
                                            _ptr(ab_i), _ptr(ab_d), _ptr(ba_i), _ptr(ba_d)))
        return ab_i, ab_d, ba_i, ba_d

    def match_rops_host(self, q, t, block=10000):
        q = np.ascontiguousarray(q, np.float32); t = np.ascontiguousarray(t, np.float32)
        idx = np.zeros(q.shape[0], np.int32); dist = np.zeros(q.shape[0], np.float32)
        self.check(_lib.lgr_match_rops(self.h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], int(block), _ptr(idx), _ptr(dist)))
        return idx, dist

    def fpfh_host(self, kps, surf, radius):
        kps = np.ascontiguousarray(kps, np.float32); surf = np.ascontiguousarray(surf, np.float32)
        out = np.zeros((kps.shape[0], 33), np.float32)
        self.check(_lib.lgr_fpfh(self.h, _ptr(kps), kps.shape[0], _ptr(surf), surf.shape[0], C.c_float(radius), _ptr(out)))
        return out

    # ---- filters / correspondence search -------------------------------------------------------------------
    def filter(self, matching_id, src, tgt, ij, dij, ji, dji, distance_thr, cluster_k=40):
        out = self.empty((src.shape[0], 4), self.torch.int32)
        n = C.c_int(0)
        self.check(_lib.lgr_filter_dev(self.h, int(matching_id), _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0],
                                       _ptr(ij), _ptr(dij), _ptr(ji), _ptr(dji), C.c_float(distance_thr), int(cluster_k),
                                       _ptr(out), C.byref(n)))
        self._join()
        return out[: n.value].cpu().numpy().view(CORR_DTYPE).reshape(-1)

    def correspondences(self, src, tgt, params, descriptor="fpfh"):
        """descriptor: 'fpfh' (lgr_correspondences_dev) or 'shot' / 'rops' / a FeatureParams (lgr_correspondences_ex_dev)."""
        out = self.empty((src.shape[0], 4), self.torch.int32)
        n = C.c_int(0)
        if isinstance(descriptor, str) and descriptor == "fpfh":
            self.check(_lib.lgr_correspondences_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params),
                                                    _ptr(out), C.byref(n)))
        else:
            f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
            self.check(_lib.lgr_correspondences_ex_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params),
                                                       C.byref(f), _ptr(out), C.byref(n)))
        return out[: n.value]

    # ---- prepared clouds (lgr_cloud: the per-cloud half of the search, run once) ----------------------------
    def _prepare_cloud(self, fn, pts, params, side, descriptor):
        f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
        h = C.c_void_p()
        self.check(fn(self.h, _ptr(pts), pts.shape[0], int(side), C.byref(params), C.byref(f), C.byref(h)))
        return PreparedCloud(self, h)

    def prepare_cloud(self, pts, params, side=0, descriptor="fpfh"):
        """lgr_cloud_prepare_dev: pts a cuda float32 [n,12] (copied: the object owns its memory).  side 0 / 1: which of the vp_* /
        iss_radius_* fields of params the cloud is prepared with."""
        return self._prepare_cloud(_lib.lgr_cloud_prepare_dev, pts, params, side, descriptor)

    def prepare_cloud_host(self, pts, params, side=0, descriptor="fpfh"):
        return self._prepare_cloud(_lib.lgr_cloud_prepare, np.ascontiguousarray(pts, np.float32), params, side, descriptor)

    def correspondences_prepared(self, a, b, params, descriptor="fpfh"):
        """lgr_correspondences_prepared_dev on two PreparedCloud: what correspondences() returns for their clouds."""
        out = self.empty((max(a.info().n, 1), 4), self.torch.int32)
        n = C.c_int(0)
        f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
        self.check(_lib.lgr_correspondences_prepared_dev(self.h, a.h, b.h, C.byref(params), C.byref(f), _ptr(out), C.byref(n)))
        return out[: n.value]

    def align_prepared(self, a, b, params, descriptor="fpfh", metric_params=None):
        """lgr_align_prepared: what align_ex2() returns for the two clouds, apart from the time fields."""
        res = Result()
        f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
        self.check(_lib.lgr_align_prepared(self.h, a.h, b.h, C.byref(params), C.byref(f),
                                           C.byref(metric_params) if metric_params is not None else None, C.byref(res)))
        return res

    def stage_ms(self):
        out = (C.c_float * 12)()
        _lib.lgr_ctx_stage_ms(self.h, out)
        return list(out)

    # ---- RANSAC ---------------------------------------------------------------------------------------------
    def _corr_dev(self, corr):
        if isinstance(corr, np.ndarray):
            return self.torch.from_numpy(np.ascontiguousarray(corr).view(np.int32).reshape(-1, 4)).to(self._dev())
        return corr

    def ransac_samples(self, seed, first, n, n_corr, n_samples=3):
        out = self.empty((n, n_samples), self.torch.int32)
        self.check(_lib.lgr_ransac_samples_n_dev(self.h, C.c_uint64(seed), int(first), int(n), int(n_corr), int(n_samples), _ptr(out)))
        return out

    def evaluate(self, src, tgt, corr, T, metric_id=METRIC_UNIFORMITY, score_id=SCORE_MSE):
        corr = self._corr_dev(corr)
        c = corr.shape[0]
        mask = self.empty((max(c, 1),), self.torch.uint8)
        T16 = (C.c_float * 16)(*np.asarray(T, np.float32).T.reshape(16).tolist())
        ni, rm, me = C.c_int(0), C.c_float(0), C.c_float(0)
        self.check(_lib.lgr_evaluate_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), c, T16,
                                         int(metric_id), int(score_id), _ptr(mask), C.byref(ni), C.byref(rm), C.byref(me)))
        self._join()
        return mask[:c].cpu().numpy(), ni.value, rm.value, me.value

    def choose_best_hypothesis(self, src, tgt, corr, tns):
        corr = self._corr_dev(corr)
        n = len(tns)
        buf = np.ascontiguousarray(np.stack([np.asarray(T, np.float32).T.reshape(16) for T in tns]), np.float32) if n else np.zeros((1, 16), np.float32)
        out = (C.c_float * 16)()
        bi = C.c_int(-1)
        uni = np.zeros(max(n, 1), np.float32)
        self.check(_lib.lgr_choose_best_hypothesis_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), corr.shape[0],
                                                       _ptr(buf), n, out, C.byref(bi), _ptr(uni)))
        return bi.value, np.array(out, np.float32).reshape(4, 4).T.copy(), uni[:n].copy()

    def evaluate_plane(self, src, tgt, T, score_id=SCORE_CONSTANT, seed=566, counter=0, with_pairs=False):
        T16 = (C.c_float * 16)(*np.asarray(T, np.float32).T.reshape(16).tolist())
        n, rm, me, th, npairs = C.c_int(0), C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        pairs = np.zeros((max(int(0.01 * src.shape[0]), 1), 2), np.int32) if with_pairs else None
        self.check(_lib.lgr_evaluate_plane_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], T16, int(score_id), C.c_uint64(seed),
                                               C.c_uint32(counter), C.byref(n), C.byref(rm), C.byref(me), C.byref(th), _ptr(pairs), C.byref(npairs)))
        out = dict(n_inl=n.value, rmse=rm.value, metric=me.value, thr=th.value)
        if with_pairs:
            out["pairs"] = pairs[: npairs.value].copy()
        return out

    def evaluate_plane_weighted(self, src, tgt, T, weights, weights_sum, score_id=SCORE_CONSTANT, seed=566, counter=0, with_pairs=False):
        """lgr_evaluate_plane_weighted_dev: weights = cuda float32 [ns], weights_sum = the metric's denominator."""
        T16 = (C.c_float * 16)(*np.asarray(T, np.float32).T.reshape(16).tolist())
        n, rm, me, th, npairs = C.c_int(0), C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        pairs = np.zeros((max(int(0.01 * src.shape[0]), 1), 2), np.int32) if with_pairs else None
        self.check(_lib.lgr_evaluate_plane_weighted_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], T16, int(score_id), C.c_uint64(seed),
                                                        C.c_uint32(counter), _ptr(weights.contiguous()), C.c_float(weights_sum), C.byref(n), C.byref(rm),
                                                        C.byref(me), C.byref(th), _ptr(pairs), C.byref(npairs)))
        out = dict(n_inl=n.value, rmse=rm.value, metric=me.value, thr=th.value)
        if with_pairs:
            out["pairs"] = pairs[: npairs.value].copy()
        return out

    def weights(self, pts, weight="constant", nr_points=30, with_sum=True):
        """the weight map of weight (name or LGR_WEIGHT_*) on cuda points [n, 12]: (cuda float32 [n], weights_sum or None)."""
        wid = WEIGHT_IDS.get(weight, weight) if isinstance(weight, str) else int(weight)
        out = self.empty((max(pts.shape[0], 1),), self.torch.float32)
        s = C.c_float(0)
        self.check(_lib.lgr_weights_dev(self.h, _ptr(pts), pts.shape[0], int(wid), int(nr_points), _ptr(out), C.byref(s) if with_sum else None))
        return out[: pts.shape[0]], (s.value if with_sum else None)

    def weights_host(self, pts, weight="constant", nr_points=30):
        pts = np.ascontiguousarray(pts, np.float32)
        wid = WEIGHT_IDS.get(weight, weight) if isinstance(weight, str) else int(weight)
        out = np.zeros(max(pts.shape[0], 1), np.float32)
        s = C.c_float(0)
        self.check(_lib.lgr_weights(self.h, _ptr(pts), pts.shape[0], int(wid), int(nr_points), _ptr(out), C.byref(s)))
        return out[: pts.shape[0]], s.value

    def principal_curvatures(self, pts, k=30):
        """pcl::PrincipalCurvaturesEstimation over k neighbours in the cloud itself: (pc1, pc2), cuda float32 [n] each."""
        n = pts.shape[0]
        pc1 = self.empty((max(n, 1),), self.torch.float32); pc2 = self.empty((max(n, 1),), self.torch.float32)
        self.check(_lib.lgr_principal_curvatures_dev(self.h, _ptr(pts), n, int(k), _ptr(pc1), _ptr(pc2)))
        return pc1[:n], pc2[:n]

    def ransac_ex(self, src, tgt, corr, params, mparams=None):
        """lgr_ransac_ex_dev (mparams: a MetricParams, None = the defaults)."""
        corr = self._corr_dev(corr)
        c = corr.shape[0]
        res = Result()
        mask = self.empty((max(c, 1),), self.torch.uint8)
        self.check(_lib.lgr_ransac_ex_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), c,
                                          C.byref(params), C.byref(mparams) if mparams is not None else None, C.byref(res), _ptr(mask)))
        self._join()
        return res, mask[:c].cpu().numpy()

    def ransac_plane_gate(self):
        """(hypotheses scored on a sparse plane subset, those of them the gate abandoned) in the last ransac / ransac_ex / align call"""
        out = (C.c_uint * 2)()
        self.check(_lib.lgr_ransac_last_plane_gate(self.h, out))
        return out[0], out[1]

    def ransac_replay(self, src, tgt, corr, params, triples):
        torch = self.torch
        corr = self._corr_dev(corr)
        n = triples.shape[0]
        assert triples.shape[1] == params.n_samples, "one row of params.n_samples correspondence indices per hypothesis"
        ok = self.empty((n,), torch.uint8); Ts = self.empty((n, 16), torch.float32)
        ninl = self.empty((n,), torch.int32); met = self.empty((n,), torch.float32)
        self.check(_lib.lgr_ransac_replay_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), corr.shape[0],
                                              C.byref(params), _ptr(triples), n, _ptr(ok), _ptr(Ts), _ptr(ninl), _ptr(met)))
        self._join()
        return ok.cpu().numpy(), Ts.cpu().numpy(), ninl.cpu().numpy(), met.cpu().numpy()

    def ransac(self, src, tgt, corr, params):
        corr = self._corr_dev(corr)
        c = corr.shape[0]
        res = Result()
        mask = self.empty((max(c, 1),), self.torch.uint8)
        self.check(_lib.lgr_ransac_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), c,
                                       C.byref(params), C.byref(res), _ptr(mask)))
        self._join()
        return res, mask[:c].cpu().numpy()

    def ransac_multi(self, src, tgt, corr, params, max_set=64):
        """lgr_ransac_multi_dev: the loop with the set of distinct hypotheses -> (Result, [Hypothesis] in set order, best_index)."""
        corr = self._corr_dev(corr)
        res = Result()
        out = (Hypothesis * max(int(max_set), 1))()
        n, bi = C.c_int(0), C.c_int(-1)
        self.check(_lib.lgr_ransac_multi_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), corr.shape[0],
                                             C.byref(params), int(max_set), C.byref(res), out, C.byref(n), C.byref(bi)))
        return res, [out[i] for i in range(n.value)], bi.value

    def ransac_multi_host(self, src, tgt, corr, params, max_set=64):
        """lgr_ransac_multi: clouds [n, 12] float32 and correspondences (CORR_DTYPE) in host memory."""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        corr = np.ascontiguousarray(corr)
        res = Result()
        out = (Hypothesis * max(int(max_set), 1))()
        n, bi = C.c_int(0), C.c_int(-1)
        self.check(_lib.lgr_ransac_multi(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), corr.shape[0],
                                         C.byref(params), int(max_set), C.byref(res), out, C.byref(n), C.byref(bi)))
        return res, [out[i] for i in range(n.value)], bi.value

    def ransac_multi_ex(self, src, tgt, corr, params, max_set=64, metric_params=None):
        """lgr_ransac_multi_ex_dev: ransac_multi for all five metrics (metric_params: a MetricParams with device weights, None = the
        defaults; read under weighted_closest_plane only)."""
        corr = self._corr_dev(corr)
        res = Result()
        out = (Hypothesis * max(int(max_set), 1))()
        n, bi = C.c_int(0), C.c_int(-1)
        self.check(_lib.lgr_ransac_multi_ex_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), corr.shape[0],
                                                C.byref(params), C.byref(metric_params) if metric_params is not None else None, int(max_set),
                                                C.byref(res), out, C.byref(n), C.byref(bi)))
        return res, [out[i] for i in range(n.value)], bi.value

    def ransac_multi_ex_host(self, src, tgt, corr, params, max_set=64, metric_params=None):
        """lgr_ransac_multi_ex: clouds, correspondences and (metric_params) weights in host memory."""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        corr = np.ascontiguousarray(corr)
        res = Result()
        out = (Hypothesis * max(int(max_set), 1))()
        n, bi = C.c_int(0), C.c_int(-1)
        self.check(_lib.lgr_ransac_multi_ex(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), corr.shape[0],
                                            C.byref(params), C.byref(metric_params) if metric_params is not None else None, int(max_set),
                                            C.byref(res), out, C.byref(n), C.byref(bi)))
        return res, [out[i] for i in range(n.value)], bi.value

    def fold_hypotheses(self, tns, metrics, distance_thr, max_set):
        """lgr_fold_hypotheses_dev: updateHypotheses folded over the items in order.  tns: cuda float32 [n, 16] (column-major 4x4 rows),
        metrics: cuda float32 [n] -> (set transforms [m, 16], set metrics [m], source indices [m]) as numpy arrays."""
        n = int(metrics.shape[0])
        cap = max(int(max_set), 1)
        oT = self.empty((cap, 16), self.torch.float32); oM = self.empty((cap,), self.torch.float32); oI = self.empty((cap,), self.torch.int32)
        m = C.c_int(0)
        self.check(_lib.lgr_fold_hypotheses_dev(self.h, _ptr(tns) if n else None, _ptr(metrics) if n else None, n, C.c_float(distance_thr), int(max_set),
                                                _ptr(oT), _ptr(oM), _ptr(oI), C.byref(m)))
        self._join()
        return oT[: m.value].cpu().numpy(), oM[: m.value].cpu().numpy(), oI[: m.value].cpu().numpy()

    def fold_hypotheses_host(self, tns, metrics, distance_thr, max_set):
        """lgr_fold_hypotheses: numpy float32 [n, 16] / [n] in, numpy out."""
        tns = np.ascontiguousarray(tns, np.float32).reshape(-1, 16); metrics = np.ascontiguousarray(metrics, np.float32)
        n = int(metrics.shape[0])
        cap = max(int(max_set), 1)
        oT = np.zeros((cap, 16), np.float32); oM = np.zeros(cap, np.float32); oI = np.zeros(cap, np.int32)
        m = C.c_int(0)
        self.check(_lib.lgr_fold_hypotheses(self.h, _ptr(tns) if n else None, _ptr(metrics) if n else None, n, C.c_float(distance_thr), int(max_set),
                                            _ptr(oT), _ptr(oM), _ptr(oI), C.byref(m)))
        return oT[: m.value].copy(), oM[: m.value].copy(), oI[: m.value].copy()

    def choose_best_hypothesis_host(self, src, tgt, corr, tns):
        """lgr_choose_best_hypothesis: host clouds and correspondences."""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        corr = np.ascontiguousarray(corr)
        n = len(tns)
        buf = np.ascontiguousarray(np.stack([np.asarray(T, np.float32).T.reshape(16) for T in tns]), np.float32) if n else np.zeros((1, 16), np.float32)
        out = (C.c_float * 16)()
        bi = C.c_int(-1)
        uni = np.zeros(max(n, 1), np.float32)
        self.check(_lib.lgr_choose_best_hypothesis(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), corr.shape[0],
                                                   _ptr(buf), n, out, C.byref(bi), _ptr(uni)))
        return bi.value, np.array(out, np.float32).reshape(4, 4).T.copy(), uni[:n].copy()

    def gror(self, src, tgt, corr, resolution, k_optimal=800):
        corr = self._corr_dev(corr)
        c = corr.shape[0]
        res = Result()
        mask = self.empty((max(c, 1),), self.torch.uint8)
        self.check(_lib.lgr_gror_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), c,
                                     C.c_float(resolution), int(k_optimal), C.byref(res), _ptr(mask)))
        self._join()
        return res, mask[:c].cpu().numpy()

    def gror_node_degree(self, src, tgt, corr, resolution):
        corr = self._corr_dev(corr)
        c = corr.shape[0]
        deg = self.empty((max(c, 1),), self.torch.int32)
        self.check(_lib.lgr_gror_node_degree_dev(self.h, _ptr(src), _ptr(tgt), _ptr(corr), c, C.c_float(resolution), _ptr(deg)))
        self._join()
        return deg[:c].cpu().numpy()

    def teaser(self, src, tgt, corr, params):
        """lgr_teaser_dev.  src, tgt: cuda float32 [n, 12]; corr: numpy CORR_DTYPE or cuda int32 [c, 4]; params: TeaserParams (or a noise
        bound: the defaults with it) -> (Result, TeaserInfo, clique [n_clique] and nodes [n_nodes] as correspondence indices, mask [c])."""
        if not isinstance(params, TeaserParams):
            params = default_teaser_params(float(params))
        corr = self._corr_dev(corr)
        c = corr.shape[0]
        res, info = Result(), TeaserInfo()
        lists = self.empty((2 * TEASER_NODES_MAX,), self.torch.int32)
        mask = self.empty((max(c, 1),), self.torch.uint8)
        self.check(_lib.lgr_teaser_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr) if c else None, c, C.byref(params),
                                       C.byref(res), C.byref(info), _ptr(lists), _ptr(mask)))
        self._join()
        self.sync()   # (c < 3 returns with the list fill still queued)
        lists = lists.cpu().numpy()
        return res, info, lists[: info.n_clique].copy(), lists[TEASER_NODES_MAX: TEASER_NODES_MAX + info.n_nodes].copy(), mask[:c].cpu().numpy()

    def teaser_host(self, src, tgt, corr, params):
        """lgr_teaser: numpy clouds and correspondences in, the same tuple out."""
        if not isinstance(params, TeaserParams):
            params = default_teaser_params(float(params))
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32); corr = np.ascontiguousarray(corr)
        c = corr.shape[0]
        res, info = Result(), TeaserInfo()
        lists = np.zeros(2 * TEASER_NODES_MAX, np.int32); mask = np.zeros(max(c, 1), np.uint8)
        self.check(_lib.lgr_teaser(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr) if c else None, c, C.byref(params),
                                   C.byref(res), C.byref(info), _ptr(lists), _ptr(mask)))
        return res, info, lists[: info.n_clique].copy(), lists[TEASER_NODES_MAX: TEASER_NODES_MAX + info.n_nodes].copy(), mask[:c].copy()

    def refit(self, src, tgt, corr, mask=None):
        corr = self._corr_dev(corr)
        T = (C.c_float * 16)()
        self.check(_lib.lgr_refit_svd_dev(self.h, _ptr(src), _ptr(tgt), _ptr(corr), corr.shape[0], _ptr(mask), T))
        return np.array(T, np.float32).reshape(4, 4).T.copy()

    def align(self, src, tgt, params, descriptor="fpfh"):
        """descriptor: 'fpfh' (lgr_align_dev) or 'shot' / 'rops' / a FeatureParams (lgr_align_ex_dev)."""
        res = Result()
        if isinstance(descriptor, str) and descriptor == "fpfh":
            self.check(_lib.lgr_align_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params), C.byref(res)))
        else:
            f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
            self.check(_lib.lgr_align_ex_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params), C.byref(f),
                                             C.byref(res)))
        return res

    def align_ex2(self, src, tgt, params, descriptor="fpfh", mparams=None):
        """lgr_align_ex2_dev: descriptor as in align, mparams a MetricParams (None = the defaults)."""
        res = Result()
        f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
        self.check(_lib.lgr_align_ex2_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params), C.byref(f),
                                          C.byref(mparams) if mparams is not None else None, C.byref(res)))
        return res

    def align_ex2_host(self, src, tgt, params, descriptor="fpfh", mparams=None):
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        res = Result()
        f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
        self.check(_lib.lgr_align_ex2(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params), C.byref(f),
                                      C.byref(mparams) if mparams is not None else None, C.byref(res)))
        return res

    def align_host(self, src, tgt, params, descriptor="fpfh"):
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        res = Result()
        if isinstance(descriptor, str) and descriptor == "fpfh":
            self.check(_lib.lgr_align(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params), C.byref(res)))
        else:
            f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
            self.check(_lib.lgr_align_ex(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params), C.byref(f),
                                         C.byref(res)))
        return res

    # ---- ground-truth evaluation (src/analysis.cpp:218-246) --------------------------------------------------
    @staticmethod
    def _T16(T):
        return (C.c_float * 16)(*np.asarray(T, np.float32).T.reshape(16).tolist())

    def evaluate_gt(self, src, tgt, corr, T, T_gt, distance_thr, converged=True, inlier_mask=None):
        """lgr_evaluate_gt_dev: src / tgt cuda float32 [n,12], corr a cuda int32 [c,4] tensor or a numpy CORR_DTYPE array, T / T_gt 4x4,
        inlier_mask (optional) c bytes (numpy or cuda uint8).  Returns a GtEval with .correct_mask (numpy uint8 [c])."""
        torch = self.torch
        corr = self._corr_dev(corr)
        c = corr.shape[0]
        if isinstance(inlier_mask, np.ndarray):
            inlier_mask = torch.from_numpy(np.ascontiguousarray(inlier_mask, np.uint8)).to(self._dev())
        cm = self.empty((max(c, 1),), torch.uint8)
        out = GtEval()
        self.check(_lib.lgr_evaluate_gt_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), c, self._T16(T), self._T16(T_gt),
                                            C.c_float(distance_thr), int(bool(converged)), _ptr(inlier_mask), C.byref(out), _ptr(cm)))
        self._join()
        out.correct_mask = cm[:c].cpu().numpy()
        return out

    def evaluate_gt_host(self, src, tgt, corr, T, T_gt, distance_thr, converged=True, inlier_mask=None):
        """lgr_evaluate_gt: numpy in, GtEval out"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        corr = np.ascontiguousarray(corr)
        c = corr.shape[0]
        im = None if inlier_mask is None else np.ascontiguousarray(inlier_mask, np.uint8)
        cm = np.zeros(max(c, 1), np.uint8)
        out = GtEval()
        self.check(_lib.lgr_evaluate_gt(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), c, self._T16(T), self._T16(T_gt),
                                        C.c_float(distance_thr), int(bool(converged)), _ptr(im), C.byref(out), _ptr(cm)))
        out.correct_mask = cm[:c]
        return out

    @staticmethod
    def _batch_args(Ts, converged, inlier_masks, c):
        n = len(Ts)
        assert inlier_masks is None or tuple(inlier_masks.shape) == (n, c), "one mask of c bytes per transform"
        assert converged is None or len(converged) == n, "one flag per transform"
        conv = np.ones(max(n, 1), np.int32)
        if converged is not None and n:
            conv[:] = [int(bool(x)) for x in converged]
        return n, Context._tns16(Ts), conv, (GtEval * max(n, 1))()

    def evaluate_gt_batch(self, src, tgt, corr, Ts, T_gt, distance_thr, converged=None, inlier_masks=None):
        """lgr_evaluate_gt_batch_dev: the transforms Ts (4x4 each, at most GT_BATCH_MAX) judged against one ground truth.  converged: one flag
        per transform (None: all true); inlier_masks: [n, c] bytes (numpy or cuda uint8).  Returns a list of GtEval, each with
        .correct_mask (numpy uint8 [c], the same array for every member)."""
        torch = self.torch
        corr = self._corr_dev(corr)
        c = corr.shape[0]
        n, buf, conv, out = self._batch_args(Ts, converged, inlier_masks, c)
        if isinstance(inlier_masks, np.ndarray):
            inlier_masks = torch.from_numpy(np.ascontiguousarray(inlier_masks, np.uint8)).to(self._dev())
        elif inlier_masks is not None:
            inlier_masks = inlier_masks.contiguous()
        cm = self.empty((max(c, 1),), torch.uint8)
        self.check(_lib.lgr_evaluate_gt_batch_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), c, _ptr(buf), n, self._T16(T_gt),
                                                  C.c_float(distance_thr), _ptr(conv), _ptr(inlier_masks), out, _ptr(cm)))
        self._join()
        mask = cm[:c].cpu().numpy()
        res = [out[i] for i in range(n)]
        for e in res:
            e.correct_mask = mask
        return res

    def evaluate_gt_batch_host(self, src, tgt, corr, Ts, T_gt, distance_thr, converged=None, inlier_masks=None):
        """lgr_evaluate_gt_batch: numpy in, a list of GtEval out"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        corr = np.ascontiguousarray(corr)
        c = corr.shape[0]
        n, buf, conv, out = self._batch_args(Ts, converged, inlier_masks, c)
        im = None if inlier_masks is None else np.ascontiguousarray(inlier_masks, np.uint8)
        cm = np.zeros(max(c, 1), np.uint8)
        self.check(_lib.lgr_evaluate_gt_batch(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), c, _ptr(buf), n, self._T16(T_gt),
                                              C.c_float(distance_thr), _ptr(conv), _ptr(im), out, _ptr(cm)))
        res = [out[i] for i in range(n)]
        for e in res:
            e.correct_mask = cm[:c]
        return res

    # ---- the measure test type (measureTestResults, src/main.cpp:312-382) ------------------------------------
    @staticmethod
    def _measure_args(n_times, seeds):
        n = int(n_times)
        assert seeds is None or len(seeds) == n, "one seed per run"
        sd = None if seeds is None else (C.c_uint64 * max(n, 1))(*[int(s) for s in seeds])
        return n, sd, (MeasureRun * max(n, 1))(), Measurement()

    def measure(self, src, tgt, params, T_gt, n_times=10, seeds=None, descriptor="fpfh", mparams=None):
        """lgr_measure_dev: n_times seeded alignments of one pair (seeds None: params.seed + i) judged against T_gt in one batch.
        Returns (Measurement, [MeasureRun] of the runs made)."""
        n, sd, runs, m = self._measure_args(n_times, seeds)
        f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
        self.check(_lib.lgr_measure_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params), C.byref(f),
                                        C.byref(mparams) if mparams is not None else None, self._T16(T_gt), sd, n, runs, C.byref(m)))
        return m, [runs[i] for i in range(m.n_times)]

    def measure_host(self, src, tgt, params, T_gt, n_times=10, seeds=None, descriptor="fpfh", mparams=None):
        """lgr_measure: clouds [n, 12] float32 in host memory"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        n, sd, runs, m = self._measure_args(n_times, seeds)
        f = descriptor if isinstance(descriptor, FeatureParams) else feature_params(descriptor)
        self.check(_lib.lgr_measure(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], C.byref(params), C.byref(f),
                                    C.byref(mparams) if mparams is not None else None, self._T16(T_gt), sd, n, runs, C.byref(m)))
        return m, [runs[i] for i in range(m.n_times)]

    def overlap_rmse(self, src, tgt, T, T_gt, distance_thr):
        """lgr_overlap_rmse_dev -> (overlap_rmse, overlap_size, pcd_err, idx numpy int32 [ns]: the target point a source point was measured
        against, -1 where it was skipped)"""
        idx = self.empty((max(src.shape[0], 1),), self.torch.int32)
        rm, n, pe = C.c_float(0), C.c_int(0), C.c_float(0)
        self.check(_lib.lgr_overlap_rmse_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], self._T16(T), self._T16(T_gt),
                                             C.c_float(distance_thr), C.byref(rm), C.byref(n), C.byref(pe), _ptr(idx)))
        self._join()
        return rm.value, n.value, pe.value, idx[: src.shape[0]].cpu().numpy()

    def merge_overlaps(self, src, tgt, T_gt, distance_thr):
        """lgr_merge_overlaps_dev -> dict(mask_src, mask_tgt (numpy uint8), n_overlap_src, n_overlap_tgt, overlap, overlap_area)"""
        ms = self.empty((max(src.shape[0], 1),), self.torch.uint8); mt = self.empty((max(tgt.shape[0], 1),), self.torch.uint8)
        n2 = (C.c_int * 2)()
        ov, oa = C.c_float(0), C.c_float(0)
        self.check(_lib.lgr_merge_overlaps_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], self._T16(T_gt), C.c_float(distance_thr),
                                               _ptr(ms), _ptr(mt), n2, C.byref(ov), C.byref(oa)))
        self._join()
        return dict(mask_src=ms[: src.shape[0]].cpu().numpy(), mask_tgt=mt[: tgt.shape[0]].cpu().numpy(), n_overlap_src=n2[0], n_overlap_tgt=n2[1],
                    overlap=ov.value, overlap_area=oa.value)

    def normal_difference(self, src, tgt, T_gt, distance_thr):
        """lgr_normal_difference_dev -> (median normal difference in radians, points it was taken over)"""
        nd, n = C.c_float(0), C.c_int(0)
        self.check(_lib.lgr_normal_difference_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], self._T16(T_gt), C.c_float(distance_thr),
                                                  C.byref(nd), C.byref(n)))
        return nd.value, n.value

    def correct_correspondences(self, src, tgt, corr, T_gt, inlier_mask=None):
        """lgr_correct_correspondences_dev -> (correct mask numpy uint8 [c], n_correct, n_correct_inliers, n_inliers)"""
        torch = self.torch
        corr = self._corr_dev(corr)
        c = corr.shape[0]
        if isinstance(inlier_mask, np.ndarray):
            inlier_mask = torch.from_numpy(np.ascontiguousarray(inlier_mask, np.uint8)).to(self._dev())
        cm = self.empty((max(c, 1),), torch.uint8)
        n3 = (C.c_int * 3)()
        self.check(_lib.lgr_correct_correspondences_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), c, self._T16(T_gt),
                                                        _ptr(inlier_mask), _ptr(cm), n3))
        self._join()
        return cm[:c].cpu().numpy(), n3[0], n3[1], n3[2]

    # ---- the dense closest-plane evaluation (src/metric.cpp:10-53,181-231, sparse = false) and the analysis layer's metric figures ----
    @staticmethod
    def _mparams(weights, weight):
        """None (closest_plane) or a MetricParams: caller weights (numpy for host entries, cuda for _dev) or the map named by weight"""
        if weights is None and weight is None:
            return None
        return metric_params("constant" if weight is None else weight, weights)

    def evaluate_plane_dense(self, src, tgt, T, score_id=SCORE_CONSTANT, weights=None, weights_sum=None, weight=None, threshold=0.0, with_inliers=False,
                             with_nn=False):
        """lgr_evaluate_plane_dense_dev on cuda clouds [n, 12].  weights: cuda float32 [ns] (weighted_closest_plane with a caller's map), or
        weight: the name / id of a built map ('curvature', ...); neither: closest_plane.  The library takes the metric's denominator from the
        weights itself (their sequential f32 sum); weights_sum is accepted for symmetry with evaluate_plane_weighted and must equal that sum
        when given.  threshold <= 0: the target's density; > 0: used as given.  Returns a PlaneDenseEval with .inliers (numpy CORR_DTYPE
        [n_inliers]) and .nn (numpy int32 [ns], -1 = no target in range) when asked for."""
        torch = self.torch
        ns = src.shape[0]
        if weights is not None:
            weights = weights.contiguous()
            if weights_sum is not None:
                s = self._weights_sum(weights)
                if np.float32(s).view(np.uint32) != np.float32(weights_sum).view(np.uint32):
                    raise ValueError(f"weights_sum {weights_sum!r} is not the sequential f32 sum of the weights ({s!r})")
        mp = self._mparams(weights, weight)
        inl = self.empty((max(ns, 1), 4), torch.int32) if with_inliers else None
        nn = self.empty((max(ns, 1),), torch.int32) if with_nn else None
        out = PlaneDenseEval()
        self.check(_lib.lgr_evaluate_plane_dense_dev(self.h, _ptr(src), ns, _ptr(tgt), tgt.shape[0], self._T16(T), int(score_id),
                                                     C.byref(mp) if mp is not None else None, C.c_float(threshold), C.byref(out), _ptr(inl), _ptr(nn)))
        self._join()
        if with_inliers:
            out.inliers = inl[: out.n_inliers].cpu().numpy().view(CORR_DTYPE).reshape(-1)
        if with_nn:
            out.nn = nn[:ns].cpu().numpy()
        return out

    @staticmethod
    def _weights_sum(weights):
        """the sequential f32 sum of cuda weights in index order (numpy's accumulate adds one element after the other)"""
        w = weights.cpu().numpy().astype(np.float32)
        return np.add.accumulate(w, dtype=np.float32)[-1] if len(w) else np.float32(0)

    def evaluate_plane_dense_host(self, src, tgt, T, score_id=SCORE_CONSTANT, weights=None, weights_sum=None, weight=None, threshold=0.0,
                                  with_inliers=False, with_nn=False):
        """lgr_evaluate_plane_dense: numpy in (weights a numpy float32 [ns]), PlaneDenseEval out"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        ns = src.shape[0]
        if weights is not None:
            weights = np.ascontiguousarray(weights, np.float32)
        mp = self._mparams(weights, weight)
        inl = np.zeros(max(ns, 1), CORR_DTYPE) if with_inliers else None
        nn = np.zeros(max(ns, 1), np.int32) if with_nn else None
        out = PlaneDenseEval()
        self.check(_lib.lgr_evaluate_plane_dense(self.h, _ptr(src), ns, _ptr(tgt), tgt.shape[0], self._T16(T), int(score_id),
                                                 C.byref(mp) if mp is not None else None, C.c_float(threshold), C.byref(out), _ptr(inl), _ptr(nn)))
        if with_inliers:
            out.inliers = inl[: out.n_inliers].copy()
        if with_nn:
            out.nn = nn[:ns].copy()
        return out

    # ---- iterated closest-plane refinement (include/lgr.h lgr_refine_plane*) ----
    def _refine(self, fn, src, tgt, T0, score_id, max_steps, threshold, metric_params, trace):
        p = refine_params(score_id, max_steps, threshold)
        out = RefineResult()
        tr = (RefineStep * (max(p.max_steps, 0) + 2))() if trace else None
        n_tr = C.c_int(0)
        self.check(fn(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], self._T16(T0), C.byref(p),
                      C.byref(metric_params) if metric_params is not None else None, C.byref(out), tr, C.byref(n_tr) if trace else None))
        if trace:
            out.trace = [tr[i] for i in range(n_tr.value)]
        return out

    def refine_plane(self, src, tgt, T0, score_id=SCORE_MSE, max_steps=10, threshold=None, metric_params=None, trace=False):
        """lgr_refine_plane_dev on cuda clouds [n, 12]: T0 (4x4) refined by dense closest-plane steps while the metric rises -> RefineResult
        (.matrix(), .steps, .stop, .first, .rejected; .trace with trace=True).  threshold None or <= 0: the target's density.
        metric_params: a MetricParams (capi.metric_params: weight name or a cuda weight map) for the weighted estimator, None: closest_plane."""
        return self._refine(_lib.lgr_refine_plane_dev, src, tgt, T0, score_id, max_steps, threshold, metric_params, trace)

    def refine_plane_host(self, src, tgt, T0, score_id=SCORE_MSE, max_steps=10, threshold=None, metric_params=None, trace=False):
        """lgr_refine_plane: numpy in (caller weights in metric_params a numpy float32 [ns]), RefineResult out"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        return self._refine(_lib.lgr_refine_plane, src, tgt, T0, score_id, max_steps, threshold, metric_params, trace)

    # ---- point-to-plane ICP (include/lgr.h lgr_icp_plane*) ----
    def _icp(self, fn, src, tgt, T0, params, trace, kw):
        p = params if params is not None else icp_params(**kw)
        out = IcpResult()
        tr = (IcpStep * max(getattr(p, "base", p).max_iterations, 1))() if trace else None
        n_tr = C.c_int(0)
        self.check(fn(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], self._T16(T0), C.byref(p), C.byref(out), tr, C.byref(n_tr) if trace else None))
        if trace:
            out.trace = [tr[i] for i in range(n_tr.value)]
        return out

    def icp_plane(self, src, tgt, T0, params=None, trace=False, **kw):
        """lgr_icp_plane_dev on cuda clouds [n, 12] (the target with normals): T0 (4x4) refined by point-to-plane ICP -> IcpResult (.matrix(),
        .iterations, .stop, .max_dist, .pairs, .rmse, .pairs0, .rmse0; .trace with trace=True).  params: an IcpParams, or the keywords of
        capi.icp_params (max_iterations, max_dist, min_dist, shrink, rot_eps, trans_eps; max_dist <= 0: 4 x the target's density)."""
        return self._icp(_lib.lgr_icp_plane_dev, src, tgt, T0, params, trace, kw)

    def icp_plane_host(self, src, tgt, T0, params=None, trace=False, **kw):
        """lgr_icp_plane_host: numpy in, IcpResult out"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        return self._icp(_lib.lgr_icp_plane_host, src, tgt, T0, params, trace, kw)

    # ---- ICP variants (include/lgr.h lgr_icp_ex*) ----
    def _icp_ex(self, fn, src, tgt, T0, params, weights, trace, kw):
        p = params if params is not None else icp_ex_params(weights=weights, **kw)
        return self._icp(fn, src, tgt, T0, p, trace, None)

    def icp_ex(self, src, tgt, T0, variant=ICP_POINT_TO_PLANE, robust=ICP_ROBUST_NONE, robust_scale=0.0, min_normal_cos=-1.0, plane_eps=0.0, weights=None, trace=False,
               params=None, **base_kw):
        """lgr_icp_ex_dev on cuda clouds [n, 12] (both with normals where the variant or the gate reads them): T0 refined by the chosen ICP
        variant -> IcpResult as icp_plane's.  variant 'plane' / 'point' / 'plane2plane', robust 'none' / 'huber' / 'cauchy' / 'tukey' with
        robust_scale k in units of the variant's residual, min_normal_cos > -1 switches the normal gate on, plane_eps the plane-to-plane
        covariance's thin axis (0: 1e-3), weights a cuda float32 [ns] or None; base_kw: the keywords of capi.icp_params.  params: a ready
        IcpExParams instead of all of these."""
        if weights is not None:
            weights = weights.contiguous()
        return self._icp_ex(_lib.lgr_icp_ex_dev, src, tgt, T0, params, weights, trace,
                            dict(base_kw, variant=variant, robust=robust, robust_scale=robust_scale, min_normal_cos=min_normal_cos, plane_eps=plane_eps))

    def icp_ex_host(self, src, tgt, T0, variant=ICP_POINT_TO_PLANE, robust=ICP_ROBUST_NONE, robust_scale=0.0, min_normal_cos=-1.0, plane_eps=0.0, weights=None,
                    trace=False, params=None, **base_kw):
        """lgr_icp_ex_host: numpy in (weights a numpy float32 [ns] or None), IcpResult out"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        if weights is not None:
            weights = np.ascontiguousarray(weights, np.float32)
        return self._icp_ex(_lib.lgr_icp_ex_host, src, tgt, T0, params, weights, trace,
                            dict(base_kw, variant=variant, robust=robust, robust_scale=robust_scale, min_normal_cos=min_normal_cos, plane_eps=plane_eps))

    # ---- trimmed ICP and the rank select under it (include/lgr.h lgr_icp_trim*, lgr_rank_select*) ----
    def _icp_trim(self, fn, src, tgt, T0, params, trace, kw):
        p = params if params is not None else icp_trim_params(**kw)
        out = IcpResult()
        n = max(p.ex.base.max_iterations, 1)
        tr = (IcpStep * n)() if trace else None
        info = (IcpTrimStep * n)()
        n_tr = C.c_int(0)
        self.check(fn(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], self._T16(T0), C.byref(p), C.byref(out), tr, info, C.byref(n_tr)))
        if trace:
            out.trace = [tr[i] for i in range(n_tr.value)]
        out.info = [info[i] for i in range(n_tr.value)]
        return out

    def icp_trim(self, src, tgt, T0, keep=1.0, scale_from_median=0.0, trace=False, weights=None, params=None, **ex_and_base):
        """lgr_icp_trim_dev on cuda clouds [n, 12]: the loop of icp_ex where each iteration keeps the fraction `keep` of its pairs with the
        smallest residuals and, with scale_from_median > 0, scales the robust kernel by that multiple of the median residual (1.4826: the
        MAD rule) -> IcpResult as icp_ex's plus .info, one IcpTrimStep (candidates, kept, cut, scale) per evaluated iteration.
        ex_and_base: the keywords of capi.icp_ex_params; params: a ready IcpTrimParams instead of all of these."""
        if weights is not None:
            weights = weights.contiguous()
        return self._icp_trim(_lib.lgr_icp_trim_dev, src, tgt, T0, params, trace, dict(ex_and_base, keep=keep, scale_from_median=scale_from_median, weights=weights))

    def icp_trim_host(self, src, tgt, T0, keep=1.0, scale_from_median=0.0, trace=False, weights=None, params=None, **ex_and_base):
        """lgr_icp_trim_host: numpy in (weights a numpy float32 [ns] or None), IcpResult with .info out"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        if weights is not None:
            weights = np.ascontiguousarray(weights, np.float32)
        return self._icp_trim(_lib.lgr_icp_trim_host, src, tgt, T0, params, trace, dict(ex_and_base, keep=keep, scale_from_median=scale_from_median, weights=weights))

    def _rank_select(self, fn, keys, ranks, valid, below):
        ranks = [int(r) for r in np.atleast_1d(ranks)]
        n = int(keys.shape[0])
        r = (C.c_int64 * len(ranks))(*ranks)
        idx, key, nv = (C.c_int32 * len(ranks))(), (C.c_float * len(ranks))(), C.c_int64(-1)
        self.check(fn(self.h, _ptr(keys), _ptr(valid), n, r, len(ranks), idx, key, _ptr(below), C.byref(nv)))
        return dict(index=list(idx), key=[np.float32(k) for k in key], below=below, n_valid=nv.value)

    def rank_select(self, keys, ranks, valid=None):
        """lgr_rank_select_dev: keys a cuda float32 [n], valid a cuda uint8 [n] or None, ranks one or two ranks of the order (key, i) over
        the counted elements -> dict(index, key: per rank; below: cuda uint8 [n], position < ranks[0]; n_valid)"""
        import torch
        below = torch.empty(max(int(keys.shape[0]), 1), dtype=torch.uint8, device=keys.device)[:keys.shape[0]]
        return self._rank_select(_lib.lgr_rank_select_dev, keys.contiguous(), ranks, valid.contiguous() if valid is not None else None, below)

    def rank_select_host(self, keys, ranks, valid=None):
        """lgr_rank_select_host: numpy in, dict(index, key, below: numpy uint8 [n], n_valid) out"""
        keys = np.ascontiguousarray(keys, np.float32)
        valid = np.ascontiguousarray(valid, np.uint8) if valid is not None else None
        return self._rank_select(_lib.lgr_rank_select_host, keys, ranks, valid, np.zeros(len(keys), np.uint8))

    def analysis_metric(self, src, tgt, corr, T, T_gt=None, metric_id=METRIC_UNIFORMITY, score_id=SCORE_MSE, weights=None, weight=None):
        """lgr_analysis_metric_dev: what AlignmentAnalysis::start's first statement and buildCorrectInliers yield under metric_id -> MetricEval
        (T_gt None: n_correct_inliers = 0).  weights / weight: the point weights of weighted_closest_plane (neither: constant)."""
        corr = self._corr_dev(corr)
        if weights is not None:
            weights = weights.contiguous()
        mp = self._mparams(weights, weight)
        out = MetricEval()
        self.check(_lib.lgr_analysis_metric_dev(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), corr.shape[0], self._T16(T),
                                                self._T16(T_gt) if T_gt is not None else None, int(metric_id), int(score_id),
                                                C.byref(mp) if mp is not None else None, C.byref(out), None, None))
        return out

    def analysis_metric_host(self, src, tgt, corr, T, T_gt=None, metric_id=METRIC_UNIFORMITY, score_id=SCORE_MSE, weights=None, weight=None):
        """lgr_analysis_metric: numpy in, MetricEval out"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        corr = np.ascontiguousarray(corr)
        if weights is not None:
            weights = np.ascontiguousarray(weights, np.float32)
        mp = self._mparams(weights, weight)
        out = MetricEval()
        self.check(_lib.lgr_analysis_metric(self.h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(corr), corr.shape[0], self._T16(T),
                                            self._T16(T_gt) if T_gt is not None else None, int(metric_id), int(score_id),
                                            C.byref(mp) if mp is not None else None, C.byref(out), None, None))
        return out

    # ---- the debug command: temperature maps, overlap comparison, colour passes (src/main.cpp:152-284, src/common.cpp:771-963) ----
    def _temp_out_dev(self, n):
        torch = self.torch
        t = dict(temp_distance=self.empty((max(n, 1),), torch.float32), temp_normal=self.empty((max(n, 1),), torch.float32),
                 color_distance=self.empty((max(n, 1),), torch.int32), color_normal=self.empty((max(n, 1),), torch.int32),
                 nn=self.empty((max(n, 1),), torch.int32))
        return t, TemperatureOut(*[t[k].data_ptr() for k in TEMP_FIELDS])

    @staticmethod
    def _temp_out_host(n):
        t = dict(temp_distance=np.zeros(max(n, 1), np.float32), temp_normal=np.zeros(max(n, 1), np.float32), color_distance=np.zeros(max(n, 1), np.int32),
                 color_normal=np.zeros(max(n, 1), np.int32), nn=np.zeros(max(n, 1), np.int32))
        return t, TemperatureOut(*[t[k].ctypes.data for k in TEMP_FIELDS])

    def temperature_map(self, compared, reference, distance_max):
        """lgr_temperature_map_dev on cuda clouds [n, 12] -> dict(temp_distance, temp_normal (numpy float32), color_distance, color_normal
        (numpy int32, 0x00RRGGBB), nn (numpy int32, -1 = none), n_below).  With an empty cloud the arrays are empty (nothing is written)."""
        n, nr = compared.shape[0], reference.shape[0]
        t, o = self._temp_out_dev(n)
        nb = C.c_int(0)
        self.check(_lib.lgr_temperature_map_dev(self.h, _ptr(compared), n, _ptr(reference), nr, C.c_float(distance_max), C.byref(o), C.byref(nb)))
        self._join()
        m = n if nr else 0
        out = {k: v[:m].cpu().numpy() for k, v in t.items()}
        out["n_below"] = nb.value
        return out

    def temperature_map_host(self, compared, reference, distance_max):
        compared = np.ascontiguousarray(compared, np.float32); reference = np.ascontiguousarray(reference, np.float32)
        n, nr = compared.shape[0], reference.shape[0]
        t, o = self._temp_out_host(n)
        nb = C.c_int(0)
        self.check(_lib.lgr_temperature_map(self.h, _ptr(compared), n, _ptr(reference), nr, C.c_float(distance_max), C.byref(o), C.byref(nb)))
        out = {k: v[:n if nr else 0] for k, v in t.items()}
        out["n_below"] = nb.value
        return out

    def temperature_maps(self, src, tgt, T, distance_thr):
        """lgr_temperature_maps_dev -> dict(src=<as temperature_map>, tgt=<...>, moved: cuda float32 [ns, 12], the source moved by T)"""
        ns, nt = src.shape[0], tgt.shape[0]
        a, oa = self._temp_out_dev(ns)
        b, ob = self._temp_out_dev(nt)
        moved = self.empty((max(ns, 1), 12), self.torch.float32)
        nb = (C.c_int * 2)()
        self.check(_lib.lgr_temperature_maps_dev(self.h, _ptr(src), ns, _ptr(tgt), nt, self._T16(T), C.c_float(distance_thr), C.byref(oa), C.byref(ob),
                                                 _ptr(moved), nb))
        self._join()
        any_ = ns > 0 and nt > 0
        s = {k: v[:ns if any_ else 0].cpu().numpy() for k, v in a.items()}
        t = {k: v[:nt if any_ else 0].cpu().numpy() for k, v in b.items()}
        s["n_below"], t["n_below"] = nb[0], nb[1]
        return dict(src=s, tgt=t, moved=moved[:ns if any_ else 0])

    def temperature_maps_host(self, src, tgt, T, distance_thr):
        """lgr_temperature_maps: numpy in, numpy out (moved: numpy [ns, 12])"""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        ns, nt = src.shape[0], tgt.shape[0]
        a, oa = self._temp_out_host(ns)
        b, ob = self._temp_out_host(nt)
        moved = np.zeros((max(ns, 1), 12), np.float32)
        nb = (C.c_int * 2)()
        self.check(_lib.lgr_temperature_maps(self.h, _ptr(src), ns, _ptr(tgt), nt, self._T16(T), C.c_float(distance_thr), C.byref(oa), C.byref(ob),
                                             _ptr(moved), nb))
        any_ = ns > 0 and nt > 0
        s = {k: v[:ns if any_ else 0] for k, v in a.items()}
        t = {k: v[:nt if any_ else 0] for k, v in b.items()}
        s["n_below"], t["n_below"] = nb[0], nb[1]
        return dict(src=s, tgt=t, moved=moved[:ns if any_ else 0])

    @staticmethod
    def _tns16(Ts):
        flat = np.concatenate([np.asarray(T, np.float32).T.reshape(16) for T in Ts]) if len(Ts) else np.zeros(0, np.float32)
        return np.ascontiguousarray(flat, np.float32)

    def compare_overlaps(self, src, tgt, Ts, distance_thr, with_masks=True):
        """lgr_compare_overlaps_dev for the transformations Ts (4x4 each) -> dict(counts int32 [n], weighted float32 [n], counts2 int32 [n, 2],
        mask_src uint8 [n, ns], mask_tgt uint8 [n, nt]) as numpy (masks only when asked for)"""
        torch = self.torch
        ns, nt, n = src.shape[0], tgt.shape[0], len(Ts)
        tns = self._tns16(Ts)
        counts = np.zeros(max(n, 1), np.int32); w = np.zeros(max(n, 1), np.float32); c2 = np.zeros((max(n, 1), 2), np.int32)
        ms = torch.zeros((max(n * ns, 1),), dtype=torch.uint8, device=self._dev()) if with_masks else None
        mt = torch.zeros((max(n * nt, 1),), dtype=torch.uint8, device=self._dev()) if with_masks else None
        self.check(_lib.lgr_compare_overlaps_dev(self.h, _ptr(src), ns, _ptr(tgt), nt, _ptr(tns), n, C.c_float(distance_thr), _ptr(counts), _ptr(w), _ptr(c2),
                                                 _ptr(ms), _ptr(mt)))
        self._join()
        out = dict(counts=counts[:n], weighted=w[:n], counts2=c2[:n])
        if with_masks:
            out["mask_src"] = ms[: n * ns].cpu().numpy().reshape(n, ns)
            out["mask_tgt"] = mt[: n * nt].cpu().numpy().reshape(n, nt)
        return out

    def compare_overlaps_host(self, src, tgt, Ts, distance_thr, with_masks=True):
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        ns, nt, n = src.shape[0], tgt.shape[0], len(Ts)
        tns = self._tns16(Ts)
        counts = np.zeros(max(n, 1), np.int32); w = np.zeros(max(n, 1), np.float32); c2 = np.zeros((max(n, 1), 2), np.int32)
        ms = np.zeros(max(n * ns, 1), np.uint8) if with_masks else None
        mt = np.zeros(max(n * nt, 1), np.uint8) if with_masks else None
        self.check(_lib.lgr_compare_overlaps(self.h, _ptr(src), ns, _ptr(tgt), nt, _ptr(tns), n, C.c_float(distance_thr), _ptr(counts), _ptr(w), _ptr(c2),
                                             _ptr(ms), _ptr(mt)))
        out = dict(counts=counts[:n], weighted=w[:n], counts2=c2[:n])
        if with_masks:
            out["mask_src"] = ms[: n * ns].reshape(n, ns)
            out["mask_tgt"] = mt[: n * nt].reshape(n, nt)
        return out

    def nearest(self, q, pts):
        """lgr_nearest_dev: q, pts cuda float32 [n, 12] -> (idx cuda int32 [nq], d2 cuda float32 [nq]); exact for queries anywhere"""
        idx = self.empty((max(q.shape[0], 1),), self.torch.int32); d2 = self.empty((max(q.shape[0], 1),), self.torch.float32)
        self.check(_lib.lgr_nearest_dev(self.h, _ptr(q), q.shape[0], _ptr(pts), pts.shape[0], _ptr(idx), _ptr(d2)))
        self._join()
        return idx[: q.shape[0]], d2[: q.shape[0]]

    def extracted_point_ids(self, src, tgt, T_gt, extracted):
        """saveExtractedPointIds (src/feature_analysis.cpp:20-56): for every extracted point the nearest source point, the source moved by
        the ground truth, and the nearest target point (two lgr_nearest_dev calls).  src, tgt, extracted: cuda float32 [n, 12]; the source
        is moved on the host in the order the library moves a cloud, x c0 + (y c1 + (z c2 + c3)).  Returns numpy id_src / id_tgt int32 [n]
        and the two points' coordinates xyz_src / xyz_tgt float32 [n, 3] (formats.write_extracted_ids writes them)."""
        T = np.asarray(T_gt, np.float32)
        moved = src.cpu().numpy().copy()
        x, y, z = moved[:, 0].copy(), moved[:, 1].copy(), moved[:, 2].copy()
        for a in range(3):
            moved[:, a] = T[a, 0] * x + (T[a, 1] * y + (T[a, 2] * z + T[a, 3]))
        id_src = self.nearest(extracted, self.torch.from_numpy(moved).to(self._dev()))[0].cpu().numpy()
        id_tgt = self.nearest(extracted, tgt)[0].cpu().numpy()
        return dict(id_src=id_src, id_tgt=id_tgt, xyz_src=moved[id_src, :3], xyz_tgt=tgt.cpu().numpy()[id_tgt, :3])

    def color_map(self, values, vmin=None, vmax=None):
        """getColor per value of a cuda float32 vector -> numpy int32 colours.  Without a range: saveColorizedWeights' 0.01 / 0.99 quantiles
        (lgr_color_weights_dev), and the result is (colours, (q01, q99))."""
        n = values.shape[0]
        col = self.empty((max(n, 1),), self.torch.int32)
        if vmin is None and vmax is None:
            r = (C.c_float * 2)()
            self.check(_lib.lgr_color_weights_dev(self.h, _ptr(values), n, _ptr(col), r))
            self._join()
            return col[:n].cpu().numpy(), (np.float32(r[0]), np.float32(r[1]))
        self.check(_lib.lgr_color_map_dev(self.h, _ptr(values), n, C.c_float(vmin), C.c_float(vmax), _ptr(col)))
        self._join()
        return col[:n].cpu().numpy()

    def color_map_host(self, values, vmin=None, vmax=None):
        values = np.ascontiguousarray(values, np.float32)
        n = values.shape[0]
        col = np.zeros(max(n, 1), np.int32)
        if vmin is None and vmax is None:
            r = (C.c_float * 2)()
            self.check(_lib.lgr_color_weights(self.h, _ptr(values), n, _ptr(col), r))
            return col[:n], (np.float32(r[0]), np.float32(r[1]))
        self.check(_lib.lgr_color_map(self.h, _ptr(values), n, C.c_float(vmin), C.c_float(vmax), _ptr(col)))
        return col[:n]

    @staticmethod
    def _corr_host(c):
        return np.zeros(0, CORR_DTYPE) if c is None else np.ascontiguousarray(np.asarray(c).view(CORR_DTYPE).reshape(-1))

    def color_correspondences(self, n, key_points, corr, correct, inliers, is_source):
        """lgr_color_correspondences_dev: the colours savePointCloudWithCorrespondences gives n points.  key_points: None (no key points: beige
        base) or int32 indices; corr / correct / inliers: None or correspondences (numpy CORR_DTYPE or cuda int32 [c, 4]) -> numpy int32 [n]"""
        torch = self.torch
        lists = [self._corr_dev(self._corr_host(x) if x is None or isinstance(x, np.ndarray) else x) for x in (corr, correct, inliers)]
        kp, n_kp = None, 0
        if key_points is not None:
            k = np.ascontiguousarray(key_points.cpu().numpy() if hasattr(key_points, "cpu") else key_points, np.int32)
            n_kp = len(k)
            kp = torch.from_numpy(np.concatenate([k, np.zeros(1, np.int32)])).to(self._dev())   # never a null pointer: "key points given"
        col = self.empty((max(n, 1),), torch.int32)
        args = []
        for x in lists:
            args += [_ptr(x) if x.shape[0] else None, x.shape[0]]
        self.check(_lib.lgr_color_correspondences_dev(self.h, int(n), _ptr(kp), n_kp, *args, int(bool(is_source)), _ptr(col)))
        self._join()
        return col[:n].cpu().numpy()

    def color_correspondences_host(self, n, key_points, corr, correct, inliers, is_source):
        lists = [self._corr_host(x) for x in (corr, correct, inliers)]
        kp, n_kp = None, 0
        if key_points is not None:
            n_kp = len(key_points)
            kp = np.concatenate([np.ascontiguousarray(key_points, np.int32), np.zeros(1, np.int32)])
        col = np.zeros(max(n, 1), np.int32)
        args = []
        for x in lists:
            args += [_ptr(x) if x.shape[0] else None, x.shape[0]]
        self.check(_lib.lgr_color_correspondences(self.h, int(n), _ptr(kp), n_kp, *args, int(bool(is_source)), _ptr(col)))
        return col[:n]
