"""multi-view-registration_amd -- MI355X-native ICP hot path of
fanxiaochen/Multi-View-Registration (`mvr`).

This package is a thin ctypes view of the C-ABI in include/mvr_hip.h
(libmvr_hip.so: hand-written HIP kernels for gfx950 + the host-side solves).
The product host code is C++ (include/mvr/*.hpp, the PCL-style shim the
reference's Registrator call sites compile against); Python is only used to
drive tests and bench.py.  There is no CPU fallback: without the built
extension the import fails, without a GPU Context() raises.

Import with importlib (the directory name has hyphens):
    mvr = importlib.import_module("multi-view-registration_amd")
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys
import warnings

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmvr_hip.so")
if os.environ.get("MVR_LIB_VARIANT"):      # tuning experiments only (tools/build_variant.sh): build/libmvr_hip_<name>.so
    LIB_PATH = os.path.join(os.path.dirname(_HERE), "build", "libmvr_hip_%s.so" % os.environ["MVR_LIB_VARIANT"])

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libmvr_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). There is no fallback implementation.")



def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so (SONAME libamdhip64.so.7, the name libmvr_hip.so needs) but
    ask for it as "libamdhip64.so"; if libmvr_hip.so were loaded first against
    /opt/rocm, a later `import torch` would bring a SECOND runtime into the
    process and find no GPU.  Loading torch's copy first makes both import
    orders resolve to the same runtime.  MVR_HIP_RUNTIME=system skips this."""
    if os.environ.get("MVR_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)
            # ... and one RCCL: the copy built for that runtime (loaded only when a multi-GPU entry point is used)
            r = os.path.join(os.path.dirname(p), "librccl.so")
            if os.path.exists(r):
                os.environ.setdefault("MVR_RCCL_LIB", r)


_share_hip_runtime_with_torch()
_lib = C.CDLL(LIB_PATH)

MAX_SLOTS = 256
MAX_KNN = 64            # MVR_MAX_KNN
OK, E_ARG, E_HIP, E_NOCORR, E_NOMEM, E_SINGULAR, E_RCCL = 0, -1, -2, -3, -4, -5, -6
CONV_STATES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE",
               "NO_CORRESPONDENCES")
K_NN, K_REDUCE, K_XFORM, K_GLUE, K_NN_GRID, K_NN_WIDE = 0, 1, 2, 3, 4, 5


class MvrError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = _lib.mvr_strerror(status).decode()
        super().__init__("mvr status %d (%s)%s" % (status, msg, (": " + detail) if detail else ""))


class IcpParams(C.Structure):
    _fields_ = [("use_reciprocal", C.c_int), ("max_corr_dist", C.c_double),
                ("max_iterations", C.c_int), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_eps", C.c_double), ("fma_dist", C.c_int), ("point_to_plane", C.c_int)]


class IcpStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("state", C.c_int),
                ("n_corr", C.c_int), ("mse", C.c_double), ("evals", C.c_double),
                ("fwd_queries", C.c_double), ("ms", C.c_double)]


class Rejector(C.Structure):
    """mvr_rejector"""
    _fields_ = [("kind", C.c_int), ("value", C.c_double), ("min_correspondences", C.c_uint32), ("max_iterations", C.c_uint32),
                ("refine", C.c_int), ("seed", C.c_uint64)]


class RejectorStage(C.Structure):
    """mvr_rejector_stage"""
    _fields_ = [("in_", C.c_uint32), ("out", C.c_uint32), ("threshold", C.c_float)]


MAX_REJECTORS = 8       # MVR_MAX_REJECTORS
REJ_DISTANCE, REJ_MEDIAN, REJ_TRIMMED, REJ_SURFACE_NORMAL, REJ_ONE_TO_ONE, REJ_SAMPLE_CONSENSUS = 0, 1, 2, 3, 4, 5
REJ_KINDS = {"distance": REJ_DISTANCE, "median": REJ_MEDIAN, "trimmed": REJ_TRIMMED, "surface_normal": REJ_SURFACE_NORMAL,
             "one_to_one": REJ_ONE_TO_ONE, "sample_consensus": REJ_SAMPLE_CONSENSUS}


class RejSacResult(C.Structure):
    """mvr_rej_sac_result"""
    _fields_ = [("found", C.c_int), ("live", C.c_uint32), ("valid", C.c_uint32), ("inliers", C.c_uint32), ("ransac_inliers", C.c_uint32),
                ("iterations", C.c_int), ("attempts", C.c_int), ("skipped", C.c_int), ("best_attempt", C.c_int),
                ("refine_rounds", C.c_int), ("k", C.c_double), ("T", C.c_float * 16), ("ransac_T", C.c_float * 16)]


class RejSacTrace(C.Structure):
    """mvr_rej_sac_trace"""
    _fields_ = [("status", C.c_int), ("query", C.c_uint32 * 3), ("match", C.c_uint32 * 3), ("T", C.c_float * 16),
                ("inliers", C.c_uint32), ("k", C.c_double)]


class IcpIterTrace(C.Structure):
    """mvr_icp_iter_trace"""
    _fields_ = [("n_found", C.c_uint32), ("stages", RejectorStage * MAX_REJECTORS), ("n_corr", C.c_uint32), ("mse", C.c_double),
                ("tr", C.c_float * 16)]


class GicpParams(C.Structure):
    """mvr_gicp_params"""
    _fields_ = [("max_corr_dist", C.c_double), ("use_reciprocal", C.c_int), ("fma_dist", C.c_int), ("max_iterations", C.c_int),
                ("max_inner_iterations", C.c_int), ("transformation_epsilon", C.c_double), ("rotation_epsilon", C.c_double),
                ("gicp_epsilon", C.c_double), ("inner_rot_tol", C.c_double), ("inner_trans_tol", C.c_double), ("inner_chunk", C.c_int)]


class GicpIterTrace(C.Structure):
    """mvr_gicp_iter_trace"""
    _fields_ = [("n_found", C.c_uint32), ("stages", RejectorStage * MAX_REJECTORS), ("n_corr", C.c_uint32), ("mse", C.c_double),
                ("f0", C.c_double), ("f1", C.c_double), ("inner_evals", C.c_uint32), ("inner_accepted", C.c_uint32),
                ("lambda_", C.c_double), ("tr", C.c_float * 16)]


class GicpInfo(C.Structure):
    """mvr_gicp_info"""
    _fields_ = [("evaluations", C.c_uint32), ("accepted", C.c_uint32), ("lambda_", C.c_double), ("f0", C.c_double), ("f1", C.c_double)]


NDT_STOPS = ("NOT", "STEP", "ITERATIONS", "FLAT", "NO_DECREASE", "NO_OVERLAP")      # MVR_NDT_*


class NdtParams(C.Structure):
    """mvr_ndt_params"""
    _fields_ = [("resolution", C.c_double), ("step_size", C.c_double), ("outlier_ratio", C.c_double), ("transformation_epsilon", C.c_double),
                ("min_covar_eigvalue_mult", C.c_double), ("origin", C.c_double * 3), ("max_iterations", C.c_int), ("max_line_evals", C.c_int),
                ("min_points_per_voxel", C.c_int)]


class NdtStats(C.Structure):
    """mvr_ndt_stats"""
    _fields_ = [("iterations", C.c_int), ("stop", C.c_int), ("converged", C.c_int), ("evaluations", C.c_int), ("n_cells", C.c_uint32),
                ("n_pairs", C.c_double), ("score", C.c_double), ("ms", C.c_double)]


class NdtIterTrace(C.Structure):
    """mvr_ndt_iter_trace"""
    _fields_ = [("a", C.c_double), ("delta_norm", C.c_double), ("trials", C.c_int), ("reversed", C.c_int), ("fallback", C.c_int),
                ("stop", C.c_int), ("score", C.c_double), ("count", C.c_double), ("p", C.c_double * 6)]


NDT_EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))      # mvr_ndt_eval_fn


class PairMoments(C.Structure):
    _fields_ = [("n", C.c_double), ("mean_src", C.c_double * 3), ("mean_tgt", C.c_double * 3),
                ("mse", C.c_double), ("sigma", C.c_double * 9)]


class PairMoments2(C.Structure):
    _fields_ = [("n", C.c_double), ("origin", C.c_double * 3), ("sp", C.c_double * 3),
                ("sq", C.c_double * 3), ("spp", C.c_double * 6), ("sqq", C.c_double * 6),
                ("spq", C.c_double * 9), ("sum_d2", C.c_double)]


class SynthParams(C.Structure):
    _fields_ = [("n_views", C.c_int), ("seed", C.c_uint64), ("noise_sigma", C.c_double),
                ("pivot", C.c_double * 3), ("axis", C.c_double * 3)]


class NormalParams(C.Structure):
    """mvr_normal_params"""
    _fields_ = [("k", C.c_int), ("radius", C.c_double), ("viewpoint", C.c_float * 3), ("fma_dist", C.c_int)]


class SorParams(C.Structure):
    """mvr_sor_params"""
    _fields_ = [("mean_k", C.c_int), ("stddev_mul", C.c_double), ("negative", C.c_int), ("fma_dist", C.c_int)]


class SorStats(C.Structure):
    """mvr_sor_stats"""
    _fields_ = [("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double), ("n_valid", C.c_size_t)]


class RorParams(C.Structure):
    """mvr_ror_params"""
    _fields_ = [("radius", C.c_double), ("min_neighbors", C.c_int), ("negative", C.c_int), ("fma_dist", C.c_int)]


class MlsParams(C.Structure):
    """mvr_mls_params"""
    _fields_ = [("radius", C.c_double), ("order", C.c_int), ("sqr_gauss_param", C.c_double), ("compute_normals", C.c_int),
                ("orient", C.c_int), ("viewpoint", C.c_float * 3), ("fma_dist", C.c_int)]


class FpfhParams(C.Structure):
    """mvr_fpfh_params"""
    _fields_ = [("radius", C.c_double), ("fma_dist", C.c_int)]


class PfhParams(C.Structure):
    """mvr_pfh_params"""
    _fields_ = [("radius", C.c_double), ("k", C.c_int), ("fma_dist", C.c_int)]


class ShotParams(C.Structure):
    """mvr_shot_params"""
    _fields_ = [("radius", C.c_double), ("lrf_radius", C.c_double), ("fma_dist", C.c_int)]


class RadiusParams(C.Structure):
    """mvr_radius_params"""
    _fields_ = [("radius", C.c_double), ("max_nn", C.c_uint32), ("sorted", C.c_int), ("fma_dist", C.c_int)]


class McParams(C.Structure):
    """mvr_mc_params"""
    _fields_ = [("res", C.c_int * 3), ("iso_level", C.c_float), ("percentage_extend_grid", C.c_float), ("dist_ignore", C.c_float),
                ("weld", C.c_int), ("fma_dist", C.c_int)]


class IssParams(C.Structure):
    """mvr_iss_params"""
    _fields_ = [("salient_radius", C.c_double), ("non_max_radius", C.c_double), ("gamma_21", C.c_double), ("gamma_32", C.c_double),
                ("min_neighbors", C.c_int), ("fma_dist", C.c_int)]


class IssBorderParams(C.Structure):
    """mvr_iss_border_params"""
    _fields_ = [("border_radius", C.c_double), ("angle_threshold", C.c_double)]


class BoundaryParams(C.Structure):
    """mvr_boundary_params"""
    _fields_ = [("radius", C.c_double), ("angle_threshold", C.c_double), ("min_neighbors", C.c_int), ("fma_dist", C.c_int)]


class SacParams(C.Structure):
    """mvr_sac_params"""
    _fields_ = [("model", C.c_int), ("threshold", C.c_double), ("max_iterations", C.c_int), ("probability", C.c_double),
                ("optimize", C.c_int), ("axis", C.c_double * 3), ("eps_angle", C.c_double), ("seed", C.c_uint64),
                ("negative", C.c_int), ("fma_dist", C.c_int)]


class SacResult(C.Structure):
    """mvr_sac_result"""
    _fields_ = [("found", C.c_int), ("inliers", C.c_uint32), ("ransac_inliers", C.c_uint32), ("iterations", C.c_int),
                ("attempts", C.c_int), ("skipped", C.c_int), ("best_attempt", C.c_int), ("k", C.c_double),
                ("coefficients", C.c_float * 4), ("ransac_coefficients", C.c_float * 4)]


class SacTrace(C.Structure):
    """mvr_sac_trace"""
    _fields_ = [("status", C.c_int), ("sample", C.c_uint32 * 3), ("coefficients", C.c_float * 4), ("inliers", C.c_uint32),
                ("k", C.c_double)]


class ClusterParams(C.Structure):
    """mvr_cluster_params"""
    _fields_ = [("tolerance", C.c_double), ("min_size", C.c_uint32), ("max_size", C.c_uint32), ("use_normals", C.c_int),
                ("eps_angle", C.c_double), ("negative", C.c_int), ("keep", C.c_uint32), ("fma_dist", C.c_int)]


class ClusterResult(C.Structure):
    """mvr_cluster_result"""
    _fields_ = [("n_active", C.c_uint32), ("n_components", C.c_uint32), ("n_clusters", C.c_uint32), ("n_clustered", C.c_uint32),
                ("largest", C.c_uint32), ("too_small", C.c_uint32), ("too_large", C.c_uint32)]


SAC_MODELS = {"plane": 0, "perpendicular_plane": 1}   # mvr_sac_params.model: SACMODEL_PLANE, SACMODEL_PERPENDICULAR_PLANE
BOUNDARY_MIN_ANGLE = math.pi / 4   # MVR_BOUNDARY_MIN_ANGLE: the smallest angle_threshold the boundary rule accepts
FPFH_BINS = 11          # MVR_FPFH_BINS: a signature is 3 * 11 = 33 floats
PFH_DIM = 125           # MVR_PFH_DIM: 5 * 5 * 5 joint bins
SHOT_DIM = 352          # MVR_SHOT_DIM: 32 volumes x 11 shape slots
PFH_STAGE = 256         # MVR_PFH_STAGE: neighbours staged on chip; above it the tiled path
PREREJ_MAX_SAMPLES = 8  # MVR_PREREJ_MAX_SAMPLES
RADIUS_STAGE = 1024     # MVR_RADIUS_STAGE: entries of a radius-search row ordered on chip; above it the long-row path
MC_MAX_VERTICES = 1 << 27   # MVR_MC_MAX_VERTICES: the most lattice vertices of one marching-cubes call (rule M12)
RADIUS_MAX_TOTAL = 0x7FFFFFFF   # MVR_RADIUS_MAX_TOTAL: the most entries one mvr_radius_search returns (rule RS8)


class PrerejParams(C.Structure):
    """mvr_prerej_params"""
    _fields_ = [("max_iterations", C.c_int), ("nr_samples", C.c_int), ("k", C.c_int), ("similarity", C.c_double),
                ("max_dist", C.c_double), ("inlier_fraction", C.c_double), ("seed", C.c_uint64), ("fma_dist", C.c_int)]


class PrerejResult(C.Structure):
    """mvr_prerej_result"""
    _fields_ = [("converged", C.c_int), ("best_iteration", C.c_int), ("inliers", C.c_uint32), ("error", C.c_double),
                ("rejected", C.c_uint32), ("scored", C.c_uint32), ("T", C.c_float * 16)]


class PrerejTrace(C.Structure):
    """mvr_prerej_trace"""
    _fields_ = [("status", C.c_int), ("src", C.c_uint32 * PREREJ_MAX_SAMPLES), ("tgt", C.c_uint32 * PREREJ_MAX_SAMPLES),
                ("inliers", C.c_uint32), ("error", C.c_double), ("T", C.c_float * 16)]


_fp, _dp, _u32p, _i32p = (C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                          C.POINTER(C.c_int32))
_vp, _sz, _u8p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8)

# name -> (restype, argtypes); also the list the symbol-export test checks
SIGNATURES = {
    "mvr_ctx_create": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "mvr_ctx_create_on_stream": (C.c_int, [C.POINTER(_vp), C.c_int, _vp]),
    "mvr_ctx_destroy": (C.c_int, [_vp]),
    "mvr_ctx_sync": (C.c_int, [_vp]),
    "mvr_strerror": (C.c_char_p, [C.c_int]),
    "mvr_last_error": (C.c_char_p, [_vp]),
    "mvr_device_info": (C.c_int, [_vp, C.c_char_p, _sz, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mvr_cloud_upload": (C.c_int, [_vp, C.c_int, _fp, _sz, _sz]),
    "mvr_cloud_download": (C.c_int, [_vp, C.c_int, _fp, _sz, _sz, C.POINTER(_sz)]),
    "mvr_cloud_size": (C.c_int, [_vp, C.c_int, C.POINTER(_sz)]),
    "mvr_cloud_reserve": (C.c_int, [_vp, C.c_int, _sz]),
    "mvr_cloud_copy": (C.c_int, [_vp, C.c_int, C.c_int]),
    "mvr_cloud_append": (C.c_int, [_vp, C.c_int, C.c_int]),
    "mvr_cloud_denoise": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _u32p]),
    "mvr_cloud_voxel_grid": (C.c_int, [_vp, C.c_int, C.c_int, _fp, C.c_uint, C.POINTER(_sz), _u32p, C.POINTER(C.c_int)]),
    "mvr_cloud_statistical_outlier_removal": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(SorParams), C.POINTER(_sz), _u32p, _fp,
                                                        C.POINTER(SorStats)]),
    "mvr_cloud_radius_outlier_removal": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(RorParams), C.POINTER(_sz), _u32p, _u32p]),
    "mvr_cloud_mls": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(MlsParams), C.POINTER(_sz), _u32p, _fp]),
    "mvr_cloud_fpfh": (C.c_int, [_vp, C.c_int, C.POINTER(FpfhParams), _fp, _fp, _u32p]),
    "mvr_cloud_pfh": (C.c_int, [_vp, C.c_int, C.POINTER(PfhParams), _fp, _u32p, _u32p]),
    "mvr_cloud_estimate_normals_at": (C.c_int, [_vp, C.c_int, _u32p, C.c_size_t, C.c_int, C.POINTER(NormalParams), C.c_int, _fp, _fp]),
    "mvr_cloud_fpfh_at": (C.c_int, [_vp, C.c_int, _u32p, C.c_size_t, C.c_int, C.POINTER(FpfhParams), _fp, _u32p]),
    "mvr_cloud_pfh_at": (C.c_int, [_vp, C.c_int, _u32p, C.c_size_t, C.c_int, C.POINTER(PfhParams), _fp, _u32p, _u32p]),
    "mvr_cloud_shot_lrf": (C.c_int, [_vp, C.c_int, C.POINTER(ShotParams), _fp, _u32p]),
    "mvr_cloud_shot": (C.c_int, [_vp, C.c_int, C.POINTER(ShotParams), _fp, _fp, _fp, C.POINTER(C.c_uint64), _u32p]),
    "mvr_cloud_shot_at": (C.c_int, [_vp, C.c_int, _u32p, C.c_size_t, C.c_int, C.POINTER(ShotParams), _fp, _fp, _fp,
                                    C.POINTER(C.c_uint64), _u32p]),
    "mvr_radius_default_params": (None, [C.POINTER(RadiusParams)]),
    "mvr_radius_search": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(RadiusParams), C.POINTER(C.c_uint64), _u32p, _fp, _sz, C.POINTER(_sz)]),
    "mvr_mc_default_params": (None, [C.POINTER(McParams)]),
    "mvr_mc_case": (C.c_int, [C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_int8)]),
    "mvr_cloud_marching_cubes_hoppe": (C.c_int, [_vp, C.c_int, C.POINTER(McParams), _fp, _fp, _sz, _u32p, C.POINTER(C.c_uint64),
                                                 C.POINTER(C.c_uint64)]),
    "mvr_cloud_iss_keypoints": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(IssParams), C.POINTER(_sz), _u32p, _dp, _u32p, _u32p]),
    "mvr_cloud_iss_keypoints_border": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(IssParams), C.POINTER(IssBorderParams), C.POINTER(_sz), _u32p,
                                                 _dp, _u32p, _u32p, _u8p, _u8p]),
    "mvr_cloud_boundary": (C.c_int, [_vp, C.c_int, C.POINTER(BoundaryParams), _u8p, _fp, _u32p]),
    "mvr_cloud_segment_plane": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(SacParams), C.POINTER(SacResult), C.POINTER(_sz), _u32p, _u8p,
                                          C.POINTER(SacTrace), _sz]),
    "mvr_cloud_extract_indices": (C.c_int, [_vp, C.c_int, C.c_int, _u32p, _sz, C.c_int, C.POINTER(_sz)]),
    "mvr_cluster_default_params": (None, [C.POINTER(ClusterParams)]),
    "mvr_cloud_euclidean_clusters": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(ClusterParams), _u32p, _sz, C.POINTER(ClusterResult),
                                               C.POINTER(_sz), _u32p, _sz, _u32p, _u32p]),
    "mvr_feature_knn": (C.c_int, [_vp, _fp, _sz, _fp, _sz, C.c_int, C.c_int, _u32p, _fp]),
    "mvr_pose_scores": (C.c_int, [_vp, C.c_int, C.c_int, _fp, _sz, C.c_double, C.c_int, _u32p, _dp]),
    "mvr_align_prerejective": (C.c_int, [_vp, C.c_int, C.c_int, _fp, _fp, C.POINTER(PrerejParams), _fp, C.POINTER(PrerejResult),
                                         C.POINTER(PrerejTrace)]),
    "mvr_align_prerejective_dim": (C.c_int, [_vp, C.c_int, C.c_int, _fp, _fp, C.c_int, C.POINTER(PrerejParams), _fp, C.POINTER(PrerejResult),
                                             C.POINTER(PrerejTrace)]),
    "mvr_cloud_set_global_base": (C.c_int, [_vp, C.c_int, _sz]),
    "mvr_cloud_append_range": (C.c_int, [_vp, C.c_int, C.c_int, _sz, _sz, _sz]),
    "mvr_nn_forward_keys": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_int, _vp]),
    "mvr_pair_moments2_from_keys": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, C.c_int, C.c_int, _dp, _vp]),
    "mvr_cloud_clear": (C.c_int, [_vp, C.c_int]),
    "mvr_cloud_transform": (C.c_int, [_vp, C.c_int, C.c_int, _dp]),
    "mvr_cloud_transform_f32": (C.c_int, [_vp, C.c_int, C.c_int, _fp]),
    "mvr_cloud_upload_normals": (C.c_int, [_vp, C.c_int, _fp, _sz, _sz]),
    "mvr_cloud_download_normals": (C.c_int, [_vp, C.c_int, _fp, _sz, _sz, C.POINTER(_sz)]),
    "mvr_nn": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _u32p, _fp]),
    "mvr_knn": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _u32p, _fp]),
    "mvr_cloud_estimate_normals": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(NormalParams), C.POINTER(_fp)]),
    "mvr_correspondences": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                      _i32p, _i32p, _fp, _sz, C.POINTER(_sz)]),
    "mvr_pair_moments": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                   C.POINTER(PairMoments)]),
    "mvr_pair_moments2": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _sz, _sz,
                                    _dp, C.POINTER(PairMoments2)]),
    "mvr_pair_moments2_dev": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _sz,
                                        _sz, _dp, _vp]),
    "mvr_cloud_transform_batch": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp]),
    "mvr_pair_moments2_batch": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_double, C.c_int,
                                          C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _dp,
                                          C.POINTER(PairMoments2), _vp]),
    "mvr_seq_align_sharded": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams), _dp, _fp, C.POINTER(IcpStats)]),
    "mvr_seq_run_sharded": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams), _dp, C.c_int, _dp,
                                      C.POINTER(C.c_int), _fp, C.POINTER(IcpStats), C.POINTER(C.c_int)]),
    "mvr_seq_run": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams), C.c_int, _dp,
                              C.POINTER(C.c_int), _fp, C.POINTER(IcpStats), C.POINTER(C.c_int)]),
    "mvr_pair_batch_correspondences": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _fp, _sz, C.POINTER(_sz)]),
    "mvr_pair_moments2_from_corr": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _sz, _dp,
                                              C.POINTER(PairMoments2)]),
    "mvr_umeyama_from_moments": (C.c_int, [C.POINTER(PairMoments), _fp, _dp]),
    "mvr_moments_from_moments2": (C.c_int, [C.POINTER(PairMoments2), C.POINTER(PairMoments)]),
    "mvr_icp_align": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams), _fp,
                                C.POINTER(IcpStats)]),
    "mvr_correspondences_rejected": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(Rejector), C.c_int,
                                               _i32p, _i32p, _fp, _sz, C.POINTER(_sz), C.POINTER(RejectorStage)]),
    "mvr_reject_correspondences": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _fp, _sz, C.POINTER(Rejector), C.c_int,
                                             _i32p, _i32p, _fp, _sz, C.POINTER(_sz), C.POINTER(RejectorStage)]),
    "mvr_reject_sample_consensus": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _fp, _sz, C.POINTER(Rejector),
                                              C.POINTER(RejSacResult), _i32p, _i32p, _fp, _sz, C.POINTER(_sz),
                                              C.POINTER(RejSacTrace), _sz]),
    "mvr_ctx_last_sample_consensus": (C.c_int, [_vp, C.POINTER(RejSacResult)]),
    "mvr_icp_align_rejected": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(IcpParams), C.POINTER(Rejector), C.c_int, _fp,
                                         C.POINTER(IcpStats), C.POINTER(IcpIterTrace), C.c_int]),
    "mvr_gicp_default_params": (None, [C.POINTER(GicpParams)]),
    "mvr_icp_align_gicp": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(GicpParams), C.POINTER(Rejector), C.c_int, _fp,
                                     C.POINTER(IcpStats), C.POINTER(GicpIterTrace), C.c_int]),
    "mvr_gicp_sums": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _sz, _dp, C.c_double, _dp]),
    "mvr_gicp_solve": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _sz, C.POINTER(GicpParams), _dp, C.POINTER(GicpInfo)]),
    "mvr_ndt_default_params": (None, [C.POINTER(NdtParams)]),
    "mvr_ndt_constants": (C.c_int, [C.POINTER(NdtParams), _dp, _dp]),
    "mvr_ndt_direction": (C.c_int, [_dp, _dp]),
    "mvr_ndt_newton": (C.c_int, [C.POINTER(NdtParams), NDT_EVAL_FN, _vp, _dp, _dp, C.POINTER(NdtStats), C.POINTER(NdtIterTrace), C.c_int]),
    "mvr_ndt_cells": (C.c_int, [_vp, C.c_int, C.POINTER(NdtParams), _sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), _dp, _dp,
                                C.POINTER(_sz)]),
    "mvr_ndt_sums": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(NdtParams), _dp, _dp, _dp]),
    "mvr_ndt_align": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(NdtParams), _dp, _fp, _dp, C.POINTER(NdtStats),
                                C.POINTER(NdtIterTrace), C.c_int]),
    "mvr_fitness": (C.c_int, [_vp, C.c_int, C.c_int, _fp, C.c_double, C.c_int, _dp]),
    "mvr_lum_edge_from_moments": (C.c_int, [C.POINTER(PairMoments2), _dp, _dp, _dp, _dp, _dp]),
    "mvr_lum_edge_from_moments_x4": (C.c_int, [C.POINTER(PairMoments2), _dp, _dp, _dp, _dp, _dp]),
    "mvr_lum_compute": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(PairMoments2), C.c_int, C.c_double, _dp,
                                  C.POINTER(C.c_int)]),
    "mvr_ring_host_step": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, _dp, C.c_int,
                                     _dp, _dp, _fp, _dp, _dp, C.POINTER(C.c_int)]),
    "mvr_ring_step": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                C.POINTER(C.c_int), C.c_double, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _fp, _dp, _dp,
                                C.POINTER(C.c_int), _dp, _dp]),
    "mvr_ring_run": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                               C.POINTER(C.c_int), C.c_double, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _fp, _dp, _dp,
                               C.POINTER(C.c_int), _dp, _dp]),
    "mvr_comm_unique_id": (C.c_int, [C.c_char_p]),
    "mvr_ctx_comm_init": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int]),
    "mvr_ctx_comm_destroy": (C.c_int, [_vp]),
    "mvr_ctx_comm_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mvr_rccl_library": (C.c_char_p, []),
    "mvr_pool_trim": (C.c_uint64, [C.POINTER(C.c_uint64)]),
    "mvr_ring_segments": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "mvr_ring_run_sharded": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.c_double, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _fp, _dp, _dp,
                                       C.POINTER(C.c_int), _dp, _dp]),
    "mvr_ctx_project": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int]),
    "mvr_debug_order": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "mvr_ring_rows_sharded": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.c_double, C.c_int, C.c_int, _dp, _dp, _dp]),
    "mvr_world_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.POINTER(C.c_int)]),
    "mvr_world_destroy": (C.c_int, [_vp]),
    "mvr_world_size": (C.c_int, [_vp]),
    "mvr_world_ctx": (_vp, [_vp, C.c_int]),
    "mvr_world_last_error": (C.c_char_p, [_vp]),
    "mvr_world_upload": (C.c_int, [_vp, C.c_int, _fp, _sz, _sz]),
    "mvr_world_ring_run": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                     C.POINTER(C.c_int), C.c_double, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _fp, _dp, _dp,
                                     C.POINTER(C.c_int), _dp, _dp]),
    "mvr_pose_to_mat4": (None, [_dp, _dp]),
    "mvr_lum_incidence": (None, [_dp, _dp]),
    "mvr_refine_axis": (C.c_int, [C.c_int, _dp, C.c_float, _fp, _fp]),
    "mvr_turntable_angle": (C.c_double, [C.c_int, C.c_int]),
    "mvr_axis_rotation": (None, [_dp, _dp, C.c_double, _dp]),
    "mvr_mat4d_mul": (None, [_dp, _dp, _dp]),
    "mvr_mat4f_mul": (None, [_fp, _fp, _fp]),
    "mvr_ctx_tune": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "mvr_ctx_stat": (C.c_int, [_vp, C.c_char_p, _dp]),
    "mvr_ctx_pass_log": (C.c_int, [_vp, _dp, C.c_int, C.POINTER(C.c_int)]),
    "mvr_debug_counters": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_int]),
    "mvr_prof_enable": (C.c_int, [_vp, C.c_int]),
    "mvr_prof_reset": (C.c_int, [_vp]),
    "mvr_prof_get": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64), _dp, _dp]),
    "mvr_synth_default": (None, [C.POINTER(SynthParams), C.c_int, C.c_int]),
    "mvr_synth_view": (C.c_int, [C.POINTER(SynthParams), C.c_int, _sz, _fp, _fp]),
    "mvr_synth_prior": (None, [C.POINTER(SynthParams), _dp, _dp]),
}
for _name, (_res, _args) in SIGNATURES.items():
    _f = getattr(_lib, _name)
    _f.restype, _f.argtypes = _res, _args


def _chk(rc, ctx=None, allow=()):
    if rc != OK and rc not in allow:
        detail = _lib.mvr_last_error(ctx).decode() if ctx else ""
        raise MvrError(rc, detail)
    return rc


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def to_cm(T, dtype):
    """(4,4) math layout T[r,c] -> 16 column-major values (Eigen::Matrix4f memory)."""
    return np.ascontiguousarray(np.asarray(T, dtype=dtype).T).reshape(16)


def from_cm(v):
    return np.array(v).reshape(4, 4).T.copy()


# --------------------------------------------------------------- host helpers

def mc_case(cube):
    """mvr_mc_case: row `cube` (0..255) of the marching-cubes case tables (rule M10) -> (edge bits, int8[16] edge triples,
    -1 terminated); host only"""
    e, t = C.c_uint16(), np.empty(16, np.int8)
    _chk(_lib.mvr_mc_case(int(cube), C.byref(e), _p(t, C.c_int8)))
    return int(e.value), t


def icp_params(reciprocal=True, max_dist=4.0, max_iter=10, teps=1e-6, feps=64.0, fma=False, point_to_plane=False):
    """Defaults = the reference's settings at mvr/src/registrator.cpp:551-560
    (max_iterations is the caller's; with feps=64 every align is one iteration)."""
    return IcpParams(int(reciprocal), float(max_dist), int(max_iter), float(teps), float(feps),
                     int(fma), int(point_to_plane))


def rejector(kind, value=0.0, min_correspondences=0, max_iterations=0, refine=0, seed=0) -> Rejector:
    """One stage of a rejector chain (mvr_rejector): kind = "distance" (value: the largest distance), "median" (the factor),
    "trimmed" (the overlap ratio; min_correspondences), "surface_normal" (the smallest cosine), "one_to_one",
    "sample_consensus" (the inlier threshold; max_iterations, 0 = 1000; refine; seed), or a REJ_* number."""
    return Rejector(REJ_KINDS[kind] if isinstance(kind, str) else int(kind), float(value), int(min_correspondences),
                    int(max_iterations), int(bool(refine)), int(seed))


def _rej_sac_dict(res) -> dict:
    return dict(found=bool(res.found), live=int(res.live), valid=int(res.valid), inliers=int(res.inliers),
                ransac_inliers=int(res.ransac_inliers), iterations=res.iterations, attempts=res.attempts, skipped=res.skipped,
                best_attempt=res.best_attempt, refine_rounds=res.refine_rounds, k=res.k, T=from_cm(np.array(res.T, np.float32)),
                ransac_T=from_cm(np.array(res.ransac_T, np.float32)))


def gicp_params(**kw) -> GicpParams:
    """mvr_gicp_params with PCL's defaults (mvr_gicp_default_params); keywords = the fields: max_corr_dist, use_reciprocal,
    fma_dist, max_iterations, max_inner_iterations, transformation_epsilon, rotation_epsilon, gicp_epsilon, inner_rot_tol,
    inner_trans_tol, inner_chunk."""
    p = GicpParams()
    _lib.mvr_gicp_default_params(C.byref(p))
    names = {f[0]: f[1] for f in GicpParams._fields_}
    for k, v in kw.items():
        if k not in names:
            raise TypeError("gicp_params: no field %r" % k)
        setattr(p, k, float(v) if names[k] is C.c_double else int(v))
    return p


def ndt_params(**kw) -> NdtParams:
    """mvr_ndt_params with PCL's defaults (mvr_ndt_default_params; they are meant for metres: resolution and step_size are in
    the cloud's unit); keywords = the fields: resolution, step_size, outlier_ratio, transformation_epsilon,
    min_covar_eigvalue_mult, origin (3 values), max_iterations, max_line_evals, min_points_per_voxel."""
    p = NdtParams()
    _lib.mvr_ndt_default_params(C.byref(p))
    names = {f[0]: f[1] for f in NdtParams._fields_}
    for k, v in kw.items():
        if k not in names:
            raise TypeError("ndt_params: no field %r" % k)
        if k == "origin":
            p.origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, float(v) if names[k] is C.c_double else int(v))
    return p


def ndt_constants(params: NdtParams, guess=None):
    """mvr_ndt_constants: rule N11's parameter checks on the host -> (d1, d2, d3) of rule N2; raises MvrError(E_ARG)"""
    d = np.empty(3, np.float64)
    G = None if guess is None else to_cm(guess, np.float64)
    _chk(_lib.mvr_ndt_constants(C.byref(params), None if G is None else _p(G, C.c_double), _p(d, C.c_double)))
    return tuple(d)


def ndt_direction(sums):
    """mvr_ndt_direction: rule N7's delta = -H^+ g from the 29 sums -> (delta float64[6], rc); rc is OK or E_SINGULAR"""
    s, d = np.ascontiguousarray(sums, np.float64), np.empty(6, np.float64)
    assert s.shape == (29,)
    rc = _chk(_lib.mvr_ndt_direction(_p(s, C.c_double), _p(d, C.c_double)), allow=(E_SINGULAR,))
    return d, rc


def _ndt_trace(tr, n):
    return [dict(a=tr[k].a, delta_norm=tr[k].delta_norm, trials=tr[k].trials, reversed=bool(tr[k].reversed),
                 fallback=bool(tr[k].fallback), stop=NDT_STOPS[tr[k].stop], score=tr[k].score, count=tr[k].count,
                 p=np.array(tr[k].p, np.float64)) for k in range(n)]


def ndt_newton(params: NdtParams, fn, trace_cap=None):
    """mvr_ndt_newton: rules N7-N9 on the host, from p = 0, on the sums fn(p float64[6]) returns (29 values; an int instead is
    a status: non-zero ends the run at once and comes back as rc) -> dict(rc, stop, converged, iterations, evaluations, p,
    sums, trace); rc is OK, E_NOCORR (stop NO_OVERLAP) or fn's status, and after fn's status only rc is there.  trace_cap:
    the records to keep (default: all)."""
    raised, said = [], []

    def call(user, p, out):
        try:
            r = fn(np.array(p[:6], np.float64))
            if isinstance(r, (int, np.integer)):
                if int(r) == OK:
                    raise ValueError("ndt_newton: fn returned OK without sums")
                said.append(int(r))
                return int(r)
            r = np.asarray(r, np.float64)
            assert r.shape == (29,)
            for k in range(29):
                out[k] = r[k]
            return OK
        except BaseException as e:      # (an exception must not cross the C frames)
            raised.append(e)
            return E_ARG
    cb = NDT_EVAL_FN(call)
    x, sums, st = np.empty(6, np.float64), np.empty(29, np.float64), NdtStats()
    cap = max(1, int(params.max_iterations)) + 1 if trace_cap is None else int(trace_cap)
    tr = (NdtIterTrace * max(1, cap))()
    rc = _lib.mvr_ndt_newton(C.byref(params), cb, None, _p(x, C.c_double), _p(sums, C.c_double), C.byref(st), tr, cap)
    if raised:
        raise raised[0]
    if rc not in (OK, E_NOCORR):
        if not (said and said[-1] == rc):
            _chk(rc)
        return dict(rc=rc)
    n_it = st.iterations + (1 if st.stop in (3, 4) else 0)
    return dict(rc=rc, stop=NDT_STOPS[st.stop], converged=bool(st.converged), iterations=st.iterations, evaluations=st.evaluations,
                p=x, sums=sums, score=st.score, count=st.n_pairs, trace=_ndt_trace(tr, min(cap, n_it)))


def _chain(chain):
    chain = list(chain or ())
    arr = (Rejector * max(1, len(chain)))(*chain)
    return arr, len(chain)


def _stage_dicts(st, n):
    return [dict(n_in=st[k].in_, n_out=st[k].out, threshold=np.float32(st[k].threshold)) for k in range(n)]


def synth_params(n_views=12, config_id=0) -> SynthParams:
    sp = SynthParams()
    _lib.mvr_synth_default(C.byref(sp), n_views, config_id)
    return sp


def synth_view(sp: SynthParams, view: int, n: int, normals=False):
    pts = np.empty((n, 4), np.float32)
    nrm = np.empty((n, 4), np.float32) if normals else None
    _chk(_lib.mvr_synth_view(C.byref(sp), view, n, _p(pts, C.c_float),
                             _p(nrm, C.c_float) if normals else None))
    return (pts, nrm) if normals else pts


def synth_prior(sp: SynthParams):
    piv, ax = np.empty(3), np.empty(3)
    _lib.mvr_synth_prior(C.byref(sp), _p(piv, C.c_double), _p(ax, C.c_double))
    return piv, ax


def turntable_angle(view, n_views=12) -> float:
    return float(_lib.mvr_turntable_angle(view, n_views))


def axis_rotation(pivot, axis, angle):
    p, a = np.ascontiguousarray(pivot, np.float64), np.ascontiguousarray(axis, np.float64)
    T = np.empty(16)
    _lib.mvr_axis_rotation(_p(p, C.c_double), _p(a, C.c_double), float(angle), _p(T, C.c_double))
    return from_cm(T)


def mat4d_mul(A, B):
    a, b, c = to_cm(A, np.float64), to_cm(B, np.float64), np.empty(16)
    _lib.mvr_mat4d_mul(_p(a, C.c_double), _p(b, C.c_double), _p(c, C.c_double))
    return from_cm(c)


def mat4f_mul(A, B):
    a, b, c = to_cm(A, np.float32), to_cm(B, np.float32), np.empty(16, np.float32)
    _lib.mvr_mat4f_mul(_p(a, C.c_float), _p(b, C.c_float), _p(c, C.c_float))
    return from_cm(c)


def pose_to_mat4(pose):
    p, T = np.ascontiguousarray(pose, np.float64), np.empty(16)
    _lib.mvr_pose_to_mat4(_p(p, C.c_double), _p(T, C.c_double))
    return from_cm(T)


def lum_incidence(pose):
    p, H = np.ascontiguousarray(pose, np.float64), np.empty(36)
    _lib.mvr_lum_incidence(_p(p, C.c_double), _p(H, C.c_double))
    return H.reshape(6, 6)


def refine_axis(poses, pivot_y):
    """Registrator::refineAxis on the registered views' (4,4) column-vector poses -> (rc, axis f32[3], pivot f32[3])."""
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16)
    ax, pv = np.zeros(3, np.float32), np.zeros(3, np.float32)
    rc = _lib.mvr_refine_axis(len(P), _p(P, C.c_double), float(np.float32(pivot_y)), _p(ax, C.c_float), _p(pv, C.c_float))
    return rc, ax, pv


def moments_to_dict(m: PairMoments):
    return dict(n=m.n, mean_src=np.array(m.mean_src), mean_tgt=np.array(m.mean_tgt), mse=m.mse,
                sigma=np.array(m.sigma).reshape(3, 3))


def umeyama_from_moments(m: PairMoments):
    T, sv = np.empty(16, np.float32), np.empty(3)
    rc = _lib.mvr_umeyama_from_moments(C.byref(m), _p(T, C.c_float), _p(sv, C.c_double))
    if rc != OK:
        return None, None
    return from_cm(T), sv


def moments_from_moments2(m2: PairMoments2) -> PairMoments:
    out = PairMoments()
    _chk(_lib.mvr_moments_from_moments2(C.byref(m2), C.byref(out)))
    return out


def moments2_from_row(row) -> PairMoments2:
    """32-double device row {n, origin, sp, sq, spp, sqq, spq, 0} -> struct."""
    m2 = PairMoments2()
    C.memmove(C.byref(m2), np.ascontiguousarray(row, np.float64).ctypes.data, C.sizeof(m2))
    return m2


def lum_edge_from_moments(m2: PairMoments2, pose_s, pose_t):
    ps, pt = np.ascontiguousarray(pose_s, np.float64), np.ascontiguousarray(pose_t, np.float64)
    MM, MZ, ss = np.empty(36), np.empty(6), C.c_double()
    rc = _lib.mvr_lum_edge_from_moments(C.byref(m2), _p(ps, C.c_double), _p(pt, C.c_double),
                                        _p(MM, C.c_double), _p(MZ, C.c_double), C.byref(ss))
    return rc, MM.reshape(6, 6), MZ, ss.value


def lum_edge_from_moments_x4(m2s, poses_s, poses_t):
    """Four edges through the AVX2 pass of LUM::computeEdge: (rc, MM[4,6,6], MZ[4,6], ss[4])."""
    arr = (PairMoments2 * 4)(*m2s)
    ps, pt = np.ascontiguousarray(poses_s, np.float64).reshape(4, 6), np.ascontiguousarray(poses_t, np.float64).reshape(4, 6)
    MM, MZ, ss = np.empty((4, 36)), np.empty((4, 6)), np.empty(4)
    rc = _lib.mvr_lum_edge_from_moments_x4(arr, _p(ps, C.c_double), _p(pt, C.c_double), _p(MM, C.c_double), _p(MZ, C.c_double), _p(ss, C.c_double))
    return rc, MM.reshape(4, 6, 6), MZ, ss


_edge_cache = {}


def ring_host_step(n_views, edges, rows, origin, poses, lum_iterations=16):
    """One call for the host side of a global step.  rows: (ne, 32) float64 edge
    table; poses: list of (4,4) float64.  Returns (rc, new_poses, info dict)."""
    ne = len(edges)
    key = tuple(map(tuple, edges))
    if _edge_cache.get("key") != key:                       # the graph of a registration does not change between steps
        _edge_cache.update(key=key, es=(C.c_int * ne)(*[e[0] for e in edges]), et=(C.c_int * ne)(*[e[1] for e in edges]))
    es, et = _edge_cache["es"], _edge_cache["et"]
    R = np.ascontiguousarray(rows, np.float64).reshape(ne, 32)
    o = np.ascontiguousarray(origin, np.float64)
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(n_views, 4, 4).transpose(0, 2, 1)).reshape(n_views, 16)
    lum = np.zeros((n_views, 6))
    pT, pn, pm, its = np.empty((ne, 16), np.float32), np.empty(ne), np.empty(ne), C.c_int()
    rc = _lib.mvr_ring_host_step(n_views, ne, es, et, _p(R, C.c_double), _p(o, C.c_double), int(lum_iterations),
                                 _p(P, C.c_double), _p(lum, C.c_double), _p(pT, C.c_float), _p(pn, C.c_double),
                                 _p(pm, C.c_double), C.byref(its))
    new = list(np.ascontiguousarray(P.reshape(n_views, 4, 4).transpose(0, 2, 1)))
    info = dict(pair_T=list(np.ascontiguousarray(pT.reshape(ne, 4, 4).transpose(0, 2, 1))), pair_n=pn.tolist(),
                pair_mse=pm.tolist(), lum_pose=lum, lum_iterations=its.value)
    return rc, new, info


def lum_compute(n, edges, moments2, max_iterations=5, threshold=0.0, poses=None):
    ne = len(edges)
    es = (C.c_int * ne)(*[e[0] for e in edges])
    et = (C.c_int * ne)(*[e[1] for e in edges])
    arr = (PairMoments2 * ne)(*moments2)
    P = np.zeros((n, 6)) if poses is None else np.array(poses, np.float64).reshape(n, 6)
    P = np.ascontiguousarray(P)
    its = C.c_int()
    rc = _lib.mvr_lum_compute(n, ne, es, et, arr, int(max_iterations), float(threshold),
                              _p(P, C.c_double), C.byref(its))
    return rc, P, its.value


# ------------------------------------------------------------------- context

class Context:
    """One GPU context (mvr_ctx): device clouds in numbered slots + the hot path."""

    def __init__(self, device=0, stream=None):
        h = _vp()
        rc = _lib.mvr_ctx_create_on_stream(C.byref(h), int(device), _vp(stream) if stream else None)
        if rc != OK:
            raise MvrError(rc, "mvr_ctx_create: no usable GPU or HIP failure; there is no CPU fallback")
        self._h = h

    def close(self):
        if self._h:
            _lib.mvr_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- clouds
    def upload(self, slot, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        if pts.ndim != 2 or pts.shape[1] not in (3, 4):
            raise ValueError("points must be (n,4) or (n,3) float32")
        _chk(_lib.mvr_cloud_upload(self._h, slot, _p(pts, C.c_float), len(pts), 4 * pts.shape[1]), self._h)

    def size(self, slot) -> int:
        n = _sz()
        _chk(_lib.mvr_cloud_size(self._h, slot, C.byref(n)), self._h)
        return n.value

    def download(self, slot, packed=False):
        n = self.size(slot)
        out = np.empty((n, 3 if packed else 4), np.float32)
        got = _sz()
        _chk(_lib.mvr_cloud_download(self._h, slot, _p(out, C.c_float), n, 12 if packed else 16,
                                     C.byref(got)), self._h)
        return out

    def upload_normals(self, slot, normals):
        nr = np.ascontiguousarray(normals, np.float32)
        if nr.ndim != 2 or nr.shape[1] not in (3, 4):
            raise ValueError("normals must be (n,4) or (n,3) float32")
        _chk(_lib.mvr_cloud_upload_normals(self._h, slot, _p(nr, C.c_float), len(nr), 4 * nr.shape[1]), self._h)

    def download_normals(self, slot):
        n = self.size(slot)
        out = np.empty((n, 4), np.float32)
        got = _sz()
        _chk(_lib.mvr_cloud_download_normals(self._h, slot, _p(out, C.c_float), n, 16, C.byref(got)), self._h)
        return out[:got.value]

    def reserve(self, slot, cap):
        _chk(_lib.mvr_cloud_reserve(self._h, slot, cap), self._h)

    def copy(self, dst, src):
        _chk(_lib.mvr_cloud_copy(self._h, dst, src), self._h)

    def append(self, dst, src):
        _chk(_lib.mvr_cloud_append(self._h, dst, src), self._h)

    def clear(self, slot):
        _chk(_lib.mvr_cloud_clear(self._h, slot), self._h)

    def transform(self, dst, src, T):
        """getTransformedPoints semantics (f64 pose)."""
        t = to_cm(T, np.float64)
        _chk(_lib.mvr_cloud_transform(self._h, dst, src, _p(t, C.c_double)), self._h)

    def transform_f32(self, dst, src, T):
        """pcl::transformPointCloud semantics (f32 pose)."""
        t = to_cm(T, np.float32)
        _chk(_lib.mvr_cloud_transform_f32(self._h, dst, src, _p(t, C.c_float)), self._h)

    # -- hot path
    def nn(self, q_slot, t_slot, fma=False):
        n = self.size(q_slot)
        idx, d2 = np.empty(n, np.uint32), np.empty(n, np.float32)
        _chk(_lib.mvr_nn(self._h, q_slot, t_slot, int(fma), _p(idx, C.c_uint32), _p(d2, C.c_float)), self._h)
        return idx, d2

    def knn(self, q_slot, t_slot, k, fma=False):
        """exact k nearest neighbours of every point of q_slot in t_slot: (idx[n, k] uint32, d2[n, k] float32), each row
        ascending by (d2, index); UINT32_MAX / +inf where the target holds fewer than k points"""
        n = self.size(q_slot)
        idx, d2 = np.empty((n, k), np.uint32), np.empty((n, k), np.float32)
        _chk(_lib.mvr_knn(self._h, q_slot, t_slot, int(k), int(fma), _p(idx, C.c_uint32), _p(d2, C.c_float)), self._h)
        return idx, d2

    def marching_cubes_hoppe(self, slot, res=(32, 32, 32), iso_level=0.0, percentage_extend_grid=0.0, dist_ignore=-1.0, weld=False,
                             return_grid=False, fma=False, count_only=False):
        """pcl::MarchingCubesHoppe::reconstruct of the cloud in slot with its normals (rules M1-M15:
        mvr_cloud_marching_cubes_hoppe in mvr_hip.h) -> (vertices (3 T, 3) float32, polygons (T, 3) uint32[, grid res float32]);
        polygon t of the soup is (3t, 3t + 1, 3t + 2).  weld: the welded vertices (V, 3) and the polygons over them (M13).
        count_only: (T[, grid])."""
        res = tuple(int(r) for r in res)
        if len(res) != 3:
            raise ValueError("res must have three entries")
        p = McParams((C.c_int * 3)(*res), float(iso_level), float(percentage_extend_grid), float(dist_ignore), int(bool(weld)), int(bool(fma)))
        lattice = res[0] * res[1] * res[2]
        grid = np.empty(res, np.float32) if return_grid and min(res) >= 2 and lattice <= MC_MAX_VERTICES else None
        gp = _p(grid, C.c_float) if grid is not None else None
        T, V = C.c_uint64(0), C.c_uint64(0)
        if count_only:
            _chk(_lib.mvr_cloud_marching_cubes_hoppe(self._h, int(slot), C.byref(p), gp, None, 0, None, C.byref(T), C.byref(V)), self._h)
            return (int(T.value), grid) if return_grid else int(T.value)
        # a first capacity from the lattice's faces; a surface that needs more says how much (M11) and is asked again
        cap = max(1024, 8 * (res[0] * res[1] + res[1] * res[2] + res[0] * res[2])) if min(res) >= 2 else 1
        while True:
            verts = np.empty((3 * cap, 3), np.float32)
            idx = np.empty(3 * cap, np.uint32) if weld else None
            rc = _lib.mvr_cloud_marching_cubes_hoppe(self._h, int(slot), C.byref(p), gp, _p(verts, C.c_float), cap,
                                                     _p(idx, C.c_uint32) if weld else None, C.byref(T), C.byref(V))
            if rc == E_ARG and int(T.value) > cap:
                cap = int(T.value)
                continue
            _chk(rc, self._h)
            break
        t, v = int(T.value), int(V.value)
        polys = idx[:3 * t].reshape(t, 3).copy() if weld else np.arange(3 * t, dtype=np.uint32).reshape(t, 3)
        out = (verts[:v].copy(), polys)
        return out + (grid,) if return_grid else out

    def radius_search(self, q_slot, t_slot, radius, max_nn=0, sorted=True, fma=False, count_only=False):
        """pcl::search::KdTree::radiusSearch of every point of q_slot in t_slot, as CSR lists (rules RS1-RS11: mvr_radius_search
        in mvr_hip.h): (offsets uint64[n + 1], idx uint32[total], d2 float32[total]), the row of query i at offsets[i] ..
        offsets[i + 1], ascending by (d2, index) when sorted or capped by max_nn > 0.  count_only: (offsets, total)."""
        if not (math.isfinite(float(radius)) and float(radius) > 0.0):
            raise ValueError("radius must be finite and > 0")
        if not 0 <= int(max_nn) <= 0xFFFFFFFF:
            raise ValueError("max_nn must be in 0..2^32 - 1")
        for s in (q_slot, t_slot):
            if not 0 <= int(s) < MAX_SLOTS:
                raise ValueError("bad slot %r" % (s,))
        n = self.size(int(q_slot))
        p = RadiusParams(float(radius), int(max_nn), int(bool(sorted)), int(bool(fma)))
        offsets = np.empty(n + 1, np.uint64)
        total = _sz(0)
        _chk(_lib.mvr_radius_search(self._h, int(q_slot), int(t_slot), C.byref(p), _p(offsets, C.c_uint64), None, None, 0, C.byref(total)), self._h)
        if count_only:
            return offsets, int(total.value)
        m = int(total.value)
        idx, d2 = np.empty(m, np.uint32), np.empty(m, np.float32)
        if m:
            _chk(_lib.mvr_radius_search(self._h, int(q_slot), int(t_slot), C.byref(p), _p(offsets, C.c_uint64), _p(idx, C.c_uint32),
                                        _p(d2, C.c_float), m, C.byref(total)), self._h)
        return offsets, idx, d2

    def estimate_normals(self, slots, k=None, radius=None, viewpoint=(0.0, 0.0, 0.0), curvature=False, fma=False):
        """pcl::NormalEstimation of every slot against itself (one call): the normals go into the slots (download_normals,
        point-to-plane ICP).  Exactly one of k / radius.  curvature=True returns the curvature array (a list of them when
        `slots` is a list)."""
        one = np.isscalar(slots)
        sl = [int(slots)] if one else [int(s) for s in slots]
        p = NormalParams(int(k or 0), float(radius or 0.0), (C.c_float * 3)(*[float(v) for v in viewpoint]), int(fma))
        arr = (C.c_int * max(len(sl), 1))(*sl)
        curv = [np.empty(self.size(s), np.float32) for s in sl] if curvature else None
        cptr = (_fp * max(len(sl), 1))(*[_p(a, C.c_float) for a in curv]) if curvature else None
        _chk(_lib.mvr_cloud_estimate_normals(self._h, len(sl), arr, C.byref(p), cptr), self._h)
        if not curvature:
            return None
        return curv[0] if one else curv

    def denoise(self, slot, segment_threshold=10, triangle_length=2.5):
        """PointCloud::denoise in place.  Returns (kept original indices in output order, number of components).
        A point with a non-finite x, y or z is linked to nothing: a component of its own (counted; kept exactly when
        segment_threshold <= 1, at its place in the order) that takes no part in the sizing of the grid; a cloud with no
        finite point is sized like a single point (rules D1-D4 of mvr_cloud_denoise in mvr_hip.h)."""
        n = self.size(slot)
        idx = np.empty(max(n, 1), np.uint32)
        kept, comps = C.c_size_t(), C.c_size_t()
        _chk(_lib.mvr_cloud_denoise(self._h, slot, int(segment_threshold), float(triangle_length), C.byref(kept), C.byref(comps),
                                    _p(idx, C.c_uint32)), self._h)
        return idx[:kept.value].copy(), comps.value

    def voxel_grid(self, dst, src, leaf, min_points=0, return_map=False):
        """pcl::VoxelGrid::filter of slot src into slot dst (may be src): the centroid of every occupied voxel, in ascending
        voxel index, averaged normals when src has normals (rules: mvr_cloud_voxel_grid in mvr_hip.h).  leaf: a scalar or
        three values.  Returns n_out, or (n_out, voxel_of) with return_map (voxel_of[i]: output position of source point i's
        voxel, UINT32_MAX for a non-finite point or a dropped voxel).  When PCL's integer indices would overflow, the output
        is a copy of the input and a warning says so, as PCL's does."""
        lf = np.asarray(leaf, np.float32).reshape(-1)
        if lf.size == 1:
            lf = np.repeat(lf, 3)
        if lf.size != 3:
            raise ValueError("leaf must be a scalar or three values")
        lf = np.ascontiguousarray(lf)
        n = self.size(src)
        vmap = np.empty(max(n, 1), np.uint32) if return_map else None
        n_out, passthrough = _sz(), C.c_int()
        _chk(_lib.mvr_cloud_voxel_grid(self._h, int(dst), int(src), _p(lf, C.c_float), int(min_points), C.byref(n_out),
                                       _p(vmap, C.c_uint32) if return_map else None, C.byref(passthrough)), self._h)
        if passthrough.value:
            warnings.warn("[pcl::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. "
                          "Integer indices would overflow.")
        if return_map:
            return n_out.value, vmap[:n]
        return n_out.value

    def statistical_outlier_removal(self, dst, src, mean_k, stddev_mul, negative=False, fma=False, return_index=False,
                                    return_dist=False, return_stats=False):
        """pcl::StatisticalOutlierRemoval::filter of slot src into slot dst (may be src): the points whose mean distance to
        their mean_k nearest other points is not above mean + stddev_mul * stddev, in their original order (negative: the
        complement); normals follow (rules: mvr_cloud_statistical_outlier_removal in mvr_hip.h).  Returns n_out, or a tuple
        (n_out[, kept_index][, mean_dist][, stats]) with the return_* options: kept_index = original indices of the output
        points, mean_dist = one f32 per SOURCE point (NaN for a non-finite point), stats = dict(mean, stddev, threshold,
        n_valid)."""
        n = self.size(src)
        p = SorParams(int(mean_k), float(stddev_mul), int(bool(negative)), int(bool(fma)))
        idx = np.empty(max(n, 1), np.uint32) if return_index else None
        md = np.empty(max(n, 1), np.float32) if return_dist else None
        st, n_out = SorStats(), _sz()
        _chk(_lib.mvr_cloud_statistical_outlier_removal(self._h, int(dst), int(src), C.byref(p), C.byref(n_out),
                                                        _p(idx, C.c_uint32) if return_index else None,
                                                        _p(md, C.c_float) if return_dist else None, C.byref(st)), self._h)
        out = [n_out.value]
        if return_index:
            out.append(idx[:n_out.value].copy())
        if return_dist:
            out.append(md[:n])
        if return_stats:
            out.append({"mean": st.mean, "stddev": st.stddev, "threshold": st.threshold, "n_valid": int(st.n_valid)})
        return out[0] if len(out) == 1 else tuple(out)

    def radius_outlier_removal(self, dst, src, radius, min_neighbors, negative=False, fma=False, return_index=False,
                               return_counts=False):
        """pcl::RadiusOutlierRemoval::filter of slot src into slot dst (may be src): the points with at least min_neighbors
        other points within radius, in their original order (negative: the complement); normals follow (rules:
        mvr_cloud_radius_outlier_removal in mvr_hip.h).  Returns n_out, or (n_out[, kept_index][, neighbor_count]); the
        counts are one uint32 per SOURCE point."""
        n = self.size(src)
        p = RorParams(float(radius), int(min_neighbors), int(bool(negative)), int(bool(fma)))
        idx = np.empty(max(n, 1), np.uint32) if return_index else None
        cnt = np.empty(max(n, 1), np.uint32) if return_counts else None
        n_out = _sz()
        _chk(_lib.mvr_cloud_radius_outlier_removal(self._h, int(dst), int(src), C.byref(p), C.byref(n_out),
                                                   _p(idx, C.c_uint32) if return_index else None,
                                                   _p(cnt, C.c_uint32) if return_counts else None), self._h)
        out = [n_out.value]
        if return_index:
            out.append(idx[:n_out.value].copy())
        if return_counts:
            out.append(cnt[:n])
        return out[0] if len(out) == 1 else tuple(out)

    def mls(self, dst, src, radius, order=2, sqr_gauss_param=0.0, compute_normals=False, orient="viewpoint",
            viewpoint=(0.0, 0.0, 0.0), fma=False, return_index=False, return_curvature=False):
        """pcl::MovingLeastSquares::process of slot src into slot dst (may be src): every point with at least 3 neighbours
        within radius, projected onto the plane through them and -- order 2, at least 6 neighbours -- onto the weighted
        quadratic fitted over that plane, in their original order (rules: mvr_cloud_mls in mvr_hip.h).  sqr_gauss_param 0
        selects radius * radius.  compute_normals replaces the slot's normals by those of the fit, oriented towards
        `viewpoint` (orient="viewpoint") or along the source slot's own normals (orient="normals"); without it the source's
        normals follow their points.  Returns n_out, or (n_out[, kept_index][, curvature]): kept_index = original indices
        of the output points, curvature = one f32 per OUTPUT point."""
        if orient not in ("viewpoint", "normals"):
            raise ValueError("orient must be 'viewpoint' or 'normals'")
        n = self.size(src)
        p = MlsParams(float(radius), int(order), float(sqr_gauss_param), int(bool(compute_normals)), int(orient == "normals"),
                      (C.c_float * 3)(*[float(v) for v in viewpoint]), int(bool(fma)))
        idx = np.empty(max(n, 1), np.uint32) if return_index else None
        curv = np.empty(max(n, 1), np.float32) if return_curvature else None
        n_out = _sz()
        _chk(_lib.mvr_cloud_mls(self._h, int(dst), int(src), C.byref(p), C.byref(n_out),
                                _p(idx, C.c_uint32) if return_index else None,
                                _p(curv, C.c_float) if return_curvature else None), self._h)
        out = [n_out.value]
        if return_index:
            out.append(idx[:n_out.value].copy())
        if return_curvature:
            out.append(curv[:n_out.value].copy())
        return out[0] if len(out) == 1 else tuple(out)

    def fpfh(self, slot, radius, fma=False, return_spfh=False, return_counts=False):
        """pcl::FPFHEstimation::compute of slot against itself, radius mode, with the slot's own normals (estimate_normals or
        upload_normals first): the (n, 33) float32 signatures, row = point index (rules: mvr_cloud_fpfh in mvr_hip.h).  A point
        with a non-finite coordinate or normal gets a NaN row.  Returns the signatures, or (fpfh[, spfh][, neighbor_count])
        with the return_* options: spfh = the intermediate (n, 33) simplified histograms, neighbor_count = one uint32 per
        point, the point itself included."""
        n = self.size(slot)
        p = FpfhParams(float(radius), int(bool(fma)))
        out = np.empty((n, 3 * FPFH_BINS), np.float32)
        sp = np.empty((n, 3 * FPFH_BINS), np.float32) if return_spfh else None
        cnt = np.empty(n, np.uint32) if return_counts else None
        _chk(_lib.mvr_cloud_fpfh(self._h, int(slot), C.byref(p), _p(out, C.c_float), _p(sp, C.c_float) if return_spfh else None,
                                 _p(cnt, C.c_uint32) if return_counts else None), self._h)
        res = [out]
        if return_spfh:
            res.append(sp)
        if return_counts:
            res.append(cnt)
        return res[0] if len(res) == 1 else tuple(res)

    def pfh(self, slot, radius=None, k=None, fma=False, return_counts=False, return_neighbors=False):
        """pcl::PFHEstimation::compute of slot against itself with the slot's own normals (estimate_normals or upload_normals
        first), exactly one of radius / k (1..MAX_KNN) set: the (n, 125) float32 signatures, row = point index (rules P1-P8:
        mvr_cloud_pfh in mvr_hip.h).  A point with a non-finite coordinate or normal gets a NaN row.  Returns the signatures, or
        (pfh[, counts][, neighbor_count]) with the return_* options: counts = the (n, 125) uint32 pair counts the signatures
        are scaled from, neighbor_count = one uint32 per point (radius mode: the point itself included)."""
        if (radius is None) == (k is None):
            raise ValueError("exactly one of radius / k")
        if k is not None and not 1 <= int(k) <= MAX_KNN:
            raise ValueError("k must be in 1..%d" % MAX_KNN)
        if radius is not None and not (math.isfinite(float(radius)) and float(radius) > 0.0):
            raise ValueError("radius must be finite and > 0")
        n = self.size(slot)
        p = PfhParams(float(radius or 0.0), int(k or 0), int(bool(fma)))
        out = np.empty((n, PFH_DIM), np.float32)
        cnt = np.empty((n, PFH_DIM), np.uint32) if return_counts else None
        nb = np.empty(n, np.uint32) if return_neighbors else None
        _chk(_lib.mvr_cloud_pfh(self._h, int(slot), C.byref(p), _p(out, C.c_float), _p(cnt, C.c_uint32) if return_counts else None,
                                _p(nb, C.c_uint32) if return_neighbors else None), self._h)
        res = [out]
        if return_counts:
            res.append(cnt)
        if return_neighbors:
            res.append(nb)
        return res[0] if len(res) == 1 else tuple(res)

    def _at_rows(self, q_slot, indices):
        """the query convention of the *_at calls (rule Q1): (indices as a contiguous uint32 array or None, its pointer, rows)"""
        if indices is None:
            return None, None, self.size(q_slot)
        a = np.asarray(indices)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("indices must be a one-dimensional integer array")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("indices must fit 32 unsigned bits")
        a = np.ascontiguousarray(a, np.uint32)
        # (a non-NULL pointer also for an empty list: NULL means "every point")
        return a, (_p(a, C.c_uint32) if a.size else C.cast((C.c_uint32 * 1)(), _u32p)), int(a.size)

    def estimate_normals_at(self, q_slot, surface_slot, indices=None, k=None, radius=None, viewpoint=(0.0, 0.0, 0.0), store=False,
                            fma=False):
        """pcl::NormalEstimation at the points `indices` of q_slot (None: all of them) with surface_slot as search surface
        (setSearchSurface / setIndices; rules Q1-Q8: mvr_cloud_estimate_normals_at in mvr_hip.h).  Exactly one of k / radius.
        Returns (normals (rows, 3) float32, curvature (rows,) float32); store=True (indices None only) also puts the normals
        into q_slot."""
        _, ptr, rows = self._at_rows(q_slot, indices)
        p = NormalParams(int(k or 0), float(radius or 0.0), (C.c_float * 3)(*[float(v) for v in viewpoint]), int(bool(fma)))
        nrm = np.empty((rows, 4), np.float32)
        curv = np.empty(rows, np.float32)
        _chk(_lib.mvr_cloud_estimate_normals_at(self._h, int(q_slot), ptr, rows if ptr is not None else 0, int(surface_slot), C.byref(p),
                                                int(bool(store)), _p(nrm, C.c_float), _p(curv, C.c_float)), self._h)
        return nrm[:, :3].copy(), curv

    def fpfh_at(self, q_slot, surface_slot, radius, indices=None, fma=False, return_counts=False):
        """pcl::FPFHEstimation at the points `indices` of q_slot (None: all of them) over surface_slot and ITS normals
        (setSearchSurface / setIndices; rules Q1-Q8: mvr_cloud_fpfh_at in mvr_hip.h): the (rows, 33) float32 signatures, row r
        for indices[r]; with return_counts also neighbor_count (rows,) uint32.  Only the SPFH rows the queries' neighbours
        need are computed."""
        _, ptr, rows = self._at_rows(q_slot, indices)
        p = FpfhParams(float(radius), int(bool(fma)))
        out = np.empty((rows, 3 * FPFH_BINS), np.float32)
        cnt = np.empty(rows, np.uint32) if return_counts else None
        _chk(_lib.mvr_cloud_fpfh_at(self._h, int(q_slot), ptr, rows if ptr is not None else 0, int(surface_slot), C.byref(p),
                                    _p(out, C.c_float), _p(cnt, C.c_uint32) if return_counts else None), self._h)
        return (out, cnt) if return_counts else out

    def pfh_at(self, q_slot, surface_slot, indices=None, radius=None, k=None, fma=False, return_counts=False, return_neighbors=False):
        """pcl::PFHEstimation at the points `indices` of q_slot (None: all of them) over surface_slot and ITS normals, exactly
        one of radius / k set (rules Q1-Q8: mvr_cloud_pfh_at in mvr_hip.h): the (rows, 125) float32 signatures, or
        (pfh[, counts][, neighbor_count]) with the return_* options, as pfh() gives them."""
        if (radius is None) == (k is None):
            raise ValueError("exactly one of radius / k")
        _, ptr, rows = self._at_rows(q_slot, indices)
        p = PfhParams(float(radius or 0.0), int(k or 0), int(bool(fma)))
        out = np.empty((rows, PFH_DIM), np.float32)
        cnt = np.empty((rows, PFH_DIM), np.uint32) if return_counts else None
        nb = np.empty(rows, np.uint32) if return_neighbors else None
        _chk(_lib.mvr_cloud_pfh_at(self._h, int(q_slot), ptr, rows if ptr is not None else 0, int(surface_slot), C.byref(p),
                                   _p(out, C.c_float), _p(cnt, C.c_uint32) if return_counts else None,
                                   _p(nb, C.c_uint32) if return_neighbors else None), self._h)
        res = [out]
        if return_counts:
            res.append(cnt)
        if return_neighbors:
            res.append(nb)
        return res[0] if len(res) == 1 else tuple(res)

    @staticmethod
    def _shot_params(radius, lrf_radius, fma):
        return ShotParams(float(radius), float(radius if lrf_radius is None else lrf_radius), int(bool(fma)))

    def shot_lrf(self, slot, radius, fma=False, return_neighbors=False):
        """pcl::SHOTLocalReferenceFrameEstimation::compute of slot against itself (rules L1-L7: mvr_cloud_shot in mvr_hip.h; no
        normals needed): the (n, 9) float32 frames, row-major x, y, z axes, NaN where fewer than 5 OTHER points lie within radius;
        with return_neighbors also their number, (n,) uint32."""
        n = self.size(slot)
        p = self._shot_params(radius, 0.0, fma)
        out = np.empty((n, 9), np.float32)
        nb = np.empty(n, np.uint32) if return_neighbors else None
        _chk(_lib.mvr_cloud_shot_lrf(self._h, int(slot), C.byref(p), _p(out, C.c_float), _p(nb, C.c_uint32) if return_neighbors else None),
             self._h)
        return (out, nb) if return_neighbors else out

    def _shot_call(self, rows, call, lrf, return_lrf, return_sums, return_neighbors):
        fr = None
        if lrf is not None:
            fr = np.ascontiguousarray(lrf, np.float32)
            if fr.shape != (rows, 9):
                raise ValueError("lrf must be a (rows, 9) float32 table")
        out = np.empty((rows, SHOT_DIM), np.float32)
        lo = np.empty((rows, 9), np.float32) if return_lrf else None
        sm = np.empty((rows, SHOT_DIM), np.uint64) if return_sums else None
        nb = np.empty(rows, np.uint32) if return_neighbors else None
        _chk(call(_p(fr, C.c_float) if fr is not None and rows else None, _p(out, C.c_float), _p(lo, C.c_float) if return_lrf else None,
                  _p(sm, C.c_uint64) if return_sums else None, _p(nb, C.c_uint32) if return_neighbors else None), self._h)
        res = [out] + [x for x, want in ((lo, return_lrf), (sm, return_sums), (nb, return_neighbors)) if want]
        return res[0] if len(res) == 1 else tuple(res)

    def shot(self, slot, radius, lrf_radius=None, lrf=None, fma=False, return_lrf=False, return_sums=False, return_neighbors=False):
        """pcl::SHOTEstimation::compute (SHOT352) of slot against itself with the slot's own normals (rules L1-L7 and H1-H9:
        mvr_cloud_shot in mvr_hip.h): the (n, 352) float32 unit-norm signatures, row = point index.  lrf_radius (None: radius)
        is setLRFRadius; lrf, an (n, 9) table, is setInputReferenceFrames (no frame is then computed).  Returns the signatures,
        or (shot[, lrf][, sums][, neighbor_count]) with the return_* options: lrf = the frames used, sums = the (n, 352) uint64
        fixed-point sums the rows are normalised from, neighbor_count = one uint32 per point (the point itself included)."""
        p = self._shot_params(radius, lrf_radius, fma)
        return self._shot_call(self.size(slot), lambda *a: _lib.mvr_cloud_shot(self._h, int(slot), C.byref(p), *a), lrf, return_lrf,
                               return_sums, return_neighbors)

    def shot_at(self, q_slot, surface_slot, radius, indices=None, lrf_radius=None, lrf=None, fma=False, return_lrf=False,
                return_sums=False, return_neighbors=False):
        """pcl::SHOTEstimation at the points `indices` of q_slot (None: all of them) over surface_slot and ITS normals
        (setSearchSurface / setIndices; rules Q1-Q8): the (rows, 352) float32 signatures, row r for indices[r], and the
        return_* options of shot(); lrf is a (rows, 9) table."""
        _, ptr, rows = self._at_rows(q_slot, indices)
        p = self._shot_params(radius, lrf_radius, fma)
        return self._shot_call(rows, lambda *a: _lib.mvr_cloud_shot_at(self._h, int(q_slot), ptr, rows if ptr is not None else 0,
                                                                       int(surface_slot), C.byref(p), *a), lrf, return_lrf, return_sums,
                               return_neighbors)

    def boundary(self, slot, radius, angle_threshold=math.pi / 2, min_neighbors=0, fma=False, return_gap=False, return_counts=False):
        """pcl::BoundaryEstimation::compute of slot against itself, radius mode, with the slot's own normals (estimate_normals or
        upload_normals first): one bool per point, whether the neighbours within radius, projected onto the point's tangent
        plane, leave an angular gap above angle_threshold (rules B1-B7: mvr_cloud_boundary in mvr_hip.h; angle_threshold in
        [BOUNDARY_MIN_ANGLE, 2 pi)).  min_neighbors > 0 also asks for that many neighbours, the point itself included.  Returns
        the flags, or (flags[, max_gap][, neighbor_count]) with the return_* options: max_gap = one float32 per point, the
        largest gap (exact from a sector width, pi / 8, upwards), neighbor_count = one uint32 per point."""
        n = self.size(slot)
        p = BoundaryParams(float(radius), float(angle_threshold), int(min_neighbors), int(bool(fma)))
        flag = np.empty(max(n, 1), np.uint8)
        gap = np.empty(max(n, 1), np.float32) if return_gap else None
        cnt = np.empty(max(n, 1), np.uint32) if return_counts else None
        _chk(_lib.mvr_cloud_boundary(self._h, int(slot), C.byref(p), _p(flag, C.c_uint8), _p(gap, C.c_float) if return_gap else None,
                                     _p(cnt, C.c_uint32) if return_counts else None), self._h)
        res = [flag[:n].astype(bool)]
        if return_gap:
            res.append(gap[:n])
        if return_counts:
            res.append(cnt[:n])
        return res[0] if len(res) == 1 else tuple(res)

    def iss_keypoints(self, dst, src, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, fma=False,
                      return_index=False, return_saliency=False, return_counts=False, *, border_radius=0.0, angle_threshold=math.pi / 2,
                      return_edges=False):
        """pcl::ISSKeypoint3D::compute of slot src into slot dst (may be src; -1: no output slot, the host arrays only): the
        points whose scatter over salient_radius passes both eigenvalue ratio tests and whose smallest eigenvalue no neighbour
        within non_max_radius exceeds, in their original order; normals follow (rules K1-K11: mvr_cloud_iss_keypoints in
        mvr_hip.h).  border_radius > 0 (the slot then needs normals) first drops every point that has a boundary point --
        Context.boundary at border_radius, angle_threshold and this call's min_neighbors -- within border_radius.  Returns
        n_out, or (n_out[, kept_index][, saliency][, salient_count, nms_count][, edge, border]) with the return_* options:
        kept_index = original indices of the keypoints, saliency = one float64 per SOURCE point (0: not salient), the counts
        one uint32 per SOURCE point, edge / border = one bool per SOURCE point (all False without a border radius)."""
        n = self.size(src)
        p = IssParams(float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32), int(min_neighbors), int(bool(fma)))
        idx = np.empty(max(n, 1), np.uint32) if return_index else None
        sal = np.empty(max(n, 1), np.float64) if return_saliency else None
        sc = np.empty(max(n, 1), np.uint32) if return_counts else None
        nc = np.empty(max(n, 1), np.uint32) if return_counts else None
        n_out = _sz()
        args = (_p(idx, C.c_uint32) if return_index else None, _p(sal, C.c_double) if return_saliency else None,
                _p(sc, C.c_uint32) if return_counts else None, _p(nc, C.c_uint32) if return_counts else None)
        edge = border = None
        if float(border_radius) == 0.0:
            _chk(_lib.mvr_cloud_iss_keypoints(self._h, int(dst), int(src), C.byref(p), C.byref(n_out), *args), self._h)
            if return_edges:
                edge, border = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        else:
            b = IssBorderParams(float(border_radius), float(angle_threshold))
            if return_edges:
                edge, border = np.empty(max(n, 1), np.uint8), np.empty(max(n, 1), np.uint8)
            _chk(_lib.mvr_cloud_iss_keypoints_border(self._h, int(dst), int(src), C.byref(p), C.byref(b), C.byref(n_out), *args,
                                                     _p(edge, C.c_uint8) if return_edges else None,
                                                     _p(border, C.c_uint8) if return_edges else None), self._h)
        out = [n_out.value]
        if return_index:
            out.append(idx[:n_out.value].copy())
        if return_saliency:
            out.append(sal[:n])
        if return_counts:
            out += [sc[:n], nc[:n]]
        if return_edges:
            out += [edge[:n].astype(bool), border[:n].astype(bool)]
        return out[0] if len(out) == 1 else tuple(out)

    def segment_plane(self, dst, src, threshold, model="plane", max_iterations=1000, probability=0.99, optimize=True, axis=None,
                      eps_angle=None, seed=0, negative=False, fma=False, return_index=False, return_trace=False):
        """pcl::SACSegmentation (SAC_RANSAC; model "plane" or "perpendicular_plane" with axis and eps_angle) of slot src, then
        pcl::ExtractIndices into slot dst (may be src; -1: no output slot): the largest plane's inliers, or with negative
        everything else (rules P1-P12: mvr_cloud_segment_plane in mvr_hip.h).  A pure function of its arguments, seed
        included.  Returns a dict(found, inliers, ransac_inliers, iterations, attempts, skipped, best_attempt, k,
        coefficients (4) float32, ransac_coefficients (4) float32, n_out), followed with return_index by the inliers' original
        indices (ascending, uint32) and with return_trace by dict(status[t], sample[t, 3], coefficients[t, 4], inliers[t],
        k[t]) over the attempts made."""
        if model not in SAC_MODELS:
            raise ValueError("model must be one of %s" % sorted(SAC_MODELS))
        n = self.size(src)
        ax = (0.0, 0.0, 0.0) if axis is None else tuple(float(v) for v in axis)
        p = SacParams(SAC_MODELS[model], float(threshold), int(max_iterations), float(probability), int(bool(optimize)),
                      (C.c_double * 3)(*ax), 0.0 if eps_angle is None else float(eps_angle), int(seed), int(bool(negative)), int(bool(fma)))
        res = SacResult()
        n_out = _sz()
        idx = np.empty(max(n, 1), np.uint32) if return_index else None
        cap = 11 * max(int(max_iterations), 0) + 1 if return_trace else 0      # counted attempts <= max_iterations + 1, skipped <= 10 x
        tr = (SacTrace * cap)() if return_trace else None
        _chk(_lib.mvr_cloud_segment_plane(self._h, int(dst), int(src), C.byref(p), C.byref(res), C.byref(n_out),
                                          _p(idx, C.c_uint32) if return_index else None, None, tr, cap), self._h)
        out = [dict(found=bool(res.found), inliers=int(res.inliers), ransac_inliers=int(res.ransac_inliers), iterations=res.iterations,
                    attempts=res.attempts, skipped=res.skipped, best_attempt=res.best_attempt, k=res.k,
                    coefficients=np.array(res.coefficients, np.float32), ransac_coefficients=np.array(res.ransac_coefficients, np.float32),
                    n_out=n_out.value)]
        if return_index:
            out.append(idx[:res.inliers].copy())
        if return_trace:
            dt = np.dtype([("status", np.int32), ("sample", np.uint32, 3), ("coefficients", np.float32, 4), ("inliers", np.uint32),
                           ("k", np.float64)], align=True)
            assert dt.itemsize == C.sizeof(SacTrace)
            a = np.frombuffer(tr, dtype=dt, count=cap)[:res.attempts].copy()
            out.append({k: np.ascontiguousarray(a[k]) for k in ("status", "sample", "coefficients", "inliers", "k")})
        return out[0] if len(out) == 1 else tuple(out)

    def extract_indices(self, dst, src, index, negative=False) -> int:
        """pcl::ExtractIndices::filter: slot dst (may be src) gets the points of slot src listed in index, or with negative all
        the others, in ascending original index, normals following (mvr_cloud_extract_indices).  Returns their number."""
        idx = np.ascontiguousarray(index, np.uint32).ravel()
        n_out = _sz()
        _chk(_lib.mvr_cloud_extract_indices(self._h, int(dst), int(src), _p(idx, C.c_uint32) if len(idx) else None, len(idx),
                                            int(bool(negative)), C.byref(n_out)), self._h)
        return n_out.value

    def euclidean_clusters(self, dst, src, tolerance, min_size=1, max_size=2**31 - 1, eps_angle=None, index=None, negative=False,
                           keep=1, fma=False, return_lists=False, return_labels=False):
        """pcl::EuclideanClusterExtraction of slot src (rules E1-E8: mvr_cloud_euclidean_clusters in mvr_hip.h): the connected
        components of the points within `tolerance` of each other whose size lies in [min_size, max_size], largest first;
        with eps_angle (radians) the slot's normals must also agree (pcl::extractEuclideanClusters with normals).  index
        (setIndices; None: every point) restricts the clustering to the listed points, or with negative to the others.  Slot
        dst (may be src; -1: no output slot) gets the first `keep` clusters in ascending original index.  Returns a
        dict(n_active, n_components, n_clusters, n_clustered, largest, too_small, too_large, n_out), followed with
        return_lists by the list of the clusters' index arrays (uint32, ascending) and with return_labels by the rank of every
        point's cluster (uint32; UINT32_MAX: in none)."""
        n = self.size(src)
        p = ClusterParams(float(tolerance), int(min_size), int(max_size), int(eps_angle is not None),
                          0.0 if eps_angle is None else float(eps_angle), int(bool(negative)), int(keep), int(bool(fma)))
        idx, count = None, 0
        if index is not None:
            idx = np.ascontiguousarray(index, np.uint32).ravel()
            count = len(idx)
            if count == 0:
                idx = np.zeros(1, np.uint32)      # an empty list is still a list (E1): the pointer must not be NULL
        res = ClusterResult()
        n_out = _sz()
        off = np.empty(n + 2, np.uint32) if return_lists else None
        cidx = np.empty(max(n, 1), np.uint32) if return_lists else None
        lab = np.empty(max(n, 1), np.uint32) if return_labels else None
        _chk(_lib.mvr_cloud_euclidean_clusters(self._h, int(dst), int(src), C.byref(p), _p(idx, C.c_uint32) if idx is not None else None, count,
                                               C.byref(res), C.byref(n_out), _p(off, C.c_uint32) if return_lists else None,
                                               n + 2 if return_lists else 0, _p(cidx, C.c_uint32) if return_lists else None,
                                               _p(lab, C.c_uint32) if return_labels else None), self._h)
        out = [dict(n_active=int(res.n_active), n_components=int(res.n_components), n_clusters=int(res.n_clusters),
                    n_clustered=int(res.n_clustered), largest=int(res.largest), too_small=int(res.too_small), too_large=int(res.too_large),
                    n_out=n_out.value)]
        if return_lists:
            out.append([cidx[off[k]:off[k + 1]].copy() for k in range(res.n_clusters)])
        if return_labels:
            out.append(lab[:n].copy())
        return out[0] if len(out) == 1 else tuple(out)

    def feature_knn(self, q, t, k):
        """exact k nearest neighbours of every row of q among the rows of t in feature space (33, 125 or 352 floats per row, FLANN's
        L2_Simple in f32; rules M1-M3: mvr_feature_knn in mvr_hip.h): (idx[nq, k] uint32, d2[nq, k] float32), each row ascending
        by (d2, index); UINT32_MAX / +inf for a non-finite query row and beyond the listable targets"""
        q, t = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)
        if q.ndim != 2 or t.ndim != 2 or q.shape[1] != t.shape[1]:
            raise ValueError("q and t must be (n, dim) float32 tables of one dim")
        idx, d2 = np.empty((len(q), k), np.uint32), np.empty((len(q), k), np.float32)
        _chk(_lib.mvr_feature_knn(self._h, _p(q, C.c_float), len(q), _p(t, C.c_float), len(t), q.shape[1], int(k),
                                  _p(idx, C.c_uint32), _p(d2, C.c_float)), self._h)
        return idx, d2

    def pose_scores(self, src, tgt, T, max_dist, fma=False):
        """inliers and error of every pose in T ((count, 4, 4), math layout) of slot src against slot tgt (rules S1-S2:
        mvr_pose_scores in mvr_hip.h): (inliers[count] uint32, error[count] float64; DBL_MAX where no point is an inlier)"""
        T = np.asarray(T, np.float32).reshape(-1, 4, 4)
        cm = np.ascontiguousarray(T.transpose(0, 2, 1)).reshape(-1, 16)
        inl, err = np.empty(len(cm), np.uint32), np.empty(len(cm), np.float64)
        _chk(_lib.mvr_pose_scores(self._h, int(src), int(tgt), _p(cm, C.c_float), len(cm), float(max_dist), int(bool(fma)),
                                  _p(inl, C.c_uint32), _p(err, C.c_double)), self._h)
        return inl, err

    def align_prerejective(self, src, tgt, src_feat, tgt_feat, max_iterations=1000, nr_samples=3, k=2, similarity=0.9,
                           max_dist=4.0, inlier_fraction=0.25, seed=0, fma=False, guess=None, return_trace=False):
        """pcl::SampleConsensusPrerejective::align of slot src onto slot tgt from their (n, 33), (n, 125) or (n, 352) descriptors (rules A1-A6:
        mvr_align_prerejective in mvr_hip.h; k = setCorrespondenceRandomness).  A pure function of its arguments.  Returns a
        dict(converged, best_iteration, inliers, error, rejected, scored, T (4, 4) float32), or (that, trace) with return_trace:
        trace = dict(status[it], src[it, nr_samples], tgt[it, nr_samples], inliers[it], error[it], T[it, 4, 4])."""
        sf, tf = np.ascontiguousarray(src_feat, np.float32), np.ascontiguousarray(tgt_feat, np.float32)
        dim = sf.shape[1] if sf.ndim == 2 else 0
        if dim not in (3 * FPFH_BINS, PFH_DIM, SHOT_DIM) or sf.shape != (self.size(src), dim) or tf.shape != (self.size(tgt), dim):
            raise ValueError("descriptors must be (n, 33), (n, 125) or (n, 352) float32 tables of one width, one row per point of the slot")
        p = PrerejParams(int(max_iterations), int(nr_samples), int(k), float(similarity), float(max_dist), float(inlier_fraction),
                         int(seed), int(bool(fma)))
        g = to_cm(guess, np.float32) if guess is not None else None
        res = PrerejResult()
        tr = (PrerejTrace * max(int(max_iterations), 1))() if return_trace else None
        _chk(_lib.mvr_align_prerejective_dim(self._h, int(src), int(tgt), _p(sf, C.c_float), _p(tf, C.c_float), dim, C.byref(p),
                                             _p(g, C.c_float) if g is not None else None, C.byref(res), tr), self._h)
        out = dict(converged=bool(res.converged), best_iteration=res.best_iteration, inliers=int(res.inliers), error=res.error,
                   rejected=int(res.rejected), scored=int(res.scored), T=from_cm(np.array(res.T, np.float32)))
        if not return_trace:
            return out
        dt = np.dtype([("status", np.int32), ("src", np.uint32, PREREJ_MAX_SAMPLES), ("tgt", np.uint32, PREREJ_MAX_SAMPLES),
                       ("inliers", np.uint32), ("error", np.float64), ("T", np.float32, 16)], align=True)
        assert dt.itemsize == C.sizeof(PrerejTrace)
        a = np.frombuffer(tr, dtype=dt, count=max(int(max_iterations), 0)).copy()
        trace = {k: np.ascontiguousarray(v) for k, v in dict(
            status=a["status"], src=a["src"][:, :nr_samples], tgt=a["tgt"][:, :nr_samples], inliers=a["inliers"], error=a["error"],
            T=a["T"].reshape(-1, 4, 4).transpose(0, 2, 1)).items()}
        return out, trace

    # ---- target sharding over ranks (sequential mode): see seq.py
    def set_global_base(self, slot, global_begin):
        _chk(_lib.mvr_cloud_set_global_base(self._h, slot, int(global_begin)), self._h)

    def append_range(self, dst, src, src_begin, count, global_begin):
        _chk(_lib.mvr_cloud_append_range(self._h, dst, src, int(src_begin), int(count), int(global_begin)), self._h)

    def nn_forward_keys(self, s, t, max_dist, dev_ptr, fma=False):
        """forward NN of slot s in the (shard) slot t -> Ns signed 64-bit keys with GLOBAL target indices at dev_ptr"""
        _chk(_lib.mvr_nn_forward_keys(self._h, s, t, float(max_dist), int(fma), _vp(dev_ptr)), self._h)

    def pair_moments2_from_keys(self, s, t, keys_dev_ptr, max_dist, origin, out_dev_ptr, reciprocal=True, fma=False):
        o = np.ascontiguousarray(origin, np.float64)
        _chk(_lib.mvr_pair_moments2_from_keys(self._h, s, t, _vp(keys_dev_ptr), float(max_dist), int(reciprocal), int(fma),
                                              _p(o, C.c_double), _vp(out_dev_ptr)), self._h)

    def correspondences(self, s, t, max_dist, reciprocal=True, fma=False):
        n = self.size(s)
        q, m, d = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        cnt = _sz()
        _chk(_lib.mvr_correspondences(self._h, s, t, float(max_dist), int(reciprocal), int(fma),
                                      _p(q, C.c_int32), _p(m, C.c_int32), _p(d, C.c_float), n,
                                      C.byref(cnt)), self._h)
        k = cnt.value
        return q[:k].copy(), m[:k].copy(), d[:k].copy()

    def correspondences_rejected(self, s, t, max_dist, chain, reciprocal=True, fma=False):
        """mvr_correspondences_rejected: the correspondences of slots s -> t that the rejector chain (a list of rejector(...))
        leaves -> (query, match, d2, stages), stages = one dict(n_in, n_out, threshold) per stage."""
        n = self.size(s)
        q, m, d = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        arr, nc = _chain(chain)
        st, cnt = (RejectorStage * MAX_REJECTORS)(), _sz()
        _chk(_lib.mvr_correspondences_rejected(self._h, s, t, float(max_dist), int(reciprocal), int(fma), arr, nc, _p(q, C.c_int32),
                                               _p(m, C.c_int32), _p(d, C.c_float), n, C.byref(cnt), st), self._h)
        k = cnt.value
        return q[:k].copy(), m[:k].copy(), d[:k].copy(), _stage_dicts(st, nc)

    def reject_correspondences(self, s, t, query, match, dist2, chain):
        """mvr_reject_correspondences: the chain on the caller's list -> (query, match, d2, stages), ascending query index."""
        qi, mi = np.ascontiguousarray(query, np.int32), np.ascontiguousarray(match, np.int32)
        di = np.ascontiguousarray(dist2, np.float32)
        n = len(qi)
        q, m, d = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        arr, nc = _chain(chain)
        st, cnt = (RejectorStage * MAX_REJECTORS)(), _sz()
        _chk(_lib.mvr_reject_correspondences(self._h, s, t, _p(qi, C.c_int32), _p(mi, C.c_int32), _p(di, C.c_float), n, arr, nc,
                                             _p(q, C.c_int32), _p(m, C.c_int32), _p(d, C.c_float), n, C.byref(cnt), st), self._h)
        k = cnt.value
        return q[:k].copy(), m[:k].copy(), d[:k].copy(), _stage_dicts(st, nc)

    def reject_sample_consensus(self, s, t, query, match, dist2, rejector, return_trace=False):
        """mvr_reject_sample_consensus (rules C1-C12): pcl::registration::CorrespondenceRejectorSampleConsensus on the caller's
        list, the points taken from slots s and t -> (query, match, d2, result[, trace]).  result: dict(found, live, valid,
        inliers, ransac_inliers, iterations, attempts, skipped, best_attempt, refine_rounds, k, T, ransac_T ((4,4) float32));
        trace: dict(status[t], query[t, 3], match[t, 3], T[t, 16] (column-major), inliers[t], k[t]) over the attempts made."""
        qi, mi = np.ascontiguousarray(query, np.int32), np.ascontiguousarray(match, np.int32)
        di = np.ascontiguousarray(dist2, np.float32)
        n = len(qi)
        q, m, d = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        res, cnt = RejSacResult(), _sz()
        mi_ = int(rejector.max_iterations) or 1000
        cap = 11 * mi_ + 1 if return_trace else 0      # counted attempts <= max_iterations + 1, skipped <= 10 x
        dt = np.dtype([("status", np.int32), ("query", np.uint32, 3), ("match", np.uint32, 3), ("T", np.float32, 16),
                       ("inliers", np.uint32), ("k", np.float64)], align=True)
        assert dt.itemsize == C.sizeof(RejSacTrace)
        tr = np.zeros(max(cap, 1), dt)
        _chk(_lib.mvr_reject_sample_consensus(self._h, s, t, _p(qi, C.c_int32), _p(mi, C.c_int32), _p(di, C.c_float), n,
                                              C.byref(rejector), C.byref(res), _p(q, C.c_int32), _p(m, C.c_int32), _p(d, C.c_float),
                                              n, C.byref(cnt), C.cast(tr.ctypes.data, C.POINTER(RejSacTrace)) if return_trace else None,
                                              cap), self._h)
        k = cnt.value
        out = (q[:k].copy(), m[:k].copy(), d[:k].copy(), _rej_sac_dict(res))
        if return_trace:
            a = tr[:res.attempts]
            out += ({key: np.ascontiguousarray(a[key]) for key in ("status", "query", "match", "T", "inliers", "k")},)
        return out

    def last_sample_consensus(self) -> dict:
        """mvr_ctx_last_sample_consensus: the result of the last sample-consensus stage that ran on this context (inside a chain
        of any entry) -- what getBestTransformation() reads after an align."""
        res = RejSacResult()
        _chk(_lib.mvr_ctx_last_sample_consensus(self._h, C.byref(res)), self._h)
        return _rej_sac_dict(res)

    def icp_align_rejected(self, src, tgt, out, params: IcpParams, chain, return_trace=False):
        """mvr_icp_align_rejected -> (T (4,4) float32, stats dict, rc[, trace]); rc is OK or E_NOCORR.  trace: one dict per iteration
        (n_found, stages, n_corr, mse, tr (4,4) float32: the incremental transformation)."""
        T, st = np.empty(16, np.float32), IcpStats()
        arr, nc = _chain(chain)
        cap = max(1, int(params.max_iterations)) if return_trace else 0
        tr = (IcpIterTrace * max(1, cap))()
        rc = _chk(_lib.mvr_icp_align_rejected(self._h, src, tgt, out, C.byref(params), arr, nc, _p(T, C.c_float), C.byref(st),
                                              tr if return_trace else None, cap), self._h, allow=(E_NOCORR,))
        stats = self._stats(st)
        if not return_trace:
            return from_cm(T), stats, rc
        n_it = min(cap, stats["iterations"] + (1 if rc == E_NOCORR else 0))
        trace = [dict(n_found=tr[k].n_found, stages=_stage_dicts(tr[k].stages, nc), n_corr=tr[k].n_corr, mse=tr[k].mse,
                      tr=from_cm(np.array(tr[k].tr, np.float32))) for k in range(n_it)]
        return from_cm(T), stats, rc, trace

    def icp_align_gicp(self, src, tgt, out, params: GicpParams, chain=(), return_trace=False):
        """mvr_icp_align_gicp -> (T (4,4) float32, stats dict, rc[, trace]); rc is OK, E_NOCORR or E_SINGULAR.  trace: one dict per
        outer iteration (n_found, stages, n_corr, mse, f0, f1, inner_evals, inner_accepted, lambda, tr (4,4) float32)."""
        T, st = np.empty(16, np.float32), IcpStats()
        arr, nc = _chain(chain)
        cap = max(1, int(params.max_iterations)) if return_trace else 0
        tr = (GicpIterTrace * max(1, cap))()
        rc = _chk(_lib.mvr_icp_align_gicp(self._h, src, tgt, out, C.byref(params), arr, nc, _p(T, C.c_float), C.byref(st),
                                          tr if return_trace else None, cap), self._h, allow=(E_NOCORR, E_SINGULAR))
        stats = self._stats(st)
        if not return_trace:
            return from_cm(T), stats, rc
        n_it = min(cap, stats["iterations"] + (1 if rc != OK else 0))
        trace = [{"n_found": tr[k].n_found, "stages": _stage_dicts(tr[k].stages, nc), "n_corr": tr[k].n_corr, "mse": tr[k].mse,
                  "f0": tr[k].f0, "f1": tr[k].f1, "inner_evals": tr[k].inner_evals, "inner_accepted": tr[k].inner_accepted,
                  "lambda": tr[k].lambda_, "tr": from_cm(np.array(tr[k].tr, np.float32))} for k in range(n_it)]
        return from_cm(T), stats, rc, trace

    def gicp_sums(self, s, t, query, match, X=None, gicp_epsilon=1e-3):
        """mvr_gicp_sums: the 29 sums of rule G5 at X ((4,4) float64, identity by default) over the caller's list -> float64[29]"""
        qi, mi = np.ascontiguousarray(query, np.int32), np.ascontiguousarray(match, np.int32)
        Xc = to_cm(np.eye(4) if X is None else X, np.float64)
        out = np.empty(29, np.float64)
        _chk(_lib.mvr_gicp_sums(self._h, s, t, _p(qi, C.c_int32), _p(mi, C.c_int32), len(qi), _p(Xc, C.c_double), float(gicp_epsilon),
                                _p(out, C.c_double)), self._h)
        return out

    def gicp_solve(self, s, t, query, match, params: GicpParams):
        """mvr_gicp_solve: the inner optimisation (rules G5-G7) over the caller's list -> (X (4,4) float64, info dict(evaluations,
        accepted, lambda, f0, f1), rc); rc is OK, E_NOCORR or E_SINGULAR."""
        qi, mi = np.ascontiguousarray(query, np.int32), np.ascontiguousarray(match, np.int32)
        X, info = np.empty(16, np.float64), GicpInfo()
        rc = _chk(_lib.mvr_gicp_solve(self._h, s, t, _p(qi, C.c_int32), _p(mi, C.c_int32), len(qi), C.byref(params), _p(X, C.c_double),
                                      C.byref(info)), self._h, allow=(E_NOCORR, E_SINGULAR))
        return from_cm(X), {"evaluations": info.evaluations, "accepted": info.accepted, "lambda": info.lambda_, "f0": info.f0,
                            "f1": info.f1}, rc

    def ndt_cells(self, tgt, params: NdtParams):
        """mvr_ndt_cells: the kept cells of rule N3 in ascending voxel index -> dict(key uint64[n], count uint32[n],
        mean float64[n, 3], icov float64[n, 6] (xx xy xz yy yz zz))"""
        n = _sz()
        _chk(_lib.mvr_ndt_cells(self._h, tgt, C.byref(params), 0, None, None, None, None, C.byref(n)), self._h)
        m = n.value
        key, cnt = np.empty(max(m, 1), np.uint64), np.empty(max(m, 1), np.uint32)
        mean, icov = np.empty((max(m, 1), 3), np.float64), np.empty((max(m, 1), 6), np.float64)
        _chk(_lib.mvr_ndt_cells(self._h, tgt, C.byref(params), m, _p(key, C.c_uint64), _p(cnt, C.c_uint32), _p(mean, C.c_double),
                                _p(icov, C.c_double), C.byref(n)), self._h)
        assert n.value == m
        return dict(key=key[:m], count=cnt[:m], mean=mean[:m], icov=icov[:m])

    def ndt_sums(self, src, tgt, params: NdtParams, p=None, guess=None):
        """mvr_ndt_sums: the 29 sums of rule N6 at the pose p (6 values, zero by default) on top of the guess ((4,4) float64,
        identity by default) -> float64[29]"""
        x = np.ascontiguousarray(np.zeros(6) if p is None else p, np.float64)
        assert x.shape == (6,)
        G = None if guess is None else to_cm(guess, np.float64)
        out = np.empty(29, np.float64)
        _chk(_lib.mvr_ndt_sums(self._h, src, tgt, C.byref(params), None if G is None else _p(G, C.c_double), _p(x, C.c_double),
                               _p(out, C.c_double)), self._h)
        return out

    def ndt_align(self, src, tgt, out, params: NdtParams, guess=None, return_trace=False, trace_cap=None):
        """mvr_ndt_align -> (T (4,4) float32, X (4,4) float64, stats dict, rc[, trace]); rc is OK or E_NOCORR (no overlap at the
        start).  trace: one dict per iteration (a, delta_norm, trials, reversed, fallback, stop, score, count, p float64[6]),
        the first trace_cap of them (default: all)."""
        T, X, st = np.empty(16, np.float32), np.empty(16, np.float64), NdtStats()
        G = None if guess is None else to_cm(guess, np.float64)
        cap = (max(1, int(params.max_iterations)) + 1 if trace_cap is None else int(trace_cap)) if return_trace else 0
        tr = (NdtIterTrace * max(1, cap))()
        rc = _chk(_lib.mvr_ndt_align(self._h, src, tgt, out, C.byref(params), None if G is None else _p(G, C.c_double), _p(T, C.c_float),
                                     _p(X, C.c_double), C.byref(st), tr if return_trace else None, cap), self._h, allow=(E_NOCORR,))
        stats = dict(iterations=st.iterations, stop=NDT_STOPS[st.stop], converged=bool(st.converged), evaluations=st.evaluations,
                     n_cells=st.n_cells, n_pairs=st.n_pairs, score=st.score, ms=st.ms)
        if not return_trace:
            return from_cm(T), from_cm(X), stats, rc
        # (an iteration that stopped without a step -- FLAT, NO_DECREASE -- leaves a record too)
        n_it = st.iterations + (1 if st.stop in (3, 4) else 0)
        return from_cm(T), from_cm(X), stats, rc, _ndt_trace(tr, min(cap, n_it))

    def pair_batch_correspondences(self, k, cap):
        """(query, match, d2) of pair k of the last fused batch / ring step (mvr_pair_batch_correspondences)"""
        q, m, d = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.float32)
        cnt = _sz()
        _chk(_lib.mvr_pair_batch_correspondences(self._h, int(k), _p(q, C.c_int32), _p(m, C.c_int32), _p(d, C.c_float), cap, C.byref(cnt)), self._h)
        n = min(cnt.value, cap)
        return q[:n].copy(), m[:n].copy(), d[:n].copy()

    def pair_moments(self, s, t, max_dist, reciprocal=True, fma=False) -> PairMoments:
        out = PairMoments()
        _chk(_lib.mvr_pair_moments(self._h, s, t, float(max_dist), int(reciprocal), int(fma),
                                   C.byref(out)), self._h)
        return out

    def pair_moments2(self, s, t, max_dist, origin, reciprocal=True, fma=False, q_begin=0,
                      q_count=None) -> PairMoments2:
        out = PairMoments2()
        o = np.ascontiguousarray(origin, np.float64)
        qc = (1 << 62) if q_count is None else int(q_count)
        _chk(_lib.mvr_pair_moments2(self._h, s, t, float(max_dist), int(reciprocal), int(fma),
                                    int(q_begin), qc, _p(o, C.c_double), C.byref(out)), self._h)
        return out

    def pair_moments2_dev(self, s, t, max_dist, origin, dev_ptr, reciprocal=True, fma=False,
                          q_begin=0, q_count=None):
        o = np.ascontiguousarray(origin, np.float64)
        qc = (1 << 62) if q_count is None else int(q_count)
        _chk(_lib.mvr_pair_moments2_dev(self._h, s, t, float(max_dist), int(reciprocal), int(fma),
                                        int(q_begin), qc, _p(o, C.c_double), _vp(dev_ptr)), self._h)

    def transform_batch(self, dst_slots, src_slots, poses):
        """slot dst[k] = pose[k] applied to slot src[k] (mvr_cloud_transform semantics), all clouds in one launch."""
        n = len(dst_slots)
        d = (C.c_int * n)(*[int(v) for v in dst_slots])
        s = (C.c_int * n)(*[int(v) for v in src_slots])
        # (4,4) column-vector matrices -> column-major 16-vectors: one transpose for all clouds
        T = (np.ascontiguousarray(np.asarray(poses, np.float64).reshape(n, 4, 4).transpose(0, 2, 1)).reshape(n, 16) if n
             else np.zeros((0, 16)))
        _chk(_lib.mvr_cloud_transform_batch(self._h, n, d, s, _p(T, C.c_double)), self._h)

    def ring_step(self, posed_slots, raw_slots, edges, poses, max_dist, origin, lum_iterations=16, reciprocal=True, fma=False,
                  steps=None, _entry=None):
        """mvr_ring_step: one outer pass of registrationLUM in one native call (single process).  edges: [(src view,
        tgt view)]; poses: list of (4,4) float64.  Returns (new poses, info) like ring_host_step, plus info["rows"]
        (ne x 32 edge table) and info["timing_ms"] = (enqueue, GPU wait + copy, host solve).  poses may be a list of
        (4,4) arrays or one (V,4,4) array; the new poses come back as a (V,4,4) array.  steps=K: K passes in one
        native call (mvr_ring_run)."""
        V, ne = len(posed_slots), len(edges)
        key = (tuple(posed_slots), tuple(raw_slots), tuple(edges))
        st = getattr(self, "_ring_static", None)
        if st is None or st[0] != key:                      # the slot / edge arrays of a registration never change
            st = (key, (C.c_int * V)(*[int(v) for v in posed_slots]), (C.c_int * V)(*[int(v) for v in raw_slots]),
                  (C.c_int * ne)(*[int(e[0]) for e in edges]), (C.c_int * ne)(*[int(e[1]) for e in edges]))
            self._ring_static = st
        _, ps, rs, es, et = st
        # (4,4) column-vector matrices <-> the library's column-major 16-vectors: one transpose for all views
        P = np.ascontiguousarray(np.asarray(poses, np.float64).transpose(0, 2, 1)).reshape(V, 16)
        o = np.ascontiguousarray(origin, np.float64)
        lum, rows, tm = np.zeros((V, 6)), np.empty((ne, 32)), np.zeros(3)
        pT, pn, pm, its = np.empty((ne, 16), np.float32), np.empty(ne), np.empty(ne), C.c_int()
        args = (V, ps, rs, ne, es, et, float(max_dist), int(reciprocal), int(fma), _p(o, C.c_double), int(lum_iterations),
                _p(P, C.c_double), _p(lum, C.c_double), _p(pT, C.c_float), _p(pn, C.c_double), _p(pm, C.c_double), C.byref(its),
                _p(rows, C.c_double), _p(tm, C.c_double))
        if steps is None:
            _chk(_lib.mvr_ring_step(self._h, *args), self._h)
        else:                     # mvr_ring_run: `steps` passes in one call; outputs of the last one, timing summed
            _chk((_entry or _lib.mvr_ring_run)(self._h, int(steps), *args), self._h)
        new = np.ascontiguousarray(P.reshape(V, 4, 4).transpose(0, 2, 1))        # (V,4,4): indexable like the list that came in
        info = dict(pair_T=np.ascontiguousarray(pT.reshape(ne, 4, 4).transpose(0, 2, 1)), pair_n=pn.tolist(),
                    pair_mse=pm.tolist(), lum_pose=lum, lum_iterations=its.value, rows=rows, timing_ms=tuple(tm.tolist()))
        return new, info

    # ---- multi-GPU (mvr_world.cpp): one process per GPU
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """ncclCommInitRank on this context's device (collective: every rank calls it with rank 0's unique id)."""
        assert len(unique_id) == 128
        _torch_before_rccl()
        _chk(_lib.mvr_ctx_comm_init(self._h, unique_id, int(rank), int(world)), self._h)

    def project(self, world, rank=0, peer_rows=None):
        """mvr_ctx_project: ring_run_sharded then runs as `rank` of `world` on this one GPU, the absent peers' rows added behind
        the all-reduce (peer_rows: (ne, 32) float64); world <= 1 switches it off"""
        if world <= 1:
            _chk(_lib.mvr_ctx_project(self._h, 0, 0, None, 0), self._h)
            return
        rows = np.ascontiguousarray(peer_rows, np.float64)
        _chk(_lib.mvr_ctx_project(self._h, int(world), int(rank), _p(rows, C.c_double), rows.shape[0]), self._h)

    def debug_order(self, slot):
        """diagnostics: the ordering of the cloud in `slot` (sorted position -> original index), or None while it has none"""
        n = C.c_size_t()
        _chk(_lib.mvr_debug_order(self._h, int(slot), None, 0, C.byref(n)), self._h)
        if n.value == 0:
            return None
        buf = np.zeros(n.value, np.uint32)
        _chk(_lib.mvr_debug_order(self._h, int(slot), buf.ctypes.data, n.value, C.byref(n)), self._h)
        return buf

    def comm_destroy(self):
        _chk(_lib.mvr_ctx_comm_destroy(self._h), self._h)

    def comm_info(self):
        """(rank, world, ranks RCCL itself reports for the communicator; 0 = no communicator)"""
        r, w, n = C.c_int(), C.c_int(), C.c_int()
        _chk(_lib.mvr_ctx_comm_info(self._h, C.byref(r), C.byref(w), C.byref(n)), self._h)
        return r.value, w.value, n.value

    def ring_run_sharded(self, posed_slots, raw_slots, edges, poses, max_dist, origin, steps=1, lum_iterations=16, reciprocal=True,
                         fma=False):
        """mvr_ring_run_sharded: this rank's share of `steps` outer passes + one RCCL all-reduce of the edge table per
        pass; same arguments and results as ring_step(steps=...) on every rank."""
        return self.ring_step(posed_slots, raw_slots, edges, poses, max_dist, origin, lum_iterations=lum_iterations,
                              reciprocal=reciprocal, fma=fma, steps=steps, _entry=_lib.mvr_ring_run_sharded)

    def ring_rows_sharded(self, rank, world, posed_slots, raw_slots, edges, poses, max_dist, origin, reciprocal=True, fma=False):
        """mvr_ring_rows_sharded: the rows of the edge table that `rank` of `world` contributes to one pass (host, (ne, 32))"""
        V, ne = len(posed_slots), len(edges)
        ps, rs = (C.c_int * V)(*[int(v) for v in posed_slots]), (C.c_int * V)(*[int(v) for v in raw_slots])
        es, et = (C.c_int * ne)(*[int(e[0]) for e in edges]), (C.c_int * ne)(*[int(e[1]) for e in edges])
        P = np.ascontiguousarray(np.asarray(poses, np.float64).transpose(0, 2, 1)).reshape(V, 16)
        o, rows = np.ascontiguousarray(origin, np.float64), np.zeros((ne, 32))
        _chk(_lib.mvr_ring_rows_sharded(self._h, int(rank), int(world), V, ps, rs, ne, es, et, float(max_dist), int(reciprocal), int(fma),
                                        _p(o, C.c_double), _p(P, C.c_double), _p(rows, C.c_double)), self._h)
        return rows

    def pair_moments2_batch(self, pairs, max_dist, origin, dev_ptr=None, reciprocal=True, fma=False, ranges=None):
        """All scan pairs of one global iteration in one call: one launch per stage for all pairs (culled
        search) or one pair per worker stream (brute force).  pairs: [(src, tgt)]; ranges: [(q_begin, q_count)] or None.
        Returns a list of PairMoments2 (host) or, with dev_ptr (device [n][32] float64), None."""
        n = len(pairs)
        src = (C.c_int * n)(*[int(a) for a, _ in pairs])
        dst = (C.c_int * n)(*[int(b) for _, b in pairs])
        qb = qn = None
        if ranges is not None:
            qb = (C.c_size_t * n)(*[int(a) for a, _ in ranges])
            qn = (C.c_size_t * n)(*[(1 << 62) if c is None else int(c) for _, c in ranges])
        o = np.ascontiguousarray(origin, np.float64)
        out = None if dev_ptr else (PairMoments2 * n)()
        _chk(_lib.mvr_pair_moments2_batch(self._h, n, src, dst, float(max_dist), int(reciprocal), int(fma), qb, qn,
                                          _p(o, C.c_double), out, _vp(dev_ptr) if dev_ptr else None), self._h)
        return None if dev_ptr else list(out)

    def pair_moments2_from_corr(self, s, t, query, match, origin) -> PairMoments2:
        q = np.ascontiguousarray(query, np.int32)
        m = np.ascontiguousarray(match, np.int32)
        o = np.ascontiguousarray(origin, np.float64)
        out = PairMoments2()
        _chk(_lib.mvr_pair_moments2_from_corr(self._h, s, t, _p(q, C.c_int32), _p(m, C.c_int32), len(q),
                                              _p(o, C.c_double), C.byref(out)), self._h)
        return out

    def icp_align(self, src, tgt, out, params: IcpParams):
        """Returns (T (4,4) float32, stats dict, rc); rc is OK or E_NOCORR."""
        T, st = np.empty(16, np.float32), IcpStats()
        rc = _chk(_lib.mvr_icp_align(self._h, src, tgt, out, C.byref(params), _p(T, C.c_float),
                                     C.byref(st)), self._h, allow=(E_NOCORR,))
        stats = dict(iterations=st.iterations, converged=bool(st.converged),
                     state=CONV_STATES[st.state], n_corr=st.n_corr, mse=st.mse, evals=st.evals,
                     fwd_queries=st.fwd_queries, ms=st.ms)
        return from_cm(T), stats, rc

    @staticmethod
    def _stats(st):
        return dict(iterations=st.iterations, converged=bool(st.converged), state=CONV_STATES[st.state], n_corr=st.n_corr, mse=st.mse,
                    evals=st.evals, fwd_queries=st.fwd_queries, ms=st.ms)

    def seq_align_sharded(self, src, tgt, out, params: IcpParams, origin):
        """mvr_seq_align_sharded: one align of the full source against this rank's target shard -> (T, stats, rc)"""
        T, st, o = np.empty(16, np.float32), IcpStats(), np.ascontiguousarray(origin, np.float64)
        rc = _chk(_lib.mvr_seq_align_sharded(self._h, src, tgt, out, C.byref(params), _p(o, C.c_double), _p(T, C.c_float), C.byref(st)),
                  self._h, allow=(E_NOCORR,))
        return from_cm(T), self._stats(st), rc

    def seq_run_sharded(self, raw_slots, target_slot, source_slot, out_slot, params: IcpParams, origin, poses, repeat=1):
        """mvr_seq_run_sharded: registrationICP with the growing target sharded over the context's communicator.
        poses: V (4,4) float64 -> (new poses (V,4,4), log: list of dict(view, T, iterations, state, n_corr, mse, ...))"""
        V = len(raw_slots)
        rs = (C.c_int * V)(*[int(v) for v in raw_slots])
        P = np.ascontiguousarray(np.asarray(poses, np.float64).transpose(0, 2, 1)).reshape(V, 16)
        cap = max(1, repeat * (V - 1))
        views, Ts, sts, n = (C.c_int * cap)(), np.zeros((cap, 16), np.float32), (IcpStats * cap)(), C.c_int()
        o = np.ascontiguousarray(origin, np.float64)
        _chk(_lib.mvr_seq_run_sharded(self._h, V, rs, int(target_slot), int(source_slot), int(out_slot), C.byref(params), _p(o, C.c_double),
                                      int(repeat), _p(P, C.c_double), views, _p(Ts, C.c_float), sts, C.byref(n)), self._h)
        log = [dict(self._stats(sts[k]), view=views[k], T=from_cm(Ts[k])) for k in range(n.value)]
        return np.ascontiguousarray(P.reshape(V, 4, 4).transpose(0, 2, 1)), log

    def seq_run(self, raw_slots, target_slot, source_slot, out_slot, params: IcpParams, poses, repeat=1):
        """mvr_seq_run: registrationICP (registrator.cpp:526-588) on one GPU as one native call -- `repeat` sweeps of aligns of
        views 1, V-1, 2, ... against the growing model.  poses: V (4,4) float64 -> (new poses (V,4,4), log as seq_run_sharded)"""
        V = len(raw_slots)
        rs = (C.c_int * V)(*[int(v) for v in raw_slots])
        P = np.ascontiguousarray(np.asarray(poses, np.float64).transpose(0, 2, 1)).reshape(V, 16)
        cap = max(1, repeat * (V - 1))
        views, Ts, sts, n = (C.c_int * cap)(), np.zeros((cap, 16), np.float32), (IcpStats * cap)(), C.c_int()
        _chk(_lib.mvr_seq_run(self._h, V, rs, int(target_slot), int(source_slot), int(out_slot), C.byref(params), int(repeat),
                              _p(P, C.c_double), views, _p(Ts, C.c_float), sts, C.byref(n)), self._h)
        log = [dict(self._stats(sts[k]), view=views[k], T=from_cm(Ts[k])) for k in range(n.value)]
        return np.ascontiguousarray(P.reshape(V, 4, 4).transpose(0, 2, 1)), log

    def fitness(self, inp, tgt, T, max_range=np.finfo(np.float64).max, fma=False) -> float:
        t, s = to_cm(T, np.float32), C.c_double()
        _chk(_lib.mvr_fitness(self._h, inp, tgt, _p(t, C.c_float), float(max_range), int(fma),
                              C.byref(s)), self._h)
        return s.value

    # -- misc
    def sync(self):
        _chk(_lib.mvr_ctx_sync(self._h), self._h)

    def device_info(self):
        name = C.create_string_buffer(64)
        ncu, mhz = C.c_int(), C.c_int()
        _chk(_lib.mvr_device_info(self._h, name, 64, C.byref(ncu), C.byref(mhz)), self._h)
        return name.value.decode(), ncu.value, mhz.value

    def tune(self, **kw):
        """NN launch knobs (nn_q, nn_sub, nn_blocks_per_cu); results do not depend on them."""
        for k, v in kw.items():
            _chk(_lib.mvr_ctx_tune(self._h, k.encode(), int(v)), self._h)

    def stat(self, key) -> float:
        """mvr_ctx_stat: "piped_passes", "fused_passes", "blocking_events", "pipeline" """
        v = C.c_double()
        _chk(_lib.mvr_ctx_stat(self._h, key.encode(), C.byref(v)), self._h)
        return v.value

    def pass_log(self):
        """wall ms of every pass of the last ring run (mvr_ctx_pass_log)"""
        n = C.c_int()
        _chk(_lib.mvr_ctx_pass_log(self._h, None, 0, C.byref(n)), self._h)
        ms = np.zeros(max(n.value, 1))
        _chk(_lib.mvr_ctx_pass_log(self._h, _p(ms, C.c_double), n.value, C.byref(n)), self._h)
        return ms[: n.value].tolist()

    def debug_counters(self, reset=False):
        out = (C.c_uint64 * 4)()
        _chk(_lib.mvr_debug_counters(self._h, out, int(reset)), self._h)
        return list(out)

    def prof_enable(self, on=True):
        _chk(_lib.mvr_prof_enable(self._h, int(on)), self._h)

    def prof_reset(self):
        _chk(_lib.mvr_prof_reset(self._h), self._h)

    def prof_get(self, family):
        n, ms, w = C.c_uint64(), C.c_double(), C.c_double()
        _chk(_lib.mvr_prof_get(self._h, family, C.byref(n), C.byref(ms), C.byref(w)), self._h)
        return n.value, ms.value, w.value


# ------------------------------------------------------------------ multi-GPU

def _torch_before_rccl():
    """The library's collectives run on PyTorch-ROCm's copy of RCCL when this process can import torch (MVR_RCCL_LIB above).  A
    process that initialises that RCCL through the library and imports torch only AFTERWARDS aborts when it exits ("double free or
    corruption": the two libraries' exit handlers then run in the wrong order -- DESIGN.md section 10); imported first, never.  So the
    first multi-GPU entry point imports it, if it is there and this RCCL is the one in use."""
    if "torch" in sys.modules or "torch" not in os.environ.get("MVR_RCCL_LIB", ""):
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def comm_unique_id() -> bytes:
    """ncclGetUniqueId (rank 0); hand the 128 bytes to the other ranks by the launcher's means."""
    _torch_before_rccl()
    buf = C.create_string_buffer(128)
    _chk(_lib.mvr_comm_unique_id(buf))
    return buf.raw


def rccl_library() -> str:
    return _lib.mvr_rccl_library().decode()


def pool_trim():
    """give the idle blocks of the library's allocation cache back to the runtime (mvr_pool_trim); returns
    dict(freed_bytes, cached_bytes, hits, misses)"""
    st = (C.c_uint64 * 3)()
    freed = _lib.mvr_pool_trim(st)
    return dict(freed_bytes=int(freed), cached_bytes=int(st[0]), hits=int(st[1]), misses=int(st[2]))


def ring_segments(edge_queries, world, rank):
    """the sharding of the ring pass: [(edge, first query, count)] of `rank` (mvr_ring_segments)"""
    ne = len(edge_queries)
    q = (C.c_size_t * max(ne, 1))(*[int(v) for v in edge_queries])
    se, sb, sc, n = (C.c_int * max(ne, 1))(), (C.c_size_t * max(ne, 1))(), (C.c_size_t * max(ne, 1))(), C.c_int()
    _chk(_lib.mvr_ring_segments(ne, q, int(world), int(rank), se, sb, sc, C.byref(n)))
    return [(se[k], sb[k], sc[k]) for k in range(n.value)]


class _BorrowedContext(Context):
    """a rank's context of a World: owned by the world, never destroyed from here"""

    def __init__(self, handle):
        self._h = handle

    def close(self):
        self._h = None


class World:
    """One process, n GPUs (mvr_world_create: one context per device + ncclCommInitAll)."""

    def __init__(self, n_dev, device_ids=None):
        h = _vp()
        ids = (C.c_int * n_dev)(*device_ids) if device_ids is not None else None
        _torch_before_rccl()
        rc = _lib.mvr_world_create(C.byref(h), int(n_dev), ids)
        if rc != OK:
            raise MvrError(rc, "mvr_world_create(%d): %s" % (n_dev, rccl_library()))
        self._h, self.n = h, n_dev

    def ctx(self, rank) -> Context:
        return _BorrowedContext(_vp(_lib.mvr_world_ctx(self._h, int(rank))))

    def upload(self, slot, pts):
        pts = np.ascontiguousarray(pts, np.float32)
        rc = _lib.mvr_world_upload(self._h, int(slot), _p(pts, C.c_float), len(pts), 4 * pts.shape[1])
        if rc != OK:
            raise MvrError(rc, _lib.mvr_world_last_error(self._h).decode())

    def ring_run(self, posed_slots, raw_slots, edges, poses, max_dist, origin, steps=1, lum_iterations=16, reciprocal=True, fma=False):
        V, ne = len(posed_slots), len(edges)
        ps, rs = (C.c_int * V)(*[int(v) for v in posed_slots]), (C.c_int * V)(*[int(v) for v in raw_slots])
        es, et = (C.c_int * ne)(*[int(e[0]) for e in edges]), (C.c_int * ne)(*[int(e[1]) for e in edges])
        P = np.ascontiguousarray(np.asarray(poses, np.float64).transpose(0, 2, 1)).reshape(V, 16)
        o = np.ascontiguousarray(origin, np.float64)
        lum, rows, tm = np.zeros((V, 6)), np.empty((ne, 32)), np.zeros(3)
        pT, pn, pm, its = np.empty((ne, 16), np.float32), np.empty(ne), np.empty(ne), C.c_int()
        rc = _lib.mvr_world_ring_run(self._h, int(steps), V, ps, rs, ne, es, et, float(max_dist), int(reciprocal), int(fma),
                                     _p(o, C.c_double), int(lum_iterations), _p(P, C.c_double), _p(lum, C.c_double), _p(pT, C.c_float),
                                     _p(pn, C.c_double), _p(pm, C.c_double), C.byref(its), _p(rows, C.c_double), _p(tm, C.c_double))
        if rc != OK:
            raise MvrError(rc, _lib.mvr_world_last_error(self._h).decode())
        new = np.ascontiguousarray(P.reshape(V, 4, 4).transpose(0, 2, 1))
        return new, dict(pair_T=np.ascontiguousarray(pT.reshape(ne, 4, 4).transpose(0, 2, 1)), pair_n=pn.tolist(), pair_mse=pm.tolist(),
                         lum_pose=lum, lum_iterations=its.value, rows=rows, timing_ms=tuple(tm.tolist()))

    def close(self):
        if self._h:
            _lib.mvr_world_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
