"""ctypes binding of liborbhip.so (include/orbhip.h). Fails loudly when the library is absent."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "liborbhip.so"
_lib = None


class OrbHipError(RuntimeError):
    CODES = {-1: "ORBHIP_ERR_ARG", -2: "ORBHIP_ERR_CAPACITY", -3: "ORBHIP_ERR_DEVICE", -4: "ORBHIP_ERR_NOT_PD",
             -5: "ORBHIP_ERR_UNSUPPORTED", -6: "ORBHIP_ERR_EMPTY", -7: "ORBHIP_ERR_TIMEOUT"}

    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__(f"{what}: {self.CODES.get(code, code)}")


def library_path() -> str:
    # ORBHIP_LIB: an A/B build of the same library (tools/build_ab.sh); default the in-tree build
    return os.environ.get("ORBHIP_LIB") or os.path.join(_HERE, _LIB_NAME)


class KP(ctypes.Structure):
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("size", ctypes.c_float), ("angle", ctypes.c_float),
                ("response", ctypes.c_float), ("octave", ctypes.c_int32)]


KP_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32),
                     ("response", np.float32), ("octave", np.int32)])


class OrbParams(ctypes.Structure):
    _fields_ = [("n_features", ctypes.c_int32), ("scale_factor", ctypes.c_float), ("n_levels", ctypes.c_int32),
                ("ini_th_fast", ctypes.c_int32), ("min_th_fast", ctypes.c_int32)]


class StereoParams(ctypes.Structure):
    _fields_ = [("bf", ctypes.c_float), ("b", ctypes.c_float), ("center_patch", ctypes.c_int32)]


class BAProblemC(ctypes.Structure):
    _fields_ = [("n_poses", ctypes.c_int32), ("n_points", ctypes.c_int32), ("n_edges", ctypes.c_int32),
                ("pose_q", ctypes.c_void_p), ("pose_t", ctypes.c_void_p), ("pose_fixed", ctypes.c_void_p),
                ("points", ctypes.c_void_p), ("edge_pose", ctypes.c_void_p), ("edge_point", ctypes.c_void_p),
                ("edge_uv", ctypes.c_void_p), ("edge_octave", ctypes.c_void_p), ("inv_sigma2", ctypes.c_void_p),
                ("n_octaves", ctypes.c_int32), ("fx", ctypes.c_float), ("fy", ctypes.c_float),
                ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("huber_delta", ctypes.c_float),
                ("iterations", ctypes.c_int32), ("early_stop", ctypes.c_int32)]


class BAStereoProblemC(ctypes.Structure):
    _fields_ = [("mono", BAProblemC), ("edge_ur", ctypes.c_void_p), ("bf", ctypes.c_float),
                ("huber_delta_stereo", ctypes.c_float)]


class BAResultC(ctypes.Structure):
    _fields_ = [("pose_q", ctypes.c_void_p), ("pose_t", ctypes.c_void_p), ("points", ctypes.c_void_p),
                ("edge_chi2", ctypes.c_void_p), ("edge_depth_ok", ctypes.c_void_p),
                ("initial_chi2", ctypes.c_double), ("final_chi2", ctypes.c_double),
                ("iterations_done", ctypes.c_int32), ("lm_trials", ctypes.c_int32)]


class PoseProblemC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("pose_q", ctypes.c_void_p), ("pose_t", ctypes.c_void_p),
                ("points", ctypes.c_void_p), ("uv", ctypes.c_void_p), ("octave", ctypes.c_void_p),
                ("inv_sigma2", ctypes.c_void_p), ("n_octaves", ctypes.c_int32), ("fx", ctypes.c_float),
                ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float)]


class PoseStereoProblemC(ctypes.Structure):
    _fields_ = PoseProblemC._fields_ + [("u_right", ctypes.c_void_p), ("bf", ctypes.c_float)]


class PoseResultC(ctypes.Structure):
    _fields_ = [("pose_q", ctypes.c_float * 4), ("pose_t", ctypes.c_float * 3), ("outlier", ctypes.c_void_p),
                ("n_inliers", ctypes.c_int32), ("lm_trials", ctypes.c_int32)]


class PinholeC(ctypes.Structure):
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("k1", ctypes.c_float), ("k2", ctypes.c_float), ("p1", ctypes.c_float), ("p2", ctypes.c_float),
                ("k3", ctypes.c_float)]


class FrameC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("kps", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("claimed", ctypes.c_void_p),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float), ("max_y", ctypes.c_float),
                ("scale_factors", ctypes.c_void_p), ("n_levels", ctypes.c_int32), ("log_scale_factor", ctypes.c_float),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("pose_q", ctypes.c_float * 4), ("pose_t", ctypes.c_float * 3)]


class StereoViewC(ctypes.Structure):
    _fields_ = [("frame", FrameC), ("u_right", ctypes.c_void_p), ("bf", ctypes.c_float), ("b", ctypes.c_float)]


class ProjLastC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("points", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("octave", ctypes.c_void_p), ("angle", ctypes.c_void_p)]


class InitFrameC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("kps", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("min_x", ctypes.c_float),
                ("max_x", ctypes.c_float), ("min_y", ctypes.c_float), ("max_y", ctypes.c_float)]


class TriKeyFrameC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("kps", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("node", ctypes.c_void_p),
                ("weight", ctypes.c_void_p), ("has_mp", ctypes.c_void_p), ("fx", ctypes.c_float),
                ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("pose_q", ctypes.c_float * 4), ("pose_t", ctypes.c_float * 3)]


class TriStereoKeyFrameC(ctypes.Structure):
    _fields_ = [("kf", TriKeyFrameC), ("u_right", ctypes.c_void_p), ("depth", ctypes.c_void_p),
                ("bf", ctypes.c_float), ("b", ctypes.c_float)]


class TriParamsC(ctypes.Structure):
    _fields_ = [("cos_parallax_max", ctypes.c_double), ("ratio_factor", ctypes.c_float),
                ("far_threshold", ctypes.c_float)]


class NewPointsC(ctypes.Structure):
    _fields_ = [("match12", ctypes.c_void_p), ("nmatches", ctypes.c_void_p), ("gated", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("x3d_all", ctypes.c_void_p), ("first", ctypes.c_void_p),
                ("nnew", ctypes.c_void_p), ("new_nbr", ctypes.c_void_p), ("new_idx1", ctypes.c_void_p),
                ("new_idx2", ctypes.c_void_p), ("new_x3d", ctypes.c_void_p)]


class KfdbQueryC(ctypes.Structure):
    _fields_ = [("query_id", ctypes.c_int64), ("words", ctypes.c_void_p), ("values", ctypes.c_void_p),
                ("n", ctypes.c_int32), ("covis", ctypes.c_void_p), ("kf_map", ctypes.c_void_p),
                ("query_map", ctypes.c_int32), ("kf_flags", ctypes.c_void_p)]


class LocalPointsC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("points", ctypes.c_void_p), ("normals", ctypes.c_void_p),
                ("min_dist", ctypes.c_void_p), ("max_dist", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("skip", ctypes.c_void_p)]


class Sim3ProblemC(ctypes.Structure):
    _fields_ = [("cam1", ctypes.c_float * 4), ("cam2", ctypes.c_float * 4), ("n", ctypes.c_int32),
                ("X1", ctypes.c_void_p), ("X2", ctypes.c_void_p), ("max_err1", ctypes.c_void_p),
                ("max_err2", ctypes.c_void_p), ("fix_scale", ctypes.c_int32), ("min_inliers", ctypes.c_int32),
                ("n_hyp", ctypes.c_int32), ("triples", ctypes.c_void_p)]


class Sim3ResultC(ctypes.Structure):
    _fields_ = [("n_inliers", ctypes.c_void_p), ("hyp", ctypes.c_void_p), ("inliers", ctypes.c_void_p),
                ("sel", ctypes.c_float * 13), ("converged", ctypes.c_int32), ("best", ctypes.c_int32)]


class TwoViewProblemC(ctypes.Structure):
    _fields_ = [("n1", ctypes.c_int32), ("n2", ctypes.c_int32), ("kps1", ctypes.c_void_p), ("kps2", ctypes.c_void_p),
                ("matches12", ctypes.c_void_p), ("K", ctypes.c_float * 4), ("sigma", ctypes.c_float),
                ("n_hyp", ctypes.c_int32), ("sets", ctypes.c_void_p)]


class TwoViewResultC(ctypes.Structure):
    _fields_ = [("p3d", ctypes.c_void_p), ("triangulated", ctypes.c_void_p), ("inliers_h", ctypes.c_void_p),
                ("inliers_f", ctypes.c_void_p), ("success", ctypes.c_int32), ("model", ctypes.c_int32),
                ("best_h", ctypes.c_int32), ("best_f", ctypes.c_int32), ("chosen", ctypes.c_int32),
                ("SH", ctypes.c_float), ("SF", ctypes.c_float), ("H21", ctypes.c_float * 9),
                ("F21", ctypes.c_float * 9), ("R21", ctypes.c_float * 9), ("t21", ctypes.c_float * 3),
                ("n_good", ctypes.c_int32 * 8), ("parallax", ctypes.c_float * 8), ("cos_sel", ctypes.c_float * 8)]


class Sim3OptProblemC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("X1c", ctypes.c_void_p), ("X2c", ctypes.c_void_p), ("obs1", ctypes.c_void_p),
                ("obs2", ctypes.c_void_p), ("inv_sigma2_1", ctypes.c_void_p), ("inv_sigma2_2", ctypes.c_void_p),
                ("cam1", ctypes.c_float * 4), ("cam2", ctypes.c_float * 4), ("q", ctypes.c_double * 4),
                ("t", ctypes.c_double * 3), ("s", ctypes.c_double), ("th2", ctypes.c_double),
                ("fix_scale", ctypes.c_int32)]


class Sim3OptResultC(ctypes.Structure):
    _fields_ = [("q", ctypes.c_double * 4), ("t", ctypes.c_double * 3), ("s", ctypes.c_double),
                ("n_in", ctypes.c_int32), ("n_bad", ctypes.c_int32), ("lm_trials", ctypes.c_int32),
                ("keep", ctypes.c_void_p)]


class EssentialGraphProblemC(ctypes.Structure):
    _fields_ = [("n_vertices", ctypes.c_int32), ("S", ctypes.c_void_p), ("fixed", ctypes.c_void_p),
                ("n_edges", ctypes.c_int32), ("edge_ij", ctypes.c_void_p), ("edge_S", ctypes.c_void_p),
                ("fix_scale", ctypes.c_int32), ("iterations", ctypes.c_int32), ("lambda_init", ctypes.c_double),
                ("n_points", ctypes.c_int32), ("points", ctypes.c_void_p), ("point_ref", ctypes.c_void_p)]


class EssentialGraphResultC(ctypes.Structure):
    _fields_ = [("S", ctypes.c_void_p), ("points", ctypes.c_void_p), ("chi2_initial", ctypes.c_double),
                ("chi2_final", ctypes.c_double), ("iterations_run", ctypes.c_int32), ("lm_trials", ctypes.c_int32),
                ("lm_rejected", ctypes.c_int32), ("solver", ctypes.c_int32)]


# every symbol include/orbhip.h declares (tests check the export table against this list)
EXPORTED = ["orbhip_abi_version", "orbhip_create", "orbhip_destroy", "orbhip_level_info", "orbhip_max_keypoints",
            "orbhip_extract", "orbhip_extract_batch_device", "orbhip_extract_stereo", "orbhip_extract_stereo_device",
            "orbhip_descriptor_distance", "orbhip_match_bf",
            "orbhip_match_pairs_device", "orbhip_match_frames_device", "orbhip_profile_stage",
            "orbhip_profile_collect", "orbhip_launch_graphs", "orbhip_ba_solve", "orbhip_ba_solve_batch", "orbhip_ba_stats",
            "orbhip_ba_solve_stereo", "orbhip_ba_solve_stereo_batch", "orbhip_bgr_to_gray_device",
            "orbhip_comm_unique_id", "orbhip_comm_init", "orbhip_ba_solve_sharded", "orbhip_ba_solve_sharded_segments",
            "orbhip_ba_solve_shards_local",
            "orbhip_vocab_create", "orbhip_vocab_load_text", "orbhip_vocab_destroy", "orbhip_vocab_info",
            "orbhip_bow_transform", "orbhip_bow_transform_device", "orbhip_search_bow",
            "orbhip_pose_optimization", "orbhip_pose_optimization_batch", "orbhip_search_by_projection_last",
            "orbhip_search_local_points", "orbhip_search_for_initialization",
            "orbhip_pose_optimization_stereo", "orbhip_pose_optimization_stereo_batch",
            "orbhip_search_by_projection_last_stereo", "orbhip_search_local_points_stereo",
            "orbhip_triangulation_geometry", "orbhip_search_for_triangulation",
            "orbhip_create_new_map_points", "orbhip_triangulate_matches", "orbhip_fuse", "orbhip_fuse_stereo",
            "orbhip_search_for_triangulation_stereo", "orbhip_create_new_map_points_stereo",
            "orbhip_triangulate_matches_stereo",
            "orbhip_fuse_sim3", "orbhip_search_by_projection_sim3",
            "orbhip_sim3_solve", "orbhip_sim3_solve_batch",
            "orbhip_two_view_reconstruct", "orbhip_two_view_reconstruct_batch",
            "orbhip_optimize_sim3", "orbhip_optimize_sim3_batch", "orbhip_optimize_essential_graph",
            "orbhip_kfdb_create", "orbhip_kfdb_destroy", "orbhip_kfdb_add", "orbhip_kfdb_erase",
            "orbhip_kfdb_detect_relocalization", "orbhip_kfdb_detect_nbest",
            "orbhip_frontend_create", "orbhip_frontend_destroy", "orbhip_frontend_push", "orbhip_frontend_view",
            "orbhip_frontend_wait", "orbhip_frontend_context", "orbhip_undistort_keypoints",
            "orbhip_undistort_keypoints_device", "orbhip_image_bounds"]


def lib():
    """Load liborbhip.so (raises if it was not built — there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    # torch-ROCm bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's). Load it first
    # so liborbhip binds to the SAME HIP runtime: device pointers from torch tensors are then
    # valid in our kernels, and torch does not fail to initialise a second runtime.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(path):
        raise OrbHipError(-3, f"{path} missing — run __graft_entry__.build()")
    L = ctypes.CDLL(path)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.orbhip_abi_version.restype = i32
    L.orbhip_create.argtypes = [ctypes.POINTER(vp), i32, ctypes.POINTER(OrbParams)]
    L.orbhip_destroy.argtypes = [vp]
    L.orbhip_level_info.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.orbhip_max_keypoints.argtypes = [vp, i32, i32]
    L.orbhip_extract.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, ctypes.POINTER(i32),
                                 ctypes.POINTER(i32)]
    L.orbhip_extract_batch_device.argtypes = [vp, vp, i32, i32, i32, i32, ctypes.c_int64, i32, i32, vp, vp, i32,
                                              vp, vp, vp]
    sp = ctypes.POINTER(StereoParams)
    L.orbhip_extract_stereo.argtypes = [vp, vp, vp, i32, i32, i32, sp, vp, vp, ctypes.POINTER(i32), vp, vp,
                                        ctypes.POINTER(i32), i32, vp, vp, vp, ctypes.POINTER(i32)]
    L.orbhip_extract_stereo_device.argtypes = [vp, vp, i32, i32, i32, i32, ctypes.c_int64, sp, vp, vp, i32, vp, vp,
                                               vp, vp, vp, vp, vp]
    # the stereo kernels alone on caller-supplied keypoints (tests compare them with the restatement)
    L.orbhip_test_stereo_match.argtypes = [vp, vp, vp, i32, i32, sp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp,
                                           ctypes.POINTER(i32)]
    # k_stereo_median alone on caller-supplied status / SAD arrays
    L.orbhip_test_stereo_median.argtypes = [vp, vp, vp, vp, vp, i32, ctypes.POINTER(i32)]
    L.orbhip_descriptor_distance.argtypes = [vp, vp]
    L.orbhip_match_bf.argtypes = [vp, vp, vp, i32, vp, vp, i32, i32, f32, i32, vp, vp, vp]
    L.orbhip_match_pairs_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, i32, vp, vp, vp, vp, vp]
    L.orbhip_match_frames_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, vp, vp, vp, vp, vp]
    L.orbhip_vocab_create.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, ctypes.POINTER(vp)]
    L.orbhip_vocab_load_text.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp)]
    L.orbhip_vocab_destroy.argtypes = [vp]
    L.orbhip_vocab_info.argtypes = [vp, vp, vp, vp, vp]
    L.orbhip_bow_transform.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    L.orbhip_bow_transform_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.orbhip_search_bow.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, f32, i32, i32, vp]
    L.orbhip_comm_unique_id.argtypes = [vp]
    L.orbhip_comm_init.argtypes = [vp, i32, i32, vp]
    L.orbhip_ba_solve_sharded.argtypes = [vp, ctypes.POINTER(BAProblemC), ctypes.POINTER(BAResultC), vp]
    L.orbhip_ba_solve_sharded_segments.argtypes = [vp, ctypes.POINTER(BAProblemC), i32, ctypes.POINTER(BAResultC), vp]
    L.orbhip_ba_solve_shards_local.argtypes = [vp, ctypes.POINTER(BAProblemC), i32, ctypes.POINTER(BAResultC), vp]
    L.orbhip_bgr_to_gray_device.argtypes = [vp, vp, i32, i32, i32, i32, ctypes.c_int64, vp, i32, ctypes.c_int64, vp]
    L.orbhip_profile_stage.argtypes = [vp, i32]
    L.orbhip_profile_collect.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    L.orbhip_launch_graphs.argtypes = [vp]
    L.orbhip_ba_solve.argtypes = [vp, ctypes.POINTER(BAProblemC), ctypes.POINTER(BAResultC), vp]
    L.orbhip_ba_solve_batch.argtypes = [vp, ctypes.POINTER(BAProblemC), i32, ctypes.POINTER(BAResultC), vp]
    L.orbhip_ba_solve_stereo.argtypes = [vp, ctypes.POINTER(BAStereoProblemC), ctypes.POINTER(BAResultC), vp]
    L.orbhip_ba_solve_stereo_batch.argtypes = [vp, ctypes.POINTER(BAStereoProblemC), i32, ctypes.POINTER(BAResultC),
                                               vp]
    L.orbhip_ba_stats.argtypes = [vp, vp]
    L.orbhip_pose_optimization.argtypes = [vp, ctypes.POINTER(PoseProblemC), ctypes.POINTER(PoseResultC)]
    L.orbhip_pose_optimization_batch.argtypes = [vp, ctypes.POINTER(PoseProblemC), i32, ctypes.POINTER(PoseResultC)]
    L.orbhip_search_by_projection_last.argtypes = [vp, ctypes.POINTER(FrameC), ctypes.POINTER(ProjLastC), f32, i32,
                                                   vp]
    L.orbhip_search_local_points.argtypes = [vp, ctypes.POINTER(FrameC), ctypes.POINTER(LocalPointsC), f32, f32, f32,
                                             i32, f32, vp, vp, vp]
    L.orbhip_pose_optimization_stereo.argtypes = [vp, ctypes.POINTER(PoseStereoProblemC), ctypes.POINTER(PoseResultC)]
    L.orbhip_pose_optimization_stereo_batch.argtypes = [vp, ctypes.POINTER(PoseStereoProblemC), i32,
                                                        ctypes.POINTER(PoseResultC)]
    L.orbhip_search_by_projection_last_stereo.argtypes = [vp, ctypes.POINTER(StereoViewC), ctypes.POINTER(ProjLastC),
                                                          vp, vp, f32, i32, vp, ctypes.POINTER(i32)]
    L.orbhip_search_local_points_stereo.argtypes = [vp, ctypes.POINTER(StereoViewC), ctypes.POINTER(LocalPointsC),
                                                    f32, f32, f32, i32, f32, vp, vp, vp, vp]
    L.orbhip_search_for_initialization.argtypes = [vp, ctypes.POINTER(InitFrameC), ctypes.POINTER(InitFrameC), vp,
                                                   i32, f32, i32, vp]
    L.orbhip_triangulation_geometry.argtypes = [ctypes.POINTER(TriKeyFrameC), ctypes.POINTER(TriKeyFrameC), vp, vp]
    L.orbhip_search_for_triangulation.argtypes = [vp, ctypes.POINTER(TriKeyFrameC), ctypes.POINTER(TriKeyFrameC), i32,
                                                  vp, vp, i32, i32, vp, vp]
    L.orbhip_create_new_map_points.argtypes = [vp, ctypes.POINTER(TriKeyFrameC), ctypes.POINTER(TriKeyFrameC), i32, vp,
                                               vp, vp, i32, i32, ctypes.POINTER(TriParamsC),
                                               ctypes.POINTER(NewPointsC)]
    L.orbhip_triangulate_matches.argtypes = [vp, ctypes.POINTER(TriKeyFrameC), ctypes.POINTER(TriKeyFrameC), i32, vp,
                                             vp, vp, i32, ctypes.POINTER(TriParamsC), ctypes.POINTER(NewPointsC)]
    tsk = ctypes.POINTER(TriStereoKeyFrameC)
    L.orbhip_search_for_triangulation_stereo.argtypes = [vp, tsk, tsk, i32, vp, vp, i32, i32, vp, vp]
    L.orbhip_create_new_map_points_stereo.argtypes = [vp, tsk, tsk, i32, vp, vp, i32, i32, ctypes.POINTER(TriParamsC),
                                                      ctypes.POINTER(NewPointsC), vp]
    L.orbhip_triangulate_matches_stereo.argtypes = [vp, tsk, tsk, i32, vp, vp, vp, i32, ctypes.POINTER(TriParamsC),
                                                    ctypes.POINTER(NewPointsC), vp]
    L.orbhip_fuse.argtypes = [vp, ctypes.POINTER(FrameC), i32, ctypes.POINTER(LocalPointsC), vp, vp, f32, vp, vp, vp,
                              vp]
    L.orbhip_fuse_stereo.argtypes = [vp, ctypes.POINTER(StereoViewC), i32, ctypes.POINTER(LocalPointsC), vp, vp, f32, vp,
                                     vp, vp, vp]
    L.orbhip_fuse_sim3.argtypes = [vp, ctypes.POINTER(FrameC), i32, ctypes.POINTER(LocalPointsC), vp, f32, vp, vp, vp, vp]
    L.orbhip_search_by_projection_sim3.argtypes = [vp, ctypes.POINTER(FrameC), ctypes.POINTER(LocalPointsC), f32, f32,
                                                   vp, vp, vp]
    L.orbhip_sim3_solve.argtypes = [vp, ctypes.POINTER(Sim3ProblemC), ctypes.POINTER(Sim3ResultC)]
    L.orbhip_sim3_solve_batch.argtypes = [vp, ctypes.POINTER(Sim3ProblemC), i32, ctypes.POINTER(Sim3ResultC)]
    L.orbhip_two_view_reconstruct.argtypes = [vp, ctypes.POINTER(TwoViewProblemC), ctypes.POINTER(TwoViewResultC)]
    L.orbhip_two_view_reconstruct_batch.argtypes = [vp, ctypes.POINTER(TwoViewProblemC), i32,
                                                    ctypes.POINTER(TwoViewResultC)]
    L.orbhip_optimize_sim3.argtypes = [vp, ctypes.POINTER(Sim3OptProblemC), ctypes.POINTER(Sim3OptResultC)]
    L.orbhip_optimize_sim3_batch.argtypes = [vp, ctypes.POINTER(Sim3OptProblemC), i32, ctypes.POINTER(Sim3OptResultC)]
    L.orbhip_optimize_essential_graph.argtypes = [vp, ctypes.POINTER(EssentialGraphProblemC),
                                                  ctypes.POINTER(EssentialGraphResultC)]
    L.orbhip_kfdb_create.argtypes = [vp, i32, ctypes.POINTER(vp)]
    L.orbhip_kfdb_destroy.argtypes = [vp]
    L.orbhip_kfdb_add.argtypes = [vp, i32, vp, vp, i32]
    L.orbhip_kfdb_erase.argtypes = [vp, i32]
    L.orbhip_kfdb_detect_relocalization.argtypes = [vp, ctypes.POINTER(KfdbQueryC), vp, i32]
    L.orbhip_kfdb_detect_nbest.argtypes = [vp, ctypes.POINTER(KfdbQueryC), vp, i32, vp, vp, vp, vp]
    L.orbhip_frontend_create.argtypes = [ctypes.POINTER(vp), i32, ctypes.POINTER(OrbParams), i32, i32, i32, i32, f32,
                                         i32]
    L.orbhip_frontend_destroy.argtypes = [vp]
    L.orbhip_frontend_push.argtypes = [vp, vp, i32, i32, i32]
    L.orbhip_frontend_view.argtypes = [vp, i32, vp]
    L.orbhip_frontend_wait.argtypes = [vp, i32, vp]
    L.orbhip_frontend_context.argtypes = [vp, i32, ctypes.POINTER(vp)]
    L.orbhip_undistort_keypoints.argtypes = [vp, ctypes.POINTER(PinholeC), vp, i32, vp]
    L.orbhip_undistort_keypoints_device.argtypes = [vp, ctypes.POINTER(PinholeC), vp, vp, i32, i32, vp, vp]
    L.orbhip_image_bounds.argtypes = [vp, ctypes.POINTER(PinholeC), i32, i32, vp]
    L.orbhip_test_sincosf.argtypes = [vp, vp, vp, ctypes.c_int64]
    L.orbhip_test_sincosf_sweep.argtypes = [ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    L.orbhip_test_sincosf_sweep.restype = ctypes.c_int64
    # measurement hooks of the dense Cholesky (HIP events around back-to-back launches)
    L.orbhip_test_cholesky.argtypes = [vp, vp, vp, i32, vp, ctypes.POINTER(f32)]
    L.orbhip_test_cholesky_reg.argtypes = [vp, vp, vp, i32, i32, ctypes.POINTER(f32), vp]
    L.orbhip_test_cholesky_blocked.argtypes = [vp, vp, vp, i32, ctypes.POINTER(f32)]
    L.orbhip_test_cholesky_dag.argtypes = [vp, vp, vp, i32, i32, i32, ctypes.POINTER(f32), vp]
    # host only: the matcher's dispatch decision for a call shape (tests assert the route they mean to reach)
    L.orbhip_test_match_route.argtypes = [i32, i32, i32, i32, vp]
    # the persistent KeyFrame members of a KeyFrameDatabase, per slot (tests compare them with the oracle's)
    L.orbhip_test_kfdb_members.argtypes = [vp, i32, vp, vp, vp]
    # the stored list capacity of the Sim3 projection search (tests build a chain deeper than it)
    L.orbhip_test_sim3_list_cap.argtypes = []
    # host only: the projection searches' route for a call's sizes; the last search on a context
    L.orbhip_test_proj_route.argtypes = [i32, i32, i32, vp]
    L.orbhip_test_proj_stats.argtypes = [vp, vp]
    # the last SearchForInitialization on a context: form, round, init_ahead, sizes, need counts
    L.orbhip_test_init_stats.argtypes = [vp, vp]
    # host only: SearchForInitialization's envelope (return code, LDS, list capacity, round cap)
    L.orbhip_test_init_route.argtypes = [i32, i32, i32, i32, vp]
    # the device's PredictScale against host levels over a range of float bit patterns
    L.orbhip_test_predict_scale_sweep.argtypes = [ctypes.c_uint32, ctypes.c_uint32, f32, i32, vp]
    L.orbhip_test_predict_scale_sweep.restype = ctypes.c_int64
    # host only: the steps the device compares a ratio against (one per level, from the host's log)
    L.orbhip_test_level_thresholds.argtypes = [f32, i32, vp]
    # one host frame's intermediates (pyramid levels 1.., candidates per cell, kept keypoints per level,
    # the device error word) and a plan's cell table: tests compare every stage with the oracle
    L.orbhip_test_extract_debug.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbhip_test_cells.argtypes = [vp, i32, i32, vp, i32]
    # host only: OptimizeEssentialGraph's argument check; n, the solver route and H's block count
    L.orbhip_test_essential_graph_check.argtypes = [ctypes.POINTER(EssentialGraphProblemC),
                                                    ctypes.POINTER(EssentialGraphResultC), vp]
    _lib = L
    return L


def torch_stream(stream=None):
    """hipStream_t for a device call on torch tensors: the given torch stream, else torch's
    CURRENT stream (handle 0 = the HIP null stream, which the ABI takes as such) — so the call
    is ordered after the torch work that produced its inputs and before torch reads its
    outputs."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise OrbHipError(rc, what)
    return rc


def ptr(a) -> int | None:
    """Data pointer of a numpy array or a torch tensor (host or device)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        # (the array interface, not a.ctypes: building that object cost ~3 us per pointer, ~14 per
        # BA call)
        return a.__array_interface__["data"][0]
    return a.data_ptr()


class Context:
    """Owns one orbhip_ctx (device memory, pinned staging, one HIP stream). device < 0 (the default):
    the calling thread's current HIP device, i.e. the rank's GPU after torch.cuda.set_device."""

    def __init__(self, device: int = -1, n_features=1000, scale_factor=1.2, n_levels=8, ini_th_fast=20,
                 min_th_fast=7):
        self._h = ctypes.c_void_p()
        prm = OrbParams(int(n_features), float(scale_factor), int(n_levels), int(ini_th_fast), int(min_th_fast))
        check(lib().orbhip_create(ctypes.byref(self._h), int(device), ctypes.byref(prm)), "orbhip_create")

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().orbhip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
