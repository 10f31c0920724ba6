"""ctypes binding of liborbline_hip.so (include/orbline.h, include/orbline_types.h).

The library is built in-tree by `make -C orb_line_slam_amd/csrc` (or __graft_entry__.build()).
Importing this module never touches the GPU; creating a context does.  A missing library is a hard
error -- there is no pure-Python or CPU path behind these classes.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OLF_LIB_PATH", os.path.join(_HERE, "csrc", "liborbline_hip.so"))
SYNTH_PATH = os.path.join(_HERE, "csrc", "libolf_synth.so")

OLF_OK, OLF_ERR_INVALID, OLF_ERR_CAPACITY, OLF_ERR_HIP, OLF_ERR_NODEVICE = 0, -1, -2, -3, -4
DESC_BYTES = 32

# cv::KeyPoint (28 B) and cv::line_descriptor::KeyLine (68 B) record layouts
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"),
                          ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"), ("startPointY", "<f4"),
                          ("endPointX", "<f4"), ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"),
                          ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"),
                          ("lineLength", "<f4"), ("numOfPixels", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28 and KEYLINE_DTYPE.itemsize == 68


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("conv_gauss_sum256", C.c_int32)]


class LineParams(C.Structure):
    _fields_ = [("lsd_nfeatures", C.c_int32), ("min_line_length", C.c_double), ("lsd_refine", C.c_int32),
                ("lsd_scale", C.c_double), ("lsd_sigma_scale", C.c_double), ("lsd_quant", C.c_double),
                ("lsd_ang_th", C.c_double), ("lsd_log_eps", C.c_double), ("lsd_density_th", C.c_double),
                ("lsd_n_bins", C.c_int32), ("conv_gauss_sum256", C.c_int32), ("conv_resize_exact", C.c_int32), ("conv_seed_order", C.c_int32),
                ("conv_libm_float", C.c_int32)]


class StereoParams(C.Structure):
    _fields_ = [("fx", C.c_float), ("bf", C.c_float), ("matching_s_ws", C.c_int32), ("line_sim_th", C.c_double),
                ("min_ratio_12_l", C.c_double), ("min_disp", C.c_double), ("line_horiz_th", C.c_double),
                ("stereo_overlap_th", C.c_double), ("ls_min_disp_ratio", C.c_double), ("best_lr_matches", C.c_int32),
                ("conv_eigen_recip", C.c_int32)]


class OlfParams(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("struct_size", C.c_uint32), ("orb", OrbParams), ("line", LineParams), ("stereo", StereoParams)]


class FrameBuffers(C.Structure):
    """olf_frame_buffers (include/orbline.h): device or host pointers of the fused stereo-frame entry"""
    _fields_ = [(n, C.c_void_p) for n in ("kps", "desc", "counts", "uright", "depth", "kls", "ldesc", "lcounts", "lmatches12",
                                          "ldisp", "lle")]


class FrameViewC(C.Structure):
    """olf_frame_view (include/orbline.h): the Frame / KeyFrame members read by the per-frame ORBmatcher searches"""
    _fields_ = ([(n, C.c_void_p) for n in ("keys", "desc", "uright")] + [("n", C.c_int32)] +
                [(n, C.c_void_p) for n in ("mp_valid", "mp_obs", "mp_bad", "mp_world", "mp_desc", "outlier", "Tcw")] +
                [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "mbf", "minX", "maxX", "minY", "maxY")] +
                [("scale_factors", C.c_void_p), ("n_levels", C.c_int32)] +
                [(n, C.c_void_p) for n in ("mp_maxd", "mp_mind", "fv_nodes", "fv_offsets", "fv_features")] + [("fv_n", C.c_int32)] +
                [(n, C.c_void_p) for n in ("grid_offsets", "grid_index")])


class TrackBatchC(C.Structure):
    """olf_track_batch (include/orbline.h): device pointers of a batch of frames as SearchByProjection(Frame, Frame) reads them"""
    _fields_ = ([(n, C.c_void_p) for n in ("kps", "desc", "counts")] + [("img_stride", C.c_int32)] +
                [(n, C.c_void_p) for n in ("uright", "cell_offsets", "cell_index", "Tcw", "mp_world", "mp_valid", "mp_obs", "outlier", "mp_desc")] +
                [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "mbf", "minX", "maxX", "minY", "maxY")])


class Sim3RansacC(C.Structure):
    """olf_sim3_ransac (include/orbline.h): SetRansacParameters and the window of one Sim3Solver::iterate"""
    _fields_ = [("fix_scale", C.c_int32), ("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("n_iterations", C.c_int32)]


class Sim3SolverIoC(C.Structure):
    """olf_sim3_solver_io (include/orbline.h): the carried state and the outputs of the solvers of a list of pairs"""
    _fields_ = [(n, C.c_void_p) for n in ("iterations_done", "best_inliers", "best_s", "best_R", "best_t", "best_T12", "accepted", "no_more", "n_inliers",
                                          "inliers", "n_correspondences", "counts")]


class PnpRansacC(C.Structure):
    """olf_pnp_ransac (include/orbline.h): SetRansacParameters and the window of one PnPsolver::iterate"""
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32), ("n_iterations", C.c_int32),
                ("epsilon", C.c_float), ("th2", C.c_float)]


class PnpSolverIoC(C.Structure):
    """olf_pnp_solver_io (include/orbline.h): the carried state and the outputs of the solvers of a list of pairs"""
    _fields_ = [(n, C.c_void_p) for n in ("iterations_done", "best_inliers", "best_Tcw", "best_flags", "refined_inliers", "refined_Tcw", "refined_flags",
                                          "accepted", "no_more", "n_inliers", "inliers", "Tcw", "n_correspondences", "counts")]


class InitializerParamsC(C.Structure):
    """olf_initializer_params (include/orbline.h): Initializer(frame, sigma, iterations) and ReconstructH / ReconstructF's minParallax, minTriangulated"""
    _fields_ = [("sigma", C.c_float), ("max_iterations", C.c_int32), ("min_parallax", C.c_float), ("min_triangulated", C.c_int32)]


class InitializerIoC(C.Structure):
    """olf_initializer_io (include/orbline.h): the outputs of Initializer::Initialize for a list of pairs"""
    _fields_ = [(n, C.c_void_p) for n in ("ok", "n_correspondences", "model", "score_H", "score_F", "H21", "F21", "inliers_H", "inliers_F", "R21", "t21", "P3D",
                                          "triangulated", "n_good", "cos_parallax", "hypothesis")]


class LocalMapC(C.Structure):
    """olf_local_map (include/orbline.h): the local map of a batch as device arrays, and optionally each frame's list of indices into it"""
    _fields_ = ([(n, C.c_void_p) for n in ("world", "normal", "maxd", "mind", "desc", "obs", "bad")] + [("n_mp", C.c_int32)] +
                [(n, C.c_void_p) for n in ("list_offsets", "list_index")] + [("n_entries", C.c_int32)])


class LineBatchC(C.Structure):
    """olf_line_batch (include/orbline.h): device pointers of a batch of frames as the line searches read them"""
    _fields_ = ([(n, C.c_void_p) for n in ("kls", "ldesc", "lcounts")] + [("img_stride", C.c_int32)] + [(n, C.c_void_p) for n in ("ldisp", "Tcw")] +
                [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "minX", "maxX", "minY", "maxY")])


class LocalLineMapC(C.Structure):
    """olf_local_line_map (include/orbline.h): the map lines of a batch as device arrays, and optionally each frame's list of indices into them"""
    _fields_ = ([(n, C.c_void_p) for n in ("world", "desc", "obs", "bad")] + [("n_ml", C.c_int32)] +
                [(n, C.c_void_p) for n in ("list_offsets", "list_index")] + [("n_entries", C.c_int32)])


class MapGraphC(C.Structure):
    """olf_map_graph (include/orbline_types.h): one snapshot of the map as Tracking::UpdateLocalMap walks it"""
    _fields_ = ([(n, C.c_int32) for n in ("n_kf", "n_mp", "n_ml")] +
                [(n, C.c_void_p) for n in ("mp_obs_offsets", "mp_obs_kf", "mp_bad", "ml_bad", "kf_bad", "kf_mp_offsets", "kf_mp_index", "kf_ml_offsets", "kf_ml_index",
                                           "kf_covis_offsets", "kf_covis_index", "kf_child_offsets", "kf_child_index", "kf_parent")])


class CullViewC(C.Structure):
    """olf_cull_view (include/orbline_types.h): what KeyFrameCulling reads beyond an olf_map_graph"""
    _fields_ = [(n, C.c_void_p) for n in ("mp_obs_slot", "mp_nobs", "kf_slot_octave", "kf_slot_depth", "kf_slot_stereo", "kf_th_depth", "kf_mode")]


class PoseParamsC(C.Structure):
    """olf_pose_params (include/orbline.h): Config's optimisation parameters as Optimizer::PoseOptimizationWithLine reads them"""
    _fields_ = ([("max_iters_ref", C.c_int32)] + [(n, C.c_double) for n in ("homog_th", "min_error", "min_error_change", "inlier_k")] +
                [(n, C.c_int32) for n in ("use_motion_model", "has_points", "has_lines")])


class PoseBatchC(C.Structure):
    """olf_pose_batch (include/orbline.h): a batch of frames as the pose optimiser reads them"""
    _fields_ = ([(n, C.c_void_p) for n in ("kps", "counts", "kls", "lcounts")] + [("img_stride", C.c_int32)] +
                [(n, C.c_void_p) for n in ("lle", "Tcw", "Tcw_prev", "DT_cov_in")] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy")] +
                [(n, C.c_void_p) for n in ("frame_mp", "mp_index_offset", "mp_world")] + [("n_mp", C.c_int32)] +
                [(n, C.c_void_p) for n in ("frame_ml", "ml_index_offset", "ml_world")] + [("n_ml", C.c_int32)] +
                [(n, C.c_void_p) for n in ("outlier", "outlier_l")])


class PoseOutputsC(C.Structure):
    """olf_pose_outputs (include/orbline.h): what the pose optimiser writes per frame"""
    _fields_ = [(n, C.c_void_p) for n in ("Tcw_out", "DT", "DT_cov", "DT_cov_eig", "err_norm", "good", "outlier_out", "outlier_l_out", "n_inliers", "iters", "status")]


class PosePointsBatchC(C.Structure):
    """olf_pose_points_batch (include/orbline.h): the rows Optimizer::PoseOptimization reads"""
    _fields_ = ([(n, C.c_void_p) for n in ("kps", "counts")] + [("img_stride", C.c_int32), ("uright", C.c_void_p)] +
                [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "bf")] + [(n, C.c_void_p) for n in ("Tcw", "frame_mp", "mp_world")] + [("n_mp", C.c_int32)] +
                [(n, C.c_void_p) for n in ("mp_index_offset", "pairs", "row_active")])


class PosePointsOutputsC(C.Structure):
    """olf_pose_points_outputs (include/orbline.h): what Optimizer::PoseOptimization writes per row"""
    _fields_ = [(n, C.c_void_p) for n in ("Tcw_out", "outlier_out", "n_good", "n_initial", "chi2", "passes", "iters", "status")]


class OptSim3IoC(C.Structure):
    """olf_optimize_sim3_io (include/orbline.h): the in / out match rows and the outputs of Optimizer::OptimizeSim3 for a list of pairs"""
    _fields_ = [(n, C.c_void_p) for n in ("matches12", "S12_out", "s12_out", "R12_out", "t12_out", "Scw_out", "n_inliers", "n_correspondences", "n_bad_first",
                                          "iters", "status", "chi2")]


class DiscardBatchC(C.Structure):
    """olf_discard_batch (include/orbline.h): the rows the "discard outliers" loops read and change"""
    _fields_ = ([(n, C.c_void_p) for n in ("counts", "lcounts")] + [("img_stride", C.c_int32)] +
                [(n, C.c_void_p) for n in ("frame_mp", "frame_ml", "outlier", "outlier_l", "mp_index_offset", "ml_index_offset", "mp_obs", "ml_obs")] +
                [("n_mp", C.c_int32), ("n_ml", C.c_int32)])


class LandmarksBatchC(C.Structure):
    """olf_landmarks_batch (include/orbline.h): the frames of a batch as the three producers of stereo landmarks read them"""
    _fields_ = ([(n, C.c_void_p) for n in ("kps", "counts", "kls", "lcounts")] + [("img_stride", C.c_int32)] +
                [(n, C.c_void_p) for n in ("depth", "ldisp", "Twc", "frame_mp", "frame_ml", "mp_nobs")] + [("n_mp", C.c_int32), ("ml_nobs", C.c_void_p), ("n_ml", C.c_int32)] +
                [(n, C.c_void_p) for n in ("new_base_mp", "new_base_ml")] + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "mbf", "thDepth")])


LANDMARKS_OUTPUTS = ("n_visited", "n_created", "visit_order", "visit_order_l", "created_order", "created_order_l", "created", "created_l", "frame_mp_out",
                     "frame_ml_out", "mp_world", "mp_normal", "mp_maxd", "mp_mind", "ml_world_d", "ml_world", "status")


class LandmarksOutputsC(C.Structure):
    """olf_landmarks_outputs (include/orbline.h)"""
    _fields_ = [(n, C.c_void_p) for n in LANDMARKS_OUTPUTS]


class KeyFrameTestBatchC(C.Structure):
    """olf_keyframe_test_batch (include/orbline.h): what Tracking::NeedNewKeyFrame reads of a batch of frames"""
    _fields_ = ([(n, C.c_void_p) for n in ("counts", "lcounts")] + [("img_stride", C.c_int32)] +
                [(n, C.c_void_p) for n in ("depth", "frame_mp", "outlier", "ldisp", "frame_ml", "outlier_l", "ldisp_frame", "rows", "n_ref_matches",
                                           "n_ref_matches_l", "n_inliers")] + [("mbf", C.c_float), ("thDepth", C.c_float)])


KEYFRAME_TEST_OUTPUTS = ("need", "interrupt_ba", "counts", "conditions", "status")


class KeyFrameTestOutputsC(C.Structure):
    """olf_keyframe_test_outputs (include/orbline.h)"""
    _fields_ = [(n, C.c_void_p) for n in KEYFRAME_TEST_OUTPUTS]


class BowCsrC(C.Structure):
    """olf_bow_csr (include/orbline.h): n BoW vectors as offsets, ascending word ids and values"""
    _fields_ = [(n, C.c_void_p) for n in ("off", "ids", "vals")]


class KfdbTablesC(C.Structure):
    """olf_kfdb_tables (include/orbline.h): one vocabulary's [n_queries][n_slots] common / first / score tables"""
    _fields_ = [(n, C.c_void_p) for n in ("common", "first", "score")]


KFDB_MAX_WORDS, KFDB_MAX_SLOTS, KFDB_MAX_CELLS = 4096, 1 << 20, 1 << 26
KFDB_LOOP, KFDB_LOOP_LINE, KFDB_RELOC, KFDB_RELOC_LINE = range(4)


# Frame::mGrid as two int32 arrays (include/orbline_types.h) and one Frame::GetFeaturesInArea call
GRID_COLS, GRID_ROWS, GRID_CELLS, GRID_MAX_KEYS = 64, 48, 3072, 8192
AREA_QUERY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("r", "<f4"), ("min_level", "<i4"), ("max_level", "<i4")])
assert AREA_QUERY_DTYPE.itemsize == 20


class OlfError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        super().__init__(f"{where}: status {code}: {last_error()}")


_lib = None


def _torch_runtime_first():
    """PyTorch ships its own copy of the HIP runtime.  A process that uses both this library and torch (bench.py, pipeline.py,
    distributed.py) must bring torch's runtime up first: the other order leaves this library without a visible device.  So when torch
    is installed it is imported and initialised before the library is loaded (set OLF_NO_TORCH=1 to skip: pure ctypes use)."""
    import importlib.util
    if os.environ.get("OLF_NO_TORCH") or importlib.util.find_spec("torch") is None:
        return
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass


def lib():
    """The loaded C-ABI library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C orb_line_slam_amd/csrc` "
                              "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
        _torch_runtime_first()
        L = C.CDLL(LIB_PATH)
        L.olf_last_error.restype = C.c_char_p
        L.olf_ctx_create.argtypes = [C.POINTER(OlfParams), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.olf_ctx_destroy.argtypes = [C.c_void_p]
        L.olf_ctx_destroy.restype = None
        L.olf_ctx_synchronize.argtypes = [C.c_void_p]
        L.olf_ctx_poll_status.argtypes = [C.c_void_p]
        L.olf_orb_scale_tables.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        L.olf_orb_level_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_orb_capacity.argtypes = [C.c_void_p]
        L.olf_orb_extract_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_orb_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_orb_pyramid_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.olf_orb_debug_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.olf_stereo_points_dev.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        L.olf_stereo_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.olf_match_bf_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        L.olf_match_bf.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p]
        L.olf_knn2.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_hamming_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.olf_line_capacity.argtypes = [C.c_void_p]
        L.olf_line_extract_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.olf_line_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.olf_lbd_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.olf_lsd_debug_scaled.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.olf_stereo_lines_dev.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        L.olf_stereo_lines.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        L.olf_stereo_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(FrameBuffers), C.c_void_p]
        L.olf_stereo_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(FrameBuffers)]
        L.olf_match_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_search_by_projection.argtypes = [C.c_void_p, C.POINTER(FrameViewC), C.POINTER(FrameViewC), C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.olf_search_by_projection_match12.argtypes = [C.c_void_p, C.POINTER(FrameViewC), C.POINTER(FrameViewC), C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_search_by_bow.argtypes = [C.c_void_p, C.POINTER(FrameViewC), C.POINTER(FrameViewC), C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        L.olf_search_for_initialization.argtypes = [C.c_void_p, C.POINTER(FrameViewC), C.POINTER(FrameViewC), C.c_void_p, C.c_int, C.c_float, C.c_int,
                                                    C.c_void_p, C.c_void_p]
        V = C.POINTER(FrameViewC)
        L.olf_is_in_frustum.argtypes = [V, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float] + [C.c_void_p] * 4
        L.olf_search_by_projection_kf.argtypes = [C.c_void_p, V, V, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.olf_search_by_bow_kf.argtypes = [C.c_void_p, V, V, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        L.olf_search_for_triangulation.argtypes = [C.c_void_p, V, V, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.olf_fuse_search.argtypes = [C.c_void_p, V, C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_fuse_search_sim3.argtypes = [C.c_void_p, V, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_void_p, C.c_void_p]
        L.olf_search_by_projection_sim3.argtypes = [C.c_void_p, V, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_search_by_sim3.argtypes = [C.c_void_p, V, V, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_search_local_map.argtypes = [C.c_void_p, C.POINTER(FrameViewC), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        L.olf_match_candidates_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_frame_grid_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_float] * 4 + [C.c_void_p] * 3
        L.olf_frame_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_float] * 4 + [C.c_void_p] * 2
        L.olf_features_in_area_dev.argtypes = ([C.c_void_p] * 4 + [C.c_float] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
        L.olf_features_in_area.argtypes = ([C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_float] * 4 +
                                           [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
        L.olf_ctx_device_buffers.argtypes = [C.c_void_p, C.POINTER(FrameBuffers)]
        L.olf_cvt_gray.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.olf_remap_linear.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.olf_debug_lsd_waves.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.olf_debug_lsd_pool.argtypes = [C.c_void_p, C.c_int]
        L.olf_debug_lsd_groups.argtypes = [C.c_void_p, C.c_int]
        L.olf_debug_lsd_scatter.argtypes = [C.c_void_p, C.c_int]
        L.olf_debug_lsd_log_cap.argtypes = [C.c_void_p, C.c_int]
        L.olf_debug_seed_sort_mode.argtypes = [C.c_void_p, C.c_int]
        L.olf_debug_seed_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
        L.olf_frames_pack_bound.argtypes = [C.c_void_p, C.c_int]
        L.olf_frames_pack_bound.restype = C.c_size_t
        L.olf_frames_pack_dev.argtypes = [C.c_void_p, C.POINTER(FrameBuffers), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.olf_ctx_set_input_event.argtypes = [C.c_void_p, C.c_void_p]
        L.olf_ctx_set_deferred_join.argtypes = [C.c_void_p, C.c_int]
        L.olf_stereo_frames_join_dev.argtypes = [C.c_void_p, C.c_void_p]
        L.olf_stereo_points_mask_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.olf_search_by_projection_batch_dev.argtypes = [C.c_void_p, C.POINTER(TrackBatchC), C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_unproject_stereo_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_float] * 4 + [C.c_void_p] * 3
        L.olf_predict_scale_thresholds.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.olf_is_in_frustum_batch_dev.argtypes = [C.c_void_p, C.POINTER(TrackBatchC), C.c_int, C.POINTER(LocalMapC), C.c_void_p, C.c_float] + [C.c_void_p] * 5
        L.olf_search_local_map_batch_dev.argtypes = [C.c_void_p, C.POINTER(TrackBatchC), C.c_int, C.POINTER(LocalMapC), C.c_void_p, C.c_float, C.c_float,
                                                     C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_is_in_frustum_l.argtypes = [V, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_local_lines_assign.argtypes = ([C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_float] * 4 +
                                             [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
        L.olf_track_lines_assign.argtypes = ([C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_float] * 4 +
                                             [C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p])
        L.olf_is_in_frustum_l_batch_dev.argtypes = [C.c_void_p, C.POINTER(LineBatchC), C.c_int, C.POINTER(LocalLineMapC)] + [C.c_void_p] * 4
        L.olf_search_local_lines_batch_dev.argtypes = [C.c_void_p, C.POINTER(LineBatchC), C.c_int, C.POINTER(LocalLineMapC), C.c_void_p, C.c_float] + [C.c_void_p] * 6
        L.olf_track_lines_batch_dev.argtypes = ([C.c_void_p, C.POINTER(LineBatchC), C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double] +
                                                [C.c_void_p] * 5)
        L.olf_debug_copy_bandwidth.argtypes =[C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
        L.olf_debug_fdiv_sweep.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.olf_debug_sqrtq_sweep.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
        L.olf_debug_align_sweep.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.olf_debug_seed_sort_wide.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]
        L.olf_distinctive_descriptors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.olf_voc_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.olf_voc_load_text.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.olf_voc_destroy.argtypes = [C.c_void_p]
        L.olf_voc_destroy.restype = None
        L.olf_voc_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 6
        L.olf_bow_words_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_bow_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.olf_search_by_bow_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.olf_search_for_triangulation_batch_dev.argtypes = ([C.c_void_p, C.c_void_p, C.POINTER(TrackBatchC), C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 3 +
                                                             [C.c_void_p] * 3)
        L.olf_search_by_bow_pairs_dev.argtypes = ([C.c_void_p, C.c_void_p, C.POINTER(TrackBatchC), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                                   C.c_int, C.c_int] + [C.c_void_p] * 3)
        L.olf_fuse_search_batch_dev.argtypes = ([C.c_void_p, C.POINTER(TrackBatchC), C.c_int, C.POINTER(LocalMapC)] + [C.c_void_p] * 3 + [C.c_float] +
                                                [C.c_void_p] * 4)
        L.olf_search_by_sim3_pairs_dev.argtypes = ([C.c_void_p, C.POINTER(TrackBatchC), C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4 + [C.c_float] +
                                                   [C.c_void_p] * 5)
        L.olf_search_by_projection_kf_pairs_dev.argtypes = ([C.c_void_p, C.POINTER(TrackBatchC), C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4 +
                                                            [C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3)
        L.olf_search_by_projection_sim3_batch_dev.argtypes = ([C.c_void_p, C.POINTER(TrackBatchC), C.c_int, C.POINTER(LocalMapC)] + [C.c_void_p] * 2 +
                                                              [C.c_float] + [C.c_void_p] * 3)
        L.olf_bow_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        P = C.c_void_p
        L.olf_kfdb_create.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P)]
        L.olf_kfdb_destroy.argtypes = [P]
        L.olf_kfdb_destroy.restype = None
        L.olf_kfdb_add.argtypes = [P, P, P, C.c_int, P, P, C.c_int, C.POINTER(C.c_int32)]
        L.olf_kfdb_erase.argtypes = [P, C.c_int32]
        L.olf_kfdb_clear.argtypes = [P]
        L.olf_kfdb_size.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.olf_kfdb_state.argtypes = [P, P, P, P]
        L.olf_kfdb_tables_dev.argtypes = [P, C.c_int, C.POINTER(BowCsrC), C.POINTER(BowCsrC), C.POINTER(KfdbTablesC), C.POINTER(KfdbTablesC), P]
        L.olf_kfdb_select.argtypes = ([P, C.c_int, C.c_int] + [P] * 8 + [C.c_int, C.POINTER(KfdbTablesC), C.POINTER(KfdbTablesC), P, P, C.c_int])
        L.olf_kfdb_detect.argtypes = ([P, C.c_int, C.c_int, P, C.POINTER(BowCsrC), C.POINTER(BowCsrC)] + [P] * 9 + [C.c_int])
        L.olf_bow_score_pairs_dev.argtypes = [P, C.c_int, C.c_int, P, C.POINTER(BowCsrC), C.c_int, P, P]
        L.olf_bow_score.argtypes = [P, P, P, C.c_int, P, P, C.c_int, C.POINTER(C.c_double)]
        L.olf_update_local_map_batch_dev.argtypes = ([P, C.POINTER(MapGraphC), C.c_int, C.c_int] + [P] * 8 + [P, P, C.c_int] * 3 + [P])
        L.olf_update_local_map.argtypes = ([P, C.POINTER(MapGraphC), C.c_int, C.c_int] + [P] * 8 + [P, P, C.c_int] * 3)
        L.olf_update_connections_batch_dev.argtypes = ([P, C.POINTER(MapGraphC), C.c_int, P, C.c_int] + [P] * 3 + [P, P, P, C.c_int] * 2 + [P])
        L.olf_update_connections.argtypes = ([P, C.POINTER(MapGraphC), C.c_int, P, C.c_int] + [P] * 3 + [P, P, P, C.c_int] * 2)
        L.olf_best_covisibles_batch_dev.argtypes = [P, C.c_int] + [P] * 6
        L.olf_keyframe_culling_tables_dev.argtypes = [P, C.POINTER(MapGraphC), C.POINTER(CullViewC), C.c_int, P, C.c_int] + [P] * 6 + [C.c_int, P]
        L.olf_keyframe_culling_replay.argtypes = [C.POINTER(MapGraphC), C.POINTER(CullViewC), C.c_int] + [P] * 13
        L.olf_keyframe_culling.argtypes = [P, C.POINTER(MapGraphC), C.POINTER(CullViewC), C.c_int, P, C.c_int] + [P] * 10
        L.olf_tracked_map_points_batch_dev.argtypes = [P, C.POINTER(MapGraphC), P, P, C.c_int, P, C.c_int, C.c_int, P, P, P]
        L.olf_tracked_map_points.argtypes = [P, C.POINTER(MapGraphC), P, P, C.c_int, P, C.c_int, C.c_int, P, P]
        L.olf_map_point_culling_dev.argtypes = [P, C.c_int] + [P] * 5 + [C.c_int64, C.c_int, P, P]
        L.olf_map_point_culling.argtypes = [P, C.c_int] + [P] * 5 + [C.c_int64, C.c_int, P]
        L.olf_compute_f12_pairs_dev.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, C.c_int, P, P, P]
        L.olf_compute_f12.argtypes = [P, P] + [C.c_float] * 4 + [P]
        L.olf_create_new_map_points_batch_dev.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, P, C.c_float, C.c_int, P, P, C.c_int, P, P, P, P]
        L.olf_create_new_map_points.argtypes = [C.POINTER(TrackBatchC), C.c_int, C.c_int, P, C.c_float, P, C.c_int, C.c_int, P, P, C.c_int, P, P, P, P]
        L.olf_compute_f12_pairs.argtypes = [P, P, C.c_int] + [C.c_float] * 4 + [C.c_int, P, P]
        L.olf_create_new_map_points_pairs.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, P, C.c_float, C.c_int, P, P, C.c_int, P, P, P]
        L.olf_update_normal_and_depth_points.argtypes = [P, C.POINTER(MapGraphC), C.POINTER(CullViewC), C.c_int] + [P] * 7
        L.olf_sim3_solver_pairs_dev.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, P, C.c_int, P, P, C.POINTER(Sim3RansacC), P, C.POINTER(Sim3SolverIoC), P]
        L.olf_sim3_filter_matches_dev.argtypes = [P, C.c_int, P, P, P, P, P]
        L.olf_sim3_solver.argtypes = [C.POINTER(TrackBatchC), C.c_int, C.c_int, P, P, C.c_int, C.c_int, C.c_int, P, C.POINTER(Sim3RansacC), P,
                                      C.POINTER(Sim3SolverIoC), P]
        L.olf_sim3_solver_pairs.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, P, C.c_int, P, P, C.POINTER(Sim3RansacC), P, C.POINTER(Sim3SolverIoC)]
        L.olf_debug_sim3_solver_lds_limit.argtypes = [C.c_int]
        L.olf_debug_sim3_solver_gate.argtypes = [C.c_float, P]
        L.olf_debug_sim3_solver_cap.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, P]
        L.olf_pnp_solver_pairs_dev.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, P, C.c_int, P, P, C.POINTER(PnpRansacC), P, C.POINTER(PnpSolverIoC), P]
        L.olf_pnp_apply_inliers_dev.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, C.c_int] + [P] * 9
        L.olf_pnp_solver.argtypes = [C.POINTER(TrackBatchC), C.c_int, C.c_int, P, P, C.c_int, C.c_int, C.c_int, P, C.POINTER(PnpRansacC), P,
                                     C.POINTER(PnpSolverIoC), P]
        L.olf_pnp_solver_pairs.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, P, C.c_int, P, P, C.POINTER(PnpRansacC), P, C.POINTER(PnpSolverIoC)]
        L.olf_debug_pnp_solver_lds_limit.argtypes = [C.c_int]
        L.olf_debug_pnp_solver_parameters.argtypes = [C.c_int, C.POINTER(PnpRansacC), P, P]
        L.olf_initializer_pairs_dev.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, C.c_int, P, P, C.POINTER(InitializerParamsC), P, C.POINTER(InitializerIoC), P]
        L.olf_initializer_apply_dev.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, C.c_int] + [P] * 10
        L.olf_initializer.argtypes = [C.POINTER(TrackBatchC), C.c_int, C.c_int, C.c_int, C.c_int, P, C.POINTER(InitializerParamsC), P, C.POINTER(InitializerIoC), P]
        L.olf_initializer_pairs.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, C.c_int, P, P, C.POINTER(InitializerParamsC), P, C.POINTER(InitializerIoC)]
        L.olf_debug_initializer_lds_limit.argtypes = [C.c_int]
        L.olf_debug_initializer_cos_thresholds.argtypes = [C.c_float, P, P]
        L.olf_debug_initializer_sample.argtypes = [C.c_int, P, P]
        L.olf_update_normal_and_depth_dev.argtypes = [P, C.POINTER(MapGraphC), C.POINTER(CullViewC), C.c_int] + [P] * 8
        L.olf_update_normal_and_depth.argtypes = [C.POINTER(MapGraphC), C.POINTER(CullViewC), C.c_int] + [P] * 5 + [C.c_int] + [P] * 4
        L.olf_pose_default_params.argtypes = [C.POINTER(PoseParamsC)]
        L.olf_pose_default_params.restype = None
        L.olf_pose_optimization_with_line_batch_dev.argtypes = [P, C.POINTER(PoseBatchC), C.c_int, C.POINTER(PoseParamsC), C.POINTER(PoseOutputsC), P]
        L.olf_pose_optimization_with_line.argtypes = [C.POINTER(PoseBatchC), C.c_int, C.c_int, P, C.c_int, C.POINTER(PoseParamsC), C.POINTER(PoseOutputsC)]
        L.olf_discard_outliers_batch_dev.argtypes = [P, C.POINTER(DiscardBatchC), C.c_int, C.c_int, C.c_int, C.c_int, P, P]
        L.olf_pose_optimization_with_line_frame.argtypes = [P, C.POINTER(PoseBatchC), C.POINTER(PoseParamsC), C.POINTER(PoseOutputsC)]
        L.olf_discard_outliers_frame.argtypes = [P, C.POINTER(DiscardBatchC), C.c_int, C.c_int, C.c_int, P]
        L.olf_discard_outliers.argtypes = [C.POINTER(DiscardBatchC), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P]
        L.olf_pose_optimization_batch_dev.argtypes = [P, C.POINTER(PosePointsBatchC), C.c_int, C.c_int, C.POINTER(PosePointsOutputsC), P]
        L.olf_pose_optimization.argtypes = [C.POINTER(PosePointsBatchC), C.c_int, C.c_int, P, C.c_int, C.POINTER(PosePointsOutputsC)]
        L.olf_pose_optimization_rows.argtypes = [P, C.POINTER(PosePointsBatchC), C.c_int, C.c_int, C.POINTER(PosePointsOutputsC)]
        L.olf_debug_pose_points_lds_limit.argtypes = [C.c_int]
        L.olf_optimize_sim3_pairs_dev.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, P, C.c_int, P, P, P, P, C.c_float, C.c_int, P, C.POINTER(OptSim3IoC), P]
        L.olf_optimize_sim3.argtypes = [C.POINTER(TrackBatchC), C.c_int, C.c_int, P, P, C.c_int, C.c_int, C.c_int, C.c_float, P, P, C.c_float, C.c_int,
                                        C.POINTER(OptSim3IoC)]
        L.olf_optimize_sim3_pairs.argtypes = [P, C.POINTER(TrackBatchC), C.c_int, P, C.c_int, P, P, P, P, C.c_float, C.c_int, P, C.POINTER(OptSim3IoC)]
        L.olf_debug_optimize_sim3_lds_limit.argtypes = [C.c_int]
        L.olf_debug_optimize_sim3_jacobian.argtypes = [P, C.c_int, P, P, P, C.c_int, P]
        L.olf_stereo_landmarks_batch_dev.argtypes = [P, C.POINTER(LandmarksBatchC), C.c_int, C.c_int, C.POINTER(LandmarksOutputsC), P]
        L.olf_stereo_landmarks.argtypes = [C.POINTER(LandmarksBatchC), C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int, C.POINTER(LandmarksOutputsC)]
        L.olf_stereo_landmarks_frames.argtypes = [P, C.POINTER(LandmarksBatchC), C.c_int, C.c_int, C.POINTER(LandmarksOutputsC)]
        L.olf_need_new_keyframe_batch_dev.argtypes = [P, C.POINTER(KeyFrameTestBatchC), C.c_int, C.POINTER(KeyFrameTestOutputsC), P]
        L.olf_need_new_keyframe.argtypes = [C.POINTER(KeyFrameTestBatchC), C.c_int, C.c_int, C.c_int, C.POINTER(KeyFrameTestOutputsC)]
        L.olf_need_new_keyframe_frames.argtypes = [P, C.POINTER(KeyFrameTestBatchC), C.c_int, C.POINTER(KeyFrameTestOutputsC)]
        L.olf_profile_enable.argtypes = [C.c_void_p, C.c_int]
        L.olf_profile_reset.argtypes = [C.c_void_p]
        L.olf_profile_stage_name.restype = C.c_char_p
        L.olf_profile_stage_name.argtypes = [C.c_int]
        L.olf_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def last_error():
    return lib().olf_last_error().decode()


def device_count():
    return int(lib().olf_device_count())


def default_params():
    p = OlfParams()
    rc = lib().olf_default_params(C.byref(p))
    if rc != OLF_OK:
        raise OlfError(rc, "olf_default_params")
    return p


def check(rc, where):
    if rc != OLF_OK:
        raise OlfError(rc, where)


def ptr(a):
    """void* of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One olf_ctx: fixed image size, parameters and per-call image capacity."""

    def __init__(self, params, width, height, max_images):
        self.params, self.width, self.height, self.max_images = params, int(width), int(height), int(max_images)
        h = C.c_void_p()
        check(lib().olf_ctx_create(C.byref(params), self.width, self.height, self.max_images, C.byref(h)), "olf_ctx_create")
        self.handle = h
        self.nlevels = params.orb.nlevels
        self.orb_capacity = int(lib().olf_orb_capacity(self.handle))
        self.line_capacity = int(lib().olf_line_capacity(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            lib().olf_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile(self, on=True):
        check(lib().olf_profile_enable(self.handle, int(on)), "olf_profile_enable")
        check(lib().olf_profile_reset(self.handle), "olf_profile_reset")

    def profile_read(self):
        """{stage: (total_ms, calls)} accumulated since profile(True)"""
        n = lib().olf_profile_stage_count()
        ms = np.zeros(n, np.float64)
        calls = np.zeros(n, np.int32)
        check(lib().olf_profile_read(self.handle, ptr(ms), ptr(calls)), "olf_profile_read")
        return {lib().olf_profile_stage_name(i).decode(): (float(ms[i]), int(calls[i])) for i in range(n)}

    def synchronize(self):
        """wait for the context's streams; raises OlfError if a *_dev call issued since the last check overflowed a device buffer"""
        check(lib().olf_ctx_synchronize(self.handle), "olf_ctx_synchronize")

    def set_input_event(self, event):
        """olf_ctx_set_input_event: `event` a recorded torch.cuda.Event (or None): the line stream of olf_stereo_frames_dev then waits for it instead of
        forking from the caller's stream, so batch k + 1's LSD front runs beside batch k's tail.  The context keeps the raw handle only: keep the
        event alive while it is set."""
        check(lib().olf_ctx_set_input_event(self.handle, C.c_void_p(event.cuda_event) if event is not None else None), "olf_ctx_set_input_event")

    def poll_status(self):
        """the same check without waiting for any stream (the caller has synchronised its own)"""
        check(lib().olf_ctx_poll_status(self.handle), "olf_ctx_poll_status")
