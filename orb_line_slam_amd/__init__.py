"""orb_line_slam_amd -- MI355X (gfx950) implementation of the per-frame feature path of
ORB_Line_SLAM: ORBextractor, Lineextractor, ORBmatcher / LineMatcher Hamming searches and the
Frame stereo matchers, as hand-written HIP kernels behind a C ABI (include/orbline.h).

The Python classes here mirror the reference's C++ class surfaces (same names, argument meaning and
error behaviour) on top of that C ABI via ctypes.  There is no CPU fallback: constructing any
compute object without the built HIP library or without a GPU raises.
"""
from ._lib import (KEYPOINT_DTYPE, KEYLINE_DTYPE, OlfError, OlfParams, default_params, device_count,
                   lib, last_error)
from .extractor import ORBextractor, Lineextractor
from .matcher import ORBmatcher, FrameView, KeyFrameView, MapPointView, MapPointGeom
from .vocabulary import ORBVocabulary, LineVocabulary
from .database import KeyFrameDatabase
from .localmap import MapGraph, UpdateLocalMap, update_local_map_batch
from .connections import UpdateConnections, update_connections_batch, best_covisibles_batch
from .culling import (CullView, keyframe_culling_tables_batch, keyframe_culling_replay, KeyFrameCulling, tracked_map_points_batch, TrackedMapPoints,
                      map_point_culling, MapPointCulling)
from .pose import (pose_params, pose_optimization_with_line_batch, PoseOptimizationWithLine, pose_optimization_with_line_host, discard_outliers_batch,
                   DiscardOutliers, discard_outliers_host)
from .posepoints import pose_optimization_batch, PoseOptimization, pose_optimization_host
from .newpoints import (compute_f12_pairs, ComputeF12, create_new_map_points_batch, CreateNewMapPoints, update_normal_and_depth, UpdateNormalAndDepth)
from .keyframe import (stereo_landmarks_batch, need_new_keyframe_batch, StereoInitialization, CreateNewKeyFrame, UpdateLastFrame, NeedNewKeyFrame,
                       keyframe_rows)
from .sim3solver import sim3_ransac, sim3_state, sim3_draws, sim3_solver_batch, sim3_filter_matches, Sim3Solve, sim3_solver_pairs
from .optsim3 import optimize_sim3_state, optimize_sim3_batch, OptimizeSim3, optimize_sim3_pairs, optimize_sim3_jacobian
from .pnpsolver import pnp_ransac, pnp_state, pnp_draws, pnp_solver_batch, pnp_apply_inliers, PnPSolve, pnp_solver_pairs
from .initializer import (initializer_params, initializer_draws, initializer_state, initializer_batch, initializer_pairs, Initialize, initializer_apply,
                          parallax_degrees)
from . import matcher as LineMatcher
from .frame import StereoFrontEnd, StereoFrames, assign_features_to_grid, features_in_area
from . import synth

__all__ = ["ORBextractor", "Lineextractor", "ORBmatcher", "FrameView", "KeyFrameView", "MapPointView", "MapPointGeom", "ORBVocabulary", "LineVocabulary", "KeyFrameDatabase", "MapGraph", "UpdateLocalMap", "update_local_map_batch", "UpdateConnections", "update_connections_batch", "best_covisibles_batch", "CullView", "keyframe_culling_tables_batch", "keyframe_culling_replay", "KeyFrameCulling", "tracked_map_points_batch", "TrackedMapPoints", "map_point_culling", "MapPointCulling", "pose_params", "pose_optimization_with_line_batch", "PoseOptimizationWithLine", "pose_optimization_with_line_host", "discard_outliers_batch", "DiscardOutliers", "discard_outliers_host", "pose_optimization_batch", "PoseOptimization", "pose_optimization_host", "compute_f12_pairs", "ComputeF12", "create_new_map_points_batch", "CreateNewMapPoints", "update_normal_and_depth", "UpdateNormalAndDepth", "stereo_landmarks_batch", "need_new_keyframe_batch", "StereoInitialization", "CreateNewKeyFrame", "UpdateLastFrame", "NeedNewKeyFrame", "keyframe_rows", "sim3_ransac", "sim3_state", "sim3_draws", "sim3_solver_batch", "sim3_filter_matches", "Sim3Solve", "sim3_solver_pairs", "optimize_sim3_state", "optimize_sim3_batch", "OptimizeSim3", "optimize_sim3_pairs", "optimize_sim3_jacobian", "pnp_ransac", "pnp_state", "pnp_draws", "pnp_solver_batch", "pnp_apply_inliers", "PnPSolve", "pnp_solver_pairs", "initializer_params", "initializer_draws", "initializer_state", "initializer_batch", "initializer_pairs", "Initialize", "initializer_apply", "parallax_degrees", "LineMatcher", "StereoFrontEnd", "StereoFrames", "assign_features_to_grid", "features_in_area", "KEYPOINT_DTYPE", "KEYLINE_DTYPE", "OlfError", "OlfParams", "default_params",
           "device_count", "lib", "last_error", "synth"]
