"""The entries that produce map arrays: LocalMapping::ComputeF12 (src/LocalMapping.cc:536-553) for a list of key-frame pairs and
MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:342-383) for a list of map points of one snapshot (include/orbline.h; csrc/newpoints_batch.hip,
newpoints_host.cpp, newpoints_terms.hpp).

  compute_f12_pairs         device tensors: F12 of every listed pair, the d_F12 of ORBmatcher.search_for_triangulation_batch
  ComputeF12                host arrays, no device: one pair from its two poses
  update_normal_and_depth   device tensors: normal, maxd and mind of the listed points, in place
  UpdateNormalAndDepth      host arrays, no device

The normal is summed over a point's observation row in row order.  The reference iterates a std::map<KeyFrame*, size_t>, i.e. in address order; a caller
who lets ascending key-frame index stand for ascending address (C.15 / C.16) passes every row of mp_obs ascending."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import lib, ptr
from .culling import CullView, _graph_dev
from .matcher import _call_dev, _ctx, _dev, _new

STATUS_OCTAVE, STATUS_POINT_INDEX, STATUS_KF_INDEX = 256, 512, 4096  # the bits UpdateNormalAndDepth returns


def compute_f12_pairs(Tcw, camera, pairs, out=None, n_frames=None, context=None):
    """olf_compute_f12_pairs_dev on torch's current stream, without a synchronise.  Tcw: float32 device tensor [n_frames, 16] (mTcw, row-major); camera =
    (fx, fy, cx, cy); pairs: int32 device tensor [n_pairs, 2] = (kf1, kf2).  Returns the float32 device tensor F12 [n_pairs, 9] (row-major, x1^T F12 x2).
    A pair outside the batch or with kf1 == kf2 keeps what `out` held and is reported by the context's next synchronize() / poll_status()."""
    import torch
    ctx = _ctx(context)
    n_pairs = int(pairs.shape[0])
    n = int(Tcw.shape[0]) if n_frames is None else int(n_frames)
    if out is None:
        out = _new((n_pairs, 9), dtype=torch.float32)
    tb = _lib.TrackBatchC()
    tb.Tcw = _dev(Tcw, torch.float32, "Tcw")
    tb.fx, tb.fy, tb.cx, tb.cy = (float(v) for v in camera)
    _call_dev("olf_compute_f12_pairs_dev", ctx, C.byref(tb), n, n_pairs, _dev(pairs, torch.int32, "pairs"), _dev(out, torch.float32, "F12"))
    return out


def ComputeF12(Tcw1, Tcw2, camera):
    """LocalMapping::ComputeF12(pKF1, pKF2) from host arrays, no device: olf_compute_f12.  Tcw1, Tcw2: the 4 x 4 poses; camera = (fx, fy, cx, cy).
    Returns F12 as a float32 array [3, 3]."""
    T1, T2 = (np.ascontiguousarray(T, dtype=np.float32).reshape(-1) for T in (Tcw1, Tcw2))
    if T1.shape[0] != 16 or T2.shape[0] != 16:
        raise ValueError("ComputeF12: two 4 x 4 poses expected")
    F = np.zeros(9, np.float32)
    _lib.check(lib().olf_compute_f12(ptr(T1), ptr(T2), *(float(v) for v in camera), ptr(F)), "olf_compute_f12")
    return F.reshape(3, 3)


CODE_NONE, CODE_TRIANGULATED, CODE_UNPROJECT_1, CODE_UNPROJECT_2 = 0, 1, 2, 3
CODE_LOW_PARALLAX, CODE_W_ZERO, CODE_Z1, CODE_Z2, CODE_REPROJ_1, CODE_REPROJ_2, CODE_ZERO_DIST, CODE_SCALE_RATIO = range(16, 24)


def create_new_map_points_batch(n_frames, kps, counts, uright, depth, Tcw, camera, mb, pairs, matches12, monocular=False, img_stride=2, out=None, context=None):
    """olf_create_new_map_points_batch_dev on torch's current stream, without a synchronise: the body of LocalMapping::CreateNewMapPoints behind the search
    for every match of every listed pair.  kps / counts in the extractor's layout (frame j = image j * img_stride), uright, depth [n_frames, capacity],
    Tcw [n_frames, 4, 4]: device tensors; camera = (fx, fy, cx, cy, mbf); mb: the key frames' mb; pairs int32 [n_pairs, 2]; matches12 int32
    [n_pairs, capacity] as search_for_triangulation_batch returns it.  out = (x3D, code, nnew) to write into (rows of refused pairs keep what they hold).
    Returns (x3D float32 [n_pairs, capacity, 3], code uint8 [n_pairs, capacity], nnew int32 [n_pairs]) as device tensors; the codes are CODE_*."""
    import torch
    ctx = _ctx(context)
    n_pairs, cap = int(pairs.shape[0]), ctx.orb_capacity
    if tuple(pairs.shape) != (n_pairs, 2) or matches12.numel() < n_pairs * cap:
        raise ValueError("create_new_map_points_batch: pairs [n_pairs, 2] and matches12 [n_pairs, capacity] expected")
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride = _dev(kps, None, "kps"), _dev(counts, torch.int32, "counts"), int(img_stride)
    tb.uright, tb.Tcw = _dev(uright, torch.float32, "uright"), _dev(Tcw, torch.float32, "Tcw")
    tb.fx, tb.fy, tb.cx, tb.cy, tb.mbf = (float(v) for v in camera)
    if out is None:
        out = (_new((n_pairs, cap, 3), dtype=torch.float32), _new((n_pairs, cap), dtype=torch.uint8), _new((n_pairs,)))
    x3D, code, nnew = out
    _call_dev("olf_create_new_map_points_batch_dev", ctx, C.byref(tb), int(n_frames), _dev(depth, torch.float32, "depth"), float(mb), n_pairs,
              _dev(pairs, torch.int32, "pairs"), _dev(matches12, torch.int32, "matches12"), int(bool(monocular)), _dev(x3D, torch.float32, "x3D"),
              _dev(code, torch.uint8, "code"), _dev(nnew, torch.int32, "nnew"))
    return out


def CreateNewMapPoints(kps, counts, uright, depth, Tcw, camera, mb, scale_factors, pairs, matches12, monocular=False, img_stride=1):
    """The same from host arrays, no device: olf_create_new_map_points.  kps: KEYPOINT_DTYPE [n_frames * img_stride, capacity]; counts
    [n_frames * img_stride]; uright, depth [n_frames, capacity]; Tcw [n_frames, 4, 4]; scale_factors: mvScaleFactors.  Returns (x3D [n_pairs, capacity, 3],
    code [n_pairs, capacity], nnew [n_pairs], status) with status the bits 256 (octave) / 2048 (pair)."""
    kps = np.ascontiguousarray(kps, dtype=_lib.KEYPOINT_DTYPE)
    uright, depth = (np.ascontiguousarray(a, dtype=np.float32) for a in (uright, depth))
    Tcw = np.ascontiguousarray(Tcw, dtype=np.float32)
    n_frames, cap = uright.shape
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if kps.shape != (n_frames * img_stride, cap) or counts.shape[0] != n_frames * img_stride or depth.shape != uright.shape or Tcw.size != 16 * n_frames:
        raise ValueError("CreateNewMapPoints: kps [n_frames * img_stride, capacity], counts, uright / depth [n_frames, capacity], Tcw [n_frames, 4, 4] expected")
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    m12 = np.ascontiguousarray(matches12, dtype=np.int32)
    n_pairs = pairs.shape[0]
    if m12.shape != (n_pairs, cap):
        raise ValueError("CreateNewMapPoints: matches12 [n_pairs, capacity] expected")
    sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride, tb.uright, tb.Tcw = ptr(kps), ptr(counts), int(img_stride), ptr(uright), ptr(Tcw)
    tb.fx, tb.fy, tb.cx, tb.cy, tb.mbf = (float(v) for v in camera)
    x3D, code, nnew, status = np.zeros((n_pairs, cap, 3), np.float32), np.zeros((n_pairs, cap), np.uint8), np.zeros(n_pairs, np.int32), C.c_int32(0)
    _lib.check(lib().olf_create_new_map_points(C.byref(tb), cap, n_frames, ptr(depth), float(mb), ptr(sf), sf.shape[0], n_pairs, ptr(pairs), ptr(m12),
                                               int(bool(monocular)), ptr(x3D), ptr(code), ptr(nnew), C.addressof(status)), "olf_create_new_map_points")
    return x3D, code, nnew, int(status.value)


def update_normal_and_depth(graph, view, mp_world, mp_ref_kf, kf_Ow, normal, maxd, mind, points=None, n_points=None, context=None):
    """olf_update_normal_and_depth_dev on torch's current stream, without a synchronise.  graph / view: a MapGraph and its CullView (their device copies
    are made once) or an _lib.MapGraphC / _lib.CullViewC of device pointers; mp_world float32 [n_mp, 3], mp_ref_kf int32 [n_mp], kf_Ow float32 [n_kf, 3]:
    device tensors; points: int32 device tensor [n_points], or None for the points 0 .. n_points - 1 (n_points defaults to every point).  normal
    [n_mp, 3], maxd, mind [n_mp]: float32 device tensors, written in place for the listed points that are not bad and have observations.  mvScaleFactors
    are the context's.  Malformed indices are left out and reported by the context's next synchronize() / poll_status()."""
    import torch
    ctx = _ctx(context)
    g = _graph_dev(graph)
    v = view.c_dev() if isinstance(view, CullView) else view
    n = int(n_points) if n_points is not None else int(points.shape[0]) if points is not None else int(g.n_mp)
    f32, i32 = torch.float32, torch.int32
    _call_dev("olf_update_normal_and_depth_dev", ctx, C.byref(g), C.byref(v), n, _dev(points, i32, "points"), _dev(mp_world, f32, "mp_world"),
              _dev(mp_ref_kf, i32, "mp_ref_kf"), _dev(kf_Ow, f32, "kf_Ow"), _dev(normal, f32, "normal"), _dev(maxd, f32, "maxd"), _dev(mind, f32, "mind"))
    return normal, maxd, mind


def UpdateNormalAndDepth(graph, view, mp_world, mp_ref_kf, kf_Ow, scale_factors, normal=None, maxd=None, mind=None, points=None):
    """MapPoint::UpdateNormalAndDepth of the listed points (None: every point) from host arrays, no device: olf_update_normal_and_depth.  graph / view: a
    MapGraph and its CullView; scale_factors: mvScaleFactors.  normal [n_mp, 3], maxd, mind [n_mp]: the arrays as they stand (None: zeros); copies are
    changed and returned with the status bits (256 an octave outside the levels, 512 a point index, 4096 a key-frame index or slot): (normal, maxd,
    mind, status)."""
    n_mp, n_kf = graph.n_mp, graph.n_kf
    world = np.ascontiguousarray(mp_world, dtype=np.float32).reshape(-1)
    ref = np.ascontiguousarray(mp_ref_kf, dtype=np.int32).reshape(-1)
    Ow = np.ascontiguousarray(kf_Ow, dtype=np.float32).reshape(-1)
    sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
    if world.shape[0] != 3 * n_mp or ref.shape[0] != n_mp or Ow.shape[0] != 3 * n_kf:
        raise ValueError("UpdateNormalAndDepth: mp_world [n_mp, 3], mp_ref_kf [n_mp] and kf_Ow [n_kf, 3] expected")
    out = [np.zeros(s, np.float32) if a is None else np.array(a, dtype=np.float32).reshape(-1) for a, s in ((normal, 3 * n_mp), (maxd, n_mp), (mind, n_mp))]
    if [a.shape[0] for a in out] != [3 * n_mp, n_mp, n_mp]:
        raise ValueError("UpdateNormalAndDepth: normal [n_mp, 3], maxd [n_mp] and mind [n_mp] expected")
    lst = None if points is None else np.ascontiguousarray(points, dtype=np.int32).reshape(-1)
    n = n_mp if lst is None else lst.shape[0]
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)            # (an array without entries keeps an address)
    status = C.c_int32(0)
    g, v = graph.c(), view.c()
    _lib.check(lib().olf_update_normal_and_depth(C.byref(g), C.byref(v), n, ptr(lst), ptr(pad(world)), ptr(pad(ref)), ptr(pad(Ow)), ptr(sf), sf.shape[0],
                                                 ptr(pad(out[0])), ptr(pad(out[1])), ptr(pad(out[2])), C.addressof(status)), "olf_update_normal_and_depth")
    return out[0].reshape(n_mp, 3), out[1], out[2], int(status.value)
