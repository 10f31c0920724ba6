"""The key-frame step: which stereo features of a frame get a new map point or map line, in which order and with what geometry -- the loops of
Tracking::StereoInitialization (src/Tracking.cc:639-677), CreateNewKeyFrame (:1744-1865) and UpdateLastFrame (:1092-1204) -- and the decision of
Tracking::NeedNewKeyFrame (:1606-1725) (include/orbline.h; csrc/keyframe_batch.hip, keyframe_host.cpp, keyframe_terms.hpp).

  stereo_landmarks_batch     device tensors: the visit and creation lists, the new landmarks and the updated mvpMapPoints / mvpMapLines of every frame
  need_new_keyframe_batch    device tensors: the decision, the four counts and the six conditions of every frame
  StereoInitialization, CreateNewKeyFrame, UpdateLastFrame, NeedNewKeyFrame      host arrays, no device

The outputs are dicts keyed by the field names of olf_landmarks_outputs / olf_keyframe_test_outputs.  `created` goes into olf_track_batch.mp_valid and
`mp_world` into olf_track_batch.mp_world as they are (the temporal points of UpdateLastFrame)."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import lib, ptr
from .matcher import _call_dev, _ctx, _dev

LANDMARKS_INIT, LANDMARKS_KEYFRAME, LANDMARKS_LASTFRAME = 0, 1, 2
STATUS_NAN_DEPTH, STATUS_HELD_INDEX, STATUS_OCTAVE = 1, 2, 4         # a frame's status word of the landmark entries
STATUS_LDISP_RANGE = 1                                               # a row's status word of the key-frame test
ROW_FIELDS = ("mnId", "mnLastKeyFrameId", "mnLastRelocFrameId", "mMinFrames", "mMaxFrames", "nKFs", "bLocalMappingIdle", "KeyframesInQueue", "mbOnlyTracking",
              "stopped", "monocular")
COND_C1A, COND_C1B, COND_C1C, COND_C1C_L, COND_C2, COND_C2_L = (1 << k for k in range(6))


def keyframe_rows(rows):
    """rows of the tracker's scalars as the int32 array [n, 11] the key-frame test reads: a sequence of dicts keyed by ROW_FIELDS (missing: 0), or an array"""
    if len(rows) and isinstance(rows[0], dict):
        rows = [[int(r.get(k, 0)) for k in ROW_FIELDS] for r in rows]
    a = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).astype(np.uint32).view(np.int32) if len(rows) else np.zeros((0, len(ROW_FIELDS)), np.int32))
    if a.ndim != 2 or a.shape[1] != len(ROW_FIELDS):
        raise ValueError("keyframe rows: [n, 11] expected (ROW_FIELDS)")
    return a


def _landmark_shapes(n, cap, lcap):
    i32, u8, f32, f64 = np.int32, np.uint8, np.float32, np.float64
    return {"n_visited": ((n, 2), i32), "n_created": ((n, 2), i32), "visit_order": ((n, cap), i32), "visit_order_l": ((n, lcap), i32),
            "created_order": ((n, cap), i32), "created_order_l": ((n, lcap), i32), "created": ((n, cap), u8), "created_l": ((n, lcap), u8),
            "frame_mp_out": ((n, cap), i32), "frame_ml_out": ((n, lcap), i32), "mp_world": ((n, cap, 3), f32), "mp_normal": ((n, cap, 3), f32),
            "mp_maxd": ((n, cap), f32), "mp_mind": ((n, cap), f32), "ml_world_d": ((n, lcap, 6), f64), "ml_world": ((n, lcap, 6), f32), "status": ((n,), i32)}


def _test_shapes(n):
    return {"need": ((n,), np.uint8), "interrupt_ba": ((n,), np.uint8), "counts": ((n, 4), np.int32), "conditions": ((n,), np.int32), "status": ((n,), np.int32)}


def _torch_dtype(dt):
    import torch
    return {np.int32: torch.int32, np.uint8: torch.uint8, np.float32: torch.float32, np.float64: torch.float64}[dt]


def _dev_outputs(shapes, out, struct, skip=()):
    """the output tensors of a device entry (those of `out` where given, zeros otherwise) and the struct of their addresses"""
    import torch
    res, o = {}, struct()
    for name, (shape, dt) in shapes.items():
        if name in skip:
            continue
        t = out.get(name) if out else None
        if t is None:
            t = torch.zeros(shape, dtype=_torch_dtype(dt), device="cuda")
        if t.numel() < int(np.prod(shape)):
            raise ValueError(f"{name}: a tensor of shape {shape} expected")
        res[name] = t
        setattr(o, name, _dev(t, _torch_dtype(dt), name))
    return res, o


def stereo_landmarks_batch(n_frames, mode, kps, counts, kls, lcounts, depth, ldisp, Twc, camera, th_depth, frame_mp=None, frame_ml=None, mp_nobs=None,
                           ml_nobs=None, n_mp=0, n_ml=0, new_base_mp=None, new_base_ml=None, img_stride=2, double_lines=True, out=None, context=None):
    """olf_stereo_landmarks_batch_dev on torch's current stream, without a synchronise.  mode: LANDMARKS_INIT / _KEYFRAME / _LASTFRAME.  kps / counts and
    kls / lcounts in the extractors' layout (frame j = image j * img_stride); depth [n_frames, capacity] (mvDepth), ldisp [n_frames, line capacity, 2]
    (mvDisparity_l), Twc [n_frames, 4, 4] (rows of mRwc | mOw): device tensors; camera = (fx, fy, cx, cy, mbf); th_depth: mThDepth.  frame_mp / frame_ml:
    mvpMapPoints / mvpMapLines as int32 map indices (negative: NULL), or None: nothing is held; mp_nobs [n_mp], ml_nobs [n_ml]: Observations(); new_base_*
    int32 [n_frames]: the index of each frame's first new landmark (None: n_mp / n_ml).  out: a dict of tensors to write into.  Returns the dict of
    output tensors (olf_landmarks_outputs; ml_world_d only with double_lines)."""
    import torch
    ctx = _ctx(context)
    n, i32, f32 = int(n_frames), torch.int32, torch.float32
    b = _lib.LandmarksBatchC()
    b.kps, b.counts, b.kls, b.lcounts, b.img_stride = _dev(kps, None, "kps"), _dev(counts, i32, "counts"), _dev(kls, None, "kls"), _dev(lcounts, i32, "lcounts"), int(img_stride)
    b.depth, b.ldisp, b.Twc = _dev(depth, f32, "depth"), _dev(ldisp, f32, "ldisp"), _dev(Twc, f32, "Twc")
    b.frame_mp, b.frame_ml, b.mp_nobs, b.ml_nobs = _dev(frame_mp, i32, "frame_mp"), _dev(frame_ml, i32, "frame_ml"), _dev(mp_nobs, i32, "mp_nobs"), _dev(ml_nobs, i32, "ml_nobs")
    b.n_mp, b.n_ml = int(n_mp), int(n_ml)
    b.new_base_mp, b.new_base_ml = _dev(new_base_mp, i32, "new_base_mp"), _dev(new_base_ml, i32, "new_base_ml")
    b.fx, b.fy, b.cx, b.cy, b.mbf = (float(v) for v in camera)
    b.thDepth = float(th_depth)
    res, o = _dev_outputs(_landmark_shapes(n, ctx.orb_capacity, ctx.line_capacity), out, _lib.LandmarksOutputsC, () if double_lines else ("ml_world_d",))
    _call_dev("olf_stereo_landmarks_batch_dev", ctx, C.byref(b), n, int(mode), C.byref(o))
    return res


def _host_landmarks(mode, kps, counts, kls, lcounts, depth, ldisp, Twc, camera, th_depth, scale_factors, frame_mp=None, frame_ml=None, mp_nobs=None, ml_nobs=None,
                    new_base_mp=None, new_base_ml=None, img_stride=1):
    """olf_stereo_landmarks from host arrays, no device.  kps: KEYPOINT_DTYPE [n_frames * img_stride, capacity], kls: KEYLINE_DTYPE [n_frames * img_stride,
    line capacity], counts / lcounts [n_frames * img_stride]; the other arguments as stereo_landmarks_batch; scale_factors: mvScaleFactors.  Returns the
    dict of output arrays."""
    f32, i32 = np.float32, np.int32
    kps, kls = np.ascontiguousarray(kps, dtype=_lib.KEYPOINT_DTYPE), np.ascontiguousarray(kls, dtype=_lib.KEYLINE_DTYPE)
    depth, ldisp, Twc = (np.ascontiguousarray(a, dtype=f32) for a in (depth, ldisp, Twc))
    counts, lcounts = (np.ascontiguousarray(a, dtype=i32).reshape(-1) for a in (counts, lcounts))
    n, cap = depth.shape
    lcap = ldisp.shape[1] if ldisp.ndim == 3 else -1
    if (kps.shape != (n * img_stride, cap) or kls.shape != (n * img_stride, lcap) or ldisp.shape != (n, lcap, 2) or counts.shape[0] != n * img_stride or
            lcounts.shape[0] != n * img_stride or Twc.size != 16 * n):
        raise ValueError("stereo landmarks: kps [n * img_stride, capacity], kls [n * img_stride, line capacity], depth [n, capacity], ldisp [n, line capacity, 2], "
                         "Twc [n, 4, 4] expected")
    opt = lambda a, shape: None if a is None else np.ascontiguousarray(a, dtype=i32).reshape(shape)
    frame_mp, frame_ml, new_base_mp, new_base_ml = opt(frame_mp, (n, cap)), opt(frame_ml, (n, lcap)), opt(new_base_mp, (n,)), opt(new_base_ml, (n,))
    mp_nobs, ml_nobs = opt(mp_nobs, (-1,)), opt(ml_nobs, (-1,))
    sf = np.ascontiguousarray(scale_factors, dtype=f32).reshape(-1)
    b = _lib.LandmarksBatchC()
    b.kps, b.counts, b.kls, b.lcounts, b.img_stride = ptr(kps), ptr(counts), ptr(kls), ptr(lcounts), int(img_stride)
    b.depth, b.ldisp, b.Twc, b.frame_mp, b.frame_ml = ptr(depth), ptr(ldisp), ptr(Twc), ptr(frame_mp), ptr(frame_ml)
    b.n_mp, b.n_ml = (0 if a is None else a.shape[0] for a in (mp_nobs, ml_nobs))
    pad = lambda a: a if a is None or a.size else np.zeros(1, a.dtype)      # (an array without entries keeps an address)
    mp_nobs, ml_nobs = pad(mp_nobs), pad(ml_nobs)
    b.mp_nobs, b.ml_nobs = ptr(mp_nobs), ptr(ml_nobs)
    b.new_base_mp, b.new_base_ml = ptr(new_base_mp), ptr(new_base_ml)
    b.fx, b.fy, b.cx, b.cy, b.mbf = (float(v) for v in camera)
    b.thDepth = float(th_depth)
    res = {k: np.zeros(shape, dt) for k, (shape, dt) in _landmark_shapes(n, cap, lcap).items()}
    o = _lib.LandmarksOutputsC()
    for k, a in res.items():
        setattr(o, k, ptr(a if a.size else np.zeros(1, a.dtype)))
    _lib.check(lib().olf_stereo_landmarks(C.byref(b), cap, lcap, n, int(mode), ptr(sf), sf.shape[0], C.byref(o)), "olf_stereo_landmarks")
    return res


def StereoInitialization(*args, **kw):
    """The landmark loops of Tracking::StereoInitialization (src/Tracking.cc:639-677) from host arrays: see _host_landmarks for the arguments (kps, counts,
    kls, lcounts, depth, ldisp, Twc, camera, th_depth, scale_factors, ...)."""
    return _host_landmarks(LANDMARKS_INIT, *args, **kw)


def CreateNewKeyFrame(*args, **kw):
    """The landmark loops of Tracking::CreateNewKeyFrame (src/Tracking.cc:1744-1865) from host arrays; arguments as StereoInitialization."""
    return _host_landmarks(LANDMARKS_KEYFRAME, *args, **kw)


def UpdateLastFrame(*args, **kw):
    """The landmark loops of Tracking::UpdateLastFrame (src/Tracking.cc:1092-1204) from host arrays; arguments as StereoInitialization."""
    return _host_landmarks(LANDMARKS_LASTFRAME, *args, **kw)


def need_new_keyframe_batch(n_frames, counts, lcounts, depth, ldisp, rows, n_ref_matches, n_ref_matches_l, n_inliers, mbf, th_depth, frame_mp=None, outlier=None,
                            frame_ml=None, outlier_l=None, ldisp_frame=None, img_stride=2, out=None, context=None):
    """olf_need_new_keyframe_batch_dev on torch's current stream, without a synchronise.  counts / lcounts in the extractors' layout; depth [n_frames,
    capacity], ldisp [n_frames, line capacity, 2]; rows int32 [n_frames, 11] (keyframe_rows); n_ref_matches, n_ref_matches_l [n_frames] as
    tracked_map_points_batch returns them; n_inliers [n_frames, 2] as the pose optimisation returns it; frame_mp / frame_ml int32, outlier / outlier_l
    uint8 per frame, or None; ldisp_frame int32 [n_frames]: the frame whose disparities row j reads (None: j): device tensors.  Returns the dict of output
    tensors (olf_keyframe_test_outputs)."""
    import torch
    ctx = _ctx(context)
    n, i32, f32, u8 = int(n_frames), torch.int32, torch.float32, torch.uint8
    b = _lib.KeyFrameTestBatchC()
    b.counts, b.lcounts, b.img_stride = _dev(counts, i32, "counts"), _dev(lcounts, i32, "lcounts"), int(img_stride)
    b.depth, b.frame_mp, b.outlier = _dev(depth, f32, "depth"), _dev(frame_mp, i32, "frame_mp"), _dev(outlier, u8, "outlier")
    b.ldisp, b.frame_ml, b.outlier_l = _dev(ldisp, f32, "ldisp"), _dev(frame_ml, i32, "frame_ml"), _dev(outlier_l, u8, "outlier_l")
    b.ldisp_frame, b.rows = _dev(ldisp_frame, i32, "ldisp_frame"), _dev(rows, i32, "rows")
    b.n_ref_matches, b.n_ref_matches_l, b.n_inliers = _dev(n_ref_matches, i32, "n_ref_matches"), _dev(n_ref_matches_l, i32, "n_ref_matches_l"), _dev(n_inliers, i32, "n_inliers")
    b.mbf, b.thDepth = float(mbf), float(th_depth)
    res, o = _dev_outputs(_test_shapes(n), out, _lib.KeyFrameTestOutputsC)
    _call_dev("olf_need_new_keyframe_batch_dev", ctx, C.byref(b), n, C.byref(o))
    return res


def NeedNewKeyFrame(counts, lcounts, depth, ldisp, rows, n_ref_matches, n_ref_matches_l, n_inliers, mbf, th_depth, frame_mp=None, outlier=None, frame_ml=None,
                    outlier_l=None, ldisp_frame=None, img_stride=1):
    """Tracking::NeedNewKeyFrame (src/Tracking.cc:1606-1725) for every row from host arrays, no device: olf_need_new_keyframe.  Arguments as
    need_new_keyframe_batch; rows: keyframe_rows' input.  Returns the dict of output arrays."""
    f32, i32, u8 = np.float32, np.int32, np.uint8
    depth, ldisp = (np.ascontiguousarray(a, dtype=f32) for a in (depth, ldisp))
    n, cap = depth.shape
    lcap = ldisp.shape[1] if ldisp.ndim == 3 else -1
    counts, lcounts = (np.ascontiguousarray(a, dtype=i32).reshape(-1) for a in (counts, lcounts))
    rows = keyframe_rows(rows)
    nref, nref_l = (np.ascontiguousarray(a, dtype=i32).reshape(-1) for a in (n_ref_matches, n_ref_matches_l))
    ninl = np.ascontiguousarray(n_inliers, dtype=i32).reshape(-1)
    if (ldisp.shape != (n, lcap, 2) or counts.shape[0] != n * img_stride or lcounts.shape[0] != n * img_stride or rows.shape[0] != n or nref.shape[0] != n or
            nref_l.shape[0] != n or ninl.shape[0] != 2 * n):
        raise ValueError("NeedNewKeyFrame: depth [n, capacity], ldisp [n, line capacity, 2], rows [n, 11], n_ref_matches [n], n_inliers [n, 2] expected")
    opt = lambda a, dt, shape: None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(shape)
    frame_mp, frame_ml, ldisp_frame = opt(frame_mp, i32, (n, cap)), opt(frame_ml, i32, (n, lcap)), opt(ldisp_frame, i32, (n,))
    outlier, outlier_l = opt(outlier, u8, (n, cap)), opt(outlier_l, u8, (n, lcap))
    b = _lib.KeyFrameTestBatchC()
    b.counts, b.lcounts, b.img_stride = ptr(counts), ptr(lcounts), int(img_stride)
    b.depth, b.frame_mp, b.outlier, b.ldisp, b.frame_ml, b.outlier_l = ptr(depth), ptr(frame_mp), ptr(outlier), ptr(ldisp), ptr(frame_ml), ptr(outlier_l)
    b.ldisp_frame, b.rows, b.n_ref_matches, b.n_ref_matches_l, b.n_inliers = ptr(ldisp_frame), ptr(rows), ptr(nref), ptr(nref_l), ptr(ninl)
    b.mbf, b.thDepth = float(mbf), float(th_depth)
    res = {k: np.zeros(shape, dt) for k, (shape, dt) in _test_shapes(n).items()}
    o = _lib.KeyFrameTestOutputsC()
    for k, a in res.items():
        setattr(o, k, ptr(a if a.size else np.zeros(1, a.dtype)))
    _lib.check(lib().olf_need_new_keyframe(C.byref(b), cap, lcap, n, C.byref(o)), "olf_need_new_keyframe")
    return res
