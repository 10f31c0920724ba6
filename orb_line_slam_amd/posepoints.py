"""int Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:239-451): the olf_pose_optimization* entries (include/orbline.h; csrc/posepoints_batch.hip,
posepoints_host.cpp, posepoints_terms.hpp).

  pose_optimization_batch    torch device tensors in, a dict of device tensors out, on torch's current stream, no synchronise
  PoseOptimization           one frame, numpy in and out, on the device through the host-pointer form
  pose_optimization_host     one frame, numpy in and out, the host form: no context and no device

Row status bits (the `status` output): 1 a held point at depth 0, 2 H, b, step or estimate not finite (either way the pose went through unchanged and
n_good is 0), 4 a held feature's octave is outside the levels (it was left out).  The loops that follow a call are discard_outliers_* of pose.py (mode 0
after the tracker's calls, mode 1 with stereo=True in relocalisation), with zero line counts."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import KEYPOINT_DTYPE, lib, ptr

ST_DEPTH, ST_NOT_FINITE, ST_OCTAVE = 1, 2, 4
OUTPUTS = (("Tcw_out", np.float32, (16,)), ("n_good", np.int32, ()), ("n_initial", np.int32, ()), ("passes", np.int32, ()), ("iters", np.int32, (4,)),
           ("status", np.int32, ()))
ROWS = (("outlier_out", np.uint8), ("chi2", np.float32))


def pose_optimization_batch(kps, counts, img_stride, uright, camera, Tcw, frame_mp, mp_world, n_frames=None, mp_index_offset=None, pairs=None, row_active=None,
                            out=None, context=None, n_rows=None):
    """olf_pose_optimization_batch_dev on torch's current stream, without a synchronise.  kps / counts per image in the extractor's layout (frame j = image
    j * img_stride); uright [n_frames, capacity] float32; camera = (fx, fy, cx, cy, mbf); Tcw [n_rows, 16] float32; frame_mp [n_rows, capacity] int32 indices
    into mp_world [n_mp, 3] float32 (negative: none); mp_index_offset [n_rows] int32 or None.  Without pairs row r reads frame r; with pairs [n_rows, 2] =
    (key frame, frame) row r reads frame pairs[r, 1] and its indices are relative to key frame pairs[r, 0]'s plane of mp_world [n_frames, capacity, 3]:
    Tcw, frame_mp and row_active are then pnp_solver_batch's Tcw, pnp_apply_inliers' out and the solver's accepted.  Returns a dict of device tensors,
    one row per row: Tcw_out, outlier_out, n_good (-1: the row was left alone), n_initial, chi2, passes, iters, status; `out` may bring any of them.
    n_rows: the number of rows when Tcw is longer."""
    import torch
    from .matcher import _call_dev, _ctx, _dev, _new
    from .pose import _torch_dtype
    ctx = _ctx(context)
    n_rows = int(Tcw.shape[0]) if n_rows is None else int(n_rows)
    n_frames = int(n_frames) if n_frames is not None else int(uright.shape[0])
    f32, i32 = torch.float32, torch.int32
    b = _lib.PosePointsBatchC()
    b.kps, b.counts, b.img_stride, b.uright = _dev(kps, None, "kps"), _dev(counts, i32, "counts"), int(img_stride), _dev(uright, f32, "uright")
    b.fx, b.fy, b.cx, b.cy, b.bf = (float(v) for v in camera)
    b.Tcw, b.frame_mp, b.mp_world = _dev(Tcw, f32, "Tcw"), _dev(frame_mp, i32, "frame_mp"), _dev(mp_world, f32, "mp_world")
    b.n_mp = 0 if mp_world is None else int(mp_world.numel() // 3)
    b.mp_index_offset, b.pairs, b.row_active = _dev(mp_index_offset, i32, "mp_index_offset"), _dev(pairs, i32, "pairs"), _dev(row_active, i32, "row_active")
    if out is None:
        out = {}
    for name, t, shape in OUTPUTS:
        out.setdefault(name, _new((n_rows,) + shape, dtype=_torch_dtype(t)))
    for name, t in ROWS:
        out.setdefault(name, _new((n_rows, ctx.orb_capacity), dtype=_torch_dtype(t)))
    o = _lib.PosePointsOutputsC()
    for name, t in [(n, t) for n, t, _ in OUTPUTS] + list(ROWS):
        setattr(o, name, _dev(out[name], _torch_dtype(t), name))
    _call_dev("olf_pose_optimization_batch_dev", ctx, C.byref(b), n_rows, n_frames, C.byref(o))
    return out


def _frame(keys, uright, Tcw, frame_mp, mp_world, cap, who):
    keys = np.ascontiguousarray(keys, dtype=KEYPOINT_DTYPE).reshape(-1)
    n = keys.shape[0]
    cap = n if cap is None else cap
    if n > cap:
        raise ValueError(f"{who}: {n} key points exceed the capacity {cap}")
    kp, ur, fmp = np.zeros(max(cap, 1), KEYPOINT_DTYPE), np.full(max(cap, 1), -1.0, np.float32), np.full(max(cap, 1), -1, np.int32)
    kp[:n], ur[:n], fmp[:n] = keys, np.asarray(uright, np.float32).reshape(-1), np.asarray(frame_mp, np.int32).reshape(-1)
    mpw = np.ascontiguousarray(mp_world if mp_world is not None else np.zeros((0, 3)), dtype=np.float32).reshape(-1, 3)
    T = np.ascontiguousarray(Tcw, dtype=np.float32).reshape(-1)
    if T.shape[0] != 16:
        raise ValueError(f"{who}: Tcw is a 4 x 4 matrix")
    return n, cap, kp, ur, fmp, mpw, T


def _one_row(call, who, keys, uright, Tcw, camera, frame_mp, mp_world, mp_index_offset, cap):
    n, cap, kp, ur, fmp, mpw, T = _frame(keys, uright, Tcw, frame_mp, mp_world, cap, who)
    counts, offs = np.array([n], np.int32), np.array([mp_index_offset], np.int32)
    b = _lib.PosePointsBatchC()
    b.kps, b.counts, b.img_stride, b.uright = ptr(kp), ptr(counts), 1, ptr(ur)
    b.fx, b.fy, b.cx, b.cy, b.bf = (float(v) for v in camera)
    b.Tcw, b.frame_mp, b.mp_world, b.n_mp, b.mp_index_offset = ptr(T), ptr(fmp), ptr(mpw) if mpw.shape[0] else None, mpw.shape[0], ptr(offs)
    out = {name: np.zeros((1,) + shape, t) for name, t, shape in OUTPUTS}
    for name, t in ROWS:
        out[name] = np.zeros(max(cap, 1), t)
    o = _lib.PosePointsOutputsC()
    for name in out:
        setattr(o, name, ptr(out[name]))
    call(b, cap, o)
    res = {name: out[name].reshape(shape).copy() if shape else out[name].reshape(-1)[0].item() for name, _, shape in OUTPUTS}
    for name, _ in ROWS:
        res[name] = out[name][:n].copy()
    return res


def pose_optimization_host(keys, uright, Tcw, camera, frame_mp, mp_world, inv_level_sigma2, mp_index_offset=0, capacity=None):
    """olf_pose_optimization: one frame on the host, no context and no device.  keys: KEYPOINT_DTYPE (mvKeysUn); uright [N] (mvuRight, negative: monocular);
    Tcw 4 x 4; camera = (fx, fy, cx, cy, mbf); frame_mp [N]: indices into mp_world [n_mp, 3], negative = none; inv_level_sigma2: mvInvLevelSigma2.  Returns a
    dict of Tcw_out [16], outlier_out [N], n_good, n_initial, chi2 [N], passes, iters [4], status (bit 512 of a context goes into it here)."""
    sig = np.ascontiguousarray(inv_level_sigma2, dtype=np.float32).reshape(-1)
    call = lambda b, cap, o: _lib.check(lib().olf_pose_optimization(C.byref(b), cap, 1, ptr(sig), sig.shape[0], C.byref(o)), "olf_pose_optimization")
    return _one_row(call, "pose_optimization_host", keys, uright, Tcw, camera, frame_mp, mp_world, mp_index_offset, capacity)


def PoseOptimization(keys, uright, Tcw, camera, frame_mp, mp_world, mp_index_offset=0, context=None):
    """Optimizer::PoseOptimization for one frame from host arrays, on the device (olf_pose_optimization_rows, one row); arguments and result as
    pose_optimization_host, the level table being the context's"""
    from .matcher import _ctx
    ctx = _ctx(context)
    call = lambda b, cap, o: _lib.check(lib().olf_pose_optimization_rows(ctx.handle, C.byref(b), 1, 1, C.byref(o)), "olf_pose_optimization_rows")
    return _one_row(call, "PoseOptimization", keys, uright, Tcw, camera, frame_mp, mp_world, mp_index_offset, ctx.orb_capacity)
