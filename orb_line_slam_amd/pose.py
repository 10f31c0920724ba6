"""Optimizer::PoseOptimizationWithLine (src/Optimizer.cc:604-697) and the "discard outliers" loops after its three calls (src/Tracking.cc:1034-1074,
:1547-1590): the olf_pose_optimization_with_line* and olf_discard_outliers* entries (include/orbline.h; csrc/pose_batch.hip, pose_host.cpp, pose_terms.hpp).

  pose_params                          olf_pose_params with Config's defaults, fields overridden by keyword
  pose_optimization_with_line_batch    torch device tensors in, a dict of device tensors out, on torch's current stream, no synchronise
  PoseOptimizationWithLine             one frame, numpy in and out, on the device
  pose_optimization_with_line_host     one frame, numpy in and out, the host form: no context and no device
  discard_outliers_batch, DiscardOutliers, discard_outliers_host   the same three forms of the loops

Frame status bits (the `status` output): 1 a pass started without an active feature, 2 H, g or DT not finite (either way the pose went through unchanged),
4 a held feature's octave is outside the levels (it was left out)."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import KEYLINE_DTYPE, KEYPOINT_DTYPE, lib, ptr

ST_NO_FEATURE, ST_NOT_FINITE, ST_OCTAVE = 1, 2, 4
OUTPUTS = (("Tcw_out", np.float32, (16,)), ("DT", np.float64, (16,)), ("DT_cov", np.float64, (36,)), ("DT_cov_eig", np.float64, (6,)), ("err_norm", np.float64, ()),
           ("good", np.uint8, ()), ("n_inliers", np.int32, (2,)), ("iters", np.int32, (4,)), ("status", np.int32, ()))


def pose_params(**fields):
    """olf_pose_params: src/Config.cpp:42-82 (max_iters_ref 10, homog_th / min_error / min_error_change 1e-7, inlier_k 4, use_motion_model, has_points,
    has_lines 1), with the given fields replaced"""
    p = _lib.PoseParamsC()
    lib().olf_pose_default_params(C.byref(p))
    for k, v in fields.items():
        if not hasattr(p, k):
            raise TypeError(f"pose_params: no field {k}")
        setattr(p, k, v)
    return p


def _torch_dtype(t):
    import torch
    return {np.float32: torch.float32, np.float64: torch.float64, np.uint8: torch.uint8, np.int32: torch.int32}[t]


def pose_optimization_with_line_batch(kps, counts, kls, lcounts, img_stride, lle, Tcw, camera, frame_mp, mp_world, frame_ml, ml_world, n_frames=None, Tcw_prev=None,
                                      DT_cov_in=None, mp_index_offset=None, ml_index_offset=None, outlier=None, outlier_l=None, params=None, out=None, context=None):
    """olf_pose_optimization_with_line_batch_dev on torch's current stream, without a synchronise.  kps / counts / kls / lcounts per image in the extractor's
    layout (frame j = image j * img_stride); lle [n_frames, line capacity, 3] float64; Tcw (the prior), Tcw_prev (None: empty) [n_frames, 16] float32;
    DT_cov_in [n_frames, 36] float64 or None; camera = (fx, fy, cx, cy); frame_mp [n_frames, capacity] int32 indices into mp_world [n_mp, 3] float32
    (negative: none), mp_index_offset [n_frames] int32 or None -- e.g. the output of search_by_projection_batch with mp_world the last frames' planes
    viewed flat and offset j * capacity; the same triple for lines (ml_world [n_ml, 6]).  The two frame-to-frame outputs differ: search_by_projection_batch
    returns indices into the LAST frame's features (offset j * capacity), track_lines_batch returns the ids its caller gave the last frame's lines -- map
    indices, when those are the ids -- so its cur_ml goes in as frame_ml with ml_index_offset None, as the local-map searches' outputs do.  outlier /
    outlier_l: uint8 flags on entry or None (with has_points / has_lines = 0 they stay in force: removeOutliers never touches that kind).  Returns a dict
    of device tensors: Tcw_out, DT, DT_cov, DT_cov_eig, err_norm, good, outlier_out, outlier_l_out, n_inliers, iters, status (one row per frame);
    `out` may bring any of them, outlier_out / outlier_l_out may be the inputs themselves."""
    import torch
    from .matcher import _call_dev, _ctx, _dev, _new
    ctx = _ctx(context)
    n = int(n_frames) if n_frames is not None else int(Tcw.shape[0])
    cap, lcap = ctx.orb_capacity, ctx.line_capacity
    f32, f64, i32, u8 = torch.float32, torch.float64, torch.int32, torch.uint8
    b = _lib.PoseBatchC()
    b.kps, b.counts, b.kls, b.lcounts, b.img_stride = _dev(kps, None, "kps"), _dev(counts, i32, "counts"), _dev(kls, None, "kls"), _dev(lcounts, i32, "lcounts"), int(img_stride)
    b.lle, b.Tcw, b.Tcw_prev, b.DT_cov_in = _dev(lle, f64, "lle"), _dev(Tcw, f32, "Tcw"), _dev(Tcw_prev, f32, "Tcw_prev"), _dev(DT_cov_in, f64, "DT_cov_in")
    b.fx, b.fy, b.cx, b.cy = (float(v) for v in camera)
    b.frame_mp, b.mp_index_offset, b.mp_world = _dev(frame_mp, i32, "frame_mp"), _dev(mp_index_offset, i32, "mp_index_offset"), _dev(mp_world, f32, "mp_world")
    b.frame_ml, b.ml_index_offset, b.ml_world = _dev(frame_ml, i32, "frame_ml"), _dev(ml_index_offset, i32, "ml_index_offset"), _dev(ml_world, f32, "ml_world")
    b.n_mp = 0 if mp_world is None else int(mp_world.numel() // 3)
    b.n_ml = 0 if ml_world is None else int(ml_world.numel() // 6)
    b.outlier, b.outlier_l = _dev(outlier, u8, "outlier"), _dev(outlier_l, u8, "outlier_l")
    if out is None:
        out = {}
    for name, t, shape in OUTPUTS:
        out.setdefault(name, _new((n,) + shape, dtype=_torch_dtype(t)))
    out.setdefault("outlier_out", _new((n, cap), dtype=u8))
    out.setdefault("outlier_l_out", _new((n, lcap), dtype=u8))
    o = _lib.PoseOutputsC()
    for name, t, _ in OUTPUTS:
        setattr(o, name, _dev(out[name], _torch_dtype(t), name))
    o.outlier_out, o.outlier_l_out = _dev(out["outlier_out"], u8, "outlier_out"), _dev(out["outlier_l_out"], u8, "outlier_l_out")
    p = params if params is not None else pose_params()
    _call_dev("olf_pose_optimization_with_line_batch_dev", ctx, C.byref(b), n, C.byref(p), C.byref(o))
    return out


def _rows(keys, keylines, lle, frame_mp, frame_ml, outlier, outlier_l, cap, lcap, who):
    """one frame's host arrays as rows of the given capacities (None: the arrays' own lengths)"""
    keys = np.ascontiguousarray(keys, dtype=KEYPOINT_DTYPE).reshape(-1)
    keylines = np.ascontiguousarray(keylines, dtype=KEYLINE_DTYPE).reshape(-1)
    n, nl = keys.shape[0], keylines.shape[0]
    cap, lcap = (n if cap is None else cap), (nl if lcap is None else lcap)
    if n > cap or nl > lcap:
        raise ValueError(f"{who}: {n} key points / {nl} key lines exceed the capacities {cap} / {lcap}")

    def row(a, m, length, dtype, fill, tail=()):
        r = np.full((max(length, 1),) + tail, fill, dtype)
        if a is not None:
            a = np.asarray(a, dtype=dtype).reshape((-1,) + tail)
            if a.shape[0] != m:
                raise ValueError(f"{who}: one entry per feature expected")
            r[:m] = a
        return r

    kp, kl = np.zeros(max(cap, 1), KEYPOINT_DTYPE), np.zeros(max(lcap, 1), KEYLINE_DTYPE)
    kp[:n], kl[:nl] = keys, keylines
    return dict(n=n, nl=nl, cap=cap, lcap=lcap, kps=kp, kls=kl, lle=row(lle, nl, lcap, np.float64, 0.0, (3,)), frame_mp=row(frame_mp, n, cap, np.int32, -1),
                frame_ml=row(frame_ml, nl, lcap, np.int32, -1), outlier=row(outlier, n, cap, np.uint8, 0), outlier_l=row(outlier_l, nl, lcap, np.uint8, 0))


def _maps(mp_world, ml_world):
    mpw = np.ascontiguousarray(mp_world if mp_world is not None else np.zeros((0, 3)), dtype=np.float32).reshape(-1, 3)
    mlw = np.ascontiguousarray(ml_world if ml_world is not None else np.zeros((0, 6)), dtype=np.float32).reshape(-1, 6)
    return mpw, mlw


def _mat(a, n, dtype, who):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"{who}: {n} entries expected")
    return a


def _frame_result(out, r):
    res = {name: out[name].reshape(shape).copy() if shape else out[name].reshape(-1)[0].item() for name, _, shape in OUTPUTS}
    res["outlier_out"], res["outlier_l_out"] = out["outlier_out"].reshape(-1)[:r["n"]].copy(), out["outlier_l_out"].reshape(-1)[:r["nl"]].copy()
    return res


def pose_optimization_with_line_host(keys, keylines, lle, Tcw, camera, frame_mp, mp_world, frame_ml, ml_world, inv_level_sigma2, Tcw_prev=None, DT_cov_in=None,
                                     mp_index_offset=0, ml_index_offset=0, outlier=None, outlier_l=None, params=None, capacity=None, line_capacity=None):
    """olf_pose_optimization_with_line: one frame on the host, no context and no device.  keys / keylines: KEYPOINT_DTYPE / KEYLINE_DTYPE arrays (mvKeysUn,
    mvKeysUn_Line); lle [N_l, 3] (mvle_l); Tcw, Tcw_prev (None: empty): 4 x 4; frame_mp [N] / frame_ml [N_l]: indices into mp_world [n_mp, 3] / ml_world
    [n_ml, 6], negative = none; inv_level_sigma2: mvInvLevelSigma2.  Returns a dict of Tcw_out [16], DT [16], DT_cov [36], DT_cov_eig [6], err_norm, good,
    outlier_out [N], outlier_l_out [N_l], n_inliers [2], iters [4], status (the bits 512 / 1024 of a context go into it here)."""
    who = "pose_optimization_with_line_host"
    r = _rows(keys, keylines, lle, frame_mp, frame_ml, outlier, outlier_l, capacity, line_capacity, who)
    mpw, mlw = _maps(mp_world, ml_world)
    sig = np.ascontiguousarray(inv_level_sigma2, dtype=np.float32).reshape(-1)
    T, Tp, cov = _mat(Tcw, 16, np.float32, who), _mat(Tcw_prev, 16, np.float32, who), _mat(DT_cov_in, 36, np.float64, who)
    counts, lcounts = np.array([r["n"]], np.int32), np.array([r["nl"]], np.int32)
    offs, offl = np.array([mp_index_offset], np.int32), np.array([ml_index_offset], np.int32)
    b = _lib.PoseBatchC()
    b.kps, b.counts, b.kls, b.lcounts, b.img_stride = ptr(r["kps"]), ptr(counts), ptr(r["kls"]), ptr(lcounts), 1
    b.lle, b.Tcw, b.Tcw_prev, b.DT_cov_in = ptr(r["lle"]), ptr(T), ptr(Tp), ptr(cov)
    b.fx, b.fy, b.cx, b.cy = (float(v) for v in camera)
    b.frame_mp, b.mp_index_offset, b.mp_world, b.n_mp = ptr(r["frame_mp"]), ptr(offs), ptr(mpw) if mpw.shape[0] else None, mpw.shape[0]
    b.frame_ml, b.ml_index_offset, b.ml_world, b.n_ml = ptr(r["frame_ml"]), ptr(offl), ptr(mlw) if mlw.shape[0] else None, mlw.shape[0]
    b.outlier, b.outlier_l = ptr(r["outlier"]), ptr(r["outlier_l"])
    out = {name: np.zeros((1,) + shape, t) for name, t, shape in OUTPUTS}
    out["outlier_out"], out["outlier_l_out"] = np.zeros(max(r["cap"], 1), np.uint8), np.zeros(max(r["lcap"], 1), np.uint8)
    o = _lib.PoseOutputsC()
    for name in out:
        setattr(o, name, ptr(out[name]))
    p = params if params is not None else pose_params()
    _lib.check(lib().olf_pose_optimization_with_line(C.byref(b), r["cap"], r["lcap"], ptr(sig), sig.shape[0], C.byref(p), C.byref(o)), "olf_pose_optimization_with_line")
    return _frame_result(out, r)


def PoseOptimizationWithLine(keys, keylines, lle, Tcw, camera, frame_mp, mp_world, frame_ml, ml_world, Tcw_prev=None, DT_cov_in=None, mp_index_offset=0,
                             ml_index_offset=0, outlier=None, outlier_l=None, params=None, context=None):
    """Optimizer::PoseOptimizationWithLine for one frame from host arrays, on the device (a batch of one); arguments and result as
    pose_optimization_with_line_host, the level table being the context's.  The context's next synchronize() / poll_status() reports indices outside the maps."""
    import torch
    from .matcher import _ctx
    who = "PoseOptimizationWithLine"
    ctx = _ctx(context)
    r = _rows(keys, keylines, lle, frame_mp, frame_ml, outlier, outlier_l, ctx.orb_capacity, ctx.line_capacity, who)
    mpw, mlw = _maps(mp_world, ml_world)
    dev = lambda a: torch.from_numpy(a).cuda()
    raw = lambda a: dev(np.ascontiguousarray(a).view(np.uint8).reshape(-1))
    opt = lambda a, n, t: None if a is None else dev(_mat(a, n, t, who).reshape(1, n))
    pad = lambda a: a if a.shape[0] else np.zeros((1,) + a.shape[1:], a.dtype)
    out = pose_optimization_with_line_batch(raw(r["kps"]), dev(np.array([r["n"]], np.int32)), raw(r["kls"]), dev(np.array([r["nl"]], np.int32)), 1, dev(r["lle"][None]),
                                            opt(Tcw, 16, np.float32), camera, dev(r["frame_mp"][None]), dev(pad(mpw)) if mpw.shape[0] else None, dev(r["frame_ml"][None]),
                                            dev(pad(mlw)) if mlw.shape[0] else None, 1, opt(Tcw_prev, 16, np.float32), opt(DT_cov_in, 36, np.float64),
                                            dev(np.array([mp_index_offset], np.int32)), dev(np.array([ml_index_offset], np.int32)), dev(r["outlier"][None]),
                                            dev(r["outlier_l"][None]), params, None, ctx)
    return _frame_result({k: v.cpu().numpy() for k, v in out.items()}, r)


def _discard_c(counts, lcounts, img_stride, frame_mp, frame_ml, outlier, outlier_l, mp_index_offset, ml_index_offset, mp_obs, ml_obs, n_mp, n_ml, conv):
    d = _lib.DiscardBatchC()
    d.counts, d.lcounts, d.img_stride = conv(counts), conv(lcounts), int(img_stride)
    d.frame_mp, d.frame_ml, d.outlier, d.outlier_l = conv(frame_mp), conv(frame_ml), conv(outlier), conv(outlier_l)
    d.mp_index_offset, d.ml_index_offset, d.mp_obs, d.ml_obs = conv(mp_index_offset), conv(ml_index_offset), conv(mp_obs), conv(ml_obs)
    d.n_mp, d.n_ml = int(n_mp), int(n_ml)
    return d


def discard_outliers_batch(counts, lcounts, img_stride, frame_mp, frame_ml, outlier, outlier_l, n_mp, n_ml, mode, only_tracking=False, stereo=True, mp_obs=None,
                           ml_obs=None, mp_index_offset=None, ml_index_offset=None, out=None, context=None):
    """olf_discard_outliers_batch_dev on torch's current stream, without a synchronise: the loops after Optimizer::PoseOptimizationWithLine for every frame.
    frame_mp / frame_ml (int32) and outlier / outlier_l (uint8) [n_frames, capacity] are changed in place; mp_obs [n_mp] / ml_obs [n_ml] uint8:
    Observations() > 0 (None: all).  mode 0: src/Tracking.cc:1034-1074; mode 1: :1547-1590 with only_tracking (mbOnlyTracking) and stereo
    (mSensor == System::STEREO).  Returns the int32 device tensor n_matches [n_frames, 2]: points, lines."""
    import torch
    from .matcher import _call_dev, _ctx, _dev, _new
    ctx = _ctx(context)
    n = int(frame_mp.shape[0])
    if out is None:
        out = _new((n, 2))
    d = _discard_c(counts, lcounts, img_stride, frame_mp, frame_ml, outlier, outlier_l, mp_index_offset, ml_index_offset, mp_obs, ml_obs, n_mp, n_ml, lambda a: _dev(a))
    _call_dev("olf_discard_outliers_batch_dev", ctx, C.byref(d), n, int(mode), int(bool(only_tracking)), int(bool(stereo)), _dev(out, torch.int32, "n_matches"))
    return out


def _discard_rows(frame_mp, frame_ml, outlier, outlier_l, mp_obs, ml_obs):
    fmp, fml = np.array(frame_mp, dtype=np.int32).reshape(-1), np.array(frame_ml, dtype=np.int32).reshape(-1)
    o, ol = np.array(outlier, dtype=np.uint8).reshape(-1), np.array(outlier_l, dtype=np.uint8).reshape(-1)
    if o.shape != fmp.shape or ol.shape != fml.shape:
        raise ValueError("discard outliers: one flag per feature expected")
    obs = None if mp_obs is None else np.ascontiguousarray(mp_obs, dtype=np.uint8).reshape(-1)
    lobs = None if ml_obs is None else np.ascontiguousarray(ml_obs, dtype=np.uint8).reshape(-1)
    return fmp, fml, o, ol, obs, lobs


def discard_outliers_host(frame_mp, frame_ml, outlier, outlier_l, n_mp, n_ml, mode, only_tracking=False, stereo=True, mp_obs=None, ml_obs=None, mp_index_offset=0,
                          ml_index_offset=0):
    """olf_discard_outliers: the loops for one frame on the host, no context.  Returns a dict of frame_mp, frame_ml, outlier, outlier_l (the changed copies),
    n_matches [2] and status (bits 512 / 1024: an index outside the map was left alone)."""
    fmp, fml, o, ol, obs, lobs = _discard_rows(frame_mp, frame_ml, outlier, outlier_l, mp_obs, ml_obs)
    counts, lcounts = np.array([fmp.shape[0]], np.int32), np.array([fml.shape[0]], np.int32)
    offs, offl = np.array([mp_index_offset], np.int32), np.array([ml_index_offset], np.int32)
    pad = lambda a: a if a.shape[0] else np.zeros(1, a.dtype)
    keep = [pad(fmp), pad(fml), pad(o), pad(ol)]
    d = _discard_c(counts, lcounts, 1, keep[0], keep[1], keep[2], keep[3], offs, offl, obs, lobs, n_mp, n_ml, ptr)
    nm, st = np.zeros(2, np.int32), np.zeros(1, np.int32)
    _lib.check(lib().olf_discard_outliers(C.byref(d), fmp.shape[0], fml.shape[0], int(mode), int(bool(only_tracking)), int(bool(stereo)), ptr(nm), ptr(st)),
               "olf_discard_outliers")
    return dict(frame_mp=keep[0][:fmp.shape[0]], frame_ml=keep[1][:fml.shape[0]], outlier=keep[2][:fmp.shape[0]], outlier_l=keep[3][:fml.shape[0]], n_matches=nm,
                status=int(st[0]))


def DiscardOutliers(frame_mp, frame_ml, outlier, outlier_l, n_mp, n_ml, mode, only_tracking=False, stereo=True, mp_obs=None, ml_obs=None, mp_index_offset=0,
                    ml_index_offset=0, context=None):
    """the loops for one frame from host arrays, on the device (a batch of one); result as discard_outliers_host without `status`: the context's next
    synchronize() / poll_status() reports indices outside the maps"""
    import torch
    from .matcher import _ctx
    ctx = _ctx(context)
    fmp, fml, o, ol, obs, lobs = _discard_rows(frame_mp, frame_ml, outlier, outlier_l, mp_obs, ml_obs)
    if fmp.shape[0] > ctx.orb_capacity or fml.shape[0] > ctx.line_capacity:
        raise ValueError("DiscardOutliers: more features than the context's capacities")

    def row(a, cap, fill):
        r = np.full((1, cap), fill, a.dtype)
        r[0, :a.shape[0]] = a
        return torch.from_numpy(r).cuda()

    dev = lambda a: None if a is None else torch.from_numpy(a if a.shape[0] else np.zeros(1, a.dtype)).cuda()
    t = [row(fmp, ctx.orb_capacity, -1), row(fml, ctx.line_capacity, -1), row(o, ctx.orb_capacity, 0), row(ol, ctx.line_capacity, 0)]
    nm = discard_outliers_batch(dev(np.array([fmp.shape[0]], np.int32)), dev(np.array([fml.shape[0]], np.int32)), 1, t[0], t[1], t[2], t[3], n_mp, n_ml, mode, only_tracking,
                                stereo, dev(obs), dev(lobs), dev(np.array([mp_index_offset], np.int32)), dev(np.array([ml_index_offset], np.int32)), None, ctx)
    h = [x.cpu().numpy()[0] for x in t]
    return dict(frame_mp=h[0][:fmp.shape[0]], frame_ml=h[1][:fml.shape[0]], outlier=h[2][:fmp.shape[0]], outlier_l=h[3][:fml.shape[0]], n_matches=nm.cpu().numpy()[0])
