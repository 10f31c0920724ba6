"""int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:2013-2208) as LoopClosing::ComputeSim3 calls it per
candidate (src/LoopClosing.cc:332), for a list of key-frame pairs: the olf_optimize_sim3* entries (include/orbline.h; csrc/optsim3_batch.hip,
optsim3_host.cpp, optsim3_api.cpp, optsim3_terms.hpp).

  optimize_sim3_state     the outputs of n pairs, zero-initialised: device tensors or host arrays
  optimize_sim3_batch     device tensors: every listed pair, on torch's current stream, without a synchronise
  OptimizeSim3            host arrays, no device: one pair
  optimize_sim3_pairs     host arrays, staged and run on the device
  optimize_sim3_jacobian  tests: the numeric Jacobian of one edge, as the host form computes it

The entry stands behind ORBmatcher's search_by_sim3 for pairs and takes what that took: the same pairs, the solver's best_s / best_R / best_t, and the
match rows it extended, which are changed in place (an outlier becomes -1).  Pair status bits: 1 a depth of exactly 0 at an evaluation, 2 H, b, step or
estimate not finite (either way S12_out is the input and n_inliers is 0), 4 a correspondence's octave is outside the levels (it was left out); the host
form adds 2048 for a refused pair."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import lib, ptr
from .sim3solver import _host_batch

ST_DEPTH, ST_NOT_FINITE, ST_OCTAVE, STATUS_PAIR = 1, 2, 4, 2048
_OUT = (("S12_out", np.float64, (8,)), ("s12_out", np.float32, ()), ("R12_out", np.float32, (9,)), ("t12_out", np.float32, (3,)), ("Scw_out", np.float32, (16,)),
        ("n_inliers", np.int32, ()), ("n_correspondences", np.int32, ()), ("n_bad_first", np.int32, ()), ("iters", np.int32, (2,)), ("status", np.int32, ()),
        ("chi2", np.float32, None))


def optimize_sim3_state(n_pairs, capacity, device=True):
    """The output arrays of olf_optimize_sim3_io for n_pairs pairs, all zero, as a dict: device tensors (device=True) or numpy arrays"""
    st = {}
    for name, dt, tail in _OUT:
        shape = (n_pairs,) + ((capacity, 2) if tail is None else tail)
        if device:
            import torch
            st[name] = torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
        else:
            st[name] = np.zeros(shape, dt)
    return st


def _io(matches12, st, address, row=None):
    io = _lib.OptSim3IoC()
    io.matches12 = address(matches12, "matches12")
    for name, _, _ in _OUT:
        setattr(io, name, address(st[name] if row is None else st[name][row], name))
    return io


def optimize_sim3_batch(n_frames, kps, counts, Tcw, mp_world, camera, pairs, matches12, s12, R12, t12, th2=10.0, fix_scale=False, row_active=None, mp_valid=None,
                        mp_bad=None, img_stride=2, out=None, context=None):
    """olf_optimize_sim3_pairs_dev on torch's current stream, without a synchronise.  kps / counts in the extractor's layout (frame j = image j * img_stride),
    Tcw [n_frames, 4, 4], mp_world [n_frames, capacity, 3], mp_valid / mp_bad [n_frames, capacity] (uint8, or None): device tensors; camera = (fx, fy, cx,
    cy); pairs int32 [n_pairs, 2]; matches12 int32 [n_pairs, capacity], changed in place; s12 [n_pairs], R12 [n_pairs, 9], t12 [n_pairs, 3] float32: the
    solver's best_s / best_R / best_t; row_active int32 [n_pairs] or None: the solver's accepted.  out: optimize_sim3_state(...) on the device (None: a new
    one).  Returns out: S12_out, s12_out, R12_out, t12_out, Scw_out, n_inliers (-1: the pair was left alone), n_correspondences, n_bad_first, iters, status,
    chi2."""
    import torch
    from .matcher import _call_dev, _ctx, _dev
    ctx = _ctx(context)
    n_pairs, cap = int(pairs.shape[0]), ctx.orb_capacity
    if tuple(pairs.shape) != (n_pairs, 2) or matches12.numel() < n_pairs * cap or s12.numel() < n_pairs or R12.numel() < 9 * n_pairs or t12.numel() < 3 * n_pairs:
        raise ValueError("optimize_sim3_batch: pairs [n_pairs, 2], matches12 [n_pairs, capacity], s12 [n_pairs], R12 [n_pairs, 9] and t12 [n_pairs, 3] expected")
    if out is None:
        out = optimize_sim3_state(n_pairs, cap)
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride = _dev(kps, None, "kps"), _dev(counts, torch.int32, "counts"), int(img_stride)
    tb.Tcw, tb.mp_world, tb.mp_valid = _dev(Tcw, torch.float32, "Tcw"), _dev(mp_world, torch.float32, "mp_world"), _dev(mp_valid, torch.uint8, "mp_valid")
    tb.fx, tb.fy, tb.cx, tb.cy = (float(v) for v in camera)
    io = _io(matches12, out, lambda a, name: _dev(a, None, name))
    _call_dev("olf_optimize_sim3_pairs_dev", ctx, C.byref(tb), int(n_frames), _dev(mp_bad, torch.uint8, "mp_bad"), n_pairs, _dev(pairs, torch.int32, "pairs"),
              _dev(s12, torch.float32, "s12"), _dev(R12, torch.float32, "R12"), _dev(t12, torch.float32, "t12"), float(th2), int(bool(fix_scale)),
              _dev(row_active, torch.int32, "row_active"), C.byref(io))
    return out


def _sim(s12, R12, t12, n):
    s = np.ascontiguousarray(s12, dtype=np.float32).reshape(-1)
    R = np.ascontiguousarray(R12, dtype=np.float32).reshape(-1)
    t = np.ascontiguousarray(t12, dtype=np.float32).reshape(-1)
    if s.shape[0] != n or R.shape[0] != 9 * n or t.shape[0] != 3 * n:
        raise ValueError("s12 [n_pairs], R12 [n_pairs, 9] and t12 [n_pairs, 3] expected")
    return s, R, t


def OptimizeSim3(kps, counts, Tcw, mp_world, camera, inv_level_sigma2, pair, matches12, s12, R12, t12, th2=10.0, fix_scale=False, mp_valid=None, mp_bad=None,
                 img_stride=1):
    """Optimizer::OptimizeSim3 for one pair from host arrays, no device: olf_optimize_sim3.  pair = (kf1, kf2); matches12 [capacity] int32, changed in
    place; s12, R12 [9], t12 [3]: the start; inv_level_sigma2: mvInvLevelSigma2.  Returns a dict of the outputs of optimize_sim3_state for this pair
    (scalars as Python numbers; status carries 2048 for a refused pair)."""
    tb, n_frames, cap, keep = _host_batch(kps, counts, Tcw, mp_world, camera, mp_valid, img_stride)
    if not (isinstance(matches12, np.ndarray) and matches12.dtype == np.int32 and matches12.flags.c_contiguous and matches12.size == cap):
        raise ValueError("OptimizeSim3: matches12, a contiguous int32 array [capacity] that is changed in place, expected")
    sig = np.ascontiguousarray(inv_level_sigma2, dtype=np.float32).reshape(-1)
    bad = None if mp_bad is None else np.ascontiguousarray(mp_bad, dtype=np.uint8)
    s, R, t = _sim(s12, R12, t12, 1)
    st = optimize_sim3_state(1, max(cap, 1), device=False)
    io = _io(matches12, st, lambda a, name: a.ctypes.data)
    _lib.check(lib().olf_optimize_sim3(C.byref(tb), cap, n_frames, ptr(bad), ptr(sig), sig.shape[0], int(pair[0]), int(pair[1]), float(s[0]), ptr(R), ptr(t),
                                       float(th2), int(bool(fix_scale)), C.byref(io)), "olf_optimize_sim3")
    return {name: (st[name][0].copy() if st[name][0].ndim else st[name][0].item()) for name, _, _ in _OUT}


def optimize_sim3_pairs(kps, counts, Tcw, mp_world, camera, pairs, matches12, s12, R12, t12, th2=10.0, fix_scale=False, row_active=None, mp_valid=None,
                        mp_bad=None, img_stride=1, out=None, context=None):
    """The batch from host arrays ON THE DEVICE: olf_optimize_sim3_pairs (stages, runs the kernel, synchronises).  Shapes as optimize_sim3_batch; matches12
    int32 [n_pairs, capacity], changed in place; out: optimize_sim3_state(..., device=False) (None: a new one).  A set status bit of the context raises
    OlfError with the outputs complete."""
    from .matcher import _ctx
    ctx = _ctx(context)
    tb, n_frames, cap, keep = _host_batch(kps, counts, Tcw, mp_world, camera, mp_valid, img_stride)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n_pairs = pairs.shape[0]
    if cap != ctx.orb_capacity or not (isinstance(matches12, np.ndarray) and matches12.dtype == np.int32 and matches12.flags.c_contiguous and
                                       matches12.shape == (n_pairs, cap)):
        raise ValueError("optimize_sim3_pairs: planes of the context's capacity and matches12, a contiguous int32 array [n_pairs, capacity], expected")
    bad = None if mp_bad is None else np.ascontiguousarray(mp_bad, dtype=np.uint8)
    act = None if row_active is None else np.ascontiguousarray(row_active, dtype=np.int32)
    s, R, t = _sim(s12, R12, t12, n_pairs)
    if out is None:
        out = optimize_sim3_state(n_pairs, cap, device=False)
    io = _io(matches12, out, lambda a, name: a.ctypes.data)
    _lib.check(lib().olf_optimize_sim3_pairs(ctx.handle, C.byref(tb), n_frames, ptr(bad), n_pairs, ptr(pairs), ptr(s), ptr(R), ptr(t), float(th2),
                                             int(bool(fix_scale)), ptr(act), C.byref(io)), "olf_optimize_sim3_pairs")
    return out


def optimize_sim3_jacobian(S12, camera, X, obs, inverse=False, fix_scale=False):
    """olf_debug_optimize_sim3_jacobian: the [2, 7] numeric Jacobian (base_binary_edge.hpp:176-200) of EdgeSim3ProjectXYZ (inverse=False, X = P2c) or
    EdgeInverseSim3ProjectXYZ (inverse=True, X = P1c) at the estimate S12 [8] = (qx, qy, qz, qw, t, s); camera = (fx, fy, cx, cy); obs [2]"""
    S = np.ascontiguousarray(S12, dtype=np.float64).reshape(8)
    cam = np.ascontiguousarray(camera, dtype=np.float64).reshape(-1)[:4].copy()
    X, obs = np.ascontiguousarray(X, dtype=np.float64).reshape(3), np.ascontiguousarray(obs, dtype=np.float64).reshape(2)
    J = np.zeros((2, 7))
    _lib.check(lib().olf_debug_optimize_sim3_jacobian(ptr(S), int(bool(fix_scale)), ptr(cam), ptr(X), ptr(obs), int(bool(inverse)), ptr(J)),
               "olf_debug_optimize_sim3_jacobian")
    return J
