"""Initializer::Initialize (src/Initializer.cc:44-121) as Tracking::MonocularInitialization drives it (src/Tracking.cc:722, :756-772), for a list of
(reference frame, current frame) pairs (include/orbline.h; csrc/initializer_batch.hip, initializer_host.cpp, initializer_api.cpp, initializer_terms.hpp).

  initializer_params      olf_initializer_params: sigma, max_iterations, min_parallax, min_triangulated (the tracker's 1.0, 200, 1.0, 50)
  initializer_state       the outputs of n pairs, zero-initialised: device tensors or host arrays
  initializer_batch       device tensors: Initialize of every listed pair, without a synchronise
  initializer_apply       device tensors: what the tracker does with a successful initialisation (:758-772)
  Initialize              host arrays, no device: one pair
  initializer_pairs       host arrays, staged and run on the device
  initializer_draws       the random stream of C.20 for tests and tools: uint32 values below 2^31
  parallax_degrees        the degrees of a stored cos_parallax (C.34: the library stores cosines and compares cosines)

The random stream is the caller's: draws [n_pairs, max_iterations, 8].  The matches rows are exactly what search_for_initialization
writes."""
import ctypes as C
import numpy as np
from . import _lib, _ransac
from ._lib import lib, ptr
from .matcher import _call_dev, _ctx, _dev

STATUS_PAIR, STATUS_DEGENERATE, STATUS_NAN = 2048, 32768, 65536

# (name, dtype, tail): tail is the shape behind [n_pairs], or None for a row of the capacity
_STATE = (("ok", np.int32, ()), ("n_correspondences", np.int32, ()), ("model", np.int32, ()), ("score_H", np.float32, ()), ("score_F", np.float32, ()),
          ("H21", np.float32, (9,)), ("F21", np.float32, (9,)), ("inliers_H", np.uint8, None), ("inliers_F", np.uint8, None), ("R21", np.float32, (9,)),
          ("t21", np.float32, (3,)), ("P3D", np.float32, "p3d"), ("triangulated", np.uint8, None), ("n_good", np.int32, (8,)),
          ("cos_parallax", np.float32, (8,)), ("hypothesis", np.int32, ()))


def initializer_params(sigma=1.0, max_iterations=200, min_parallax=1.0, min_triangulated=50):
    """olf_initializer_params; the defaults are the tracker's (src/Tracking.cc:722, src/Initializer.cc:116-118)"""
    p = _lib.InitializerParamsC()
    p.sigma, p.max_iterations, p.min_parallax, p.min_triangulated = float(sigma), int(max_iterations), float(min_parallax), int(min_triangulated)
    return p


def initializer_state(n_pairs, capacity, device=True):
    """The arrays of olf_initializer_io for n_pairs pairs, all zero, as a dict: device tensors (device=True) or numpy arrays"""
    st = {}
    for name, dt, tail in _STATE:
        shape = (n_pairs,) + ((capacity,) if tail is None else (capacity, 3) if tail == "p3d" else tail)
        if device:
            import torch
            st[name] = torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
        else:
            st[name] = np.zeros(shape, dt)
    return st


def _io(st, address, row=None):
    return _ransac.io_block(_lib.InitializerIoC, _STATE, st, address, row)


def initializer_draws(n_pairs, max_iterations, seed):
    """[n_pairs, max_iterations, 8] uint32 values below 2^31, as rand() returns them"""
    return _ransac.draws(n_pairs, max_iterations, 8, seed)


def parallax_degrees(cos_parallax):
    """acos(c) * 180 / CV_PI as CheckRT forms it (:901): acosf, a float product, a double quotient, stored to float"""
    c = np.asarray(cos_parallax, np.float32)
    return ((np.arccos(c).astype(np.float32) * np.float32(180)).astype(np.float64) / np.pi).astype(np.float32)


def _host_batch(kps, counts, camera, img_stride):
    kps = np.ascontiguousarray(kps, dtype=_lib.KEYPOINT_DTYPE)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if kps.ndim != 2 or kps.shape[0] != counts.shape[0] or kps.shape[0] % img_stride:
        raise ValueError("kps [n_frames * img_stride, capacity] and counts [n_frames * img_stride] expected")
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride = ptr(kps), ptr(counts), int(img_stride)
    tb.fx, tb.fy, tb.cx, tb.cy = (float(v) for v in camera)
    return tb, kps.shape[0] // img_stride, kps.shape[1], (kps, counts)


def initializer_batch(n_frames, kps, counts, camera, pairs, matches, draws, state, params, img_stride=2, context=None):
    """olf_initializer_pairs_dev on torch's current stream, without a synchronise.  kps / counts in the extractor's layout (frame j = image j *
    img_stride): device tensors; camera = (fx, fy, cx, cy); pairs int32 [n_pairs, 2] = (reference frame, current frame); matches int32 [n_pairs,
    capacity] as search_for_initialization writes it; draws uint32-valued tensor [n_pairs, max_iterations, 8]; state: initializer_state(...) on the
    device, written in place; params: initializer_params(...).  Returns state."""
    import torch
    ctx = _ctx(context)
    n_pairs, cap = int(pairs.shape[0]), ctx.orb_capacity
    if tuple(pairs.shape) != (n_pairs, 2) or matches.numel() < n_pairs * cap or draws.numel() < 8 * n_pairs * params.max_iterations:
        raise ValueError("initializer_batch: pairs [n_pairs, 2], matches [n_pairs, capacity] and draws [n_pairs, max_iterations, 8] expected")
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride = _dev(kps, None, "kps"), _dev(counts, torch.int32, "counts"), int(img_stride)
    tb.fx, tb.fy, tb.cx, tb.cy = (float(v) for v in camera)
    io = _io(state, lambda a, name: _dev(a, None, name))
    _call_dev("olf_initializer_pairs_dev", ctx, C.byref(tb), int(n_frames), n_pairs, _dev(pairs, torch.int32, "pairs"), _dev(matches, torch.int32, "matches"),
              C.byref(params), _dev(draws, None, "draws"), C.byref(io))
    return state


def initializer_apply(n_frames, counts, pairs, matches, state, out=None, n_matches=None, Tcw=None, img_stride=2, context=None):
    """olf_initializer_apply_dev on torch's current stream: for every pair whose state says ok, out[p, i] = matches[p, i] where the match is a
    correspondence and triangulated, -1 elsewhere; n_matches[p] the count that remains; Tcw[p] the current frame's pose from R21 and t21.  Other pairs keep
    their rows.  None for an output makes a new tensor (out: a copy of matches; the others zeros).  Returns (out, n_matches, Tcw)."""
    import torch
    ctx = _ctx(context)
    n_pairs = int(pairs.shape[0])
    out = matches.clone() if out is None else out
    n_matches = torch.zeros((n_pairs,), dtype=torch.int32, device="cuda") if n_matches is None else n_matches
    Tcw = torch.zeros((n_pairs, 16), dtype=torch.float32, device="cuda") if Tcw is None else Tcw
    tb = _lib.TrackBatchC()
    tb.counts, tb.img_stride = _dev(counts, torch.int32, "counts"), int(img_stride)
    _call_dev("olf_initializer_apply_dev", ctx, C.byref(tb), int(n_frames), n_pairs, _dev(pairs, torch.int32, "pairs"), _dev(matches, torch.int32, "matches"),
              _dev(state["triangulated"], torch.uint8, "triangulated"), _dev(state["ok"], torch.int32, "ok"), _dev(state["R21"], torch.float32, "R21"),
              _dev(state["t21"], torch.float32, "t21"), _dev(out, torch.int32, "out"), _dev(n_matches, torch.int32, "n_matches"),
              _dev(Tcw, torch.float32, "Tcw"))
    return out, n_matches, Tcw


def Initialize(kps, counts, camera, pair, matches, draws, state, params, row=0, img_stride=1):
    """Initializer::Initialize of one pair from host arrays, no device: olf_initializer.  pair = (reference frame, current frame); matches [capacity];
    draws [max_iterations, 8]; state: initializer_state(..., device=False), whose row `row` is this pair's and is written in place.  Returns the status
    bits (2048 a refused pair, 32768 a degenerate hypothesis, 65536 a NaN cosine)."""
    tb, n_frames, cap, keep = _host_batch(kps, counts, camera, img_stride)
    m = np.ascontiguousarray(matches, dtype=np.int32).reshape(-1)
    dr = np.ascontiguousarray(draws, dtype=np.uint32).reshape(-1)
    if m.shape[0] != cap or dr.shape[0] < 8 * max(params.max_iterations, 0):
        raise ValueError("Initialize: matches [capacity] and draws [max_iterations, 8] expected")
    io = _io(state, _ransac.host_address, row=slice(row, row + 1))
    status = C.c_int32(0)
    _lib.check(lib().olf_initializer(C.byref(tb), cap, n_frames, int(pair[0]), int(pair[1]), ptr(m), C.byref(params), ptr(dr), C.byref(io),
                                     C.addressof(status)), "olf_initializer")
    return int(status.value)


def initializer_pairs(kps, counts, camera, pairs, matches, draws, state, params, img_stride=1, context=None):
    """The batch from host arrays ON THE DEVICE: olf_initializer_pairs (stages, runs the kernel, synchronises).  Shapes as initializer_batch; state:
    initializer_state(..., device=False), written in place.  A set status bit raises OlfError with the outputs complete."""
    ctx = _ctx(context)
    tb, n_frames, cap, keep = _host_batch(kps, counts, camera, img_stride)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    m = np.ascontiguousarray(matches, dtype=np.int32)
    dr = np.ascontiguousarray(draws, dtype=np.uint32)
    n_pairs = pairs.shape[0]
    if cap != ctx.orb_capacity or m.shape != (n_pairs, cap) or dr.size != 8 * n_pairs * params.max_iterations:
        raise ValueError("initializer_pairs: key points of the context's capacity, matches [n_pairs, capacity] and draws [n_pairs, max_iterations, 8] expected")
    io = _io(state, _ransac.host_address)
    _lib.check(lib().olf_initializer_pairs(ctx.handle, C.byref(tb), n_frames, n_pairs, ptr(pairs), ptr(m), C.byref(params), ptr(dr), C.byref(io)),
               "olf_initializer_pairs")
    return state
