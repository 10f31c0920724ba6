"""Sim3Solver's RANSAC (src/Sim3Solver.cc) as LoopClosing::ComputeSim3 drives it (src/LoopClosing.cc:280-307), for a list of key-frame pairs
(include/orbline.h; csrc/sim3solver_batch.hip, sim3solver_host.cpp, sim3solver_api.cpp, sim3solver_terms.hpp).

  sim3_state              the carried state and the outputs of n solvers, zero-initialised: device tensors or host arrays
  sim3_solver_batch       device tensors: one iterate(n_iterations) of every listed pair, without a synchronise
  sim3_filter_matches     device tensors: the matches kept where the accepted hypothesis has an inlier (:319-324)
  Sim3Solve               host arrays, no device: one pair
  sim3_solver_pairs       host arrays, staged and run on the device
  sim3_draws              the random stream of C.20 for tests and tools: uint32 values below 2^31

The random stream is the caller's: draws [n_pairs, max_iterations, 3], indexed by absolute iteration, so a resumed call reads on.
best_s / best_R / best_t of the state are what ORBmatcher.search_by_sim3_pairs takes as s12 / R12 / t12."""
import ctypes as C
import numpy as np
from . import _lib, _ransac
from ._lib import lib, ptr
from .matcher import _call_dev, _ctx, _dev

STATUS_OCTAVE, STATUS_PAIR = 256, 2048

_STATE = (("iterations_done", np.int32, ()), ("best_inliers", np.int32, ()), ("best_s", np.float32, ()), ("best_R", np.float32, (9,)),
          ("best_t", np.float32, (3,)), ("best_T12", np.float32, (16,)), ("accepted", np.int32, ()), ("no_more", np.int32, ()), ("n_inliers", np.int32, ()),
          ("inliers", np.uint8, None), ("n_correspondences", np.int32, ()), ("counts", np.int32, None))


def sim3_ransac(fix_scale=False, probability=0.99, min_inliers=20, max_iterations=300, n_iterations=5):
    """olf_sim3_ransac: SetRansacParameters(probability, min_inliers, max_iterations) and the window of one iterate(n_iterations)"""
    r = _lib.Sim3RansacC()
    r.fix_scale, r.probability, r.min_inliers, r.max_iterations, r.n_iterations = int(bool(fix_scale)), float(probability), int(min_inliers), int(max_iterations), int(n_iterations)
    return r


def sim3_state(n_pairs, capacity, max_iterations, device=True, counts=True):
    """The arrays of olf_sim3_solver_io for n_pairs new solvers, all zero, as a dict: device tensors (device=True) or numpy arrays.  counts=False leaves the
    per-iteration counts out."""
    return _ransac.new_state(_STATE, n_pairs, capacity, max_iterations, device, counts)


def _io(st, address, row=None):
    return _ransac.io_block(_lib.Sim3SolverIoC, _STATE, st, address, row)


def sim3_draws(n_pairs, max_iterations, seed):
    """[n_pairs, max_iterations, 3] uint32 values below 2^31, as rand() returns them"""
    return _ransac.draws(n_pairs, max_iterations, 3, seed)


def sim3_solver_batch(n_frames, kps, counts, Tcw, mp_world, camera, pairs, matches12, draws, state, ransac, mp_valid=None, mp_bad=None, img_stride=2,
                      context=None):
    """olf_sim3_solver_pairs_dev on torch's current stream, without a synchronise.  kps / counts in the extractor's layout (frame j = image j * img_stride),
    Tcw [n_frames, 4, 4], mp_world [n_frames, capacity, 3], mp_valid / mp_bad [n_frames, capacity] (uint8, or None): device tensors; camera = (fx, fy, cx,
    cy); pairs int32 [n_pairs, 2]; matches12 int32 [n_pairs, capacity] as search_by_bow_pairs writes it; draws uint32-valued int32 / uint32 tensor
    [n_pairs, max_iterations, 3]; state: sim3_state(...) on the device, changed in place; ransac: sim3_ransac(...).  Returns state."""
    import torch
    ctx = _ctx(context)
    n_pairs, cap = int(pairs.shape[0]), ctx.orb_capacity
    if tuple(pairs.shape) != (n_pairs, 2) or matches12.numel() < n_pairs * cap or draws.numel() < 3 * n_pairs * ransac.max_iterations:
        raise ValueError("sim3_solver_batch: pairs [n_pairs, 2], matches12 [n_pairs, capacity] and draws [n_pairs, max_iterations, 3] expected")
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride = _dev(kps, None, "kps"), _dev(counts, torch.int32, "counts"), int(img_stride)
    tb.Tcw, tb.mp_world, tb.mp_valid = _dev(Tcw, torch.float32, "Tcw"), _dev(mp_world, torch.float32, "mp_world"), _dev(mp_valid, torch.uint8, "mp_valid")
    tb.fx, tb.fy, tb.cx, tb.cy = (float(v) for v in camera)
    io = _io(state, lambda a, name: _dev(a, None, name))
    _call_dev("olf_sim3_solver_pairs_dev", ctx, C.byref(tb), int(n_frames), _dev(mp_bad, torch.uint8, "mp_bad"), n_pairs, _dev(pairs, torch.int32, "pairs"),
              _dev(matches12, torch.int32, "matches12"), C.byref(ransac), _dev(draws, None, "draws"), C.byref(io))
    return state


def sim3_filter_matches(matches12, inliers, n_inliers=None, out=None, context=None):
    """olf_sim3_filter_matches_dev on torch's current stream: out[p, i] = matches12[p, i] where inliers[p, i] is set, -1 elsewhere (out=None: a new tensor;
    out may be matches12).  n_inliers (or None): pairs with a negative value keep their row of out."""
    import torch
    ctx = _ctx(context)
    if out is None:
        out = torch.full_like(matches12, -1)
    _call_dev("olf_sim3_filter_matches_dev", ctx, int(matches12.shape[0]), _dev(matches12, torch.int32, "matches12"), _dev(inliers, torch.uint8, "inliers"),
              _dev(n_inliers, torch.int32, "n_inliers"), _dev(out, torch.int32, "out"))
    return out


def _host_batch(kps, counts, Tcw, mp_world, camera, mp_valid, img_stride):
    return _ransac.host_batch(kps, counts, mp_world, camera, mp_valid, img_stride, Tcw=Tcw)


def Sim3Solve(kps, counts, Tcw, mp_world, camera, scale_factors, pair, matches12, draws, state, ransac, row=0, mp_valid=None, mp_bad=None, img_stride=1):
    """One iterate(n_iterations) of one Sim3Solver from host arrays, no device: olf_sim3_solver.  pair = (kf1, kf2); matches12 [capacity]; draws
    [max_iterations, 3]; state: sim3_state(..., device=False), whose row `row` is this solver's and is changed in place.  Returns the status bits (256 an
    octave outside the levels, 2048 a refused pair)."""
    tb, n_frames, cap, keep = _host_batch(kps, counts, Tcw, mp_world, camera, mp_valid, img_stride)
    m12 = np.ascontiguousarray(matches12, dtype=np.int32).reshape(-1)
    dr = np.ascontiguousarray(draws, dtype=np.uint32).reshape(-1)
    sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
    bad = None if mp_bad is None else np.ascontiguousarray(mp_bad, dtype=np.uint8)
    if m12.shape[0] != cap or dr.shape[0] < 3 * ransac.max_iterations:
        raise ValueError("Sim3Solve: matches12 [capacity] and draws [max_iterations, 3] expected")
    io = _io(state, _ransac.host_address, row=slice(row, row + 1))
    status = C.c_int32(0)
    _lib.check(lib().olf_sim3_solver(C.byref(tb), cap, n_frames, ptr(bad), ptr(sf), sf.shape[0], int(pair[0]), int(pair[1]), ptr(m12), C.byref(ransac), ptr(dr),
                                     C.byref(io), C.addressof(status)), "olf_sim3_solver")
    return int(status.value)


def sim3_solver_pairs(kps, counts, Tcw, mp_world, camera, pairs, matches12, draws, state, ransac, mp_valid=None, mp_bad=None, img_stride=1, context=None):
    """The batch from host arrays ON THE DEVICE: olf_sim3_solver_pairs (stages, runs the kernel, synchronises).  Shapes as sim3_solver_batch; state:
    sim3_state(..., device=False), changed in place.  A set status bit raises OlfError with the outputs complete."""
    ctx = _ctx(context)
    tb, n_frames, cap, keep = _host_batch(kps, counts, Tcw, mp_world, camera, mp_valid, img_stride)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    m12 = np.ascontiguousarray(matches12, dtype=np.int32)
    dr = np.ascontiguousarray(draws, dtype=np.uint32)
    bad = None if mp_bad is None else np.ascontiguousarray(mp_bad, dtype=np.uint8)
    n_pairs = pairs.shape[0]
    if cap != ctx.orb_capacity or m12.shape != (n_pairs, cap) or dr.size != 3 * n_pairs * ransac.max_iterations:
        raise ValueError("sim3_solver_pairs: planes of the context's capacity, matches12 [n_pairs, capacity] and draws [n_pairs, max_iterations, 3] expected")
    io = _io(state, _ransac.host_address)
    _lib.check(lib().olf_sim3_solver_pairs(ctx.handle, C.byref(tb), n_frames, ptr(bad), n_pairs, ptr(pairs), ptr(m12), C.byref(ransac), ptr(dr), C.byref(io)),
               "olf_sim3_solver_pairs")
    return state
