"""PnPsolver's RANSAC (src/PnPsolver.cc) as Tracking::Relocalization drives it (src/Tracking.cc:2255-2308), for a list of (key frame, frame) pairs
(include/orbline.h; csrc/pnpsolver_batch.hip, pnpsolver_host.cpp, pnpsolver_api.cpp, pnpsolver_terms.hpp).

  pnp_state               the carried state and the outputs of n solvers, zero-initialised: device tensors or host arrays
  pnp_solver_batch        device tensors: one iterate(n_iterations) of every listed pair, without a synchronise
  pnp_apply_inliers       device tensors: what the tracker does with an accepted solver's inliers (:2297-2308)
  PnPSolve                host arrays, no device: one pair
  pnp_solver_pairs        host arrays, staged and run on the device
  pnp_draws               the random stream of C.20 for tests and tools: uint32 values below 2^31

The random stream is the caller's: draws [n_pairs, max_iterations, 4], indexed by absolute iteration modulo max_iterations (C.26), so a
resumed call reads on.  Tcw of the state is what ORBmatcher's search_by_projection_kf_pairs takes as the candidate's own pose."""
import ctypes as C
import numpy as np
from . import _lib, _ransac
from ._lib import lib, ptr
from .matcher import _call_dev, _ctx, _dev

STATUS_OCTAVE, STATUS_PAIR, STATUS_DEGENERATE = 256, 2048, 32768

_STATE = (("iterations_done", np.int32, ()), ("best_inliers", np.int32, ()), ("best_Tcw", np.float32, (16,)), ("best_flags", np.uint8, None),
          ("refined_inliers", np.int32, ()), ("refined_Tcw", np.float32, (16,)), ("refined_flags", np.uint8, None), ("accepted", np.int32, ()),
          ("no_more", np.int32, ()), ("n_inliers", np.int32, ()), ("inliers", np.uint8, None), ("Tcw", np.float32, (16,)), ("n_correspondences", np.int32, ()),
          ("counts", np.int32, None))


def pnp_ransac(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991, n_iterations=5):
    """olf_pnp_ransac: SetRansacParameters(probability, min_inliers, max_iterations, min_set, epsilon, th2) and the window of one iterate(n_iterations);
    the defaults are the tracker's (src/Tracking.cc:2256, :2281)"""
    r = _lib.PnpRansacC()
    r.probability, r.min_inliers, r.max_iterations, r.min_set, r.n_iterations = float(probability), int(min_inliers), int(max_iterations), int(min_set), int(n_iterations)
    r.epsilon, r.th2 = float(epsilon), float(th2)
    return r


def pnp_state(n_pairs, capacity, max_iterations, device=True, counts=True):
    """The arrays of olf_pnp_solver_io for n_pairs new solvers, all zero, as a dict: device tensors (device=True) or numpy arrays.  counts=False leaves the
    per-iteration counts out."""
    return _ransac.new_state(_STATE, n_pairs, capacity, max_iterations, device, counts)


def _io(st, address, row=None):
    return _ransac.io_block(_lib.PnpSolverIoC, _STATE, st, address, row)


def pnp_draws(n_pairs, max_iterations, seed):
    """[n_pairs, max_iterations, 4] uint32 values below 2^31, as rand() returns them"""
    return _ransac.draws(n_pairs, max_iterations, 4, seed)


def _dev_batch(kps, counts, mp_world, camera, mp_valid, img_stride):
    import torch
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride = _dev(kps, None, "kps"), _dev(counts, torch.int32, "counts"), int(img_stride)
    tb.mp_world, tb.mp_valid = _dev(mp_world, torch.float32, "mp_world"), _dev(mp_valid, torch.uint8, "mp_valid")
    tb.fx, tb.fy, tb.cx, tb.cy = (float(v) for v in camera)
    return tb


def pnp_solver_batch(n_frames, kps, counts, mp_world, camera, pairs, matches, draws, state, ransac, mp_valid=None, mp_bad=None, img_stride=2, context=None):
    """olf_pnp_solver_pairs_dev on torch's current stream, without a synchronise.  kps / counts in the extractor's layout (frame j = image j * img_stride),
    mp_world [n_frames, capacity, 3], mp_valid / mp_bad [n_frames, capacity] (uint8, or None): device tensors; camera = (fx, fy, cx, cy); pairs int32
    [n_pairs, 2] = (key frame, frame); matches int32 [n_pairs, capacity] as search_by_bow_pairs writes it; draws uint32-valued int32 / uint32 tensor
    [n_pairs, max_iterations, 4]; state: pnp_state(...) on the device, changed in place; ransac: pnp_ransac(...).  Returns state."""
    import torch
    ctx = _ctx(context)
    n_pairs, cap = int(pairs.shape[0]), ctx.orb_capacity
    if tuple(pairs.shape) != (n_pairs, 2) or matches.numel() < n_pairs * cap or draws.numel() < 4 * n_pairs * ransac.max_iterations:
        raise ValueError("pnp_solver_batch: pairs [n_pairs, 2], matches [n_pairs, capacity] and draws [n_pairs, max_iterations, 4] expected")
    tb = _dev_batch(kps, counts, mp_world, camera, mp_valid, img_stride)
    io = _io(state, lambda a, name: _dev(a, None, name))
    _call_dev("olf_pnp_solver_pairs_dev", ctx, C.byref(tb), int(n_frames), _dev(mp_bad, torch.uint8, "mp_bad"), n_pairs, _dev(pairs, torch.int32, "pairs"),
              _dev(matches, torch.int32, "matches"), C.byref(ransac), _dev(draws, None, "draws"), C.byref(io))
    return state


def pnp_apply_inliers(n_frames, counts, pairs, matches, state, out=None, cur_valid=None, already_found=None, img_stride=2, context=None):
    """olf_pnp_apply_inliers_dev on torch's current stream: for every pair whose state says accepted, out[p, i] = matches[p, i] where inliers[p, i] is set,
    -1 elsewhere; cur_valid[p, i] = 1 / 0 likewise; already_found[p, v] = 1 for every inlier's key-frame feature v, 0 elsewhere.  Other pairs keep their
    rows.  None for an output makes a new tensor (out: a copy of matches; the masks: zeros).  Returns (out, cur_valid, already_found)."""
    import torch
    ctx = _ctx(context)
    n_pairs = int(pairs.shape[0])
    out = matches.clone() if out is None else out
    cur_valid = torch.zeros(matches.shape, dtype=torch.uint8, device="cuda") if cur_valid is None else cur_valid
    already_found = torch.zeros(matches.shape, dtype=torch.uint8, device="cuda") if already_found is None else already_found
    tb = _lib.TrackBatchC()
    tb.counts, tb.img_stride = _dev(counts, torch.int32, "counts"), int(img_stride)
    _call_dev("olf_pnp_apply_inliers_dev", ctx, C.byref(tb), int(n_frames), n_pairs, _dev(pairs, torch.int32, "pairs"), _dev(matches, torch.int32, "matches"),
              _dev(state["inliers"], torch.uint8, "inliers"), _dev(state["accepted"], torch.int32, "accepted"), _dev(state["n_inliers"], torch.int32, "n_inliers"),
              _dev(out, torch.int32, "out"), _dev(cur_valid, torch.uint8, "cur_valid"), _dev(already_found, torch.uint8, "already_found"))
    return out, cur_valid, already_found


def PnPSolve(kps, counts, mp_world, camera, scale_factors, pair, matches, draws, state, ransac, row=0, mp_valid=None, mp_bad=None, img_stride=1):
    """One iterate(n_iterations) of one PnPsolver from host arrays, no device: olf_pnp_solver.  pair = (key frame, frame); matches [capacity]; draws
    [max_iterations, 4]; state: pnp_state(..., device=False), whose row `row` is this solver's and is changed in place.  Returns the status bits (256 an
    octave outside the levels, 2048 a refused pair, 32768 a degenerate hypothesis)."""
    tb, n_frames, cap, keep = _ransac.host_batch(kps, counts, mp_world, camera, mp_valid, img_stride)
    m = np.ascontiguousarray(matches, dtype=np.int32).reshape(-1)
    dr = np.ascontiguousarray(draws, dtype=np.uint32).reshape(-1)
    sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
    bad = None if mp_bad is None else np.ascontiguousarray(mp_bad, dtype=np.uint8)
    if m.shape[0] != cap or dr.shape[0] < 4 * ransac.max_iterations:
        raise ValueError("PnPSolve: matches [capacity] and draws [max_iterations, 4] expected")
    io = _io(state, _ransac.host_address, row=slice(row, row + 1))
    status = C.c_int32(0)
    _lib.check(lib().olf_pnp_solver(C.byref(tb), cap, n_frames, ptr(bad), ptr(sf), sf.shape[0], int(pair[0]), int(pair[1]), ptr(m), C.byref(ransac), ptr(dr),
                                    C.byref(io), C.addressof(status)), "olf_pnp_solver")
    return int(status.value)


def pnp_solver_pairs(kps, counts, mp_world, camera, pairs, matches, draws, state, ransac, mp_valid=None, mp_bad=None, img_stride=1, context=None):
    """The batch from host arrays ON THE DEVICE: olf_pnp_solver_pairs (stages, runs the kernel, synchronises).  Shapes as pnp_solver_batch; state:
    pnp_state(..., device=False), changed in place.  A set status bit raises OlfError with the outputs complete."""
    ctx = _ctx(context)
    tb, n_frames, cap, keep = _ransac.host_batch(kps, counts, mp_world, camera, mp_valid, img_stride)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    m = np.ascontiguousarray(matches, dtype=np.int32)
    dr = np.ascontiguousarray(draws, dtype=np.uint32)
    bad = None if mp_bad is None else np.ascontiguousarray(mp_bad, dtype=np.uint8)
    n_pairs = pairs.shape[0]
    if cap != ctx.orb_capacity or m.shape != (n_pairs, cap) or dr.size != 4 * n_pairs * ransac.max_iterations:
        raise ValueError("pnp_solver_pairs: planes of the context's capacity, matches [n_pairs, capacity] and draws [n_pairs, max_iterations, 4] expected")
    io = _io(state, _ransac.host_address)
    _lib.check(lib().olf_pnp_solver_pairs(ctx.handle, C.byref(tb), n_frames, ptr(bad), n_pairs, ptr(pairs), ptr(m), C.byref(ransac), ptr(dr), C.byref(io)),
               "olf_pnp_solver_pairs")
    return state
