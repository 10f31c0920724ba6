"""What the wrappers of the two RANSAC solvers (sim3solver.py, pnpsolver.py) share.  A solver names its state as a field table of (name, dtype, tail):
tail is the shape behind [n_pairs], or None for a row -- [capacity] per pair, and [max_iterations] for "counts"."""
import numpy as np
from . import _lib
from ._lib import ptr


def new_state(fields, n_pairs, capacity, max_iterations, device, counts):
    """the arrays of a solver's io block for n_pairs new solvers, all zero, as a dict: device tensors or numpy arrays; counts=False leaves "counts" out"""
    st = {}
    for name, dt, tail in fields:
        if name == "counts" and not counts:
            st[name] = None
            continue
        shape = (n_pairs,) + ((max_iterations,) if name == "counts" else (capacity,) if tail is None else tail)
        if device:
            import torch
            st[name] = torch.zeros(shape, dtype=getattr(torch, np.dtype(dt).name), device="cuda")
        else:
            st[name] = np.zeros(shape, dt)
    return st


def io_block(io_type, fields, st, address, row=None):
    """io_type filled with address(array, name) of every field of st, or of its rows `row`"""
    io = io_type()
    for name, _, _ in fields:
        setattr(io, name, address(st[name] if row is None or st[name] is None else st[name][row], name))
    return io


def host_address(a, name):
    return None if a is None else a.ctypes.data


def draws(n_pairs, max_iterations, width, seed):
    """[n_pairs, max_iterations, width] uint32 values below 2^31, as rand() returns them (C.20)"""
    return np.random.default_rng(seed).integers(0, 1 << 31, size=(n_pairs, max_iterations, width), dtype=np.uint32)


def host_batch(kps, counts, mp_world, camera, mp_valid, img_stride, Tcw=None):
    """TrackBatchC over host arrays (Tcw only where the solver reads poses); returns it with n_frames, the capacity and the arrays it points into"""
    kps = np.ascontiguousarray(kps, dtype=_lib.KEYPOINT_DTYPE)
    world = np.ascontiguousarray(mp_world, dtype=np.float32)
    n_frames, cap = world.shape[0], world.shape[1]
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    Tcw = None if Tcw is None else np.ascontiguousarray(Tcw, dtype=np.float32)
    ok = kps.shape == (n_frames * img_stride, cap) and counts.shape[0] == n_frames * img_stride and world.shape == (n_frames, cap, 3)
    if not ok or (Tcw is not None and Tcw.size != 16 * n_frames):
        raise ValueError("kps [n_frames * img_stride, capacity], counts%s and mp_world [n_frames, capacity, 3] expected" % ("" if Tcw is None else ", Tcw [n_frames, 4, 4]"))
    valid = None if mp_valid is None else np.ascontiguousarray(mp_valid, dtype=np.uint8)
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride, tb.Tcw, tb.mp_world, tb.mp_valid = ptr(kps), ptr(counts), int(img_stride), ptr(Tcw), ptr(world), ptr(valid)
    tb.fx, tb.fy, tb.cx, tb.cy = (float(v) for v in camera)
    return tb, n_frames, cap, (kps, counts, Tcw, world, valid)
