"""What the *_latency.py tools share, stated once: the common arguments, the bench's shuffled synthetic batch with everything the tools extract from it
(made when first asked for, so a tool pays only for what it reads and nothing is made inside a timed window that the tool did not ask for before it), the
stopwatch (HIP events, warmed up, median of five windows of ten calls) and the host view of one frame of the batch for the host entries of the C ABI.
Imported by the tools from their own directory:  from latency_common import BenchBatch, host_view, parser
(kfdb_latency.py, which uses no images, takes side_stream and windows only; bench and the synthetic generator are imported when a batch is made)"""
import argparse, os, sys, time
from functools import cached_property
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import torch
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, matcher
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, check, lib


def parser(pairs_help=None):
    """--config, --pairs and --distinct; a tool adds its own"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--pairs", type=int, default=0, help=pairs_help)
    ap.add_argument("--distinct", type=int, default=512)
    return ap


def side_stream():
    """make a side stream torch's current one and return its handle"""
    torch.cuda.set_stream(torch.cuda.Stream())          # (the default stream's handle, 0, would send every *_dev call to the context's own stream)
    return torch.cuda.current_stream().cuda_stream


def zeros(shape, dt):
    return torch.zeros(shape, dtype=dt, device="cuda")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def windows(fn, events=True):
    """two warm calls, then five windows of ten calls, by HIP events or (for calls that return to the host) by the host clock between two synchronisations:
    (median, min, max) in ms per call"""
    fn(); fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                fn()
            b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / 10)
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            ms.append(1e2 * (time.perf_counter() - t0))
    return sorted(ms)[2], min(ms), max(ms)


class BenchBatch:
    """The left and right images of the bench's shuffled batch on the device, in a context made for them, on a side stream.  Everything extracted from them
    is an attribute made on first use, by the calls and in the layout the tools have always used:
      kps, desc, counts, ur, dp    olf_orb_extract_dev + olf_stereo_points_dev          valid           olf_stereo_points_mask_dev
      offs, idx                    olf_frame_grid_dev over the left frames (grid())      eye, world      identity poses, matcher.unproject_stereo under them
      kls, ldesc, lcounts, lm12, ldisp, lle    olf_line_extract_dev + olf_stereo_lines_dev               sf              olf_orb_scale_tables
      cnt, hk, hd, hu, hw, hv      the left frames' counts, keys, descriptors, uright, world points and valid mask on the host"""

    def __init__(self, args, tag_width=58):
        import bench
        from orb_line_slam_amd import synth
        self.tag_width = tag_width          # the column of the tag in the lines timed() prints
        self.cfg = cfg = bench.CONFIGS[args.config]
        self.W, self.H, self.B = cfg["w"], cfg["h"], args.pairs or cfg["pairs"]
        self.params = _lib.default_params()
        self.params.orb.nfeatures, self.params.line.lsd_nfeatures = cfg["nf"], cfg["nl"]
        self.params.stereo.fx, self.params.stereo.bf = cfg["fx"], cfg["bf"]
        self.ctx = _lib.Context(self.params, self.W, self.H, 2 * self.B)
        self.s, self.L, self.cap = side_stream(), lib(), self.ctx.orb_capacity
        nd = min(args.distinct, self.B)
        host = synth.stereo_batch(7000, nd, self.W, self.H)
        order = np.random.default_rng(1234).permutation(np.arange(self.B) % nd)          # the bench's shuffled batch
        self.imgs = torch.from_numpy(host[np.stack([2 * order, 2 * order + 1], 1).reshape(-1)].copy()).cuda()
        self.fx, self.cx, self.cy, self.mbf = float(cfg["fx"]), self.W / 2.0, self.H / 2.0, float(cfg["bf"])
        self.cam, self.bounds = (self.fx, self.fx, self.cx, self.cy, self.mbf), (0.0, float(self.W), 0.0, float(self.H))
        self.keep = []          # what the host views point to

    def timed(self, tag, fn, note=""):
        """windows(fn) by HIP events, printed in the tools' one line -- `note`: what a tool says between "per call (" and "median" -- and the median
        returned"""
        med, lo, hi = windows(fn)
        self.ctx.synchronize()
        print("%-*s %8.3f ms per call (%smedian of 5 windows of 10, HIP events; min %.3f max %.3f)" % (self.tag_width, tag, med, note, lo, hi), flush=True)
        return med

    @cached_property
    def _points(self):
        B, cap, L, h, s = self.B, self.cap, self.L, self.ctx.handle, self.s
        kps, desc, counts = zeros((2 * B, cap, 28), torch.uint8), zeros((2 * B, cap, 32), torch.uint8), zeros((2 * B,), torch.int32)
        ur, dp = zeros((B, cap), torch.float32), zeros((B, cap), torch.float32)
        check(L.olf_orb_extract_dev(h, self.imgs.data_ptr(), 2 * B, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), s), "olf_orb_extract_dev")
        check(L.olf_stereo_points_dev(h, B, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), ur.data_ptr(), dp.data_ptr(), s), "olf_stereo_points_dev")
        return kps, desc, counts, ur, dp

    kps, desc, counts, ur, dp = (property(lambda self, i=i: self._points[i]) for i in range(5))

    @cached_property
    def valid(self):
        v = zeros((self.B, self.cap), torch.uint8)
        check(self.L.olf_stereo_points_mask_dev(self.ctx.handle, self.dp.data_ptr(), self.B * self.cap, v.data_ptr(), self.s), "olf_stereo_points_mask_dev")
        return v

    @cached_property
    def _grid(self):
        return zeros((self.B, _lib.GRID_CELLS + 1), torch.int32), zeros((self.B, self.cap), torch.int32)

    offs, idx = (property(lambda self, i=i: self._grid[i]) for i in range(2))

    def grid(self):
        """fill offs / idx (a call of its own, because one tool times it)"""
        check(self.L.olf_frame_grid_dev(self.ctx.handle, self.B, 2, self.kps.data_ptr(), self.counts.data_ptr(), *self.bounds, self.offs.data_ptr(),
                                        self.idx.data_ptr(), self.s), "olf_frame_grid_dev")

    @cached_property
    def eye(self):
        return torch.eye(4, dtype=torch.float32, device="cuda").repeat(self.B, 1, 1).contiguous()

    @cached_property
    def world(self):
        return matcher.unproject_stereo(self.B, self.kps, self.counts, self.dp, self.cam[:4], self.eye, img_stride=2, context=self.ctx)

    @cached_property
    def _lines(self):
        B, cap, L, h, s = self.B, self.ctx.line_capacity, self.L, self.ctx.handle, self.s
        kls, ldesc, lcounts = zeros((2 * B, cap, 68), torch.uint8), zeros((2 * B, cap, 32), torch.uint8), zeros((2 * B,), torch.int32)
        lm12, ldisp, lle = zeros((B, cap), torch.int32), zeros((B, cap, 2), torch.float32), zeros((B, cap, 3), torch.float64)
        check(L.olf_line_extract_dev(h, self.imgs.data_ptr(), 2 * B, kls.data_ptr(), ldesc.data_ptr(), lcounts.data_ptr(), s), "olf_line_extract_dev")
        check(L.olf_stereo_lines_dev(h, B, kls.data_ptr(), ldesc.data_ptr(), lcounts.data_ptr(), lm12.data_ptr(), ldisp.data_ptr(), lle.data_ptr(), s),
              "olf_stereo_lines_dev")
        return kls, ldesc, lcounts, lm12, ldisp, lle

    kls, ldesc, lcounts, lm12, ldisp, lle = (property(lambda self, i=i: self._lines[i]) for i in range(6))

    @cached_property
    def sf(self):
        sf = np.zeros(self.ctx.nlevels, np.float32)
        self.L.olf_orb_scale_tables(self.ctx.handle, sf.ctypes.data, None, None, None, None)
        return sf

    # the left frames on the host
    cnt = cached_property(lambda self: self.counts.cpu().numpy()[0::2])
    hk = cached_property(lambda self: self.kps.cpu().numpy().reshape(2 * self.B, self.cap * 28).view(KEYPOINT_DTYPE)[0::2])
    hd = cached_property(lambda self: np.ascontiguousarray(self.desc.cpu().numpy()[0::2]))
    hu = cached_property(lambda self: self.ur.cpu().numpy())
    hw = cached_property(lambda self: self.world.cpu().numpy())
    hv = cached_property(lambda self: self.valid.cpu().numpy().astype(bool))


def host_view(batch, j, kind="frame", **state):
    """The olf_frame_view (matcher._view_c) of left frame j of the batch for a host entry: its first cnt[j] key points and descriptors, the batch's camera,
    bounds and scale factors, no Python grid (the host entries build their own or read none).  kind: "frame" (a FrameView) or "keyframe" (a KeyFrameView).
    `state`: the members the search reads, by their FrameView names (mvuRight, mTcw, mFeatVec, mp_valid, mp_obs, mp_bad, mvbOutlier, mp_world, mp_desc,
    mp_maxd, mp_mind); whatever is not given is None.  A bool array given as state is pointed to as it is, so the caller sees what the search writes and
    can reset it.  The arrays stay alive in batch.keep."""
    n = int(min(batch.cnt[j], batch.cap))
    cls = {"frame": ola.FrameView, "keyframe": ola.KeyFrameView}[kind]
    v = cls.__new__(cls)
    v.mvKeysUn, v.mDescriptors, v.N, v.mvScaleFactors = batch.hk[j, :n], batch.hd[j, :n], n, batch.sf
    v.fx = v.fy = batch.fx; v.cx, v.cy, v.mbf = batch.cx, batch.cy, batch.mbf
    v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY = batch.bounds
    v.mvuRight = v.mTcw = v.mp_valid = v.mp_obs = v.mp_bad = v.mvbOutlier = v.mp_world = v.mp_desc = None
    v.mFeatVec = {}
    for name, a in state.items():
        setattr(v, name, a)
    return matcher._view_c(v, batch.keep)
