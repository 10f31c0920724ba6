"""Rows per second of olf_pose_optimization_batch_dev (csrc/posepoints_batch.hip: Optimizer::PoseOptimization, one workgroup per row) at 1, 64 and 1024
rows of 100 / 500 / 2000 held points, and the host form's (olf_pose_optimization) time for the same rows.  The context has nfeatures = 2000 (the default
capacity, where the edges of a row take 58 KB of LDS).  The rows are synthetic (no image is read): points at 2-15 m observed with half a pixel of noise
times the level's scale, two in three stereo, one gross outlier in ten, a start pose a few centimetres and tenths of a degree off.  --distinct different
rows are tiled over the list.
    python tools/pose_points_latency.py [--distinct 16] [--host-rows 8] [--held 100,500,2000] [--rows 1,64,1024]
HIP events, warmed up, median of five windows of ten calls; the host form by the host clock over --host-rows rows."""
import math
import time
import numpy as np
from latency_common import parser, side_stream, up, windows
import torch
from orb_line_slam_amd import _lib, posepoints
from orb_line_slam_amd._lib import KEYPOINT_DTYPE

ap = parser()
ap.set_defaults(distinct=16)
ap.add_argument("--host-rows", type=int, default=8)
ap.add_argument("--held", default="100,500,2000", help="held points per row, comma-separated")
ap.add_argument("--rows", default="1,64,1024", help="rows per call, comma-separated")
args = ap.parse_args()
W, H, fx, bf = 1241, 376, 718.856, 386.1448
cx, cy = W / 2.0, H / 2.0
params = _lib.default_params()
params.orb.nfeatures = 2000
ctx = _lib.Context(params, W, H, 2)          # (the entry reads no image: the context gives the capacity and the level table)
side_stream()
cap, nlev = ctx.orb_capacity, ctx.nlevels
sf, sig = np.zeros(nlev, np.float32), np.zeros(nlev, np.float32)
_lib.lib().olf_orb_scale_tables(ctx.handle, sf.ctypes.data, None, None, sig.ctypes.data, None)
rng = np.random.default_rng(78)
print(f"capacity {cap}; clocks as the machine leaves them (not pinned)", flush=True)


def rot(r):
    a = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / a
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def se3(r, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(r), t
    return T


def rows(D, held):
    kps, ur, Tcw, fmp, worlds = np.zeros((D, cap), KEYPOINT_DTYPE), np.full((D, cap), -1.0, np.float32), np.zeros((D, 16), np.float32), np.full((D, cap), -1, np.int32), []
    for j in range(D):
        Tt = se3(rng.uniform(-0.2, 0.2, 3), rng.uniform(-1, 1, 3))
        Tcw[j] = (se3(rng.uniform(-0.006, 0.006, 3), rng.uniform(-0.05, 0.05, 3)) @ Tt).astype(np.float32).reshape(16)
        Tinv = np.linalg.inv(Tt)
        u, v, z, octave = rng.uniform(20, W - 20, held), rng.uniform(20, H - 20, held), rng.uniform(2, 15, held), rng.integers(0, nlev, held)
        P = np.stack([(u - cx) * z / fx, (v - cy) * z / fx, z], 1)
        worlds.append((P @ Tinv[:3, :3].T + Tinv[:3, 3]).astype(np.float32))
        d = rng.normal(0.0, 1.0, (held, 3)) * (0.5 * sf[octave])[:, None]
        gross = rng.random(held) < 0.1
        d[gross, :2] += rng.choice([-1.0, 1.0], (int(gross.sum()), 2)) * rng.uniform(20, 60, (int(gross.sum()), 2))
        kps["x"][j, :held], kps["y"][j, :held], kps["octave"][j, :held] = u + d[:, 0], v + d[:, 1], octave
        ur[j, :held] = np.where(np.arange(held) % 3 == 1, -1.0, u - bf / z + d[:, 2])
        fmp[j, :held] = j * held + np.arange(held)
    return kps, ur, Tcw, fmp, np.concatenate(worlds)


line = "%-34s %5d rows of %4d held: %9.3f ms per call, %10.0f rows/s (median of 5 windows of 10, HIP events; min %.3f max %.3f ms)"
for held in (int(v) for v in args.held.split(",")):
    D = args.distinct
    kps, ur, Tcw, fmp, world = rows(D, min(held, cap))
    for B in (int(v) for v in args.rows.split(",")):
        tile = np.arange(B) % D
        d = dict(kps=up(kps[tile].view(np.uint8).reshape(-1)), counts=up(np.full(B, min(held, cap), np.int32)), ur=up(ur[tile]), Tcw=up(Tcw[tile]), fmp=up(fmp[tile]), mpw=up(world))
        out = {}
        run = lambda: posepoints.pose_optimization_batch(d["kps"], d["counts"], 1, d["ur"], (fx, fx, cx, cy, bf), d["Tcw"], d["fmp"], d["mpw"], n_frames=B, out=out, context=ctx)
        res = run()
        torch.cuda.synchronize()
        if B == 64:
            it, st = res["iters"].cpu().numpy(), res["status"].cpu().numpy()
            print(f"  {held} held: status 0 in {int((st == 0).sum())} of {B} rows, Levenberg iterations per row {it.sum(1).mean():.1f}, good per row {res['n_good'].float().mean().item():.0f}", flush=True)
        t = windows(run)
        print(line % ("olf_pose_optimization_batch_dev", B, held, t[0], 1e3 * B / t[0], t[1], t[2]), flush=True)
    n = min(args.host_rows, D)
    t0 = time.perf_counter()
    for j in range(n):
        posepoints.pose_optimization_host(kps[j, :held], ur[j, :held], Tcw[j], (fx, fx, cx, cy, bf), fmp[j, :held], world, sig)
    dt = (time.perf_counter() - t0) / n
    print(f"{'olf_pose_optimization (host form)':34s} {n:5d} rows of {held:4d} held: {1e3 * dt:9.3f} ms per row, {1 / dt:10.0f} rows/s (host clock, wrapper included)", flush=True)
ctx.poll_status()
ctx.close()
