"""Latency of olf_pose_optimization_with_line_batch_dev (csrc/pose_batch.hip: Optimizer::PoseOptimizationWithLine, one workgroup per frame) and of
olf_discard_outliers_batch_dev for the bench's batch shape: --pairs frames (default: the configuration's) in a context with the configuration's image size
and capacities.  The frames are synthetic (no image is read): every frame carries nfeatures key points of which --held-points hold a map point and
0.6 * lsd_nfeatures key lines of which --held-lines hold a map line, at 2-15 m, observed with half a pixel of noise times the level's scale under a motion
of a few centimetres, a prior off by as much, and one gross outlier in ten.  --distinct different frames are tiled over the batch.
    python tools/pose_latency.py [--config C3] [--pairs N] [--distinct 16] [--held-points 0.2] [--held-lines 0.4]
HIP events, warmed up, median of five windows of ten calls."""
import math
import numpy as np
from latency_common import parser, side_stream, up, windows
import torch
import bench
from orb_line_slam_amd import _lib, pose
from orb_line_slam_amd._lib import KEYLINE_DTYPE, KEYPOINT_DTYPE

ap = parser("frames per call (default: the configuration's pairs per step)")
ap.set_defaults(distinct=16)
ap.add_argument("--held-points", type=float, default=0.2)
ap.add_argument("--held-lines", type=float, default=0.4)
args = ap.parse_args()
cfg = bench.CONFIGS[args.config]
W, H, B = cfg["w"], cfg["h"], args.pairs or cfg["pairs"]
params = _lib.default_params()
params.orb.nfeatures, params.line.lsd_nfeatures = cfg["nf"], cfg["nl"]
ctx = _lib.Context(params, W, H, 2)          # (the entry reads no image: the context gives the capacities and the level table)
side_stream()
cap, lcap, nlev = ctx.orb_capacity, ctx.line_capacity, ctx.nlevels
fx = fy = float(cfg["fx"])
cx, cy = W / 2.0, H / 2.0
sf = np.zeros(nlev, np.float32)
_lib.lib().olf_orb_scale_tables(ctx.handle, sf.ctypes.data, None, None, None, None)
rng = np.random.default_rng(77)
N, NL = min(cfg["nf"], cap), min(int(0.6 * cfg["nl"]), lcap)


def rot(r):
    a = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / a
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def se3(r, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(r), t
    return T


def unproject(Tinv, u, v, z):
    P = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    return (P @ Tinv[:3, :3].T + Tinv[:3, 3]).astype(np.float32)


def project(T, X):
    P = X.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    return cx + fx * P[:, 0] / P[:, 2], cy + fy * P[:, 1] / P[:, 2]


def noise(octave, n):
    d = rng.normal(0.0, 1.0, (n, 2)) * (0.5 * sf[octave])[:, None]
    gross = rng.random(n) < 0.1
    d[gross] += rng.choice([-1.0, 1.0], (int(gross.sum()), 2)) * rng.uniform(20, 60, (int(gross.sum()), 2))
    return d


D = min(args.distinct, B)
kps, kls = np.zeros((D, cap), KEYPOINT_DTYPE), np.zeros((D, lcap), KEYLINE_DTYPE)
lle, Tcw, Tprev = np.zeros((D, lcap, 3)), np.zeros((D, 16), np.float32), np.zeros((D, 16), np.float32)
fmp, fml = np.full((D, cap), -1, np.int32), np.full((D, lcap), -1, np.int32)
worlds, lworlds, held_total = [], [], [0, 0]
for j in range(D):
    Tp = se3(rng.uniform(-0.2, 0.2, 3), rng.uniform(-1, 1, 3))
    Mt = se3(rng.uniform(-0.006, 0.006, 3), rng.uniform(-0.05, 0.05, 3))
    Tt = (Mt @ Tp).astype(np.float32).astype(np.float64)
    Tcw[j], Tprev[j] = (se3(rng.uniform(-0.006, 0.006, 3), rng.uniform(-0.05, 0.05, 3)) @ Mt @ Tp).astype(np.float32).reshape(16), Tp.astype(np.float32).reshape(16)
    Tinv = np.linalg.inv(Tt)
    octave = rng.integers(0, nlev, N)
    kps["octave"][j, :N], kps["x"][j, :N], kps["y"][j, :N] = octave, rng.uniform(20, W - 20, N), rng.uniform(20, H - 20, N)
    held = np.flatnonzero(rng.random(N) < args.held_points)
    Xw = unproject(Tinv, rng.uniform(20, W - 20, len(held)), rng.uniform(20, H - 20, len(held)), rng.uniform(2, 15, len(held)))
    u, v = project(Tt, Xw)
    d = noise(octave[held], len(held))
    kps["x"][j, held], kps["y"][j, held] = u + d[:, 0], v + d[:, 1]
    fmp[j, held] = sum(len(w) for w in worlds) + np.arange(len(held))
    worlds.append(Xw)
    loct = rng.integers(0, nlev, NL)
    u0, v0, ang, length = rng.uniform(40, W - 120, NL), rng.uniform(40, H - 100, NL), rng.uniform(-1.2, 1.2, NL), rng.uniform(30, 70, NL)
    u1, v1 = u0 + length * np.cos(ang), v0 + length * np.sin(ang)
    lheld = np.flatnonzero(rng.random(NL) < args.held_lines)
    Ls = np.concatenate([unproject(Tinv, u0[lheld], v0[lheld], rng.uniform(2, 15, len(lheld))), unproject(Tinv, u1[lheld], v1[lheld], rng.uniform(2, 15, len(lheld)))], 1)
    (a0, b0), (a1, b1) = project(Tt, Ls[:, :3]), project(Tt, Ls[:, 3:])
    d0, d1 = noise(loct[lheld], len(lheld)), noise(loct[lheld], len(lheld))
    u0[lheld], v0[lheld], u1[lheld], v1[lheld] = a0 + d0[:, 0], b0 + d0[:, 1], a1 + d1[:, 0], b1 + d1[:, 1]
    kls["octave"][j, :NL] = loct
    kls["startPointX"][j, :NL], kls["startPointY"][j, :NL], kls["endPointX"][j, :NL], kls["endPointY"][j, :NL] = u0, v0, u1, v1
    s = np.stack([kls[k][j, :NL].astype(np.float64) for k in ("startPointX", "startPointY", "endPointX", "endPointY")], 1)
    le = np.stack([s[:, 1] - s[:, 3], s[:, 2] - s[:, 0], s[:, 0] * s[:, 3] - s[:, 1] * s[:, 2]], 1)          # sp x ep, src/Frame.cc:939-941
    lle[j, :NL] = le / np.sqrt(le[:, 0] ** 2 + le[:, 1] ** 2)[:, None]
    fml[j, lheld] = sum(len(w) for w in lworlds) + np.arange(len(lheld))
    lworlds.append(Ls)
    held_total[0] += len(held); held_total[1] += len(lheld)

tile = np.arange(B) % D
d = dict(kps=up(kps[tile].view(np.uint8).reshape(-1)), kls=up(kls[tile].view(np.uint8).reshape(-1)), counts=up(np.full(B, N, np.int32)), lcounts=up(np.full(B, NL, np.int32)),
         lle=up(lle[tile]), Tcw=up(Tcw[tile]), Tprev=up(Tprev[tile]), fmp=up(fmp[tile]), fml=up(fml[tile]), mpw=up(np.concatenate(worlds)), mlw=up(np.concatenate(lworlds)))
print(f"{args.config}: {B} frames ({D} distinct) of {N} key points / {NL} key lines at capacities {cap} / {lcap}; held per frame {held_total[0] / D:.0f} points, "
      f"{held_total[1] / D:.0f} lines", flush=True)
out = {}
run = lambda: pose.pose_optimization_with_line_batch(d["kps"], d["counts"], d["kls"], d["lcounts"], 1, d["lle"], d["Tcw"], (fx, fy, cx, cy), d["fmp"], d["mpw"], d["fml"],
                                                     d["mlw"], n_frames=B, Tcw_prev=d["Tprev"], out=out, context=ctx)
res = run()
torch.cuda.synchronize()
st, it, inl = res["status"].cpu().numpy(), res["iters"].cpu().numpy(), res["n_inliers"].cpu().numpy()
print(f"status 0 in {int((st == 0).sum())} frames, good in {int(res['good'].sum())}; evaluations per frame {it.sum(1).mean():.1f}; inliers per frame {inl[:, 0].mean():.0f} points, "
      f"{inl[:, 1].mean():.0f} lines", flush=True)
line = "%-44s %8.3f ms per call (%d frames; median of 5 windows of 10, HIP events; min %.3f max %.3f)"
t = windows(run)
print(line % ("olf_pose_optimization_with_line_batch_dev", t[0], B, t[1], t[2]), flush=True)
flags = [res["outlier_out"].clone(), res["outlier_l_out"].clone()]
held_rows, n_matches = [d["fmp"].clone(), d["fml"].clone()], torch.zeros((B, 2), dtype=torch.int32, device="cuda")
run_d = lambda: pose.discard_outliers_batch(d["counts"], d["lcounts"], 1, held_rows[0], held_rows[1], flags[0], flags[1], int(d["mpw"].shape[0]), int(d["mlw"].shape[0]), 1,
                                            False, False, out=n_matches, context=ctx)          # (mode 1 on a mono sensor changes no row: every call does the same work)
run_d()
t = windows(run_d)
print(line % ("olf_discard_outliers_batch_dev (mode 1)", t[0], B, t[1], t[2]), flush=True)
ctx.poll_status()
ctx.close()
