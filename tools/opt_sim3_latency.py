"""Pairs per second of olf_optimize_sim3_pairs_dev (csrc/optsim3_batch.hip: Optimizer::OptimizeSim3, one workgroup per key-frame pair) at 1 and 1024 pairs
of 20 / 100 / 300 correspondences, and the host form's (olf_optimize_sim3) time for the same pairs.  The context has nfeatures = 2000 by default (a
capacity at which a pair's 69 bytes per feature do not fit the 60 KB of LDS a workgroup takes, so the correspondences live in the batch scratch slot);
--nfeatures 700 gives a capacity whose slab fits and measures the LDS path.  The pairs are synthetic (no image is read): kf2 points at 2-15 m, a
similarity of scale 1.3 with a translation of up to a metre, both images observed with half a pixel of noise times the level's scale, one gross outlier in
ten, a start a few centimetres, a degree and 2 % of scale off.  --distinct different pairs are tiled over the list.  The entry nulls outliers in the match
rows it is given, so every timed call first restores the rows with one device copy, which is inside the measured time.
    python tools/opt_sim3_latency.py [--distinct 16] [--host-pairs 8] [--nfeatures 2000]
HIP events, warmed up, median of five windows of ten calls; the host form by the host clock over --host-pairs pairs."""
import math
import time
import numpy as np
from latency_common import parser, side_stream, up, windows
import torch
from orb_line_slam_amd import _lib, optsim3
from orb_line_slam_amd._lib import KEYPOINT_DTYPE

ap = parser()
ap.set_defaults(distinct=16)
ap.add_argument("--host-pairs", type=int, default=8)
ap.add_argument("--nfeatures", type=int, default=2000)
args = ap.parse_args()
W, H, fx = 1241, 376, 718.856
cx, cy = W / 2.0, H / 2.0
params = _lib.default_params()
params.orb.nfeatures = args.nfeatures
ctx = _lib.Context(params, W, H, 2)          # (the entry reads no image: the context gives the capacity and the level table)
side_stream()
cap, nlev = ctx.orb_capacity, ctx.nlevels
sf, sig = np.zeros(nlev, np.float32), np.zeros(nlev, np.float32)
_lib.lib().olf_orb_scale_tables(ctx.handle, sf.ctypes.data, None, None, sig.ctypes.data, None)
rng = np.random.default_rng(79)
print(f"capacity {cap} ({'LDS' if 69 * cap + 64 <= 60 * 1024 else 'scratch-slot'} path); clocks as the machine leaves them (not pinned)", flush=True)


def rot(r):
    a = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / a
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def se3(r, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(r), t
    return T


def pairs_of(D, n):
    """D pairs on 2 D frames: frame 2 j is kf1, 2 j + 1 is kf2; feature i of kf1 matches feature n - 1 - i of kf2"""
    kps, Tcw, world = np.zeros((2 * D, cap), KEYPOINT_DTYPE), np.zeros((2 * D, 16), np.float32), np.zeros((2 * D, cap, 3), np.float32)
    rows, s12, R12, t12 = np.full((D, cap), -1, np.int32), np.zeros(D, np.float32), np.zeros((D, 9), np.float32), np.zeros((D, 3), np.float32)
    for j in range(D):
        T1, T2 = se3(rng.uniform(-0.2, 0.2, 3), rng.uniform(-1, 1, 3)), se3(rng.uniform(-0.2, 0.2, 3), rng.uniform(-1, 1, 3))
        Tcw[2 * j], Tcw[2 * j + 1] = T1.astype(np.float32).reshape(16), T2.astype(np.float32).reshape(16)
        R, t, s = rot(rng.uniform(-0.1, 0.1, 3)), rng.uniform(-1, 1, 3), 1.3
        u, v, z = rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n), rng.uniform(2, 15, n)
        X2 = np.stack([(u - cx) * z / fx, (v - cy) * z / fx, z], 1)
        X1 = s * X2 @ R.T + t
        o1, o2 = rng.integers(0, nlev, n), rng.integers(0, nlev, n)
        e1, e2 = rng.normal(0, 1, (n, 2)) * (0.5 * sf[o1])[:, None], rng.normal(0, 1, (n, 2)) * (0.5 * sf[o2])[:, None]
        gross = rng.random(n) < 0.1
        e2[gross] += rng.choice([-1.0, 1.0], (int(gross.sum()), 2)) * rng.uniform(20, 60, (int(gross.sum()), 2))
        back = n - 1 - np.arange(n)
        T1i, T2i = np.linalg.inv(T1), np.linalg.inv(T2)
        world[2 * j, :n], world[2 * j + 1, back] = X1 @ T1i[:3, :3].T + T1i[:3, 3], X2 @ T2i[:3, :3].T + T2i[:3, 3]
        kps["x"][2 * j, :n], kps["y"][2 * j, :n], kps["octave"][2 * j, :n] = cx + fx * X1[:, 0] / X1[:, 2] + e1[:, 0], cy + fx * X1[:, 1] / X1[:, 2] + e1[:, 1], o1
        kps["x"][2 * j + 1, back], kps["y"][2 * j + 1, back], kps["octave"][2 * j + 1, back] = u + e2[:, 0], v + e2[:, 1], o2
        rows[j, :n] = back
        dR = rot(rng.normal(size=3) * math.radians(1.0) / math.sqrt(3))
        s12[j], R12[j], t12[j] = 1.02 * s, (dR @ R).astype(np.float32).reshape(9), (1.02 * dR @ t + rng.normal(size=3) * 0.02).astype(np.float32)
    return kps, Tcw, world, rows, s12, R12, t12


line = "%-34s %5d pairs of %4d corr.: %9.3f ms per call, %10.0f pairs/s (median of 5 windows of 10, HIP events; min %.3f max %.3f ms)"
cam = (fx, fx, cx, cy)
for n in (20, 100, 300):
    D = args.distinct
    n = min(n, cap)
    kps, Tcw, world, rows, s12, R12, t12 = pairs_of(D, n)
    d_kps, d_counts, d_T, d_world = up(kps.view(np.uint8).reshape(-1)), up(np.full(2 * D, n, np.int32)), up(Tcw), up(world)
    for B in (1, 1024):
        tile = np.arange(B) % D
        pr = np.stack([2 * tile, 2 * tile + 1], 1).astype(np.int32)
        d_pairs, d_rows0, d_s, d_R, d_t = up(pr), up(rows[tile]), up(s12[tile]), up(R12[tile]), up(t12[tile])
        d_rows = d_rows0.clone()
        out = optsim3.optimize_sim3_state(B, cap)

        def run():
            d_rows.copy_(d_rows0)
            return optsim3.optimize_sim3_batch(2 * D, d_kps, d_counts, d_T, d_world, cam, d_pairs, d_rows, d_s, d_R, d_t, th2=10.0, fix_scale=False, img_stride=1, out=out, context=ctx)

        res = run()
        torch.cuda.synchronize()
        if B == 1024:
            it, st = res["iters"].cpu().numpy(), res["status"].cpu().numpy()
            print(f"  {n} correspondences: status 0 in {int((st == 0).sum())} of {B} pairs, Levenberg iterations per pair {it.sum(1).mean():.1f}, "
                  f"inliers per pair {res['n_inliers'].float().mean().item():.0f}, nBad {res['n_bad_first'].float().mean().item():.1f}", flush=True)
        t = windows(run)
        print(line % ("olf_optimize_sim3_pairs_dev", B, n, t[0], 1e3 * B / t[0], t[1], t[2]), flush=True)
    k = min(args.host_pairs, D)
    if k <= 0:
        continue
    t0 = time.perf_counter()
    for j in range(k):
        optsim3.OptimizeSim3(kps[2 * j:2 * j + 2], np.full(2, n, np.int32), Tcw[2 * j:2 * j + 2].reshape(2, 4, 4), world[2 * j:2 * j + 2], cam, sig, (0, 1), rows[j].copy(),
                             s12[j], R12[j], t12[j], th2=10.0, fix_scale=False)
    dt = (time.perf_counter() - t0) / k
    print(f"{'olf_optimize_sim3 (host form)':34s} {k:5d} pairs of {n:4d} corr.: {1e3 * dt:9.3f} ms per pair, {1 / dt:10.0f} pairs/s (host clock, wrapper included)", flush=True)
ctx.poll_status()
ctx.close()
