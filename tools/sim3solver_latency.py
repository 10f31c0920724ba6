"""Latency of the batched Sim3Solver (csrc/sim3solver_batch.hip) beside a loop of its host form, on fabricated loop candidates: every pair owns two key
frames that see --matches points under a similarity of its own (scale 0.5 to 2), --share of them inliers with up to 0.3 px of image noise, the others
displaced by tens of pixels; octaves over the context's levels.  One call is find(): a window of 300 over new solvers -- about the size of a BoW match
set, which is a supposition about real loads:  python tools/sim3solver_latency.py [--pairs 3072] [--matches 150] [--share 0.5] [--host-pairs 64]
Device entry: HIP events, warmed up, median of five windows of ten calls (the state is reset by a device copy inside the timed call).  Host loop: host
clock, on a sample of the pairs, results checked against the device's bit for bit."""
import argparse
import time
import numpy as np
import torch
from latency_common import side_stream, up, windows
from orb_line_slam_amd import _lib, sim3solver

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=3072)
ap.add_argument("--matches", type=int, default=150)
ap.add_argument("--share", type=float, default=0.5)
ap.add_argument("--features", type=int, default=2000, help="nfeatures of the context: its capacity is the row length")
ap.add_argument("--window", type=int, default=300)
ap.add_argument("--host-pairs", type=int, default=64)
args = ap.parse_args()
W, H, CAM = 640, 480, (400.0, 400.0, 320.0, 240.0)
p = _lib.default_params()
p.orb.nfeatures = args.features
ctx = _lib.Context(p, W, H, 2)
side_stream()
cap, P, N = ctx.orb_capacity, args.pairs, min(args.matches, ctx.orb_capacity)
sf = np.zeros(ctx.nlevels, np.float32)
_lib.lib().olf_orb_scale_tables(ctx.handle, sf.ctypes.data, None, None, None, None)
rng = np.random.default_rng(1)
f32 = np.float32

# frames 2k and 2k + 1 of pair k: identity poses, so world = camera coordinates; X1 = s R X2 + t
z = rng.uniform(2, 12, (P, N))
X1 = np.stack([(rng.uniform(40, W - 40, (P, N)) - CAM[2]) / CAM[0] * z, (rng.uniform(40, H - 40, (P, N)) - CAM[3]) / CAM[1] * z, z], 2)
axis = rng.normal(size=(P, 3))
axis /= np.linalg.norm(axis, axis=1, keepdims=True)
ang = np.radians(rng.uniform(2, 20, P))
K = np.zeros((P, 3, 3))
K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
Rm = np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
s, t = rng.choice([0.5, 1.0, 2.0], P), rng.uniform(-0.5, 0.5, (P, 3))
X2 = np.einsum("pnk,pkj->pnj", X1 - t[:, None], Rm) / s[:, None, None]
u, v = CAM[0] * X2[..., 0] / X2[..., 2] + CAM[2], CAM[1] * X2[..., 1] / X2[..., 2] + CAM[3]
rad = np.where(rng.random((P, N)) < args.share, rng.uniform(0, 0.3, (P, N)), rng.uniform(30, 80, (P, N)))
phi = rng.uniform(0, 2 * np.pi, (P, N))
u, v = u + rad * np.cos(phi), v + rad * np.sin(phi)
X2 = np.stack([(u - CAM[2]) / CAM[0] * X2[..., 2], (v - CAM[3]) / CAM[1] * X2[..., 2], X2[..., 2]], 2)
world = np.zeros((2 * P, cap, 3), f32)
world[0::2, :N], world[1::2, :N] = X1, X2
kps = np.zeros((2 * P, cap), _lib.KEYPOINT_DTYPE)
kps["octave"][:, :N] = rng.integers(0, ctx.nlevels, (2 * P, N))
counts = np.full(2 * P, N, np.int32)
Tcw = np.tile(np.eye(4, dtype=f32), (2 * P, 1, 1))
pairs = np.stack([2 * np.arange(P), 2 * np.arange(P) + 1], 1).astype(np.int32)
rows = np.full((P, cap), -1, np.int32)
rows[:, :N] = np.arange(N)
draws = sim3solver.sim3_draws(P, 300, 7)
rn = sim3solver.sim3_ransac(False, 0.99, 20, 300, args.window)
print(f"{P} pairs, {N} correspondences each, {100 * args.share:.0f} % inliers, capacity {cap}, window {args.window}", flush=True)

d_kps, d_counts, d_T, d_world = up(kps.view(np.uint8).reshape(2 * P, cap, -1)), up(counts), up(Tcw), up(world)
d_pairs, d_rows, d_draws = up(pairs), up(rows), up(draws.view(np.int32))
zero = sim3solver.sim3_state(P, cap, 300)
st = sim3solver.sim3_state(P, cap, 300)


def call():
    for k in ("iterations_done", "best_inliers"):
        st[k].copy_(zero[k])
    sim3solver.sim3_solver_batch(2 * P, d_kps, d_counts, d_T, d_world, CAM, d_pairs, d_rows, d_draws, st, rn, img_stride=1, context=ctx)


med, lo, hi = windows(call)
print("%-44s %8.3f ms per call (median; %.3f .. %.3f), %.2f us per pair" % ("olf_sim3_solver_pairs_dev", med, lo, hi, 1e3 * med / max(P, 1)), flush=True)
torch.cuda.synchronize()
ctx.poll_status()
dev = {k: v.cpu().numpy() for k, v in st.items()}
print("  accepted %d of %d; iterations per pair: mean %.1f, max %d" % (dev["accepted"].sum(), P, dev["iterations_done"].mean(), dev["iterations_done"].max()), flush=True)

sample = np.unique(np.linspace(0, P - 1, min(args.host_pairs, P)).astype(int)) if P else np.zeros(0, int)
host = sim3solver.sim3_state(len(sample), cap, 300, device=False)
t0 = time.perf_counter()
for r, q in enumerate(sample):
    a, b = pairs[q]
    sim3solver.Sim3Solve(kps[a:b + 1], counts[a:b + 1], Tcw[a:b + 1], world[a:b + 1], CAM, sf, (0, 1), rows[q], draws[q], host, rn, row=r)
dt = time.perf_counter() - t0
same = sum(int(all(np.array_equal(np.nan_to_num(host[k][r]), np.nan_to_num(dev[k][q])) for k in host)) for r, q in enumerate(sample))
print("%-44s %8.3f ms per pair (host clock, through the Python wrapper); %d of %d pairs identical to the batch entry" %
      ("loop of olf_sim3_solver", 1e3 * dt / max(len(sample), 1), same, len(sample)), flush=True)
assert same == len(sample), "the host form and the batch entry disagree"
ctx.close()
