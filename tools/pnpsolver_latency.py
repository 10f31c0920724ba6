"""Latency of the batched PnPsolver (csrc/pnpsolver_batch.hip) beside a loop of its host form, on fabricated relocalisation candidates: every pair owns a
key frame whose features hold --matches points and a lost frame that sees them under a pose of its own, --share of them noise-free inliers, the others
displaced by tens of pixels; octaves over the context's levels.  The batched call runs twice over new solvers: as find() (n_iterations 0: up to the cap)
and as the tracker's window of 5 -- which the reference's loop condition also runs up to the cap, so the two differ only beyond it; the size of a BoW
match set is a supposition about real loads:  python tools/pnpsolver_latency.py [--pairs 1024] [--matches 100] [--share 0.6] [--host-pairs 64]
Device entry: HIP events, warmed up, median of five windows of ten calls (the state is reset by a device copy inside the timed call).  Host loop: host
clock, on a sample of the pairs, results checked against the device's bit for bit."""
import argparse
import time
import numpy as np
import torch
from latency_common import side_stream, up, windows
from orb_line_slam_amd import _lib, pnpsolver

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1024)
ap.add_argument("--matches", type=int, default=100)
ap.add_argument("--share", type=float, default=0.6)
ap.add_argument("--features", type=int, default=1000, help="nfeatures of the context: its capacity is the row length")
ap.add_argument("--host-pairs", type=int, default=64)
args = ap.parse_args()
W, H, CAM = 640, 480, (400.0, 400.0, 320.0, 240.0)
MAX_ITS = 300
p = _lib.default_params()
p.orb.nfeatures = args.features
ctx = _lib.Context(p, W, H, 2)
side_stream()
cap, P, N = ctx.orb_capacity, args.pairs, min(args.matches, ctx.orb_capacity)
sf = np.zeros(ctx.nlevels, np.float32)
_lib.lib().olf_orb_scale_tables(ctx.handle, sf.ctypes.data, None, None, None, None)
rng = np.random.default_rng(1)
f32 = np.float32

# frames 2k (key frame) and 2k + 1 (lost frame) of pair k: Xc = R Xw + t
z = rng.uniform(2, 12, (P, N))
Xc = np.stack([(rng.uniform(40, W - 40, (P, N)) - CAM[2]) / CAM[0] * z, (rng.uniform(40, H - 40, (P, N)) - CAM[3]) / CAM[1] * z, z], 2)
axis = rng.normal(size=(P, 3))
axis /= np.linalg.norm(axis, axis=1, keepdims=True)
ang = np.radians(rng.uniform(2, 20, P))
K = np.zeros((P, 3, 3))
K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
Rm = np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
t = rng.uniform(-0.5, 0.5, (P, 3))
Xw = np.einsum("pnk,pkj->pnj", Xc - t[:, None], Rm).astype(f32)
Xc = np.einsum("pnj,pkj->pnk", Xw.astype(np.float64), Rm) + t[:, None]
u, v = CAM[0] * Xc[..., 0] / Xc[..., 2] + CAM[2], CAM[1] * Xc[..., 1] / Xc[..., 2] + CAM[3]
rad = np.where(rng.random((P, N)) < args.share, 0.0, rng.uniform(30, 80, (P, N)))
phi = rng.uniform(0, 2 * np.pi, (P, N))
world = np.zeros((2 * P, cap, 3), f32)
world[0::2, :N] = Xw
kps = np.zeros((2 * P, cap), _lib.KEYPOINT_DTYPE)
kps["octave"][:, :N] = rng.integers(0, ctx.nlevels, (2 * P, N))
kps["x"][1::2, :N], kps["y"][1::2, :N] = (u + rad * np.cos(phi)).astype(f32), (v + rad * np.sin(phi)).astype(f32)
counts = np.full(2 * P, N, np.int32)
pairs = np.stack([2 * np.arange(P), 2 * np.arange(P) + 1], 1).astype(np.int32)
rows = np.full((P, cap), -1, np.int32)
rows[:, :N] = np.arange(N)
draws = pnpsolver.pnp_draws(P, MAX_ITS, 7)
print(f"{P} pairs, {N} correspondences each, {100 * args.share:.0f} % inliers, capacity {cap}", flush=True)

d_kps, d_counts, d_world = up(kps.view(np.uint8).reshape(2 * P, cap, -1)), up(counts), up(world)
d_pairs, d_rows, d_draws = up(pairs), up(rows), up(draws.view(np.int32))
zero = pnpsolver.pnp_state(P, cap, MAX_ITS)
st = pnpsolver.pnp_state(P, cap, MAX_ITS)
sample = np.unique(np.linspace(0, P - 1, min(args.host_pairs, P)).astype(int)) if P else np.zeros(0, int)

for name, window in (("find()", 0), ("window of 5", 5)):
    rn = pnpsolver.pnp_ransac(max_iterations=MAX_ITS, n_iterations=window)

    def call():
        for k in ("iterations_done", "best_inliers", "refined_inliers"):
            st[k].copy_(zero[k])
        pnpsolver.pnp_solver_batch(2 * P, d_kps, d_counts, d_world, CAM, d_pairs, d_rows, d_draws, st, rn, img_stride=1, context=ctx)

    med, lo, hi = windows(call)
    print("%-44s %8.3f ms per call (median; %.3f .. %.3f), %.2f us per pair" % ("olf_pnp_solver_pairs_dev, " + name, med, lo, hi, 1e3 * med / max(P, 1)), flush=True)
    torch.cuda.synchronize()
    ctx.poll_status()
    dev = {k: v.cpu().numpy() for k, v in st.items()}
    print("  a pose for %d of %d; iterations per pair: mean %.1f, max %d" % (dev["accepted"].sum(), P, dev["iterations_done"].mean(), dev["iterations_done"].max()), flush=True)
    host = pnpsolver.pnp_state(len(sample), cap, MAX_ITS, device=False)
    t0 = time.perf_counter()
    for r, q in enumerate(sample):
        a, b = pairs[q]
        pnpsolver.PnPSolve(kps[a:b + 1], counts[a:b + 1], world[a:b + 1], CAM, sf, (0, 1), rows[q], draws[q], host, rn, row=r)
    dt = time.perf_counter() - t0
    # (best_flags, refined_flags, inliers, Tcw and counts keep what an earlier timed call left where this one writes nothing: compared where written)
    keys = ("iterations_done", "best_inliers", "best_Tcw", "refined_inliers", "refined_Tcw", "accepted", "no_more", "n_inliers", "n_correspondences")
    same = 0
    for r, q in enumerate(sample):
        ok = all(np.array_equal(np.nan_to_num(host[k][r]), np.nan_to_num(dev[k][q])) for k in keys)
        ok = ok and np.array_equal(host["inliers"][r, :N], dev["inliers"][q, :N])
        ok = ok and (not host["accepted"][r] or np.array_equal(host["Tcw"][r], dev["Tcw"][q]))
        done = min(int(host["iterations_done"][r]), MAX_ITS)
        ok = ok and np.array_equal(host["counts"][r, :done], dev["counts"][q, :done])
        same += int(ok)
    print("%-44s %8.3f ms per pair (host clock, through the Python wrapper); %d of %d pairs identical to the batch entry" %
          ("loop of olf_pnp_solver, " + name, 1e3 * dt / max(len(sample), 1), same, len(sample)), flush=True)
    assert same == len(sample), "the host form and the batch entry disagree"
ctx.close()
