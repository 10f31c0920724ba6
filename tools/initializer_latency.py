"""Latency of the batched Initializer (csrc/initializer_batch.hip) beside a loop of its host form, on fabricated initialisation attempts: every pair owns a
reference frame and a current frame that see --matches common points of a general scene under a motion of its own (a small rotation, a sideways
translation), a tenth of a pixel of noise, --outliers of the matches wrong; both frames carry a few unmatched key points more.  The size of a match set
after SearchForInitialization is a supposition about real loads:
    python tools/initializer_latency.py [--pairs 1024] [--matches 300] [--outliers 0.1] [--host-pairs 32] [--iterations 200]
Device entry: HIP events, warmed up, median of five windows of calls.  Host loop: host clock, on a sample of the pairs, results checked against the
device's bit for bit."""
import argparse
import time
import numpy as np
import torch
from latency_common import side_stream, up, windows
from orb_line_slam_amd import _lib, initializer

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1024)
ap.add_argument("--matches", type=int, default=300)
ap.add_argument("--outliers", type=float, default=0.1)
ap.add_argument("--iterations", type=int, default=200)
ap.add_argument("--features", type=int, default=448, help="nfeatures of the context: its capacity is the row length")
ap.add_argument("--host-pairs", type=int, default=32)
args = ap.parse_args()
W, H, CAM = 640, 480, (500.0, 500.0, 320.0, 240.0)
p = _lib.default_params()
p.orb.nfeatures = args.features
ctx = _lib.Context(p, W, H, 2)
side_stream()
cap, P = ctx.orb_capacity, args.pairs
N = min(args.matches, cap - 20)
N1, N2 = N + 20, N + 12
rng = np.random.default_rng(1)
f32 = np.float32

# frames 2k (reference) and 2k + 1 (current) of pair k
z = rng.uniform(4, 12, (P, N))
X = np.stack([rng.uniform(-3, 3, (P, N)), rng.uniform(-2, 2, (P, N)), z], 2)
ang = rng.uniform(-0.05, 0.05, (P, 3))
t = np.stack([rng.uniform(0.4, 0.8, P) * rng.choice([-1, 1], P), rng.uniform(-0.1, 0.1, P), rng.uniform(-0.15, 0.15, P)], 1)
cx_, sx_, cy_, sy_, cz_, sz_ = np.cos(ang[:, 0]), np.sin(ang[:, 0]), np.cos(ang[:, 1]), np.sin(ang[:, 1]), np.cos(ang[:, 2]), np.sin(ang[:, 2])
Rm = np.zeros((P, 3, 3))
Rm[:, 0] = np.stack([cz_ * cy_, cz_ * sy_ * sx_ - sz_ * cx_, cz_ * sy_ * cx_ + sz_ * sx_], 1)
Rm[:, 1] = np.stack([sz_ * cy_, sz_ * sy_ * sx_ + cz_ * cx_, sz_ * sy_ * cx_ - cz_ * sx_], 1)
Rm[:, 2] = np.stack([-sy_, cy_ * sx_, cy_ * cx_], 1)
Xc = np.einsum("pnj,pkj->pnk", X, Rm) + t[:, None]
kps = np.zeros((2 * P, cap), _lib.KEYPOINT_DTYPE)
kps["x"], kps["y"], kps["class_id"] = rng.uniform(20, W - 20, (2 * P, cap)), rng.uniform(20, H - 20, (2 * P, cap)), -1
u2, v2 = CAM[0] * Xc[..., 0] / Xc[..., 2] + CAM[2] + rng.normal(0, 0.1, (P, N)), CAM[1] * Xc[..., 1] / Xc[..., 2] + CAM[3] + rng.normal(0, 0.1, (P, N))
wrong = rng.random((P, N)) < args.outliers
u2, v2 = np.where(wrong, rng.uniform(20, W - 20, (P, N)), u2), np.where(wrong, rng.uniform(20, H - 20, (P, N)), v2)
kps["x"][0::2, :N], kps["y"][0::2, :N] = CAM[0] * X[..., 0] / z + CAM[2] + rng.normal(0, 0.1, (P, N)), CAM[1] * X[..., 1] / z + CAM[3] + rng.normal(0, 0.1, (P, N))
kps["x"][1::2, :N], kps["y"][1::2, :N] = u2[:, ::-1], v2[:, ::-1]      # current feature N - 1 - q sees what reference feature q sees
counts = np.tile(np.array([N1, N2], np.int32), P)
pairs = np.stack([2 * np.arange(P), 2 * np.arange(P) + 1], 1).astype(np.int32)
rows = np.full((P, cap), -1, np.int32)
rows[:, :N] = N - 1 - np.arange(N)
prm = initializer.initializer_params(max_iterations=args.iterations)
draws = initializer.initializer_draws(P, args.iterations, 7)
print(f"{P} pairs, {N} correspondences each ({100 * args.outliers:.0f} % wrong), {N1} and {N2} key points, {args.iterations} iterations, capacity {cap}", flush=True)

d_kps, d_counts = up(kps.view(np.uint8).reshape(2 * P, cap, -1)), up(counts)
d_pairs, d_rows, d_draws = up(pairs), up(rows), up(draws.view(np.int32))
st = initializer.initializer_state(P, cap)


def call():
    initializer.initializer_batch(2 * P, d_kps, d_counts, CAM, d_pairs, d_rows, d_draws, st, prm, img_stride=1, context=ctx)


med, lo, hi = windows(call)
print("%-36s %9.3f ms per call (median; %.3f .. %.3f), %.2f us per pair" % ("olf_initializer_pairs_dev", med, lo, hi, 1e3 * med / max(P, 1)), flush=True)
torch.cuda.synchronize()
ctx.poll_status()
dev = {k: v.cpu().numpy() for k, v in st.items()}
print("  initialised %d of %d; model F for %d, H for %d" % ((dev["ok"] == 1).sum(), P, (dev["model"] == 2).sum(), (dev["model"] == 1).sum()), flush=True)
sample = np.unique(np.linspace(0, P - 1, min(args.host_pairs, P)).astype(int)) if P else np.zeros(0, int)
host = initializer.initializer_state(len(sample), cap, device=False)
t0 = time.perf_counter()
for r, q in enumerate(sample):
    a, b = pairs[q]
    initializer.Initialize(kps[a:b + 1], counts[a:b + 1], CAM, (0, 1), rows[q], draws[q], host, prm, row=r)
dt = time.perf_counter() - t0
same = 0
for r, q in enumerate(sample):
    keys = [k for k in host if k not in ("R21", "t21", "P3D", "triangulated")] + (["R21", "t21", "P3D", "triangulated"] if host["ok"][r] == 1 else [])
    same += int(all(np.array_equal(np.ascontiguousarray(host[k][r]).view(np.uint8), np.ascontiguousarray(dev[k][q]).view(np.uint8)) for k in keys))
print("%-36s %9.3f ms per pair (host clock, through the Python wrapper); %d of %d pairs identical to the batch entry" %
      ("loop of olf_initializer", 1e3 * dt / max(len(sample), 1), same, len(sample)), flush=True)
assert same == len(sample), "the host form and the batch entry disagree"
ctx.close()
