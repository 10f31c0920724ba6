"""Latency of olf_update_local_map_batch_dev (csrc/localmap_batch.hip: Tracking::UpdateLocalMap for a batch of frames) beside the call it feeds,
olf_search_local_map_batch_dev, on one synthetic batch: tests/localmap_scenes.py's large_scene -- by default 256 frames of 2000 features, about 70 % of
which hold a map point, against a map of 1500 key frames of up to 2000 slots and 150 000 points along a trajectory.  The frames' key points and descriptors
and the map points' positions and descriptors are random (identity poses, points spread through the frustum), so the search does its frustum pass, its grid
walks and its distances, and matches little.
    python tools/localmap_latency.py [--frames 256] [--features 2000] [--kfs 1500] [--points 150000]
Both entries: HIP events, warmed up, median of five windows of ten calls.  The lists the search reads are the device outputs of the first entry."""
import argparse, os, sys, time
import numpy as np
from latency_common import ROOT, side_stream, up, windows
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import localmap_scenes as S
from orb_line_slam_amd import MapGraph, _lib, localmap, matcher
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, check, lib

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--features", type=int, default=2000)
ap.add_argument("--kfs", type=int, default=1500)
ap.add_argument("--points", type=int, default=150000)
args = ap.parse_args()
B, N = args.frames, args.features
W, H = 640, 480
p = _lib.default_params()
p.orb.nfeatures = N
ctx = _lib.Context(p, W, H, 2)
cap = ctx.orb_capacity
stream = side_stream()
rng = np.random.default_rng(7)
f32 = np.float32

t0 = time.perf_counter()
scene = S.large_scene(11, args.kfs, args.points, B, N)
graph = MapGraph(**scene.graph())
print(f"scene: {graph.n_kf} key frames, {graph.n_mp} points, {len(graph.kf_mp_index)} slots ({len(graph.kf_mp_index) / graph.n_kf:.0f} per key frame), "
      f"{len(graph.mp_obs_kf) / graph.n_mp:.1f} observations per point; built in {time.perf_counter() - t0:.1f} s", flush=True)
fmp = np.full((B, cap), -1, np.int32)
fmp[:, :N] = np.asarray(scene.frame_mp, np.int32)
d_fmp, d_cnt = up(fmp), up(np.full(B, N, np.int32))

# ---- UpdateLocalMap: a first call sizes the lists
res = localmap.update_local_map_batch(graph, B, d_fmp, d_cnt, capacities=(0, 0, 0), context=ctx)
torch.cuda.synchronize()
caps = [int(res[k + "_offsets"][B].item()) for k in ("kf", "mp", "ml")]
try:
    ctx.poll_status()
except _lib.OlfError:
    pass                                                             # (the capacity flag of the sizing call)
out = {}
run = lambda: localmap.update_local_map_batch(graph, B, d_fmp, d_cnt, capacities=caps, out=out, context=ctx)
res = run()
t_update = windows(run)
ctx.synchronize()
nk = np.diff(res["kf_offsets"].cpu().numpy())
npnt = np.diff(res["mp_offsets"].cpu().numpy())
print(f"{B} frames of {N} features ({(fmp >= 0).sum() / B:.0f} held points each): local key frames per frame mean {nk.mean():.1f} (min {nk.min()}, max {nk.max()}), "
      f"local points per frame mean {npnt.mean():.0f} (min {npnt.min()}, max {npnt.max()}), {caps[1]} list entries", flush=True)
print("%-40s %8.3f ms per call (median of 5 windows of 10, HIP events; min %.3f max %.3f)" % (("olf_update_local_map_batch_dev",) + t_update), flush=True)

# ---- the search the lists feed: random frames and random map geometry
kps = np.zeros((B, cap), KEYPOINT_DTYPE)
kps["x"][:, :N], kps["y"][:, :N] = rng.uniform(8, W - 8, (B, N)), rng.uniform(8, H - 8, (B, N))
kps["octave"][:, :N] = rng.integers(0, 8, (B, N))
kps["size"], kps["class_id"] = 31, -1
desc = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
d_kps, d_desc, d_ur = up(kps.view(np.uint8).reshape(B, cap, 28)), up(desc), up(np.full((B, cap), -1, f32))
FX, CX, CY, MBF = 450.0, W / 2.0, H / 2.0, 45.0
cam, bounds = (FX, FX, CX, CY, MBF), (0.0, float(W), 0.0, float(H))
offs, idx = torch.zeros((B, _lib.GRID_CELLS + 1), dtype=torch.int32, device="cuda"), torch.zeros((B, cap), dtype=torch.int32, device="cuda")
check(lib().olf_frame_grid_dev(ctx.handle, B, 1, d_kps.data_ptr(), d_cnt.data_ptr(), *bounds, offs.data_ptr(), idx.data_ptr(), stream), "olf_frame_grid_dev")
sf = np.zeros(ctx.nlevels, f32)
lib().olf_orb_scale_tables(ctx.handle, sf.ctypes.data, None, None, None, None)
n_mp = graph.n_mp
z = rng.uniform(2, 20, n_mp)
world = np.stack([(rng.uniform(-40, W + 40, n_mp) - CX) * z / FX, (rng.uniform(-40, H + 40, n_mp) - CY) * z / FX, z], 1)
dist = np.linalg.norm(world, axis=1)
lm = matcher.LocalMapDev(up(world.astype(f32)), up((world / dist[:, None]).astype(f32)), up((dist * sf[rng.integers(0, 8, n_mp)] * 0.95).astype(f32)),
                         up((dist * 0.95 / sf[-1]).astype(f32)), up(rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)), up(np.ones(n_mp, np.uint8)),
                         up(graph.mp_bad), res["mp_offsets"], res["mp_index"], n_mp=n_mp)
Tcw = torch.eye(4, dtype=torch.float32, device="cuda").repeat(B, 1, 1).contiguous()
s_out = (torch.zeros((B, cap), dtype=torch.int32, device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda"))
search = lambda: matcher.search_local_map_batch(B, d_kps, d_desc, d_cnt, d_ur, offs, idx, Tcw, lm, cam, bounds, th=1.0, nnratio=0.8, frame_mp=res["frame_mp"],
                                                img_stride=1, out=s_out, context=ctx)
t_search = windows(search)
ctx.synchronize()
print("%-40s %8.3f ms per call (median of 5 windows of 10, HIP events; min %.3f max %.3f)" % (("olf_search_local_map_batch_dev",) + t_search), flush=True)
print(f"  matches per frame: mean {s_out[1].float().mean().item():.1f}; building the lists / searching them: {t_update[0] / t_search[0]:.2f}", flush=True)
ctx.close()
