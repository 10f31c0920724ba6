"""Latency of olf_keyframe_culling_tables_dev (csrc/culling_batch.hip: the data-parallel part of LocalMapping::KeyFrameCulling) on the map of
tests/localmap_scenes.py's large_scene -- by default 1500 key frames of up to 2000 slots and 150 000 points along a trajectory, with octaves, depths and
stereo flags drawn here -- with the `--listed` newest key frames listed (a covisibility list) and with every key frame listed; beside them the host time of
olf_keyframe_culling_replay on the downloaded tables, and olf_tracked_map_points_batch_dev and olf_map_point_culling_dev on the same map.
    python tools/culling_latency.py [--kfs 1500] [--points 150000] [--listed 32]
The device entries: HIP events, warmed up, median of five windows of ten calls.  The replay: the host clock, the median of five runs."""
import argparse, os, sys, time
import numpy as np
from latency_common import ROOT, side_stream, up, windows
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import localmap_scenes as S
from orb_line_slam_amd import CullView, MapGraph, _lib, culling

ap = argparse.ArgumentParser()
ap.add_argument("--kfs", type=int, default=1500)
ap.add_argument("--points", type=int, default=150000)
ap.add_argument("--listed", type=int, default=32)
args = ap.parse_args()
ctx = _lib.Context(_lib.default_params(), 320, 240, 2)
stream = side_stream()

t0 = time.perf_counter()
scene = S.large_scene(11, args.kfs, args.points, 1, 8)
graph = MapGraph(**scene.graph())
rng = np.random.default_rng(3)
slot_of = [{p: i for i, p in enumerate(r)} for r in scene.kf_mp]      # (large_scene puts a point into a key frame's row once, as it adds the observation)
stereo = [rng.random(len(r)) < 0.7 for r in scene.kf_mp]
view = CullView(graph, mp_obs_slot=[[slot_of[k][p] for k in r] for p, r in enumerate(scene.mp_obs)],
                mp_nobs=[sum(2 if stereo[k][slot_of[k][p]] else 1 for k in r) for p, r in enumerate(scene.mp_obs)],
                kf_slot_octave=[np.minimum(rng.geometric(0.45, len(r)) - 1, 7) for r in scene.kf_mp], kf_slot_depth=[rng.uniform(1, 50, len(r)) for r in scene.kf_mp],
                kf_slot_stereo=stereo, kf_th_depth=[35.0] * graph.n_kf, kf_mode=[2] + [0] * (graph.n_kf - 1))
print(f"scene: {graph.n_kf} key frames, {graph.n_mp} points, {len(graph.kf_mp_index)} slots ({len(graph.kf_mp_index) / graph.n_kf:.0f} per key frame), "
      f"{len(graph.mp_obs_kf) / graph.n_mp:.1f} observations per point; built in {time.perf_counter() - t0:.1f} s", flush=True)

for name, lst in (("the %d newest key frames listed" % args.listed, np.arange(graph.n_kf - 1, max(graph.n_kf - 1 - args.listed, -1), -1).astype(np.int32)),
                  ("all %d key frames listed" % graph.n_kf, None)):
    n = graph.n_kf if lst is None else len(lst)
    d_lst = None if lst is None else up(lst)
    cap = culling.listed_slots(graph, lst)
    out = {}
    run = lambda: culling.keyframe_culling_tables_batch(graph, view, d_lst, n_list=n, slot_capacity=cap, out=out, context=ctx)
    res = run()
    t_dev = windows(run)
    ctx.synchronize()
    tab = {k: v.cpu().numpy() for k, v in res.items()}
    print(f"{name}: {cap} slots, {int(tab['n_mps'].sum())} counted, {int(tab['n_redundant'].sum())} redundant, {int(tab['redundant'].sum())} key frames redundant as the map stands",
          flush=True)
    print("%-40s %8.3f ms per call (median of 5 windows of 10, HIP events; min %.3f max %.3f)" % (("olf_keyframe_culling_tables_dev",) + t_dev), flush=True)
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        rep = culling.keyframe_culling_replay(graph, view, lst, tab["n_mps"], tab["n_redundant"], tab["row_offsets"], tab["slot_count"], tab["slot_flags"])
        ms.append(1e3 * (time.perf_counter() - t0))
    print("%-40s %8.3f ms per call (host clock, median of 5; min %.3f max %.3f): %d culled, %d points went bad" %
          ("olf_keyframe_culling_replay", sorted(ms)[2], min(ms), max(ms), int((rep["decision"] == 1).sum()), len(rep["went_bad"])), flush=True)

d_nobs = up(view.mp_nobs)
ref = up(rng.integers(-1, graph.n_kf, 256).astype(np.int32))          # the reference key frames of a batch of 256 frames
tracked = {}
run_tracked = lambda: culling.tracked_map_points_batch(graph, d_nobs, ref, min_obs_points=3, out=tracked, context=ctx)
run_tracked()
print("%-40s %8.3f ms per call (256 key frames; median of 5 windows of 10, HIP events; min %.3f max %.3f)" % (("olf_tracked_map_points_batch_dev",) + windows(run_tracked)), flush=True)
n_recent = 4096
recent = [up(a) for a in ((rng.random(n_recent) < 0.1).astype(np.uint8), rng.integers(0, 40, n_recent).astype(np.int32), rng.integers(0, 40, n_recent).astype(np.int32),
                          rng.integers(0, 6, n_recent).astype(np.int32), rng.integers(0, 11, n_recent).astype(np.int64))]
action = torch.zeros(n_recent, dtype=torch.uint8, device="cuda")
run_mp = lambda: culling.map_point_culling(*recent, 10, False, out=action, context=ctx)
run_mp()
t_mp = windows(run_mp)
print("%-40s %8.3f ms per call (%d points; median of 5 windows of 10, HIP events; min %.3f max %.3f)" % ("olf_map_point_culling_dev", t_mp[0], n_recent, t_mp[1], t_mp[2]), flush=True)
ctx.poll_status()
ctx.close()
