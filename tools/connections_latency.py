"""Latency of olf_update_connections_batch_dev (csrc/connections_batch.hip: KeyFrame::UpdateConnections for a list of key frames) on the map of
tests/localmap_scenes.py's large_scene -- by default 1500 key frames of up to 2000 slots and 150 000 points along a trajectory -- with every key frame listed
and with 32 listed, and of olf_best_covisibles_batch_dev on the rows the first run leaves.  For orientation, beside them, the host time of the same walk with
the reference's data structures (tools/connections_host_walk.cpp: std::map observations copied per point, a std::map KFcounter; compiled -O3 here, one host
thread), whose ordered rows' lengths and weights are compared with the device's.
    python tools/connections_latency.py [--kfs 1500] [--points 150000] [--listed 32] [--th 15]
The device entries: HIP events, warmed up, median of five windows of ten calls.  The host walk: the host clock, the median of five runs."""
import argparse, ctypes, os, subprocess, sys, tempfile, time
import numpy as np
from latency_common import ROOT, side_stream, up, windows
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import localmap_scenes as S
from orb_line_slam_amd import MapGraph, _lib, connections

ap = argparse.ArgumentParser()
ap.add_argument("--kfs", type=int, default=1500)
ap.add_argument("--points", type=int, default=150000)
ap.add_argument("--listed", type=int, default=32)
ap.add_argument("--th", type=int, default=connections.OLF_COVIS_TH)
args = ap.parse_args()
ctx = _lib.Context(_lib.default_params(), 320, 240, 2)
stream = side_stream()

t0 = time.perf_counter()
scene = S.large_scene(11, args.kfs, args.points, 1, 8)
scene.kf_covis = [[] for _ in range(args.kfs)]                       # (yet to be computed)
graph = MapGraph(**scene.graph())
print(f"scene: {graph.n_kf} key frames, {graph.n_mp} points, {len(graph.kf_mp_index)} slots ({len(graph.kf_mp_index) / graph.n_kf:.0f} per key frame), "
      f"{len(graph.mp_obs_kf) / graph.n_mp:.1f} observations per point; built in {time.perf_counter() - t0:.1f} s", flush=True)

tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "libconnections_host_walk.so")
subprocess.run(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "connections_host_walk.cpp")], check=True)
hw = ctypes.CDLL(so)
hw.cw_create.restype = ctypes.c_void_p
hw.cw_create.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5
hw.cw_destroy.argtypes = [ctypes.c_void_p]
hw.cw_update_connections.restype = ctypes.c_long
hw.cw_update_connections.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_long)]
host_map = hw.cw_create(graph.n_kf, graph.n_mp, *(_lib.ptr(getattr(graph, k)) for k in ("mp_obs_offsets", "mp_obs_kf", "mp_bad", "kf_mp_offsets", "kf_mp_index")))

rng = np.random.default_rng(5)
for name, lst in (("all %d key frames listed" % graph.n_kf, None), ("%d listed" % args.listed, np.sort(rng.choice(graph.n_kf, min(args.listed, graph.n_kf), replace=False)).astype(np.int32))):
    n = graph.n_kf if lst is None else len(lst)
    d_lst = None if lst is None else up(lst)
    res = connections.update_connections_batch(graph, d_lst, n_list=n, th=args.th, capacities=(0, 0), context=ctx)      # a first call sizes the lists
    torch.cuda.synchronize()
    caps = [int(res[k + "_offsets"][n].item()) for k in ("conn", "covis")]
    try:
        ctx.poll_status()
    except _lib.OlfError:
        pass                                                         # (the capacity flag of the sizing call)
    out = {}
    run = lambda: connections.update_connections_batch(graph, d_lst, n_list=n, th=args.th, capacities=caps, out=out, context=ctx)
    res = run()
    t_dev = windows(run)
    ctx.synchronize()
    print(f"{name}: {caps[0]} connected entries ({caps[0] / n:.1f} per key frame), {caps[1]} ordered entries ({caps[1] / n:.1f}), th = {args.th}", flush=True)
    print("%-40s %8.3f ms per call (median of 5 windows of 10, HIP events; min %.3f max %.3f)" % (("olf_update_connections_batch_dev",) + t_dev), flush=True)
    host_list = np.arange(graph.n_kf, dtype=np.int32) if lst is None else lst
    ms, chk = [], ctypes.c_long(0)
    for _ in range(5):
        t0 = time.perf_counter()
        total = hw.cw_update_connections(host_map, _lib.ptr(host_list), n, args.th, ctypes.byref(chk))
        ms.append(1e3 * (time.perf_counter() - t0))
    same = total == caps[1] and chk.value == int(res["covis_weight"][:caps[1]].sum().item())
    print("%-40s %8.3f ms per call (host clock, median of 5; min %.3f max %.3f); ordered rows %s the device's" % ("std::map walk, one host thread", sorted(ms)[2], min(ms), max(ms),
                                                                                                                "equal" if same else "DIFFER FROM"), flush=True)
    if lst is None:
        best = {}
        run_best = lambda: connections.best_covisibles_batch(res["conn_offsets"], res["conn_index"], res["conn_weight"], n_rows=n, out=best, context=ctx)
        run_best()
        t_best = windows(run_best)
        ctx.synchronize()
        print("%-40s %8.3f ms per call (median of 5 windows of 10, HIP events; min %.3f max %.3f)" % (("olf_best_covisibles_batch_dev",) + t_best), flush=True)
hw.cw_destroy(host_map)
ctx.poll_status()
ctx.close()
