"""Latency of the batched SearchLocalPoints (csrc/local_batch.hip: olf_search_local_map_batch_dev = isInFrustum + SearchByProjection(F, vpMapPoints, th))
beside the only other way to get its results -- a loop of olf_is_in_frustum + olf_search_local_map, two host calls per frame -- on the left frames of the
bench's synthetic batch.  The map is made of the batch's own stereo points (olf_unproject_stereo_dev, identity poses); frame j's local map is the points of
frames j - 1, j and j + 1, in that order; the frames hold nothing on entry; predicted pose: a 0.02 m translation; th = 1, nnratio = 0.8:
    python tools/local_map_latency.py [--config C3] [--pairs 3072]
Device entry: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise."""
import time
import numpy as np
from latency_common import BenchBatch, host_view, parser, up, zeros as z
import torch
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, matcher

ap = parser()
ap.add_argument("--host-frames", type=int, default=0, help="frames the host loop covers (0: all)")
ap.add_argument("--th", type=float, default=1.0)
ap.add_argument("--nnratio", type=float, default=0.8)
args = ap.parse_args()
batch = BenchBatch(args)
ctx, L, W, H, B, cap = batch.ctx, batch.L, batch.W, batch.H, batch.B, batch.cap
kps, desc, counts, ur = batch.kps, batch.desc, batch.counts, batch.ur
cam, bounds = batch.cam, batch.bounds
Tcw = batch.eye.clone()
Tcw[:, 0, 3] = 0.02
world, offs, idx = batch.world, batch.offs, batch.idx
batch.grid()
sf = batch.sf

# the map: point f * cap + i is the stereo point of feature i of frame f, as the frame that made it would describe it (MapPoint::UpdateNormalAndDepth)
torch.cuda.synchronize()
cnt, hk, hd, hu, hw, hz = batch.cnt, batch.hk, batch.hd, batch.hu, batch.hw.reshape(B * cap, 3), batch.dp.cpu().numpy()
dist = np.linalg.norm(hw.astype(np.float64), axis=1)
m_world = hw
m_normal = (hw / np.maximum(dist, 1e-9)[:, None]).astype(np.float32)
m_maxd = (dist * sf[np.clip(hk["octave"].reshape(-1), 0, ctx.nlevels - 1)] * 0.95).astype(np.float32)
m_mind = (m_maxd / sf[-1]).astype(np.float32)
m_desc = np.ascontiguousarray(hd.reshape(B * cap, 32))
m_obs, m_bad = np.ones(B * cap, np.uint8), np.zeros(B * cap, np.uint8)
own = [f * cap + np.flatnonzero(hz[f, :cnt[f]] > 0) for f in range(B)]
lists = [np.concatenate([own[f] for f in (j - 1, j, j + 1) if 0 <= f < B]).astype(np.int32) for j in range(B)]
l_offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
lm = matcher.LocalMapDev(up(m_world), up(m_normal), up(m_maxd), up(m_mind), up(m_desc), up(m_obs), up(m_bad), up(l_offs), up(np.concatenate(lists)), n_mp=B * cap)
out = (z((B, cap), torch.int32), z((B,), torch.int32))
search = lambda: matcher.search_local_map_batch(B, kps, desc, counts, ur, offs, idx, Tcw, lm, cam, bounds, th=args.th, nnratio=args.nnratio, out=out, context=ctx)
fr_out = (z((int(l_offs[-1]),), torch.uint8), z((int(l_offs[-1]),), torch.int32), z((int(l_offs[-1]),), torch.float32), z((int(l_offs[-1]), 3), torch.float32))
frustum = lambda: matcher.is_in_frustum_batch(B, Tcw, lm, cam, bounds, 0.5, out=fr_out, context=ctx)
frames_note = "%d frames; " % B
print(f"{args.config} {W}x{H}, {B} stereo pairs, capacity {cap}, th {args.th}, nnratio {args.nnratio}; map {B * cap} slots, {int(l_offs[-1])} list entries "
      f"({l_offs[-1] / B:.0f} per frame)", flush=True)
t_fr = batch.timed("olf_is_in_frustum_batch_dev (the frustum pass alone)", frustum, note=frames_note)
t_batch = batch.timed("olf_search_local_map_batch_dev", search, note=frames_note)
torch.cuda.synchronize()
n_dev, m_dev = out[1].cpu().numpy(), out[0].cpu().numpy()
print("  key points per frame: mean %.0f; matches per frame: mean %.1f, min %d, max %d; in view: %.1f %% of the entries" %
      (cnt.mean(), n_dev.mean(), n_dev.min(), n_dev.max(), 100.0 * float(fr_out[0].float().mean())), flush=True)

# the host entries, two calls per frame, on the downloaded arrays (each frame's local map gathered beforehand)
hT = Tcw.cpu().numpy()
nh = min(args.host_frames or B, B)
views, held, maps = [], [], []
for j in range(nh):
    n = int(cnt[j])
    held.append((np.zeros(n, bool), np.zeros(n, bool)))      # mp_valid, mp_obs: the search marks the features it fills
    views.append(host_view(batch, j, mvuRight=hu[j, :n], mTcw=hT[j], mp_valid=held[j][0], mp_obs=held[j][1], mp_bad=np.zeros(n, bool), mvbOutlier=np.zeros(n, bool),
                           mp_world=np.zeros((n, 3), np.float32), mp_desc=hd[j, :n]))
    li = lists[j]
    a = np.ascontiguousarray
    maps.append(dict(n=len(li), world=a(m_world[li]), normal=a(m_normal[li]), maxd=a(m_maxd[li]), mind=a(m_mind[li]), desc=a(m_desc[li]), obs=a(m_obs[li]),
                     bad=a(m_bad[li]), inv=np.zeros(len(li), np.uint8), lvl=np.zeros(len(li), np.int32), cos=np.zeros(len(li), np.float32),
                     proj=np.zeros((len(li), 3), np.float32)))
hm, hn = np.full((nh, cap), -1, np.int32), np.zeros(nh, np.int32)
p = lambda x: x.ctypes.data


def host_frame(j):
    q = maps[j]
    rc = L.olf_is_in_frustum(views[j], q["n"], p(q["world"]), p(q["normal"]), p(q["maxd"]), p(q["mind"]), 0.5, p(q["inv"]), p(q["lvl"]), p(q["cos"]), p(q["proj"]))
    assert rc == 0, _lib.last_error()
    rc = L.olf_search_local_map(ctx.handle, views[j], q["n"], p(q["inv"]), p(q["bad"]), p(q["lvl"]), p(q["cos"]), p(q["proj"]), p(q["desc"]), p(q["obs"]), args.th,
                                args.nnratio, hm[j].ctypes.data, hn[j:].ctypes.data)
    assert rc == 0, _lib.last_error()


host_frame(0)                                             # warm
held[0][0][:], held[0][1][:] = False, False
torch.cuda.synchronize()
t0 = time.perf_counter()
for j in range(nh):
    host_frame(j)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
same = 0
for j in range(nh):
    mm = np.where(hm[j] >= 0, lists[j][np.maximum(hm[j], 0)], -1) if len(lists[j]) else hm[j]      # list positions -> map indices
    same += int(hn[j] == n_dev[j] and np.array_equal(mm, m_dev[j]))
print("%-58s %8.3f ms per frame, %.1f ms for %d frames (host clock, arrays already on the host); %d of %d frames identical to the batch entry" %
      ("loop of olf_is_in_frustum + olf_search_local_map", 1e3 * dt / nh, 1e3 * dt, nh, same, nh), flush=True)
print("  batch entry per frame: %.4f ms; ratio loop / batch over %d frames: %.1f" % (t_batch / B, nh, (1e3 * dt / nh) / (t_batch / B)), flush=True)

# candidate statistics of a sample of frames: the windows of the entries in view on the frame's grid
lens = []
for j in np.linspace(0, nh - 1, min(nh, 32)).astype(int):
    q = maps[j]
    ok = q["inv"].astype(bool)
    qs = np.zeros(int(ok.sum()), _lib.AREA_QUERY_DTYPE)
    r = np.where(q["cos"][ok] > 0.998, np.float32(2.5), np.float32(4.0))
    if args.th != 1.0:
        r = r * np.float32(args.th)
    qs["x"], qs["y"], qs["r"] = q["proj"][ok, 0], q["proj"][ok, 1], r * sf[q["lvl"][ok]]
    qs["min_level"], qs["max_level"] = q["lvl"][ok] - 1, q["lvl"][ok]
    keys = hk[j, :int(cnt[j])]
    g = ola.assign_features_to_grid(keys, bounds, context=ctx)
    co, _ = ola.features_in_area(keys, g, bounds, qs, context=ctx)
    lens.append(np.diff(co))
lens = np.concatenate(lens)
print("  candidate lists (%d entries in view of %d sampled frames): mean %.2f, median %d, p99 %d, max %d, empty %.1f %%, longer than 4: %.1f %%, longer than 64: %d" %
      (len(lens), min(nh, 32), lens.mean(), np.median(lens), np.percentile(lens, 99), lens.max(), 100.0 * (lens == 0).mean(), 100.0 * (lens > 4).mean(),
       int((lens > 64).sum())), flush=True)
ctx.close()
