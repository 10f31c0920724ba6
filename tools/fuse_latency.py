"""Latency of the batched Fuse search (csrc/fuse_batch.hip) beside the only other way to get its results -- a loop of olf_fuse_search /
olf_fuse_search_sim3, one host call per key frame, with the views and the map already on the host -- on the left frames of the bench's synthetic
batch: the map is the batch's own stereo points (olf_unproject_stereo_dev, identity poses), frame j's list holds the stereo points of frames j - 1, j
and j + 1, and a frame holds its own points, so a third of its list is skipped as held; th = 3; both forms (the Sim3 poses are 1.25 * identity):
  python tools/fuse_latency.py [--config C3] [--pairs 3072] [--host-frames 64]
Device entry: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise.  The sampled frames' host
results are compared with the batch rows; a mismatch ends the tool with a non-zero status."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import torch
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, matcher, synth
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, check, lib
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--pairs", type=int, default=0, help="stereo pairs = key frames of the batch (0: the configuration's default)")
ap.add_argument("--distinct", type=int, default=512)
ap.add_argument("--host-frames", type=int, default=64, help="key frames, evenly spread over the batch, the host loop covers")
args = ap.parse_args()
cfg = bench.CONFIGS[args.config]
W, H, B = cfg["w"], cfg["h"], args.pairs or cfg["pairs"]
params = _lib.default_params()
params.orb.nfeatures, params.line.lsd_nfeatures = cfg["nf"], cfg["nl"]
params.stereo.fx, params.stereo.bf = cfg["fx"], cfg["bf"]
ctx = _lib.Context(params, W, H, 2 * B)
torch.cuda.set_stream(torch.cuda.Stream())          # (the default stream's handle, 0, would send every *_dev call to the context's own stream)
cap, L, s = ctx.orb_capacity, lib(), torch.cuda.current_stream().cuda_stream
nd = min(args.distinct, B)
host = synth.stereo_batch(7000, nd, W, H)
order = np.random.default_rng(1234).permutation(np.arange(B) % nd)          # the bench's shuffled batch
imgs = torch.from_numpy(host[np.stack([2 * order, 2 * order + 1], 1).reshape(-1)].copy()).cuda()
z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
kps, desc, counts = z((2 * B, cap, 28), torch.uint8), z((2 * B, cap, 32), torch.uint8), z((2 * B,), torch.int32)
ur, dp, valid = z((B, cap), torch.float32), z((B, cap), torch.float32), z((B, cap), torch.uint8)
offs, idx = z((B, _lib.GRID_CELLS + 1), torch.int32), z((B, cap), torch.int32)
fx, cx, cy, mbf = float(cfg["fx"]), W / 2.0, H / 2.0, float(cfg["bf"])
cam, bounds = (fx, fx, cx, cy, mbf), (0.0, float(W), 0.0, float(H))
check(L.olf_orb_extract_dev(ctx.handle, imgs.data_ptr(), 2 * B, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), s), "olf_orb_extract_dev")
check(L.olf_stereo_points_dev(ctx.handle, B, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), ur.data_ptr(), dp.data_ptr(), s), "olf_stereo_points_dev")
check(L.olf_stereo_points_mask_dev(ctx.handle, dp.data_ptr(), B * cap, valid.data_ptr(), s), "olf_stereo_points_mask_dev")
check(L.olf_frame_grid_dev(ctx.handle, B, 2, kps.data_ptr(), counts.data_ptr(), *bounds, offs.data_ptr(), idx.data_ptr(), s), "olf_frame_grid_dev")
eye = torch.eye(4, dtype=torch.float32, device="cuda").repeat(B, 1, 1).contiguous()
world = matcher.unproject_stereo(B, kps, counts, dp, cam[:4], eye, img_stride=2, context=ctx)
torch.cuda.synchronize()
sf = np.zeros(ctx.nlevels, np.float32)
L.olf_orb_scale_tables(ctx.handle, sf.ctypes.data, None, None, None, None)

# the map on the host (it is what the host loop reads), then on the device: point j * cap + i is feature i of frame j
hv, hw = valid.cpu().numpy().astype(bool), world.cpu().numpy().reshape(B * cap, 3)
hk = kps.cpu().numpy().reshape(2 * B, cap * 28).view(KEYPOINT_DTYPE)[0::2]
hd, hu, cnt = np.ascontiguousarray(desc.cpu().numpy()[0::2]), ur.cpu().numpy(), counts.cpu().numpy()[0::2]
dist = np.linalg.norm(hw.astype(np.float64), axis=1)
live = hv.reshape(-1) & (dist > 0)
m_normal = np.where(live[:, None], hw / np.maximum(dist, 1e-9)[:, None], 0).astype(np.float32)
m_maxd = (dist * sf[np.clip(hk["octave"].reshape(-1), 0, ctx.nlevels - 1)] * 0.95).astype(np.float32)
m_mind = (m_maxd / sf[-1]).astype(np.float32)
m_desc, m_bad = hd.reshape(B * cap, 32), ~live
own = [j * cap + np.flatnonzero(live[j * cap:(j + 1) * cap]) for j in range(B)]
lists = [np.concatenate([own[k] for k in (j - 1, j, j + 1) if 0 <= k < B]) for j in range(B)]
h_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
h_idx = np.concatenate(lists).astype(np.int32)
h_fmp = np.where(live.reshape(B, cap), np.arange(B * cap).reshape(B, cap), -1).astype(np.int32)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
lmap = matcher.LocalMapDev(up(hw), up(m_normal), up(m_maxd), up(m_mind), up(m_desc), None, up(m_bad.astype(np.uint8)), up(h_off), up(h_idx), n_mp=B * cap)
fmp = up(h_fmp)
hS = np.stack([np.eye(4, dtype=np.float32)] * B)
hS[:, :3] *= np.float32(1.25)
Scw, NE = up(hS), len(h_idx)
out = (z((NE,), torch.int32), z((NE,), torch.int32), z((B,), torch.int32))
search = lambda S: matcher.fuse_search_batch(B, kps, desc, counts, ur, offs, idx, eye, lmap, cam, bounds, th=3.0, Scw=S, frame_mp=fmp, img_stride=2, out=out,
                                             context=ctx)


def timed(tag, fn):
    fn(); fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            fn()
        b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / 10)
    ctx.synchronize()
    print("%-58s %8.3f ms per call (median of 5 windows of 10, HIP events; min %.3f max %.3f)" % (tag, sorted(ms)[2], min(ms), max(ms)), flush=True)
    return sorted(ms)[2]


print(f"{args.config} {W}x{H}, {B} key frames, {NE} entries ({NE / B:.0f} per key frame), map of {int(live.sum())} stereo points, capacity {cap}, th 3", flush=True)
sample = np.unique(np.linspace(0, B - 1, min(args.host_frames, B)).astype(int))
keep, views = [], {}
for j in sample:
    n = int(min(cnt[j], cap))
    v = ola.KeyFrameView.__new__(ola.KeyFrameView)       # (no Python grid: the host form builds its own)
    v.mvKeysUn, v.mDescriptors, v.mvuRight, v.N, v.mvScaleFactors = hk[j, :n], hd[j, :n], hu[j, :n], n, sf
    v.fx = v.fy = fx; v.cx, v.cy, v.mbf = cx, cy, mbf
    v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY = bounds
    v.mTcw, v.mFeatVec = np.eye(4, dtype=np.float32), {}
    v.mp_valid = v.mp_obs = v.mp_bad = v.mvbOutlier = v.mp_world = v.mp_desc = None
    views[j] = matcher._view_c(v, keep)
geom = {}
for j in sample:
    o = lists[j]
    skip = (m_bad[o] | ((o >= j * cap) & (o < (j + 1) * cap))).astype(np.uint8)     # bad, or held by the key frame
    geom[j] = [np.ascontiguousarray(a) for a in (skip, hw[o], m_normal[o], m_maxd[o], m_mind[o], m_desc[o])]
p = lambda a: a.ctypes.data
bad = 0
for sim3 in (False, True):
    tag = "olf_fuse_search_batch_dev, " + ("Sim3 form" if sim3 else "plain form")
    t_batch = timed(tag, lambda: search(Scw if sim3 else None))
    bi, bd, nf = (o.cpu().numpy() for o in out)
    print("  entries that find a key point: %d (%.1f %%), within TH_LOW: %d; batch entry per key frame: %.2f us, per entry: %.1f ns" %
          ((bi >= 0).sum(), 100.0 * (bi >= 0).mean(), nf.sum(), 1e3 * t_batch / B, 1e6 * t_batch / max(NE, 1)), flush=True)
    res = {j: (np.zeros(len(lists[j]), np.int32), np.zeros(len(lists[j]), np.int32)) for j in sample}

    def call(j):
        g, (ri, rd) = geom[j], res[j]
        if sim3:
            return L.olf_fuse_search_sim3(ctx.handle, views[j], p(hS[j]), len(lists[j]), *(p(a) for a in g), 3.0, p(ri), p(rd))
        return L.olf_fuse_search(ctx.handle, views[j], len(lists[j]), *(p(a) for a in g), 3.0, None, p(ri), p(rd))
    call(sample[0])          # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for j in sample:
        rc = call(j)
        assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    same = sum(int(np.array_equal(res[j][0], bi[h_off[j]:h_off[j + 1]]) and np.array_equal(res[j][1], bd[h_off[j]:h_off[j + 1]]) and
                   nf[j] == ((res[j][0] >= 0) & (res[j][1] <= 50)).sum()) for j in sample)
    print("%-58s %8.3f ms per key frame, %.1f ms for %d key frames (host clock, views and map already on the host); %d of %d identical to the batch rows" %
          ("loop of " + ("olf_fuse_search_sim3" if sim3 else "olf_fuse_search"), 1e3 * dt / len(sample), 1e3 * dt, len(sample), same, len(sample)), flush=True)
    print("  host loop per key frame / batch entry per key frame: %.0f" % ((dt / len(sample)) / (1e-3 * t_batch / B)), flush=True)
    bad += len(sample) - same
ctx.close()
if bad:
    sys.exit("the host form and the batch entry disagree")
