"""Latency of the batched Fuse search (csrc/fuse_batch.hip) beside the only other way to get its results -- a loop of olf_fuse_search /
olf_fuse_search_sim3, one host call per key frame, with the views and the map already on the host -- on the left frames of the bench's synthetic
batch: the map is the batch's own stereo points (olf_unproject_stereo_dev, identity poses), frame j's list holds the stereo points of frames j - 1, j
and j + 1, and a frame holds its own points, so a third of its list is skipped as held; th = 3; both forms (the Sim3 poses are 1.25 * identity):
  python tools/fuse_latency.py [--config C3] [--pairs 3072] [--host-frames 64]
Device entry: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise.  The sampled frames' host
results are compared with the batch rows; a mismatch ends the tool with a non-zero status."""
import sys, time
import numpy as np
from latency_common import BenchBatch, host_view, parser, up, zeros as z
import torch
from orb_line_slam_amd import _lib, matcher

ap = parser("stereo pairs = key frames of the batch (0: the configuration's default)")
ap.add_argument("--host-frames", type=int, default=64, help="key frames, evenly spread over the batch, the host loop covers")
args = ap.parse_args()
batch = BenchBatch(args)
ctx, L, W, H, B, cap = batch.ctx, batch.L, batch.W, batch.H, batch.B, batch.cap
kps, desc, counts, ur, valid = batch.kps, batch.desc, batch.counts, batch.ur, batch.valid
cam, bounds, offs, idx = batch.cam, batch.bounds, batch.offs, batch.idx
batch.grid()
eye, world = batch.eye, batch.world
torch.cuda.synchronize()
sf = batch.sf

# the map on the host (it is what the host loop reads), then on the device: point j * cap + i is feature i of frame j
hv, hw, hk, hd, hu = batch.hv, batch.hw.reshape(B * cap, 3), batch.hk, batch.hd, batch.hu
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
lmap = matcher.LocalMapDev(up(hw), up(m_normal), up(m_maxd), up(m_mind), up(m_desc), None, up(m_bad.astype(np.uint8)), up(h_off), up(h_idx), n_mp=B * cap)
fmp = up(h_fmp)
hS = np.stack([np.eye(4, dtype=np.float32)] * B)
hS[:, :3] *= np.float32(1.25)
Scw, NE = up(hS), len(h_idx)
out = (z((NE,), torch.int32), z((NE,), torch.int32), z((B,), torch.int32))
search = lambda S: matcher.fuse_search_batch(B, kps, desc, counts, ur, offs, idx, eye, lmap, cam, bounds, th=3.0, Scw=S, frame_mp=fmp, img_stride=2, out=out,
                                             context=ctx)
print(f"{args.config} {W}x{H}, {B} key frames, {NE} entries ({NE / B:.0f} per key frame), map of {int(live.sum())} stereo points, capacity {cap}, th 3", flush=True)
sample = np.unique(np.linspace(0, B - 1, min(args.host_frames, B)).astype(int))
# (the host form reads none of the views' own map-point state)
views = {j: host_view(batch, j, "keyframe", mvuRight=hu[j, :int(min(batch.cnt[j], cap))], mTcw=np.eye(4, dtype=np.float32)) for j in sample}
geom = {}
for j in sample:
    o = lists[j]
    skip = (m_bad[o] | ((o >= j * cap) & (o < (j + 1) * cap))).astype(np.uint8)     # bad, or held by the key frame
    geom[j] = [np.ascontiguousarray(a) for a in (skip, hw[o], m_normal[o], m_maxd[o], m_mind[o], m_desc[o])]
p = lambda a: a.ctypes.data
bad = 0
for sim3 in (False, True):
    tag = "olf_fuse_search_batch_dev, " + ("Sim3 form" if sim3 else "plain form")
    t_batch = batch.timed(tag, lambda: search(Scw if sim3 else None))
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
