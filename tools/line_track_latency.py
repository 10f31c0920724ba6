"""Latency of the batched line half of tracking (csrc/line_batch.hip: olf_is_in_frustum_l_batch_dev, olf_search_local_lines_batch_dev,
olf_track_lines_batch_dev) beside the only other way to the results of the local search -- per frame: download the frame's lines, olf_is_in_frustum_l, gather
the in-view descriptors, olf_match_bf, olf_local_lines_assign -- on the left frames of the bench's synthetic batch.  The map lines are the batch's own stereo
lines (both end points unprojected with their disparities, identity poses); frame j's local lines are those of frames j - 1, j and j + 1, in that order; the
frames hold nothing on entry; predicted pose: a 0.02 m translation; nnr = Config::minRatio12L():
    python tools/line_track_latency.py [--config C3] [--pairs 3072]
Device entries: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise."""
import ctypes as C, time
import numpy as np
from latency_common import BenchBatch, parser, up, zeros as z
import torch
from orb_line_slam_amd import _lib, matcher
from orb_line_slam_amd._lib import KEYLINE_DTYPE

ap = parser()
ap.add_argument("--host-frames", type=int, default=0, help="frames the host loop covers (0: all)")
args = ap.parse_args()
batch = BenchBatch(args)
ctx, L, W, H, B, cap, params = batch.ctx, batch.L, batch.W, batch.H, batch.B, batch.ctx.line_capacity, batch.params
nnr = float(params.stereo.min_ratio_12_l)
kls, ldesc, lcounts, ldisp = batch.kls, batch.ldesc, batch.lcounts, batch.ldisp
(fx, _, cx, cy, mbf), cam, bounds = batch.cam, batch.cam, batch.bounds
Tcw = batch.eye          # (this tool reads the identity poses nowhere else: the predicted poses are written into them)
Tcw[:, 0, 3] = 0.02

# the map: line f * cap + i is the stereo line i of frame f -- GetWorldPos() from the end points and their disparities, the line's own descriptor
torch.cuda.synchronize()
cnt = lcounts.cpu().numpy()[0::2]
hk = kls.cpu().numpy().reshape(2 * B, cap * 68).view(KEYLINE_DTYPE)[0::2]
hd, hdisp = ldesc.cpu().numpy()[0::2], ldisp.cpu().numpy()
with np.errstate(divide="ignore", invalid="ignore"):
    zs, ze = mbf / hdisp[:, :, 0].astype(np.float64), mbf / hdisp[:, :, 1].astype(np.float64)
    m_world = np.stack([(hk["startPointX"] - cx) * zs / fx, (hk["startPointY"] - cy) * zs / fx, zs, (hk["endPointX"] - cx) * ze / fx, (hk["endPointY"] - cy) * ze / fx, ze], 2)
stereo = (hdisp[:, :, 0] > 0) & (hdisp[:, :, 1] > 0) & (np.arange(cap)[None, :] < cnt[:, None])
m_world = np.where(stereo[:, :, None], m_world, 0.0).astype(np.float32).reshape(B * cap, 6)
m_desc = np.ascontiguousarray(hd.reshape(B * cap, 32))
m_obs, m_bad = (np.arange(B * cap) % 2).astype(np.uint8), np.zeros(B * cap, np.uint8)
own = [f * cap + np.flatnonzero(stereo[f]) for f in range(B)]
lists = [np.concatenate([own[f] for f in (j - 1, j, j + 1) if 0 <= f < B]).astype(np.int32) for j in range(B)]
l_offs = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
ne = int(l_offs[-1])
lm = matcher.LocalLineMapDev(up(m_world), up(m_desc), up(m_obs), up(m_bad), up(l_offs), up(np.concatenate(lists)), n_ml=B * cap)
out = (z((ne,), torch.uint8), z((ne, 4), torch.float32), z((ne,), torch.int32), z((B, cap), torch.int32), z((B,), torch.int32))
search = lambda: matcher.search_local_lines_batch(B, kls, ldesc, lcounts, ldisp, Tcw, lm, cam, bounds, nnr, out=out, context=ctx)
fr_out = (z((ne,), torch.uint8), z((ne, 4), torch.float32))
frustum = lambda: matcher.is_in_frustum_l_batch(B, Tcw, lm, cam, bounds, out=fr_out, context=ctx)
last_ml = up(np.where(stereo, np.arange(B * cap).reshape(B, cap), -1).astype(np.int32)[:B - 1])
tr_out = (z((B - 1, cap), torch.int32), z((B - 1, cap), torch.int32), z((B - 1,), torch.int32))
track = lambda: matcher.track_lines_batch(B, kls, ldesc, lcounts, ldisp, last_ml, bounds, nnr, best_lr=bool(params.stereo.best_lr_matches), out=tr_out, context=ctx)
frames_note = "%d frames; " % B
print(f"{args.config} {W}x{H}, {B} stereo pairs, line capacity {cap}, nnr {nnr}; map {B * cap} slots, {ne} list entries ({ne / B:.0f} per frame)", flush=True)
t_fr = batch.timed("olf_is_in_frustum_l_batch_dev (the frustum pass alone)", frustum, note=frames_note)
t_batch = batch.timed("olf_search_local_lines_batch_dev", search, note=frames_note)
t_track = batch.timed("olf_track_lines_batch_dev (%d pairs)" % (B - 1), track, note=frames_note)
torch.cuda.synchronize()
v_dev, p_dev, m_dev, f_dev, n_dev = (x.cpu().numpy() for x in out)
print("  lines per frame: mean %.0f; in view: %.1f %% of the entries; n_inliers_ls per frame: mean %.1f, min %d, max %d; f2f n_inliers_ls: mean %.1f" %
      (cnt.mean(), 100.0 * v_dev.mean(), n_dev.mean(), n_dev.min(), n_dev.max(), float(tr_out[2].float().mean())), flush=True)

# the host way, frame by frame
hT = Tcw.cpu().numpy()
nh = min(args.host_frames or B, B)
p = lambda x: x.ctypes.data
views = []
for j in range(nh):
    f = _lib.FrameViewC()
    f.Tcw = p(hT[j])
    f.fx, f.fy, f.cx, f.cy, f.mbf = cam
    f.minX, f.maxX, f.minY, f.maxY = bounds
    views.append(f)
res = [None] * nh


def host_frame(j):
    n = int(cnt[j])
    k = kls[2 * j, :n].cpu().numpy().reshape(-1).view(KEYLINE_DTYPE)                       # download
    d, dis = ldesc[2 * j, :n].cpu().numpy(), ldisp[j, :n].cpu().numpy()
    li = lists[j]
    w = np.ascontiguousarray(m_world[li])
    inv, proj = np.zeros(len(li), np.uint8), np.zeros((len(li), 4), np.float32)
    assert L.olf_is_in_frustum_l(C.byref(views[j]), len(li), p(w), p(inv), p(proj)) == 0, _lib.last_error()
    ranks = np.flatnonzero(inv)
    midx = np.ascontiguousarray(li[ranks])
    q = np.ascontiguousarray(m_desc[midx])                                                   # gather
    m12 = np.full(len(ranks), -1, np.int32)
    if len(ranks) and n:
        assert L.olf_match_bf(ctx.handle, p(q), len(ranks), p(d), n, nnr, 0, p(m12)) == 0, _lib.last_error()
    fm, ni, pr = np.full(n, -1, np.int32), np.zeros(1, np.int32), np.ascontiguousarray(proj[ranks])
    assert L.olf_local_lines_assign(len(ranks), p(m12), p(midx), p(pr), p(k), n, p(dis), *bounds, B * cap, p(m_obs), p(fm), p(ni)) == 0, _lib.last_error()
    res[j] = (inv, proj, ranks, m12, fm, int(ni[0]))


host_frame(0)                                             # warm
torch.cuda.synchronize()
t0 = time.perf_counter()
for j in range(nh):
    host_frame(j)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
same = 0
for j in range(nh):
    inv, proj, ranks, m12, fm, ni = res[j]
    b, e = l_offs[j], l_offs[j + 1]
    me = np.full(e - b, -1, np.int32)
    me[ranks] = m12
    ok = np.array_equal(v_dev[b:e], inv) and np.array_equal(p_dev[b:e][ranks].view(np.uint32), proj[ranks].view(np.uint32)) and np.array_equal(m_dev[b:e], me)
    same += int(ok and np.array_equal(f_dev[j, :len(fm)], fm) and (f_dev[j, len(fm):] == -1).all() and ni == n_dev[j])
print("%-58s %8.3f ms per frame, %.1f ms for %d frames (host clock); %d of %d frames identical to the batch entry" %
      ("loop: download, olf_is_in_frustum_l, gather, olf_match_bf, olf_local_lines_assign", 1e3 * dt / nh, 1e3 * dt, nh, same, nh), flush=True)
print("  batch entry per frame: %.4f ms; ratio loop / batch over %d frames: %.1f" % (t_batch / B, nh, (1e3 * dt / nh) / (t_batch / B)), flush=True)
ctx.close()
