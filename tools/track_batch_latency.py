"""Latency of the batched SearchByProjection(Frame, Frame) (csrc/track_batch.hip) beside the only other way to get its results -- a loop of
olf_search_by_projection_match12, one host call per pair -- and beside its sibling olf_search_by_bow_batch_dev, on the left frames of the bench's
synthetic batch (identity poses, a 0.02 m predicted translation, th = 7):  python tools/track_batch_latency.py [--config C3] [--pairs 3072]
Device entries: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise."""
import time
import numpy as np
from latency_common import BenchBatch, host_view, parser, zeros as z
import torch
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, matcher
from orb_line_slam_amd._lib import check
import bench

ap = parser()
ap.add_argument("--host-pairs", type=int, default=0, help="pairs the host loop covers (0: all)")
ap.add_argument("--th", type=float, default=7.0)
args = ap.parse_args()
batch = BenchBatch(args)
ctx, L, s, W, H, B, cap = batch.ctx, batch.L, batch.s, batch.W, batch.H, batch.B, batch.cap
kps, desc, counts, ur, valid = batch.kps, batch.desc, batch.counts, batch.ur, batch.valid
(fx, _, cx, cy, mbf), bounds = batch.cam, batch.bounds
Tcw = batch.eye.clone()
Tcw[:, 0, 3] = 0.02
world, offs, idx, grid = batch.world, batch.offs, batch.idx, batch.grid
out = (z((B - 1, cap), torch.int32), z((B - 1, cap), torch.int32), z((B - 1,), torch.int32))
search = lambda: matcher.search_by_projection_batch(B, kps, desc, counts, ur, offs, idx, Tcw, world, (fx, fx, cx, cy, mbf), bounds, args.th,
                                                    mp_valid=valid, out=out, context=ctx)
pairs_note = "%d pairs; " % (B - 1)
print(f"{args.config} {W}x{H}, {B} stereo pairs, capacity {cap}, th {args.th}", flush=True)
batch.timed("olf_frame_grid_dev (the grids the search reads)", grid, note=pairs_note)
t_batch = batch.timed("olf_search_by_projection_batch_dev", search, note=pairs_note)
n_dev, m_dev, m12_dev = out[2].cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy()
cnt = batch.cnt
print("  key points per frame: mean %.0f; matches per pair: mean %.1f, min %d, max %d" % (cnt.mean(), n_dev.mean(), n_dev.min(), n_dev.max()), flush=True)

# the sibling: SearchByBoW over the same batch
cn0, de0 = counts[:16].cpu().numpy(), desc[:16].cpu().numpy()
from orb_line_slam_amd.vocabulary import ORBVocabulary
voc = ORBVocabulary.from_arrays(10, 6, *bench.synthetic_vocabulary(10, 6, np.concatenate([de0[i, :cn0[i]] for i in range(min(2 * B, 16))])), context=ctx)
f2f, f2f_n = z((B, 2 * cap), torch.int32), z((B,), torch.int32)
batch.timed("olf_search_by_bow_batch_dev (ComputeBoW included)",
      lambda: check(L.olf_search_by_bow_batch_dev(ctx.handle, voc._h, B, 2, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), valid.data_ptr(), None, 0.7, 1, 4,
                                                  f2f.data_ptr(), f2f_n.data_ptr(), s), "olf_search_by_bow_batch_dev"), note=pairs_note)

# the host entry, one call per pair, on the downloaded arrays
hk, hd, hu, hw, hv, hT, sf = batch.hk, batch.hd, batch.hu, batch.hw, batch.hv, Tcw.cpu().numpy(), batch.sf
nh = min(args.host_pairs or B - 1, B - 1)


def view(j, mp_valid, mp_obs):
    n = int(cnt[j])
    return host_view(batch, j, mvuRight=hu[j, :n], mTcw=hT[j], mp_valid=mp_valid, mp_obs=mp_obs, mp_world=hw[j, :n], mp_desc=hd[j, :n], mp_bad=np.zeros(n, bool),
                     mvbOutlier=np.zeros(n, bool))


last_c = [view(j, hv[j, :int(cnt[j])].copy(), np.ones(int(cnt[j]), bool)) for j in range(nh)]
cur_state = [(np.zeros(int(cnt[j]), bool), np.zeros(int(cnt[j]), bool)) for j in range(1, nh + 1)]      # the CurrentFrame starts without map points
cur_c = [view(j + 1, *cur_state[j]) for j in range(nh)]
hm, hm12, hn = np.full((nh, cap), -1, np.int32), np.full((nh, cap), -1, np.int32), np.zeros(nh, np.int32)
L.olf_search_by_projection_match12(ctx.handle, cur_c[0], last_c[0], args.th, 0, 1, hm[0].ctypes.data, hm12[0].ctypes.data, hn[0:].ctypes.data)      # warm
cur_state[0][0][:], cur_state[0][1][:] = False, False
hm[0], hm12[0] = -1, -1
torch.cuda.synchronize()
t0 = time.perf_counter()
for j in range(nh):
    rc = L.olf_search_by_projection_match12(ctx.handle, cur_c[j], last_c[j], args.th, 0, 1, hm[j].ctypes.data, hm12[j].ctypes.data, hn[j:].ctypes.data)
    assert rc == 0, _lib.last_error()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
same = sum(int(hn[j] == n_dev[j] and np.array_equal(hm[j], m_dev[j]) and np.array_equal(hm12[j], m12_dev[j])) for j in range(nh))
print("%-58s %8.3f ms per call, %.1f ms for %d pairs (host clock, arrays already on the host); %d of %d pairs identical to the batch entry" %
      ("loop of olf_search_by_projection_match12", 1e3 * dt / nh, 1e3 * dt, nh, same, nh), flush=True)
print("  batch entry per pair: %.4f ms" % (t_batch / (B - 1)), flush=True)

# candidate statistics of a sample of pairs: the windows of the LastFrame's queries on the CurrentFrame's grid
lens = []
for j in np.linspace(0, nh - 1, min(nh, 32)).astype(int):
    nl, keys_c = int(cnt[j]), hk[j + 1, :int(cnt[j + 1])]
    Xc = hw[j, :nl] + hT[j + 1][:3, 3]
    ok = hv[j, :nl] & (Xc[:, 2] > 0)
    q = np.zeros(int(ok.sum()), _lib.AREA_QUERY_DTYPE)
    o = hk[j, :nl]["octave"][ok]
    q["x"], q["y"] = fx * Xc[ok, 0] / Xc[ok, 2] + cx, fx * Xc[ok, 1] / Xc[ok, 2] + cy
    q["r"], q["min_level"], q["max_level"] = np.float32(args.th) * sf[o], o - 1, o + 1
    g = ola.assign_features_to_grid(keys_c, bounds, context=ctx)
    co, _ = ola.features_in_area(keys_c, g, bounds, q, context=ctx)
    lens.append(np.diff(co))
lens = np.concatenate(lens)
print("  candidate lists (%d queries of %d sampled pairs): mean %.2f, median %d, p99 %d, max %d, empty %.1f %%, longer than 64: %d" %
      (len(lens), min(nh, 32), lens.mean(), np.median(lens), np.percentile(lens, 99), lens.max(), 100.0 * (lens == 0).mean(), int((lens > 64).sum())), flush=True)
voc.clear()
ctx.close()
