"""Latency of the batched SearchByProjection(Frame, Frame) (csrc/track_batch.hip) beside the only other way to get its results -- a loop of
olf_search_by_projection_match12, one host call per pair -- and beside its sibling olf_search_by_bow_batch_dev, on the left frames of the bench's
synthetic batch (identity poses, a 0.02 m predicted translation, th = 7):  python tools/track_batch_latency.py [--config C3] [--pairs 3072]
Device entries: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise."""
import argparse, ctypes as C, os, sys, time
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
ap.add_argument("--pairs", type=int, default=0)
ap.add_argument("--distinct", type=int, default=512)
ap.add_argument("--host-pairs", type=int, default=0, help="pairs the host loop covers (0: all)")
ap.add_argument("--th", type=float, default=7.0)
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
check(L.olf_orb_extract_dev(ctx.handle, imgs.data_ptr(), 2 * B, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), s), "olf_orb_extract_dev")
check(L.olf_stereo_points_dev(ctx.handle, B, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), ur.data_ptr(), dp.data_ptr(), s), "olf_stereo_points_dev")
check(L.olf_stereo_points_mask_dev(ctx.handle, dp.data_ptr(), B * cap, valid.data_ptr(), s), "olf_stereo_points_mask_dev")
fx, cx, cy, mbf = float(cfg["fx"]), W / 2.0, H / 2.0, float(cfg["bf"])
bounds = (0.0, float(W), 0.0, float(H))
eye = torch.eye(4, dtype=torch.float32, device="cuda").repeat(B, 1, 1).contiguous()
Tcw = eye.clone()
Tcw[:, 0, 3] = 0.02
world = matcher.unproject_stereo(B, kps, counts, dp, (fx, fx, cx, cy), eye, context=ctx)
offs, idx = z((B, _lib.GRID_CELLS + 1), torch.int32), z((B, cap), torch.int32)
grid = lambda: check(L.olf_frame_grid_dev(ctx.handle, B, 2, kps.data_ptr(), counts.data_ptr(), *bounds, offs.data_ptr(), idx.data_ptr(), s), "olf_frame_grid_dev")
out = (z((B - 1, cap), torch.int32), z((B - 1, cap), torch.int32), z((B - 1,), torch.int32))
search = lambda: matcher.search_by_projection_batch(B, kps, desc, counts, ur, offs, idx, Tcw, world, (fx, fx, cx, cy, mbf), bounds, args.th,
                                                    mp_valid=valid, out=out, context=ctx)


def timed(tag, fn, unit):
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
    print("%-58s %8.3f ms per call (%d pairs; median of 5 windows of 10, HIP events; min %.3f max %.3f)%s" % (tag, sorted(ms)[2], B - 1, min(ms), max(ms), unit), flush=True)
    return sorted(ms)[2]


print(f"{args.config} {W}x{H}, {B} stereo pairs, capacity {cap}, th {args.th}", flush=True)
timed("olf_frame_grid_dev (the grids the search reads)", grid, "")
t_batch = timed("olf_search_by_projection_batch_dev", search, "")
n_dev, m_dev, m12_dev = out[2].cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy()
cnt = counts.cpu().numpy()[0::2]
print("  key points per frame: mean %.0f; matches per pair: mean %.1f, min %d, max %d" % (cnt.mean(), n_dev.mean(), n_dev.min(), n_dev.max()), flush=True)

# the sibling: SearchByBoW over the same batch
cn0, de0 = counts[:16].cpu().numpy(), desc[:16].cpu().numpy()
from orb_line_slam_amd.vocabulary import ORBVocabulary
voc = ORBVocabulary.from_arrays(10, 6, *bench.synthetic_vocabulary(10, 6, np.concatenate([de0[i, :cn0[i]] for i in range(min(2 * B, 16))])), context=ctx)
f2f, f2f_n = z((B, 2 * cap), torch.int32), z((B,), torch.int32)
timed("olf_search_by_bow_batch_dev (ComputeBoW included)",
      lambda: check(L.olf_search_by_bow_batch_dev(ctx.handle, voc._h, B, 2, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), valid.data_ptr(), None, 0.7, 1, 4,
                                                  f2f.data_ptr(), f2f_n.data_ptr(), s), "olf_search_by_bow_batch_dev"), "")

# the host entry, one call per pair, on the downloaded arrays
hk = kps.cpu().numpy().reshape(2 * B, cap * 28).view(KEYPOINT_DTYPE)[0::2]
hd, hu = desc.cpu().numpy()[0::2], ur.cpu().numpy()
hw, hv, hT = world.cpu().numpy(), valid.cpu().numpy().astype(bool), Tcw.cpu().numpy()
sf = np.zeros(ctx.nlevels, np.float32)
L.olf_orb_scale_tables(ctx.handle, sf.ctypes.data_as(C.c_void_p), None, None, None, None)
nh = min(args.host_pairs or B - 1, B - 1)
views, keep = [], []
for j in range(nh + 1):
    n = int(cnt[j])
    v = ola.FrameView.__new__(ola.FrameView)             # (no Python grid: the host entry builds its own)
    v.mvKeysUn, v.mDescriptors, v.mvuRight, v.N, v.mvScaleFactors = hk[j, :n], hd[j, :n], hu[j, :n], n, sf
    v.fx = v.fy = fx; v.cx, v.cy, v.mbf = cx, cy, mbf
    v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY = bounds
    v.mTcw, v.mFeatVec = hT[j], {}
    v.mp_valid, v.mp_world, v.mp_desc, v.mp_obs = hv[j, :n].copy(), hw[j, :n], hd[j, :n], np.ones(n, bool)
    v.mp_bad, v.mvbOutlier = np.zeros(n, bool), np.zeros(n, bool)
    views.append(v)
last_c = [matcher._view_c(v, keep) for v in views[:-1]]
cur_c = []
for v in views[1:]:
    v.mp_valid, v.mp_obs = np.zeros(v.N, bool), np.zeros(v.N, bool)      # the CurrentFrame starts without map points
    cur_c.append(matcher._view_c(v, keep))
hm, hm12, hn = np.full((nh, cap), -1, np.int32), np.full((nh, cap), -1, np.int32), np.zeros(nh, np.int32)
L.olf_search_by_projection_match12(ctx.handle, cur_c[0], last_c[0], args.th, 0, 1, hm[0].ctypes.data, hm12[0].ctypes.data, hn[0:].ctypes.data)      # warm
views[1].mp_valid[:], views[1].mp_obs[:] = False, False
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
    lv, cv = views[j], views[j + 1]
    Xc = hw[j, :lv.N] + hT[j + 1][:3, 3]
    ok = hv[j, :lv.N] & (Xc[:, 2] > 0)
    q = np.zeros(int(ok.sum()), _lib.AREA_QUERY_DTYPE)
    o = lv.mvKeysUn["octave"][ok]
    q["x"], q["y"] = fx * Xc[ok, 0] / Xc[ok, 2] + cx, fx * Xc[ok, 1] / Xc[ok, 2] + cy
    q["r"], q["min_level"], q["max_level"] = np.float32(args.th) * sf[o], o - 1, o + 1
    g = ola.assign_features_to_grid(cv.mvKeysUn, bounds, context=ctx)
    co, _ = ola.features_in_area(cv.mvKeysUn, g, bounds, q, context=ctx)
    lens.append(np.diff(co))
lens = np.concatenate(lens)
print("  candidate lists (%d queries of %d sampled pairs): mean %.2f, median %d, p99 %d, max %d, empty %.1f %%, longer than 64: %d" %
      (len(lens), min(nh, 32), lens.mean(), np.median(lens), np.percentile(lens, 99), lens.max(), 100.0 * (lens == 0).mean(), int((lens > 64).sum())), flush=True)
voc.clear()
ctx.close()
