"""Latency of the batched SearchForTriangulation (csrc/triangulation_batch.hip) beside the only other way to get its results -- a loop of
olf_search_for_triangulation, one host call per key-frame pair, with the views and their feature vectors already on the host -- on the left frames of
the bench's synthetic batch: every frame against its 10 predecessors (the shape of LocalMapping::CreateNewMapPoints), F12 for identity rotation and a
sideways baseline of 0.05 m per frame, an ORBvoc-shaped (k = 10, L = 6) vocabulary drawn from the batch, levelsup 4; a feature holds a map point where
it has a stereo depth:  python tools/triangulation_latency.py [--config C3] [--pairs 3072] [--host-pairs 64]
Device entry: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise."""
import argparse, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
import torch
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, matcher, synth
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, check, lib
from orb_line_slam_amd.vocabulary import ORBVocabulary
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C3")
ap.add_argument("--pairs", type=int, default=0, help="stereo pairs = frames of the batch (0: the configuration's default)")
ap.add_argument("--distinct", type=int, default=512)
ap.add_argument("--neighbours", type=int, default=10, help="predecessors every frame is matched against")
ap.add_argument("--host-pairs", type=int, default=64, help="key-frame pairs, evenly spread over the list, the host loop covers")
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
torch.cuda.synchronize()
fx, cx, cy = float(cfg["fx"]), W / 2.0, H / 2.0
cam = (fx, fx, cx, cy)
hT = np.stack([np.eye(4, dtype=np.float32)] * B)
hT[:, 0, 3] = -0.05 * np.arange(B)
pairs = np.array([(j, j - d) for j in range(B) for d in range(1, args.neighbours + 1) if j - d >= 0], np.int32).reshape(-1, 2)
Ki = np.linalg.inv(np.array([[fx, 0, cx], [0, fx, cy], [0, 0, 1]], np.float64))


def f12(a, b):          # LocalMapping::ComputeF12 for identity rotations: t12 = t1w - t2w
    t = hT[a, :3, 3].astype(np.float64) - hT[b, :3, 3].astype(np.float64)
    return (Ki.T @ np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ Ki).astype(np.float32)


hF = np.stack([f12(a, b) for a, b in pairs]) if len(pairs) else np.zeros((0, 3, 3), np.float32)
P = len(pairs)
cn0, de0 = counts[:16].cpu().numpy(), desc[:16].cpu().numpy()
voc = ORBVocabulary.from_arrays(10, 6, *bench.synthetic_vocabulary(10, 6, np.concatenate([de0[i, :cn0[i]] for i in range(min(2 * B, 16))])), context=ctx)
Tcw, d_pairs, d_F = torch.from_numpy(hT).cuda(), torch.from_numpy(pairs).cuda(), torch.from_numpy(hF).cuda()
out = (z((P, cap), torch.int32), z((P,), torch.int32))
search = lambda: matcher.search_for_triangulation_batch(voc, B, kps, desc, counts, ur, Tcw, d_pairs, d_F, cam, mp_valid=valid, levelsup=4, out=out, context=ctx)


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


print(f"{args.config} {W}x{H}, {B} frames, {P} key-frame pairs ({args.neighbours} predecessors each), capacity {cap}, levelsup 4", flush=True)
t_batch = timed("olf_search_for_triangulation_batch_dev (ComputeBoW included)", search)
m_dev, n_dev = out[0].cpu().numpy(), out[1].cpu().numpy()
cnt, hv = counts.cpu().numpy()[0::2], valid.cpu().numpy().astype(bool)
free = np.array([(~hv[j, :cnt[j]]).sum() for j in range(B)])
print("  key points per frame: mean %.0f, without a map point: mean %.0f; matches per pair: mean %.2f, min %d, max %d" %
      (cnt.mean(), free.mean(), n_dev.mean(), n_dev.min(), n_dev.max()), flush=True)
print("  batch entry per pair: %.2f us" % (1e3 * t_batch / max(P, 1)), flush=True)

# the host form, one call per pair of a sample, on downloaded arrays whose feature vectors are already made
sample = np.unique(np.linspace(0, P - 1, min(args.host_pairs, P)).astype(int)) if P else np.zeros(0, int)
hk = kps.cpu().numpy().reshape(2 * B, cap * 28).view(KEYPOINT_DTYPE)[0::2]
hd, hu = desc.cpu().numpy()[0::2], ur.cpu().numpy()
sf = np.zeros(ctx.nlevels, np.float32)
L.olf_orb_scale_tables(ctx.handle, sf.ctypes.data, None, None, None, None)
views, keep = {}, []
for j in sorted({int(f) for q in sample for f in pairs[q]}):
    n = int(cnt[j])
    v = ola.FrameView.__new__(ola.FrameView)             # (no Python grid: this search reads none)
    v.mvKeysUn, v.mDescriptors, v.mvuRight, v.N, v.mvScaleFactors = hk[j, :n], hd[j, :n], hu[j, :n], n, sf
    v.fx = v.fy = fx; v.cx, v.cy, v.mbf = cx, cy, float(cfg["bf"])
    v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY = 0.0, float(W), 0.0, float(H)
    v.mTcw, v.mp_valid = hT[j], hv[j, :n].copy()
    v.mp_world, v.mp_desc, v.mp_obs, v.mp_bad, v.mvbOutlier = None, None, None, None, None
    _, v.mFeatVec = voc.transform(v.mDescriptors, 4)
    views[j] = matcher._view_c(v, keep)
hm, hn = np.full((len(sample), cap), -1, np.int32), np.zeros(len(sample), np.int32)
call = lambda r, q: L.olf_search_for_triangulation(ctx.handle, views[int(pairs[q, 0])], views[int(pairs[q, 1])], hF[q].ctypes.data, None, 0, 1, hm[r].ctypes.data, hn[r:].ctypes.data)
if len(sample):
    call(0, sample[0])          # warm
    hm[0] = -1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r, q in enumerate(sample):
        rc = call(r, q)
        assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    same = sum(int(hn[r] == n_dev[q] and np.array_equal(hm[r], m_dev[q])) for r, q in enumerate(sample))
    print("%-58s %8.3f ms per pair, %.1f ms for %d pairs (host clock, views and feature vectors already on the host); %d of %d pairs identical to the batch entry" %
          ("loop of olf_search_for_triangulation", 1e3 * dt / len(sample), 1e3 * dt, len(sample), same, len(sample)), flush=True)
    print("  host loop per pair / batch entry per pair: %.0f" % ((dt / len(sample)) / (1e-3 * t_batch / P)), flush=True)
    assert same == len(sample), "the host form and the batch entry disagree"
voc.clear()
ctx.close()
