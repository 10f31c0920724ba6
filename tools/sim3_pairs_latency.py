"""Latency of SearchBySim3 over a pair list (olf_search_by_sim3_pairs_dev, csrc/sim3_batch.hip) beside the loop it replaces -- olf_search_by_sim3, one host
call per pair, with the views already on the host -- on the left frames of the bench's synthetic batch: identity poses and the identity similarity, a
feature holds a map point where it has a stereo depth (olf_unproject_stereo_dev), mfMaxDistance from the depth and the octave, th = 7.5, no pre-matches.
Three shapes:
  one ComputeSim3 round   the current key frame against 8 and against 32 candidates (LoopClosing::ComputeSim3)
  throughput              every frame of the batch against its predecessor (a few thousand pairs)
python tools/sim3_pairs_latency.py [--config C3] [--pairs 3072] [--host-pairs 64]
Device entry: HIP events, warmed up, median of five windows of ten calls; every call starts from vpMatches12 = NULL, so the refill of that array (one
fill_ of n_pairs x capacity words) is inside the window.  Host loop: host clock, ending in a synchronise; the throughput shape's loop covers a sample
of the pairs.  Every looped pair is compared with the entry's rows and count; a difference ends the tool with a non-zero status."""
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
ap.add_argument("--host-pairs", type=int, default=64, help="pairs of the throughput shape, evenly spread, the host loop covers")
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

# the per-feature map-point arrays, made on the host (the host loop reads them there), then uploaded
hv, hw = valid.cpu().numpy().astype(bool), world.cpu().numpy()
hk = kps.cpu().numpy().reshape(2 * B, cap * 28).view(KEYPOINT_DTYPE)[0::2]
hd, cnt = np.ascontiguousarray(desc.cpu().numpy()[0::2]), counts.cpu().numpy()[0::2]
dist = np.linalg.norm(hw.astype(np.float64), axis=2)
h_maxd = (dist * sf[np.clip(hk["octave"], 0, ctx.nlevels - 1)] * 0.95).astype(np.float32)
h_mind = (h_maxd / sf[-1]).astype(np.float32)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
maxd, mind = up(h_maxd), up(h_mind)
print(f"{args.config} {W}x{H}, {B} key frames, capacity {cap}, key points per frame: mean {cnt.mean():.0f}, of which hold a point: {hv.sum() / B:.0f}; th 7.5",
      flush=True)


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
    print("%-66s %8.3f ms per call (median of 5 windows of 10, HIP events; min %.3f max %.3f)" % (tag, sorted(ms)[2], min(ms), max(ms)), flush=True)
    return sorted(ms)[2]


keep, views = [], {}


def host_view(j):
    if j not in views:
        n = int(min(cnt[j], cap))
        v = ola.KeyFrameView.__new__(ola.KeyFrameView)       # (no Python grid: the host form builds its own)
        v.mvKeysUn, v.mDescriptors, v.mvuRight, v.N, v.mvScaleFactors = hk[j, :n], hd[j, :n], None, n, sf
        v.fx = v.fy = fx; v.cx, v.cy, v.mbf = cx, cy, mbf
        v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY = bounds
        v.mTcw, v.mFeatVec = np.eye(4, dtype=np.float32), {}
        v.mp_valid, v.mp_bad, v.mp_obs, v.mvbOutlier = hv[j, :n].copy(), np.zeros(n, bool), None, None
        v.mp_world, v.mp_desc, v.mp_maxd, v.mp_mind = hw[j, :n], hd[j, :n], h_maxd[j, :n], h_mind[j, :n]
        views[j] = (matcher._view_c(v, keep), n)
    return views[j]


R_I, t_0 = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)
p = lambda a: a.ctypes.data


def host_loop(pairs):
    """olf_search_by_sim3 per pair: (seconds, rows, vnMatch1 rows, vnMatch2 rows, counts)"""
    vs = [(host_view(int(a)), host_view(int(b))) for a, b in pairs]          # (laying the arrays out for the C ABI is not counted)
    hm, h1, h2 = (np.full((len(pairs), cap), -1, np.int32) for _ in range(3))
    hn = np.zeros(len(pairs), np.int32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r, ((va, na), (vb, nb)) in enumerate(vs):
        rc = L.olf_search_by_sim3(ctx.handle, va, vb, p(hm[r]), 1.0, p(R_I), p(t_0), 7.5, p(h1[r]), p(h2[r]), p(hn[r:]))
        assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, hm, h1, h2, hn


bad = 0


def shape(tag, pairs, host_sample):
    global bad
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    P, nf = len(pairs), int(pairs.max()) + 1
    d_pairs = torch.from_numpy(pairs).cuda()
    s12, R12, t12 = torch.ones(P, device="cuda"), torch.eye(3, device="cuda").repeat(P, 1, 1).contiguous(), z((P, 3), torch.float32)
    m12 = torch.full((P, cap), -1, dtype=torch.int32, device="cuda")
    out = (z((P, cap), torch.int32), z((P, cap), torch.int32), z((P,), torch.int32))

    def run():
        m12.fill_(-1)
        matcher.search_by_sim3_pairs(nf, kps, desc, counts, offs, idx, eye, world, maxd, mind, d_pairs, s12, R12, t12, cam, bounds, matches12=m12, th=7.5,
                                     mp_valid=valid, out=out, context=ctx)
    t = timed(f"{tag}: olf_search_by_sim3_pairs_dev, {P} pairs of {nf} frames", run)
    ctx.poll_status()
    dm, d1, d2, dn = m12.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy()
    print("  nfound per pair: mean %.1f, min %d, max %d; vnMatch1 entries per pair: mean %.1f; per pair %.2f us" %
          (dn.mean(), dn.min(), dn.max(), (d1 >= 0).sum() / P, 1e3 * t / P), flush=True)
    sample = np.unique(np.linspace(0, P - 1, min(host_sample, P)).astype(int))
    host_loop(pairs[sample[:1]])           # warm
    dt, hm, h1, h2, hn = host_loop(pairs[sample])
    same = sum(int(hn[r] == dn[q] and np.array_equal(hm[r], dm[q]) and np.array_equal(h1[r], d1[q]) and np.array_equal(h2[r], d2[q])) for r, q in enumerate(sample))
    print("  loop it replaces: olf_search_by_sim3 x %d pairs %.1f ms, %.3f ms per pair (host clock, views already on the host); %d of %d pairs identical to the entry's" %
          (len(sample), 1e3 * dt, 1e3 * dt / len(sample), same, len(sample)), flush=True)
    print("  loop per pair / entry per pair: %.0f" % ((dt / len(sample)) / (1e-3 * t / P)), flush=True)
    bad += len(sample) - same


for ncand in (8, 32):
    if B > ncand:
        shape(f"one round, {ncand} candidates", [(ncand, c) for c in range(ncand)], ncand)
shape("throughput", [(j, j - 1) for j in range(1, B)], args.host_pairs)
ctx.close()
if bad:
    sys.exit("the host form and the device entry disagree")
