"""Latency of the two key-frame forms of SearchByProjection for batches (olf_search_by_projection_kf_pairs_dev, olf_search_by_projection_sim3_batch_dev,
csrc/projection_batch.hip) beside the loops they replace -- olf_search_by_projection_kf and olf_search_by_projection_sim3, one host call per pair or key
frame, with the views already on the host -- on the left frames of the bench's synthetic batch: identity poses, a feature holds a map point where it has a
stereo depth (olf_unproject_stereo_dev), mfMaxDistance from the depth and the octave.  Shapes:
  one relocalisation round   one frame against 8 and against 32 candidate key frames (Tracking::Relocalization), th / ORBdist = 10 / 100 and 3 / 64
  one loop projection        8 and 32 key frames against the points of one other frame under the identity Sim3 (LoopClosing::ComputeSim3), th = 10 and 6
python tools/projection_pairs_latency.py [--config C3] [--pairs 3072]
Device entries: HIP events, warmed up, median of five windows of ten calls; the loop form's calls start from vpMatched = NULL, so the refill of that array
is inside the window.  Host loops: host clock, ending in a synchronise.  Every looped pair / key frame is compared with the entry's row and count; a
difference ends the tool with a non-zero status."""
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
print(f"{args.config} {W}x{H}, {B} key frames, capacity {cap}, key points per frame: mean {cnt.mean():.0f}, of which hold a point: {hv.sum() / B:.0f}",
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


def host_view(j, role="kf"):
    """frame j as an olf_frame_view: in the key-frame role with the points it holds, in the current-frame role with an mvpMapPoints mask of its own"""
    if (j, role) not in views:
        n = int(min(cnt[j], cap))
        v = ola.KeyFrameView.__new__(ola.KeyFrameView)       # (no Python grid: the host form builds its own)
        v.mvKeysUn, v.mDescriptors, v.mvuRight, v.N, v.mvScaleFactors = hk[j, :n], hd[j, :n], None, n, sf
        v.fx = v.fy = fx; v.cx, v.cy, v.mbf = cx, cy, mbf
        v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY = bounds
        v.mTcw, v.mFeatVec = np.eye(4, dtype=np.float32), {}
        v.mp_valid, v.mp_bad, v.mp_obs, v.mvbOutlier = (hv[j, :n].copy() if role == "kf" else np.zeros(n, bool)), np.zeros(n, bool), None, None
        v.mp_world, v.mp_desc, v.mp_maxd, v.mp_mind = hw[j, :n], hd[j, :n], h_maxd[j, :n], h_mind[j, :n]
        views[(j, role)] = (matcher._view_c(v, keep), n, v)
    return views[(j, role)]


p = lambda a: a.ctypes.data
bad = 0


def reloc_round(ncand, th, orb):
    """frame ncand against the key frames 0 .. ncand - 1"""
    global bad
    pairs = np.ascontiguousarray([(ncand, c) for c in range(ncand)], np.int32)
    P, nf = len(pairs), ncand + 1
    d_pairs = torch.from_numpy(pairs).cuda()
    out = (z((P, cap), torch.int32), z((P,), torch.int32))

    def run():
        matcher.search_by_projection_kf_pairs(nf, kps, desc, counts, offs, idx, world, maxd, mind, d_pairs, cam, bounds, th=th, ORBdist=orb, Tcw=eye,
                                              mp_valid=valid, out=out, context=ctx)
    t = timed(f"relocalisation, {ncand} candidates, th {th:g} ORBdist {orb}: olf_search_by_projection_kf_pairs_dev", run)
    ctx.poll_status()
    dm, dn = out[0].cpu().numpy(), out[1].cpu().numpy()
    cur, ncur, vcur = host_view(ncand, "cur")
    kfs = [host_view(c) for c in range(ncand)]
    hm, hn = np.full((P, cap), -1, np.int32), np.zeros(P, np.int32)

    def loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r, (vk, nk, _) in enumerate(kfs):
            vcur.mp_valid[:] = False                         # (every candidate starts from its own copy of the frame's map points: none here)
            rc = L.olf_search_by_projection_kf(ctx.handle, cur, vk, None, th, orb, 1, p(hm[r]), p(hn[r:]))
            assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    loop()
    dt = loop()
    same = sum(int(hn[r] == dn[r] and np.array_equal(hm[r], dm[r])) for r in range(P))
    print("  nmatches per pair: mean %.1f, min %d, max %d" % (dn.mean(), dn.min(), dn.max()), flush=True)
    print("  loop it replaces: olf_search_by_projection_kf x %d pairs %.2f ms (host clock, views already on the host); %d of %d pairs identical to the entry's; loop / entry: %.1f"
          % (P, 1e3 * dt, same, P, 1e3 * dt / t), flush=True)
    bad += P - same


def loop_round(nkf, th):
    """the key frames 0 .. nkf - 1 against the points frame nkf holds, under the identity Sim3"""
    global bad
    n = int(min(cnt[nkf], cap))
    held = np.flatnonzero(hv[nkf, :n])
    m_world = np.ascontiguousarray(hw[nkf, held])
    m_normal = (m_world / np.linalg.norm(m_world.astype(np.float64), axis=1)[:, None]).astype(np.float32)
    m_maxd, m_mind, m_desc = np.ascontiguousarray(h_maxd[nkf, held]), np.ascontiguousarray(h_mind[nkf, held]), np.ascontiguousarray(hd[nkf, held])
    n_mp = len(held)
    lm = matcher.LocalMapDev(up(m_world), up(m_normal), up(m_maxd), up(m_mind), up(m_desc), None, z((n_mp,), torch.uint8))
    Scw = eye[:nkf].contiguous()
    fm = torch.full((nkf, cap), -1, dtype=torch.int32, device="cuda")
    nm = z((nkf,), torch.int32)

    def run():
        fm.fill_(-1)
        matcher.search_by_projection_sim3_batch(nkf, kps, desc, counts, offs, idx, lm, Scw, fm, cam, bounds, th=th, out=nm, context=ctx)
    t = timed(f"loop form, {nkf} key frames x {n_mp} points, th {th:g}: olf_search_by_projection_sim3_batch_dev", run)
    ctx.poll_status()
    dm, dn = fm.cpu().numpy(), nm.cpu().numpy()
    kfs = [host_view(c) for c in range(nkf)]
    hm, hn = np.full((nkf, cap), -1, np.int32), np.zeros(nkf, np.int32)
    S_I, skip = np.eye(4, dtype=np.float32), np.zeros(n_mp, np.uint8)
    matched = np.zeros(cap, np.uint8)

    def loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r, (vk, nk, _) in enumerate(kfs):
            matched[:] = 0
            rc = L.olf_search_by_projection_sim3(ctx.handle, vk, p(S_I), n_mp, p(skip), p(m_world), p(m_normal), p(m_maxd), p(m_mind), p(m_desc), float(th),
                                                 p(matched), p(hm[r]), p(hn[r:]))
            assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    loop()
    dt = loop()
    same = sum(int(hn[r] == dn[r] and np.array_equal(hm[r], dm[r])) for r in range(nkf))
    print("  nmatches per key frame: mean %.1f, min %d, max %d" % (dn.mean(), dn.min(), dn.max()), flush=True)
    print("  loop it replaces: olf_search_by_projection_sim3 x %d key frames %.2f ms (host clock, views already on the host); %d of %d identical to the entry's; loop / entry: %.1f"
          % (nkf, 1e3 * dt, same, nkf, 1e3 * dt / t), flush=True)
    bad += nkf - same


for ncand in (8, 32):
    if B > ncand:
        for th, orb in ((10.0, 100), (3.0, 64)):
            reloc_round(ncand, th, orb)
for nkf in (8, 32):
    if B > nkf:
        for th in (10.0, 6.0):
            loop_round(nkf, th)
ctx.close()
if bad:
    sys.exit("a host form and its device entry disagree")
