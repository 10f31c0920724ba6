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
import sys, time
import numpy as np
from latency_common import BenchBatch, host_view, parser, up, zeros as z
import torch
from orb_line_slam_amd import _lib, matcher

ap = parser("stereo pairs = key frames of the batch (0: the configuration's default)")
args = ap.parse_args()
batch = BenchBatch(args, tag_width=66)
ctx, L, W, H, B, cap = batch.ctx, batch.L, batch.W, batch.H, batch.B, batch.cap
kps, desc, counts, valid = batch.kps, batch.desc, batch.counts, batch.valid
cam, bounds, offs, idx = batch.cam, batch.bounds, batch.offs, batch.idx
batch.grid()
eye, world = batch.eye, batch.world
torch.cuda.synchronize()
sf = batch.sf

# the per-feature map-point arrays, made on the host (the host loop reads them there), then uploaded
hv, hw, hk, hd, cnt = batch.hv, batch.hw, batch.hk, batch.hd, batch.cnt
dist = np.linalg.norm(hw.astype(np.float64), axis=2)
h_maxd = (dist * sf[np.clip(hk["octave"], 0, ctx.nlevels - 1)] * 0.95).astype(np.float32)
h_mind = (h_maxd / sf[-1]).astype(np.float32)
maxd, mind = up(h_maxd), up(h_mind)
print(f"{args.config} {W}x{H}, {B} key frames, capacity {cap}, key points per frame: mean {cnt.mean():.0f}, of which hold a point: {hv.sum() / B:.0f}",
      flush=True)
views = {}


def role_view(j, role="kf"):
    """frame j as an olf_frame_view: in the key-frame role with the points it holds, in the current-frame role with an mvpMapPoints mask of its own (returned
    beside the view, for the loop to clear)"""
    if (j, role) not in views:
        n = int(min(cnt[j], cap))
        held = hv[j, :n].copy() if role == "kf" else np.zeros(n, bool)
        views[(j, role)] = (host_view(batch, j, "keyframe", mTcw=np.eye(4, dtype=np.float32), mp_valid=held, mp_bad=np.zeros(n, bool), mp_world=hw[j, :n],
                                       mp_desc=hd[j, :n], mp_maxd=h_maxd[j, :n], mp_mind=h_mind[j, :n]), n, held)
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
    t = batch.timed(f"relocalisation, {ncand} candidates, th {th:g} ORBdist {orb}: olf_search_by_projection_kf_pairs_dev", run)
    ctx.poll_status()
    dm, dn = out[0].cpu().numpy(), out[1].cpu().numpy()
    cur, ncur, cur_held = role_view(ncand, "cur")
    kfs = [role_view(c) for c in range(ncand)]
    hm, hn = np.full((P, cap), -1, np.int32), np.zeros(P, np.int32)

    def loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r, (vk, nk, _) in enumerate(kfs):
            cur_held[:] = False                             # (every candidate starts from its own copy of the frame's map points: none here)
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
    t = batch.timed(f"loop form, {nkf} key frames x {n_mp} points, th {th:g}: olf_search_by_projection_sim3_batch_dev", run)
    ctx.poll_status()
    dm, dn = fm.cpu().numpy(), nm.cpu().numpy()
    kfs = [role_view(c) for c in range(nkf)]
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
