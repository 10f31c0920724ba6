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
import sys, time
import numpy as np
from latency_common import BenchBatch, host_view, parser, up, zeros as z
import torch
from orb_line_slam_amd import _lib, matcher

ap = parser("stereo pairs = key frames of the batch (0: the configuration's default)")
ap.add_argument("--host-pairs", type=int, default=64, help="pairs of the throughput shape, evenly spread, the host loop covers")
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
print(f"{args.config} {W}x{H}, {B} key frames, capacity {cap}, key points per frame: mean {cnt.mean():.0f}, of which hold a point: {hv.sum() / B:.0f}; th 7.5",
      flush=True)
views = {}


def kf_view(j):
    if j not in views:
        n = int(min(cnt[j], cap))
        views[j] = (host_view(batch, j, "keyframe", mTcw=np.eye(4, dtype=np.float32), mp_valid=hv[j, :n].copy(), mp_bad=np.zeros(n, bool), mp_world=hw[j, :n],
                               mp_desc=hd[j, :n], mp_maxd=h_maxd[j, :n], mp_mind=h_mind[j, :n]), n)
    return views[j]


R_I, t_0 = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)
p = lambda a: a.ctypes.data


def host_loop(pairs):
    """olf_search_by_sim3 per pair: (seconds, rows, vnMatch1 rows, vnMatch2 rows, counts)"""
    vs = [(kf_view(int(a)), kf_view(int(b))) for a, b in pairs]          # (laying the arrays out for the C ABI is not counted)
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
    t = batch.timed(f"{tag}: olf_search_by_sim3_pairs_dev, {P} pairs of {nf} frames", run)
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
