"""Latency of the batched ComputeF12, CreateNewMapPoints and UpdateNormalAndDepth (csrc/newpoints_batch.hip) beside loops of their host forms, on the left
frames of the bench's synthetic batch: every frame against its 10 predecessors (the shape of LocalMapping::CreateNewMapPoints), identity rotations and a
sideways baseline of 0.05 m per frame, the match rows of olf_search_for_triangulation_batch_dev (vocabulary and settings of tools/triangulation_latency.py;
not timed here), monocular = 1 so that no pair is skipped for its baseline; then one map point per (pair, idx1) slot, observed by the pair's two key
frames and bad where nothing was created, for UpdateNormalAndDepth:  python tools/newpoints_latency.py [--config C3] [--pairs 3072] [--host-pairs 64]
Device entries: HIP events, warmed up, median of five windows of ten calls.  Host loops: host clock, on a sample of the pairs, results checked."""
import time
import numpy as np
from latency_common import BenchBatch, parser, up, zeros as z
import torch
from orb_line_slam_amd import _lib, matcher, newpoints
from orb_line_slam_amd.vocabulary import ORBVocabulary
import bench

ap = parser("stereo pairs = frames of the batch (0: the configuration's default)")
ap.add_argument("--neighbours", type=int, default=10, help="predecessors every frame is matched against")
ap.add_argument("--host-pairs", type=int, default=64, help="key-frame pairs, evenly spread over the list, the host loops cover")
args = ap.parse_args()
batch = BenchBatch(args)
ctx, W, H, B, cap = batch.ctx, batch.W, batch.H, batch.B, batch.cap
kps, desc, counts, ur, dp, valid = batch.kps, batch.desc, batch.counts, batch.ur, batch.dp, batch.valid
torch.cuda.synchronize()
cam4, cam5 = batch.cam[:4], batch.cam
mb = float(np.float32(batch.mbf) / np.float32(batch.fx))
hT = np.stack([np.eye(4, dtype=np.float32)] * B)
hT[:, 0, 3] = -0.05 * np.arange(B)
pairs = np.array([(j, j - d) for j in range(B) for d in range(1, args.neighbours + 1) if j - d >= 0], np.int32).reshape(-1, 2)
P = len(pairs)
Tcw, d_pairs = up(hT), up(pairs)
print(f"{args.config} {W}x{H}, {B} frames, {P} key-frame pairs ({args.neighbours} predecessors each), capacity {cap}", flush=True)

# ComputeF12
F12 = z((P, 9), torch.float32)
t_f12 = batch.timed("olf_compute_f12_pairs_dev", lambda: newpoints.compute_f12_pairs(Tcw, cam4, d_pairs, out=F12, context=ctx))
hF = F12.cpu().numpy()
sample = np.unique(np.linspace(0, P - 1, min(args.host_pairs, P)).astype(int)) if P else np.zeros(0, int)
t0 = time.perf_counter()
hostF = [newpoints.ComputeF12(hT[a], hT[b], cam4).reshape(-1) for a, b in pairs[sample]]
dt = time.perf_counter() - t0
assert all(np.array_equal(hostF[r].view(np.uint32), hF[q].view(np.uint32)) for r, q in enumerate(sample)), "olf_compute_f12 and the batch entry disagree"
print("%-58s %8.3f ms per pair (host clock, through the Python wrapper); %d pairs identical to the batch entry" % ("loop of olf_compute_f12", 1e3 * dt / max(len(sample), 1), len(sample)), flush=True)

# the match rows
cn0, de0 = counts[:16].cpu().numpy(), desc[:16].cpu().numpy()
voc = ORBVocabulary.from_arrays(10, 6, *bench.synthetic_vocabulary(10, 6, np.concatenate([de0[i, :cn0[i]] for i in range(min(2 * B, 16))])), context=ctx)
m12, nm = matcher.search_for_triangulation_batch(voc, B, kps, desc, counts, ur, Tcw, d_pairs, F12, cam4, mp_valid=valid, levelsup=4, context=ctx)

# CreateNewMapPoints
out = (z((P, cap, 3), torch.float32), z((P, cap), torch.uint8), z((P,), torch.int32))
create = lambda: newpoints.create_new_map_points_batch(B, kps, counts, ur, dp, Tcw, cam5, mb, d_pairs, m12, monocular=True, img_stride=2, out=out, context=ctx)
t_new = batch.timed("olf_create_new_map_points_batch_dev", create)
x3D, code, nnew = (t.cpu().numpy() for t in out)
n_m = nm.cpu().numpy()
print("  matches per pair: mean %.2f, max %d; created per pair: mean %.2f; codes: %s" %
      (n_m.mean(), n_m.max(), nnew.mean(), dict(zip(*(v.tolist() for v in np.unique(code[code > 0], return_counts=True))))), flush=True)
print("  batch entry per pair: %.2f us, per match: %.3f us" % (1e3 * t_new / max(P, 1), 1e3 * t_new / max(int(n_m.sum()), 1)), flush=True)
hk, cnt, hu, hdp, hm12 = np.ascontiguousarray(batch.hk), np.ascontiguousarray(batch.cnt), batch.hu, dp.cpu().numpy(), m12.cpu().numpy()
if len(sample):
    t0 = time.perf_counter()
    hx, hc, hn, hs = newpoints.CreateNewMapPoints(hk, cnt, hu, hdp, hT, cam5, mb, batch.sf, pairs[sample], hm12[sample], monocular=True)
    dt = time.perf_counter() - t0
    same = sum(int(hn[r] == nnew[q] and np.array_equal(hc[r], code[q]) and np.array_equal(hx[r].view(np.uint32), x3D[q].view(np.uint32))) for r, q in enumerate(sample))
    print("%-58s %8.3f ms per pair, %.1f ms for %d pairs (host clock, arrays already on the host); %d of %d pairs identical to the batch entry" %
          ("olf_create_new_map_points over the sample", 1e3 * dt / len(sample), 1e3 * dt, len(sample), same, len(sample)), flush=True)
    print("  host form per pair / batch entry per pair: %.0f" % ((dt / len(sample)) / (1e-3 * t_new / P)), flush=True)
    assert same == len(sample) and hs == 0, "the host form and the batch entry disagree"

# UpdateNormalAndDepth: one point per (pair, idx1) slot
n_mp = P * cap
made = (out[1] >= 1) & (out[1] <= 3)
slot1 = torch.arange(cap, dtype=torch.int32, device="cuda").repeat(P)
obs_kf = d_pairs.repeat_interleave(cap, 0).reshape(-1).contiguous()                       # (kf1, kf2) of every slot's pair
obs_slot = torch.stack([slot1, torch.clamp(m12.reshape(-1), min=0)], 1).reshape(-1).contiguous()
obs_off = torch.arange(0, 2 * n_mp + 1, 2, dtype=torch.int32, device="cuda")
mp_bad = (~made).reshape(-1).to(torch.uint8)
kmp_off = torch.arange(0, (B + 1) * cap, cap, dtype=torch.int32, device="cuda")
octave = kps.reshape(2 * B, cap, 7, 4)[0::2, :, 5, 0].contiguous().clamp(max=ctx.nlevels - 1)      # the low byte of the octave of every left key point
hOw = np.zeros((B, 3), np.float32)
hOw[:, 0] = 0.05 * np.arange(B)
Ow, ref = up(hOw), d_pairs[:, 0].repeat_interleave(cap).contiguous()
g, v = _lib.MapGraphC(), _lib.CullViewC()
g.n_kf, g.n_mp = B, n_mp
g.mp_obs_offsets, g.mp_obs_kf, g.mp_bad, g.kf_mp_offsets, v.mp_obs_slot, v.kf_slot_octave = (t.data_ptr() for t in (obs_off, obs_kf, mp_bad, kmp_off, obs_slot, octave))
world = out[0].reshape(n_mp, 3)
normal, maxd, mind = z((n_mp, 3), torch.float32), z((n_mp,), torch.float32), z((n_mp,), torch.float32)
t_und = batch.timed("olf_update_normal_and_depth_dev (every slot)", lambda: newpoints.update_normal_and_depth(g, v, world, ref, Ow, normal, maxd, mind, context=ctx))
n_made = int(made.sum())
print("  %d points, %d of them not bad: %.3f us per point that is not bad" % (n_mp, n_made, 1e3 * t_und / max(n_made, 1)), flush=True)
lst = torch.nonzero(made.reshape(-1)).reshape(-1).to(torch.int32).contiguous()
t_lst = batch.timed("olf_update_normal_and_depth_dev (the list of created)", lambda: newpoints.update_normal_and_depth(g, v, world, ref, Ow, normal, maxd, mind, points=lst, context=ctx))
if len(sample):                                                       # the host form on the slots of the first pairs
    from orb_line_slam_amd import CullView, MapGraph
    hp = min(len(sample), P)
    ns = hp * cap
    h = lambda t, n: t[:n].cpu().numpy()
    hg = MapGraph(mp_obs=h(obs_kf, 2 * ns).reshape(ns, 2), mp_bad=h(mp_bad, ns), kf_bad=[0] * B, kf_mp=[[-1] * cap] * B, kf_covis=[[]] * B, kf_children=[[]] * B,
                  kf_parent=[-1] * B)
    hv = CullView(hg, mp_obs_slot=h(obs_slot, 2 * ns).reshape(ns, 2), mp_nobs=[2] * ns, kf_slot_octave=octave.cpu().numpy(), kf_slot_depth=np.zeros((B, cap)),
                  kf_slot_stereo=np.zeros((B, cap)), kf_th_depth=np.zeros(B), kf_mode=np.zeros(B))
    t0 = time.perf_counter()
    hn_, hmax, hmin, hs = newpoints.UpdateNormalAndDepth(hg, hv, x3D.reshape(n_mp, 3)[:ns], h(ref, ns), hOw, batch.sf)
    dt = time.perf_counter() - t0
    ok = all(np.array_equal(a.view(np.uint32), b[:ns].cpu().numpy().view(np.uint32)) for a, b in ((hn_, normal), (hmax, maxd), (hmin, mind)))
    n_s = int(made.reshape(-1)[:ns].sum())
    print("%-58s %8.3f us per point that is not bad, %.1f ms for the %d slots of %d pairs (host clock); identical to the device: %s" %
          ("olf_update_normal_and_depth", 1e6 * dt / max(n_s, 1), 1e3 * dt, ns, hp, ok), flush=True)
    assert ok and hs == 0, "the host form and the device entry disagree"
voc.clear()
ctx.close()
