"""Latency of the batched SearchForTriangulation (csrc/triangulation_batch.hip) beside the only other way to get its results -- a loop of
olf_search_for_triangulation, one host call per key-frame pair, with the views and their feature vectors already on the host -- on the left frames of
the bench's synthetic batch: every frame against its 10 predecessors (the shape of LocalMapping::CreateNewMapPoints), F12 for identity rotation and a
sideways baseline of 0.05 m per frame, an ORBvoc-shaped (k = 10, L = 6) vocabulary drawn from the batch, levelsup 4; a feature holds a map point where
it has a stereo depth:  python tools/triangulation_latency.py [--config C3] [--pairs 3072] [--host-pairs 64]
Device entry: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise."""
import time
import numpy as np
from latency_common import BenchBatch, host_view, parser, zeros as z
import torch
from orb_line_slam_amd import _lib, matcher
from orb_line_slam_amd.vocabulary import ORBVocabulary
import bench

ap = parser("stereo pairs = frames of the batch (0: the configuration's default)")
ap.add_argument("--neighbours", type=int, default=10, help="predecessors every frame is matched against")
ap.add_argument("--host-pairs", type=int, default=64, help="key-frame pairs, evenly spread over the list, the host loop covers")
args = ap.parse_args()
batch = BenchBatch(args)
ctx, L, W, H, B, cap = batch.ctx, batch.L, batch.W, batch.H, batch.B, batch.cap
kps, desc, counts, ur, valid = batch.kps, batch.desc, batch.counts, batch.ur, batch.valid
torch.cuda.synchronize()
fx, _, cx, cy = cam = batch.cam[:4]
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
print(f"{args.config} {W}x{H}, {B} frames, {P} key-frame pairs ({args.neighbours} predecessors each), capacity {cap}, levelsup 4", flush=True)
t_batch = batch.timed("olf_search_for_triangulation_batch_dev (ComputeBoW included)", search)
m_dev, n_dev = out[0].cpu().numpy(), out[1].cpu().numpy()
cnt, hv = batch.cnt, batch.hv
free = np.array([(~hv[j, :cnt[j]]).sum() for j in range(B)])
print("  key points per frame: mean %.0f, without a map point: mean %.0f; matches per pair: mean %.2f, min %d, max %d" %
      (cnt.mean(), free.mean(), n_dev.mean(), n_dev.min(), n_dev.max()), flush=True)
print("  batch entry per pair: %.2f us" % (1e3 * t_batch / max(P, 1)), flush=True)

# the host form, one call per pair of a sample, on downloaded arrays whose feature vectors are already made
sample = np.unique(np.linspace(0, P - 1, min(args.host_pairs, P)).astype(int)) if P else np.zeros(0, int)
hd, hu = batch.hd, batch.hu
views = {}
for j in sorted({int(f) for q in sample for f in pairs[q]}):
    n = int(cnt[j])
    views[j] = host_view(batch, j, mvuRight=hu[j, :n], mTcw=hT[j], mp_valid=hv[j, :n].copy(), mFeatVec=voc.transform(hd[j, :n], 4)[1])
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
