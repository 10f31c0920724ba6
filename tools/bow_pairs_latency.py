"""Latency of SearchByBoW over a pair list (olf_search_by_bow_pairs_dev, csrc/bow_match.hip), both forms, beside the loop it replaces -- olf_bow_transform
per frame, then olf_search_by_bow (frame form) or olf_search_by_bow_kf (key-frame form) per pair, on downloaded arrays -- on the left frames of the
bench's synthetic batch, an ORBvoc-shaped (k = 10, L = 6) vocabulary drawn from the batch, levelsup 4, nnratio 0.7; a feature holds a map point where it
has a stereo depth.  Two shapes per form:
  relocalisation   one frame against 8 and against 32 candidate key frames (Tracking::Relocalization, LoopClosing::ComputeSim3), 2000 features each
  throughput       every frame of the batch against its predecessor (a few thousand pairs)
python tools/bow_pairs_latency.py [--config C3] [--pairs 3072] [--host-pairs 64]
Device entry: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise; the throughput shape's loop
covers a sample of the pairs.  Every host result is checked against the device entry's."""
import time
import numpy as np
from latency_common import BenchBatch, host_view, parser, zeros as z
import torch
from orb_line_slam_amd import _lib, matcher
from orb_line_slam_amd.vocabulary import ORBVocabulary
import bench

ap = parser("stereo pairs = frames of the batch (0: the configuration's default)")
ap.add_argument("--host-pairs", type=int, default=64, help="pairs of the throughput shape, evenly spread, the host loop covers")
args = ap.parse_args()
batch = BenchBatch(args, tag_width=66)
ctx, L, W, H, B, cap = batch.ctx, batch.L, batch.W, batch.H, batch.B, batch.cap
kps, desc, counts, valid = batch.kps, batch.desc, batch.counts, batch.valid
torch.cuda.synchronize()
cn0, de0 = counts[:16].cpu().numpy(), desc[:16].cpu().numpy()
voc = ORBVocabulary.from_arrays(10, 6, *bench.synthetic_vocabulary(10, 6, np.concatenate([de0[i, :cn0[i]] for i in range(min(2 * B, 16))])), context=ctx)
cnt = batch.cnt
print(f"{args.config} {W}x{H}, {B} frames, capacity {cap}, key points per frame: mean {cnt.mean():.0f}; levelsup 4, nnratio 0.7", flush=True)

# the host side: downloaded arrays, one view per frame, made when a loop first needs the frame
hd, hv = batch.hd, batch.hv


def host_loop(frames, pairs, form):
    """olf_bow_transform per frame of `frames`, then the host search per pair: (seconds for the transforms, seconds for the searches, rows, counts)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fvs = {j: voc.transform(hd[j, :int(cnt[j])], 4)[1] for j in frames}
    t1 = time.perf_counter()
    # (laying the arrays out for the C ABI is not counted)
    views = {j: host_view(batch, j, mp_valid=hv[j, :int(cnt[j])].copy(), mp_bad=np.zeros(int(cnt[j]), bool), mFeatVec=fvs[j]) for j in frames}
    fn = L.olf_search_by_bow if form == matcher.BOW_KF_FRAME else L.olf_search_by_bow_kf
    hm, hn = np.full((len(pairs), cap), -1, np.int32), np.zeros(len(pairs), np.int32)
    t2 = time.perf_counter()
    for r, (a, b) in enumerate(pairs):
        rc = fn(ctx.handle, views[int(a)], views[int(b)], 0.7, 1, hm[r].ctypes.data, hn[r:].ctypes.data)
        assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return t1 - t0, t3 - t2, hm, hn


def shape(tag, pairs, host_sample):
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    P = len(pairs)
    d_pairs = torch.from_numpy(pairs).cuda()
    # the entry builds the FeatureVector of every frame below n_frames: the relocalisation shapes hand over only the frames they name
    nf = int(pairs.max()) + 1
    for form, name in ((matcher.BOW_KF_FRAME, "OLF_BOW_KF_FRAME"), (matcher.BOW_KF_KF, "OLF_BOW_KF_KF")):
        out = (z((P, cap), torch.int32), z((P,), torch.int32))
        run = lambda: matcher.search_by_bow_pairs(voc, nf, kps, desc, counts, d_pairs, mp_valid=valid, form=form, nnratio=0.7, levelsup=4, out=out, context=ctx)
        t = batch.timed(f"{tag}, {name}: olf_search_by_bow_pairs_dev, {P} pairs of {nf} frames", run)
        m_dev, n_dev = out[0].cpu().numpy(), out[1].cpu().numpy()
        print("  matches per pair: mean %.1f, min %d, max %d; per pair %.2f us" % (n_dev.mean(), n_dev.min(), n_dev.max(), 1e3 * t / P), flush=True)
        sample = np.unique(np.linspace(0, P - 1, min(host_sample, P)).astype(int))
        frames = sorted({int(f) for q in sample for f in pairs[q]})
        host_loop(sorted({int(f) for f in pairs[sample[0]]}), pairs[sample[:1]], form)           # warm
        tt, ts, hm, hn = host_loop(frames, pairs[sample], form)
        same = sum(int(hn[r] == n_dev[q] and np.array_equal(hm[r], m_dev[q])) for r, q in enumerate(sample))
        print("  loop it replaces: olf_bow_transform x %d frames %.1f ms + %s x %d pairs %.1f ms = %.1f ms (host clock); %d of %d pairs identical to the entry's" %
              (len(frames), 1e3 * tt, "olf_search_by_bow" if form == matcher.BOW_KF_FRAME else "olf_search_by_bow_kf", len(sample), 1e3 * ts, 1e3 * (tt + ts), same,
               len(sample)), flush=True)
        if len(sample) == P:
            print("  loop / entry: %.0f" % (1e3 * (tt + ts) / t), flush=True)
        else:
            print("  loop per pair (transform per frame included) / entry per pair: %.0f" % ((tt / len(frames) + ts / len(sample)) / (1e-3 * t / P)), flush=True)
        assert same == len(sample), "the host form and the device entry disagree"


# first = the candidate key frame, second = the lost frame (frame form); first = the current key frame, second = the candidate (key-frame form): the
# lists below put the single frame second, and both forms run on the same list
for ncand in (8, 32):
    if B > ncand:
        shape(f"relocalisation {ncand}", [(c, ncand) for c in range(ncand)], ncand)
shape("throughput", [(j, j + 1) for j in range(B - 1)], args.host_pairs)
voc.clear()
ctx.close()
