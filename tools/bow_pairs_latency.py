"""Latency of SearchByBoW over a pair list (olf_search_by_bow_pairs_dev, csrc/bow_match.hip), both forms, beside the loop it replaces -- olf_bow_transform
per frame, then olf_search_by_bow (frame form) or olf_search_by_bow_kf (key-frame form) per pair, on downloaded arrays -- on the left frames of the
bench's synthetic batch, an ORBvoc-shaped (k = 10, L = 6) vocabulary drawn from the batch, levelsup 4, nnratio 0.7; a feature holds a map point where it
has a stereo depth.  Two shapes per form:
  relocalisation   one frame against 8 and against 32 candidate key frames (Tracking::Relocalization, LoopClosing::ComputeSim3), 2000 features each
  throughput       every frame of the batch against its predecessor (a few thousand pairs)
python tools/bow_pairs_latency.py [--config C3] [--pairs 3072] [--host-pairs 64]
Device entry: HIP events, warmed up, median of five windows of ten calls.  Host loop: host clock, ending in a synchronise; the throughput shape's loop
covers a sample of the pairs.  Every host result is checked against the device entry's."""
import argparse, ctypes as C, os, sys, time
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
check(L.olf_orb_extract_dev(ctx.handle, imgs.data_ptr(), 2 * B, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), s), "olf_orb_extract_dev")
check(L.olf_stereo_points_dev(ctx.handle, B, kps.data_ptr(), desc.data_ptr(), counts.data_ptr(), ur.data_ptr(), dp.data_ptr(), s), "olf_stereo_points_dev")
check(L.olf_stereo_points_mask_dev(ctx.handle, dp.data_ptr(), B * cap, valid.data_ptr(), s), "olf_stereo_points_mask_dev")
torch.cuda.synchronize()
cn0, de0 = counts[:16].cpu().numpy(), desc[:16].cpu().numpy()
voc = ORBVocabulary.from_arrays(10, 6, *bench.synthetic_vocabulary(10, 6, np.concatenate([de0[i, :cn0[i]] for i in range(min(2 * B, 16))])), context=ctx)
cnt = counts.cpu().numpy()[0::2]
print(f"{args.config} {W}x{H}, {B} frames, capacity {cap}, key points per frame: mean {cnt.mean():.0f}; levelsup 4, nnratio 0.7", flush=True)


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


# the host side: downloaded arrays, one view per frame, made when a loop first needs the frame
hk = kps.cpu().numpy().reshape(2 * B, cap * 28).view(KEYPOINT_DTYPE)[0::2]
hd, hv = desc.cpu().numpy()[0::2], valid.cpu().numpy().astype(bool)
sf = np.zeros(ctx.nlevels, np.float32)
L.olf_orb_scale_tables(ctx.handle, sf.ctypes.data, None, None, None, None)
keep = []


def host_view(j, fv):
    n = int(cnt[j])
    v = ola.FrameView.__new__(ola.FrameView)             # (no Python grid: this search reads none)
    v.mvKeysUn, v.mvKeys, v.mDescriptors, v.mvuRight, v.N, v.mvScaleFactors = hk[j, :n], hk[j, :n], hd[j, :n], None, n, sf
    v.fx = v.fy = float(cfg["fx"]); v.cx, v.cy, v.mbf = W / 2.0, H / 2.0, float(cfg["bf"])
    v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY = 0.0, float(W), 0.0, float(H)
    v.mTcw, v.mp_valid, v.mp_bad = None, hv[j, :n].copy(), np.zeros(n, bool)
    v.mp_world, v.mp_desc, v.mp_obs, v.mvbOutlier = None, None, None, None
    v.mFeatVec = fv
    return matcher._view_c(v, keep)


def host_loop(frames, pairs, form):
    """olf_bow_transform per frame of `frames`, then the host search per pair: (seconds for the transforms, seconds for the searches, rows, counts)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fvs = {j: voc.transform(hd[j, :int(cnt[j])], 4)[1] for j in frames}
    t1 = time.perf_counter()
    views = {j: host_view(j, fvs[j]) for j in frames}          # (laying the arrays out for the C ABI is not counted)
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
        t = timed(f"{tag}, {name}: olf_search_by_bow_pairs_dev, {P} pairs of {nf} frames", run)
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
