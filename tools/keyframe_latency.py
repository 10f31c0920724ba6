"""Latency of the batched key-frame step (csrc/keyframe_batch.hip) -- olf_stereo_landmarks_batch_dev in its two sorted modes and
olf_need_new_keyframe_batch_dev -- on the left frames of the bench's synthetic batch, at the whole batch and at one frame, beside their host forms on 16
threads (the host forms are plain C and the wrappers release the interpreter lock: a thread per chunk of frames).  Every second feature holds a landmark,
half of those without observations; identity poses.  python tools/keyframe_latency.py [--config C3] [--pairs 3072] [--host-frames 512] [--threads 16]
Device entries: HIP events, warmed up, median of five windows of ten calls.  Host forms: host clock over a sample of the frames, results compared with the
device's.  The bytes a call moves are computed from the shapes: the planes it reads (for created features also their key point or key line) plus every
output plane."""
import time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
from latency_common import BenchBatch, parser, up
import torch
from orb_line_slam_amd import _lib, keyframe

ap = parser("stereo pairs = frames of the batch (0: the configuration's default)")
ap.add_argument("--host-frames", type=int, default=512, help="frames, evenly spread over the batch, the host forms cover")
ap.add_argument("--threads", type=int, default=16, help="threads the host forms run on")
args = ap.parse_args()
batch = BenchBatch(args)
ctx, B, cap, lcap = batch.ctx, batch.B, batch.cap, batch.ctx.line_capacity
kps, counts, dp, kls, lcounts, ldisp, eye = batch.kps, batch.counts, batch.dp, batch.kls, batch.lcounts, batch.ldisp, batch.eye
torch.cuda.synchronize()
th_depth = batch.mbf * 35.0 / batch.fx                               # mThDepth = mbf * ThDepth / fx
nobs = np.array([0, 2], np.int32)
h_fmp = np.tile(np.where(np.arange(cap) % 2, np.arange(cap) // 2 % 2, -1).astype(np.int32), (B, 1))
h_fml = np.tile(np.where(np.arange(lcap) % 2, np.arange(lcap) // 2 % 2, -1).astype(np.int32), (B, 1))
fmp, fml, d_nobs = up(h_fmp), up(h_fml), up(nobs)
print(f"{args.config} {batch.W}x{batch.H}, {B} frames, capacity {cap} key points / {lcap} key lines, thDepth {th_depth:.3f}", flush=True)

outs = {}
for mode, name in ((keyframe.LANDMARKS_KEYFRAME, "KEYFRAME"), (keyframe.LANDMARKS_LASTFRAME, "LASTFRAME")):
    for n in (B, 1):
        out = {k: torch.zeros(shape, dtype=keyframe._torch_dtype(dt), device="cuda") for k, (shape, dt) in keyframe._landmark_shapes(n, cap, lcap).items()}
        call = lambda: keyframe.stereo_landmarks_batch(n, mode, kps, counts, kls, lcounts, dp, ldisp, eye, batch.cam, th_depth, frame_mp=fmp, frame_ml=fml, mp_nobs=d_nobs,
                                                       ml_nobs=d_nobs, n_mp=2, n_ml=2, img_stride=2, out=out, context=ctx)
        t = batch.timed(f"olf_stereo_landmarks_batch_dev {name}, {n} frame{'s' * (n > 1)}", call)
        if n == B:
            outs[mode] = {k: v.cpu().numpy() for k, v in out.items()}
            nc = outs[mode]["n_created"].astype(np.int64)
            read = B * (cap * 4 + lcap * 8 + cap * 4 + lcap * 4 + 64 + 8) + int(nc[:, 0].sum()) * 28 + int(nc[:, 1].sum()) * 68
            written = sum(v.nbytes for v in outs[mode].values())
            print("  visited per frame: %.1f points, %.1f lines; created: %.1f, %.1f; %.1f MB read + %.1f MB written: %.1f GB/s; %.2f us per frame" %
                  (*outs[mode]["n_visited"].mean(0), *nc.mean(0), read / 1e6, written / 1e6, (read + written) / (1e6 * t), 1e3 * t / B), flush=True)

rows = keyframe.keyframe_rows([dict(mnId=100 + j, mnLastKeyFrameId=90 + j % 40, mMaxFrames=30, nKFs=5, bLocalMappingIdle=j & 1, KeyframesInQueue=j % 4) for j in range(B)])
nref, ninl = np.full(B, 100, np.int32), np.stack([20 + np.arange(B) % 70, 20 + np.arange(B) % 60], 1).astype(np.int32)
outl = torch.zeros((B, cap), dtype=torch.uint8, device="cuda")
outl_l = torch.zeros((B, lcap), dtype=torch.uint8, device="cuda")
d_rows, d_nref, d_ninl = up(rows), up(nref), up(ninl)
for n in (B, 1):
    tout = {k: torch.zeros(shape, dtype=keyframe._torch_dtype(dt), device="cuda") for k, (shape, dt) in keyframe._test_shapes(n).items()}
    call = lambda: keyframe.need_new_keyframe_batch(n, counts, lcounts, dp, ldisp, d_rows, d_nref, d_nref, d_ninl, batch.mbf, th_depth, frame_mp=fmp, outlier=outl,
                                                    frame_ml=fml, outlier_l=outl_l, img_stride=2, out=tout, context=ctx)
    t = batch.timed(f"olf_need_new_keyframe_batch_dev, {n} frame{'s' * (n > 1)}", call)
    if n == B:
        test = {k: v.cpu().numpy() for k, v in tout.items()}
        read = B * (cap * 9 + lcap * 13 + 4 * (2 + 11 + 4))
        print("  key frames needed: %d of %d; %.1f MB read: %.1f GB/s; %.2f us per frame" % (test["need"].sum(), B, read / 1e6, read / (1e6 * t), 1e3 * t / B), flush=True)

# the host forms over a sample of the frames, a chunk per thread
sample = np.unique(np.linspace(0, B - 1, min(args.host_frames, B)).astype(int))
hk, hcnt = np.ascontiguousarray(batch.hk[sample]), np.ascontiguousarray(batch.cnt[sample])
hkl = np.ascontiguousarray(kls.cpu().numpy().reshape(2 * B, lcap * 68).view(_lib.KEYLINE_DTYPE)[0::2][sample])
hlcnt = np.ascontiguousarray(lcounts.cpu().numpy()[0::2][sample])
hdp, hld, heye = dp.cpu().numpy()[sample], ldisp.cpu().numpy()[sample], np.tile(np.eye(4, dtype=np.float32), (len(sample), 1, 1))
chunks = [c for c in np.array_split(np.arange(len(sample)), args.threads) if len(c)]


def host_landmarks(mode, c):
    fn = keyframe.CreateNewKeyFrame if mode == keyframe.LANDMARKS_KEYFRAME else keyframe.UpdateLastFrame
    return fn(hk[c], hcnt[c], hkl[c], hlcnt[c], hdp[c], hld[c], heye[c], batch.cam, th_depth, batch.sf, frame_mp=h_fmp[sample][c], frame_ml=h_fml[sample][c], mp_nobs=nobs,
              ml_nobs=nobs)


def host_need(c):
    return keyframe.NeedNewKeyFrame(hcnt[c], hlcnt[c], hdp[c], hld[c], rows[sample][c], nref[sample][c], nref[sample][c], ninl[sample][c], batch.mbf, th_depth,
                                    frame_mp=h_fmp[sample][c], frame_ml=h_fml[sample][c])


with ThreadPoolExecutor(args.threads) as pool:
    for mode, name in ((keyframe.LANDMARKS_KEYFRAME, "KEYFRAME"), (keyframe.LANDMARKS_LASTFRAME, "LASTFRAME")):
        t0 = time.perf_counter()
        parts = list(pool.map(lambda c: host_landmarks(mode, c), chunks))
        dt = time.perf_counter() - t0
        same = all(np.array_equal(np.concatenate([p[k] for p in parts]).view(np.uint8), outs[mode][k][sample].view(np.uint8)) for k in outs[mode])
        print("%-58s %8.3f ms for %d frames on %d threads, %.2f us per frame (host clock, through the Python wrapper); identical to the device: %s" %
              (f"olf_stereo_landmarks {name}", 1e3 * dt, len(sample), len(chunks), 1e6 * dt / len(sample), same), flush=True)
        assert same, "the host form and the device entry disagree"
    t0 = time.perf_counter()
    parts = list(pool.map(host_need, chunks))
    dt = time.perf_counter() - t0
    same = all(np.array_equal(np.concatenate([p[k] for p in parts]), test[k][sample]) for k in test)
    print("%-58s %8.3f ms for %d frames on %d threads, %.2f us per frame (host clock, through the Python wrapper); identical to the device: %s" %
          ("olf_need_new_keyframe", 1e3 * dt, len(sample), len(chunks), 1e6 * dt / len(sample), same), flush=True)
    assert same, "the host form and the device entry disagree"
ctx.close()
