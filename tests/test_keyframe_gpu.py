"""olf_stereo_landmarks_batch_dev and olf_need_new_keyframe_batch_dev on the device against their host forms and the line-by-line restatement
(tests/keyframe_reference.py) on every scene of tests/keyframe_scenes.py -- integers equal, floats and doubles equal as bit patterns --, with sentinel
outputs that show what is written, the chain into olf_search_by_projection_batch_dev on extracted frames, a full row at the default capacity, the
capacity error and the repeatability of a call."""
import ctypes as C
import numpy as np
import pytest
import keyframe_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, keyframe, synth
from orb_line_slam_amd._lib import OLF_ERR_CAPACITY
from test_keyframe_cpu import HOST, assert_planes, host_landmarks

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = {np.dtype(np.int32): -77, np.dtype(np.uint8): 99, np.dtype(np.float32): -7.5, np.dtype(np.float64): -7.5}


def context(nfeatures=None, nlines=None, w=640, h=480):
    p = _lib.default_params()
    if nfeatures is not None:
        p.orb.nfeatures = nfeatures
    if nlines is not None:
        p.line.lsd_nfeatures = nlines
    return _lib.Context(p, w, h, 2)


def scale_factors(c):
    sf = np.zeros(c.nlevels, F)
    _lib.lib().olf_orb_scale_tables(c.handle, sf.ctypes.data, None, None, None, None)
    return sf


@pytest.fixture(scope="module")
def ctx():
    c = context(S.CAP - 64, S.LCAP)                                  # (eight levels, eight spare key points each)
    assert c.orb_capacity == S.CAP and c.line_capacity == S.LCAP and np.array_equal(scale_factors(c), S.SF)
    yield c
    c.close()


def up(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a, dtype)
    if a.dtype.fields:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a).cuda()


def sentinel_outputs(shapes, extra_rows=1):
    """output tensors with extra_rows rows more than the call needs, every element a sentinel"""
    import torch
    out = {}
    for k, (shape, dt) in shapes.items():
        shape = (shape[0] + extra_rows,) + tuple(shape[1:])
        out[k] = torch.full(shape, SENTINEL[np.dtype(dt)], dtype=keyframe._torch_dtype(dt), device="cuda")
    return out


def untouched(t):
    import torch
    value = {torch.int32: -77, torch.uint8: 99, torch.float32: -7.5, torch.float64: -7.5}[t.dtype]
    return bool((t == value).all())


def device_landmarks(ctx, mode, frames, labels, img_stride=1, hold=True, bases=None, n_frames=None, double_lines=True):
    """the planes of the first n_frames frames as numpy arrays; the rows behind them must still hold their sentinels"""
    import torch
    c, lc = S.counts_of(labels, frames)
    a = S.batch_arrays(frames, c, lc, ctx.orb_capacity, ctx.line_capacity, img_stride)
    n = len(frames) if n_frames is None else n_frames
    kw = dict(mp_nobs=up(S.MP_NOBS), ml_nobs=up(S.ML_NOBS), n_mp=S.N_MP, n_ml=S.N_ML)
    if hold:
        kw.update(frame_mp=up(a["frame_mp"]), frame_ml=up(a["frame_ml"]))
    if bases is not None:
        kw.update(new_base_mp=up(bases[0]), new_base_ml=up(bases[1]))
    out = sentinel_outputs(keyframe._landmark_shapes(n, ctx.orb_capacity, ctx.line_capacity), len(frames) - n + 1)
    res = keyframe.stereo_landmarks_batch(n, mode, up(a["kps"]), up(a["counts"]), up(a["kls"]), up(a["lcounts"]), up(a["depth"]), up(a["ldisp"]), up(a["Twc"]), S.CAM5, S.TH,
                                          img_stride=img_stride, double_lines=double_lines, out=out, context=ctx, **kw)
    torch.cuda.synchronize()
    ctx.poll_status()                                                # (raises on a set bit) the frames' words, never the context's
    for k, t in out.items():
        assert untouched(t[n:]), k
    assert double_lines or untouched(out["ml_world_d"])
    return {k: t[:n].cpu().numpy() for k, t in res.items()}


# ---- the landmark entry ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("img_stride, hold, with_bases", [(1, True, False), (2, True, True), (1, False, False)])
def test_landmarks_against_host_and_reference(ctx, mode, img_stride, hold, with_bases):
    labels, frames = S.scene_set()
    n = len(frames)
    bases = (np.arange(n, dtype=np.int32) * 1000 + 7, np.arange(n, dtype=np.int32) * 300 - 5) if with_bases else None
    got = device_landmarks(ctx, mode, frames, labels, img_stride, hold, bases)
    host, exp = host_landmarks(mode, frames, labels, img_stride, hold, bases)
    assert_planes(got, host, labels)
    assert_planes(got, exp, labels)
    assert S.same(got["ml_world"], got["ml_world_d"].astype(F))


def test_landmarks_write_their_frames_and_nothing_else(ctx):
    labels, frames = S.scene_set()
    full = device_landmarks(ctx, 1, frames, labels)
    part = device_landmarks(ctx, 1, frames, labels, n_frames=len(frames) - 3)      # (checks the sentinels of the three rows behind)
    assert_planes(part, {k: v[:len(frames) - 3] for k, v in full.items()})
    none = device_landmarks(ctx, 1, frames, labels, n_frames=0)                     # n_frames == 0 writes nothing
    assert all(v.shape[0] == 0 for v in none.values())
    single = device_landmarks(ctx, 2, frames, labels, double_lines=False)           # ml_world_d may be NULL
    assert "ml_world_d" not in single
    assert_planes(single, {k: v for k, v in device_landmarks(ctx, 2, frames, labels).items() if k != "ml_world_d"})


def test_landmarks_twice_on_one_stream(ctx):
    labels, frames = S.scene_set()
    a, b = device_landmarks(ctx, 1, frames, labels, 2), device_landmarks(ctx, 1, frames, labels, 2)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("nfeatures", [None, 5000])
def test_full_row_at_the_default_capacity(nfeatures):
    """a context at the default parameters, and one of 5000 key points -- 8192 slots, the 64 KB of keys that need the large-LDS launch --, a frame with
    every feature close: the whole row is sorted, visited and created"""
    c = context(nfeatures)
    try:
        cap, lcap, sf = c.orb_capacity, c.line_capacity, scale_factors(c)
        assert cap >= 1000 and lcap >= 100 and (nfeatures is None or 4096 < cap <= _lib.GRID_MAX_KEYS)
        rng = np.random.default_rng(9)
        z = rng.uniform(0.3, 3.8, cap).astype(F)
        z[::7] = z[3]                                                # ties all over the row
        fr = S.make_frame(6, z, S._ldisp(rng, lcap, lcap), S._held(rng, cap, S.N_MP), None)
        fr.keys["octave"] = rng.integers(0, len(sf), cap)
        got = device_landmarks(c, 1, [fr, fr], ["full", "full"], img_stride=2)
        assert got["n_visited"].tolist() == [[cap, lcap]] * 2
        a = S.batch_arrays([fr, fr], [cap, cap], [lcap, lcap], cap, lcap)
        host = keyframe.CreateNewKeyFrame(a["kps"], a["counts"], a["kls"], a["lcounts"], a["depth"], a["ldisp"], a["Twc"], S.CAM5, S.TH, sf, frame_mp=a["frame_mp"],
                                          frame_ml=a["frame_ml"], mp_nobs=S.MP_NOBS, ml_nobs=S.ML_NOBS)
        assert_planes(got, host)
        assert_planes(got, S.expected([fr, fr], 1, a, S.camera(sf), cap, lcap))
    finally:
        c.close()


def test_oversized_context_is_refused():
    big_p = _lib.default_params()
    big_p.orb.nfeatures = _lib.GRID_MAX_KEYS + 1
    big = _lib.Context(big_p, 640, 480, 1)
    try:
        assert big.orb_capacity > _lib.GRID_MAX_KEYS
        labels, frames = S.scene_set()
        a = S.batch_arrays(frames[:1], [0], [0])
        b = _lib.LandmarksBatchC()
        b.kps, b.counts, b.kls, b.lcounts, b.img_stride = tuple(_lib.ptr(a[k]) for k in ("kps", "counts", "kls", "lcounts")) + (1,)
        b.depth, b.ldisp, b.Twc = _lib.ptr(a["depth"]), _lib.ptr(a["ldisp"]), _lib.ptr(a["Twc"])      # (refused before anything is read)
        outs = {k: np.zeros(8, dt) for k, (_, dt) in keyframe._landmark_shapes(1, 1, 1).items()}
        o = _lib.LandmarksOutputsC()
        for k, v in outs.items():
            setattr(o, k, _lib.ptr(v))
        assert _lib.lib().olf_stereo_landmarks_batch_dev(big.handle, C.byref(b), 1, 1, C.byref(o), None) == OLF_ERR_CAPACITY
        assert "olf_stereo_landmarks_batch_dev" in _lib.last_error()
        ka = S.keyframe_arrays(frames[:1], [S._row()], [None], [None])
        t, to = _lib.KeyFrameTestBatchC(), _lib.KeyFrameTestOutputsC()
        rows = keyframe.keyframe_rows(ka["rows"])
        t.counts, t.lcounts, t.img_stride, t.depth, t.ldisp, t.rows = _lib.ptr(ka["counts"]), _lib.ptr(ka["lcounts"]), 1, _lib.ptr(ka["depth"]), _lib.ptr(ka["ldisp"]), _lib.ptr(rows)
        t.n_ref_matches, t.n_ref_matches_l, t.n_inliers = _lib.ptr(ka["n_ref_matches"]), _lib.ptr(ka["n_ref_matches_l"]), _lib.ptr(ka["n_inliers"])
        for k in _lib.KEYFRAME_TEST_OUTPUTS:
            setattr(to, k, _lib.ptr(outs["status"]))
        assert _lib.lib().olf_need_new_keyframe_batch_dev(big.handle, C.byref(t), 1, C.byref(to), None) == OLF_ERR_CAPACITY
    finally:
        big.close()


def test_host_pointer_forms_on_the_device(ctx):
    """olf_stereo_landmarks_frames and olf_need_new_keyframe_frames: host arrays staged, the same kernels, the outputs back; equal to the host forms"""
    labels, frames = S.scene_set()
    n = len(frames)
    c, lc = S.counts_of(labels, frames)
    a = S.batch_arrays(frames, c, lc, img_stride=2)
    b = _lib.LandmarksBatchC()
    b.kps, b.counts, b.kls, b.lcounts, b.img_stride = tuple(_lib.ptr(a[k]) for k in ("kps", "counts", "kls", "lcounts")) + (2,)
    b.depth, b.ldisp, b.Twc, b.frame_mp, b.frame_ml = (_lib.ptr(a[k]) for k in ("depth", "ldisp", "Twc", "frame_mp", "frame_ml"))
    b.mp_nobs, b.n_mp, b.ml_nobs, b.n_ml = _lib.ptr(S.MP_NOBS), S.N_MP, _lib.ptr(S.ML_NOBS), S.N_ML
    b.fx, b.fy, b.cx, b.cy, b.mbf, b.thDepth = (*S.CAM5, float(S.TH))
    for mode in (1, 2):
        outs = {k: np.full(shape, SENTINEL[np.dtype(dt)], dt) for k, (shape, dt) in keyframe._landmark_shapes(n, S.CAP, S.LCAP).items()}
        o = _lib.LandmarksOutputsC()
        for k, v in outs.items():
            setattr(o, k, _lib.ptr(v))
        _lib.check(_lib.lib().olf_stereo_landmarks_frames(ctx.handle, C.byref(b), n, mode, C.byref(o)), "olf_stereo_landmarks_frames")
        assert_planes(outs, host_landmarks(mode, frames, labels, 2)[0], labels)
    kframes, rows, outlier, outlier_l = S.keyframe_scene()
    n = len(kframes)
    ka = S.keyframe_arrays(kframes, rows, outlier, outlier_l)
    lf = np.arange(n, dtype=np.int32) - 1
    krows = keyframe.keyframe_rows(ka["rows"])
    t, to = _lib.KeyFrameTestBatchC(), _lib.KeyFrameTestOutputsC()
    t.counts, t.lcounts, t.img_stride, t.rows, t.ldisp_frame = _lib.ptr(ka["counts"]), _lib.ptr(ka["lcounts"]), 1, _lib.ptr(krows), _lib.ptr(lf)
    t.depth, t.frame_mp, t.outlier, t.ldisp, t.frame_ml, t.outlier_l = (_lib.ptr(ka[k]) for k in ("depth", "frame_mp", "outlier", "ldisp", "frame_ml", "outlier_l"))
    t.n_ref_matches, t.n_ref_matches_l, t.n_inliers, t.mbf, t.thDepth = _lib.ptr(ka["n_ref_matches"]), _lib.ptr(ka["n_ref_matches_l"]), _lib.ptr(ka["n_inliers"]), S.MBF, float(S.TH)
    kouts = {k: np.full(shape, SENTINEL[np.dtype(dt)], dt) for k, (shape, dt) in keyframe._test_shapes(n).items()}
    for k, v in kouts.items():
        setattr(to, k, _lib.ptr(v))
    _lib.check(_lib.lib().olf_need_new_keyframe_frames(ctx.handle, C.byref(t), n, C.byref(to)), "olf_need_new_keyframe_frames")
    assert_planes(kouts, S.keyframe_expected(kframes, rows, outlier, outlier_l, S.camera(), lf))


# ---- the key-frame test ---------------------------------------------------------------------------------------------------------------------------------------
def device_need(ctx, a, n, lf=None, img_stride=1, bare=False):
    import torch
    out = sentinel_outputs(keyframe._test_shapes(n))
    kw = {} if bare else dict(frame_mp=up(a["frame_mp"]), outlier=up(a["outlier"]), frame_ml=up(a["frame_ml"]), outlier_l=up(a["outlier_l"]))
    res = keyframe.need_new_keyframe_batch(n, up(a["counts"]), up(a["lcounts"]), up(a["depth"]), up(a["ldisp"]), up(keyframe.keyframe_rows(a["rows"])), up(a["n_ref_matches"]),
                                           up(a["n_ref_matches_l"]), up(a["n_inliers"]), S.MBF, S.TH, ldisp_frame=None if lf is None else up(lf), img_stride=img_stride,
                                           out=out, context=ctx, **kw)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert untouched(t[n:]), k
    return {k: t[:n].cpu().numpy() for k, t in res.items()}


@pytest.mark.parametrize("ldisp_frame", ["none", "previous", "shorter"])
def test_need_new_keyframe_against_host_and_reference(ctx, ldisp_frame):
    frames, rows, outlier, outlier_l = S.keyframe_scene()
    n = len(frames)
    lf = None if ldisp_frame == "none" else np.arange(n, dtype=np.int32) - 1
    if ldisp_frame == "shorter":
        short = min(range(n), key=lambda j: frames[j].N_l if frames[j].N_l else 10 ** 6)
        lf = np.where(np.arange(n) % 2, short, np.arange(n)[::-1]).astype(np.int32)
    for img_stride in (1, 2):
        a = S.keyframe_arrays(frames, rows, outlier, outlier_l, img_stride=img_stride)
        got = device_need(ctx, a, n, lf, img_stride)
        host = keyframe.NeedNewKeyFrame(a["counts"], a["lcounts"], a["depth"], a["ldisp"], a["rows"], a["n_ref_matches"], a["n_ref_matches_l"], a["n_inliers"], S.MBF, S.TH,
                                        frame_mp=a["frame_mp"], outlier=a["outlier"], frame_ml=a["frame_ml"], outlier_l=a["outlier_l"], ldisp_frame=lf, img_stride=img_stride)
        assert_planes(got, host)
        assert_planes(got, S.keyframe_expected(frames, rows, outlier, outlier_l, S.camera(), lf))
    assert all(v.shape[0] == 0 for v in device_need(ctx, a, 0, lf, 2).values())      # n_frames == 0 writes nothing
    bare = device_need(ctx, a, n, None, 2, bare=True)
    assert not bare["counts"][:, [0, 2]].any()
    again = device_need(ctx, a, n, lf, 2)
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)


# ---- the chain: UpdateLastFrame's temporal points into SearchByProjection(Frame, Frame) -----------------------------------------------------------------------
def test_temporal_points_feed_search_by_projection(oracle):
    """three extracted stereo frames: `created` as mp_valid and `mp_world` as mp_world, straight from the device, give the matches of the same call with
    planes made by the host form"""
    import torch
    w, h, th = 640, 480, 7.0
    p = oracle.full_params(2000, 500)
    fe = ola.StereoFrontEnd(p, w, h, max_pairs=3)
    imgs = np.zeros((6, h, w), np.uint8)
    imgs[:2] = synth.stereo_batch(41, 1, w, h)
    imgs[2:4], imgs[4:6] = np.roll(imgs[:2], 3, axis=2), np.roll(imgs[:2], 6, axis=2)
    f = fe.frames(imgs)
    fb, n = fe._last_frames("test")
    cap, lcap = fe.ctx.orb_capacity, fe.ctx.line_capacity
    fx, cx, cy, mbf = float(p.stereo.fx), w / 2.0, h / 2.0, float(p.stereo.bf)
    cam5, thd = (fx, fx, cx, cy, mbf), mbf * 35.0 / fx
    eye = np.tile(np.eye(4, dtype=F), (3, 1, 1))
    Tcw = eye.copy()
    Tcw[:, 0, 3] = 0.02
    # every second stereo point already holds a map point with observations: UpdateLastFrame leaves those alone
    nobs = np.array([0, 2], np.int32)
    fmp = np.where(np.arange(cap) % 2, 1, -1).astype(np.int32)[None].repeat(3, 0).copy()
    dev = keyframe.stereo_landmarks_batch(3, keyframe.LANDMARKS_LASTFRAME, fb.kps, fb.counts, fb.kls, fb.lcounts, fb.depth, fb.ldisp, up(eye), cam5, thd, frame_mp=up(fmp),
                                          mp_nobs=up(nobs), n_mp=2, img_stride=2, context=fe.ctx)
    res = fe.search_by_projection_batch(Tcw, dev["mp_world"], cam5, th, mp_valid=dev["created"])
    torch.cuda.synchronize()
    kps = np.zeros((6, cap), _lib.KEYPOINT_DTYPE)
    kls = np.zeros((6, lcap), _lib.KEYLINE_DTYPE)
    counts, lcounts, depth, ldisp = np.zeros(6, np.int32), np.zeros(6, np.int32), np.full((3, cap), -1, F), np.full((3, lcap, 2), -1, F)
    for i in range(3):
        g = f.pair(i)
        nk, nl = len(g["mvKeys"]), len(g["mvKeys_Line"])
        kps[2 * i, :nk], kls[2 * i, :nl], counts[2 * i], lcounts[2 * i] = g["mvKeys"], g["mvKeys_Line"], nk, nl
        depth[i, :nk], ldisp[i, :nl] = g["mvDepth"], g["mvDisparity_l"]
    host = keyframe.UpdateLastFrame(kps, counts, kls, lcounts, depth, ldisp, eye, cam5, thd, scale_factors(fe.ctx), frame_mp=fmp, mp_nobs=nobs, img_stride=2)
    assert host["n_created"][:, 0].min() >= 40 and (host["n_created"][:, 0] < host["n_visited"][:, 0]).all()
    for k in ("n_visited", "n_created", "visit_order", "created_order", "created", "mp_world", "mp_normal", "mp_maxd", "mp_mind", "created_l", "ml_world", "status"):
        assert S.same(dev[k].cpu().numpy(), host[k]), k
    res_h = fe.search_by_projection_batch(Tcw, up(host["mp_world"]), cam5, th, mp_valid=up(host["created"]))
    torch.cuda.synchronize()
    for a, b in zip(res, res_h):
        assert torch.equal(a, b)
    assert int(res[2].min()) >= 1                                    # nmatches of both pairs: temporal points are found again
