"""olf_stereo_landmarks and olf_need_new_keyframe without a device: what the scene builder promises (tests/keyframe_scenes.py), the host forms against the
line-by-line restatement (tests/keyframe_reference.py) on every scene and in every mode -- integers equal, floats and doubles equal as bit patterns --,
the prefix-length identity against the reference's loop, the point geometry against olf_update_normal_and_depth on a one-observation graph, the float
copy of the line endpoints, the argument checks, the exports, the adaptor, and the host source under sanitizers in a process of its own."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import keyframe_reference as R
import keyframe_scenes as S
from orb_line_slam_amd import _lib, keyframe, newpoints
from orb_line_slam_amd._lib import OLF_ERR_INVALID, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
HOST = (keyframe.StereoInitialization, keyframe.CreateNewKeyFrame, keyframe.UpdateLastFrame)      # indexed by the mode


def assert_planes(got, exp, labels=None):
    for k, e in exp.items():
        if k not in got:
            continue
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        g = g.reshape(e.shape)
        if not S.same(g, e):
            bad = np.flatnonzero((S.bits(g) != S.bits(e)).reshape(len(e), -1).any(1))
            raise AssertionError((k, [(int(j), labels[j] if labels else "") for j in bad[:6]], g[bad[0]].reshape(-1)[:12], e[bad[0]].reshape(-1)[:12]))


def host_landmarks(mode, frames, labels, img_stride=1, hold=True, bases=None, sf=S.SF):
    c, lc = S.counts_of(labels, frames)
    a = S.batch_arrays(frames, c, lc, img_stride=img_stride)
    kw = dict(mp_nobs=S.MP_NOBS, ml_nobs=S.ML_NOBS)
    if hold:
        kw.update(frame_mp=a["frame_mp"], frame_ml=a["frame_ml"])
    if bases is not None:
        kw.update(new_base_mp=bases[0], new_base_ml=bases[1])
    got = HOST[mode](a["kps"], a["counts"], a["kls"], a["lcounts"], a["depth"], a["ldisp"], a["Twc"], S.CAM5, S.TH, sf, img_stride=img_stride, **kw)
    exp = S.expected(frames, mode, a, S.camera(sf), new_base_mp=None if bases is None else bases[0], new_base_ml=None if bases is None else bases[1], hold=hold)
    return got, exp


# ---- the scene builder --------------------------------------------------------------------------------------------------------------------------------
def test_scene_conditions():
    labels, frames = S.scene_set()
    K = S.camera()
    a = S.batch_arrays(frames, *S.counts_of(labels, frames))
    e = S.expected(frames, 1, a, K)
    at = lambda s: next(j for j, lab in enumerate(labels) if s in lab)
    # the counts around the thresholds, and what the walk makes of them
    assert [e["n_visited"][at(f"count {n} /"), 0] for n in (0, 1, 100, 101, 102, 255, 256, 257)] == [0, 1, 100, 101, 101, 101, 101, 101]
    assert [e["n_visited"][at(f"lcount {n}"), 1] for n in (0, 1, 50, 51, 52)] == [0, 1, 50, 51, 51]
    assert [e["n_visited"][at(f"nClose {n} /"), 0] for n in (99, 100, 101, 300, 0)] == [101, 101, 102, 300, 101]
    assert [e["n_visited"][at(f"line nClose {n}"), 1] for n in (49, 50, 51, 150, 0)] == [51, 51, 52, 150, 51]
    assert e["n_visited"][at("depth == thDepth"), 0] == 124 and e["n_visited"][at("99 close and one at thDepth"), 0] == 101      # 120 + 3 at the threshold, + 1
    # a block of equal depths straddles the break: the last visited and the first unvisited share a depth
    for lab, h, key in (("ties across the break", 0, "visit_order"), ("line ties across the break", 1, "visit_order_l")):
        j = at(lab)
        fr, n = frames[j], e["n_visited"][j, h]
        zs = fr.depth if h == 0 else np.maximum(F(S.MBF) / fr.ldisp[:, 0], F(S.MBF) / fr.ldisp[:, 1])
        last = e[key][j, n - 1]
        unvisited = np.setdiff1d(np.flatnonzero(zs == zs[last]), e[key][j, :n])
        assert len(unvisited) and unvisited.min() > last and np.sum(zs[e[key][j, :n]] == zs[last]) > 1
    j = at("z = 0, -0")
    assert e["n_visited"][j, 0] == 101 and 7 not in e["visit_order"][j, :101]      # +inf sorts last; 0, -0, negative, NaN and -inf never enter
    ee = S.expected(frames, 0, a, K)
    assert ee["created"][j, [7, 121]].all() and not ee["created"][j, [3, 50, 51, 120, 199]].any()      # INIT mode takes every z > 0, +inf included
    j = at("line disparities")
    assert not e["created_l"][j, [0, 2, 3, 5]].any() and set(e["visit_order_l"][j, :e["n_visited"][j, 1]]) & {1, 4, 6} == set()      # +0 gives +inf: kept, sorted last
    ek = S.expected(frames, 1, a, K, hold=False)
    assert ek["visit_order_l"][j, 0] == 8 and ek["visit_order_l"][j, 1] == 9      # the depths -0 and +0 tie: the index decides
    assert e["status"][at("NaN line depth")] == 1 and e["n_visited"][at("NaN line depth"), 1] == 0 and e["status"][at("NaN start disparity")] == 0
    assert e["status"][at("held entries, some outside")] & 2 and e["status"][at("held lines, some outside")] & 2 and e["status"][at("octave outside")] == 4
    # the line depth comes from either endpoint
    j = at("line nClose 150")
    sz, ez = F(S.MBF) / frames[j].ldisp[:, 0], F(S.MBF) / frames[j].ldisp[:, 1]
    assert (sz > ez).sum() > 20 and (ez > sz).sum() > 20
    # held entries of every kind are visited
    j = at("nClose 300")
    held = np.array(frames[j].mp)
    assert (held < 0).sum() > 20 and ((held >= 0) & (S.MP_NOBS[np.maximum(held, 0)] == 0)).sum() > 20 and ((held >= 0) & (S.MP_NOBS[np.maximum(held, 0)] >= 1)).sum() > 20
    assert 0 < e["n_created"][j, 0] < 300
    # no stereo point: UpdateLastFrame returns before its lines, CreateNewKeyFrame does not
    j = at("no stereo point")
    assert e["n_visited"][j].tolist() == [0, 51] and S.expected(frames, 2, a, K)["n_visited"][j].tolist() == [0, 0]


def test_keyframe_scene_conditions():
    frames, rows, outlier, outlier_l = S.keyframe_scene()
    e = S.keyframe_expected(frames, rows, outlier, outlier_l, S.camera())
    cond = e["conditions"].tolist()
    assert cond[:13] == [0, 1, 2, 4, 8, 16, 32, 62, 61, 59, 55, 47, 31]      # every condition true alone, then false alone
    k = 13
    assert cond[k:k + 4] == [1, 1, 17, 17] and [r["nKFs"] for r in rows[k:k + 4]] == [0, 1, 2, 3]      # 50 < 100 * 0.4f fails below two key frames
    assert cond[k + 4:k + 7] == [17, 1, 1 + 32]                     # 39 < 40.0f holds, 40 fails; the line twin
    k = 20
    assert cond[k:k + 4] == [16, 4 + 16, 1, 1 + 16]                  # c1c: 25 < 25.0 fails, 24 holds; c2: 75 < 75.0f fails, 74 holds
    assert cond[k + 4] & 4                                           # 16777216 < 67108865 * 0.25 holds in double; in float both sides are 16777216
    assert cond[k + 5] == 1 and cond[k + 7] == 1                     # 25165824 < 33554433 * 0.75f fails in float; in double the product is 25165824.75
    assert np.float64(25165824) < np.float64(33554433) * 0.75 and not F(16777216) < F(67108865) * F(0.25)
    k = 28
    assert e["need"][k:k + 2].tolist() == [1, 0] and e["interrupt_ba"][k:k + 3].tolist() == [1, 1, 1] and e["need"][k + 2] == 0      # queue 2, queue 3, monocular
    assert cond[k + 5:k + 8] == [0, 0, 0] and e["need"][k + 5:k + 8].tolist() == [0, 0, 0] and e["need"][k + 8] == 1      # the early returns; nKFs == mMaxFrames passes
    assert cond[k + 9] & 1 and cond[k + 10] & 3 == 2 and cond[k + 11] & 3 == 0 and e["need"][k + 12] == 1      # unsigned sums wrap at 32 bits
    assert cond[-2] == 60 and e["counts"][-2, 0] < 100 and e["counts"][-2, 1] > 70 and e["counts"][-2, 2] < 20 and e["counts"][-2, 3] > 100      # bNeedToInsertClose twice


# ---- the host forms against the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("img_stride, hold, with_bases", [(1, True, False), (2, True, True), (1, False, False)])
def test_host_landmarks_against_reference(mode, img_stride, hold, with_bases):
    labels, frames = S.scene_set()
    n = len(frames)
    bases = (np.arange(n, dtype=np.int32) * 1000 + 7, np.arange(n, dtype=np.int32) * 300 - 5) if with_bases else None
    got, exp = host_landmarks(mode, frames, labels, img_stride, hold, bases)
    assert_planes(got, exp, labels)
    assert S.same(got["ml_world"], got["ml_world_d"].astype(F))      # Converter::toCvMat of the doubles
    assert (got["visit_order"] >= 0).sum(1).tolist() == got["n_visited"][:, 0].tolist() and (got["created_order_l"] >= 0).sum(1).tolist() == got["n_created"][:, 1].tolist()


def test_host_landmarks_at_a_full_default_row():
    """2032 key points and 512 key lines, every feature close: the whole row is sorted and visited"""
    rng = np.random.default_rng(3)
    fr = S.make_frame(5, rng.uniform(0.3, 3.8, 2032).astype(F), S._ldisp(rng, 512, 512), S._held(rng, 2032, S.N_MP), None)
    a = S.batch_arrays([fr], [2032], [512], cap=2032, lcap=512)
    got = keyframe.CreateNewKeyFrame(a["kps"], a["counts"], a["kls"], a["lcounts"], a["depth"], a["ldisp"], a["Twc"], S.CAM5, S.TH, S.SF, frame_mp=a["frame_mp"],
                                     frame_ml=a["frame_ml"], mp_nobs=S.MP_NOBS, ml_nobs=S.ML_NOBS)
    assert got["n_visited"].tolist() == [[2032, 512]]
    assert_planes(got, S.expected([fr], 1, a, S.camera(), cap=2032, lcap=512))


def test_prefix_length_identity():
    """the visited prefix as the library forms it -- from two counts -- against the reference's loop with its break, over random rows"""
    rng = np.random.default_rng(11)
    frames, want = [], []
    for k in range(60):
        n, nl = int(rng.integers(0, 400)), int(rng.integers(0, 200))
        n_close, nl_close = int(rng.integers(0, n + 1)) if k % 3 else min(n, int(rng.integers(95, 106))), int(rng.integers(0, nl + 1)) if k % 3 else min(nl, int(rng.integers(45, 56)))
        fr = S.make_frame(300 + k, S._depths(rng, n, n_close), S._ldisp(rng, nl, nl_close))
        frames.append(fr)
        lz = np.maximum(F(S.MBF) / fr.ldisp[:, 0], F(S.MBF) / fr.ldisp[:, 1])
        want.append([R.visited_by_loop(sorted(fr.depth), S.TH, 100), R.visited_by_loop(sorted(lz), S.TH, 50)])
    a = S.batch_arrays(frames, [fr.N for fr in frames], [fr.N_l for fr in frames])
    for mode in (1, 2):
        got = HOST[mode](a["kps"], a["counts"], a["kls"], a["lcounts"], a["depth"], a["ldisp"], a["Twc"], S.CAM5, S.TH, S.SF)
        assert got["n_visited"].tolist() == want
    # and the formula itself, restated here, on rows of every small shape
    for _ in range(3000):
        n, least = int(rng.integers(0, 12)), int(rng.integers(0, 6))
        zs = sorted(rng.integers(0, 8, n).astype(F))
        n_close = int(np.sum(~(np.array(zs, F) > F(3.5))))
        assert R.visited_by_loop(zs, F(3.5), least) == min(n, max(n_close, least) + 1)


@pytest.mark.parametrize("mode", [0, 1])
def test_point_geometry_equals_update_normal_and_depth(mode):
    """INIT and KEYFRAME mode: normal, maxd and mind equal olf_update_normal_and_depth on a one-observation graph built from the same arrays; LASTFRAME mode
    (the constructor) differs from them in the sign of a zero only"""
    from orb_line_slam_amd import CullView, MapGraph
    labels, frames = S.scene_set()
    got, _ = host_landmarks(mode, frames, labels)
    last, _ = host_landmarks(2, frames, labels)
    checked = 0
    for j, fr in enumerate(frames):
        idx = got["created_order"][j, :got["n_created"][j, 0]]
        idx = idx[(fr.keys["octave"][idx] >= 0) & (fr.keys["octave"][idx] < 8)]
        if not len(idx):
            continue
        n = len(idx)
        g = MapGraph(mp_obs=[[0]] * n, mp_bad=[0] * n, kf_bad=[0], kf_mp=[[-1] * n], kf_covis=[[]], kf_children=[[]], kf_parent=[-1])
        v = CullView(g, mp_obs_slot=[[k] for k in range(n)], mp_nobs=[1] * n, kf_slot_octave=[list(fr.keys["octave"][idx])], kf_slot_depth=np.zeros((1, n)),
                     kf_slot_stereo=np.zeros((1, n)), kf_th_depth=np.zeros(1), kf_mode=np.zeros(1))
        normal, maxd, mind, status = newpoints.UpdateNormalAndDepth(g, v, got["mp_world"][j, idx], np.zeros(n, np.int32), fr.Twc[:3, 3].reshape(1, 3), S.SF)
        assert status == 0 and S.same(normal, got["mp_normal"][j, idx]) and S.same(maxd, got["mp_maxd"][j, idx]) and S.same(mind, got["mp_mind"][j, idx])
        checked += n
    assert checked > 1500
    if mode == 1:
        both = (got["created"] == 1) & (last["created"] == 1)
        a, b = got["mp_normal"][both], last["mp_normal"][both]
        assert np.array_equal(a, b) and S.same(got["mp_maxd"][both], last["mp_maxd"][both])      # equal as values: -0 == +0
        # the one bit pattern: a component that underflows to -0 in `x / norm` stays -0 in the constructor and becomes +0 in `zeros + x`.  Every input
        # is a normal float: Pos - Ow = (-7e-28, 2.3e27, 1e10), the reciprocal norm is 4e-28, their product is below the smallest denormal.
        fr = S.make_frame(1, [1e10], np.zeros((0, 2)))
        fr.keys["x"], fr.keys["y"], fr.keys["octave"] = np.nextafter(F(S.CX), F(0)), F(1e20), 2
        fr.Twc = np.eye(4, dtype=F)
        fr.Twc[0, 0] = 1e-30
        arr = S.batch_arrays([fr], [1], [0])
        res = [HOST[m](arr["kps"], arr["counts"], arr["kls"], arr["lcounts"], arr["depth"], arr["ldisp"], arr["Twc"], S.CAM5, S.TH, S.SF)["mp_normal"][0, 0] for m in (1, 2)]
        assert S.bits(res[1])[0] == 0x80000000 and S.bits(res[0])[0] == 0 and np.array_equal(res[0], res[1])
        assert_planes(dict(mp_normal=np.stack(res)), dict(mp_normal=np.stack([S.expected([fr], m, arr, S.camera())["mp_normal"][0, 0] for m in (1, 2)])))


@pytest.mark.parametrize("ldisp_frame", ["none", "previous", "shorter"])
def test_host_need_new_keyframe_against_reference(ldisp_frame):
    frames, rows, outlier, outlier_l = S.keyframe_scene()
    n = len(frames)
    lf = None if ldisp_frame == "none" else np.arange(n, dtype=np.int32) - 1
    if ldisp_frame == "shorter":
        short = min(range(n), key=lambda j: frames[j].N_l if frames[j].N_l else 10 ** 6)
        lf = np.where(np.arange(n) % 2, short, np.arange(n)[::-1]).astype(np.int32)
    for img_stride in (1, 2):
        a = S.keyframe_arrays(frames, rows, outlier, outlier_l, img_stride=img_stride)
        got = keyframe.NeedNewKeyFrame(a["counts"], a["lcounts"], a["depth"], a["ldisp"], a["rows"], a["n_ref_matches"], a["n_ref_matches_l"], a["n_inliers"], S.MBF, S.TH,
                                       frame_mp=a["frame_mp"], outlier=a["outlier"], frame_ml=a["frame_ml"], outlier_l=a["outlier_l"], ldisp_frame=lf, img_stride=img_stride)
        exp = S.keyframe_expected(frames, rows, outlier, outlier_l, S.camera(), lf)
        assert_planes(got, exp)
    assert (exp["status"] != 0).any() == (ldisp_frame != "none")
    # without the optional planes: nothing is held, nothing is an outlier
    bare = keyframe.NeedNewKeyFrame(a["counts"], a["lcounts"], a["depth"], a["ldisp"], a["rows"], a["n_ref_matches"], a["n_ref_matches_l"], a["n_inliers"], S.MBF, S.TH,
                                    img_stride=2)
    assert not bare["counts"][:, [0, 2]].any() and (bare["counts"][:, 1] >= got["counts"][:, 1]).all()


# ---- arguments and exports ---------------------------------------------------------------------------------------------------------------------------------
def test_exports():
    import orb_line_slam_amd as ola
    for name in ("stereo_landmarks_batch", "need_new_keyframe_batch", "StereoInitialization", "CreateNewKeyFrame", "UpdateLastFrame", "NeedNewKeyFrame"):
        assert name in ola.__all__ and callable(getattr(ola, name)), name
    for name in ("olf_stereo_landmarks_batch_dev", "olf_stereo_landmarks", "olf_stereo_landmarks_frames", "olf_need_new_keyframe_batch_dev", "olf_need_new_keyframe",
                 "olf_need_new_keyframe_frames"):
        assert hasattr(lib(), name), name
    header = open(os.path.join(ROOT, "include", "orbline.h")).read()
    for name in ("olf_stereo_landmarks_batch_dev", "olf_need_new_keyframe_batch_dev", "OLF_LANDMARKS_LASTFRAME", "src/Tracking.cc:639-677", ":1092-1204", ":1606-1725",
                 ":1744-1865"):
        assert name in header, name
    makefile = open(os.path.join(ROOT, "orb_line_slam_amd", "csrc", "Makefile")).read()
    assert "keyframe_api.cpp" in makefile and "keyframe_host.cpp" in makefile
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "olf_stereo_landmarks_batch_dev" in open(os.path.join(ROOT, doc)).read(), doc


FAKE_CTX = C.c_void_p(1 << 20)                                       # not a context: a call that got past its argument checks would read it


def test_argument_errors():
    L = lib()
    labels, frames = S.scene_set()
    a = S.batch_arrays(frames[:2], [frames[0].N, frames[1].N], [frames[0].N_l, frames[1].N_l])
    b = _lib.LandmarksBatchC()
    b.kps, b.counts, b.kls, b.lcounts, b.img_stride = _lib.ptr(a["kps"]), _lib.ptr(a["counts"]), _lib.ptr(a["kls"]), _lib.ptr(a["lcounts"]), 1
    b.depth, b.ldisp, b.Twc = _lib.ptr(a["depth"]), _lib.ptr(a["ldisp"]), _lib.ptr(a["Twc"])
    b.fx, b.fy, b.cx, b.cy, b.mbf, b.thDepth = (*S.CAM5, float(S.TH))
    outs = {k: np.zeros(shape, dt) for k, (shape, dt) in keyframe._landmark_shapes(2, S.CAP, S.LCAP).items()}
    o = _lib.LandmarksOutputsC()
    for k, v in outs.items():
        setattr(o, k, _lib.ptr(v))
    host = lambda bb=b, oo=o, n=2, mode=1, sf=_lib.ptr(S.SF), nl=8, cap=S.CAP: L.olf_stereo_landmarks(C.byref(bb) if bb else None, cap, S.LCAP, n, mode, sf, nl,
                                                                                                   C.byref(oo) if oo else None)
    assert host() == 0
    assert host(bb=None) == OLF_ERR_INVALID and host(oo=None) == OLF_ERR_INVALID and host(n=-1) == OLF_ERR_INVALID and host(mode=3) == OLF_ERR_INVALID
    assert host(mode=-1) == OLF_ERR_INVALID and host(sf=None) == OLF_ERR_INVALID and host(nl=0) == OLF_ERR_INVALID and host(nl=17) == OLF_ERR_INVALID
    assert "olf_stereo_landmarks" in _lib.last_error()
    assert host(cap=8193, n=0) == _lib.OLF_ERR_CAPACITY
    before = {k: v.copy() for k, v in outs.items()}
    assert host(n=0) == 0 and all(np.array_equal(outs[k], before[k]) for k in outs)      # n_frames == 0 writes nothing
    for field in ("kps", "counts", "kls", "lcounts", "depth", "ldisp", "Twc"):
        bad = _lib.LandmarksBatchC.from_buffer_copy(b)
        setattr(bad, field, None)
        assert host(bb=bad) == OLF_ERR_INVALID, field
        assert L.olf_stereo_landmarks_batch_dev(FAKE_CTX, C.byref(bad), 2, 1, C.byref(o), None) == OLF_ERR_INVALID, field
    for field in _lib.LANDMARKS_OUTPUTS:
        bad = _lib.LandmarksOutputsC.from_buffer_copy(o)
        setattr(bad, field, None)
        assert host(oo=bad) == (0 if field == "ml_world_d" else OLF_ERR_INVALID), field
    bad = _lib.LandmarksBatchC.from_buffer_copy(b)
    bad.img_stride = 0
    assert host(bb=bad) == OLF_ERR_INVALID
    bad = _lib.LandmarksBatchC.from_buffer_copy(b)
    bad.frame_mp, bad.n_mp = _lib.ptr(a["frame_mp"]), 5              # held entries and a map, but no observation counts
    assert host(bb=bad) == OLF_ERR_INVALID
    assert L.olf_stereo_landmarks_batch_dev(None, C.byref(b), 2, 1, C.byref(o), None) == OLF_ERR_INVALID
    assert L.olf_stereo_landmarks_batch_dev(FAKE_CTX, C.byref(b), 2, 7, C.byref(o), None) == OLF_ERR_INVALID and "olf_stereo_landmarks_batch_dev" in _lib.last_error()
    assert L.olf_stereo_landmarks_frames(FAKE_CTX, C.byref(b), -1, 1, C.byref(o)) == OLF_ERR_INVALID
    # the key-frame test
    t, to = _lib.KeyFrameTestBatchC(), _lib.KeyFrameTestOutputsC()
    assert L.olf_need_new_keyframe(C.byref(t), S.CAP, S.LCAP, 1, C.byref(to)) == OLF_ERR_INVALID and "olf_need_new_keyframe" in _lib.last_error()
    assert L.olf_need_new_keyframe(None, S.CAP, S.LCAP, 0, C.byref(to)) == OLF_ERR_INVALID
    assert L.olf_need_new_keyframe_batch_dev(FAKE_CTX, C.byref(t), 1, C.byref(to), None) == OLF_ERR_INVALID and "olf_need_new_keyframe_batch_dev" in _lib.last_error()
    assert L.olf_need_new_keyframe_frames(FAKE_CTX, C.byref(t), 1, C.byref(to)) == OLF_ERR_INVALID
    with pytest.raises(ValueError):
        keyframe.NeedNewKeyFrame([1], [1], np.zeros((1, 4)), np.zeros((1, 4, 2)), [[0] * 10], [0], [0], [[0, 0]], 1.0, 1.0)      # a row of ten scalars
    with pytest.raises(ValueError):
        keyframe.CreateNewKeyFrame(np.zeros((1, 4), _lib.KEYPOINT_DTYPE), [1], np.zeros((1, 3), _lib.KEYLINE_DTYPE), [1], np.zeros((1, 4)), np.zeros((1, 2, 2)), np.eye(4), S.CAM5,
                                   S.TH, S.SF)


# ---- the adaptor and the stand-alone build ----------------------------------------------------------------------------------------------------------------
def test_adaptor_through_the_host_forms(tmp_path):
    """ORB_SLAM2::CreateNewKeyFrameLandmarks, UpdateLastFrameLandmarks, StereoInitializationLandmarks and NeedNewKeyFrame against stand-in types, without a context"""
    exe = str(tmp_path / "adaptor_keyframe")
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_keyframe.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_KEYFRAME_OK" in out.stdout, out.stdout.decode()[-3000:]


def test_host_form_stands_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "keyframe_host_main")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-o", str(tmp_path / "probe"), "-"], input=b"int main() { return 0; }\n",
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if probe.returncode != 0:
        pytest.skip("this g++ has no AddressSanitizer / UBSan runtime: " + probe.stdout.decode()[-300:])
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")                  # (the shared terms include the HIP runtime's header for its types; nothing of it is linked)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include"), "-o", exe, os.path.join(ROOT, "tests", "keyframe_host_main.cpp"),
                    os.path.join(ROOT, "orb_line_slam_amd", "csrc", "keyframe_host.cpp")], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"KEYFRAME_HOST_OK" in out.stdout, out.stdout.decode()[-3000:]
