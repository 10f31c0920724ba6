"""olf_pose_optimization_with_line_batch_dev and olf_discard_outliers_batch_dev on the device, against the host form and the restatement
(pose_reference.py) over the frames of pose_scenes.SPECS: held points 0, 1, 5, 6, 7, 63, 64, 65, 255, 256, 257 and the capacity, held lines 0, 1, 2, 63,
64, 65 and the line capacity, each kind alone and both together.  tests/test_pose_cpu.py has verified for every one of these frames that its outlier
margin is at least 1e-6, that no stopping rule of the last pass is near its threshold and that the restatement's flags do not depend on its switches.

Every output is allocated SLACK elements longer than the batch needs and filled with a sentinel: nothing may be written past a count, a row or the batch.
The tolerance rule for the real outputs is pose_scenes.within_rule; flags, n_inliers, good and status are compared exactly; iters is not compared."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import pose_reference as R
import pose_scenes as S
from status_text import STATUS_TEXT
from orb_line_slam_amd import _lib, matcher, pose
from orb_line_slam_amd._lib import KEYLINE_DTYPE, KEYPOINT_DTYPE, OLF_ERR_CAPACITY, OLF_ERR_INVALID, OlfError, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 37
SENT = {np.float32: 777.0, np.float64: 777.0, np.uint8: 0xAB, np.int32: -777}
NAMES = [s[0] for s in S.SPECS]
ROWS = dict(Tcw_out=16, DT=16, DT_cov=36, DT_cov_eig=6, err_norm=1, good=1, n_inliers=2, iters=4, status=1)


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    p = _lib.default_params()
    p.orb.nfeatures = 300
    p.line.lsd_nfeatures = S.LINE_CAP
    c = _lib.Context(p, S.W, S.H, 2)
    assert c.orb_capacity == S.CAP and c.line_capacity == S.LINE_CAP and c.nlevels == S.N_LEVELS
    sig = np.zeros(c.nlevels, np.float32)
    _lib.check(lib().olf_orb_scale_tables(c.handle, None, None, None, _lib.ptr(sig), None), "olf_orb_scale_tables")
    assert np.array_equal(sig, S.level_tables()[1])                  # the scenes' level table is the context's
    yield c
    c.close()


def host_of(name, **kw):
    s = S.scene_of(name)
    return pose.pose_optimization_with_line_host(*S.call_args(s), s["inv_level_sigma2"], Tcw_prev=s["Tcw_prev"], **kw)


def run_batch(ctx, names, img_stride=1, params=None, prev="scene", offsets=False, entry_flags=None, alias=False, scenes=None):
    """the frames `names` (or the scene dicts `scenes`) as one batch on the device; returns the outputs as host arrays, one row per frame, after checking that
    every sentinel behind the batch is intact.  offsets: frame_mp / frame_ml hold each frame's own indices and mp_index_offset / ml_index_offset place them in
    the joint map.  entry_flags: {frame: (outlier, outlier_l)}; alias: the flag outputs are the inputs."""
    import torch
    scenes = scenes if scenes is not None else [S.scene_of(n) for n in names]
    n, cap, lcap = len(scenes), ctx.orb_capacity, ctx.line_capacity
    m = max(n, 1)                                                    # (an empty batch still passes addresses)
    kps, kls = np.zeros((m * img_stride, cap), KEYPOINT_DTYPE), np.zeros((m * img_stride, lcap), KEYLINE_DTYPE)
    counts, lcounts = np.full(m * img_stride, 5, np.int32), np.full(m * img_stride, 5, np.int32)         # (the images between the frames are not read)
    lle, Tcw, Tprev = np.zeros((m, lcap, 3)), np.zeros((m, 16), np.float32), np.zeros((m, 16), np.float32)
    fmp, fml = np.full((m, cap), -1, np.int32), np.full((m, lcap), -1, np.int32)
    flags, lflags = np.zeros((n, cap), np.uint8), np.zeros((n, lcap), np.uint8)
    offs, offl, worlds, lworlds = np.zeros(m, np.int32), np.zeros(m, np.int32), [np.zeros((1, 3), np.float32)], [np.zeros((1, 6), np.float32)]
    base, lbase = 1, 1
    for j, s in enumerate(scenes):
        N, NL = len(s["keys"]), len(s["keylines"])
        kps[j * img_stride, :N], kls[j * img_stride, :NL], counts[j * img_stride], lcounts[j * img_stride] = s["keys"], s["keylines"], N, NL
        lle[j, :NL], Tcw[j], Tprev[j] = s["lle"], s["Tcw"], s["Tcw"] if prev == "Tcw" else s["Tcw_prev"]
        held, lheld = s["frame_mp"] >= 0, s["frame_ml"] >= 0
        fmp[j, :N], fml[j, :NL] = s["frame_mp"], s["frame_ml"]
        if offsets:
            offs[j], offl[j] = base, lbase
        else:
            fmp[j, :N][held] += base
            fml[j, :NL][lheld] += lbase
        worlds.append(s["mp_world"].reshape(-1, 3))
        lworlds.append(s["ml_world"].reshape(-1, 6))
        base, lbase = base + len(s["mp_world"]), lbase + len(s["ml_world"])
        if entry_flags and j in entry_flags:
            flags[j, :N], lflags[j, :NL] = entry_flags[j]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    raw = lambda a: dev(a.view(np.uint8).reshape(-1))
    out = {k: torch.full((n * r + SLACK,), SENT[t], dtype=pose._torch_dtype(t), device="cuda") for (k, t, _), r in ((o, ROWS[o[0]]) for o in pose.OUTPUTS)}
    d_flags, d_lflags = dev(np.concatenate([flags.reshape(-1), np.full(SLACK, 0xAB, np.uint8)])), dev(np.concatenate([lflags.reshape(-1), np.full(SLACK, 0xAB, np.uint8)]))
    out["outlier_out"] = d_flags if alias else torch.full((n * cap + SLACK,), 0xAB, dtype=torch.uint8, device="cuda")
    out["outlier_l_out"] = d_lflags if alias else torch.full((n * lcap + SLACK,), 0xAB, dtype=torch.uint8, device="cuda")
    pose.pose_optimization_with_line_batch(raw(kps), dev(counts), raw(kls), dev(lcounts), img_stride, dev(lle), dev(Tcw), S.CAMERA, dev(fmp), dev(np.concatenate(worlds)),
                                           dev(fml), dev(np.concatenate(lworlds)), n_frames=n, Tcw_prev=None if prev is None else dev(Tprev),
                                           mp_index_offset=dev(offs) if offsets else None, ml_index_offset=dev(offl) if offsets else None,
                                           outlier=d_flags if entry_flags or alias else None, outlier_l=d_lflags if entry_flags or alias else None, params=params, out=out,
                                           context=ctx)
    torch.cuda.synchronize()
    res = {}
    for k, v in out.items():
        a = v.cpu().numpy()
        r = ROWS.get(k, cap if k == "outlier_out" else lcap)
        assert np.all(a[n * r:] == a[-1]) and a[-1] == (0xAB if a.dtype == np.uint8 else SENT[a.dtype.type]), k      # nothing behind the batch
        res[k] = a[:n * r].reshape(n, r)
    for j, s in enumerate(scenes):                                   # every flag row is complete: 0 from the count on
        assert not res["outlier_out"][j, len(s["keys"]):].any() and not res["outlier_l_out"][j, len(s["keylines"]):].any()
    return res


def frame_of(res, j, scene):
    f = {k: res[k][j] for k in res}
    f["outlier_out"], f["outlier_l_out"] = res["outlier_out"][j, :len(scene["keys"])], res["outlier_l_out"][j, :len(scene["keylines"])]
    for k in ("err_norm", "good", "status"):
        f[k] = f[k][0]
    return f


def same_bits(a, b):
    return all(np.array_equal(np.atleast_1d(a[k]).view(np.uint8), np.atleast_1d(b[k]).view(np.uint8)) for k in a if k != "iters") and np.array_equal(a["iters"], b["iters"])


def check_frame(got, name, host, ref, ratios=None):
    """one frame of the device against the host form and the restatement"""
    s, b = S.scene_of(name), ref["base"]
    for other in (host, b):
        assert np.array_equal(got["outlier_out"], other["outlier_out"]) and np.array_equal(got["outlier_l_out"], other["outlier_l_out"]), name
        assert np.array_equal(got["n_inliers"], other["n_inliers"]), name
    assert int(got["status"]) == int(host["status"]) and int(got["good"]) == int(host["good"]), name
    if got["status"]:
        assert np.array_equal(got["Tcw_out"], s["Tcw"]) and np.array_equal(got["DT"].reshape(4, 4), np.eye(4)) and not got["DT_cov"].any() and got["err_norm"] == -1.0
    if not S.determined(name):
        return          # (H is singular: what the restatement computes depends on its solver, test_pose_cpu.test_host_form_against_restatement)
    assert int(got["status"]) == int(b["status"]) and int(got["good"]) == int(b["good"]), name
    for k in S.REAL_OUTPUTS:
        ok, ratio = S.within_rule(k, got[k], ref)
        if ratios is not None:
            ratios[k] = max(ratios.get(k, 0.0), ratio)
        assert ok, (name, k, ratio, ref["spread"][k])


def check_scene(got, scene, ratios=None, **kw):
    """one frame of the device, given as a scene dict, against the host form and the restatement on the same inputs: decisions equal, real outputs within the
    tolerance rule (the restatement's sensitivity is computed for these very inputs).  kw: outlier / outlier_l on entry."""
    ref = S.reference_for(scene, **kw)
    h = pose.pose_optimization_with_line_host(*S.call_args(scene), scene["inv_level_sigma2"], Tcw_prev=scene["Tcw_prev"], **kw)
    b = ref["base"]                                                  # the conditions a frame must meet (test_pose_cpu.test_scene_conditions), for these inputs
    assert S.yardstick_is_finite(ref) and b["outlier_margin"] >= 1e-6 and not [r for r in b["stop_ratios"][3] if 0.25 <= r <= 4.0]
    assert all(np.array_equal(a["outlier_out"], b["outlier_out"]) and np.array_equal(a["outlier_l_out"], b["outlier_l_out"]) for a in ref["alts"])
    for other in (h, b):
        assert np.array_equal(got["outlier_out"], other["outlier_out"]) and np.array_equal(got["outlier_l_out"], other["outlier_l_out"])
        assert int(got["status"]) == int(other["status"]) and int(got["good"]) == int(other["good"]) and np.array_equal(got["n_inliers"], other["n_inliers"])
    for k in S.REAL_OUTPUTS:
        for what, value in (("device", got[k]), ("host form", h[k])):
            ok, ratio = S.within_rule(k, value, ref)
            assert ok, (what, k, ratio, ref["spread"][k])
            if ratios is not None and what == "device":
                ratios[k] = max(ratios.get(k, 0.0), ratio)
    return h


@pytest.fixture(scope="module")
def all_frames(ctx):
    """every frame of SPECS in one batch, the run the other tests compare bits with"""
    res = run_batch(ctx, NAMES)
    ctx.poll_status()
    return {name: frame_of(res, j, S.scene_of(name)) for j, name in enumerate(NAMES)}


def test_every_size_against_host_form_and_restatement(all_frames):
    ratios = {}
    for name in NAMES:
        check_frame(all_frames[name], name, host_of(name), S.reference_of(name), ratios)
    print("largest ratio difference / sensitivity per output (the rule allows 16):", {k: float("%.3g" % v) for k, v in ratios.items()})


@pytest.mark.parametrize("n_frames,img_stride", [(1, 1), (2, 2), (7, 1), (65, 1)])
def test_batch_sizes_and_positions(ctx, all_frames, n_frames, img_stride):
    """batches of mixed sizes; the frame both_257 at the first, a middle and the last position: a frame's outputs are the same bits wherever it stands"""
    names = [NAMES[(3 * j + n_frames) % len(NAMES)] for j in range(n_frames)]
    for pos in {0, n_frames // 2, n_frames - 1}:
        names[pos] = "both_257"
    res = run_batch(ctx, names, img_stride=img_stride)
    for j, name in enumerate(names):
        assert same_bits(frame_of(res, j, S.scene_of(name)), all_frames[name]), (j, name)
    ctx.poll_status()


def test_feature_kinds_by_parameter(ctx):
    """has_points = 0 / has_lines = 0 on a frame that holds both (as in the reference they gate removeOutliers only), and use_motion_model = 0"""
    for params in (dict(has_points=0), dict(has_lines=0), dict(use_motion_model=0)):
        res = run_batch(ctx, ["both_64", "both_gaps"], params=pose.pose_params(**params))
        for j, name in enumerate(["both_64", "both_gaps"]):
            got, ref = frame_of(res, j, S.scene_of(name)), S.reference_of(name, **params)
            check_frame(got, name, host_of(name, params=pose.pose_params(**params)), ref)
            assert "has_points" not in params or not got["outlier_out"].any()
            assert "has_lines" not in params or not got["outlier_l_out"].any()


def test_empty_previous_pose(ctx):
    """Tcw_prev NULL against Tcw_prev = Tcw: equal bits"""
    names = ["both_64", "p7", "l63"]
    a, b = run_batch(ctx, names, prev=None), run_batch(ctx, names, prev="Tcw")
    for j, name in enumerate(names):
        assert same_bits(frame_of(a, j, S.scene_of(name)), frame_of(b, j, S.scene_of(name)))
        s = S.scene_of(name)
        h = pose.pose_optimization_with_line_host(*S.call_args(s), s["inv_level_sigma2"], Tcw_prev=None)
        got = frame_of(a, j, s)
        assert np.array_equal(got["outlier_out"], h["outlier_out"]) and np.array_equal(got["outlier_l_out"], h["outlier_l_out"]) and got["status"] == h["status"]


def test_index_offsets(ctx, all_frames):
    """the frames' own indices with mp_index_offset / ml_index_offset against indices into the joint map: equal bits"""
    names = ["both_gaps", "p65", "l2", "both_full"]
    res = run_batch(ctx, names, offsets=True)
    for j, name in enumerate(names):
        assert same_bits(frame_of(res, j, S.scene_of(name)), all_frames[name]), name
    ctx.poll_status()


def test_entry_flags_given_and_aliased(ctx):
    names = ["both_64", "p255"]
    flags = {}
    for j, name in enumerate(names):
        s = S.scene_of(name)
        o, ol = np.zeros(len(s["keys"]), np.uint8), np.zeros(len(s["keylines"]), np.uint8)
        o[::5], ol[1::4] = 1, 1
        flags[j] = (o, ol)
    a, b = run_batch(ctx, names, entry_flags=flags), run_batch(ctx, names, entry_flags=flags, alias=True)
    for j, name in enumerate(names):
        s = S.scene_of(name)
        got = frame_of(a, j, s)
        assert same_bits(got, frame_of(b, j, s))
        check_scene(got, s, outlier=flags[j][0], outlier_l=flags[j][1])


def _expect_bits(ctx, bits):
    with pytest.raises(OlfError) as e:
        ctx.poll_status()
    assert e.value.code == OLF_ERR_CAPACITY and "flags=%d " % bits in str(e.value) and all(STATUS_TEXT[b] in str(e.value) for b in (512, 1024) if bits & b), str(e.value)
    ctx.poll_status()


def test_malformed_indices_and_octaves(ctx, all_frames):
    """an index past the map raises exactly bit 512 / 1024 of the context and the feature is left out; an octave past the levels sets bit 4 of the frame's
    own word.  Either way the frame is the frame without that feature, bit for bit; its neighbour in the batch is untouched."""
    s = S.scene_of("both_64")
    for what, bits, fstatus in (("point", 512, 0), ("line", 1024, 0), ("octave", 0, 4)):
        bad = dict(s, frame_mp=s["frame_mp"].copy(), frame_ml=s["frame_ml"].copy(), keys=s["keys"].copy(), keylines=s["keylines"].copy())
        without = dict(bad, frame_mp=s["frame_mp"].copy(), frame_ml=s["frame_ml"].copy())
        if what == "point":
            bad["frame_mp"][3] = 1 << 20
            without["frame_mp"][3] = -1
        elif what == "line":
            bad["frame_ml"][2] = 1 << 20
            without["frame_ml"][2] = -1
        else:
            bad["keys"]["octave"][5], bad["keylines"]["octave"][1] = S.N_LEVELS, -1
            without["frame_mp"][5], without["frame_ml"][1] = -1, -1
        res = run_batch(ctx, None, scenes=[bad, S.scene_of("p7")])
        if bits:
            _expect_bits(ctx, bits)
        else:
            ctx.poll_status()
        ref = run_batch(ctx, None, scenes=[without, S.scene_of("p7")])
        ctx.poll_status()
        got, want = frame_of(res, 0, bad), frame_of(ref, 0, without)
        assert got["status"] == fstatus and want["status"] == 0
        got["status"] = want["status"]
        assert same_bits(got, want), what
        assert same_bits(frame_of(res, 1, S.scene_of("p7")), all_frames["p7"])


def test_arguments(ctx):
    import torch
    b, o, p = _lib.PoseBatchC(), _lib.PoseOutputsC(), pose.pose_params()
    assert lib().olf_pose_optimization_with_line_batch_dev(ctx.handle, C.byref(b), 1, C.byref(p), C.byref(o), None) == OLF_ERR_INVALID
    assert lib().olf_pose_optimization_with_line_batch_dev(None, C.byref(b), 0, C.byref(p), C.byref(o), None) == OLF_ERR_INVALID
    assert lib().olf_discard_outliers_batch_dev(ctx.handle, None, 1, 0, 0, 0, None, None) == OLF_ERR_INVALID
    res = run_batch(ctx, [])                                         # n_frames == 0 writes nothing (run_batch checks the sentinels)
    assert all(v.size == 0 for v in res.values())
    torch.cuda.synchronize()
    ctx.poll_status()


# ---- the discard loops ------------------------------------------------------------------------------------------------------------------------------------
def _discard_rows(seed, n, n_map):
    rng = np.random.RandomState(seed)
    held = np.where(rng.uniform(size=n) < 0.7, rng.randint(0, n_map, n), -1).astype(np.int32)
    return held, (rng.uniform(size=n) < 0.4).astype(np.uint8)


@pytest.mark.parametrize("mode,only_tracking,stereo", [(0, 0, 1), (1, 0, 1), (1, 1, 1), (1, 0, 0)])
def test_discard_outliers_row_lengths(ctx, mode, only_tracking, stereo):
    """exact in both modes at the row lengths 0, 1, 63, 64, 65 and the capacities, against the restatement and the host form"""
    import torch
    cap, lcap, n_mp, n_ml = ctx.orb_capacity, ctx.line_capacity, 500, 90
    lengths = [(0, 0), (1, 1), (63, 63), (64, 64), (65, 65), (cap, lcap), (cap + 9, lcap + 9)]      # (a count beyond the capacity is read as the capacity)
    n = len(lengths)
    rng = np.random.RandomState(5)
    obs, lobs = (rng.uniform(size=n_mp) < 0.6).astype(np.uint8), (rng.uniform(size=n_ml) < 0.6).astype(np.uint8)
    fmp, fml = np.full((n, cap), -7, np.int32), np.full((n, lcap), -7, np.int32)
    fo, fl = np.full((n, cap), 1, np.uint8), np.full((n, lcap), 1, np.uint8)
    want = []
    for j, (a, b) in enumerate(lengths):
        a_, b_ = min(a, cap), min(b, lcap)
        (fmp[j, :a_], fo[j, :a_]), (fml[j, :b_], fl[j, :b_]) = _discard_rows(10 + j, a_, n_mp), _discard_rows(20 + j, b_, n_ml)
        want.append(R.discard_outliers(fmp[j, :a_], fml[j, :b_], fo[j, :a_], fl[j, :b_], mode, only_tracking, stereo, obs, lobs))
        h = pose.discard_outliers_host(fmp[j, :a_], fml[j, :b_], fo[j, :a_], fl[j, :b_], n_mp, n_ml, mode, only_tracking, stereo, obs, lobs)
        for k in ("frame_mp", "frame_ml", "outlier", "outlier_l", "n_matches"):
            assert list(h[k]) == list(want[-1][k]), (j, k)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [dev(fmp), dev(fml), dev(fo), dev(fl)]
    out = torch.full((2 * n + SLACK,), -777, dtype=torch.int32, device="cuda")
    pose.discard_outliers_batch(dev(np.array([l[0] for l in lengths], np.int32)), dev(np.array([l[1] for l in lengths], np.int32)), 1, d[0], d[1], d[2], d[3], n_mp, n_ml, mode,
                                only_tracking, stereo, dev(obs), dev(lobs), out=out, context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()
    got, nm = [x.cpu().numpy() for x in d], out.cpu().numpy()
    assert np.all(nm[2 * n:] == -777)
    for j, (a, b) in enumerate(lengths):
        a_, b_ = min(a, cap), min(b, lcap)
        assert list(got[0][j, :a_]) == want[j]["frame_mp"] and list(got[1][j, :b_]) == want[j]["frame_ml"], j
        assert list(got[2][j, :a_]) == want[j]["outlier"] and list(got[3][j, :b_]) == want[j]["outlier_l"], j
        assert np.all(got[0][j, a_:] == -7) and np.all(got[1][j, b_:] == -7) and np.all(got[2][j, a_:] == 1) and np.all(got[3][j, b_:] == 1), j      # the row's rest is untouched
        assert list(nm[2 * j:2 * j + 2]) == want[j]["n_matches"], j


def test_discard_chained_after_the_pose_call(ctx):
    """the rows the optimiser wrote go into the loops as they are: mode 0 leaves exactly the inliers held, and counts them"""
    import torch
    s = S.scene_of("both_gaps")
    r = pose.PoseOptimizationWithLine(*S.call_args(s), Tcw_prev=s["Tcw_prev"], context=ctx)
    g = pose.DiscardOutliers(s["frame_mp"], s["frame_ml"], r["outlier_out"], r["outlier_l_out"], len(s["mp_world"]), len(s["ml_world"]), 0, context=ctx)
    ctx.synchronize()
    assert list(g["n_matches"]) == list(r["n_inliers"]) and not g["outlier"].any() and not g["outlier_l"].any()
    assert np.array_equal(g["frame_mp"] >= 0, (s["frame_mp"] >= 0) & (r["outlier_out"] == 0)) and np.array_equal(g["frame_ml"] >= 0, (s["frame_ml"] >= 0) & (r["outlier_l_out"] == 0))
    with pytest.raises(ValueError):
        pose.DiscardOutliers(np.zeros(ctx.orb_capacity + 1), [], np.zeros(ctx.orb_capacity + 1), [], 1, 0, 0, context=ctx)
    torch.cuda.synchronize()


# ---- the reference-side adaptor and the host-pointer forms on the device ------------------------------------------------------------------------------------
def test_adaptor_on_the_device(tmp_path):
    from test_pose_cpu import build_adaptor
    exe = str(tmp_path / "adaptor_pose")
    build_adaptor(exe)
    out = subprocess.run([exe, "device"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_POSE_OK" in out.stdout, out.stdout.decode()[-3000:]


def test_numpy_form_is_the_batch_of_one(ctx, all_frames):
    """PoseOptimizationWithLine (numpy in and out, on the device) gives the bits the frame has in a batch"""
    for name in ("both_gaps", "p5_all_outliers"):
        s = S.scene_of(name)
        r = pose.PoseOptimizationWithLine(*S.call_args(s), Tcw_prev=s["Tcw_prev"], context=ctx)
        ctx.synchronize()
        got = dict(r, good=np.uint8(r["good"]), status=np.int32(r["status"]), err_norm=np.float64(r["err_norm"]))
        assert same_bits({k: got[k] for k in all_frames[name]}, all_frames[name]), name


def test_fed_from_the_frame_to_frame_search(ctx):
    """the index convention of the frame-to-frame search: the matches of olf_search_by_projection_batch_dev -- indices into the LAST frame's features -- go in
    as they are, with mp_world the batch's per-frame world planes viewed flat and mp_index_offset[j] = j * capacity for pair j's last frame; the result is
    the host form's and the restatement's on the same matches resolved by hand.  (The chain is a short one of the search's own test generator: three motions, no lines.)"""
    import torch
    import test_track_batch_gpu as TB
    frames = TB.make_chain(11, [TB.pose(tx=0.05), TB.pose(tz=-0.5), TB.pose(ry_deg=2.0)], n=120, n_dis=20)
    assert max(len(f.keys) for f in frames) <= ctx.orb_capacity
    b = TB.DeviceBatch(ctx, frames)
    matches, _, nmatches = b.search(7.0)
    n, cap, lcap = len(frames) - 1, ctx.orb_capacity, ctx.line_capacity
    assert int(nmatches.min()) >= 20
    i32, u8 = torch.int32, torch.uint8
    zl = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    offs = (torch.arange(n, dtype=i32, device="cuda") * cap).contiguous()
    prior = b.Tcw[:-1].reshape(n, 16).contiguous()                    # the last frame's pose as the prior, and as the previous pose
    out = pose.pose_optimization_with_line_batch(b.kps[1:], b.counts[1:], zl((n, lcap, 68), u8), zl((n,), i32), 1, zl((n, lcap, 3), torch.float64), prior, TB.CAM[:4], matches,
                                                 b.world.reshape(-1, 3), torch.full((n, lcap), -1, dtype=i32, device="cuda"), None, n_frames=n, Tcw_prev=prior,
                                                 mp_index_offset=offs, context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    m, world = matches.cpu().numpy(), b.world.cpu().numpy()
    sig = S.level_tables()[1]
    for j in range(n):
        cur, N = frames[j + 1], len(frames[j + 1].keys)
        scene = dict(keys=cur.keys, keylines=np.zeros(0, KEYLINE_DTYPE), lle=np.zeros((0, 3)), Tcw=frames[j].Tcw.reshape(16), Tcw_prev=frames[j].Tcw.reshape(16),
                     camera=TB.CAM[:4], frame_mp=m[j, :N], mp_world=world[j], frame_ml=np.zeros(0, np.int32), ml_world=np.zeros((0, 6), np.float32), inv_level_sigma2=sig)
        g = {k: got[k][j] for k in got}
        g.update(outlier_out=got["outlier_out"][j, :N], outlier_l_out=got["outlier_l_out"][j, :0], err_norm=got["err_norm"][j], good=got["good"][j], status=got["status"][j])
        h = check_scene(g, scene)
        assert h["status"] == 0 and h["n_inliers"][0] >= 20
        # the jitter of the chain is 2 pixels at f = 200 and depths up to 20 m: the pose comes within a few centimetres of the truth
        assert np.max(np.abs(got["Tcw_out"][j].reshape(4, 4)[:3, 3] - cur.Tcw[:3, 3])) < 0.1


def test_fed_from_the_frame_to_frame_line_tracking(ctx):
    """the index convention of the frame-to-frame line tracking: olf_track_lines_batch_dev hands the current frame's lines the IDS its caller gave the last
    frame's lines (d_last_ml), not indices into the last frame.  With map indices as ids its d_cur_ml goes in as frame_ml as it is, ml_index_offset NULL,
    against ml_world of the map -- unlike the points' matches, which are last-frame indices and need the offset.
    A synthetic pair: the last frame sees 60 map lines exactly under the previous pose (plus ten lines of nothing, in shuffled order, a sixth of its ids
    NULL), the current frame is a frame of pose_scenes over the same map lines, its descriptors four bits off the last frame's."""
    import torch
    import line_scenes as ls
    rng = np.random.RandomState(9)
    s = S.make_scene(611, 0, 60, outliers=True, extra_lines=12)
    NL, n_ml, lcap, cap = len(s["keylines"]), len(s["ml_world"]), ctx.line_capacity, ctx.orb_capacity
    Tp = s["Tcw_prev"].reshape(4, 4).astype(np.float64)
    with_angle = lambda k: ls.keylines(k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"])
    cur = with_angle(s["keylines"])
    cur["octave"] = s["keylines"]["octave"]
    ends = np.array([S._project(Tp, w[:3].astype(np.float64)) + S._project(Tp, w[3:].astype(np.float64)) for w in s["ml_world"]])
    extra = rng.uniform(30, 200, (10, 4))
    order = rng.permutation(n_ml + 10)
    last = with_angle(dict(zip(("startPointX", "startPointY", "endPointX", "endPointY"), np.concatenate([ends, extra])[order].T)))
    ids = np.concatenate([np.arange(n_ml), np.full(10, -1)])[order].astype(np.int32)
    ids[(rng.uniform(size=len(ids)) < 1 / 6)] = -1
    map_desc = rng.randint(0, 256, (n_ml + 10, 32)).astype(np.uint8)
    cur_desc = rng.randint(0, 256, (NL, 32)).astype(np.uint8)
    held = s["frame_ml"] >= 0
    cur_desc[held] = ls.flip(np.random.default_rng(3), map_desc[s["frame_ml"][held]], 4)
    kls, ldesc = np.zeros((2, lcap), KEYLINE_DTYPE), np.zeros((2, lcap, 32), np.uint8)
    kls[0, :len(last)], kls[1, :NL], ldesc[0, :len(last)], ldesc[1, :NL] = last, cur, map_desc[order], cur_desc
    last_ml = np.full((1, lcap), -1, np.int32)
    last_ml[0, :len(ids)] = ids
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_kls, d_lcounts = dev(kls.view(np.uint8).reshape(2, lcap, 68)), dev(np.array([len(last), NL], np.int32))
    _, cur_ml, ninl = matcher.track_lines_batch(2, d_kls, dev(ldesc), d_lcounts, dev(np.full((2, lcap, 2), 5.0, np.float32)), dev(last_ml), ls.BOUNDS, ls.NNR, img_stride=1,
                                                context=ctx, **ls.F2F_MODES["motion_model"])
    lle = np.zeros((1, lcap, 3))
    lle[0, :NL] = s["lle"]
    out = pose.pose_optimization_with_line_batch(torch.zeros((1, cap, 28), dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), d_kls[1:],
                                                 d_lcounts[1:], 1, dev(lle), dev(s["Tcw"][None]), S.CAMERA, torch.full((1, cap), -1, dtype=torch.int32, device="cuda"), None,
                                                 cur_ml, dev(s["ml_world"]), n_frames=1, Tcw_prev=dev(s["Tcw_prev"][None]), context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()
    fed = cur_ml.cpu().numpy()[0, :NL]
    assert int(ninl[0]) == int((fed >= 0).sum()) >= 30 and np.all(cur_ml.cpu().numpy()[0, NL:] == -1)
    assert np.array_equal(fed[fed >= 0], s["frame_ml"][fed >= 0])          # the ids are the map indices of the lines the current frame really observes
    got = {k: v.cpu().numpy()[0] for k, v in out.items()}
    got.update(outlier_out=got["outlier_out"][:0], outlier_l_out=got["outlier_l_out"][:NL], err_norm=got["err_norm"][()], good=got["good"][()], status=got["status"][()])
    h = check_scene(got, dict(s, keys=np.zeros(0, KEYPOINT_DTYPE), frame_mp=np.zeros(0, np.int32), keylines=cur, frame_ml=fed))
    assert h["status"] == 0 and h["n_inliers"][1] >= 25
    assert np.max(np.abs(got["DT"].reshape(4, 4) - s["truth"])) < 0.05


def test_state_beyond_the_lds(all_frames):
    """a context whose per-frame state (26 bytes a point, 50 a line, 16 a key) does not fit in LDS keeps it in the batch scratch slot: the same code on
    another pointer, and -- the lanes' assignment does not depend on the capacity -- the same bits"""
    p = _lib.default_params()
    p.orb.nfeatures = 6000
    p.line.lsd_nfeatures = S.LINE_CAP
    big = _lib.Context(p, S.W, S.H, 2)
    try:
        assert 26 * big.orb_capacity + 50 * big.line_capacity + 16 * max(big.orb_capacity, big.line_capacity) > 160 * 1024
        names = ["both_257", "p7", "l63", "both_full", "p0"]
        res = run_batch(big, names)
        big.poll_status()
        for j, name in enumerate(names):
            assert same_bits(frame_of(res, j, S.scene_of(name)), all_frames[name]), name
    finally:
        big.close()
