"""Optimizer::PoseOptimizationWithLine without a device: the restatement (pose_reference.py) against known motions, the conditions every frame of the
device tests must meet, the host form (olf_pose_optimization_with_line) against the restatement under the tolerance rule, the discard loops against
hand-worked rows, the undefined and edge cases, and both host forms as a stand-alone program under AddressSanitizer / UBSan.

The tolerance rule (pose_scenes.within_rule): a real output may differ from the restatement by 16 times the restatement's own sensitivity -- the largest
difference between its index-order / solve run and its reversed-order and lstsq runs -- with a floor of 64 ulp of the output's largest magnitude."""
import math
import os
import subprocess
import numpy as np
import pytest
import pose_reference as R
import pose_scenes as S
from orb_line_slam_amd import _lib
from orb_line_slam_amd._lib import OLF_ERR_INVALID, OLF_OK, lib
from orb_line_slam_amd.pose import discard_outliers_host, pose_optimization_with_line_host, pose_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [s[0] for s in S.SPECS]


def host(scene, **kw):
    return pose_optimization_with_line_host(*S.call_args(scene), scene["inv_level_sigma2"], Tcw_prev=scene["Tcw_prev"], **kw)


def restate(scene, **kw):
    return R.pose_optimization_with_line(*S.call_args(scene), scene["inv_level_sigma2"], Tcw_prev=scene["Tcw_prev"], **kw)


def same_decisions(a, b):
    return (np.array_equal(a["outlier_out"], b["outlier_out"]) and np.array_equal(a["outlier_l_out"], b["outlier_l_out"]) and
            np.array_equal(a["n_inliers"], b["n_inliers"]) and int(a["good"]) == int(b["good"]) and int(a["status"]) == int(b["status"]))


def is_pass_through(r, scene):
    return (np.array_equal(np.asarray(r["Tcw_out"]), scene["Tcw"]) and np.array_equal(np.asarray(r["DT"]).reshape(4, 4), np.eye(4)) and not np.any(r["DT_cov"]) and
            not np.any(r["DT_cov_eig"]) and r["err_norm"] == -1.0 and int(r["good"]) == 0)


# ---- (a) the restatement itself ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points,n_lines", [(40, 0), (0, 24), (30, 12)])
def test_restatement_recovers_a_noiseless_motion(n_points, n_lines):
    """exact observations (up to the float key points) and the true prior: DT is the truth.  The key points are floats, so an observation is off by up to
    2^-17 of a pixel at 320 pixels and the pose by about that over the focal length: 1e-6 is generous for every entry.  (The flags say nothing here: the
    residuals are rounding noise and removeOutliers cuts at four of its own deviations.)"""
    s = S.make_scene(11, n_points, n_lines, noise=False, true_prior=True)
    r = restate(s)
    assert r["status"] == 0
    assert np.max(np.abs(r["DT"].reshape(4, 4) - s["truth"])) < 1e-6
    assert np.max(np.abs(r["Tcw_out"] - s["Tcw_true"])) < 1e-5


@pytest.mark.parametrize("name", ["p256", "l150", "both_257"])
def test_restatement_lands_near_the_truth(name):
    """half a pixel of noise over some hundred features at f = 250: a few millimetres and hundredths of a degree; the gross outliers are found"""
    s, r = S.scene_of(name), S.reference_of(name)["base"]
    assert r["status"] == 0 and r["good"] == 1
    assert np.max(np.abs(r["DT"].reshape(4, 4) - s["truth"])) < 0.02
    held = int((s["frame_mp"] >= 0).sum() + (s["frame_ml"] >= 0).sum())
    assert 0 < held - int(r["n_inliers"].sum()) < 0.3 * held


def test_every_overlap_branch_is_taken():
    for name in NAMES:
        _, _, _, n_l, _, _ = S.spec(name)
        if n_l >= 63:
            assert S.reference_of(name)["base"]["branches"] == {0, 1, 2}, name


# ---- (b) what a frame of the device tests must satisfy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_scene_conditions(name):
    """the outlier margin is at least 1e-6, no stopping-rule ratio of the last pass lies in [1/4, 4], and the flags are the same under both switches.  For a
    frame that determines a pose the restatement and its sensitivities are finite, so the tolerance rule compares every real output of it."""
    ref = S.reference_of(name)
    b = ref["base"]
    assert S.yardstick_is_finite(ref) or not S.determined(name)
    assert b["outlier_margin"] >= 1e-6
    assert not [r for r in b["stop_ratios"][3] if 0.25 <= r <= 4.0]
    for a in ref["alts"]:
        assert np.array_equal(a["outlier_out"], b["outlier_out"]) and np.array_equal(a["outlier_l_out"], b["outlier_l_out"])


# ---- (c) the host form against the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_form_against_restatement(name):
    """Flags, n_inliers, good and status are equal and the real outputs are within the rule for every frame that determines a pose.  With fewer than six
    features H is singular and what the reference computes depends on the solver's rounding (numpy's solve and lstsq disagree there, too): the flags still
    agree for these frames, and a frame that stops passes its pose through."""
    s, ref = S.scene_of(name), S.reference_of(name)
    h, b = host(s), ref["base"]
    assert np.array_equal(h["outlier_out"], b["outlier_out"]) and np.array_equal(h["outlier_l_out"], b["outlier_l_out"]) and np.array_equal(h["n_inliers"], b["n_inliers"])
    assert not (h["status"] & ~3)
    if h["status"]:
        assert is_pass_through(h, s)
    if not S.determined(name):
        return
    assert same_decisions(h, b)
    for k in S.REAL_OUTPUTS:
        ok, ratio = S.within_rule(k, h[k], ref)
        print(f"{name} {k}: ratio {ratio:.3g} (sensitivity {ref['spread'][k]:.3g})")
        assert ok, (k, ratio)


@pytest.mark.parametrize("params", [dict(has_points=0), dict(has_lines=0), dict(use_motion_model=0), dict(inlier_k=2.5, max_iters_ref=4)])
def test_host_form_parameters(params):
    s, ref = S.scene_of("both_64"), S.reference_of("both_64", **params)
    h = host(s, params=pose_params(**params))
    assert same_decisions(h, ref["base"])
    if "has_points" in params:
        assert not h["outlier_out"].any()                            # Config::hasPoints() gates removeOutliers only: no point flag is ever set
    if "has_lines" in params:
        assert not h["outlier_l_out"].any()
    for k in S.REAL_OUTPUTS:
        ok, ratio = S.within_rule(k, h[k], ref)
        assert ok, (k, ratio)


def test_empty_previous_pose_is_the_pose():
    """mTcw_prev empty: it becomes mTcw (:613-614), bit for bit"""
    s = S.scene_of("both_64")
    a = pose_optimization_with_line_host(*S.call_args(s), s["inv_level_sigma2"], Tcw_prev=None)
    b = pose_optimization_with_line_host(*S.call_args(s), s["inv_level_sigma2"], Tcw_prev=s["Tcw"])
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


# ---- (d) the discard loops ----------------------------------------------------------------------------------------------------------------------------------
#                  held  outlier  obs > 0
ROWS = [(3, 0, 1),      # held, inlier, observed
        (4, 0, 0),      # held, inlier, not observed (a temporal point of UpdateLastFrame)
        (5, 1, 1),      # held, outlier, observed
        (6, 1, 0),      # held, outlier, not observed
        (-1, 0, 0),     # holds nothing
        (-1, 1, 0)]     # holds nothing, a stale flag: no loop looks at it


def _discard(mode, only_tracking, stereo):
    held = [r[0] for r in ROWS]
    out = [r[1] for r in ROWS]
    obs = np.zeros(8, np.uint8)
    for h, _, o in ROWS:
        if h >= 0:
            obs[h] = o
    got = discard_outliers_host(held, held[::-1], out, out[::-1], 8, 8, mode, only_tracking, stereo, obs, obs)
    ref = R.discard_outliers(held, held[::-1], out, out[::-1], mode, only_tracking, stereo, obs, obs)
    for k in ("frame_mp", "frame_ml", "outlier", "outlier_l", "n_matches"):
        assert list(got[k]) == list(ref[k]), k
    assert got["status"] == 0
    return got


def test_discard_mode_0_by_hand():
    """src/Tracking.cc:1034-1074: the two outliers are dropped and their flags cleared; of the two inliers one is observed"""
    g = _discard(0, False, True)
    assert list(g["frame_mp"]) == [3, 4, -1, -1, -1, -1] and list(g["outlier"]) == [0, 0, 0, 0, 0, 1] and list(g["n_matches"]) == [1, 1]
    assert list(g["frame_ml"]) == [-1, -1, -1, -1, 4, 3] and list(g["outlier_l"]) == [1, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("only_tracking,stereo,n,held", [(False, True, 1, [3, 4, -1, -1, -1, -1]), (True, True, 2, [3, 4, -1, -1, -1, -1]),
                                                         (False, False, 1, [3, 4, 5, 6, -1, -1]), (True, False, 2, [3, 4, 5, 6, -1, -1])])
def test_discard_mode_1_by_hand(only_tracking, stereo, n, held):
    """:1547-1590: inliers count when observed, or always with mbOnlyTracking; outliers leave only on a stereo sensor and keep their flags"""
    g = _discard(1, only_tracking, stereo)
    assert list(g["frame_mp"]) == held and list(g["outlier"]) == [0, 0, 1, 1, 0, 1] and list(g["n_matches"]) == [n, n]


def test_discard_index_outside_the_map():
    g = discard_outliers_host([2, 9, -1], [7], [1, 1, 0], [1], 9, 7, 0)
    assert list(g["frame_mp"]) == [-1, 9, -1] and list(g["outlier"]) == [0, 1, 0] and list(g["frame_ml"]) == [7] and g["status"] == 512 | 1024
    assert list(g["n_matches"]) == [0, 0]
    g = discard_outliers_host([2, 4, -1], [], [0, 0, 0], [], 3, 0, 1, mp_index_offset=-2)      # the offset applies before the range test
    assert g["status"] == 0 and list(g["n_matches"]) == [2, 0]


# ---- (e) undefined and edge cases ---------------------------------------------------------------------------------------------------------------------------
def test_no_held_feature():
    s = S.scene_of("p0")
    h = host(s)
    assert h["status"] == 1 and is_pass_through(h, s) and list(h["n_inliers"]) == [0, 0] and list(h["iters"]) == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ["p1", "l1", "l2", "both_tiny"])
def test_one_or_two_features_never_flag(name):
    """one residual: its deviation from the median is 0, so stdv = 0, no residual is below 2 * stdv, k = 0 >= int(0.2 * 1) and the mean is 0 / 0: the
    comparison with a NaN is false and the flag is cleared.  Two residuals d apart: stdv = 1.4826 d and |res - mean| <= d < 4 * stdv."""
    s = S.scene_of(name)
    h = host(s)
    assert not h["outlier_out"].any() and not h["outlier_l_out"].any() and not (h["status"] & ~2)
    assert list(h["n_inliers"]) == [int((s["frame_mp"] >= 0).sum()), int((s["frame_ml"] >= 0).sum())]
    if h["status"]:
        assert is_pass_through(h, s)


def test_five_features_singular_h():
    """H has rank five: the step is whatever the solver makes of it, but the frame ends in a defined state"""
    s = S.scene_of("p5")
    h = host(s)
    assert not (h["status"] & ~2) and np.array_equal(h["outlier_out"], S.reference_of("p5")["base"]["outlier_out"])
    assert is_pass_through(h, s) if h["status"] else np.all(np.isfinite(h["DT"]))


def test_every_feature_becomes_an_outlier():
    """five points that one removeOutliers flags, all of them: the next pass starts without an active feature, the frame stops there with status 1, its flags
    as they stood and its pose unchanged"""
    s, b = S.scene_of("p5_all_outliers"), S.reference_of("p5_all_outliers")["base"]
    h = host(s)
    assert h["status"] == 1 and b["status"] == 1 and h["outlier_out"].all() and list(h["n_inliers"]) == [0, 0] and is_pass_through(h, s)
    assert h["iters"][0] > 0 and h["iters"][3] == 0


def test_entry_flags_and_malformed_input():
    s = S.scene_of("both_64")
    flags = np.zeros(64, np.uint8)
    flags[::5] = 1
    a, b = host(s, outlier=flags), restate(s, outlier=flags)
    assert same_decisions(a, b)
    # an index past the map and an octave past the levels: the feature is left out, the bit is raised, the rest is the frame without it
    bad = dict(s, frame_mp=s["frame_mp"].copy(), keys=s["keys"].copy(), frame_ml=s["frame_ml"].copy())
    bad["frame_mp"][3], bad["frame_ml"][2] = 64, 20
    bad["keys"]["octave"][5] = 8
    a, b = host(bad), restate(bad)
    assert a["status"] == 512 | 1024 | 4 and same_decisions(a, b)
    without = dict(bad, frame_mp=bad["frame_mp"].copy(), frame_ml=bad["frame_ml"].copy())
    without["frame_mp"][[3, 5]], without["frame_ml"][2] = -1, -1
    c = host(without)
    assert c["status"] == 0
    for k in ("Tcw_out", "DT", "DT_cov", "outlier_out", "outlier_l_out", "n_inliers"):
        assert np.array_equal(a[k], c[k]), k


def test_argument_checks():
    b, o, p = _lib.PoseBatchC(), _lib.PoseOutputsC(), pose_params()
    import ctypes as C
    assert lib().olf_pose_optimization_with_line(None, 0, 0, None, 0, C.byref(p), C.byref(o)) == OLF_ERR_INVALID
    assert lib().olf_pose_optimization_with_line(C.byref(b), 0, 0, None, 0, C.byref(p), C.byref(o)) == OLF_ERR_INVALID      # no Tcw, no outputs
    assert lib().olf_discard_outliers(None, 0, 0, 0, 0, 0, None, None) == OLF_ERR_INVALID
    p.max_iters_ref = 0
    s = S.scene_of("p7")
    with pytest.raises(_lib.OlfError):
        host(s, params=p)
    assert OLF_OK == 0


# ---- (f) both host forms under sanitizers, in their own process ---------------------------------------------------------------------------------------------
def test_host_forms_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pose_host_main")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-o", str(tmp_path / "probe"), "-"], input=b"int main() { return 0; }\n",
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if probe.returncode != 0:
        pytest.skip("this g++ has no AddressSanitizer / UBSan runtime: " + probe.stdout.decode()[-300:])
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "pose_host_main.cpp"), os.path.join(ROOT, "orb_line_slam_amd", "csrc", "pose_host.cpp")], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"POSE_HOST_OK" in out.stdout, out.stdout.decode()[-3000:]


# ---- (g) the adaptor ----------------------------------------------------------------------------------------------------------------------------------------
def build_adaptor(exe):
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_pose.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_adaptor_through_the_host_form(tmp_path):
    """ORB_SLAM2::PoseOptimizationWithLine against stand-in types, without a context: the host form; no device is needed"""
    exe = str(tmp_path / "adaptor_pose")
    build_adaptor(exe)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_POSE_OK" in out.stdout, out.stdout.decode()[-3000:]
