"""Optimizer::OptimizeSim3 on the host (no GPU): the conditions every scene of optsim3_scenes must meet for the device tests to mean something, the host
form (olf_optimize_sim3) against the restatement (optsim3_reference) under the tolerance rule, the numeric Jacobian of one edge against the text of
base_binary_edge.hpp bit for bit, known answers, the adaptor on stand-in types and the host source under sanitizers in a program of its own.

The tolerance rule: discrete outputs (the match row, n_inliers, n_correspondences, n_bad_first, status) exactly; real outputs (S12_out and its float
forms, Scw_out, chi2) within 16 x the restatement's spread across its switches, with a floor of 64 float ulp (for the double S12_out too); iters is not
compared."""
import ctypes as C
import math
import os
import subprocess
import numpy as np
import pytest
import optsim3_reference as R
import optsim3_scenes as S
from orb_line_slam_amd import _lib, lib, OptimizeSim3, optimize_sim3_jacobian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLF_ERR_INVALID = -1


def host(s, pair=(0, 1), **kw):
    m = s["matches"].copy()
    args = dict(th2=s["th2"], fix_scale=s["fix_scale"], mp_valid=s["valid"], mp_bad=s["bad"])
    args.update(kw)
    return OptimizeSim3(s["keys"], s["counts"], s["Tcw"], s["world"], s["camera"], s["inv_level_sigma2"], pair, m, s["s12"], s["R12"], s["t12"], **args), m


# ---- (a) the yardstick ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_scene_conditions(name):
    ref = S.reference_of(name)
    base, alts = ref["base"], ref["alts"]
    for a in alts:                                                   # the discrete outputs do not depend on a switch
        assert np.array_equal(a["matches"], base["matches"]), name
        for k in S.DISCRETE:
            assert a[k] == base[k], (name, k)
    assert S.yardstick_is_finite(ref) or name in S.DEGENERATE
    th2 = float(np.float32(S.scene_of(name)["th2"]))
    for k, (chi, idx) in enumerate(base["log"].checks):              # every chi2 of both checks keeps 1000 x its spread from th2
        spread = np.zeros_like(chi)
        for a in alts:
            assert len(a["log"].checks) == len(base["log"].checks) and np.array_equal(a["log"].checks[k][1], idx), (name, k)
            spread = np.maximum(spread, np.abs(a["log"].checks[k][0] - chi))
        need = np.maximum(1000.0 * spread, 4.0 * float(np.finfo(np.float32).eps) * th2)
        assert np.all(np.abs(chi - th2) >= need), (name, k, float(np.min(np.abs(chi - th2) - need)))
    # with every chi2 of the first check decided, nCorrespondences - nBad is decided, and so is its comparison with 10
    assert all(a["n_correspondences"] - a["n_bad_first"] == base["n_correspondences"] - base["n_bad_first"] for a in alts)


def test_scenes_do_what_they_were_built_for():
    b = lambda n: S.reference_of(n)["base"]
    for n in S.COUNTS:
        for kind in ("free", "fixed"):
            r = b("n%d_%s" % (n, kind))
            assert r["n_correspondences"] == n and r["status"] == 0
            assert (r["n_inliers"] == 0 and r["iters"][1] == 0) if n < 10 else r["n_inliers"] > 0
            assert r["S12_out"][7] == float(np.float32(1.3)) if kind == "fixed" else True      # update[6] = 0: the scale never moves
    assert abs(b("n300_free")["S12_out"][7] - 1.3) < 0.05 and b("n300_free")["S12_out"][7] != float(S.scene_of("n300_free")["s12"])
    c = b("clean64")
    assert c["n_bad_first"] == 0 and c["n_inliers"] == 64 and 0 < c["iters"][1] <= 5
    for n in ("out20", "out20_fixed"):
        o = b(n)
        assert o["n_bad_first"] == 20 and o["n_inliers"] == 80 and int((o["matches"] >= 0).sum()) == 80
    o = b("one_side")
    chi = o["log"].checks[0][0]
    gone = (chi > S.TH2).any(axis=1)
    assert o["n_bad_first"] == 16 == int(gone.sum()) and not (chi[gone, 0] > S.TH2).any() and (chi[gone, 1] > S.TH2).all()      # e21 alone exceeds th2
    g, sg = b("gate12"), S.scene_of("gate12")
    assert g["n_correspondences"] == 12 and g["n_bad_first"] == 4 and g["n_inliers"] == 0 and int((g["matches"] >= 0).sum()) == 8
    assert g["S12_out"][7] == float(sg["s12"]) and np.array_equal(g["t12_out"], sg["t12"]) and g["s12_out"] == sg["s12"]
    a = b("all_out")
    assert a["n_bad_first"] == 40 and a["n_inliers"] == 0 and not (a["matches"] >= 0).any()
    k, sk = b("skipped"), S.scene_of("skipped")
    assert k["n_correspondences"] == 36 and k["n_bad_first"] == 0 and np.array_equal(k["matches"], sk["matches"]) and (sk["matches"] == -2).any() and \
        (sk["matches"] >= S.CAP).any()
    assert b("bad_octave")["status"] == 4 and b("bad_octave")["n_correspondences"] == 28
    assert b("depth0")["status"] == 1 and b("depth0")["n_inliers"] == 0


# ---- (b) the host form against the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_host_form_against_the_restatement(name):
    got, m = host(S.scene_of(name))
    S.check_against(got, m, S.reference_of(name), name)


def test_numeric_jacobian_is_the_text_of_base_binary_edge():
    """the column (1 / (2 * 1e-9)) * (e(+1e-9 e_d) - e(-1e-9 e_d)) of one edge, from the text, against the host form's own: bit for bit.  An analytic
    Jacobian differs from it in the seventh digit."""
    s = S.scene_of("n64_free")
    ref = S.reference_of("n64_free")["base"]
    est = ref["S12_out"]
    S12 = (list(est[:4]), list(est[4:7]), float(est[7]))
    i = int(np.nonzero(s["matches"] >= 0)[0][5])
    v = int(s["matches"][i])
    P1, P2 = R.cam_points(s["Tcw"][0], s["world"][0][i:i + 1])[0], R.cam_points(s["Tcw"][1], s["world"][1][v:v + 1])[0]
    obs1, obs2 = [float(s["keys"]["x"][0, i]), float(s["keys"]["y"][0, i])], [float(s["keys"]["x"][1, v]), float(s["keys"]["y"][1, v])]
    for fix in (False, True):
        for inverse, X, obs in ((False, P2, obs1), (True, P1, obs2)):
            want = R.numeric_jacobian_column_text(S12, fix, s["camera"], X, obs, inverse)
            got = optimize_sim3_jacobian(est, s["camera"], X, obs, inverse=inverse, fix_scale=fix)
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (fix, inverse, got - want)
            assert np.all(np.any(got[:, :6] != 0.0, axis=0))
            if fix:
                assert np.all(got[:, 6] == 0.0)
            elif inverse:                                        # (e12 does not see a left-multiplied scale: S12 X2 only grows along its ray)
                assert np.all(got[:, 6] != 0.0)
    # what it is not: the derivative in exact arithmetic.  A central difference over 2e-9 of values near 100 carries an error near 1e-14 / 2e-9
    h = 1e-6
    wide = np.zeros((2, 7))
    for d in range(7):
        u = [0.0] * 7
        u[d] = h
        ep = R.sim3_map(R.oplus(S12, list(u), False), list(P2))
        u[d] = -h
        em = R.sim3_map(R.oplus(S12, list(u), False), list(P2))
        pr = lambda p: np.array([p[0] / p[2] * s["camera"][0] + s["camera"][2], p[1] / p[2] * s["camera"][1] + s["camera"][3]])
        wide[:, d] = -(pr(ep) - pr(em)) / (2 * h)
    got = optimize_sim3_jacobian(est, s["camera"], P2, obs1)
    assert np.max(np.abs(got - wide)) < 1e-3 * np.max(np.abs(wide)) and not np.array_equal(got, wide)


def test_known_answers():
    for fix in (False, True):
        s = S.make_scene(1700 + fix, 64, fix, noise=0.0)              # exact observations
        got, m = host(s)
        s_true, R_true, t_true = s["truth"]
        assert got["n_inliers"] == 64 and got["n_bad_first"] == 0 and np.array_equal(m, s["matches"])
        S.check_against(got, m, S.reference_for(s), "exact %d" % fix)
        if not fix:                                                  # float32 points and key points: the optimum is the true similarity to a few 1e-5
            assert abs(got["S12_out"][7] - s_true) < 2e-4 and np.max(np.abs(got["t12_out"] - t_true)) < 1e-3 and np.max(np.abs(got["R12_out"].reshape(3, 3) - R_true)) < 1e-4
        T2 = s["Tcw"][1].astype(np.float64)
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = got["S12_out"][7] * got["R12_out"].reshape(3, 3).astype(np.float64), got["S12_out"][4:7]
        assert np.max(np.abs(got["Scw_out"].reshape(4, 4) - M @ T2)) < 1e-5      # Scw = S12 * T2w


def test_refused_pairs_and_argument_checks():
    s = S.scene_of("clean64")
    for pair in ((1, 1), (0, 2), (-1, 1)):
        got, m = host(s, pair=pair)
        assert got["n_inliers"] == -1 and got["status"] == 2048 and np.array_equal(m, s["matches"])
    io, tb = _lib.OptSim3IoC(), _lib.TrackBatchC()
    sig, R9, t3 = np.ones(8, np.float32), np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)
    assert lib().olf_optimize_sim3(None, 0, 1, None, _lib.ptr(sig), 8, 0, 1, 1.0, _lib.ptr(R9), _lib.ptr(t3), 10.0, 0, C.byref(io)) == OLF_ERR_INVALID
    assert lib().olf_optimize_sim3(C.byref(tb), 0, 2, None, _lib.ptr(sig), 8, 0, 1, 1.0, _lib.ptr(R9), _lib.ptr(t3), 10.0, 0, C.byref(io)) == OLF_ERR_INVALID      # no outputs
    with pytest.raises(Exception):
        host(s, th2=0.0)
    for name in ("olf_optimize_sim3_pairs_dev", "olf_optimize_sim3", "olf_optimize_sim3_pairs", "olf_debug_optimize_sim3_lds_limit", "olf_debug_optimize_sim3_jacobian"):
        assert hasattr(lib(), name), name
    header = open(os.path.join(ROOT, "include", "orbline.h")).read()
    for name in ("olf_optimize_sim3_pairs_dev", "olf_optimize_sim3_pairs", "olf_optimize_sim3_io", "olf_debug_optimize_sim3_lds_limit"):
        assert name in header
    for doc in ("include/orbline.h", "DESIGN.md", "INTEGRATION.md", "README.md", "SURVEY.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for line in text.splitlines():
            assert not ("OptimizeSim3" in line and "stays on the host" in line), (doc, line[:120])


# ---- (c) the host source under sanitizers, in its own process ---------------------------------------------------------------------------------------------------
def test_host_form_stands_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "optsim3_host_main")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-o", str(tmp_path / "probe"), "-"], input=b"int main() { return 0; }\n",
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if probe.returncode != 0:
        pytest.skip("this g++ has no AddressSanitizer / UBSan runtime: " + probe.stdout.decode()[-300:])
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "optsim3_host_main.cpp"), os.path.join(ROOT, "orb_line_slam_amd", "csrc", "optsim3_host.cpp")], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"OPTSIM3_HOST_OK" in out.stdout, out.stdout.decode()[-3000:]


# ---- (d) the adaptor --------------------------------------------------------------------------------------------------------------------------------------------
def build_adaptor(exe):
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_opt_sim3.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_adaptor_through_the_host_form(tmp_path):
    """ORB_SLAM2::OptimizeSim3 against stand-in types, without a context: the host form; no device is needed"""
    exe = str(tmp_path / "adaptor_opt_sim3")
    build_adaptor(exe)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_OPT_SIM3_OK" in out.stdout, out.stdout.decode()[-3000:]
