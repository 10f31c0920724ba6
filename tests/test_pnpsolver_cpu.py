"""olf_pnp_solver, the host form of PnPsolver's RANSAC, against the numpy restatement (tests/pnpsolver_reference.py) over the scenes of
tests/pnpsolver_scenes.py, whose builder asserts from the restatement alone that what the trajectory depends on is settled: the correspondences, the
effective min_inliers, the iteration cap, the trajectory (accepted, no_more, iterations_done, best and returned counts), the flags outside the near set and
the counts at settled iterations are exact; the returned and the best Tcw meet the project's tolerance rule -- 16 x the restatement's spread under its
switches, with a floor of 64 float ulp of the largest element.  Largest ratio measured: 0.0 of 1 under both parameter sets (every returned and
best pose equals the restatement's bit for bit; the blocked sums of Refine round to the same float32 here).  Then windows with carried state (the OR of the loop condition included), a resumed call after an acceptance,
the error returns, the exports, the adaptor against mock types and the stand-alone sanitizer program."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import pnpsolver_reference as R
import pnpsolver_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, pnpsolver

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_KEYS = tuple(k for k, _, _ in pnpsolver._STATE)
SENTINEL = -7


def prm(alt):
    return (S.ALT, S.ALT_TH2) if alt else (S.PARAMS, S.TH2)


def ransac(alt=False, n_iterations=0, **kw):
    p, th2 = prm(alt)
    args = dict(p, th2=th2, n_iterations=n_iterations)
    args.update(kw)
    return pnpsolver.pnp_ransac(**args)


def fresh_state(n_pairs, cap, max_iterations):
    """a new solver per pair; counts, the inlier rows and the returned pose start as sentinels"""
    st = pnpsolver.pnp_state(n_pairs, cap, max_iterations, device=False)
    st["counts"][:] = SENTINEL
    st["inliers"][:] = 99
    st["Tcw"][:] = 5.0
    return st


def host_call(sc, st, rn, pairs=None, rows=None, arrays=None, img_stride=1, sf=S.SF, valid=True, bad=True, only=None):
    """one olf_pnp_solver call per listed pair on its row of st; returns the status bits ORed"""
    kps, counts, world, v, b = arrays or sc.arrays
    pairs, rows = (sc.pairs if pairs is None else pairs), (sc.rows if rows is None else rows)
    bits = 0
    for p, pair in enumerate(pairs):
        if only is not None and p not in only:
            continue
        bits |= pnpsolver.PnPSolve(kps, counts, world, S.CAM, sf, pair, rows[p], sc.draws[p][:rn.max_iterations], st, rn, row=p,
                                   mp_valid=v if valid else None, mp_bad=b if bad else None, img_stride=img_stride)
    return bits


def _bits(v):
    """float32 as its bits; a NaN as one pattern (IEEE 754 leaves a NaN's sign and payload open)"""
    v = np.ascontiguousarray(v, F)
    return np.where(np.isnan(v), np.uint32(0x7fc00000), v.view(np.uint32))


def same_state(a, b, keys=STATE_KEYS):
    for k in keys:
        x, y = (_bits(v) if v.dtype == np.float32 else np.asarray(v) for v in (a[k], b[k]))
        assert np.array_equal(x, y), (k, np.argwhere(x != y)[:6])


@pytest.fixture(scope="module", params=[False, True], ids=["tracker", "alt"])
def solved(request):
    alt = request.param
    sc, an = S.scene_set(), S.analyse(alt)
    rn = ransac(alt)
    st = fresh_state(len(sc.pairs), sc.cap, rn.max_iterations)
    assert host_call(sc, st, rn) == 0
    return alt, sc, an, st


def test_builder_conditions():
    an = S.analyse(False)
    assert [a.C.N for a in an] == [0, 3, 4, 9, 10, 11, 19, 20, 21, 22, 63, 64, 65, 300, S.CAP, 41, 40, 30]
    assert [a.out.min_eff for a in an[4:10]] == [10, 10, 10, 10, 10, 11]                         # 10 up to N = 21, 11 at N = 22
    assert all(a.out.no_more and not a.out.accepted for a in an[:4])
    a = an[4]                                                        # N == minimum: one iteration, Refine fails on the strict >, the best comes back at the cap
    assert (a.out.cap, a.st.iterations_done, a.out.accepted, a.out.refined, a.out.no_more, a.out.n_inliers) == (1, 1, 1, False, 1, 10)
    assert a.log[0][4][0] == 10
    a = an[5]                                                        # accepted on the first record
    assert a.out.refined and a.st.iterations_done == min(j for j in a.log if a.log[j][0] >= a.out.min_eff) + 1
    a = an[15]                                                       # Refine rejects the record of 20, the record of 21 is accepted
    assert a.log[0][0] == 20 and a.log[0][4][0] == 20 and a.out.min_eff == 20 and a.out.refined and a.out.n_inliers == 21 and a.st.iterations_done == 4
    a = an[16]                                                       # the cap with nothing
    assert not a.out.accepted and a.out.no_more and a.st.best_inliers == 0 and a.st.iterations_done == a.out.cap == 35
    assert all(not a.out.degenerate for a in an)
    alt = S.analyse(True)
    assert sum(a.out.refined for a in alt) >= 10


def test_discrete_results_equal_the_restatement(solved):
    alt, sc, an, st = solved
    mi = prm(alt)[0]["max_iterations"]
    for p, a in enumerate(an):
        assert st["n_correspondences"][p] == a.C.N
        assert (st["accepted"][p], st["no_more"][p], st["n_inliers"][p]) == (a.out.accepted, a.out.no_more, a.out.n_inliers), p
        Nf = a.C.Nf
        assert (st["inliers"][p, Nf:] == 99).all()
        if a.C.N < a.out.min_eff:
            assert st["iterations_done"][p] == 0 and st["best_inliers"][p] == 0 and not st["best_Tcw"][p].any() and not st["inliers"][p, :Nf].any()
            continue
        assert (st["iterations_done"][p], st["best_inliers"][p]) == (a.st.iterations_done, a.st.best_inliers), p
        flags = np.zeros(Nf, np.uint8)
        flags[a.C.feat] = a.out.inliers
        assert np.array_equal(st["inliers"][p, :Nf], flags), p      # (the builder asserted that the returned sets hold no near correspondence)
        if a.st.best_flags is not None:
            bf = np.zeros(Nf, np.uint8)
            bf[a.C.feat] = a.st.best_flags
            assert np.array_equal(st["best_flags"][p, :Nf], bf), p
        for j in a.settled:
            assert st["counts"][p, j] == a.log[j][0], (p, j)
        assert (st["counts"][p, st["iterations_done"][p]:] == SENTINEL).all()
        if not a.out.accepted:
            assert (st["Tcw"][p] == 5.0).all()


def test_parameters_table():
    got_m, got_c = C.c_int32(0), C.c_int32(0)
    for kw in (S.PARAMS, S.ALT, dict(S.PARAMS, max_iterations=300), dict(S.PARAMS, epsilon=1.0), dict(S.PARAMS, epsilon=1e-4, min_inliers=1),
               dict(S.PARAMS, probability=0.5, max_iterations=5), dict(S.PARAMS, epsilon=1e-12, min_inliers=4)):
        rn = pnpsolver.pnp_ransac(**kw)
        for N in list(range(0, 600)) + [2000, 4096, 8192]:
            assert _lib.lib().olf_debug_pnp_solver_parameters(N, C.byref(rn), C.addressof(got_m), C.addressof(got_c)) == 0
            assert (got_m.value, got_c.value) == R.parameters(N, **kw), (N, kw)
    assert R.parameters(21, **dict(S.PARAMS, max_iterations=300)) == (10, 35) and R.parameters(22, **S.PARAMS)[0] == 11 and R.parameters(10, **S.PARAMS) == (10, 1)


def test_poses_meet_the_tolerance_rule(solved):
    alt, sc, an, st = solved
    worst = 0.0
    for p, a in enumerate(an):
        for key, base, alts in (("Tcw", a.out.Tcw, [o.Tcw for o, _ in a.alts]), ("best_Tcw", a.st.best_Tcw, [s.best_Tcw for _, s in a.alts])):
            if base is None:
                continue
            base = np.asarray(base, np.float64).reshape(-1)
            got = np.asarray(st[key][p], np.float64).reshape(-1)
            spread = np.max([np.abs(np.asarray(x, np.float64).reshape(-1) - base) for x in alts], axis=0)
            floor = 64 * np.spacing(F(np.abs(base).max()))
            worst = max(worst, float(np.max(np.abs(got - base) / np.maximum(16 * spread, floor))))
    print("largest ratio of the tolerance rule (1 = the bound), host form against base:", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("window", [1, 5, 300])
def test_windows_follow_the_loop_condition(solved, window):
    """a call runs until the cap is reached AND `window` iterations of its own are done (:182 is an OR): against the restatement's literal loop, and
    against find() where the cap is at least the window"""
    alt, sc, an, st = solved
    p_, th2 = prm(alt)
    mi = p_["max_iterations"]
    rn = ransac(alt, n_iterations=window)
    w = fresh_state(len(sc.pairs), sc.cap, mi)
    assert host_call(sc, w, rn) == 0
    for p, a in enumerate(an):
        s2 = R.new_state()
        o = R.iterate(a.C, sc.draws[p][:mi], s2, window, S.CAM, **p_)
        assert (w["accepted"][p], w["no_more"][p], w["n_inliers"][p], w["iterations_done"][p], w["best_inliers"][p]) == \
               (o.accepted, o.no_more, o.n_inliers, s2.iterations_done, s2.best_inliers), p
        if a.C.N >= a.out.min_eff and (a.out.refined or a.out.cap >= min(window, mi)):
            same_state({k: v[p:p + 1] for k, v in w.items()}, {k: v[p:p + 1] for k, v in st.items()})
        elif a.C.N >= a.out.min_eff:
            assert w["iterations_done"][p] == min(window, mi) > a.out.cap          # beyond the cap


def test_resumed_after_an_acceptance_and_beyond_the_cap(solved):
    """Tracking.cc:2312: the pose optimisation rejects, the solver is iterated again with its state carried -- it accepts again at the first later iteration
    with n >= min_inliers, by the carried outcome of Refine; once the cap is behind it, a window call still runs its n_iterations"""
    alt, sc, an, st = solved
    p_, th2 = prm(alt)
    mi = p_["max_iterations"]
    rn = ransac(alt, n_iterations=5)
    kps, counts, world, v, b = sc.arrays
    for p in (11, 13, 15):
        a = an[p]
        s2 = R.new_state()
        w = {k: val[p:p + 1].copy() for k, val in fresh_state(len(sc.pairs), sc.cap, mi).items()}
        seen = []
        for call in range(4):
            log = {}
            o = R.iterate(a.C, sc.draws[p][:mi], s2, 5, S.CAM, log=log, **p_)
            pnpsolver.PnPSolve(kps, counts, world, S.CAM, S.SF, sc.pairs[p], sc.rows[p], sc.draws[p][:mi], w, rn, row=0, mp_valid=v, mp_bad=b)
            assert (w["accepted"][0], w["no_more"][0], w["n_inliers"][0], w["iterations_done"][0], w["best_inliers"][0]) == \
                   (o.accepted, o.no_more, o.n_inliers, s2.iterations_done, s2.best_inliers), (p, call)
            seen.append((o.accepted, o.refined, s2.iterations_done))
        assert seen[0][1] and seen[1][1] and seen[1][2] > seen[0][2], (p, seen)      # accepted, and accepted again later


def test_octave_out_of_range_and_malformed_pairs():
    sc = S.scene_set()
    kps, counts, world, v, b = (a.copy() for a in sc.arrays)
    p = 11
    kps[sc.pairs[p][1], 5]["octave"] = 8
    rn = ransac()
    st = fresh_state(1, sc.cap, rn.max_iterations)
    bits = pnpsolver.PnPSolve(kps, counts, world, S.CAM, S.SF, sc.pairs[p], sc.rows[p], sc.draws[p][:rn.max_iterations], st, rn, mp_valid=v, mp_bad=b)
    assert bits == 256 and st["n_correspondences"][0] == 63
    C_ = R.correspondences(kps, counts, world, v, b, S.SF, S.TH2, sc.pairs[p], sc.rows[p])
    assert C_.status == 256 and C_.N == 63
    for pair in ((0, 0), (-1, 1), (0, len(sc.frames))):
        st = fresh_state(1, sc.cap, rn.max_iterations)
        bits = pnpsolver.PnPSolve(kps, counts, world, S.CAM, S.SF, pair, sc.rows[0], sc.draws[0][:rn.max_iterations], st, rn)
        assert bits == 2048 and st["n_inliers"][0] == -1 and st["n_correspondences"][0] == 0 and (st["inliers"] == 99).all()


def test_error_returns_and_exports():
    sc = S.scene_set()
    kps, counts, world, v, b = sc.arrays
    for kw in (dict(min_set=3), dict(min_set=5), dict(epsilon=0.0), dict(epsilon=1.5), dict(th2=0.0), dict(th2=-1.0), dict(min_inliers=0), dict(max_iterations=0),
               dict(probability=0.0), dict(probability=1.0), dict(n_iterations=-1)):
        rn = ransac(**kw)
        mi = max(rn.max_iterations, 1)
        st = fresh_state(1, sc.cap, mi)
        with pytest.raises(ola.OlfError):
            pnpsolver.PnPSolve(kps, counts, world, S.CAM, S.SF, sc.pairs[5], sc.rows[5], sc.draws[5][:mi], st, rn)
    for key in ("best_flags", "refined_Tcw", "Tcw"):
        st = fresh_state(1, sc.cap, 40)
        st[key] = None
        with pytest.raises(ola.OlfError):
            pnpsolver.PnPSolve(kps, counts, world, S.CAM, S.SF, sc.pairs[5], sc.rows[5], sc.draws[5][:40], st, ransac())
    L = _lib.lib()
    for name in ("olf_pnp_solver_pairs_dev", "olf_pnp_apply_inliers_dev", "olf_pnp_solver", "olf_pnp_solver_pairs", "olf_debug_pnp_solver_lds_limit"):
        assert hasattr(L, name)
    for name in ("pnp_ransac", "pnp_state", "pnp_draws", "pnp_solver_batch", "pnp_apply_inliers", "PnPSolve", "pnp_solver_pairs"):
        assert name in ola.__all__ and hasattr(ola, name)
    d = ola.pnp_draws(2, 7, 3)
    assert d.shape == (2, 7, 4) and d.dtype == np.uint32 and d.max() < 1 << 31


def build_adaptor(exe):
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_pnpsolver.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_adaptor_through_the_host_form(tmp_path):
    """ORB_SLAM2::PnPsolverOf against stand-in frame and map-point types, without a context: a single solver needs no device"""
    exe = str(tmp_path / "adaptor_pnpsolver")
    build_adaptor(exe)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_PNPSOLVER_OK" in out.stdout, out.stdout.decode()[-3000:]


def _san_probe(tmp):
    """can this machine build and run a sanitized program at all (tests/test_pose_cpu.py asks the same)"""
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    exe = os.path.join(tmp, "probe")
    if subprocess.run(["g++", "-fsanitize=address,undefined", src, "-o", exe], capture_output=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True).returncode == 0


def test_host_form_under_sanitizers(tmp_path):
    """tests/pnpsolver_host_main.cpp with pnpsolver_host.cpp under -fsanitize=address,undefined -ffp-contract=off: a stand-alone program, no device"""
    tmp = str(tmp_path)
    if not _san_probe(tmp):
        pytest.skip("no sanitizer runtime on this machine")
    exe = os.path.join(tmp, "pnpsolver_host_main")
    csrc = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + csrc, os.path.join(ROOT, "tests", "pnpsolver_host_main.cpp"), os.path.join(csrc, "pnpsolver_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "pnpsolver_host_main ok" in r.stdout
