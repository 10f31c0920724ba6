"""olf_sim3_solver, the host form of Sim3Solver's RANSAC, against the numpy restatement (tests/sim3solver_reference.py) over the scenes of
tests/sim3solver_scenes.py, whose builder asserts from the restatement alone that the discrete results are comparable exactly: the correspondences, the cap,
the accepting iteration, the state, the flags outside the near set and the integer gates are exact; R, t, s and T12 of the accepted hypothesis meet the
project's tolerance rule -- 16 x the restatement's spread under its switches, with a floor of 64 float ulp of the output's largest element.  Largest ratio
measured: 0.016 of 1 in both scale modes (the floor decides: at most one float ulp apart).  Then resumption, max_iterations 1 / 5 / 300, the error
returns, the exports, the adaptor against mock types and the stand-alone sanitizer program."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import sim3solver_reference as R
import sim3solver_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, sim3solver

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_KEYS = ("iterations_done", "best_inliers", "best_s", "best_R", "best_t", "best_T12", "accepted", "no_more", "n_inliers", "inliers",
              "n_correspondences", "counts")
SENTINEL = -7


def ransac(sc, n_iterations=S.MAX_ITS, max_iterations=S.MAX_ITS):
    return sim3solver.sim3_ransac(sc.fix_scale, S.PROB, S.MIN_INLIERS, max_iterations, n_iterations)


def fresh_state(n_pairs, cap, max_iterations=S.MAX_ITS):
    """a new solver per pair; counts and the inlier rows start as sentinels"""
    st = sim3solver.sim3_state(n_pairs, cap, max_iterations, device=False)
    st["counts"][:] = SENTINEL
    st["inliers"][:] = 99
    return st


def host_call(sc, st, rn, pairs=None, rows=None, draws=None, arrays=None, img_stride=1, sf=S.SF, valid=True, bad=True):
    """one olf_sim3_solver call per listed pair on its row of st; returns the status bits ORed"""
    kps, counts, Tcw, world, v, b = arrays or sc.arrays
    pairs, rows, draws = (sc.pairs if pairs is None else pairs), (sc.rows if rows is None else rows), (sc.draws if draws is None else draws)
    bits = 0
    for p, pair in enumerate(pairs):
        bits |= sim3solver.Sim3Solve(kps, counts, Tcw, world, S.CAM, sf, pair, rows[p], draws[p][:rn.max_iterations], st, rn, row=p,
                                     mp_valid=v if valid else None, mp_bad=b if bad else None, img_stride=img_stride)
    return bits


def _bits(v):
    """float32 as its bits; a NaN as one pattern, IEEE 754 leaving a NaN's sign and payload open (0 / 0 is 0xffc00000 on x86 and 0x7fc00000 on the device)"""
    v = np.ascontiguousarray(v, F)
    return np.where(np.isnan(v), np.uint32(0x7fc00000), v.view(np.uint32))


def same_state(a, b, keys=STATE_KEYS):
    for k in keys:
        x, y = (_bits(v) if v.dtype == np.float32 else np.asarray(v) for v in (a[k], b[k]))
        assert np.array_equal(x, y), (k, np.argwhere(x != y)[:6])


@pytest.fixture(scope="module", params=[False, True], ids=["free_scale", "fix_scale"])
def solved(request):
    sc, an = S.scene_set(request.param), S.analyse(request.param)
    st = fresh_state(len(sc.pairs), sc.cap)
    assert host_call(sc, st, ransac(sc)) == 0
    return sc, an, st


def test_builder_conditions():
    for fs in (False, True):
        an = S.analyse(fs)
        assert [a.C.N for a in an[:13]] == [0, 2, 19, 20, 21, 63, 64, 65, 300, S.CAP, 40, 30, 60]
        assert [a.out.accepted for a in an[:5]] == [0, 0, 0, 0, 1] and not an[10].out.accepted and an[10].out.no_more and an[10].st.iterations_done == 35
        assert not an[11].out.accepted and an[11].st.best_inliers == 0 and np.isnan(an[11].st.best.R).all()      # the identity sample: R is NaN
        gates = {int(g) for a in an for g in list(a.C.g1) + list(a.C.g2)}
        assert {9, 13} <= gates and len(gates) == 8


def test_discrete_results_equal_the_restatement(solved):
    sc, an, st = solved
    for p, a in enumerate(an):
        assert st["n_correspondences"][p] == a.C.N
        assert (st["accepted"][p], st["no_more"][p], st["n_inliers"][p]) == (a.out.accepted, a.out.no_more, a.out.n_inliers), p
        if a.C.N < S.MIN_INLIERS:
            assert st["iterations_done"][p] == 0 and st["best_inliers"][p] == 0 and not st["best_R"][p].any()      # state untouched
        else:
            assert (st["iterations_done"][p], st["best_inliers"][p]) == (a.st.iterations_done, a.st.best_inliers), p
        N1 = a.C.N1
        assert (st["inliers"][p, N1:] == 99).all()
        flags = st["inliers"][p, :N1]
        if a.out.accepted:
            skip = np.zeros(N1, bool)
            skip[a.C.i1[a.near_flags]] = True
            assert np.array_equal(flags[~skip], a.out.inliers[~skip]), p
        else:
            assert not flags.any()
        for j in a.clean:
            assert st["counts"][p, j] == a.counts[j], (p, j)
        assert (st["counts"][p, st["iterations_done"][p]:] == SENTINEL).all()


def test_caps_and_gates():
    for N in list(range(0, 70)) + [300, 448, 2000, 8192]:
        for m, mx in ((20, 300), (3, 1), (3, 5), (20, 5)):
            assert 1 <= R.iteration_cap(N, 0.99, m, mx) <= mx
    got = C.c_int32(0)
    for m, mx, pr in ((20, 300, 0.99), (3, 1, 0.99), (3, 5, 0.5), (20, 5, 0.99), (6, 300, 0.999), (20, 300, 0.01)):
        for N in list(range(0, 600)) + [2000, 4096, 8192]:
            assert _lib.lib().olf_debug_sim3_solver_cap(N, pr, m, mx, C.addressof(got)) == 0
            assert got.value == R.iteration_cap(N, pr, m, mx), (N, m, mx, pr)      # the table function of the C side, for every N
    assert R.iteration_cap(40, 0.99, 20, 300) == 35 and R.iteration_cap(20, 0.99, 20, 300) == 1 and R.iteration_cap(21, 0.99, 20, 300) == 3
    g = C.c_uint64(0)
    for sf in list(S.SF) + [F(1.2) ** 20]:
        assert _lib.lib().olf_debug_sim3_solver_gate(C.c_float(sf), C.addressof(g)) == 0
        assert g.value == R.gate(sf)
    assert [R.gate(s) for s in S.SF[:2]] == [9, 13]


def test_accepted_hypothesis_meets_the_tolerance_rule(solved):
    sc, an, st = solved
    worst = 0.0
    for p, a in enumerate(an):
        if not a.out.accepted:
            continue
        for key, base, alts in (("best_s", a.out.H.s, [h.s for h in a.alts]), ("best_R", a.out.H.R, [h.R for h in a.alts]),
                                ("best_t", a.out.H.t, [h.t for h in a.alts]), ("best_T12", a.out.H.T12, [h.T12 for h in a.alts])):
            base = np.asarray(base, np.float64).reshape(-1)
            got = np.asarray(st[key][p], np.float64).reshape(-1)
            spread = np.max([np.abs(np.asarray(x, np.float64).reshape(-1) - base) for x in alts], axis=0)
            floor = 64 * np.spacing(F(np.abs(base).max()))
            bound = np.maximum(16 * spread, floor)
            worst = max(worst, float(np.max(np.abs(got - base) / bound)))
    print("largest ratio of the tolerance rule (1 = the bound), host form against base:", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("window", [1, 5, 7])
def test_windows_with_carried_state_equal_find(solved, window):
    sc, an, st = solved
    P = len(sc.pairs)
    w = fresh_state(P, sc.cap)
    rn = ransac(sc, n_iterations=window)
    for _ in range(-(-S.MAX_ITS // window)):
        open_ = [p for p in range(P) if not (w["accepted"][p] or w["no_more"][p])] if _ else list(range(P))
        for p in open_:
            kps, counts, Tcw, world, v, b = sc.arrays
            sim3solver.Sim3Solve(kps, counts, Tcw, world, S.CAM, S.SF, sc.pairs[p], sc.rows[p], sc.draws[p], w, rn, row=p, mp_valid=v, mp_bad=b)
        if not open_:
            break
    same_state(w, st)


def test_resumed_after_a_rejected_acceptance(solved):
    """LoopClosing.cc:292-347: OptimizeSim3 rejects the first acceptance and iterate() is called again with mnBestInliers carried: the next acceptance
    needs n >= best, not only n > min_inliers.  Pair 8 (300 correspondences, a quarter of them inliers): the restatement says where the second acceptance
    falls and that iterations with more than min_inliers but fewer than the carried best lie in between -- the ones a fresh solver would have accepted."""
    sc, an, st = solved
    p = 8
    a = an[p]
    s2 = R.new_state()
    log = {}
    args = (S.MAX_ITS, sc.fix_scale, S.PROB, S.MIN_INLIERS, S.MAX_ITS)
    o1 = R.iterate(a.C, sc.draws[p], s2, *args, log=log)
    first = (s2.iterations_done, o1.n_inliers)
    o2 = R.iterate(a.C, sc.draws[p], s2, *args, log=log)
    assert o1.accepted and o2.accepted and o2.n_inliers >= first[1] and s2.iterations_done > first[0]
    between = [log[j][0] for j in range(first[0], s2.iterations_done - 1)]
    assert all(n < first[1] for n in between)
    if not sc.fix_scale:
        assert any(n > S.MIN_INLIERS for n in between)               # the carried best, not min_inliers, decided
    w = {k: v[p:p + 1].copy() for k, v in fresh_state(len(sc.pairs), sc.cap).items()}
    kps, counts, Tcw, world, v, b = sc.arrays
    rn = ransac(sc)
    for want_done, want_n in (first, (s2.iterations_done, o2.n_inliers)):
        sim3solver.Sim3Solve(kps, counts, Tcw, world, S.CAM, S.SF, sc.pairs[p], sc.rows[p], sc.draws[p], w, rn, row=0, mp_valid=v, mp_bad=b)
        assert (w["accepted"][0], w["iterations_done"][0], w["n_inliers"][0], w["best_inliers"][0]) == (1, want_done, want_n, want_n)
    assert (w["counts"][0, first[0]:s2.iterations_done - 1] == between).all()


@pytest.mark.parametrize("max_iterations", [1, 5, 300])
def test_max_iterations(max_iterations):
    sc, an = S.scene_set(False), S.analyse(False)
    st = fresh_state(len(sc.pairs), sc.cap, max_iterations)
    host_call(sc, st, ransac(sc, max_iterations, max_iterations))
    for p, a in enumerate(an):
        if a.C.N < S.MIN_INLIERS:
            continue
        cap = R.iteration_cap(a.C.N, S.PROB, S.MIN_INLIERS, max_iterations)
        full = a.st.iterations_done
        if a.out.accepted and full <= cap:
            assert st["accepted"][p] and st["iterations_done"][p] == full
        else:
            assert not st["accepted"][p] and st["no_more"][p] and st["iterations_done"][p] == cap


def test_octave_out_of_range_and_malformed_pairs():
    sc = S.scene_set(False)
    kps, counts, Tcw, world, v, b = (a.copy() for a in sc.arrays)
    p = 6
    kps[sc.pairs[p][0], 5]["octave"] = 8
    st = fresh_state(1, sc.cap)
    rn = ransac(sc)
    bits = sim3solver.Sim3Solve(kps, counts, Tcw, world, S.CAM, S.SF, sc.pairs[p], sc.rows[p], sc.draws[p], st, rn, mp_valid=v, mp_bad=b)
    assert bits == 256 and st["n_correspondences"][0] == 63
    C_ = R.correspondences(kps, counts, Tcw, world, v, b, tuple(F(x) for x in S.CAM), S.SF, sc.pairs[p], sc.rows[p])
    assert C_.status == 256 and C_.N == 63
    for pair in ((0, 0), (-1, 1), (0, len(sc.frames))):
        st = fresh_state(1, sc.cap)
        bits = sim3solver.Sim3Solve(kps, counts, Tcw, world, S.CAM, S.SF, pair, sc.rows[0], sc.draws[0], st, rn)
        assert bits == 2048 and st["n_inliers"][0] == -1 and st["n_correspondences"][0] == 0 and (st["inliers"] == 99).all()


def test_error_returns_and_exports():
    sc = S.scene_set(False)
    kps, counts, Tcw, world, v, b = sc.arrays
    for kw in (dict(min_inliers=2), dict(max_iterations=0), dict(probability=0.0), dict(probability=1.0), dict(n_iterations=-1)):
        args = dict(fix_scale=False, probability=0.99, min_inliers=20, max_iterations=300, n_iterations=5)
        args.update(kw)
        rn = sim3solver.sim3_ransac(**args)
        st = fresh_state(1, sc.cap, max(rn.max_iterations, 1))
        with pytest.raises(ola.OlfError):
            sim3solver.Sim3Solve(kps, counts, Tcw, world, S.CAM, S.SF, sc.pairs[5], sc.rows[5], sc.draws[5][:max(rn.max_iterations, 1)], st, rn)
    st = fresh_state(1, sc.cap)
    st["best_R"] = None
    with pytest.raises(ola.OlfError):
        sim3solver.Sim3Solve(kps, counts, Tcw, world, S.CAM, S.SF, sc.pairs[5], sc.rows[5], sc.draws[5], st, ransac(sc))
    L = _lib.lib()
    for name in ("olf_sim3_solver_pairs_dev", "olf_sim3_filter_matches_dev", "olf_sim3_solver", "olf_sim3_solver_pairs", "olf_debug_sim3_solver_lds_limit"):
        assert hasattr(L, name)
    for name in ("sim3_ransac", "sim3_state", "sim3_draws", "sim3_solver_batch", "sim3_filter_matches", "Sim3Solve", "sim3_solver_pairs"):
        assert name in ola.__all__ and hasattr(ola, name)
    d = ola.sim3_draws(2, 7, 3)
    assert d.shape == (2, 7, 3) and d.dtype == np.uint32 and d.max() < 1 << 31


def build_adaptor(exe):
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_sim3solver.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_adaptor_through_the_host_form(tmp_path):
    """ORB_SLAM2::Sim3SolverOf against stand-in key-frame and map-point types, without a context: a single solver needs no device"""
    exe = str(tmp_path / "adaptor_sim3solver")
    build_adaptor(exe)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_SIM3SOLVER_OK" in out.stdout, out.stdout.decode()[-3000:]


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
    """tests/sim3solver_host_main.cpp with sim3solver_host.cpp under -fsanitize=address,undefined -ffp-contract=off: a stand-alone program, no device"""
    tmp = str(tmp_path)
    if not _san_probe(tmp):
        pytest.skip("no sanitizer runtime on this machine")
    exe = os.path.join(tmp, "sim3solver_host_main")
    csrc = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + csrc, os.path.join(ROOT, "tests", "sim3solver_host_main.cpp"), os.path.join(csrc, "sim3solver_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "sim3solver_host_main ok" in r.stdout


def test_ransac_sample_equals_the_literal_procedure(tmp_path):
    """tests/ransac_sample_main.cpp: ransac_sample<3> (this solver's sample) and ransac_sample<4> (PnPsolver's) of csrc/ransac_terms.hpp against the
    literal array procedure, for every N from K to 9 and every tuple of positions, bit 31 of a draw included; built as the host form above is (without
    the sanitizers where the machine has no runtime for them)"""
    tmp = str(tmp_path)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if _san_probe(tmp) else []
    exe = os.path.join(tmp, "ransac_sample_main")
    csrc = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + san + ["-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc,
                                                      os.path.join(ROOT, "tests", "ransac_sample_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "ransac_sample_main ok" in r.stdout
