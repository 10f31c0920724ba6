"""olf_initializer, the host form of Initializer::Initialize, against the numpy restatement (tests/initializer_reference.py) over the scenes of
tests/initializer_scenes.py, whose builder asserts from the restatement alone that every decision is settled.  Exact: ok, model, hypothesis,
n_correspondences, n_good (a hypothesis whose CheckRT outcome the restatement's switches move for k correspondences may differ by k: none does in these
scenes), the flags and the triangulated row outside the near set, and ransac_sample<8> against the literal swap-with-back.  Under the project's tolerance
rule (at most 16 x the restatement's spread under its switches, with a floor of 64 float ulp of the largest element): score_H / score_F,
H21 and F21 (normalised by the base's largest element: the reference leaves sign and scale open), R21, t21, P3D and cos_parallax.  Largest ratios
measured: 0.0 for the scores, H21, F21, R21 and t21 (equal bit for bit), 0.031 for cos_parallax, 0.141 for P3D.  Then C.34's cosine thresholds against a sweep of acosf, the error returns, the exports, the refused pairs, the adaptor against
stand-in types and the stand-alone sanitizer program.  (olf_initializer_apply_dev is a device entry: tests/test_initializer_gpu.py holds it against its
host restatement.)"""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import initializer_reference as R
import initializer_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, initializer
from test_pnpsolver_cpu import _san_probe

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_libm = C.CDLL("libm.so.6")
_libm.acosf.restype = C.c_float
_libm.acosf.argtypes = [C.c_float]


def sentinel_state(n_pairs, cap):
    """outputs filled with sentinels, to show what a call leaves untouched"""
    st = ola.initializer_state(n_pairs, cap, device=False)
    for k, v in st.items():
        v[...] = 77 if v.dtype == np.uint8 else -7
    return st


def host_solve(pset, names=None):
    names = S.SUBSET[pset] if names is None else names
    kps, counts, pairs, matches = S.batch(names)
    prm = ola.initializer_params(**S.SETS[pset])
    st = sentinel_state(len(names), S.CAP)
    bits = 0
    for p, n in enumerate(names):
        bits |= ola.Initialize(kps, counts, S.CAM, pairs[p], matches[p], S.draws(n, prm.max_iterations), st, prm, row=p)
    return names, st, bits


@pytest.fixture(scope="module", params=["fast", "tracker", "one"])
def solved(request):
    pset = request.param
    names, st, bits = host_solve(pset)
    assert bits == 0
    return pset, names, st


def test_builder_conditions():
    S.conditions()


def test_discrete_results_equal_the_restatement(solved):
    pset, names, st = solved
    for p, n in enumerate(names):
        a, s = S.analyse(n, pset), S.scene(n)
        b = a.base
        N1 = min(int(s.counts[0]), S.CAP)
        assert (st["n_correspondences"][p], st["ok"][p], st["model"][p]) == (b.N, b.ok, b.model), n
        if b.N < 8:                                                  # only ok, model and n_correspondences are written
            for k in ("hypothesis", "score_H", "n_good", "inliers_H", "inliers_F", "H21", "R21", "P3D", "triangulated", "cos_parallax"):
                assert (st[k][p] == (77 if st[k].dtype == np.uint8 else -7)).all(), (n, k)
            continue
        assert st["hypothesis"][p] == b.hypothesis, n
        for h in range(8):
            k = int(a.unstable[h].sum()) if h < len(a.unstable) else 0
            assert abs(int(st["n_good"][p, h]) - b.n_good[h]) <= k, (n, h, st["n_good"][p], b.n_good)
        keep = ~a.near
        for key, flags in (("inliers_H", b.flags_H), ("inliers_F", b.flags_F)):
            row = st[key][p]
            assert (row[N1:] == 77).all() and not row[np.setdiff1d(np.arange(N1), b.feat)].any(), (n, key)
            assert np.array_equal(row[b.feat][keep], flags[keep].astype(np.uint8)), (n, key)
        if b.ok:
            tri = st["triangulated"][p]
            assert (tri[N1:] == 77).all() and not tri[np.setdiff1d(np.arange(N1), b.feat)].any(), n
            assert np.array_equal(tri[b.feat][keep], b.good[keep].astype(np.uint8)), n
            assert not st["P3D"][p][np.setdiff1d(np.arange(N1), b.feat)].any() and (st["P3D"][p][N1:] == -7).all(), n
        else:
            assert (st["triangulated"][p] == 77).all() and (st["P3D"][p] == -7).all() and (st["R21"][p] == -7).all() and (st["t21"][p] == -7).all(), n


def test_sample_is_the_literal_swap_with_back():
    rng = np.random.default_rng(5)
    got = np.zeros(8, np.int32)
    for N in (8, 9, 10, 15, 16, 17, 63, 64, 65, 300, 512, 8192):
        for _ in range(200):
            r = rng.integers(0, 1 << 32, size=8, dtype=np.uint32)   # (bit 31 is ignored)
            assert _lib.lib().olf_debug_initializer_sample(N, r.ctypes.data, got.ctypes.data) == 0
            assert list(got) == R.sample8(N, r), (N, r)
    r = np.full(8, 0x7fffffff, np.uint32)                            # every draw picks the back
    _lib.lib().olf_debug_initializer_sample(8, r.ctypes.data, got.ctypes.data)
    assert list(got) == R.sample8(8, r) and sorted(got) == list(range(8))


def _ratio(got, base, alts):
    base = np.asarray(base, np.float64).reshape(-1)
    got = np.asarray(got, np.float64).reshape(-1)
    spread = np.max([np.abs(np.asarray(x, np.float64).reshape(-1) - base) for x in alts], axis=0)
    floor = 64 * np.spacing(F(np.abs(base).max()))
    return float(np.max(np.abs(got - base) / np.maximum(16 * spread, floor))) if len(base) else 0.0


def _unit(M, k):
    M = np.asarray(M, np.float64).reshape(-1)
    return M / M[k]


def test_values_meet_the_tolerance_rule(solved):
    pset, names, st = solved
    worst = {}

    def note(key, v):
        worst[key] = max(worst.get(key, 0.0), v)

    for p, n in enumerate(names):
        a = S.analyse(n, pset)
        b = a.base
        if b.N < 8:
            continue
        note("score_H", _ratio(st["score_H"][p], b.score_H, [o.score_H for o in a.alts]))
        note("score_F", _ratio(st["score_F"][p], b.score_F, [o.score_F for o in a.alts]))
        for key, M, Ms in (("H21", b.H21, [o.H21 for o in a.alts]), ("F21", b.F21, [o.F21 for o in a.alts])):
            if M is None:
                assert (st[key][p] == -7).all()
                continue
            k = int(np.argmax(np.abs(np.asarray(M).reshape(-1))))
            note(key, _ratio(_unit(st[key][p], k), _unit(M, k), [_unit(x, k) for x in Ms]))
        # cos_parallax of the hypotheses whose counted set no switch moves (the alts' hypotheses are matched to the base's: ReconstructF's order follows a sign)
        for h in range(len(b.Rs)):
            if a.unstable[h].any() or b.n_good[h] == 0:
                continue
            others = []
            for o in a.alts:
                ho = int(np.argmin([np.abs(o.Rs[k] - b.Rs[h]).sum() + np.abs(o.ts[k] - b.ts[h]).sum() for k in range(len(o.Rs))]))
                others.append(o.cos_parallax[ho])
            note("cos_parallax", _ratio(st["cos_parallax"][p, h], b.cos_parallax[h], others))
        if b.ok:
            note("R21", _ratio(st["R21"][p], b.R21, [o.R21 for o in a.alts]))
            note("t21", _ratio(st["t21"][p], b.t21, [o.t21 for o in a.alts]))
            keep = b.counted & ~a.near
            for o in a.alts:
                keep &= o.counted
            note("P3D", _ratio(st["P3D"][p][b.feat][keep], b.P3D[keep], [o.P3D[keep] for o in a.alts]))
    print("largest ratios of the tolerance rule (1 = the bound), host form against base, set %s:" % pset, {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def test_cos_thresholds_against_acosf():
    """C.34: c passes `parallax > mp` iff c <= cos_gt, and `>=` iff c <= cos_ge, over the floats around each threshold and at the ends of [-1, 1]"""
    gt, ge = C.c_float(0), C.c_float(0)

    def deg(c):
        return F(float(F(_libm.acosf(float(c))) * F(180)) / R.PI)

    for mp in (1.0, 0.5, 5.0, 0.25, 45.0, 90.0, 179.0, 0.0, -1.0, 180.0, 200.0, 1e-3):
        assert _lib.lib().olf_debug_initializer_cos_thresholds(mp, C.addressof(gt), C.addressof(ge)) == 0
        for thr, strict in ((F(gt.value), True), (F(ge.value), False)):
            sweep = [F(-1), F(1), F(0), np.nextafter(F(1), F(0)), np.nextafter(F(-1), F(0))]
            if not np.isnan(thr):
                lo = hi = thr
                for _ in range(1500):
                    lo, hi = np.nextafter(lo, F(-2)), np.nextafter(hi, F(2))
                    sweep += [lo, hi]
                sweep.append(thr)
            for c in sweep:
                if not (-1 <= c <= 1):
                    continue
                want = deg(c) > F(mp) if strict else deg(c) >= F(mp)
                assert bool(want) == bool(c <= thr), (mp, strict, float(c), float(thr))
    assert _lib.lib().olf_debug_initializer_cos_thresholds(200.0, C.addressof(gt), C.addressof(ge)) == 0 and np.isnan(gt.value) and np.isnan(ge.value)
    assert _lib.lib().olf_debug_initializer_cos_thresholds(-1.0, C.addressof(gt), C.addressof(ge)) == 0 and gt.value == 1.0 and ge.value == 1.0
    assert _lib.lib().olf_debug_initializer_cos_thresholds(0.0, C.addressof(gt), C.addressof(ge)) == 0 and gt.value < 1.0 and ge.value == 1.0
    assert _lib.lib().olf_debug_initializer_cos_thresholds(1.0, C.addressof(gt), C.addressof(ge)) == 0
    assert initializer.parallax_degrees(F(gt.value)) > 1.0 and initializer.parallax_degrees(np.nextafter(F(gt.value), F(2))) <= 1.0


def test_error_returns_exports_and_refused_pairs():
    kps, counts, pairs, matches = S.batch(["general"])
    dr = S.draws("general", 24)
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(max_iterations=0), dict(min_triangulated=-1),
               dict(min_parallax=float("nan")), dict(min_parallax=float("inf"))):
        st = sentinel_state(1, S.CAP)
        with pytest.raises(ola.OlfError):
            ola.Initialize(kps, counts, S.CAM, pairs[0], matches[0], dr, st, ola.initializer_params(**dict(S.FAST, **kw)))
    for key in ("ok", "H21", "P3D", "cos_parallax"):
        st = sentinel_state(1, S.CAP)
        st[key] = None
        with pytest.raises(ola.OlfError):
            ola.Initialize(kps, counts, S.CAM, pairs[0], matches[0], dr, st, ola.initializer_params(**S.FAST))
    for pair in ((0, 0), (-1, 1), (0, 2), (2, 0)):
        st = sentinel_state(1, S.CAP)
        bits = ola.Initialize(kps, counts, S.CAM, pair, matches[0], dr, st, ola.initializer_params(**S.FAST))
        assert bits == 2048 and st["ok"][0] == -1
        assert all((v == (77 if v.dtype == np.uint8 else -7)).all() for k, v in st.items() if k != "ok")
    L = _lib.lib()
    for name in ("olf_initializer_pairs_dev", "olf_initializer_apply_dev", "olf_initializer", "olf_initializer_pairs", "olf_debug_initializer_lds_limit",
                 "olf_debug_initializer_cos_thresholds", "olf_debug_initializer_sample"):
        assert hasattr(L, name)
    for name in ("initializer_params", "initializer_draws", "initializer_batch", "initializer_pairs", "Initialize", "initializer_apply"):
        assert name in ola.__all__ and hasattr(ola, name)
    d = ola.initializer_draws(2, 7, 3)
    assert d.shape == (2, 7, 8) and d.dtype == np.uint32 and d.max() < 1 << 31


def build_adaptor(exe):
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_initializer.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_adaptor_through_the_host_form(tmp_path):
    """ORB_SLAM2::InitializerOf against stand-in frame types, without a context: a single initialiser needs no device"""
    exe = str(tmp_path / "adaptor_initializer")
    build_adaptor(exe)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_INITIALIZER_OK" in out.stdout, out.stdout.decode()[-3000:]


def test_host_form_under_sanitizers(tmp_path):
    """tests/initializer_host_main.cpp with initializer_host.cpp under -fsanitize=address,undefined -ffp-contract=off: a stand-alone program, no device"""
    tmp = str(tmp_path)
    if not _san_probe(tmp):
        pytest.skip("no sanitizer runtime on this machine")
    exe = os.path.join(tmp, "initializer_host_main")
    csrc = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + csrc, os.path.join(ROOT, "tests", "initializer_host_main.cpp"), os.path.join(csrc, "initializer_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "initializer_host_main ok" in r.stdout
