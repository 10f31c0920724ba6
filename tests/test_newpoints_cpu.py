"""olf_compute_f12, olf_create_new_map_points and olf_update_normal_and_depth without a device: the conditions the scene builder promises
(tests/newpoints_scenes.py), the host forms against the restatements (tests/newpoints_reference.py) -- F12 and normal / depth bit for bit, codes and nnew
exactly, x3D of the codes 2 / 3 bit for bit, x3D of code 1 by the tolerance rule --, malformed input, the slot-0 quirk of observations[pRefKF], the
argument checks and the exports.

Two of the reference's eight `continue`s do not occur in the scene set and cannot with the margins the builder keeps: `w == 0` (:334) needs parallel rays,
which the parallax test sends to the other branches, and `dist == 0` (:423) needs x3D on a camera centre, where z <= 0 rejects first.  The other six and
the three creating branches are asserted to occur at least 3 times each."""
import ctypes as C
import numpy as np
import pytest
import newpoints_reference as R
import newpoints_scenes as S
from orb_line_slam_amd import _lib, newpoints
from orb_line_slam_amd._lib import OLF_ERR_INVALID, lib

F = np.float32
CAP = 448


# ---- the scene builder --------------------------------------------------------------------------------------------------------------------------------
def test_scene_conditions():
    sc = S.scene_set()
    assert [len(r) for r in sc.refs] == list(S.ROW_COUNTS) + [65]
    h = S.code_histogram(sc.refs)
    print("codes of the scene set:", sorted(h.items()))
    for code in (R.TRIANGULATED, R.UNPROJECT_1, R.UNPROJECT_2, R.LOW_PARALLAX, R.Z1, R.Z2, R.REPROJ_1, R.REPROJ_2, R.SCALE_RATIO):
        assert h.get(code, 0) >= 3, (code, h)
    for fr in sc.frames[1:]:
        t = float(np.linalg.norm(fr.Tcw[:3, 3].astype(np.float64)))
        ang = np.degrees(np.arccos(np.clip((np.trace(fr.Tcw[:3, :3].astype(np.float64)) - 1) / 2, -1, 1)))
        assert 0.02 <= t <= 1.0 and ang <= 5.01


# ---- ComputeF12 -----------------------------------------------------------------------------------------------------------------------------------------
def test_f12_host_against_restatement():
    sc = S.scene_set()
    cam = (S.FX, S.FY, S.CX, S.CY)
    for a in range(6):
        for b in range(6):
            if a == b:
                continue
            got = newpoints.ComputeF12(sc.frames[a].Tcw, sc.frames[b].Tcw, cam)
            exp = R.compute_f12(sc.frames[a].Tcw, sc.frames[b].Tcw, cam)
            assert np.array_equal(S.bits(got), S.bits(exp)), (a, b, got, exp)
            # and it is a fundamental matrix: the float64 formula agrees to float accuracy
            T1, T2 = sc.frames[a].Tcw.astype(np.float64), sc.frames[b].Tcw.astype(np.float64)
            R12 = T1[:3, :3] @ T2[:3, :3].T
            t = -R12 @ T2[:3, 3] + T1[:3, 3]
            tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
            Ki = np.linalg.inv(np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]]))
            F64 = Ki.T @ tx @ R12 @ Ki
            assert np.max(np.abs(got - F64)) <= 1e-4 * np.max(np.abs(F64))


def test_f12_singular_calibration_is_zero():
    sc = S.scene_set()
    assert not newpoints.ComputeF12(sc.frames[0].Tcw, sc.frames[1].Tcw, (0.0, S.FY, S.CX, S.CY)).any()      # cv::invert of a singular matrix: zeros


# ---- CreateNewMapPoints -------------------------------------------------------------------------------------------------------------------------------
def host_create(frames, pairs, rows, monocular=False, img_stride=1, cap=CAP, mb=S.MB, sf=S.SF):
    kps, cnt, ur, depth, Tcw = S.batch_arrays(frames, cap, img_stride)
    return newpoints.CreateNewMapPoints(kps, cnt, ur, depth, Tcw, S.CAM5, mb, sf, pairs, S.match_rows(rows, cap), monocular, img_stride)


@pytest.mark.parametrize("img_stride", [1, 2])
def test_create_host_against_restatement(img_stride):
    sc = S.scene_set()
    x3D, code, nnew, status = host_create(sc.frames, sc.pairs, sc.rows, img_stride=img_stride)
    assert status == 0
    worst = S.check_rows(x3D, code, nnew, sc.refs)
    print("largest ratio of the tolerance rule, host form against base:", worst)


def test_create_host_malformed():
    sc = S.scene_set()
    good = host_create(sc.frames, sc.pairs, sc.rows)
    # bad pairs: nnew = -1, bit 2048, the neighbours as before
    pairs = [(0, 0), sc.pairs[3], (-1, 2), sc.pairs[5], (2, 6)]
    rows = [sc.rows[0], sc.rows[3], sc.rows[0], sc.rows[5], sc.rows[0]]
    x3D, code, nnew, status = host_create(sc.frames, pairs, rows)
    assert status == 2048 and list(nnew[[0, 2, 4]]) == [-1, -1, -1]
    assert not code[[0, 2, 4]].any() and not x3D[[0, 2, 4]].any()    # (the wrapper's arrays start as zeros: untouched)
    for q, p in ((1, 3), (3, 5)):
        assert np.array_equal(code[q], good[1][p]) and np.array_equal(S.bits(x3D[q]), S.bits(good[0][p])) and nnew[q] == good[2][p]
    # an idx2 outside [0, N2) is no match; an octave outside the levels leaves the match out with bit 256: both equal the run without the element
    i_a, i_b = sorted(sc.refs[5])[:2]
    row = sc.rows[5].copy()
    row[i_a] = S.POOL + 3
    frames = [fr for fr in sc.frames]
    import copy
    frames[5] = copy.deepcopy(sc.frames[5])
    frames[5].keys["octave"][i_b] = 8
    x3D, code, nnew, status = host_create(frames, [sc.pairs[5]], [row])
    clean = sc.rows[5].copy()
    clean[[i_a, i_b]] = -1
    ex3D, ecode, ennew, estatus = host_create(sc.frames, [sc.pairs[5]], [clean])
    assert status == 256 and estatus == 0
    assert np.array_equal(code, ecode) and np.array_equal(S.bits(x3D), S.bits(ex3D)) and nnew[0] == ennew[0] and code[0, i_a] == 0 and code[0, i_b] == 0


def test_create_host_baseline_skip():
    """baseline < mb skips the pair unless monocular (:249-253): nnew = 0 and an all-0 row"""
    sc = S.scene_set()
    x3D, code, nnew, status = host_create(sc.frames, [sc.pairs[5]], [sc.rows[5]], mb=50.0)
    assert status == 0 and nnew[0] == 0 and not code.any() and not x3D.any()
    x3D, code, nnew, status = host_create(sc.frames, [sc.pairs[5]], [sc.rows[5]], mb=50.0, monocular=True)
    assert code.any()


# ---- UpdateNormalAndDepth -----------------------------------------------------------------------------------------------------------------------------
def host_und(s, points=None, graph=None):
    g, v = graph or S.snapshot_graph(s)
    start = np.full((s.n_mp, 3), -7.0, F), np.full(s.n_mp, -7.0, F), np.full(s.n_mp, -7.0, F)
    return newpoints.UpdateNormalAndDepth(g, v, s.mp_world, s.ref_kf, s.kf_Ow, S.SF, *start, points=points)


def assert_und(got, exp):
    for a, b, what in zip(got[:3], exp, ("normal", "maxd", "mind")):
        assert np.array_equal(S.bits(a), S.bits(b)), (what, np.flatnonzero((S.bits(a) != S.bits(b)).reshape(len(b), -1).any(1))[:8])


def test_normal_depth_host_against_restatement():
    s = S.snapshot(3)
    got = host_und(s)
    assert got[3] == 0
    assert_und(got, S.snapshot_expected(s))
    assert (got[1][[0, 3]] == -7).all()                              # the empty row and the bad point are untouched
    lst = [5, 1, 40, 5, 3, 0]
    got = host_und(s, points=lst)
    assert_und(got, S.snapshot_expected(s, points=lst))
    assert (got[1] != -7).sum() == 3


def test_slot_0_quirk():
    """a row that does not name the reference key frame: observations[pRefKF] inserts slot 0 and mvKeysUn[0].octave is read"""
    s = S.snapshot(3)
    assert len(s.outside) >= 3
    got = host_und(s)
    for p in s.outside:
        ref = int(s.ref_kf[p])
        dist = F(np.sqrt(np.sum((s.mp_world[p] - s.kf_Ow[ref]).astype(np.float64) ** 2)))
        assert got[1][p] == dist * S.SF[s.octave[ref][0]]
    # with octave[ref][0] changed the distance follows; with another slot changed it does not
    p = s.outside[0]
    ref = int(s.ref_kf[p])
    s.octave[ref][0] = (s.octave[ref][0] + 3) % 8
    s.octave[ref][1] = (s.octave[ref][1] + 3) % 8
    again = host_und(s)
    assert again[1][p] != got[1][p] and again[1][p] == F(np.sqrt(np.sum((s.mp_world[p] - s.kf_Ow[ref]).astype(np.float64) ** 2))) * S.SF[s.octave[ref][0]]


def malformed_snapshot(s, g, v):
    """an observation by a key frame outside the graph (point 10), a slot outside its key frame's row (point 11), a reference key frame outside the graph
    (point 12), an octave outside the levels at the reference's slot (point 14): the arrays are changed in place"""
    off = g.mp_obs_offsets
    g.mp_obs_kf[off[10] + 1] = s.n_kf + 5
    v.mp_obs_slot[off[11]] = s.slots
    s.ref_kf[12] = -2
    r13 = int(s.ref_kf[14])
    slot13 = s.mp_obs_slot[14][s.mp_obs[14].index(r13)]
    v.kf_slot_octave[r13 * s.slots + slot13] = 8


def cleaned_snapshot(s):
    """the same snapshot without the offending elements"""
    import copy
    c = copy.deepcopy(s)
    for p, k in ((10, 1), (11, 0)):
        del c.mp_obs[p][k]
        del c.mp_obs_slot[p][k]
    return c


def test_normal_depth_host_malformed():
    s = S.snapshot(4)
    for p in (10, 11):                                               # (the reference key frame is not the removed observation)
        k = 1 if p == 10 else 0
        if s.mp_obs[p][k] == s.ref_kf[p]:
            s.ref_kf[p] = s.mp_obs[p][2]
    exp = list(S.snapshot_expected(cleaned_snapshot(s)))
    g, v = S.snapshot_graph(s)
    malformed_snapshot(s, g, v)
    got = host_und(s, graph=(g, v))
    assert got[3] == 256 | 4096
    for a in exp:
        a[[12, 14]] = -7                                             # untouched
    assert_und(got, exp)
    got = host_und(s, points=[s.n_mp, 2, -1], graph=(g, v))
    assert got[3] == 512 and (got[1] != -7).sum() == 1


# ---- arguments and exports ---------------------------------------------------------------------------------------------------------------------------
def test_exports():
    L = lib()
    for name in ("olf_compute_f12_pairs_dev", "olf_compute_f12", "olf_create_new_map_points_batch_dev", "olf_create_new_map_points",
                 "olf_update_normal_and_depth_dev", "olf_update_normal_and_depth"):
        assert hasattr(L, name), name


def test_argument_errors():
    L = lib()
    T = np.eye(4, dtype=F)
    out = np.zeros(9, F)
    assert L.olf_compute_f12(None, _lib.ptr(T), 1.0, 1.0, 0.0, 0.0, _lib.ptr(out)) == OLF_ERR_INVALID
    assert L.olf_compute_f12(_lib.ptr(T), _lib.ptr(T), 1.0, 1.0, 0.0, 0.0, None) == OLF_ERR_INVALID
    s = S.snapshot(3, extra=2)
    g, v = S.snapshot_graph(s)
    gc, vc = g.c(), v.c()
    st = C.c_int32(0)
    w, r, ow = (np.ascontiguousarray(a) for a in (s.mp_world, s.ref_kf, s.kf_Ow))
    n, a, b = np.zeros((s.n_mp, 3), F), np.zeros(s.n_mp, F), np.zeros(s.n_mp, F)
    call = lambda **kw: L.olf_update_normal_and_depth(*[kw.get(k, d) for k, d in (
        ("g", C.byref(gc)), ("v", C.byref(vc)), ("n", s.n_mp), ("pts", None), ("w", _lib.ptr(w)), ("r", _lib.ptr(r)), ("ow", _lib.ptr(ow)), ("sf", _lib.ptr(S.SF)),
        ("nl", 8), ("normal", _lib.ptr(n)), ("maxd", _lib.ptr(a)), ("mind", _lib.ptr(b)), ("st", C.addressof(st)))])
    assert call() == 0
    for kw in (dict(g=None), dict(v=None), dict(n=-1), dict(w=None), dict(r=None), dict(ow=None), dict(sf=None), dict(nl=0), dict(nl=17), dict(normal=None),
               dict(maxd=None), dict(mind=None), dict(st=None)):
        assert call(**kw) == OLF_ERR_INVALID, kw
    bad = g.mp_obs_offsets.copy()
    g.mp_obs_offsets[2] = g.mp_obs_offsets[3] + 1                    # not non-decreasing
    gc = g.c()
    assert call(g=C.byref(gc)) == OLF_ERR_INVALID
    g.mp_obs_offsets[:] = bad
    # olf_create_new_map_points
    sc = S.scene_set()
    kps, cnt, ur, depth, Tcw = S.batch_arrays(sc.frames, CAP)
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride, tb.uright, tb.Tcw = _lib.ptr(kps), _lib.ptr(cnt), 1, _lib.ptr(ur), _lib.ptr(Tcw)
    pairs, m12 = np.array([[0, 1]], np.int32), np.full((1, CAP), -1, np.int32)
    x3D, code, nnew = np.zeros((1, CAP, 3), F), np.zeros((1, CAP), np.uint8), np.zeros(1, np.int32)
    create = lambda **kw: L.olf_create_new_map_points(*[kw.get(k, d) for k, d in (
        ("tb", C.byref(tb)), ("cap", CAP), ("nf", 6), ("depth", _lib.ptr(depth)), ("mb", 0.2), ("sf", _lib.ptr(S.SF)), ("nl", 8), ("np", 1), ("pairs", _lib.ptr(pairs)),
        ("m12", _lib.ptr(m12)), ("mono", 0), ("x3D", _lib.ptr(x3D)), ("code", _lib.ptr(code)), ("nnew", _lib.ptr(nnew)), ("st", C.addressof(st)))])
    assert create() == 0
    for kw in (dict(tb=None), dict(cap=-1), dict(nf=-1), dict(depth=None), dict(sf=None), dict(nl=0), dict(np=-1), dict(pairs=None), dict(m12=None), dict(x3D=None),
               dict(code=None), dict(nnew=None), dict(st=None)):
        assert create(**kw) == OLF_ERR_INVALID, kw
    assert create(np=0, pairs=None, m12=None, x3D=None, code=None, nnew=None) == 0      # n_pairs == 0 writes nothing


# ---- the adaptor -----------------------------------------------------------------------------------------------------------------------------------------
def build_adaptor(exe):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(root, "tests", "adaptor_newpoints.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_adaptor_through_the_host_forms(tmp_path):
    """ORB_SLAM2::ComputeF12, CreateNewMapPoints and MapGraphOf::UpdateNormalAndDepth against stand-in types, without a context: no device is needed"""
    import subprocess
    exe = str(tmp_path / "adaptor_newpoints")
    build_adaptor(exe)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_NEWPOINTS_OK" in out.stdout, out.stdout.decode()[-3000:]
