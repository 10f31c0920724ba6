"""The host forms of the line half of tracking -- olf_is_in_frustum_l (Frame::isInFrustum_l, src/Frame.cc:446-515), olf_local_lines_assign (the loop of
Tracking::SearchLocalPointsAndLines, src/Tracking.cc:1974-2023) and olf_track_lines_assign (the f2f line tracking, :1305-1349 / :976-1020) -- against the
oracle-built expectations of line_scenes.py, bit for bit, on the scenes test_line_batch_gpu.py runs on the device.  The floors are asserted here on the
EXPECTED outputs, so the scenes are known to exercise every case of the loops before anything runs on a GPU.  No device is touched."""
import ctypes as C
import numpy as np
import pytest
import line_scenes as ls
from orb_line_slam_amd import matcher
from orb_line_slam_amd._lib import OLF_ERR_INVALID, lib, ptr

i32 = np.int32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(ls.LOCAL_CASES))
def test_is_in_frustum_l_host(oracle, name):
    frames, mp, _, _ = ls.local_case(oracle, name)
    for fr in frames:
        inv_o, proj_o = ls.expect_is_in_frustum_l(oracle, fr, mp.world, mp.bounds)
        inv, proj4 = matcher.isInFrustum_l(fr.view(mp.bounds), mp.world)
        assert np.array_equal(inv, inv_o) and np.array_equal(bits(proj4), bits(proj_o))
    assert sum(int(ls.expect_is_in_frustum_l(oracle, fr, mp.world, mp.bounds)[0].sum()) for fr in frames) >= 1000


def test_frustum_floors(oracle):
    """the shrunk bounds reject at each of the eight end point gates, and an end point of either kind lies behind the camera"""
    frames, mp, _, _ = ls.local_case(oracle, "shrunk")
    total = {}
    for fr in frames:
        for k, v in ls.frustum_gate_counts(oracle, fr, mp).items():
            total[k] = total.get(k, 0) + v
    assert len(total) == 10 and all(v >= 1 for v in total.values()), total


def host_local_assign(fr, mp, e):
    m12, fm, n = e["m12_before"].astype(i32).copy(), e["frame_ml0"].astype(i32).copy(), np.zeros(1, i32)
    midx, proj = np.ascontiguousarray(e["midx"], i32), np.ascontiguousarray(e["proj4_rank"], np.float32)
    obs = np.ascontiguousarray(mp.obs, np.uint8)
    rc = lib().olf_local_lines_assign(len(m12), ptr(m12), ptr(midx), ptr(proj), ptr(np.ascontiguousarray(fr.kls)), len(fr.kls), ptr(fr.ldisp), *mp.bounds, mp.n,
                                      ptr(obs), ptr(fm), ptr(n))
    assert rc == 0
    return m12, fm, int(n[0])


@pytest.mark.parametrize("name", list(ls.LOCAL_CASES))
def test_local_lines_assign_host(oracle, name):
    frames, mp, _, exp = ls.local_case(oracle, name)
    for fr, e in zip(frames, exp):
        m12, fm, n = host_local_assign(fr, mp, e)
        assert np.array_equal(m12, e["m12_after"]) and np.array_equal(fm, e["frame_ml"]) and n == e["n_inliers"]


@pytest.mark.parametrize("name", ["lists_a", "lists_b", "no_lists"])
def test_local_floors(oracle, name):
    frames, mp, lists, exp = ls.local_case(oracle, name)
    fl = [ls.local_floors(fr, mp, e) for fr, e in zip(frames, exp)]
    for k in ls.LOOP_FLOORS:
        assert sum(f[k] for f in fl) >= 1, (k, fl)
    want = ls.LOCAL_CASES[name]["want"]
    views = sorted(int(e["in_view"].sum()) for e in exp)
    if want is not None:
        assert views[:4] == [0, 1, 256, 257] and views[4] >= 500
        assert len(set(len(x) for x in lists)) == 5                     # uneven lists
        assert name != "lists_a" or min(len(x) for x in lists) == 0     # one of them empty
    nontrivial = [f for fr, e, f in zip(frames, exp, fl) if len(fr.kls) >= 70 and e["in_view"].sum() >= 256]
    assert len(nontrivial) >= 1 and all(f["assigned"] >= 40 for f in nontrivial), fl
    held = np.concatenate([fr.frame_ml[fr.frame_ml >= 0] for fr in frames])
    assert mp.bad[held].any() and mp.obs[held].any() and (~mp.obs[held]).any()
    assert any((e["frame_ml0"] >= 0).any() for e in exp)


@pytest.mark.parametrize("best_lr", [False, True])
@pytest.mark.parametrize("mode", list(ls.F2F_MODES))
def test_track_lines_assign_host(oracle, mode, best_lr):
    frames, exp = ls.f2f_case(oracle, mode, best_lr)
    m = ls.F2F_MODES[mode]
    for j, e in enumerate(exp):
        last, cur = frames[j], frames[j + 1]
        m12, cm, n = e["m12_before"].astype(i32).copy(), np.full(len(cur.kls), 7, i32), np.zeros(1, i32)
        rc = lib().olf_track_lines_assign(len(m12), ptr(m12), ptr(np.ascontiguousarray(last.kls)), ptr(last.ml), len(cur.kls), ptr(np.ascontiguousarray(cur.kls)),
                                          ptr(cur.ldisp), *ls.BOUNDS, int(m["skip_null"]), int(m["gates"]), float(m["delta_angle"]), float(m["pos_frac"]),
                                          ptr(cm), ptr(n))
        assert rc == 0
        assert np.array_equal(m12, e["m12"]) and np.array_equal(cm, e["cur_ml"]) and int(n[0]) == e["n_inliers"]


def test_f2f_floors(oracle):
    fl = {(mode, lr): ls.f2f_floors(*ls.f2f_case(oracle, mode, lr), mode) for mode in ls.F2F_MODES for lr in (False, True)}
    for k, f in fl.items():
        assert f["assigned"] >= 60, (k, f)
    for mode in ("motion_model", "gates_keep_null"):
        assert fl[(mode, False)]["gate_rejected"] >= 5 and fl[(mode, False)]["straddle_kept"] >= 1, fl
    assert fl[("motion_model", False)]["shared_i2"] >= 1 and fl[("reference_kf", False)]["shared_i2"] >= 1      # the last i1 wins, all are counted
    assert fl[("motion_model", False)]["null_skipped"] >= 1 and fl[("reference_kf", False)]["null_assigned"] >= 1


def test_host_forms_refuse_bad_arguments(oracle):
    frames, mp, _, exp = ls.local_case(oracle, "no_lists")
    fr, e = frames[0], exp[0]
    assert lib().olf_is_in_frustum_l(None, 1, None, None, None) == OLF_ERR_INVALID
    m12, fm, n = e["m12_before"].astype(i32).copy(), e["frame_ml0"].astype(i32).copy(), np.zeros(1, i32)
    midx, proj, obs = np.ascontiguousarray(e["midx"], i32), np.ascontiguousarray(e["proj4_rank"], np.float32), np.ascontiguousarray(mp.obs, np.uint8)
    kls = np.ascontiguousarray(fr.kls)
    call = lambda m, mi, f: lib().olf_local_lines_assign(len(m), ptr(m), ptr(mi), ptr(proj), ptr(kls), len(kls), ptr(fr.ldisp), *mp.bounds, mp.n, ptr(obs), ptr(f),
                                                         ptr(n))
    bad = m12.copy(); bad[3] = len(kls)
    assert call(bad, midx, fm) == OLF_ERR_INVALID
    bad = midx.copy(); bad[3] = mp.n
    assert call(m12, bad, fm) == OLF_ERR_INVALID
    bad = fm.copy(); bad[3] = mp.n
    assert call(m12, midx, bad) == OLF_ERR_INVALID
    assert lib().olf_local_lines_assign(len(m12), None, ptr(midx), ptr(proj), ptr(kls), len(kls), ptr(fr.ldisp), *mp.bounds, mp.n, ptr(obs), ptr(fm), ptr(n)) == OLF_ERR_INVALID
    assert lib().olf_track_lines_assign(3, None, None, None, 3, None, None, *ls.BOUNDS, 1, 1, 0.1, 0.1, None, ptr(n)) == OLF_ERR_INVALID
