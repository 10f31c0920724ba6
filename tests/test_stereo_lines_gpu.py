"""GPU parity of stereo line matching (csrc/linematch.hip, Frame::ComputeStereoMatches_Lines) on the constructed key lines of
tests/stereo_line_scenes.py -- no image is processed except in the two fused-call cases at the end.  Every comparison is bit-exact against
oracle.stereo_lines run per pair on the first nL / nR rows: matches_12 as integers, disparities as uint32, line equations as uint64.

What the scenes reach that extracted key lines do not: every Config key away from its default (best_lr_matches = 0 among them), both kernels that
fill the distance matrix (k_lines_dist_w up to kDistWaveMaxPairs pairs per call, k_lines_dist above), the stand-alone entries olf_stereo_lines /
olf_stereo_lines_dev / StereoFrontEnd.stereo_lines, end points on the border and in cell column 64 / row 48, 0 / 0 directions, divisions by zero,
exact distance ties, records on the first and last lane of a wave step, and counts 0, 1, 63, 64, 65 and the capacity in one batch.
test_stereo_lines_cpu.py asserts, on the oracle alone, that the scenes do produce these cases."""
import ctypes as C
import numpy as np
import pytest
import orb_line_slam_amd as ola
from orb_line_slam_amd import synth
from orb_line_slam_amd._lib import OLF_OK, OLF_ERR_CAPACITY, lib, ptr
import stereo_line_scenes as S

pytestmark = pytest.mark.gpu
W, H, CAP = S.HAND_W, S.HAND_H, S.CAP
SMALL_W, SMALL_H = 333, 257                    # the size of the 257-pair contexts
N_WAVE = S.dist_wave_max_pairs()               # 256: the largest call k_lines_dist_w serves
SENT_M, SENT_D, SENT_L = -7, 123.0, 7.0


def _params(oracle, ps=None):
    """640 x 480-style contexts: line capacity 160, the smallest ORB side the library builds"""
    p = oracle.full_params(50, CAP, 400.0, 40.0)
    p.orb.nlevels = 1
    return S.apply_params(p, ps or {})


def _front_end(p, w, h, max_pairs):
    fe = ola.StereoFrontEnd(p, w, h, max_pairs=max_pairs)
    assert fe.ctx.line_capacity == CAP
    return fe


_expected = {}


def _expect(oracle, pair, p, w, h, key=None):
    """the oracle's answer for one pair; `key` names pairs that repeat (computed once, never changed)"""
    if key is None or key not in _expected:
        out = oracle.stereo_lines(*pair, w, h, p.stereo)
        for a in out:
            a.setflags(write=False)
        if key is None:
            return out
        _expected[key] = out
    return _expected[key]


def _assert_pair(got, want, i):
    m, disp, le = got
    n = len(want[0])
    assert np.array_equal(m[:n], want[0]), f"pair {i}: matches_12"
    assert np.array_equal(disp[:n].view(np.uint32), want[1].view(np.uint32)), f"pair {i}: disparities"
    assert np.array_equal(le[:n].view(np.uint64), want[2].view(np.uint64)), f"pair {i}: line equations"


def _run_host(fe, pairs):
    """StereoFrontEnd.stereo_lines (olf_stereo_lines) on pairs packed with poisoned rows past each count"""
    kls, ldesc, lcounts = S.pack(pairs, CAP)
    return fe.stereo_lines(kls, ldesc, lcounts)


def _check_host(oracle, fe, pairs, p, w, h, keys=None):
    m, disp, le = _run_host(fe, pairs)
    for i, pair in enumerate(pairs):
        _assert_pair((m[i], disp[i], le[i]), _expect(oracle, pair, p, w, h, None if keys is None else keys[i]), i)
    return m, disp, le


def _default_pairs():
    return [S.cached_scene(S.SEED, *sh, W, H) for sh in S.SHAPES] + S.hand_pairs()


@pytest.fixture(scope="module")
def default_fe(oracle):
    p = _params(oracle)
    return p, _front_end(p, W, H, len(_default_pairs()))


# ---- olf_stereo_lines under the default parameters ------------------------------------------------------------------------------------------------
def test_host_entry_shapes_and_hand_scenes(oracle, default_fe):
    """one batch: the counts 0, 1, 2, 63, 64, 65, 129 and the capacity on either side, then the hand-written scenes with their stated answers"""
    p, fe = default_fe
    pairs = _default_pairs()
    counts = {len(a) for a, _, b, _ in pairs} | {len(b) for a, _, b, _ in pairs}
    assert {0, 1, 2, 63, 64, 65, 129, CAP} <= counts
    m, disp, le = _check_host(oracle, fe, pairs, p, W, H)
    for i, h in enumerate(S.hand_scenes().values(), len(S.SHAPES)):
        n = len(h["m12"])
        assert np.array_equal(m[i, :n], h["m12"])
        if h["disp"] is not None:
            assert np.array_equal(disp[i, :n], h["disp"])


# ---- every Config key away from its default ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", S.PARAM_SETS, ids=S.param_id)
def test_parameter_sweep(oracle, ps):
    p = _params(oracle, ps)
    fe = _front_end(p, W, H, len(S.SWEEP_SHAPES))
    _check_host(oracle, fe, [S.cached_scene(S.SEED, *sh, W, H) for sh in S.SWEEP_SHAPES], p, W, H)


# ---- both kernels that fill the distance matrix ---------------------------------------------------------------------------------------------------------
def _both_kernels(oracle, ps, distinct, tag):
    """one call of kDistWaveMaxPairs + 1 pairs (k_lines_dist) and one of kDistWaveMaxPairs pairs of the same data (k_lines_dist_w): each equals the
    oracle, and the pairs both calls hold are byte-identical over their rows"""
    p = _params(oracle, ps)
    fe = _front_end(p, SMALL_W, SMALL_H, N_WAVE + 1)
    idx = [i % len(distinct) for i in range(N_WAVE + 1)]
    pairs = [distinct[i] for i in idx]
    keys = [(tag, i) for i in idx]
    big = _check_host(oracle, fe, pairs, p, SMALL_W, SMALL_H, keys)
    small = _check_host(oracle, fe, pairs[:N_WAVE], p, SMALL_W, SMALL_H, keys[:N_WAVE])
    rows = np.arange(CAP)[None, :] < np.array([len(a) for a, _, _, _ in pairs[:N_WAVE]])[:, None]
    for a, b in zip(big, small):
        assert np.array_equal(a[:N_WAVE][rows].view(np.uint8), b[rows].view(np.uint8))
    return big


@pytest.mark.parametrize("best_lr", [1, 0])
def test_both_distance_kernels(oracle, best_lr):
    distinct = S.mixed_scenes(SMALL_W, SMALL_H, CAP) + S.hand_pairs(SMALL_W, SMALL_H)
    m, disp, le = _both_kernels(oracle, dict(best_lr_matches=best_lr), distinct, ("mixed", best_lr))
    if best_lr:
        for i, h in enumerate(S.hand_scenes(SMALL_W, SMALL_H).values(), 12):
            assert np.array_equal(m[i, :len(h["m12"])], h["m12"])


def test_block_boundary_both_kernels(oracle):
    """63, 64, 65, 128 and 129 left lines that all reach one right line, distances descending in steps: records on lanes 0 and 63 and on the first lane
    of the next step, and a value equal to the carried minimum that is no record.  The first line with the smallest distance must hold the right line."""
    cases = [(nL, v) for nL in S.STAIR_NL for v in "ab"]
    distinct = [S.staircase(nL, v, SMALL_W, SMALL_H) for nL, v in cases]
    m, disp, le = _both_kernels(oracle, S.STAIR_PARAMS, distinct, "stair")
    for i, (nL, v) in enumerate(cases):
        assert np.flatnonzero(m[i, :nL] >= 0).tolist() == [S.staircase_winner(nL, v)], (nL, v)


# ---- olf_stereo_lines_dev ---------------------------------------------------------------------------------------------------------------------------------
def _dev_call(fe, n_pairs, t, stream):
    return lib().olf_stereo_lines_dev(fe.ctx.handle, n_pairs, *(C.c_void_p(t[k].data_ptr()) for k in ("kls", "ldesc", "lcounts", "m12", "disp", "le")),
                                      C.c_void_p(stream.cuda_stream))


def test_dev_entry_on_a_caller_stream(oracle, default_fe):
    import torch
    p, fe = default_fe
    pairs = _default_pairs()
    n = len(pairs)
    kls, ldesc, lcounts = S.pack(pairs, CAP)
    host = fe.stereo_lines(kls, ldesc, lcounts)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = dict(kls=torch.from_numpy(kls.view(np.uint8).reshape(2 * n, -1)).cuda(), ldesc=torch.from_numpy(ldesc).cuda(), lcounts=torch.from_numpy(lcounts).cuda(),
                 m12=torch.full((n, CAP), SENT_M, dtype=torch.int32, device="cuda"), disp=torch.full((n, CAP, 2), SENT_D, dtype=torch.float32, device="cuda"),
                 le=torch.full((n, CAP, 3), SENT_L, dtype=torch.float64, device="cuda"))
        # n_pairs = 0: OK, nothing written
        assert _dev_call(fe, 0, t, st) == OLF_OK
        st.synchronize()
        assert bool((t["m12"] == SENT_M).all()) and bool((t["disp"] == SENT_D).all()) and bool((t["le"] == SENT_L).all())
        # more pairs than the context holds: the capacity error, nothing launched
        assert _dev_call(fe, n + 1, t, st) == OLF_ERR_CAPACITY and b"olf_stereo_lines_dev" in lib().olf_last_error() and b"max_images" in lib().olf_last_error()
        st.synchronize()
        assert bool((t["m12"] == SENT_M).all())
        assert _dev_call(fe, n, t, st) == OLF_OK
        st.synchronize()
        m, disp, le = t["m12"].cpu().numpy(), t["disp"].cpu().numpy(), t["le"].cpu().numpy()
    fe.ctx.synchronize()
    nL = np.array([len(a) for a, _, _, _ in pairs])
    rows = np.arange(CAP)[None, :] < nL[:, None]
    for a, b in zip((m, disp, le), host):
        assert np.array_equal(a[rows].view(np.uint8), b[rows].view(np.uint8))                 # the host entry's results
    assert (m[~rows] == SENT_M).all() and (disp[~rows] == SENT_D).all() and (le[~rows] == SENT_L).all()      # rows at or past a left count: untouched
    for i, pair in enumerate(pairs):
        _assert_pair((m[i], disp[i], le[i]), _expect(oracle, pair, p, W, H), i)


def test_host_entry_capacity_errors(default_fe):
    """(the device entry cannot see a count: a count above the capacity is the host entry's to refuse, before anything is uploaded)"""
    p, fe = default_fe
    L = lib()
    n = fe.max_pairs
    kls, ldesc, lcounts = S.pack(_default_pairs(), CAP)
    out = np.full((n + 1, CAP), SENT_M, np.int32), np.zeros((n + 1, CAP, 2), np.float32), np.zeros((n + 1, CAP, 3), np.float64)
    call = lambda n_pairs, counts: L.olf_stereo_lines(fe.ctx.handle, n_pairs, ptr(kls), ptr(ldesc), ptr(counts), *(ptr(o) for o in out))
    assert call(n + 1, lcounts) == OLF_ERR_CAPACITY and b"olf_stereo_lines: n_pairs exceeds" in L.olf_last_error()
    for bad in (CAP + 1, -1):
        for where in (0, 2 * n - 1):
            c = lcounts.copy()
            c[where] = bad
            assert call(n, c) == OLF_ERR_CAPACITY and b"olf_stereo_lines: count exceeds capacity" in L.olf_last_error()
    assert (out[0] == SENT_M).all()
    assert call(0, lcounts) == OLF_OK and (out[0] == SENT_M).all()


# ---- the fused call hands p.stereo to the same stage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [dict(best_lr_matches=0), dict(matching_s_ws=3, line_sim_th=0.9)], ids=S.param_id)
def test_fused_call_off_default_parameters(oracle, ps):
    w, h = 320, 240
    p = S.apply_params(oracle.full_params(500, 100, 300.0, 40.0), ps)
    imgs = synth.stereo_batch(11, 1, w, h)
    g = ola.StereoFrontEnd(p, w, h, max_pairs=1).frames(imgs).pair(0)
    ol, orr = oracle.line_extract(imgs[0], p.line), oracle.line_extract(imgs[1], p.line)
    assert np.array_equal(g["mvKeys_Line"], ol["kls"]) and np.array_equal(g["mvKeysRight_Line"], orr["kls"])
    want = oracle.stereo_lines(ol["kls"], ol["desc"], orr["kls"], orr["desc"], w, h, p.stereo)
    _assert_pair((g["line_matches_12"], g["mvDisparity_l"], g["mvle_l"]), want, 0)
    default = oracle.stereo_lines(ol["kls"], ol["desc"], orr["kls"], orr["desc"], w, h, oracle.full_params(500, 100, 300.0, 40.0).stereo)
    assert not np.array_equal(want[0], default[0]) and (want[0] >= 0).sum() >= 20 and (want[1][:, 0] >= 0).sum() >= 5
