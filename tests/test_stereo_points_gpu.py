"""GPU parity of Frame::ComputeStereoMatches on constructed key points and image patches (tests/stereo_point_scenes.py): the four kernels of
csrc/match.hip behind olf_stereo_points_dev against the CPU oracle, bit for bit.  The images go through olf_orb_extract_dev (which leaves the pyramids in
the context); the key point, descriptor and count buffers are then overwritten with the scene (StereoFrontEnd.stereo_points_on)."""
import numpy as np
import pytest
import orb_line_slam_amd as ola
from orb_line_slam_amd._lib import KEYPOINT_DTYPE
import stereo_point_scenes as S

pytestmark = pytest.mark.gpu
FILL = -7.0


@pytest.fixture(scope="module")
def front_ends():
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = ola.StereoFrontEnd(S.params(), w, h, max_pairs=6)
            assert made[(w, h)].ctx.orb_capacity == S.capacity()
        return made[(w, h)]
    return get


def _run(fe, scenes):
    """one olf_stereo_points_dev call over the scenes as the pairs of a batch; every pair must equal the oracle and leave what lies past its count alone"""
    cap, n = fe.ctx.orb_capacity, len(scenes)
    imgs = np.stack([s[k] for s in scenes for k in ("imgL", "imgR")])
    kps, desc, counts = np.zeros((2 * n, cap), KEYPOINT_DTYPE), np.zeros((2 * n, cap, 32), np.uint8), np.zeros(2 * n, np.int32)
    for i, s in enumerate(scenes):
        nL, nR = len(s["kpsL"]), len(s["kpsR"])
        kps[2 * i, :nL], desc[2 * i, :nL] = s["kpsL"], s["descL"]
        kps[2 * i + 1, :nR], desc[2 * i + 1, :nR] = s["kpsR"], s["descR"]
        # past the right count: the left points themselves (same row, disparity 0, descriptor distance 0) -- they would win every search if read
        extra = min(cap - nR, nL)
        kps[2 * i + 1, nR:nR + extra], desc[2 * i + 1, nR:nR + extra] = s["kpsL"][:extra], s["descL"][:extra]
        counts[2 * i], counts[2 * i + 1] = nL, nR
    ur, dp = fe.stereo_points_on(imgs, kps, desc, counts, fill=FILL)
    for i, s in enumerate(scenes):
        nL, o = len(s["kpsL"]), S.oracle_answer(s)
        assert np.array_equal(ur[i, :nL].view(np.uint32), o["uRight"].view(np.uint32)), (s["name"], np.flatnonzero(ur[i, :nL] != o["uRight"])[:8])
        assert np.array_equal(dp[i, :nL].view(np.uint32), o["depth"].view(np.uint32)), s["name"]
        assert (ur[i, nL:] == FILL).all() and (dp[i, nL:] == FILL).all(), s["name"]
    return ur, dp


def test_kind_scenes(front_ends):
    scenes = S.kind_scenes()
    small = [s for s in scenes if (s["w"], s["h"]) == (S.W, S.H)]
    assert len(small) == len(scenes) - 1
    for s in scenes:                                   # each alone, then the 320 x 240 ones as one batch
        _run(front_ends(s["w"], s["h"]), [s])
    _run(front_ends(S.W, S.H), small)
    assert sum(int((S.oracle_answer(s)["uRight"] >= 0).sum()) for s in scenes) > 100


@pytest.mark.parametrize("k", range(len(S.SHAPES) + 1))
def test_shape_scenes(front_ends, k):
    _run(front_ends(S.W, S.H), [S.shape_scenes()[k]])


def test_six_shapes_in_one_call(front_ends):
    _run(front_ends(S.W, S.H), S.shape_scenes()[:6])


def test_hand_scenes(front_ends):
    hs = S.hand_scenes()
    ur, dp = _run(front_ends(S.W, S.H), [h[0] for h in hs[:6]])
    for i, (s, want_u, want_d) in enumerate(hs[:6]):
        n = len(want_u)
        assert np.array_equal(ur[i, :n].view(np.uint32), want_u.view(np.uint32)) and np.array_equal(dp[i, :n].view(np.uint32), want_d.view(np.uint32)), s["name"]


def test_nothing_stale_after_a_full_scene(front_ends):
    fe = front_ends(S.W, S.H)
    _run(fe, [S.full_scene()] * 2)
    _run(fe, [S.kind_scenes()[3], S.shape_scenes()[2]])       # one median point; (1, 1)
    _run(fe, [S.shape_scenes()[0]])                           # no left point at all


def test_capacity_edge_of_the_lds_sorts(oracle):
    """more than 16384 key points per image: the row sort and the median sort ask for 128 KB of dynamic LDS (launch_stereo_points raises the limit)"""
    w, h = 640, 480
    p = oracle.full_params(20000, 100, S.FX, S.BF)
    fe = ola.StereoFrontEnd(p, w, h, max_pairs=1)
    cap = fe.ctx.orb_capacity
    assert 16384 < cap <= 32768
    imgL, imgR, kL, dL, kR, dR = S.big_scene(w, h, cap)
    ur, dp = fe.stereo_points_on(np.stack([imgL, imgR]), np.stack([kL, kR]), np.stack([dL, dR]), np.array([cap, cap], np.int32), fill=FILL)
    o = oracle.stereo_match_keys(imgL, imgR, p, kL, dL, kR, dR)
    assert (o["uRight"] >= 0).sum() > cap // 2 and ((o["sad"] >= 0) & (o["uRight"] < 0)).sum() > cap // 20      # matches kept, and matches the median filter dropped
    assert np.array_equal(ur[0].view(np.uint32), o["uRight"].view(np.uint32)) and np.array_equal(dp[0].view(np.uint32), o["depth"].view(np.uint32))
