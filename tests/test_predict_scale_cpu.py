"""olf_predict_scale_thresholds: MapPoint::PredictScale (src/MapPoint.cc:414-429) as a table of ratios, against the CPU oracle's Frame::isInFrustum.
The level the device predicts is "the number of thresholds <= mfMaxDistance / dist" (csrc/local_batch.hip); here that lookup must equal the level the
oracle computes with its own logf, for random ratios and for every float around every threshold.  No GPU is touched.

The oracle reports a level only for a point inside the frustum, and its distance gate (dist <= 1.2f * mfMaxDistance) rejects ratios below about 0.8333.
Such a ratio is below 1, its logarithm is negative and PredictScale clamps to level 0 whatever the scale factor, so for the rejected points the lookup
is asserted to be 0 (and the rejected points are asserted to be exactly the ones with a ratio below 1)."""
import ctypes as C
import numpy as np
import pytest
import orb_line_slam_amd as ola
from orb_line_slam_amd import matcher
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, OLF_ERR_INVALID

f32 = np.float32
CONFIGS = [(1.2, 8), (1.1, 12), (2.0, 4), (1.05, 16), (1.2, 1)]


def scale_factors(scale, n):
    """mvScaleFactor as ORBextractor::ORBextractor builds it (src/ORBextractor.cc:419-425): a running float product"""
    sf = np.ones(n, f32)
    for i in range(1, n):
        sf[i] = f32(sf[i - 1] * f32(scale))
    return sf


def oracle_levels(oracle, scale, sf, maxd, z):
    """(in view, level) of points on the optical axis at depth z, seen head-on by a camera at the origin"""
    n = len(z)
    world = np.zeros((n, 3), f32)
    world[:, 2] = z
    normal = np.tile(np.array([0, 0, 1], f32), (n, 1))
    mp = ola.MapPointGeom(world, normal, np.ascontiguousarray(maxd, f32), np.zeros(n, f32), np.zeros((n, 32), np.uint8))
    f = ola.FrameView(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), None, sf if len(sf) > 1 else scale_factors(scale, 2), 200.0, 200.0, 160.0,
                      120.0, 40.0, (0.0, 320.0, 0.0, 240.0))
    if len(sf) > 1:
        inv, lvl, _, _ = oracle.is_in_frustum(f, mp, 0.5)
        return inv, lvl
    # one level: oracle.is_in_frustum takes mfLogScaleFactor from mvScaleFactors[1], which such a pyramid does not have; the same oracle function, called
    # with logf(scale) (mfLogScaleFactor = log(mfScaleFactor), src/Frame.cc:150) and nLevels = 1
    a = np.ascontiguousarray
    inv, lvl = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    cosv, proj = np.zeros(n, f32), np.zeros((n, 3), f32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    keep = [a(f.mTcw, f32), oracle._cam(f), a(sf), mp.world, mp.normal, mp.maxd, mp.mind]
    oracle._L.orc_is_in_frustum(p(keep[0]), p(keep[1]), p(keep[2]), 1, oracle._logsf(scale_factors(scale, 2)), n, p(keep[3]), p(keep[4]), p(keep[5]), p(keep[6]),
                                C.c_float(0.5), p(inv), p(lvl), p(cosv), p(proj))
    return inv.astype(bool), lvl


def lookup(thr, ratio):
    return (thr[None, :] <= ratio[:, None]).sum(1).astype(np.int32)


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: "sf%g_n%d" % c)
def config(request):
    scale, n = request.param
    sf = scale_factors(scale, n)
    return scale, sf, matcher.predict_scale_thresholds(sf)


def test_table_shape(config):
    _, sf, thr = config
    assert thr.dtype == np.float32 and len(thr) == len(sf) - 1
    assert np.all(np.diff(thr) > 0) and np.all(thr > 1.0)
    if len(thr):
        assert thr[0].view(np.uint32) == 0x3f800001                     # log(1) = 0 is level 0; the next float is level 1


def test_default_pyramid_thresholds():
    thr = matcher.predict_scale_thresholds(scale_factors(1.2, 8))
    assert [int(x) for x in thr.view(np.uint32)] == [0x3f800001, 0x3f99999b, 0x3fb851ed, 0x3fdd2f1d, 0x4004b5df, 0x401f40a5, 0x403f1a60]


def test_random_ratios(oracle, config):
    scale, sf, thr = config
    rng = np.random.default_rng(17)
    want = np.exp(rng.uniform(np.log(0.05), np.log(50.0), 100000))
    maxd = np.full(len(want), 10.0, f32)
    z = (maxd.astype(np.float64) / want).astype(f32)                      # the point's depth = its distance: sqrt(z * z) is exact
    ratio = maxd / z                                                      # float32 division, as maxd / dist in PredictScale
    inv, lvl = oracle_levels(oracle, scale, sf, maxd, z)
    got = lookup(thr, ratio)
    # in view: ratio >= 1 / 1.2, i.e. ln(50 * 1.2) / ln(50 / 0.05) = 59.3 % of a log-uniform draw
    assert inv.sum() >= 58000 and np.array_equal(got[inv], lvl[inv])
    assert np.all(ratio[~inv] < 1.0) and np.all(got[~inv] == 0)
    assert set(np.unique(lvl[inv])) == set(range(len(sf)))                # every level is met


def test_floats_around_every_threshold(oracle, config):
    scale, sf, thr = config
    base = thr if len(thr) else np.array([1.0, scale], f32)              # (one level: no threshold; the places where a second level would begin)
    bits = (base.view(np.uint32).astype(np.int64)[:, None] + np.arange(-64, 65)[None, :]).reshape(-1).astype(np.uint32)
    ratio = bits.view(f32)
    inv, lvl = oracle_levels(oracle, scale, sf, ratio.copy(), np.ones(len(ratio), f32))      # dist = 1: maxd / dist is the ratio itself
    assert inv.all()
    assert np.array_equal(lookup(thr, ratio), lvl)
    if not len(thr):
        assert not lvl.any()
        return
    k = np.arange(len(thr))
    assert np.array_equal(lvl.reshape(len(thr), 129)[:, 63], k) and np.array_equal(lvl.reshape(len(thr), 129)[:, 64], k + 1)      # the step is at the threshold


def test_bad_arguments():
    with pytest.raises(ola.OlfError) as e:
        matcher.predict_scale_thresholds(np.array([1.0, 1.0, 1.0], f32))
    assert e.value.code == OLF_ERR_INVALID
    with pytest.raises(ola.OlfError):
        matcher.predict_scale_thresholds(np.array([1.0, 0.8], f32))
    with pytest.raises(ola.OlfError):
        matcher.predict_scale_thresholds(scale_factors(1.2, 17))            # above OLF_MAX_LEVELS
