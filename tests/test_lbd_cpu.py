"""The constructed LBD scenes (tests/lbd_scenes.py) take the oracle where tests/test_lbd_gpu.py needs it: into the NaN path, onto both sides of
every branch of the device kernels, and onto descriptors that a kernel sampling one pixel off would change.  No device here."""
import ctypes
import functools
import numpy as np
import pytest
import lbd_scenes as S

CASES = [(seed, W, H) for (W, H) in S.SIZES for seed in S.SEEDS]
KI = {name: i for i, name in enumerate(S.KINDS)}


@functools.lru_cache(maxsize=None)
def _scene(seed, W, H):
    return S.scene(seed, W, H)


@functools.lru_cache(maxsize=None)
def _run(seed, W, H, image_kind, libm_float=0, gauss_sum256=0):
    import oracle_lib
    kls, _ = _scene(seed, W, H)
    return oracle_lib.lbd_compute(S.image(image_kind, W, H, seed), kls, want_float=True, libm_float=libm_float, gauss_sum256=gauss_sum256)


def _popcount(d):
    return np.unpackbits(d, axis=1).sum(1)


@pytest.mark.parametrize("seed,W,H", CASES)
def test_nan_rows_are_where_they_are_expected(oracle, seed, W, H):
    kls, kind = _scene(seed, W, H)
    dead = S.short_len(kls) <= 0                                 # no sample at all: 0 * (1 / sqrt(0))
    assert dead.sum() == 3
    for ik in S.IMAGE_KINDS:
        d, f = _run(seed, W, H, ik)
        nan = np.isnan(f).any(1)
        assert (d[nan] == 0).all(), ik                           # a NaN compares false everywhere
        if ik in ("noise", "sinusoids", "steps"):
            assert np.array_equal(nan, dead), ik
        elif ik == "flat":
            assert nan.all()
        elif (W, H) in ((131, 64), (64, 203)):                   # the ramp: sqrt of a cancelled E[x^2] - E[x]^2 that came out negative
            assert (nan & ~dead).sum() >= 1 and not nan.all()


@pytest.mark.parametrize("seed,W,H", CASES)
@pytest.mark.parametrize("image_kind", ("noise", "sinusoids"))
def test_descriptors_are_rich_and_feel_a_one_pixel_shift(oracle, seed, W, H, image_kind):
    kls, kind = _scene(seed, W, H)
    d, f = _run(seed, W, H, image_kind)
    ok = ~np.isnan(f).any(1)
    bits = _popcount(d[ok]).mean()
    assert 96 <= bits <= 160, bits
    ds = oracle.lbd_compute(S.image(image_kind, W, H, seed), S.shifted(kls, 1))
    changed = (d != ds).any(1)[ok].mean()
    assert changed >= 0.9, changed


@pytest.mark.parametrize("seed,W,H", CASES)
def test_far_rows_have_descriptors_that_depend_on_the_wrap(oracle, seed, W, H):
    kls, kind = _scene(seed, W, H)
    far = kind == KI["far"]
    assert far.sum() >= 8
    # every far row has samples beyond the (short) cast's range
    mid = np.maximum(np.abs(kls["sPointInOctaveX"] + kls["ePointInOctaveX"]), np.abs(kls["sPointInOctaveY"] + kls["ePointInOctaveY"])) / 2
    assert (mid[far] + kls["numOfPixels"][far] / 2 + 32 > 32767).all() and (mid[~far] < 1000).all()
    for ik in ("noise", "sinusoids", "steps"):
        d, f = _run(seed, W, H, ik)
        assert not np.isnan(f[far]).any(), ik
        assert (_popcount(d[far]) > 0).all(), ik
    # clamping the coordinate to the near edge instead of wrapping it (the lean form of k_lbd_rows) gives other descriptors: move each far line to the
    # pixel the clamp would pick and compare
    d, _ = _run(seed, W, H, "noise")
    k = kls[far].copy()
    for a, b, n in (("sPointInOctaveX", "ePointInOctaveX", W), ("sPointInOctaveY", "ePointInOctaveY", H)):
        m = (k[a] + k[b]) / 2
        sh = np.where(m > 30000, (n + 100) - m, np.where(m < -30000, -100 - m, 0)).astype(np.float32)
        k[a], k[b] = k[a] + sh, k[b] + sh
    dc = oracle.lbd_compute(S.image("noise", W, H, seed), k)
    assert (dc != d[far]).any(1).sum() >= 6


@pytest.mark.parametrize("seed,W,H", CASES)
def test_every_branch_is_drawn(seed, W, H):
    kls, kind = _scene(seed, W, H)
    assert set(kind.tolist()) == set(range(len(S.KINDS)))
    assert len(kls) <= 256                                       # the capacity test_lbd_gpu.py gives its contexts
    flat = S.flat_side(kls)
    assert flat.sum() >= 20 and (~flat).sum() >= 20
    fp = kind == KI["flat_predicate"]
    assert flat[fp].any() and (~flat[fp]).any()                  # ... also among the lines one float either side of a diagonal
    lens = set(S.short_len(kls).tolist())
    for m in (16, 32, 48, 64):                                   # the 16-sample step of k_lbd_rows and its tail mask
        assert {m - 1, m, m + 1} <= lens, m
    assert {1, 2, 3} <= lens and min(lens) < 0 and 0 in lens and max(lens) > 4000
    assert {200, 0, -3, 40000, 70000} <= set(kls["numOfPixels"][kind == KI["bad_num"]].tolist())
    # exact k + 0.5 sample chains: axis-aligned, even length, integer end points; negative ties from the lines that start at (-0.5, -0.5)
    ax = kls[kind == KI["axis"]]
    half = ((ax["sPointInOctaveX"] + ax["ePointInOctaveX"]) % 2 == 1) | ((ax["sPointInOctaveY"] + ax["ePointInOctaveY"]) % 2 == 1)
    assert half.sum() >= 16 and (~half).sum() >= 16
    for c in ("sPointInOctaveX", "sPointInOctaveY"):
        assert (ax[c] == 0).any() and (ax[c] == 1).any()
    assert (ax["ePointInOctaveX"] == W - 1).any() and (ax["ePointInOctaveY"] == H - 1).any()
    assert set(ax["angle"].tolist()) == {0.0, float(S.PI), float(S.HPI), float(-S.HPI)}
    out = kls[kind == KI["outside"]]
    assert ((out["sPointInOctaveX"] == -0.5) & (out["sPointInOctaveY"] == -0.5)).sum() >= 3
    ang = np.abs(kls["angle"][kind == KI["angles"]])
    assert (ang > np.pi).sum() >= 8 and ang.max() < 120 and (ang < 2.0 ** -12).sum() >= 3 and (ang == np.float32(2.0 ** -12)).any()
    assert np.isfinite(kls["angle"]).all() and max(np.abs(kls[c]).max() for c in ("sPointInOctaveX", "sPointInOctaveY", "ePointInOctaveX", "ePointInOctaveY")) < 1e6


def test_the_convention_runs_change_descriptors(oracle):
    """conv_libm_float and conv_gauss_sum256 must each change descriptors of the rows test_lbd_gpu.py runs under them (the angle and the axis kinds over
    every size, image kind and seed), or those runs would prove nothing.  The taps change the gradient images, so nearly every row moves; the float
    overloads change a bit only where a comparison was a near tie, so their count is pooled."""
    libm = ctypes.CDLL("libm.so.6")
    for fn in (libm.cosf, libm.sinf):
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    n_libm = n_both = 0
    for seed, W, H in CASES:
        kls, kind = _scene(seed, W, H)
        ang = kind == KI["angles"]
        a = kls["angle"][ang]
        # the direction vector itself differs between the two conventions for some of the angles
        assert sum(np.float32(libm.cosf(float(x))) != np.float32(np.cos(float(x))) or np.float32(libm.sinf(float(x))) != np.float32(np.sin(float(x))) for x in a) >= 3
        for ik in S.IMAGE_KINDS:
            d, _ = _run(seed, W, H, ik)
            d1, _ = _run(seed, W, H, ik, 1, 0)
            d2, _ = _run(seed, W, H, ik, 0, 1)
            d3, _ = _run(seed, W, H, ik, 1, 1)
            n_libm += int((d1 != d)[ang].any(1).sum())
            n_both += int((d3 != d2)[ang].any(1).sum())
            if ik != "flat":
                assert (d2 != d)[ang].any(1).sum() >= 1, (seed, W, H, ik)
    assert n_libm >= 1 and n_both >= 1, (n_libm, n_both)
