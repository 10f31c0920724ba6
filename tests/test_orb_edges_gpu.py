"""GPU parity of the ORB extractor at small, odd, wide and off-default settings: every scene of tests/orb_edge_scenes.py against the CPU oracle, bit-exact
and stage by stage (pyramid, candidate lists, blurred levels, key points, descriptors), so that a mismatch names the first broken stage.  What each scene
reaches (resize kernel, cell sort path, octree branch, threshold extreme) is asserted on the oracle by tests/test_orb_edges_cpu.py.

Not covered: more than 256 survivors in one FAST cell (the third size of k_cells_sort's LDS sort).  Noise gives at most 190 in a cell of these scenes and a
contrived image was not built for it."""
import ctypes as C
import numpy as np
import pytest
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib
import orb_edge_scenes as S

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


def _bits(a):
    return a.view(np.uint32) if a.dtype.kind == "f" else a


def _compare(gk, gd, ok, od):
    assert len(gk) == len(ok), (len(gk), len(ok))
    for f in FIELDS:
        assert np.array_equal(_bits(gk[f]), _bits(ok[f])), f
    assert np.array_equal(gd, od)


@pytest.mark.parametrize("name", list(S.SCENES))
def test_scene_matches_oracle(oracle, name):
    s = S.SCENES[name]
    o = S.oracle_run(oracle, name)
    ex = ola.ORBextractor(s.nfeatures, s.scale, s.nlevels, s.ini, s.min, max_images=1)
    gk, gd = ex(o["image"])
    gw, gh = ex.level_sizes()
    assert list(zip(gw.tolist(), gh.tolist())) == o["sizes"]
    for l in range(s.nlevels):
        assert np.array_equal(ex.pyramid_level(l), o["pyramid"][l]), f"pyramid level {l}"
    for l in range(s.nlevels):
        assert np.array_equal(ex.debug_candidates(l), o["candidates"][l]), f"candidates level {l}"
    for l in range(s.nlevels):
        if o["blurred"][l].any():
            assert np.array_equal(ex.pyramid_level(l, blurred=True), o["blurred"][l]), f"blur level {l}"
    assert len(gk) == len(o["kps"]), f"returned count {len(gk)}, oracle {len(o['kps'])}"
    _compare(gk, gd, o["kps"], o["desc"])


def test_batch_of_three_odd_images(oracle):
    """three different 131 x 97 images in one call: an odd row length and image stride on the way in, each image equal to its own single-image oracle run"""
    imgs = np.stack([S.noise(201, 131, 97), S.low_contrast(202, 131, 97), S.noise(203, 131, 97)])
    ex = ola.ORBextractor(200, 1.2, 3, 20, 7, max_images=3)
    kps, desc, counts = ex.extract_batch(imgs)
    p = oracle.orb_params(200, 1.2, 3, 20, 7)
    for i in range(3):
        o = oracle.orb_extract(imgs[i], p, debug=True)
        for l in range(3):
            assert np.array_equal(ex.pyramid_level(l, image=i), o["pyramid"][l]), f"image {i} pyramid level {l}"
            assert np.array_equal(ex.debug_candidates(l, image=i), o["candidates"][l]), f"image {i} candidates level {l}"
        n = int(counts[i])
        assert n == len(o["kps"]) > 0
        _compare(kps[i, :n], desc[i, :n], o["kps"], o["desc"])


def test_strided_region_of_a_larger_image(oracle):
    """olf_orb_extract_strided on a 131 x 97 region of a 160 x 110 image (rows 160 bytes apart, the first pixel at an odd address): what the adaptor does for
    a cv::Mat whose step is not its width.  Equal to the oracle on a contiguous copy of the region."""
    big = S.noise(204, 160, 110)
    roi = big[5:102, 17:148]
    assert roi.shape == (97, 131) and roi.strides == (160, 1) and not roi.flags["C_CONTIGUOUS"]
    p = _lib.default_params()
    p.orb.nfeatures, p.orb.scale_factor, p.orb.nlevels, p.orb.ini_th_fast, p.orb.min_th_fast = 200, 1.2, 3, 20, 7
    ctx = _lib.Context(p, 131, 97, 1)
    kps, desc, n = np.zeros(ctx.orb_capacity, _lib.KEYPOINT_DTYPE), np.zeros((ctx.orb_capacity, 32), np.uint8), C.c_int32()
    try:
        rc = _lib.lib().olf_orb_extract_strided(ctx.handle, C.c_void_p(roi.ctypes.data), C.c_size_t(roi.strides[0]), _lib.ptr(kps), _lib.ptr(desc), C.byref(n))
        assert rc == _lib.OLF_OK, _lib.last_error()
        # a row stride smaller than the width is refused
        assert _lib.lib().olf_orb_extract_strided(ctx.handle, C.c_void_p(roi.ctypes.data), C.c_size_t(130), _lib.ptr(kps), _lib.ptr(desc), C.byref(n)) == _lib.OLF_ERR_INVALID
    finally:
        ctx.close()
    o = oracle.orb_extract(np.ascontiguousarray(roi), oracle.orb_params(200, 1.2, 3, 20, 7))
    assert n.value == len(o["kps"]) > 0
    _compare(kps[:n.value], desc[:n.value], o["kps"], o["desc"])


@pytest.mark.parametrize("w,h,nlevels,says", [(128, 106, 4, "62 x 62"),       # the top level is 74 x 61
                                              (4132, 96, 1, "4131"),
                                              (4200, 4132, 1, "4131")])
def test_context_creation_refuses(w, h, nlevels, says):
    """refused on the host, before anything is allocated or launched; the accepted neighbours 128 x 107 and 4131 x 96 are the scenes min_level and widest"""
    p = _lib.default_params()
    p.orb.nfeatures, p.orb.scale_factor, p.orb.nlevels = 100, 1.2, nlevels
    h_ctx = C.c_void_p()
    assert _lib.lib().olf_ctx_create(C.byref(p), w, h, 1, C.byref(h_ctx)) == _lib.OLF_ERR_INVALID
    assert not h_ctx.value
    assert says in _lib.last_error()
