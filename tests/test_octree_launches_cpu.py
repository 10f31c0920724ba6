"""The launches of k_octree as the library itself derives them (olf_debug_octree_launches: host only, the function launch_orb_octree launches from).

At the flagship shape -- 1242 x 375, 2000 features, 8 levels, scale 1.2 -- no launch may ask for more than 36 KB of LDS, so that one workgroup fits beside the
24 LSD growth agents of 5120 B that share a CU's 160 KB with it in the fused frame call, and the launch of the levels 3 to 7 for no more than 18 KB, so that
two fit.  The other cases pin the grouping: one, two and three launches, the 64 KB opt-in range, and the configuration whose lists live in global memory."""
import ctypes as C
import numpy as np
import pytest
from orb_line_slam_amd import _lib


def launches(nfeatures, nlevels, w, h, scale=1.2):
    p = _lib.default_params().orb
    p.nfeatures, p.scale_factor, p.nlevels = nfeatures, scale, nlevels
    level_launch, lds = np.full(nlevels, -1, np.int32), np.zeros(3, np.int32)
    n = _lib.lib().olf_debug_octree_launches(C.byref(p), w, h, _lib.ptr(level_launch), _lib.ptr(lds))
    assert n >= 1, n
    assert (lds[n:] == -1).all() and set(level_launch.tolist()) == set(range(n))
    return level_launch.tolist(), lds[:n].tolist()


def test_flagship_launches_fit_beside_the_growth_agents():
    levels, lds = launches(2000, 8, 1242, 375)
    assert levels == [0, 0, 0, 1, 1, 1, 1, 1]
    assert 18 * 1024 < lds[0] <= 36 * 1024 and lds[1] <= 18 * 1024
    assert lds == [62 * 448 + 4 * 512, 62 * 264 + 4 * 256]          # quotas 434 and 251: capacity quota + 8 rounded up to 8, sort keys the next power of two
    assert lds[0] + 24 * 5120 <= 160 * 1024 and 2 * lds[1] + 24 * 5120 <= 160 * 1024


@pytest.mark.parametrize("nfeatures,nlevels,w,h,levels,lds", [
    (1000, 8, 320, 240, [0] * 8, None),                              # every level at most 18 KB: one launch
    (1500, 8, 320, 240, [0, 0, 1, 1, 1, 1, 1, 1], None),             # quotas 326, 271 | 226, ...: 256 is the last quota of the small group
    (3000, 8, 320, 240, [0, 0, 1, 1, 1, 1, 2, 2], None),             # quotas 651, 543 | 452, 377, 314, 262 | 218, 183
    (1771, 1, 203, 141, [0], [62 * 1784 + 4 * 2048]),                # 116 KB: above what a launch gets unasked, below the 160 KB
    (2500, 1, 320, 240, [0], [0]),                                   # more than 2048 nodes: the lists live in global memory
])
def test_grouping(nfeatures, nlevels, w, h, levels, lds):
    got_levels, got_lds = launches(nfeatures, nlevels, w, h)
    assert got_levels == levels
    assert got_lds == sorted(got_lds, reverse=True)
    if lds is not None:
        assert got_lds == lds
    if len(got_lds) == 3:
        assert got_lds[0] > 36 * 1024 >= got_lds[1] > 18 * 1024 >= got_lds[2]
    assert all(b <= 160 * 1024 - 64 for b in got_lds)


def test_bad_arguments():
    p = _lib.default_params().orb
    out = np.zeros(16, np.int32)
    assert _lib.lib().olf_debug_octree_launches(None, 640, 480, _lib.ptr(out), _lib.ptr(out)) == _lib.OLF_ERR_INVALID
    p.nlevels = 8
    assert _lib.lib().olf_debug_octree_launches(C.byref(p), 128, 106, _lib.ptr(out), _lib.ptr(out)) == _lib.OLF_ERR_INVALID      # the top level is too small
