"""GPU parity of the ORB extractor where k_octree's per-level working set matters: the kernel sizes its LDS lists by the level it processes (62 bytes per
node of the level's key point capacity, 4 per key of the careful rounds' sort) and launch_orb_octree puts the levels into up to three launches by that size
(at most 18 KB, at most 36 KB, larger).  Key points and descriptors must equal the CPU oracle's bit for bit.

What the cases reach is asserted on the oracle's per-level candidate counts and on the sizes restated below:
  * a level with 0, with 1, with exactly its quota and with more than its quota of candidates;
  * levels of one case in one, two and all three launch groups;
  * nlevels 1, 3 and 8;
  * a level's lists above 64 KB (the opt-in attribute) and above 2048 nodes (the instance that keeps its lists in global memory)."""
import ctypes as C
import functools
import numpy as np
import pytest
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib
import orb_edge_scenes as S

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
SMALL, LARGE = (203, 141), (320, 240)


def dots(w, h, pts):
    """3 x 3 bright squares on a flat image: the upper pyramid levels see one FAST corner each, the lower ones none"""
    img = np.full((h, w), 90, np.uint8)
    for x, y in pts:
        img[y - 1:y + 2, x - 1:x + 2] = 250
    return img


IMAGES = {
    "noise_small": lambda: S.noise(301, *SMALL),
    "low_small": lambda: S.low_contrast(302, *SMALL),
    "noise_large": lambda: S.noise(301, *LARGE),
    "low_large": lambda: S.low_contrast(302, *LARGE),
    "dot1_large": lambda: dots(*LARGE, [(160, 120)]),
    "dot3_large": lambda: dots(*LARGE, [(60, 50), (100, 70), (150, 90)]),
}

# name: (image, nfeatures or None = the level-0 candidate count, nlevels, launch groups its levels fall into)
CASES = {
    "one_candidate_levels":  ("dot1_large", 1000, 8, {0}),          # candidates per level 0, 0, 1, 1, 1, 1, 1, 1
    "few_candidate_levels":  ("dot3_large", 1000, 8, {0}),          # 0, 1, 3, 3, 3, 3, 2, 2
    "exact_quota_small":     ("low_small", None, 1, {0}),           # 102 candidates, quota 102
    "exact_quota_64k":       ("noise_small", None, 1, {2}),         # 1771 candidates, quota 1771: 116 KB of lists, above the 64 KB a launch gets unasked
    "over_quota_3_levels":   ("noise_small", 1000, 3, {1}),         # quotas 396, 330, 274 against 1771, 998, 525 candidates
    "under_quota_3_levels":  ("low_small", 2400, 3, {2}),           # level 0 has 102 candidates for a quota of 949
    "straddle_18k":          ("noise_large", 1500, 8, {0, 1}),      # quotas 326, 271 | 226, 188, ...: 256 is the last quota of the 18 KB group
    "three_groups":          ("noise_large", 3000, 8, {0, 1, 2}),   # quotas 651, 543 | 452, 377, 314, 262 | 218, 183
    "low_contrast_8_levels": ("low_large", 2000, 8, {0, 1}),        # upper levels run out of candidates
    "spill":                 ("noise_large", 2500, 1, {2}),         # up to 2503 nodes: more than the 2048 whose lists fit the LDS
}


@functools.lru_cache(maxsize=None)
def _image(name):
    return IMAGES[name]()


@functools.lru_cache(maxsize=None)
def _candidates(oracle, image, nlevels):
    """candidates per level: they do not depend on nfeatures"""
    o = oracle.orb_extract(_image(image), oracle.orb_params(100, 1.2, nlevels, 20, 7), debug=True, cap=8192)
    return tuple(len(c) for c in o["candidates"])


def _lds_bytes(quota, n_ini):
    """octree_lds_bytes of a level, as olf_internal.hpp states it"""
    cap = (max(quota + 8, 4 * n_ini + 4) + 7) & ~7
    sort = 64
    while sort < quota:
        sort *= 2
    return 62 * cap + 4 * sort, cap


def _group(nbytes):
    return 0 if nbytes <= 18 * 1024 else (1 if nbytes <= 36 * 1024 else 2)


@functools.lru_cache(maxsize=None)
def _run(oracle, name):
    image, nfeatures, nlevels, _ = CASES[name]
    if nfeatures is None:
        nfeatures = _candidates(oracle, image, nlevels)[0]
    p = oracle.orb_params(nfeatures, 1.2, nlevels, 20, 7)
    o = oracle.orb_extract(_image(image), p, cap=nfeatures + 4096)
    quotas = oracle.orb_tables(p)[4].tolist()
    lw, lh = oracle.orb_level_sizes(p, _image(image).shape[1], _image(image).shape[0])
    sizes = [_lds_bytes(q, S.n_ini(int(w), int(h))) for q, w, h in zip(quotas, lw, lh)]
    return nfeatures, quotas, sizes, o


def test_cases_reach_what_they_are_named_for(oracle):
    seen = set()
    for name, (image, _, nlevels, groups) in CASES.items():
        _, quotas, sizes, _ = _run(oracle, name)
        cand = _candidates(oracle, image, nlevels)
        assert {_group(b) for b, _ in sizes} == groups, (name, sizes)
        for c, q in zip(cand, quotas):
            seen.add("0" if c == 0 else "1" if c == 1 else "exact" if c == q else "over" if c > q else "under")
    assert seen == {"0", "1", "exact", "over", "under"}
    assert {CASES[n][2] for n in CASES} == {1, 3, 8}
    big = _run(oracle, "exact_quota_64k")[2][0]
    assert 64 * 1024 < big[0] <= 160 * 1024 - 64 and big[1] <= 2048
    assert _run(oracle, "spill")[2][0][1] > 2048 and _candidates(oracle, "noise_large", 1)[0] > 2500
    # the restatement above against the library's own launches (tests/test_octree_launches_cpu.py pins those at the flagship shape)
    for name in CASES:
        image, _, nlevels, _ = CASES[name]
        nfeatures, _, sizes, _ = _run(oracle, name)
        p = _lib.default_params().orb
        p.nfeatures, p.scale_factor, p.nlevels = nfeatures, 1.2, nlevels
        level_launch, lds = np.zeros(nlevels, np.int32), np.zeros(3, np.int32)
        n = _lib.lib().olf_debug_octree_launches(C.byref(p), _image(image).shape[1], _image(image).shape[0], _lib.ptr(level_launch), _lib.ptr(lds))
        if name == "spill":
            assert n == 1 and lds[0] == 0
            continue
        groups = sorted({_group(b) for b, _ in sizes}, reverse=True)
        assert n == len(groups)
        for l, (b, _) in enumerate(sizes):
            assert groups[level_launch[l]] == _group(b) and lds[level_launch[l]] >= b
        assert sorted(lds[:n].tolist()) == sorted(max(b for b, _ in sizes if _group(b) == g) for g in groups)


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_oracle(oracle, name):
    image, _, nlevels, _ = CASES[name]
    nfeatures, _, _, o = _run(oracle, name)
    ex = ola.ORBextractor(nfeatures, 1.2, nlevels, 20, 7, max_images=1)
    gk, gd = ex(_image(image))
    assert len(gk) == len(o["kps"]), (len(gk), len(o["kps"]))
    for f in FIELDS:
        a, b = gk[f], o["kps"][f]
        assert np.array_equal(a.view(np.uint32) if a.dtype.kind == "f" else a, b.view(np.uint32) if b.dtype.kind == "f" else b), f
    assert np.array_equal(gd, o["desc"])


def test_batch_mixes_empty_and_full_levels(oracle):
    """three different images in one call (the octree grid is levels x images): each equal to its own oracle run"""
    names = ("noise_large", "dot3_large", "low_large")
    ex = ola.ORBextractor(1500, 1.2, 8, 20, 7, max_images=3)
    kps, desc, counts = ex.extract_batch(np.stack([_image(n) for n in names]))
    p = oracle.orb_params(1500, 1.2, 8, 20, 7)
    for i, n in enumerate(names):
        o = oracle.orb_extract(_image(n), p)
        c = int(counts[i])
        assert c == len(o["kps"])
        for f in FIELDS:
            a, b = kps[i, :c][f], o["kps"][f]
            assert np.array_equal(a.view(np.uint32) if a.dtype.kind == "f" else a, b.view(np.uint32) if b.dtype.kind == "f" else b), (n, f)
        assert np.array_equal(desc[i, :c], o["desc"]), n
