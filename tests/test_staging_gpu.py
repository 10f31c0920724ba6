"""The host-pointer entries share two scratch slabs of a context, which every call cuts anew (csrc/staging.hpp): one context, one sequence of calls in
which the slab is cut small, grows, stays grown and is cut again by entries of other shapes -- empty arrays, one element, odd counts that leave the next
region at a padded offset -- each result against a numpy computation made here (Hamming distances from np.unpackbits)."""
import numpy as np
import pytest

from orb_line_slam_amd import _lib, matcher, precond
from orb_line_slam_amd._lib import AREA_QUERY_DTYPE, GRID_CELLS, GRID_ROWS, KEYPOINT_DTYPE, lib, ptr

pytestmark = pytest.mark.gpu

INT_MAX = 0x7fffffff


def _ham(a, b):
    """(len(a), len(b)) Hamming distances of 256-bit rows: |a| + |b| - 2 a.b over the unpacked bits (exact in float32: every term is at most 256)"""
    A, B = np.unpackbits(a, axis=1).astype(np.float32), np.unpackbits(b, axis=1).astype(np.float32)
    return (A.sum(1)[:, None] + B.sum(1)[None, :] - 2 * (A @ B.T)).astype(np.int32)


def _knn2(q, t):
    """best index (the lowest among equals), best and second-best distance per query; -1 / INT_MAX where the train set has none"""
    n = len(q)
    idx, d0, d1 = np.full(n, -1, np.int32), np.full(n, INT_MAX, np.int32), np.full(n, INT_MAX, np.int32)
    if len(t):
        D = _ham(q, t)
        order = np.argsort(D, axis=1, kind="stable")
        idx = order[:, 0].astype(np.int32)
        d0 = D[np.arange(n), idx]
        if len(t) > 1:
            d1 = D[np.arange(n), order[:, 1]]
    return idx, d0, d1


def test_scratch_is_recut_as_it_grows_and_stays_grown():
    rng = np.random.default_rng(2024)
    desc = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ctx = _lib.Context(_lib.default_params(), 640, 480, 2)
    try:
        def knn2(nq, nt, what):
            q, t = desc(nq), desc(nt)
            if nt >= 2:
                t[1] = t[0]; q[0] = t[0]                                 # equal rows: distance 0 twice, the lower index wins
            got, want = matcher.knn2(q, t, context=ctx), _knn2(q, t)
            for g, w, name in zip(got, want, ("idx0", "dist0", "dist1")):
                assert np.array_equal(g, w), (what, name)

        knn2(1, 1, "first cut")
        knn2(300, 4096, "regrowth")
        knn2(5, 0, "empty train set")
        knn2(1, 7, "small again")

        # olf_match_candidates: three queries with 0, 1 and 2 candidates -- three candidates in all, so the distances start at a padded offset
        q, t = desc(3), desc(4)
        offs, cand = np.array([0, 0, 1, 3], np.int32), np.array([2, 3, 0], np.int32)
        dist = np.full(3, 0xffff, np.uint16)
        assert lib().olf_match_candidates(ctx.handle, ptr(q), 3, ptr(t), 4, ptr(offs), ptr(cand), ptr(dist)) == 0
        D = _ham(q, t)
        assert np.array_equal(dist, np.array([D[1, 2], D[2, 3], D[2, 0]], np.uint16))

        a, b = desc(3), desc(5)
        assert np.array_equal(matcher.distance_matrix(a, b, context=ctx), _ham(a, b).astype(np.uint16))

        # one landmark nobody observes, one with three observations: the row whose median distance to all three (itself included) is least, the first of equals
        obs = desc(3)
        med = np.sort(_ham(obs, obs), axis=1)[:, int(0.5 * (3 - 1))]
        best = matcher.ComputeDistinctiveDescriptors([np.zeros((0, 32), np.uint8), obs], context=ctx)
        assert np.array_equal(best, [-1, int(np.argmin(med))])

        # Frame::mGrid of one key: PosInGrid rounds (x - minX) * (64 / (maxX - minX)) in float
        bounds = (0.0, 640.0, 0.0, 480.0)
        key = np.zeros(1, KEYPOINT_DTYPE)
        key["x"], key["y"], key["size"], key["class_id"] = 101.0, 52.0, 31.0, -1
        wInv, hInv = np.float32(64) / np.float32(640), np.float32(48) / np.float32(480)
        cell = int(np.round(np.float32(101) * wInv)) * GRID_ROWS + int(np.round(np.float32(52) * hInv))
        want_offs = (np.arange(GRID_CELLS + 1) > cell).astype(np.int32)
        cell_offs, cell_idx = np.full(GRID_CELLS + 1, -1, np.int32), np.full(1, -1, np.int32)
        assert lib().olf_frame_grid(ctx.handle, ptr(key), 1, *bounds, ptr(cell_offs), ptr(cell_idx)) == 0
        assert np.array_equal(cell_offs, want_offs) and np.array_equal(cell_idx, [0])

        # Frame::GetFeaturesInArea, one query on that grid: the key is inside the window iff |dx| < r and |dy| < r
        query = np.zeros(1, AREA_QUERY_DTYPE)
        query["x"], query["y"], query["r"], query["min_level"], query["max_level"] = 100.0, 50.0, 5.0, -1, -1
        inside = bool(abs(np.float32(101) - np.float32(100)) < 5 and abs(np.float32(52) - np.float32(50)) < 5)
        cand_offs, cand_idx = np.full(2, -1, np.int32), np.full(1, -1, np.int32)
        assert lib().olf_features_in_area(ctx.handle, ptr(key), 1, ptr(cell_offs), ptr(cell_idx), *bounds, 1, ptr(query), ptr(cand_offs), ptr(cand_idx), 1) == 0
        assert inside and np.array_equal(cand_offs, [0, 1]) and np.array_equal(cand_idx, [0])

        # cvtColor(RGB2GRAY) of one image: (4899 R + 9617 G + 1868 B + 2^13) >> 14
        rgb = rng.integers(0, 256, (1, 480, 640, 3), dtype=np.uint8)
        c = rgb.astype(np.int64)
        gray = ((c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + (1 << 13)) >> 14).astype(np.uint8)
        assert np.array_equal(precond.cvtColor(rgb, precond.RGB2GRAY, context=ctx), gray)

        knn2(1, 1, "after everything else")
    finally:
        ctx.close()
