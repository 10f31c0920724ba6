"""Constructed key lines for Frame::ComputeStereoMatches_Lines (src/Frame.cc:878-1000), shared by test_stereo_lines_cpu.py and
test_stereo_lines_gpu.py.  No image is involved: the matcher reads four end-point fields of each key line and a 32-byte descriptor, so a
scene is two arrays of KEYLINE_DTYPE records (every other field zero) and two (n, 32) uint8 arrays.  Nothing here touches a device.

  scene(seed, nL, nR, W, H)   seeded random scene: each left line draws one of the KINDS below, its right line is derived from it
  hand_scenes(W, H)           tiny scenes whose answer a reader can check by eye (written at 640 x 480: a grid cell is 10 x 10 pixels)
  staircase(nL, variant, ..)  nL left lines against one right line that all of them reach; the Hamming distances descend in steps
  border_scene(W, H)          key lines on the image border (x == W and y == H included), any image size
  PARAM_SETS                  the off-default Config values the tests sweep

The grid is 64 x 48 cells over the image.  A right line is a candidate of a left line when it crosses the grid row of the left start
point or end point in one of the matching_s_ws + 1 cells ending at that point's cell (GridStructure::get with no vertical extent)."""
import os
import re
import numpy as np
from orb_line_slam_amd._lib import KEYLINE_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GC, GR = 64, 48
KINDS = ("plain", "horizontal", "vertical", "short", "clipped", "cell_boundary", "no_jitter", "right_reversed", "right_horizontal", "right_duplicate",
         "left_neighbour")
# (nL, nR) of the random scenes both test files run; CAP is the line capacity of the contexts (lsd_nfeatures)
CAP = 160
SHAPES = ((160, 160), (65, 129), (129, 63), (64, 64), (1, 160), (160, 1), (2, 2), (0, 5), (5, 0))
SWEEP_SHAPES = ((160, 160), (65, 129), (129, 63))
SEED = 20

# Config values away from the defaults (matching_s_ws 10, line_sim_th 0.75, min_ratio_12_l 0.9, min_disp 1, line_horiz_th 0.1, stereo_overlap_th 0.75,
# ls_min_disp_ratio 0.7, best_lr_matches 1).  min_ratio_12_l stays below 1: at or above 1 the reference's answer depends on unordered_set order.
# The last set is there for the infinite disparities alone: an exactly horizontal right line overlaps a left line's rows by 0, and 0 > stereo_overlap_th
# needs a negative threshold (line_horiz_th cannot open that gate: it closes the |sp_l.y - ep_l.y| > line_horiz_th gate with the same number).
PARAM_SETS = (
    dict(best_lr_matches=0), dict(matching_s_ws=0), dict(matching_s_ws=64), dict(line_sim_th=0.0), dict(line_sim_th=0.99), dict(min_ratio_12_l=0.5),
    dict(min_ratio_12_l=0.99), dict(min_disp=0.0), dict(min_disp=20.0), dict(line_horiz_th=5.0), dict(stereo_overlap_th=0.0), dict(stereo_overlap_th=0.95),
    dict(ls_min_disp_ratio=0.0), dict(ls_min_disp_ratio=0.95), dict(conv_eigen_recip=1), dict(best_lr_matches=0, matching_s_ws=64, line_sim_th=0.0),
    dict(stereo_overlap_th=-1.0),
)


def param_id(ps):
    return "-".join(f"{k}={v}" for k, v in ps.items())


def apply_params(p, ps):
    """p: OlfParams; sets p.stereo's fields from one of PARAM_SETS and returns p"""
    for k, v in ps.items():
        setattr(p.stereo, k, v)
    return p


def dist_wave_max_pairs():
    """kDistWaveMaxPairs of csrc/line_internal.hpp: calls of up to this many pairs run k_lines_dist_w, larger ones k_lines_dist"""
    text = open(os.path.join(ROOT, "orb_line_slam_amd", "csrc", "line_internal.hpp")).read()
    return int(re.search(r"constexpr\s+int\s+kDistWaveMaxPairs\s*=\s*(\d+)\s*;", text).group(1))


def keylines(seg):
    """KEYLINE_DTYPE records from rows of (startPointX, startPointY, endPointX, endPointY); the matcher reads nothing else"""
    seg = np.asarray(seg, np.float64).reshape(-1, 4)
    k = np.zeros(len(seg), KEYLINE_DTYPE)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3]
    return k


def segs_of(kls):
    return np.stack([kls["startPointX"], kls["startPointY"], kls["endPointX"], kls["endPointY"]], 1)


def grid_segs(kls, W, H):
    """the doubles the reference hands to getLineCoords: float end point times double (cells / size)"""
    s = segs_of(kls).astype(np.float64)
    return np.ascontiguousarray(s * np.array([GC / float(W), GR / float(H), GC / float(W), GR / float(H)]))


def bits(n, offset=0):
    """a descriptor with n bits set, the first at bit `offset`: the distance between bits(a) and bits(b) is |a - b|"""
    d = np.zeros(32, np.uint8)
    for b in range(offset, offset + n):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def flip(rng, d, k):
    d = d.copy()
    for b in rng.choice(256, k, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


# ---- the random scene ----------------------------------------------------------------------------------------------------------------------------
def scene(seed, nL, nR, W, H):
    """(klL, descL, klR, descR).  max(nL, nR) left lines are drawn, each of one of KINDS, and a right line is derived from each; the left side keeps
    the first nL, the right side the first nR, permuted.  All coordinates stay within [-W/4, 5W/4] x [-H/4, 5H/4]."""
    rng = np.random.default_rng(seed)
    n = max(nL, nR)
    cw, ch = W / GC, H / GR
    L, R = np.zeros((n, 4)), np.zeros((n, 4))
    dL, dR = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8)
    kinds = rng.integers(0, len(KINDS), n)
    for i in range(n):
        kind = KINDS[kinds[i]]
        if i == 0 and kind in ("right_duplicate", "left_neighbour"):
            kind = "plain"
        # the left line
        sx, sy = rng.uniform(-0.1 * W, 1.1 * W), rng.uniform(-0.1 * H, 1.1 * H)
        ang, ln = rng.uniform(-np.pi, np.pi), rng.uniform(1.5 * max(cw, ch), 0.25 * W)
        ex, ey = sx + ln * np.cos(ang), sy + ln * np.sin(ang)
        if kind == "horizontal":
            ey = sy
        elif kind == "vertical":
            ex = sx
        elif kind == "short":                                      # both end points in one cell more often than not: a 0 / 0 direction
            ln = rng.uniform(0.05, 0.9) * min(cw, ch)
            ex, ey = sx + ln * np.cos(ang), sy + ln * np.sin(ang)
        elif kind == "clipped":                                    # the extractor clips end points onto the image: x == W and y == H occur
            far = rng.integers(0, 4)
            ex += (0.6 * W, 0.0, -0.6 * W, 0.0)[far]
            ey += (0.0, 0.6 * H, 0.0, -0.6 * H)[far]
            sx, ex, sy, ey = np.clip(sx, 0, W), np.clip(ex, 0, W), np.clip(sy, 0, H), np.clip(ey, 0, H)
        elif kind == "cell_boundary":
            sx, ex = cw * np.clip(np.rint(sx / cw), 0, GC), cw * np.clip(np.rint(ex / cw), 0, GC)
            sy, ey = ch * np.clip(np.rint(sy / ch), 0, GR), ch * np.clip(np.rint(ey / ch), 0, GR)
        elif kind == "right_horizontal":                           # a shallow left line inside one grid row; the right line lies above it in the same row
            row = rng.integers(1, GR - 1)
            sx = rng.uniform(0.3 * W, 0.9 * W)
            ex = sx + rng.uniform(3 * cw, 8 * cw)
            sy = (row + rng.uniform(0.35, 0.5)) * ch
            ey = sy + rng.uniform(0.15, 0.4) * ch
        elif kind == "left_neighbour":                             # beside the previous left line, descriptor one bit away: two left lines want one right line
            off = rng.uniform(-2, 2, 4)
            sx, sy, ex, ey = L[i - 1] + off
        L[i] = np.clip(sx, -0.2 * W, 1.2 * W), np.clip(sy, -0.2 * H, 1.2 * H), np.clip(ex, -0.2 * W, 1.2 * W), np.clip(ey, -0.2 * H, 1.2 * H)
        sx, sy, ex, ey = L[i]
        dL[i] = flip(rng, dL[i - 1], 1) if kind == "left_neighbour" else rng.integers(0, 256, 32, dtype=np.uint8)
        # the right line: shifted left by a disparity, the end point by another factor, jittered; descriptor 0 - 59 bits away
        s = W / 640.0
        disp = (0.0, 0.5, 1.0, rng.uniform(1, 60) * s, rng.uniform(60, 140) * s)[rng.integers(0, 5)]
        fac = 1.0 if rng.random() < 0.5 else rng.uniform(0.5, 1.5)
        jx, jy = (0.0, 0.0) if kind == "no_jitter" else (1.5, 0.3)
        R[i] = (sx - disp + rng.uniform(-jx, jx), sy + rng.uniform(-jy, jy), ex - disp * fac + rng.uniform(-jx, jx), ey + rng.uniform(-jy, jy))
        dR[i] = flip(rng, dL[i], int(rng.integers(0, 60)))
        if kind == "right_reversed":
            R[i] = R[i][[2, 3, 0, 1]]
        elif kind == "right_horizontal":
            R[i, 1] = R[i, 3] = (row + rng.uniform(0.05, 0.25)) * ch
        elif kind == "right_duplicate":                            # the previous right line and descriptor again: an exact tie for its left line
            R[i], dR[i] = R[i - 1], dR[i - 1]
    R[:, [0, 2]] = np.clip(R[:, [0, 2]], -0.25 * W, 1.25 * W)
    perm = rng.permutation(nR)
    klL, klR = keylines(L[:nL]), keylines(R[:nR][perm])
    for k in (klL, klR):
        s = segs_of(k)
        assert (s[:, [0, 2]] >= -0.25 * W).all() and (s[:, [0, 2]] <= 1.25 * W).all() and (s[:, [1, 3]] >= -0.25 * H).all() and (s[:, [1, 3]] <= 1.25 * H).all()
    return klL, np.ascontiguousarray(dL[:nL]), klR, np.ascontiguousarray(dR[:nR][perm])


def scene_kinds(seed, n):
    """the kind drawn for each left line of scene(seed, ...) with max(nL, nR) == n"""
    kinds = np.random.default_rng(seed).integers(0, len(KINDS), n)
    out = [KINDS[k] for k in kinds]
    if out and out[0] in ("right_duplicate", "left_neighbour"):
        out[0] = "plain"
    return out


_scenes = {}


def cached_scene(seed, nL, nR, W, H):
    key = (seed, nL, nR, W, H)
    if key not in _scenes:
        _scenes[key] = scene(*key)
    return _scenes[key]


# ---- hand-written scenes, default parameters -----------------------------------------------------------------------------------------------------
# Written for 640 x 480, where a grid cell is 10 x 10 pixels; hand_scenes(W, H) scales the coordinates to another image size, which keeps every end
# point in its cell (none lies on a cell boundary, except those on the image border).  Each scene: left segments and descriptors, right segments and
# descriptors, the expected matches_12 and, where it is exact at 640 x 480, the expected disparities.
HAND_W, HAND_H = 640, 480
_HAND = {
    # one candidate only: the second-best distance stays INT_MAX and any distance passes the ratio test; the right line is the left one 20 px
    # to the left, so both disparities are exactly 20
    "single_candidate": ([(300, 105, 360, 135)], [bits(200)], [(280, 105, 340, 135)], [bits(0)], [0], [(20, 20)]),
    # the best distance twice (right 0 and 1 are both 10 away): 10 < 10 * 0.9 fails.  Left 1, far away, has right 2 to itself
    "best_twice": ([(300, 105, 360, 135), (100, 305, 160, 335)], [bits(10), bits(40)],
                   [(280, 105, 340, 135), (270, 105, 330, 135), (80, 305, 140, 335)], [bits(0), bits(20), bits(41)], [-1, 2], [(-1, -1), (20, 20)]),
    # left 0 and 1 both reach right 0 alone; the later one is strictly better (10 < 20) and takes it, the earlier one loses the mutual check
    "later_better": ([(300, 105, 360, 135), (302, 106, 362, 136)], [bits(20), bits(10)], [(280, 105, 340, 135)], [bits(0)], [-1, 0], None),
    # ... and when the later one only equals the earlier one's distance it is no new record: the earlier one keeps the right line
    "later_equal": ([(300, 105, 360, 135), (302, 106, 362, 136)], [bits(20), bits(20, 20)], [(280, 105, 340, 135)], [bits(0)], [0, -1], None),
    # the start point's window (row 10, cells 0..10) is empty, the end point's (row 30, cells 30..40) holds the short right line
    "end_window_only": ([(100, 105, 400, 305)], [bits(7)], [(370, 300, 395, 308)], [bits(0)], [0], None),
    # the right line crosses the whole image (its last cell (64, 48) is outside the grid).  Left 0 and 2 lie 30 px right of it, left 1 far from it;
    # left 2 comes later and is worse (15 > 10), so left 0 keeps the line
    "diagonal": ([(130, 75, 230, 150), (500, 50, 600, 125), (560, 405, 639, 464)], [bits(10), bits(1), bits(15)], [(0, 0, 640, 480)], [bits(0)],
                 [0, -1, -1], None),
    # the left end point x == W lands in cell column 64, one past the grid: its window is cells 54..63 of row 23, where the right line lies
    "column_64": ([(590, 200, 640, 232)], [bits(3)], [(600, 226, 630, 238)], [bits(0)], [0], None),
    # vertical lines, the left one in cell column 30.  Right 0 (column 31) is one cell right of the window, right 1 (column 20) is its first cell,
    # right 2 (column 19) one cell left of it: right 1 is the only candidate although right 0 and 2 are closer in descriptor
    "window_ends": ([(305, 100, 305, 200)], [bits(20)], [(315, 100, 315, 200), (205, 100, 205, 200), (195, 100, 195, 200)],
                    [bits(15), bits(0), bits(17)], [1], [(100, 100)]),
}


def hand_scenes(W=HAND_W, H=HAND_H):
    """{name: dict(klL, descL, klR, descR, m12, disp or None)} with the coordinates scaled from 640 x 480 to W x H"""
    sc = np.array([W / HAND_W, H / HAND_H, W / HAND_W, H / HAND_H])
    out = {}
    for name, (left, dl, right, dr, m12, disp) in _HAND.items():
        exact = disp is not None and (W, H) == (HAND_W, HAND_H)
        out[name] = dict(klL=keylines(np.array(left, np.float64) * sc), descL=np.array(dl, np.uint8).reshape(-1, 32),
                         klR=keylines(np.array(right, np.float64) * sc), descR=np.array(dr, np.uint8).reshape(-1, 32), m12=np.array(m12, np.int32),
                         disp=np.array(disp, np.float32) if exact else None)
    return out


def hand_pairs(W=HAND_W, H=HAND_H):
    return [(h["klL"], h["descL"], h["klR"], h["descR"]) for h in hand_scenes(W, H).values()]


# ---- the block-boundary scene ------------------------------------------------------------------------------------------------------------------------
STAIR_NL = (63, 64, 65, 128, 129)
STAIR_PARAMS = dict(matching_s_ws=64, line_sim_th=0.0)


def staircase_distances(nL, variant):
    """Hamming distance of left line i to the one right line.  The values descend in steps of five lines with a higher value thrown in, so most
    lines only equal the running minimum.  Line 63 of every 64 is a new record (the last lane of a wave step); the line after it (lane 0 of the next
    step) is a record too in variant "a" and equals the carried minimum -- no record -- in variant "b"."""
    cur, out = 230, []
    for i in range(nL):
        if i % 64 == 63:
            cur -= 1
        elif i % 64 == 0 and i > 0:
            cur -= 1 if variant == "a" else 0
        elif i % 5 == 0 and i > 0:
            cur -= 1
        out.append(cur + 3 if i % 7 == 3 else cur)
    return np.array(out, np.int32)


def staircase_winner(nL, variant):
    """the left line that holds the right line in the end: the first one with the smallest distance"""
    return int(np.argmin(staircase_distances(nL, variant)))


def staircase(nL, variant, W, H):
    """(klL, descL, klR, descR): parallel horizontal lines in grid row 20; with STAIR_PARAMS every left line reaches the right line"""
    y = 20.5 * H / GR
    x = np.linspace(0.1 * W, 0.6 * W, nL)
    left = np.stack([x, np.full(nL, y), x + 0.2 * W, np.full(nL, y)], 1)
    dl = np.stack([bits(int(d)) for d in staircase_distances(nL, variant)])
    return keylines(left), dl, keylines([(0.02 * W, y, 0.98 * W, y)]), bits(0).reshape(1, 32)


# ---- key lines on the border ----------------------------------------------------------------------------------------------------------------------------
def border_scene(W, H):
    """(klL, descL, klR, descR) of lines along and onto the four borders of a W x H image, x == W and y == H included, with a right line 3 px to the
    left of each (clipped to the image like the left one)"""
    m = [(0, 0, W, 0), (0, H, W, H), (0, 0, 0, H), (W, 0, W, H), (0.4 * W, H, 0.7 * W, 0.8 * H), (W, 0.3 * H, 0.8 * W, 0.5 * H), (0.5 * W, 0, 0.6 * W, 0.3 * H),
         (0, 0.5 * H, 0.2 * W, 0.7 * H), (W, H, 0.7 * W, 0.7 * H), (0, 0, 0.3 * W, 0.2 * H), (0.9 * W, 0.9 * H, W, H), (W, 0.5 * H, W - 2, 0.5 * H + 1)]
    L = np.array(m, np.float64)
    R = L.copy()
    R[:, [0, 2]] = np.clip(R[:, [0, 2]] - 3.0, 0, W)
    R[:, [1, 3]] += np.array([0.2, -0.2])
    R[:, [1, 3]] = np.clip(R[:, [1, 3]], 0, H)
    rng = np.random.default_rng(W * 1000 + H)
    dl = rng.integers(0, 256, (len(L), 32), dtype=np.uint8)
    dr = np.stack([flip(rng, d, 5) for d in dl])
    perm = rng.permutation(len(L))
    return keylines(L), dl, keylines(R[perm]), np.ascontiguousarray(dr[perm])


# ---- inputs of tests/golden/stereo_line_edges.npz ---------------------------------------------------------------------------------------------------
EDGE_KINDS = ("vertical", "short", "clipped", "cell_boundary")
EDGE_WS = (0, 10, 64)


def edge_inputs():
    """(line cases [n, 4] in grid units, [(right segments in grid units, queries [m, 5] = (spx, spy, epx, epy, ws))]): the border, cell-boundary, steep and
    clipped lines of the scenes above as the reference's getLineCoords and GridStructure::get see them"""
    klL, _, klR, _ = cached_scene(SEED, CAP, CAP, HAND_W, HAND_H)
    edge = np.flatnonzero(np.isin(scene_kinds(SEED, CAP), EDGE_KINDS))
    hs = hand_scenes()
    cases = [grid_segs(klL[edge], HAND_W, HAND_H), grid_segs(hs["diagonal"]["klR"], HAND_W, HAND_H), grid_segs(hs["column_64"]["klL"], HAND_W, HAND_H)]
    trials = []

    def queries(kl, W, H):
        c = np.trunc(grid_segs(kl, W, H)).astype(np.int64)           # (int) of the scaled end points: towards zero
        return np.concatenate([np.concatenate([c, np.full((len(c), 1), ws)], 1) for ws in EDGE_WS])
    trials.append((grid_segs(klR, HAND_W, HAND_H), queries(klL[edge], HAND_W, HAND_H)))
    for W, H in ((HAND_W, HAND_H), (333, 257)):
        bl, _, br, _ = border_scene(W, H)
        cases += [grid_segs(bl, W, H), grid_segs(br, W, H)]
        trials.append((grid_segs(br, W, H), queries(bl, W, H)))
    return np.concatenate(cases), trials


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------------------
POISON = 0xA7


def pack(pairs, cap):
    """pairs: [(klL, descL, klR, descR)] -> (kls [2n, cap], ldesc [2n, cap, 32], lcounts [2n]) as olf_stereo_lines reads them; the rows past each
    count hold poison bytes, so a kernel that reads past a count changes its answer"""
    n = len(pairs)
    kls = np.frombuffer(np.full(2 * n * cap * KEYLINE_DTYPE.itemsize, POISON, np.uint8).tobytes(), KEYLINE_DTYPE).reshape(2 * n, cap).copy()
    ldesc = np.full((2 * n, cap, 32), POISON, np.uint8)
    lcounts = np.zeros(2 * n, np.int32)
    for i, (a, da, b, db) in enumerate(pairs):
        assert len(a) <= cap and len(b) <= cap
        kls[2 * i, :len(a)], ldesc[2 * i, :len(a)], lcounts[2 * i] = a, da, len(a)
        kls[2 * i + 1, :len(b)], ldesc[2 * i + 1, :len(b)], lcounts[2 * i + 1] = b, db, len(b)
    return kls, ldesc, lcounts


def mixed_scenes(W, H, cap, n=12, seed=300):
    """n distinct scenes of mixed counts at W x H (the counts 0, 1, 63, 64, 65 and the capacity among them)"""
    shapes = [(cap, cap), (65, 129), (129, 63), (64, 64), (1, cap), (cap, 1), (2, 2), (0, 5), (5, 0), (63, 65), (100, 37), (17, cap)]
    return [cached_scene(seed + i, min(a, cap), min(b, cap), W, H) for i, (a, b) in enumerate(shapes[:n])]
