"""Scenes for olf_create_new_map_points*, olf_compute_f12* and olf_update_normal_and_depth*: key-frame pairs drawn from one pool of 3-D points seen from poses
with translations of 0.05 to 1 m and rotations up to 5 degrees, fabricated at 320 x 240 as tests/test_triangulation_batch_gpu.py fabricates its frames, with
pixel noise, wrong matches, far points and random octaves so that the branches of the loop occur; and map snapshots with observation rows of chosen
lengths.  Every candidate match is run through the restatement (tests/newpoints_reference.py) three times -- `base` and the two switched SVDs -- and is
KEPT only when the three agree on its code, every gate that depends on x3D has a relative margin of at least 1e-3 and every cosine comparison an absolute
margin of at least 1e-5 (64 float ulps of 1: each side carries a few ulps from atan2f / cosf; the x3D bound is checked rather than derived, the gates being
conditioned by the triangulation).  A row of a pair is the first n kept matches in idx1 order."""
import functools
import math
import types
import numpy as np
import newpoints_reference as R
from orb_line_slam_amd._lib import KEYPOINT_DTYPE

F = np.float32
W, H = 320, 240
FX = FY = 200.0
CX, CY = 160.0, 120.0
MBF = 40.0
MB = float(F(MBF) / F(FX))
CAM5 = (FX, FY, CX, CY, MBF)
X3D_MARGIN, COS_MARGIN = 1e-3, 1e-5
ROW_COUNTS = (0, 1, 63, 64, 65, 300)
POOL = 420


def scale_factors(n=8):
    sf = np.ones(n, F)
    for i in range(1, n):
        sf[i] = F(float(sf[i - 1]) * float(F(1.2)))
    return sf


SF = scale_factors()
RATIO_FACTOR = F(1.5) * SF[1]


# Camera centres: consecutive frames 0.23 to 0.8 m apart -- just above mb = 0.2 m, so that the parallax of a stereo point is sometimes below its stereo
# angle (UnprojectStereo) and sometimes above (triangulation) -- and frame 3 well in front of frame 2, so that near points lie behind it (z2 <= 0)
CENTRES = ((0, 0, 0), (0.25, 0.02, 0), (0.5, 0.05, 0.05), (0.5, 0.1, 0.8), (0.7, 0.05, 0.65), (0.22, -0.05, 0.05))


def _rotation(rng, max_deg):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = math.radians(rng.uniform(0, max_deg))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def make_frames(n_frames, seed):
    """n_frames views of the pool: feature i of frame j observes point perm_j[i]"""
    rng = np.random.default_rng(seed)
    far = rng.random(POOL) < 0.12
    near = ~far & (rng.random(POOL) < 0.1)                            # (in front of one key frame and behind the next that moved forward: z2 <= 0)
    Z = np.where(far, rng.uniform(150, 900, POOL), np.where(near, rng.uniform(0.15, 0.6, POOL), rng.uniform(1.5, 25, POOL)))
    X = (rng.uniform(30, 290, POOL) - CX) / FX * Z
    Y = (rng.uniform(20, 220, POOL) - CY) / FY * Z
    pts = np.stack([X, Y, Z], 1)
    frames = []
    for j in range(n_frames):
        fr = types.SimpleNamespace()
        Rm = _rotation(rng, 5.0) if j else np.eye(3)
        t = -Rm @ np.array(CENTRES[j])
        fr.Tcw = np.eye(4, dtype=F)
        fr.Tcw[:3, :3], fr.Tcw[:3, 3] = Rm.astype(F), t.astype(F)
        fr.obs = rng.permutation(POOL)
        pc = pts[fr.obs] @ Rm.T + t
        noise = rng.choice([0.0, 0.0, 0.2, 0.6, 1.5, 4.0], (POOL, 2)) * rng.normal(size=(POOL, 2))
        k = np.zeros(POOL, KEYPOINT_DTYPE)
        k["x"] = (FX * pc[:, 0] / pc[:, 2] + CX + noise[:, 0]).astype(F)
        k["y"] = (FY * pc[:, 1] / pc[:, 2] + CY + noise[:, 1]).astype(F)
        k["octave"], k["size"], k["class_id"] = rng.integers(0, 8, POOL), 31, -1
        fr.keys = k
        fr.depth = (pc[:, 2] * rng.choice([1.0, 1.0, 1.02, 0.97], POOL)).astype(F)
        stereo = (rng.random(POOL) < 0.55) & (fr.depth > 0)
        fr.uright = np.where(stereo, k["x"] - F(MBF) / fr.depth, -1.0).astype(F)
        fr.depth = np.where(stereo, fr.depth, -1.0).astype(F)
        frames.append(fr)
    return frames


def feature(fr, i):
    k = fr.keys[i]
    return (F(k["x"]), F(k["y"]), F(fr.uright[i]), F(fr.depth[i]), SF[int(k["octave"])])


def evaluate(fr1, fr2, i1, i2):
    """the restatement's three runs of one match: (base code, base x3D or None, [alt x3D ...], kept)"""
    cam = tuple(F(v) for v in CAM5)
    P1, P2 = R.kf_pose(fr1.Tcw), R.kf_pose(fr2.Tcw)
    k1, k2 = feature(fr1, i1), feature(fr2, i2)
    code, x, mg = R.create_point(P1, P2, cam, MB, RATIO_FACTOR, k1, k2, "base")
    kept = mg.cos >= COS_MARGIN and mg.x3d >= X3D_MARGIN
    alts = []
    for svd in ("f32", "rev"):
        c, xa, ma = R.create_point(P1, P2, cam, MB, RATIO_FACTOR, k1, k2, svd)
        kept = kept and c == code and ma.cos >= COS_MARGIN and ma.x3d >= X3D_MARGIN
        alts.append(xa)
    return code, x, alts, kept


def make_row(frames, a, b, n, seed):
    """n kept matches of the pair (a, b): (row [POOL] of idx2 or -1, {idx1: (code, x3D, alts)}); one candidate in seven is a wrong match"""
    rng = np.random.default_rng(seed)
    fr1, fr2 = frames[a], frames[b]
    where2 = np.argsort(fr2.obs)                                     # point -> feature of frame 2
    row, ref = np.full(POOL, -1, np.int32), {}
    for i1 in range(POOL):
        if len(ref) == n:
            break
        i2 = int(where2[fr1.obs[i1]]) if rng.random() > 1 / 7 else int(rng.integers(0, POOL))
        code, x, alts, kept = evaluate(fr1, fr2, i1, i2)
        if kept:
            row[i1], ref[i1] = i2, (code, x, alts)
    assert len(ref) == n, (a, b, n, len(ref))
    return row, ref


@functools.lru_cache(maxsize=None)
def scene_set():
    """six frames and one row per ROW_COUNTS entry, pair p = (p, (p + 1) % 6) -- and its reverse with 65 matches: computed once"""
    frames = make_frames(6, 11)
    pairs = [(p, (p + 1) % 6) for p in range(6)] + [(3, 1)]
    counts = list(ROW_COUNTS) + [65]
    rows, refs = [], []
    for p, ((a, b), n) in enumerate(zip(pairs, counts)):
        row, ref = make_row(frames, a, b, n, 100 + p)
        rows.append(row)
        refs.append(ref)
    return types.SimpleNamespace(frames=frames, pairs=pairs, rows=rows, refs=refs)


def code_histogram(refs):
    h = {}
    for ref in refs:
        for code, _, _ in ref.values():
            h[code] = h.get(code, 0) + 1
    return h


def batch_arrays(frames, cap, img_stride=1):
    """the frames as the host arrays of olf_track_batch: rows nothing may read hold octave 99, uright 5 and depth 7"""
    nf = len(frames)
    kps = np.zeros((nf * img_stride, cap), KEYPOINT_DTYPE)
    kps["octave"] = 99
    cnt = np.full(nf * img_stride, 17, np.int32)
    ur, depth, Tcw = np.full((nf, cap), 5.0, F), np.full((nf, cap), 7.0, F), np.zeros((nf, 4, 4), F)
    for j, fr in enumerate(frames):
        m = len(fr.keys)
        kps[j * img_stride, :m], cnt[j * img_stride] = fr.keys, m
        ur[j, :m], depth[j, :m], Tcw[j] = fr.uright, fr.depth, fr.Tcw
    return kps, cnt, ur, depth, Tcw


def match_rows(rows, cap, fill=-1):
    out = np.full((len(rows), cap), fill, np.int32)
    for p, r in enumerate(rows):
        out[p, :len(r)] = r
    return out


# ---- the tolerance rule for triangulated points (tests/pose_scenes.py within_rule, restated) ----------------------------------------------------------
def within_rule(got, base, alts):
    """|got - base| <= 16 x the spread of the switched runs around base, with a floor of 64 float ulp of the point's largest coordinate.  Returns (ok, ratio),
    ratio = difference / max(spread, floor / 16): ok means ratio <= 16."""
    base = np.array([float(v) for v in base])
    got = np.asarray(got, np.float64)
    if not np.all(np.isfinite(got)):
        return False, math.inf
    spread = max(float(np.max(np.abs(np.array([float(v) for v in a]) - base))) for a in alts)
    floor = 64.0 * float(np.finfo(np.float32).eps) * float(np.max(np.abs(base)))
    unit = max(spread, floor / 16.0)
    diff = float(np.max(np.abs(got - base)))
    if unit == 0.0:
        return diff == 0.0, 0.0 if diff == 0.0 else math.inf
    return diff <= 16.0 * unit, diff / unit


def check_rows(x3D, code, nnew, refs, at=None):
    """codes and nnew exactly, x3D of the codes 2 / 3 bit for bit, x3D of code 1 by the rule; everything else 0.  Returns the largest ratio of the rule."""
    worst = 0.0
    for p, ref in enumerate(refs):
        q = p if at is None else at[p]
        exp = np.zeros(code.shape[1], np.uint8)
        for i1, (c, _, _) in ref.items():
            exp[i1] = c
        assert np.array_equal(code[q], exp), (q, np.flatnonzero(code[q] != exp)[:8], code[q][code[q] != exp][:8], exp[code[q] != exp][:8])
        assert nnew[q] == sum(c in R.CREATED for c, _, _ in ref.values()), q
        made = np.isin(exp, R.CREATED)
        assert not x3D[q][~made].any(), q
        for i1, (c, x, alts) in ref.items():
            if c in (R.UNPROJECT_1, R.UNPROJECT_2):
                assert np.array_equal(x3D[q, i1].view(np.uint32), np.array(x, np.float32).view(np.uint32)), (q, i1, x3D[q, i1], x)
            elif c == R.TRIANGULATED:
                ok, ratio = within_rule(x3D[q, i1], x, alts)
                worst = max(worst, ratio)
                assert ok, (q, i1, x3D[q, i1], x, ratio)
    return worst


# ---- map snapshots for UpdateNormalAndDepth --------------------------------------------------------------------------------------------------------------
OBS_LENGTHS = (0, 1, 2, 63, 64, 65, 300)


def snapshot(seed, n_kf=320, slots=24, lengths=OBS_LENGTHS, extra=40):
    """A map of n_kf key frames of `slots` features each and one point per entry of `lengths` plus `extra` points of 3 to 12 observations.  Rows ascend
    (C.15) except for every fifth extra point, whose row is shuffled; the reference key frame is in the row except for every seventh extra point (the slot-0
    quirk); point 3 is bad.  Returns a namespace with the plain lists MapGraph / CullView take and the arrays of the entry."""
    rng = np.random.default_rng(seed)
    lens = list(lengths) + [int(v) for v in rng.integers(3, 13, extra)]
    n_mp = len(lens)
    s = types.SimpleNamespace(n_kf=n_kf, n_mp=n_mp, slots=slots)
    s.kf_Ow = rng.uniform(-3, 3, (n_kf, 3)).astype(F)
    s.mp_world = (rng.uniform(-4, 4, (n_mp, 3)) + np.array([0, 0, 12.0])).astype(F)
    s.octave = rng.integers(0, 8, (n_kf, slots))
    s.mp_obs, s.mp_obs_slot, s.ref_kf = [], [], np.zeros(n_mp, np.int32)
    for p, n in enumerate(lens):
        kfs = np.sort(rng.choice(n_kf, n, replace=False))
        if p >= len(lengths) and (p - len(lengths)) % 5 == 4:
            kfs = rng.permutation(kfs)
        s.mp_obs.append([int(v) for v in kfs])
        s.mp_obs_slot.append([int(v) for v in rng.integers(0, slots, n)])
        outside = p >= len(lengths) and (p - len(lengths)) % 7 == 6
        others = np.setdiff1d(np.arange(n_kf), kfs)
        s.ref_kf[p] = int(rng.choice(others)) if outside or n == 0 else int(rng.choice(kfs))
    s.mp_bad = np.zeros(n_mp, np.uint8)
    s.mp_bad[3] = 1
    s.outside = [p for p in range(n_mp) if lens[p] and s.ref_kf[p] not in s.mp_obs[p]]
    return s


def snapshot_graph(s):
    """(MapGraph, CullView) of a snapshot: slot i of a key frame holds no point (the entry reads no kf_mp_index)"""
    from orb_line_slam_amd import CullView, MapGraph
    g = MapGraph(mp_obs=s.mp_obs, mp_bad=s.mp_bad, kf_bad=[0] * s.n_kf, kf_mp=[[-1] * s.slots] * s.n_kf, kf_covis=[[]] * s.n_kf, kf_children=[[]] * s.n_kf,
                 kf_parent=[-1] * s.n_kf)
    v = CullView(g, mp_obs_slot=s.mp_obs_slot, mp_nobs=[len(r) for r in s.mp_obs], kf_slot_octave=s.octave, kf_slot_depth=np.zeros((s.n_kf, s.slots)),
                 kf_slot_stereo=np.zeros((s.n_kf, s.slots)), kf_th_depth=np.zeros(s.n_kf), kf_mode=np.zeros(s.n_kf))
    return g, v


def snapshot_expected(s, points=None, start=None):
    """the restatement over the listed points (None: all): (normal, maxd, mind) starting from `start` or the sentinel -7"""
    normal, maxd, mind = (np.full((s.n_mp, 3), -7.0, F), np.full(s.n_mp, -7.0, F), np.full(s.n_mp, -7.0, F)) if start is None else [a.copy() for a in start]
    for p in (range(s.n_mp) if points is None else points):
        if s.mp_bad[p]:
            continue
        r = R.update_normal_and_depth(s.mp_obs[p], s.mp_obs_slot[p], s.mp_world[p], int(s.ref_kf[p]), s.kf_Ow, s.octave[int(s.ref_kf[p])], SF)
        if r is not None:
            normal[p], maxd[p], mind[p] = r
    return normal, maxd, mind


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
