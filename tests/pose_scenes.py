"""Synthetic frames for Optimizer::PoseOptimizationWithLine: a pinhole camera for the 320 x 240 context of the batch tests, points and segments at 2-15 m,
a true motion of a few centimetres and tenths of a degree since the previous frame, a prior that is off by about as much, observation noise of half a pixel
times the level's scale and, from 64 features on, a stated share of gross outliers (tens of pixels).  mvle_l comes from the noisy end points, normalised as
src/Frame.cc:939-941 does.  Octaves span every level; vertical, horizontal and oblique observed segments are all present from three lines on.

A scene is a dict of the arguments the restatement (pose_reference.pose_optimization_with_line), the host form and the device wrappers take, plus `truth`:
the true DT = Tcw_true * inverse(Tcw_prev) as the frame's DT output states it (its inverse)."""
import math
import numpy as np

W, H = 320, 240
CAMERA = (250.0, 250.0, 160.0, 120.0)                                # fx, fy, cx, cy
N_LEVELS, SCALE_FACTOR = 8, 1.2
OUTLIER_SHARE = 0.1
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"),
                          ("startPointX", "<f4"), ("startPointY", "<f4"), ("endPointX", "<f4"), ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"),
                          ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"), ("lineLength", "<f4"), ("numOfPixels", "<i4")])


def level_tables(n_levels=N_LEVELS, scale_factor=SCALE_FACTOR):
    """mvScaleFactor and mvInvLevelSigma2 as ORBextractor::ORBextractor forms them (src/ORBextractor.cc:421-436): float tables, a double factor"""
    f = float(np.float32(scale_factor))
    sf = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        sf[i] = np.float32(float(sf[i - 1]) * f)
    sigma2 = sf * sf
    return sf, (np.float32(1.0) / sigma2).astype(np.float32)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def se3(r, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(*r), t
    return T


def _project(T, X):
    P = T[:3, :3] @ X + T[:3, 3]
    return CAMERA[2] + CAMERA[0] * P[0] / P[2], CAMERA[3] + CAMERA[1] * P[1] / P[2]


def _unproject(Tinv, u, v, z):
    Pc = np.array([(u - CAMERA[2]) * z / CAMERA[0], (v - CAMERA[3]) * z / CAMERA[1], z])
    return (Tinv[:3, :3] @ Pc + Tinv[:3, 3]).astype(np.float32)


def line_equation(sx, sy, ex, ey):
    """mvle_l of a key line, src/Frame.cc:939-941: sp x ep over the norm of its first two entries, every coefficient divided"""
    sx, sy, ex, ey = float(np.float32(sx)), float(np.float32(sy)), float(np.float32(ex)), float(np.float32(ey))
    l = [sy * 1.0 - 1.0 * ey, 1.0 * ex - sx * 1.0, sx * ey - sy * ex]
    n = math.sqrt(l[0] * l[0] + l[1] * l[1])
    return [l[0] / n, l[1] / n, l[2] / n]


def make_scene(seed, n_points, n_lines, noise=True, true_prior=False, outliers=None, n_levels=N_LEVELS, extra_points=0, extra_lines=0):
    """n_points held points and n_lines held lines; extra_* features hold nothing (they sit between the held ones).  noise=False: exact observations;
    true_prior: the prior is the true pose.  outliers: gross outliers or not (None: from 64 features of a kind on)."""
    rng = np.random.RandomState(seed)
    sf, inv_sigma2 = level_tables(n_levels)
    Tprev = se3(rng.uniform(-0.2, 0.2, 3), rng.uniform(-1.0, 1.0, 3))
    M_true = se3(rng.uniform(-0.006, 0.006, 3), rng.uniform(-0.05, 0.05, 3))
    M_prior = M_true if true_prior else se3(rng.uniform(-0.006, 0.006, 3), rng.uniform(-0.05, 0.05, 3)) @ M_true
    Tcw_true = (M_true @ Tprev).astype(np.float32)
    Tcw = (M_prior @ Tprev).astype(np.float32)
    Tprev32 = Tprev.astype(np.float32)
    Tt = Tcw_true.astype(np.float64)
    Tinv = np.linalg.inv(Tt)

    N, NL = n_points + extra_points, n_lines + extra_lines
    keys, kls = np.zeros(N, KEYPOINT_DTYPE), np.zeros(NL, KEYLINE_DTYPE)
    keys["class_id"], kls["class_id"] = -1, np.arange(NL)
    frame_mp, frame_ml = np.full(N, -1, np.int32), np.full(NL, -1, np.int32)
    mp_world, ml_world, lle = np.zeros((n_points, 3), np.float32), np.zeros((n_lines, 6), np.float32), np.zeros((NL, 3), np.float64)
    held_p = np.sort(rng.permutation(N)[:n_points]) if extra_points else np.arange(N)
    held_l = np.sort(rng.permutation(NL)[:n_lines]) if extra_lines else np.arange(NL)
    gross_p = (n_points >= 64) if outliers is None else outliers
    gross_l = (n_lines >= 64) if outliers is None else outliers

    def jitter(octave, gross):
        if not noise:
            return np.zeros(2)
        d = rng.normal(0.0, 0.5 * float(sf[octave]), 2)
        if gross:
            d = d + rng.choice([-1.0, 1.0], 2) * rng.uniform(20.0, 60.0, 2)
        return d

    for i in range(N):
        octave = i % n_levels
        keys[i]["octave"], keys[i]["size"] = octave, 31.0 * sf[octave]
        keys[i]["x"], keys[i]["y"] = rng.uniform(20, W - 20), rng.uniform(20, H - 20)
    for m, i in enumerate(held_p):
        mp_world[m] = _unproject(Tinv, rng.uniform(20, W - 20), rng.uniform(20, H - 20), rng.uniform(2.0, 15.0))
        u, v = _project(Tt, mp_world[m].astype(np.float64))
        d = jitter(int(keys[i]["octave"]), gross_p and rng.uniform() < OUTLIER_SHARE)
        keys[i]["x"], keys[i]["y"] = u + d[0], v + d[1]
        frame_mp[i] = m
    for i in range(NL):
        octave = i % n_levels
        kls[i]["octave"] = octave
        kind = i % 3                                                  # vertical, horizontal, oblique
        u0, v0 = rng.uniform(40, W - 120), rng.uniform(40, H - 100)
        length = rng.uniform(30.0, 70.0)
        if kind == 0:
            u1, v1 = u0, v0 + length
        elif kind == 1:
            u1, v1 = u0 + length, v0
        else:
            a = rng.uniform(0.4, 1.1)
            u1, v1 = u0 + length * math.cos(a), v0 + length * math.sin(a)
        s = (u0, v0, u1, v1)
        if i in set(held_l.tolist()):
            m = int(np.searchsorted(held_l, i))
            ml_world[m, :3] = _unproject(Tinv, u0, v0, rng.uniform(2.0, 15.0))
            ml_world[m, 3:] = _unproject(Tinv, u1, v1, rng.uniform(2.0, 15.0))
            a, b = _project(Tt, ml_world[m, :3].astype(np.float64)), _project(Tt, ml_world[m, 3:].astype(np.float64))
            gross = gross_l and rng.uniform() < OUTLIER_SHARE
            # an axis-aligned segment keeps its character: the noise across it is shared by both end points (the detector's segments are straight)
            d0, d1 = jitter(octave if kind == 2 else 0, gross), jitter(octave if kind == 2 else 0, False)
            if kind == 0:
                d1[0] = d0[0]
            elif kind == 1:
                d1[1] = d0[1]
            s = (a[0] + d0[0], a[1] + d0[1], b[0] + d1[0] + (d0[0] if gross and kind == 2 else 0.0), b[1] + d1[1] + (d0[1] if gross and kind == 2 else 0.0))
            frame_ml[i] = m
        kls[i]["startPointX"], kls[i]["startPointY"], kls[i]["endPointX"], kls[i]["endPointY"] = s
        kls[i]["lineLength"] = math.hypot(s[2] - s[0], s[3] - s[1])
        lle[i] = line_equation(*s)
    truth = np.linalg.inv(Tcw_true.astype(np.float64) @ np.linalg.inv(Tprev32.astype(np.float64)))
    return dict(keys=keys, keylines=kls, lle=lle, Tcw=Tcw.reshape(16), Tcw_prev=Tprev32.reshape(16), camera=CAMERA, frame_mp=frame_mp, mp_world=mp_world,
                frame_ml=frame_ml, ml_world=ml_world, inv_level_sigma2=inv_sigma2, truth=truth, Tcw_true=Tcw_true.reshape(16))


ARGS = ("keys", "keylines", "lle", "Tcw", "camera", "frame_mp", "mp_world", "frame_ml", "ml_world")


def call_args(scene):
    """the positional arguments every form takes, in order"""
    return [scene[k] for k in ARGS]


# ---- the frames the device tests run, and what the CPU tests verify about each -------------------------------------------------------------------------------
CAP, LINE_CAP = 364, 150                                             # capacities of the 320 x 240 context with nfeatures = 300, lsd_nfeatures = 150
POINT_SIZES = (0, 1, 5, 6, 7, 63, 64, 65, 255, 256, 257, CAP)
LINE_SIZES = (0, 1, 2, 63, 64, 65, LINE_CAP)
# (name, seed, held points, held lines, features that hold nothing among the points, among the lines).  A seed is replaced when its frame misses a condition
# of test_pose_cpu.test_scene_conditions; it is never excused.
SPECS = ([("p%d" % n, 100 + n, n, 0, 0, 0) for n in POINT_SIZES] + [("l%d" % n, 200 + n, 0, n, 0, 0) for n in LINE_SIZES if n] +
         [("both_small", 301, 7, 2, 0, 0), ("both_64", 302, 64, 20, 0, 0), ("both_257", 303, 257, 65, 0, 0), ("both_full", 304, CAP, LINE_CAP, 0, 0),
          ("both_gaps", 305, 63, 30, 40, 10), ("both_tiny", 306, 1, 1, 3, 2), ("p5_all_outliers", 431, 5, 0, 0, 0)])
SEED_OVERRIDE = {"p5": 418}              # 105: the flags of that frame depend on the summation order (H is singular with five features)
MIN_FEATURES = 6                     # every feature adds rank one to H, so six are the least that determine a pose


def spec(name):
    return next(s for s in SPECS if s[0] == name)


_scene_cache, _ref_cache = {}, {}


def scene_of(name):
    if name not in _scene_cache:
        _, seed, n_p, n_l, x_p, x_l = spec(name)
        _scene_cache[name] = make_scene(SEED_OVERRIDE.get(name, seed), n_p, n_l, extra_points=x_p, extra_lines=x_l)
    return _scene_cache[name]


def determined(name):
    _, _, n_p, n_l, _, _ = spec(name)
    return n_p + n_l >= MIN_FEATURES


REAL_OUTPUTS = ("Tcw_out", "DT", "DT_cov", "DT_cov_eig", "err_norm")


def reference_for(scene, params=None, **kw):
    """the restatement's result for a frame given as a scene dict: `base` (index order, numpy.linalg.solve), the two switched runs `alts`, and per real output
    the largest difference between base and a switched run -- the restatement's own sensitivity, the yardstick of the tolerance rule.  kw: further arguments
    of the restatement (outlier, outlier_l, the index offsets)."""
    import pose_reference as R
    run = lambda **sw: R.pose_optimization_with_line(*call_args(scene), scene["inv_level_sigma2"], Tcw_prev=scene["Tcw_prev"], params=params or None, **kw, **sw)
    base, alts = run(), [run(reverse=True), run(lstsq=True)]
    with np.errstate(all="ignore"):
        spread = {k: max(float(np.max(np.abs(np.asarray(a[k], dtype=np.float64) - np.asarray(base[k], dtype=np.float64)))) for a in alts) for k in REAL_OUTPUTS}
    return dict(base=base, alts=alts, spread=spread)


def reference_of(name, **params):
    """reference_for of a frame of SPECS, computed once"""
    key = (name, tuple(sorted(params.items())))
    if key not in _ref_cache:
        _ref_cache[key] = reference_for(scene_of(name), params)
    return _ref_cache[key]


def yardstick_is_finite(ref):
    """the restatement's real outputs and their sensitivities are all finite: the tolerance rule compares every one of them"""
    return all(np.all(np.isfinite(np.asarray(ref["base"][k], dtype=np.float64))) and math.isfinite(ref["spread"][k]) for k in REAL_OUTPUTS)


def ulp_floor(name, value):
    """64 ulp of the output's largest magnitude (float ulp for Tcw_out): the last few operations of the epilogue"""
    mag = float(np.max(np.abs(np.asarray(value, dtype=np.float64))))
    eps = float(np.finfo(np.float32).eps) if name == "Tcw_out" else float(np.finfo(np.float64).eps)
    return 64.0 * eps * mag


def within_rule(name, got, ref):
    """The tolerance rule for one real output: |got - base| <= 16 x the restatement's sensitivity, with a floor of 64 ulp.  Returns (ok, ratio) where ratio =
    difference / max(sensitivity, floor / 16), so ok means ratio <= 16.  Where the restatement itself is not finite, or its two settings differ without
    bound, the yardstick says nothing and the output passes with ratio 0."""
    base, spread = np.asarray(ref["base"][name], dtype=np.float64), ref["spread"][name]
    got = np.asarray(got, dtype=np.float64)
    if not (np.all(np.isfinite(base)) and math.isfinite(spread)):
        return True, 0.0
    if not np.all(np.isfinite(got)):
        return False, math.inf
    unit = max(spread, ulp_floor(name, base) / 16.0)
    diff = float(np.max(np.abs(got - base))) if got.size else 0.0
    if unit == 0.0:
        return diff == 0.0, 0.0 if diff == 0.0 else math.inf
    return diff <= 16.0 * unit, diff / unit
