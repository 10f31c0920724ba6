"""Synthetic frames for Optimizer::PoseOptimization: the pinhole camera of the 320 x 240 context of the batch tests with a stereo baseline, points at
2-15 m, a start pose 5 cm / 1 degree off the truth (unless the scene says otherwise), observation noise of half a pixel times the level's scale, monocular
(mvuRight = -1), stereo or interleaved edges.  A scene is a dict of the arguments the restatement (posepoints_reference.pose_optimization), the host form
and the device wrappers take, plus `truth` (the true Tcw).  The context of the device tests has nfeatures = 236, i.e. a capacity of 300."""
import math
import numpy as np
import pose_scenes as PS

KEYPOINT_DTYPE = PS.KEYPOINT_DTYPE
W, H, N_LEVELS = PS.W, PS.H, PS.N_LEVELS
CAMERA = PS.CAMERA + (25.0,)                                          # fx, fy, cx, cy, mbf
NFEATURES, CAP = 236, 300
HELD = (0, 2, 3, 9, 10, 11, 63, 64, 65, 255, 256, 257, CAP)
KINDS = ("mono", "stereo", "mix")
DEGENERATE = ("depth0",)                                              # the scene whose yardstick may say nothing


def make_scene(seed, n_held, kind, extra=0, outlier_share=0.0, start=(0.05, 1.0), noise=0.5, outlier_bias=None, true_pose=None, n_levels_used=N_LEVELS):
    """n_held features that hold a point and `extra` that hold none, interleaved.  start = (metres, degrees) the input pose is off.  outlier_share of the
    held features get a gross error of 30-80 px (or all the same outlier_bias, which drags the first pass)."""
    rng = np.random.RandomState(seed)
    sf, inv_sigma2 = PS.level_tables()
    T_true = PS.se3(rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.5, 0.5, 3)) if true_pose is None else true_pose
    d = rng.normal(size=3)
    d = d / np.linalg.norm(d) * start[0]
    a = rng.normal(size=3)
    a = a / np.linalg.norm(a) * math.radians(start[1])
    T_start = PS.se3(a, d) @ T_true
    n = n_held + extra
    holds = np.zeros(n, bool)
    holds[rng.permutation(n)[:n_held]] = True
    keys, ur, fmp, world = np.zeros(n, KEYPOINT_DTYPE), np.full(n, -1.0, np.float32), np.full(n, -1, np.int32), []
    Tinv = np.linalg.inv(T_true)
    n_out = int(round(outlier_share * n_held))
    out_idx = set(np.nonzero(holds)[0][rng.permutation(n_held)[:n_out]].tolist())
    for i in range(n):
        u, v, z = rng.uniform(20, W - 20), rng.uniform(20, H - 20), rng.uniform(2.0, 15.0)
        oct_ = int(rng.randint(0, n_levels_used))
        s = noise * float(sf[oct_])
        stereo = kind == "stereo" or (kind == "mix" and i % 3 != 1)
        du, dv, dr = rng.normal(0, s), rng.normal(0, s), rng.normal(0, s)
        if i in out_idx:
            if outlier_bias is None:
                ang, mag = rng.uniform(0, 2 * math.pi), rng.uniform(30, 80)
                du, dv = du + mag * math.cos(ang), dv + mag * math.sin(ang)
            else:
                du, dv = du + outlier_bias[0], dv + outlier_bias[1]
            dr = dr + du
        keys[i] = (u + du, v + dv, 31.0 * sf[oct_], 0.0, 1.0, oct_, -1)
        if stereo:
            ur[i] = u - CAMERA[4] / z + dr
        if holds[i]:
            fmp[i] = len(world)
            world.append(PS._unproject(Tinv, u, v, z))
    world = np.array(world, np.float32).reshape(-1, 3)
    return dict(keys=keys, uright=ur, Tcw=T_start.astype(np.float32), camera=CAMERA, frame_mp=fmp, mp_world=world, inv_level_sigma2=inv_sigma2, truth=T_true,
                n_held=n_held)


def _depth0(seed):
    """one held point exactly in the camera's plane z = 0 at the (axis-aligned) input pose"""
    s = make_scene(seed, 20, "mix", start=(0.0, 0.0), true_pose=np.eye(4))
    s["mp_world"][int(s["frame_mp"][s["frame_mp"] >= 0][3])] = (0.5, 0.25, 0.0)
    return s


def _bad_octave(seed):
    s = make_scene(seed, 30, "mix")
    held = np.nonzero(s["frame_mp"] >= 0)[0]
    s["keys"]["octave"][held[2]], s["keys"]["octave"][held[7]] = N_LEVELS, -1
    return s


def _past_map(seed):
    s = make_scene(seed, 30, "stereo")
    held = np.nonzero(s["frame_mp"] >= 0)[0]
    s["frame_mp"][held[5]] = s["mp_world"].shape[0]
    return s


def _empties(seed):
    """every held feature is a gross outlier of its own: pass 1 flags them all, so pass 2 starts with an empty active set"""
    return make_scene(seed, 40, "mix", outlier_share=1.0)


# name -> builder.  A seed is replaced when its scene misses a condition of test_posepoints_cpu.test_scene_conditions; it is never excused.
SPECS = {}
SEED_OVERRIDE = {3: 1503}            # 503: three edges leave the pose so weakly held that a stop rule's margin is under 1000 x its spread
for _k, _n in enumerate(HELD):
    SPECS["n%d_%s" % (_n, KINDS[_k % 3])] = (lambda n=_n, k=_k: make_scene(SEED_OVERRIDE.get(n, 500 + n), n, KINDS[k % 3], extra=0 if n == CAP else min(7, CAP - n)))
for _k, _kind in enumerate(KINDS):
    SPECS["clean64_%s" % _kind] = (lambda k=_k, kind=_kind: make_scene(600 + k, 64, kind))
    SPECS["out20_%s" % _kind] = (lambda k=_k, kind=_kind: make_scene(610 + k, 100, kind, extra=5, outlier_share=0.2))
SPECS["readmit"] = lambda: make_scene(621, 80, "mix", outlier_share=0.3, outlier_bias=(12.0, 9.0), noise=1.1)
SPECS["far_start"] = lambda: make_scene(633, 90, "mix", start=(2.5, 50.0))
SPECS["empties"] = lambda: _empties(640)
SPECS["depth0"] = lambda: _depth0(650)
SPECS["bad_octave"] = lambda: _bad_octave(660)
SPECS["past_map"] = lambda: _past_map(670)
NAMES = list(SPECS)

_scene_cache, _ref_cache = {}, {}
REAL_OUTPUTS = ("Tcw_out", "chi2")                                   # both in float: the rule's floor is 64 float ulp


def scene_of(name):
    if name not in _scene_cache:
        _scene_cache[name] = SPECS[name]()
    return _scene_cache[name]


def ref_args(s):
    return (np.column_stack([s["keys"]["x"], s["keys"]["y"]]), s["uright"], s["keys"]["octave"], s["Tcw"], s["camera"], s["frame_mp"], s["mp_world"],
            s["inv_level_sigma2"])


def reference_for(scene):
    """the restatement's result: `base`, the switched runs `alts`, and per real output the largest difference between base and a switched run -- the
    restatement's own sensitivity, the yardstick of the tolerance rule (pose_scenes.within_rule)"""
    import posepoints_reference as R
    base = R.pose_optimization(*ref_args(scene), sw=R.BASE)
    alts = [R.pose_optimization(*ref_args(scene), sw=sw) for sw in R.SWITCHED]
    with np.errstate(all="ignore"):
        spread = {k: max(float(np.max(np.abs(a[k].astype(np.float64) - base[k].astype(np.float64)), initial=0.0)) for a in alts) for k in REAL_OUTPUTS}
    return dict(base=base, alts=alts, spread=spread)


def reference_of(name):
    if name not in _ref_cache:
        _ref_cache[name] = reference_for(scene_of(name))
    return _ref_cache[name]


def yardstick_is_finite(ref):
    return all(np.all(np.isfinite(ref["base"][k].astype(np.float64))) and math.isfinite(ref["spread"][k]) for k in REAL_OUTPUTS)


def within_rule(name, got, ref):
    """pose_scenes.within_rule with both real outputs in float ulps: |got - base| <= 16 x the restatement's spread, with a floor of 64 float ulp"""
    return PS.within_rule("Tcw_out", got, dict(base={"Tcw_out": ref["base"][name]}, spread={"Tcw_out": ref["spread"][name]}))


DISCRETE = (("outlier_out", "outlier"), ("n_good", "n_good"), ("n_initial", "n_initial"), ("passes", "passes"), ("status", "status"))


def check_against(got, ref, where):
    """a library result (host form or device) against the restatement: discrete outputs exact, the real ones under the rule"""
    base = ref["base"]
    for g, r in DISCRETE:
        assert np.array_equal(np.asarray(got[g]), np.asarray(base[r])), (where, g, got[g], base[r])
    worst = 0.0
    for k in REAL_OUTPUTS:
        ok, ratio = within_rule(k, got[k], ref)
        assert ok, (where, k, ratio)
        worst = max(worst, ratio)
    return worst
