"""Synthetic key-frame pairs for Optimizer::OptimizeSim3: the pinhole camera of the 320 x 240 context of the batch tests (K1 = K2), kf2 points at 2-15 m, a
known S12 (X1c = s R X2c + t), a start off by a few cm, about a degree and 2 % of scale, observation noise of half a pixel times the level's scale in both
images.  A scene is a dict of two key frames at the capacity (keys, counts, Tcw, world, valid, bad: index 0 is kf1, 1 is kf2), the match row, the start
(s12, R12, t12), th2, fix_scale, the camera and mvInvLevelSigma2 -- what the restatement (optsim3_reference.optimize_sim3), the host form and the device
wrappers take.  The context of the device tests has nfeatures = 236, i.e. a capacity of 300, and 8 levels."""
import math
import numpy as np
import pose_scenes as PS

KEYPOINT_DTYPE = PS.KEYPOINT_DTYPE
W, H, N_LEVELS = PS.W, PS.H, PS.N_LEVELS
CAMERA = PS.CAMERA
NFEATURES, CAP = 236, 300
COUNTS = (0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257, CAP)
TH2 = 10.0
DEGENERATE = ("depth0",)                                              # the scene whose yardstick may say nothing
REAL_OUTPUTS = ("S12_out", "s12_out", "R12_out", "t12_out", "Scw_out", "chi2")
DISCRETE = ("n_inliers", "n_correspondences", "n_bad_first", "status")


def _project(X):
    return CAMERA[2] + CAMERA[0] * X[0] / X[2], CAMERA[3] + CAMERA[1] * X[1] / X[2]


def make_scene(seed, n, fix_scale, extra=0, outlier_share=0.0, outlier_side="both", start=(0.03, 1.0, 1.02), noise=0.5, identity=False):
    """n correspondences and `extra` kf1 features without one, interleaved; kf2 has five features more than it is matched to.  fix_scale: the true scale is
    1.0 and the start's 1.3 (which then stays); free: the true scale is 1.3.  start = (metres, degrees, scale factor) the input is off.  outlier_share of
    the correspondences get a gross error of 30-80 px in image 1 and 2 ("both") or in image 2 alone ("2").  identity: S12, its start and both poses are the
    identity."""
    rng = np.random.RandomState(seed)
    sf, inv_sigma2 = PS.level_tables()
    s_true = 1.0 if fix_scale else 1.3
    R_true = PS.rot(*rng.uniform(-0.1, 0.1, 3))
    t_true = rng.uniform(-1.0, 1.0, 3) * (0.03 if fix_scale else 1.0)          # (the scale is observed through t alone)
    T1w, T2w = PS.se3(rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.5, 0.5, 3)), PS.se3(rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.5, 0.5, 3))
    d = rng.normal(size=3)
    d = d / np.linalg.norm(d) * start[0]
    a = rng.normal(size=3)
    a = a / np.linalg.norm(a) * math.radians(start[1])
    dR, ds = PS.rot(*a), (1.3 if fix_scale else start[2])
    if identity:
        R_true, t_true, s_true, T1w, T2w, dR, d, ds = np.eye(3), np.zeros(3), 1.0, np.eye(4), np.eye(4), np.eye(3), np.zeros(3), 1.0
    R12, t12, s12 = dR @ R_true, ds * (dR @ t_true) + d, ds * s_true
    N1, N2 = n + extra, min(CAP, n + 5)
    holds = np.zeros(N1, bool)
    holds[rng.permutation(N1)[:n]] = True
    i2_of = rng.permutation(N2)[:n]
    keys = np.zeros((2, CAP), KEYPOINT_DTYPE)
    world = np.zeros((2, CAP, 3), np.float32)
    matches = np.full(CAP, -1, np.int32)
    n_out = int(round(outlier_share * n))
    out_k = set(rng.permutation(n)[:n_out].tolist())
    T1inv, T2inv = np.linalg.inv(T1w), np.linalg.inv(T2w)

    def key(x, y, o):
        return (x, y, 31.0 * sf[o], 0.0, 1.0, o, -1)

    def gross():
        ang, mag = rng.uniform(0, 2 * math.pi), rng.uniform(30, 80)
        return mag * math.cos(ang), mag * math.sin(ang)

    k = 0
    used2 = np.zeros(N2, bool)
    for i in range(N1):
        u, v, z = rng.uniform(30, W - 30), rng.uniform(30, H - 30), rng.uniform(2.0, 15.0)
        X2 = np.array([(u - CAMERA[2]) * z / CAMERA[0], (v - CAMERA[3]) * z / CAMERA[1], z])
        X1 = s_true * (R_true @ X2) + t_true
        o1, o2 = int(rng.randint(0, N_LEVELS)), int(rng.randint(0, N_LEVELS))
        u1, v1 = _project(X1)
        e1, e2 = rng.normal(0, noise * float(sf[o1]), 2), rng.normal(0, noise * float(sf[o2]), 2)
        if holds[i]:
            if k in out_k:
                g1, g2 = gross(), gross()
                e2 = e2 + g2
                if outlier_side == "both":
                    e1 = e1 + g1
            j = int(i2_of[k])
            used2[j] = True
            matches[i] = j
            keys[1, j] = key(u + e2[0], v + e2[1], o2)
            world[1, j] = T2inv[:3, :3] @ X2 + T2inv[:3, 3]
            k += 1
        keys[0, i] = key(u1 + e1[0], v1 + e1[1], o1)
        world[0, i] = T1inv[:3, :3] @ X1 + T1inv[:3, 3]
    for j in np.nonzero(~used2)[0]:
        keys[1, j] = key(rng.uniform(30, W - 30), rng.uniform(30, H - 30), int(rng.randint(0, N_LEVELS)))
        world[1, j] = rng.uniform(-3, 3, 3)
    return dict(keys=keys, counts=np.array([N1, N2], np.int32), Tcw=np.stack([T1w, T2w]).astype(np.float32), world=world, valid=np.ones((2, CAP), np.uint8),
                bad=np.zeros((2, CAP), np.uint8), matches=matches, s12=np.float32(s12), R12=R12.astype(np.float32).reshape(9), t12=t12.astype(np.float32),
                th2=TH2, fix_scale=int(fix_scale), camera=CAMERA, inv_level_sigma2=inv_sigma2, truth=(s_true, R_true, t_true), n=n)


def _depth0(seed):
    """one kf2 point exactly in the plane z = 0 of camera 1 at the input S12 (the identity, both poses the identity)"""
    s = make_scene(seed, 20, False, identity=True)
    i = int(np.nonzero(s["matches"] >= 0)[0][3])
    s["world"][1, s["matches"][i]] = (0.5, 0.25, 0.0)
    return s


def _bad_octave(seed):
    s = make_scene(seed, 30, False, extra=3)
    m = np.nonzero(s["matches"] >= 0)[0]
    s["keys"]["octave"][0, m[2]] = N_LEVELS
    s["keys"]["octave"][1, s["matches"][m[7]]] = -1
    return s


def _skipped(seed):
    """entries that are no correspondence and keep their value: -2, a value >= N2, a kf1 feature that holds no point, one that holds a bad point, and an
    entry whose kf2 point is bad"""
    s = make_scene(seed, 40, False, extra=6)
    m = np.nonzero(s["matches"] >= 0)[0]
    none = np.nonzero(s["matches"] < 0)[0]
    s["matches"][none[0]] = -2
    s["matches"][none[1]] = int(s["counts"][1])
    s["matches"][none[2]] = CAP + 7
    s["valid"][0, m[1]] = 0
    s["bad"][0, m[4]] = 1
    s["bad"][1, s["matches"][m[9]]] = 1
    s["valid"][1, s["matches"][m[12]]] = 0
    return s


_scene_cache, _ref_cache = {}, {}

# name -> builder.  A seed is replaced when its scene misses a condition of test_optsim3_cpu.test_scene_conditions; it is never excused.
SPECS = {}
SEED_OVERRIDE = {"gate12": 915}     # 905: five iterations from its start leave ten of the twelve above th2, not the four outliers alone
for _n in COUNTS:
    for _fix in (0, 1):
        _name = "n%d_%s" % (_n, "fixed" if _fix else "free")
        SPECS[_name] = (lambda n=_n, fix=_fix, name=_name: make_scene(SEED_OVERRIDE.get(name, 700 + 2 * n + fix), n, bool(fix), extra=0 if n == CAP else min(7, CAP - n)))
SPECS["clean64"] = lambda: make_scene(SEED_OVERRIDE.get("clean64", 901), 64, False, extra=4)
SPECS["out20"] = lambda: make_scene(SEED_OVERRIDE.get("out20", 902), 100, False, extra=5, outlier_share=0.2)
SPECS["out20_fixed"] = lambda: make_scene(SEED_OVERRIDE.get("out20_fixed", 903), 100, True, extra=5, outlier_share=0.2)
SPECS["one_side"] = lambda: make_scene(SEED_OVERRIDE.get("one_side", 904), 80, False, extra=5, outlier_share=0.2, outlier_side="2")
SPECS["gate12"] = lambda: make_scene(SEED_OVERRIDE.get("gate12", 905), 12, False, extra=3, outlier_share=4.0 / 12.0)
SPECS["all_out"] = lambda: make_scene(SEED_OVERRIDE.get("all_out", 906), 40, False, extra=3, outlier_share=1.0)
SPECS["skipped"] = lambda: _skipped(SEED_OVERRIDE.get("skipped", 907))
SPECS["bad_octave"] = lambda: _bad_octave(SEED_OVERRIDE.get("bad_octave", 908))
SPECS["depth0"] = lambda: _depth0(SEED_OVERRIDE.get("depth0", 909))


def _swapped():
    """clean64 read the other way round: the pair (kf2, kf1), the row inverted, the start inverted.  In a batch it shares clean64's two frames, so both
    stand on either side of a pair"""
    s = scene_of("clean64")
    inv = np.full(CAP, -1, np.int32)
    i = np.nonzero(s["matches"] >= 0)[0]
    inv[s["matches"][i]] = i
    R, t, sc = s["R12"].reshape(3, 3).astype(np.float64), s["t12"].astype(np.float64), float(s["s12"])
    sw = dict(s, matches=inv, s12=np.float32(1.0 / sc), R12=R.T.astype(np.float32).reshape(9), t12=(-(1.0 / sc) * (R.T @ t)).astype(np.float32))
    for k in ("keys", "counts", "Tcw", "world", "valid", "bad"):
        sw[k] = s[k][::-1].copy()
    return sw


SPECS["swapped"] = _swapped
NAMES = list(SPECS)



def scene_of(name):
    if name not in _scene_cache:
        _scene_cache[name] = SPECS[name]()
    return _scene_cache[name]


def reference_for(scene):
    """the restatement's result: `base`, the switched runs `alts`, and per real output the largest difference between base and a switched run -- the
    restatement's own sensitivity, the yardstick of the tolerance rule (pose_scenes.within_rule)"""
    import optsim3_reference as R
    base = R.optimize_sim3(scene, sw=R.BASE)
    alts = [R.optimize_sim3(scene, sw=sw) for sw in R.SWITCHED]
    with np.errstate(all="ignore"):
        spread = {k: max(float(np.max(np.abs(np.asarray(a[k], np.float64) - np.asarray(base[k], np.float64)), initial=0.0)) for a in alts) for k in REAL_OUTPUTS}
    return dict(base=base, alts=alts, spread=spread)


def reference_of(name):
    if name not in _ref_cache:
        _ref_cache[name] = reference_for(scene_of(name))
    return _ref_cache[name]


def yardstick_is_finite(ref):
    return all(np.all(np.isfinite(np.asarray(ref["base"][k], np.float64))) and math.isfinite(ref["spread"][k]) for k in REAL_OUTPUTS)


def within_rule(name, got, ref):
    """pose_scenes.within_rule with every real output's floor in float ulps (the double S12_out too): |got - base| <= 16 x the restatement's spread, with a
    floor of 64 float ulp"""
    return PS.within_rule("Tcw_out", got, dict(base={"Tcw_out": ref["base"][name]}, spread={"Tcw_out": ref["spread"][name]}))


def check_against(got, got_matches, ref, where):
    """a library result (host form or device) and the match row it left against the restatement: discrete outputs exact, the real ones under the rule"""
    base = ref["base"]
    assert np.array_equal(np.asarray(got_matches), base["matches"]), (where, "matches")
    for g in DISCRETE:
        assert int(got[g]) == int(base[g]), (where, g, got[g], base[g])
    worst = 0.0
    for k in REAL_OUTPUTS:
        ok, ratio = within_rule(k, got[k], ref)
        assert ok, (where, k, ratio)
        worst = max(worst, ratio)
    return worst
