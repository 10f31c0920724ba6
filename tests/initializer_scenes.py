"""Constructed two-view scenes for Initializer::Initialize at a capacity of 512: the smallest shapes where the code can go wrong.  Every scene is one
(reference, current) pair with its own two frames.  analyse() runs the restatement (tests/initializer_reference.py) under its switches and asserts FROM
THE RESTATEMENT ALONE that every decision of a scene is settled -- the same under all switches, with a margin: the winner of each RANSAC (its sample
set and the gap to the next score), RH against 0.40, the d1 / d2 and d2 / d3 gates, the nGood comparisons, the parallax comparisons; and that at most a
quarter of a scene's correspondences are "near" a threshold (a chi-square or a CheckRT comparison within 1e-3 relative, or a flag that differs between
switches).  What the tests compare exactly is compared outside the near set.

Parameter sets: FAST (sigma 1, 24 iterations) for every scene; TRACKER (sigma 1, 200 iterations, the tracker's) and ONE (sigma 2, one iteration) for a
few, which keeps the restatement's run time down."""
import functools
import math
import numpy as np
import initializer_reference as R
from orb_line_slam_amd import _lib

F = np.float32
CAP = 512
CAM = (500.0, 500.0, 320.0, 240.0)
FAST = dict(sigma=1.0, max_iterations=24, min_parallax=1.0, min_triangulated=50)
TRACKER = dict(sigma=1.0, max_iterations=200, min_parallax=1.0, min_triangulated=50)
ONE = dict(sigma=2.0, max_iterations=1, min_parallax=1.0, min_triangulated=50)
SETS = {"fast": FAST, "tracker": TRACKER, "one": ONE}

# name, kind, N correspondences, unmatched keys in frame 1 / frame 2, outlier fraction, noise (pixels), seed
SCENES = [
    ("n0", "general", 0, 120, 90, 0.0, 0.1, 1), ("n7", "general", 7, 40, 30, 0.0, 0.1, 2), ("n8", "general", 8, 40, 30, 0.0, 0.1, 3),
    ("n9", "general", 9, 40, 30, 0.0, 0.1, 4), ("n63", "general", 63, 5, 9, 0.0, 0.1, 5), ("n64", "general", 64, 0, 0, 0.0, 0.1, 6),
    ("n65", "general", 65, 17, 3, 0.0, 0.1, 7), ("n255", "general", 255, 1, 0, 0.0, 0.1, 8), ("n256", "planar", 256, 0, 7, 0.0, 0.1, 9),
    ("n257", "general", 257, 100, 255, 0.0, 0.1, 10), ("cap", "general", CAP, 0, 0, 0.0, 0.1, 11), ("beyond", "planar", 300, 212, 212, 0.0, 0.1, 12),
    ("planar", "planar", 180, 37, 11, 0.0, 0.1, 13), ("general", "general", 180, 11, 37, 0.0, 0.1, 14), ("rotation", "rotation", 180, 20, 20, 0.0, 0.1, 15),
    ("lowpar", "lowpar", 180, 20, 20, 0.0, 0.1, 16), ("similar", "similar", 200, 10, 10, 0.0, 0.1, 108), ("good50", "general", 50, 30, 30, 0.0, 0.1, 18),
    ("good51", "general", 51, 30, 30, 0.0, 0.1, 19), ("good52", "general", 52, 30, 30, 0.0, 0.1, 20), ("outliers", "general", 200, 25, 25, 0.3, 0.1, 100),
]
NAMES = [s[0] for s in SCENES]
SUBSET = {"fast": NAMES, "tracker": ["general", "planar", "n9"], "one": ["general", "planar", "n8", "n65"]}


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _project(X, Rm, t):
    Xc = X @ Rm.T + t
    return np.stack([CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]], 1)


def _points(rng, kind, n):
    x, y = rng.uniform(-3, 3, n), rng.uniform(-2, 2, n)
    if kind == "planar":                                             # wide and tilted: the twin solution of the decomposition puts a third of the points behind a camera
        x, y = rng.uniform(-4, 4, n), rng.uniform(-2.8, 2.8, n)
        return np.stack([x, y, 6 + 0.5 * x], 1)
    if kind == "lowpar":
        return np.stack([12 * x, 12 * y, rng.uniform(60, 110, n)], 1)
    if kind == "similar":
        z = np.where(np.arange(n) < int(0.75 * n), rng.uniform(4000, 9000, n), rng.uniform(4, 9, n))
        return np.stack([x * z / 6, y * z / 6, z], 1)
    return np.stack([x, y, rng.uniform(4, 12, n)], 1)


class Scene:
    pass


@functools.lru_cache(maxsize=None)
def scene(name):
    _, kind, N, e1, e2, out, noise, seed = SCENES[NAMES.index(name)]
    rng = np.random.default_rng(1000 + seed)
    Rm = _rot(0.02, -0.03, 0.015)
    t = np.array([0.0, 0.0, 0.0]) if kind == "rotation" else np.array([0.05, 0.004, 0.01]) if kind == "lowpar" else np.array([0.6, 0.05, 0.12])
    if kind == "rotation":
        Rm = _rot(0.05, -0.08, 0.03)
    if kind == "planar":
        Rm, t = _rot(0.02, -0.1, 0.015), np.array([2.0, 0.2, 0.1])
    X = _points(rng, kind, N)
    p1, p2 = _project(X, np.eye(3), np.zeros(3)), _project(X, Rm, t)
    p1, p2 = p1 + rng.normal(0, noise, p1.shape), p2 + rng.normal(0, noise, p2.shape)
    nout = int(out * N)
    if nout:
        p2[rng.choice(N, nout, replace=False)] = np.stack([rng.uniform(20, 620, nout), rng.uniform(20, 460, nout)], 1)
    N1, N2 = N + e1, N + e2
    s = Scene()
    s.name, s.N, s.N1, s.N2 = name, N, N1, N2
    s.kp = np.zeros((2, CAP), _lib.KEYPOINT_DTYPE)
    s.kp["x"], s.kp["y"], s.kp["class_id"] = rng.uniform(20, 620, (2, CAP)), rng.uniform(20, 460, (2, CAP)), -1
    pos1, pos2 = np.sort(rng.choice(N1, N, replace=False)), rng.permutation(N2)[:N]
    s.kp["x"][0, pos1], s.kp["y"][0, pos1] = p1[:, 0], p1[:, 1]
    s.kp["x"][1, pos2], s.kp["y"][1, pos2] = p2[:, 0], p2[:, 1]
    s.matches = np.full(CAP, -1, np.int32)
    s.matches[pos1] = pos2
    free = np.setdiff1d(np.arange(N1), pos1)
    s.matches[free[0::3]] = N2 + 3                                   # "none" as the matchers spell it: -1, -2 and >= N2
    s.matches[free[1::3]] = -2
    s.matches[N1:] = np.arange(CAP - N1) % max(N2, 1)                # beyond N1: never read
    s.counts = np.array([N1, N2], np.int32)
    if name == "beyond":
        s.counts = np.array([CAP + 100, CAP + 7], np.int32)          # counts beyond the capacity are read as the capacity
    return s


def draws(name, max_iterations):
    return np.random.default_rng(77 + 131 * SCENES[NAMES.index(name)][7]).integers(0, 1 << 31, size=(max_iterations, 8), dtype=np.uint32)


def restate(name, pset, **switches):
    s = scene(name)
    p = SETS[pset]
    n1, n2 = min(int(s.counts[0]), CAP), min(int(s.counts[1]), CAP)
    kp1 = np.stack([s.kp["x"][0, :n1], s.kp["y"][0, :n1]], 1)
    kp2 = np.stack([s.kp["x"][1, :n2], s.kp["y"][1, :n2]], 1)
    return R.initialize(kp1, kp2, s.matches, CAM, draws(name, p["max_iterations"]), **p, **switches)


class Analysis:
    pass


def _gap(log, win, N, dr):
    """how far, relatively, the winner's score is ahead of the best iteration that drew another set of eight"""
    if win < 0:
        return math.inf
    mine = sorted(R.sample8(N, dr[win]))
    rest = [v for it, v in enumerate(log) if sorted(R.sample8(N, dr[it])) != mine]
    return math.inf if not rest else (log[win] - max(rest)) / log[win]


@functools.lru_cache(maxsize=None)
def analyse(name, pset):
    """the restatement of a scene under its switches, with the builder's assertions"""
    a = Analysis()
    a.base = restate(name, pset)
    a.alts = [restate(name, pset, svd="lapack"), restate(name, pset, fill="alt")]
    b = a.base
    a.near = np.zeros(b.N, bool)
    a.ng_spread = 0
    a.unstable = [x.copy() for x in getattr(b, "near_h", [])]      # per hypothesis: the correspondences whose CheckRT outcome the switches move
    if b.N < 8:
        return a
    p = SETS[pset]
    dr = draws(name, p["max_iterations"])
    assert not b.degenerate, name
    for o in a.alts:
        for win, owin, log in ((b.win_H, o.win_H, b.log_H), (b.win_F, o.win_F, b.log_F)):
            same_set = win >= 0 and owin >= 0 and sorted(R.sample8(b.N, dr[win])) == sorted(R.sample8(b.N, dr[owin]))
            assert win == owin or same_set, (name, pset, "winner", win, owin)
        assert o.model == b.model and abs(b.RH - 0.40) > 0.01 and abs(o.RH - 0.40) > 0.01, (name, pset, "RH", b.RH, o.RH)
        assert o.ok == b.ok, (name, pset, "ok")
        spread = int(np.abs(np.sort(o.n_good) - np.sort(b.n_good)).max())      # (the order of ReconstructF's four follows the null vector's sign)
        a.ng_spread = max(a.ng_spread, spread)
        if b.gates is not None:
            for g, og in zip(b.gates, o.gates):
                assert (g < 1.00001) == (og < 1.00001) and abs(g - 1.00001) > 1e-5 and abs(og - 1.00001) > 1e-5, (name, pset, "gate", g, og)
        for k, v in b.margins.items():                               # a count margin has to clear what the counts move by between switches
            room = 1e-2 + (0 if k == "parallax" else spread)
            assert (v > 0) == (o.margins[k] > 0) and abs(v) > room and abs(o.margins[k]) > room, (name, pset, k, v, o.margins[k])
        a.near |= (o.flags_H != b.flags_H) | (o.flags_F != b.flags_F)
        for h in range(len(getattr(o, "Rs", []))):                   # hypothesis h of this run is the base's nearest one (ReconstructF's order follows a sign)
            hb = int(np.argmin([np.abs(o.Rs[h] - b.Rs[k]).sum() + np.abs(o.ts[h] - b.ts[k]).sum() for k in range(len(b.Rs))]))
            a.unstable[hb] |= (o.counted_h[h] != b.counted_h[hb]) | o.near_h[h]
        if b.model == o.model and hasattr(b, "near_rt"):
            a.near |= o.near_rt
        if b.ok:
            a.near |= (o.counted != b.counted) | (o.good != b.good)
    for chi in (b.chi_H, b.chi_F):
        if chi is not None:
            a.near |= (np.abs(chi - 1) < 1e-3).any(1)
    if hasattr(b, "near_rt"):
        a.near |= b.near_rt
    assert a.near.sum() * 4 <= b.N, (name, pset, "near", int(a.near.sum()), b.N)
    # the winners are ahead of the next score by more than rounding (iterations that drew the same eight points aside)
    gaps = _gap(b.log_H, b.win_H, b.N, dr), _gap(b.log_F, b.win_F, b.N, dr)
    assert min(gaps) > 1e-5, (name, pset, "gap", gaps)
    return a


def conditions():
    """what the scene list is there to cover, asserted from the restatement"""
    A = {n: analyse(n, "fast").base for n in NAMES}
    assert [A[n].N for n in NAMES[:12]] == [0, 7, 8, 9, 63, 64, 65, 255, 256, 257, CAP, 300]
    assert A["planar"].model == 1 and A["planar"].ok == 1 and A["general"].model == 2 and A["general"].ok == 1
    assert A["rotation"].model == 1 and A["rotation"].ok == 0
    assert A["lowpar"].ok == 0 and A["lowpar"].margins["parallax"] < 0
    assert A["similar"].model == 2 and A["similar"].ok == 0 and A["similar"].margins["second"] < 0
    for n, k in (("good50", 50), ("good51", 51), ("good52", 52)):
        assert A[n].model == 2 and max(A[n].n_good) == k and A[n].ok == 1, (n, A[n].n_good, A[n].model, A[n].ok)
    assert A["outliers"].ok == 1 and 120 <= A["outliers"].n_inliers <= 150
    assert A["beyond"].ok == 1


def batch(names):
    """the scenes `names` as one batch: kps [2 n, CAP], counts [2 n], pairs [n, 2], matches [n, CAP]"""
    S = [scene(n) for n in names]
    kps = np.concatenate([s.kp for s in S], 0)
    counts = np.concatenate([s.counts for s in S])
    pairs = np.array([[2 * i, 2 * i + 1] for i in range(len(S))], np.int32)
    matches = np.stack([s.matches for s in S], 0)
    return kps, counts, pairs, matches
