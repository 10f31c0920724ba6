"""Scenes for olf_pnp_solver*: (key frame, frame) pairs at 320 x 240 with 8 levels and a capacity of 504 (what a context of 440 features takes), like tests/sim3solver_scenes.py.  Pair k owns
frames 2k (the key frame, whose features hold the 3-D points) and 2k + 1 (the lost frame, whose features are the 2-D points); row[i] names the key-frame
feature whose point frame feature i sees.  Inliers are noise-free (the float32 projection of the float32 point), outliers are displaced by tens of pixels,
so a four-inlier sample has an exact solution and counts are decisive.  The builder (analyse) classifies every evaluated iteration FROM THE RESTATEMENT
ALONE: settled (count and chosen variant agree under every switch) or open, asserts that everything the trajectory depends on is settled, and prints the
open share per scene."""
import functools
import math
import types
import numpy as np
import pnpsolver_reference as R
from orb_line_slam_amd._lib import KEYPOINT_DTYPE

F = np.float32
W, H = 320, 240
CAM = (200.0, 200.0, 160.0, 120.0)
CAP = 504
PARAMS = dict(probability=0.99, min_inliers=10, max_iterations=40, min_set=4, epsilon=0.5)      # the tracker's, with a cap that keeps the suite quick
TH2 = 5.991
ALT = dict(probability=0.95, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.3)          # off the defaults; the one set with 300 iterations
ALT_TH2 = 9.0


def scale_factors(n=8):
    sf = np.ones(n, F)
    for i in range(1, n):
        sf[i] = F(float(sf[i - 1]) * float(F(1.2)))
    return sf


SF = scale_factors()
SPEC = types.SimpleNamespace
# N correspondences, of which `inl` are inliers of the true pose (None: all); special: see make_pair
PAIR_SPECS = (
    SPEC(N=0), SPEC(N=3), SPEC(N=4), SPEC(N=9), SPEC(N=10),          # 0-3: below the minimum; 4: N == minimum, one iteration, Refine fails on the strict >
    SPEC(N=11), SPEC(N=19, inl=15), SPEC(N=20, inl=14), SPEC(N=21, inl=16), SPEC(N=22, inl=17),      # 5: accepted on the first record
    SPEC(N=63, inl=45), SPEC(N=64, inl=40), SPEC(N=65, inl=50), SPEC(N=300, inl=200), SPEC(N=None, inl=300),
    SPEC(N=41, special="two_poses"),                                 # 15: a record of exactly min_inliers that Refine rejects, then a better one
    SPEC(N=40, inl=5),                                               # 16: reaches the cap with nothing
    SPEC(N=30, special="duplicate"),                                 # 17: iteration 0 samples a duplicated 3-D point
)


def _rotation(rng, max_deg):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = math.radians(rng.uniform(0.2 * max_deg, max_deg))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K


def _project(Rm, t, Xw):
    Xc = Xw.astype(np.float64) @ Rm.T + t
    return np.stack([CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]], 1)


def _world(rng, Rm, t, n):
    z = rng.uniform(2.0, 12.0, n)
    Xc = np.stack([(rng.uniform(20, 300, n) - CAM[2]) / CAM[0] * z, (rng.uniform(20, 220, n) - CAM[3]) / CAM[1] * z, z], 1)
    return ((Xc - t) @ Rm).astype(F)


def make_pair(spec, cap, seed):
    """the key frame, the frame and the row between them"""
    rng = np.random.default_rng(seed)
    N = cap if spec.N is None else spec.N
    special = getattr(spec, "special", None)
    n_extra = 0 if N == cap else min(5, cap - N)                      # row entries that are no correspondence: -1, -2, >= N_kf, unheld, bad
    Nf = N + n_extra
    Rm, t = _rotation(rng, 25.0), rng.uniform(-0.5, 0.5, 3)
    Xw = _world(rng, Rm, t, Nf)
    if special == "duplicate":
        Xw[1] = Xw[0]
    uv = _project(Rm, t, Xw)
    inl = np.ones(Nf, bool)
    n_inl = N if getattr(spec, "inl", None) is None else spec.inl
    if special == "two_poses":                                       # 0-19 under pose A (exactly min_inliers), 20-40 under pose B
        R2, t2 = _rotation(rng, 25.0), rng.uniform(-0.5, 0.5, 3)
        Xw[20:] = _world(rng, R2, t2, Nf - 20)
        uv[20:] = _project(R2, t2, Xw[20:])
    else:
        inl[rng.permutation(N)[:N - n_inl]] = False
        if special == "duplicate":
            inl[:4] = True
    ang, rad = rng.uniform(0, 2 * math.pi, Nf), rng.uniform(30, 80, Nf)
    uv = np.where(inl[:, None], uv, uv + (rad * np.stack([np.cos(ang), np.sin(ang)])).T)
    perm = rng.permutation(Nf)                                        # frame feature i sees key-frame feature perm[i]
    kf, fr = types.SimpleNamespace(n=Nf), types.SimpleNamespace(n=Nf)
    for f in (kf, fr):
        f.keys = np.zeros(Nf, KEYPOINT_DTYPE)
        f.keys["x"], f.keys["y"] = rng.uniform(0, W, Nf).astype(F), rng.uniform(0, H, Nf).astype(F)
        f.keys["octave"], f.keys["size"], f.keys["class_id"] = rng.integers(0, 8, Nf), 31, -1
        f.world, f.valid, f.bad = np.zeros((Nf, 3), F), np.ones(Nf, np.uint8), np.zeros(Nf, np.uint8)
    kf.world[perm] = Xw
    fr.keys["x"], fr.keys["y"] = uv[:, 0].astype(F), uv[:, 1].astype(F)
    fr.world[:] = 77.0                                                # (the frame's own points are not read)
    row = np.full(cap, -1, np.int32)
    row[:Nf] = perm
    if n_extra:
        x = N + np.arange(n_extra)
        row[x[0]] = -1
        if n_extra > 1: row[x[1]] = -2
        if n_extra > 2: row[x[2]] = Nf + 3                            # >= N_kf
        if n_extra > 3: kf.valid[perm[x[3]]] = 0
        if n_extra > 4: kf.bad[perm[x[4]]] = 1
    return [kf, fr], row


def batch_arrays(frames, cap, img_stride=1):
    """(kps [n * img_stride, cap], counts, world [n, cap, 3], valid, bad [n, cap]); the odd images of a stride-2 batch hold decoys"""
    n = len(frames)
    kps, counts = np.zeros((n * img_stride, cap), KEYPOINT_DTYPE), np.zeros(n * img_stride, np.int32)
    kps["octave"] = 99
    world = np.zeros((n, cap, 3), F)
    valid, bad = np.zeros((n, cap), np.uint8), np.zeros((n, cap), np.uint8)
    for j, f in enumerate(frames):
        kps[j * img_stride, :f.n], counts[j * img_stride] = f.keys, f.n
        world[j, :f.n], valid[j, :f.n], bad[j, :f.n] = f.world, f.valid, f.bad
        if img_stride > 1:
            counts[j * img_stride + 1] = cap
    return kps, counts, world, valid, bad


def forced_draws(N, idx):
    """raw values whose four draws pick the indices idx"""
    avail, out = list(range(N)), []
    for i in idx:
        pos = avail.index(i)
        out.append(int(math.ceil(pos / len(avail) * 2147483648.0)))
        avail[pos] = avail[-1]
        avail.pop()
    return out


# The seed of each pair's draws, chosen (by trying seeds in turn, analyse_pair deciding) so that the builder's conditions hold under both parameter sets
DRAW_SEEDS = (0, 0, 0, 41, 78, 257, 34, 107, 107, 3, 43, 65, 67, 24, 79, 0, 0, 26)


def pair_draws(p, seed):
    d = np.random.default_rng(1000 * seed + p).integers(0, 1 << 31, size=(300, 4), dtype=np.uint32)
    if p == 15:
        d[0] = forced_draws(41, (2, 5, 7, 15))                        # four of pose A first: a sample every switch of the restatement counts as 20
        d[3] = forced_draws(41, (22, 25, 30, 36))                     # then four of pose B: 21
    if p == 17:
        d[0] = forced_draws(30, (0, 1, 2, 3))                         # the duplicated point and two more
    return d


@functools.lru_cache(maxsize=None)
def scene_set(cap=CAP, seed=23):
    sc = types.SimpleNamespace(frames=[], pairs=[], rows=[], cap=cap)
    for k, spec in enumerate(PAIR_SPECS):
        fr, row = make_pair(spec, cap, seed * 1000 + k)
        sc.frames += fr
        sc.pairs.append((2 * k, 2 * k + 1))
        sc.rows.append(row)
    sc.draws = np.stack([pair_draws(p, DRAW_SEEDS[p]) for p in range(len(sc.pairs))])
    sc.arrays = batch_arrays(sc.frames, cap)
    return sc


def corr(sc, p, th2=TH2, sf=SF, img_stride=1, arrays=None):
    kps, counts, world, valid, bad = arrays or sc.arrays
    return R.correspondences(kps, counts, world, valid, bad, sf, th2, sc.pairs[p], sc.rows[p], img_stride)


def near_flags(e2, maxerr):
    """correspondences whose error lies within a part in 2^10 of the gate: the restatement does not say on which side the library puts them"""
    with np.errstate(all="ignore"):
        return ~(np.abs(e2.astype(np.float64) - maxerr) > maxerr * 2.0 ** -10)


def analyse_pair(sc, p, alt=False, draws=None):
    """find() of pair p by the restatement, base and switched, with the builder's conditions asserted.  A namespace: C, out, st (base), log, settled
    (iterations whose count and variant agree under every switch and that hold no near correspondence), alts (the switched runs' outputs and states)"""
    prm, th2 = (ALT, ALT_TH2) if alt else (PARAMS, TH2)
    mi = prm["max_iterations"]
    draws = (sc.draws[p] if draws is None else draws)[:mi]
    C = corr(sc, p, th2)
    a = types.SimpleNamespace(C=C, log={}, st=R.new_state(), alts=[], settled=[])
    a.out = R.iterate(C, draws, a.st, 0, CAM, sw=R.BASE, log=a.log, **prm)
    for sw in R.SWITCHED:
        st2 = R.new_state()
        o2 = R.iterate(C, draws, st2, 0, CAM, sw=sw, **prm)
        assert (o2.accepted, o2.no_more, o2.refined, o2.n_inliers, st2.iterations_done, st2.best_inliers) == \
               (a.out.accepted, a.out.no_more, a.out.refined, a.out.n_inliers, a.st.iterations_done, a.st.best_inliers), (p, vars(sw))
        a.alts.append((o2, st2))
    best = 0
    for j in sorted(a.log):
        n, variant, e2, flags, rec, H = a.log[j]
        same = True
        for sw in R.SWITCHED:
            H2, f2, _, n2 = R.fit(C, R.sample(C.N, draws[j % mi]), CAM, sw)
            same &= n2 == n and H2.variant == variant
        if n >= a.out.min_eff and n > best:
            best = n
            assert same and not near_flags(e2, C.maxerr).any(), (p, j, "a record iteration is open")
        if rec is not None:
            assert not near_flags(rec[2], C.maxerr).any(), (p, j, "Refine holds a near correspondence")
        if same and not near_flags(e2, C.maxerr).any():
            a.settled.append(j)
    a.open_share = 1 - len(a.settled) / len(a.log) if a.log else 0.0
    return a


@functools.lru_cache(maxsize=None)
def analyse(alt=False, cap=CAP, seed=23):
    sc = scene_set(cap, seed)
    res = []
    for p in range(len(sc.pairs)):
        a = analyse_pair(sc, p, alt)
        print(f"pnp scene {p}{' alt' if alt else ''}: N {a.C.N}, {len(a.log)} iterations, open share {a.open_share:.2f}")
        res.append(a)
    return res
