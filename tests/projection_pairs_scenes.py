"""Cases for olf_search_by_projection_kf_pairs_dev and olf_search_by_projection_sim3_batch_dev (tests/test_projection_pairs_gpu.py): fabricated frames, one
scenario_* function per case.  Every scenario builds its case, takes what the GPU test compares against from the CPU oracle (oracle_lib.
search_by_projection_kf / search_by_projection_sim3, pair by pair) and asserts, from the oracle's output or from float32 arithmetic in numpy, that the case
really occurs.  Nothing here needs a device.
Frames are fabricated as in tests/sim3_pairs_scenes.py (320 x 240, fx = fy = 200, eight levels of 1.2), whose builders this module uses.  One map point
in seven is a "twin" of its predecessor -- two pixels away, a few bits apart -- so that points compete for key points and the order of the search shows."""
import copy
import functools
import types
import numpy as np
import orb_line_slam_amd as ola
import sim3_pairs_scenes as B
from sim3_pairs_scenes import BOUNDS, CAM, CX, CY, FX, FY, H, SF8, W, cut, f32, flip, hold, key_frame, pose  # noqa: F401  (re-exported for the tests)

COUNTS = (0, 1, 63, 64, 65, 300, 900)
TH_LOW = 50
FILL = -9                                              # what the rows hold before a call where nothing may be read or must stay
# relocalisation form, (current frame, key frame): the two big frames both ways, one pair twice (its two entries get two poses), every count on either side
RELOC_PAIRS = ((6, 5), (5, 6), (6, 5), (6, 4), (6, 3), (6, 2), (5, 4), (5, 3), (5, 2), (4, 5), (6, 0), (0, 6), (6, 1), (1, 5))
RELOC_THS = (10.0, 3.0)                                # src/Tracking.cc:2322, :2336
LOOP_THS = (10, 6)                                     # src/LoopClosing.cc:381 and a narrower one (the reference's th is an int)
SEED = 25                                              # chosen on the CPU with the oracle so that the assertions of the batch scenarios hold


def bits(base, idx):
    """the descriptor `base` with exactly the bits idx flipped"""
    d = np.array(base, np.uint8, copy=True).reshape(32)
    for b in idx:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def make_map(rng, n_map):
    """points in front of the identity camera; every seventh or so is a twin of its predecessor"""
    u, v, z = rng.uniform(12, 308, n_map), rng.uniform(12, 228, n_map), rng.uniform(4, 20, n_map)
    base = rng.integers(1, 4, n_map)
    desc = rng.integers(0, 256, (n_map, 32), dtype=np.uint8)
    ang = rng.uniform(0, 360, n_map)
    for k in np.flatnonzero(rng.random(n_map) < 1 / 7):
        if k:
            u[k], v[k], z[k] = np.clip(u[k - 1] + rng.uniform(-2, 2), 12, 308), np.clip(v[k - 1] + rng.uniform(-2, 2), 12, 228), z[k - 1]
            base[k], ang[k] = base[k - 1], ang[k - 1]
            desc[k] = flip(rng, desc[k - 1], rng.integers(4, 12))[0]
    X = np.stack([(u - CX) * z / FX, (v - CY) * z / FY, z], 1)
    return types.SimpleNamespace(X=X, base=base, desc=desc, ang=ang, n=n_map)


def observe(rng, mp, T, n, jitter=4.0, angle0=0.0, kappa=0):
    """a key frame of n key points that observe the map from pose T (camera = R X + t): position = projection + jitter, octave around the point's level,
    +-2, descriptor a few bits from the point's (one in seven random), angle = the point's + angle0 + noise (one in twelve random); one key point in eight
    observes a point a second time.  It holds no point yet"""
    Xc = mp.X @ T[:3, :3].T + T[:3, 3]
    pu, pv = FX * Xc[:, 0] / Xc[:, 2] + CX, FY * Xc[:, 1] / Xc[:, 2] + CY
    vis = np.flatnonzero((Xc[:, 2] > 0) & (pu > 6) & (pu < 314) & (pv > 6) & (pv < 234))
    vis = vis[vis < max(120, int(1.4 * n))]                  # (nested pools: the small frames share the first points of the map)
    assert len(vis) >= n
    first = rng.permutation(vis)[:n - n // 8]                # (one key point in eight is a second detection of a point the frame sees already)
    src = rng.permutation(np.concatenate([first, rng.choice(first, n // 8, replace=False)]))
    octave = np.clip(mp.base[src] + kappa + rng.choice([-2, -1, -1, 0, 0, 0, 0, 1], n), 0, 7)
    keys = np.stack([pu[src] + rng.uniform(-jitter, jitter, n), pv[src] + rng.uniform(-jitter, jitter, n), octave], 1) if n else np.zeros((0, 3))
    desc = flip(rng, mp.desc[src], rng.integers(0, 12, n))
    far = rng.random(n) < 1 / 7
    desc[far] = rng.integers(0, 256, (int(far.sum()), 32), dtype=np.uint8)
    kf = key_frame(keys, desc, T)
    ang = (mp.ang[src] + angle0 + rng.normal(0, 4, n)) % 360.0
    wild = rng.random(n) < 1 / 12
    ang[wild] = rng.uniform(0, 360, int(wild.sum()))
    kf.mvKeysUn["angle"] = ang.astype(f32)
    kf.src, kf.octave, kf.dist = src, octave, np.linalg.norm(Xc[src], axis=1)
    return kf


# ---- the relocalisation form ----------------------------------------------------------------------------------------------------------------------------
def current_view(frame, Tcw, cur_valid):
    """`frame` in the CurrentFrame role of one candidate: its own pose and its own copy of mvpMapPoints (a mask)"""
    c = copy.copy(frame)
    c.mTcw = np.ascontiguousarray(Tcw, f32)
    c.mp_valid = np.array(cur_valid, bool, copy=True)
    return c


def expect_reloc_pair(oracle, cur, kf, found, th, orb, ori, cap):
    """(row over the capacity, nmatches) the entry must leave for one pair"""
    if cur.N == 0 or kf.N == 0:
        return np.full(cap, -1, np.int32), 0
    n, m = oracle.search_by_projection_kf(cur, kf, np.ascontiguousarray(found, np.uint8), float(th), int(orb), bool(ori))
    return np.concatenate([np.asarray(m, np.int32), np.full(cap - cur.N, -1, np.int32)]), int(n)


def expect_reloc(oracle, s, th, ori, cap, ths=None, orbs=None):
    rows = [expect_reloc_pair(oracle, s.curs[p], s.kfs[b], s.found[p], th if ths is None else ths[p], s.orbs[p] if orbs is None else orbs[p], ori, cap)
            for p, (a, b) in enumerate(s.pairs)]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.int32)


def make_reloc_scene(seed, cap, counts=COUNTS, n_map=1300, pairs=RELOC_PAIRS):
    rng = np.random.default_rng(seed)
    mp = make_map(rng, n_map)
    kfs = []
    for j, n in enumerate(counts):
        kf = observe(rng, mp, B.POSES[j % len(B.POSES)], n, angle0=25.0 * j)
        held = np.flatnonzero(rng.random(n) < 0.9)
        maxd = kf.dist[held] * SF8[kf.octave[held]] * rng.uniform(0.88, 0.99, len(held))
        hold(kf, held, mp.X[kf.src[held]], maxd, maxd / SF8[-1], flip(rng, mp.desc[kf.src[held]], rng.integers(0, 4, len(held))))
        kf.mp_bad[held] = rng.random(len(held)) < 0.05
        kfs.append(kf)
    s = types.SimpleNamespace(kfs=kfs, pairs=list(pairs), mp=mp)
    reroll_reloc_pairs(s, rng)
    return s


def reroll_reloc_pairs(s, rng):
    """per pair: the candidate's pose of the current frame (its own, perturbed as a PnP solution would be), the features of the current frame that hold a
    point already, sAlreadyFound over the key frame's features, ORBdist 100 / 64"""
    s.poses, s.cur_valid, s.found, s.orbs, s.curs = [], [], [], [], []
    for p, (a, b) in enumerate(s.pairs):
        T = s.kfs[a].mTcw.astype(np.float64) @ pose(*rng.uniform(-0.01, 0.01, 3), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1))
        s.poses.append(np.ascontiguousarray(T, f32))
        s.cur_valid.append(rng.random(s.kfs[a].N) < 0.1)
        s.found.append(rng.random(s.kfs[b].N) < 0.05)
        s.orbs.append(100 if p % 2 == 0 else 64)
        s.curs.append(current_view(s.kfs[a], s.poses[p], s.cur_valid[p]))


def displaced_point(oracle, cur, kf, found, th, orb):
    """a key-frame feature that, searched alone, takes a key point which the full search gave to an EARLIER feature, and that ends on another key point:
    (i, first choice, the earlier feature, what i got), or None"""
    n, full = oracle.search_by_projection_kf(cur, kf, np.ascontiguousarray(found, np.uint8), float(th), int(orb), False)
    got = {int(i): i2 for i2, i in enumerate(full) if i >= 0}
    for i in sorted(got):
        solo = copy.copy(kf)
        solo.mp_valid = np.zeros(kf.N, bool)
        solo.mp_valid[i] = True
        _, m1 = oracle.search_by_projection_kf(cur, solo, np.ascontiguousarray(found, np.uint8), float(th), int(orb), False)
        first = int(np.flatnonzero(m1 >= 0)[0])
        if first != got[i]:
            assert 0 <= full[first] < i, (i, first, full[first])
            return i, first, int(full[first]), got[i]
    return None


@functools.lru_cache(maxsize=None)
def scenario_reloc_batch(cap):
    """1: the seven frames, the fourteen pairs, th = 10 and 3, ORBdist 100 / 64 per pair, both settings of the orientation check"""
    import oracle_lib as oracle
    s = make_reloc_scene(SEED, cap)
    s.exp = {(th, ori): expect_reloc(oracle, s, th, ori, cap) for th in RELOC_THS for ori in (0, 1)}
    n10 = s.exp[(10.0, 1)][1]
    assert 2 * int((n10 >= 20).sum()) >= len(s.pairs), n10                                    # at least half of the pairs end with 20 or more matches
    assert any((s.exp[(th, 0)][1] > s.exp[(th, 1)][1]).any() for th in RELOC_THS), "the rotation check rejected nothing"
    assert not np.array_equal(s.exp[(10.0, 1)][0], s.exp[(3.0, 1)][0])                           # (the narrower window changes results)
    assert not np.array_equal(s.exp[(10.0, 1)][0][0], s.exp[(10.0, 1)][0][2])                    # (the same pair under two poses)
    assert any(v.any() for v in s.cur_valid) and any(v.any() for v in s.found)
    s.displaced = displaced_point(oracle, s.curs[0], s.kfs[s.pairs[0][1]], s.found[0], 10.0, s.orbs[0])
    assert s.displaced is not None, "no later point was displaced to its second choice"
    return s


@functools.lru_cache(maxsize=None)
def scenario_reloc_counts(cap):
    """the same kind of scene with the last frame filled to the capacity (its count will overstate it) and frame 4 cut to 40 of its 65"""
    import oracle_lib as oracle
    s = make_reloc_scene(SEED + 1, cap, counts=COUNTS[:6] + (cap,), n_map=2200, pairs=((6, 5), (5, 6), (6, 4), (4, 6)))
    s.views = list(s.kfs)
    s.views[4] = cut(s.kfs[4], 40)
    s.counts = [None] * 4 + [40, None, cap + 1000]
    full = s.kfs
    s.kfs = s.views
    reroll_reloc_pairs(s, np.random.default_rng(6))
    s.exp = expect_reloc(oracle, s, 10.0, 1, cap)
    s.kfs = full
    assert s.exp[1][0] >= 20 and (s.exp[0][0, 900:] >= 0).any() and (s.exp[0][1] >= 900).any()      # (features beyond 900 take part on both sides)
    return s


# ---- hand-built cases, relocalisation form: identity pose, camera = world coordinates -------------------------------------------------------------------
def proj_reloc(p):
    """(u, v) of a camera point in the arithmetic of reloc_point_gate: fx * xc * invzc + cx, left to right in float32, NO sign test"""
    p = np.asarray(p, f32)
    invz = f32(1.0 / np.float64(p[2]))
    return f32(f32(f32(f32(FX) * p[0]) * invz) + f32(CX)), f32(f32(f32(f32(FY) * p[1]) * invz) + f32(CY))


def level_interval(dist, level):
    """(mfMaxDistance, mfMinDistance) that predict `level` at distance dist, far from the level's thresholds and from the ends of the interval"""
    maxd = float(dist) * (0.9 if level == 0 else 1.2 ** (level - 0.5))
    return maxd, maxd / 3.5


def at(u, v, z):
    return [(u - CX) * z / FX, (v - CY) * z / FY, z]


def edge(proj, axis, bound, z=5.0):
    """(on, out): coordinate `axis` of a camera point at depth z whose projection is exactly `bound`, and the nearest float beyond it whose projection
    is not -- found by stepping through the floats around the exact solution (z = 5: the bounds are then met by x = -+4, y = -+3 exactly)"""
    f, c = (FX, CX) if axis == 0 else (FY, CY)
    x = f32((bound - c) * z / f)
    p = lambda t: proj([t, 0.0, z] if axis == 0 else [0.0, t, z])[axis]
    sign = 1.0 if bound > c else -1.0
    lo = x
    for _ in range(64):                                     # back to a float that lands on the bound
        if p(lo) == f32(bound):
            break
        lo = np.nextafter(lo, f32(0))
    assert p(lo) == f32(bound), (axis, bound)
    out = lo
    for _ in range(64):
        out = np.nextafter(out, f32(sign * 100))
        if p(out) != f32(bound):
            break
    assert sign * (float(p(out)) - bound) > 0
    return float(lo), float(out)


def _reloc_case(name, pts, levels, pdesc, cur_keys, cur_desc, want, th=10.0, orb=100, kf_angles=None, cur_angles=None, cur_valid=None, found=None,
                bad=None, unheld=(), want_n=None, want_ori=None, interval=None):
    """the key frame holds pts (camera = world coordinates) with the descriptors pdesc and the intervals of `levels`; the current frame has the key points
    cur_keys (x, y, octave) with the descriptors cur_desc.  want: the row over the current frame's features without the orientation check"""
    n = len(pts)
    kf = key_frame([(160.0, 120.0, 3)] * n, pdesc)
    iv = [level_interval(np.linalg.norm(np.asarray(p, np.float64)), lv) for p, lv in zip(pts, levels)] if interval is None else interval
    hold(kf, np.arange(n), pts, [a for a, b in iv], [b for a, b in iv], pdesc)
    for i in unheld:
        kf.mp_valid[i] = False
    if bad is not None:
        kf.mp_bad[:] = bad
    if kf_angles is not None:
        kf.mvKeysUn["angle"] = np.asarray(kf_angles, f32)
    cur = key_frame(cur_keys, cur_desc)
    if cur_angles is not None:
        cur.mvKeysUn["angle"] = np.asarray(cur_angles, f32)
    cv = np.zeros(cur.N, bool) if cur_valid is None else np.asarray(cur_valid, bool)
    return types.SimpleNamespace(name=name, kf=kf, cur=current_view(cur, np.eye(4, dtype=f32), cv), cur_valid=cv, th=th, orb=orb,
                                 found=np.zeros(n, bool) if found is None else np.asarray(found, bool), want=list(want), want_n=want_n, want_ori=want_ori)


@functools.lru_cache(maxsize=None)
def scenario_reloc_gates(cap):
    """2: every gate at its edge and the order dependence, each case a pair; `want` is worked out by hand and asserted against the oracle here"""
    import oracle_lib as oracle
    rng = np.random.default_rng(707)
    D = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    cases = []
    # two points whose best key point is K0.  P0 = D, K0 = D ^ 2 bits, P1 = D ^ 4 other bits, K1 = P1 ^ 60 further bits: dist(P0, K0) = 2, (P1, K0) = 6,
    # (P1, K1) = 60, (P0, K1) = 64; ORBdist = 62.  P0 first: K0 <- P0, K1 <- P1.  P1 first: it takes K0, and P0 finds K0 closed and K1 too far
    d = D()
    p0, k0, p1 = d, bits(d, [0, 1]), bits(d, [2, 3, 4, 5])
    k1 = bits(p1, range(6, 66))
    pts = [at(150.0, 100.0, 8.0), at(151.0, 100.5, 8.0)]
    keys = [(150.5, 100.0, 3), (151.5, 101.0, 3)]
    cases.append(_reloc_case("order_first", pts, [3, 3], [p0, p1], keys, [k0, k1], [0, 1], orb=62, want_n=2))
    cases.append(_reloc_case("order_second", pts[::-1], [3, 3], [p1, p0], keys, [k0, k1], [0, -1], orb=62, want_n=1))
    # the recompute path: Q = D, K_j = D ^ (j + 1) bits of its own (j = 0 .. 4), P_j = K_j (j = 0 .. 3) come first and take K_0 .. K_3 at distance 0;
    # Q keeps K_0 .. K_3, finds all four closed, and must end with K_4
    d = D()
    ks = [bits(d, range(16 * j, 16 * j + j + 1)) for j in range(5)]
    pts = [at(200.0 + 0.5 * j, 150.0, 8.0) for j in range(5)]
    keys = [(199.0 + j, 150.5 - 0.25 * j, 3) for j in range(5)]
    cases.append(_reloc_case("recompute", pts, [3] * 5, ks[:4] + [d], keys, ks, [0, 1, 2, 3, 4], want_n=5))
    # a key point closed on entry that would have been best: K0 at distance 2 holds a point already, K1 at distance 9 is taken
    d = D()
    cases.append(_reloc_case("closed_on_entry", [at(100.0, 60.0, 8.0)], [3], [d], [(100.5, 60.0, 3), (101.0, 61.0, 3)], [bits(d, [0, 1]), bits(d, range(9))],
                             [-1, 0], cur_valid=[True, False], want_n=1))
    # sAlreadyFound, a bad point and a feature without a point: three of four points at four places are left out
    ds = [D() for _ in range(4)]
    pts = [at(60.0 + 60 * k, 200.0, 8.0) for k in range(4)]
    keys = [(60.5 + 60 * k, 200.5, 3) for k in range(4)]
    cases.append(_reloc_case("found_bad_unheld", pts, [3] * 4, ds, keys, [bits(x, [7]) for x in ds], [-1, -1, -1, 3], found=[True, False, False, False],
                             bad=[False, True, False, False], unheld=[2], want_n=1))
    # the CLOSED image bounds: a projection exactly on the bound is taken, the next float beyond it is not.  Each point has a key point of its own
    for axis, bound, name in ((0, 320.0, "maxX"), (0, 0.0, "minX"), (1, 240.0, "maxY"), (1, 0.0, "minY")):
        on, out = edge(proj_reloc, axis, bound)
        mk = (lambda t, o: [t, o, 5.0]) if axis == 0 else (lambda t, o: [o, t, 5.0])
        pts = [mk(on, -1.2), mk(out, 1.2)]                   # (the other coordinate: v = 72 / 168, or u = 112 / 208)
        uv = [proj_reloc(p) for p in pts]
        assert uv[0][axis] == f32(bound) and uv[1][axis] != f32(bound)
        inside = lambda t, hi: float(min(max(t, 2.0), hi - 6.0))      # (a key point within 2.5 px of maxX / maxY rounds into a cell outside mGrid)
        keys = [(inside(float(a), 320.0), inside(float(b), 240.0), 3) for a, b in uv]
        ds = [D(), D()]
        cases.append(_reloc_case(f"bounds_{name}", pts, [3, 3], ds, keys, [bits(x, [3]) for x in ds], [0, -1], want_n=1))
    # the distance interval to the ulp: dist3D (= z exactly on the optical axis) at 0.8f * mind and at 1.2f * maxd is taken, one ulp outside is not
    lo, hi = f32(f32(0.8) * f32(10.0)), f32(f32(1.2) * f32(6.5))
    assert lo == f32(8.0)
    for name, zs, iv, level in (("distance_min", (lo, np.nextafter(lo, f32(0))), (8 * B.LEVEL3, 10.0), 3),
                                ("distance_max", (hi, np.nextafter(hi, f32(100))), (6.5, 1.0), 0)):
        for z, taken in zip(zs, (True, False)):
            d = D()
            cases.append(_reloc_case(f"{name}_{'in' if taken else 'out'}", [[0.0, 0.0, float(z)]], [level], [d], [(160.5, 120.25, level)], [bits(d, [1])],
                                     [0 if taken else -1], interval=[iv], want_n=int(taken)))
    # the window's levels nPredictedLevel - 1 .. nPredictedLevel + 1, at level 0 and at the top level: four points at four places, one key point each
    for name, level, octs, want in (("level_0", 0, (0, 1, 2, 3), [0, 1, -1, -1]), ("level_top", 7, (5, 6, 7, 4), [-1, 1, 2, -1])):
        ds = [D() for _ in range(4)]
        pts = [at(50.0 + 70 * k, 60.0, 8.0) for k in range(4)]
        keys = [(50.5 + 70 * k, 60.5, o) for k, o in enumerate(octs)]
        cases.append(_reloc_case(name, pts, [level] * 4, ds, keys, [bits(x, [5]) for x in ds], want, want_n=sum(w >= 0 for w in want)))
    # a distance equal to ORBdist is accepted, one above it is not
    ds = [D(), D()]
    pts = [at(100.0, 80.0, 8.0), at(200.0, 80.0, 8.0)]
    cases.append(_reloc_case("orb_dist", pts, [3, 3], ds, [(100.5, 80.5, 3), (200.5, 80.5, 2)], [bits(ds[0], range(64)), bits(ds[1], range(65))], [0, -1],
                             orb=64, want_n=1))
    # two candidates at distance 3: key point 1 lies in grid column 30, key point 0 in column 31 (cells of 5 px, rounded), so the scan meets 1 first
    d = D()
    cases.append(_reloc_case("tie_scan_order", [at(151.0, 111.0, 8.0)], [3], [d], [(153.0, 110.0, 3), (149.0, 112.0, 3)],
                             [bits(d, [0, 1, 2]), bits(d, [3, 4, 5])], [-1, 0], want_n=1))
    # a point BEHIND the camera whose projection lands inside the image is searched: (1, -1, -4) -> invzc = -0.25, u = 110, v = 170
    d = D()
    p = [1.0, -1.0, -4.0]
    assert proj_reloc(p) == (f32(110.0), f32(170.0))
    cases.append(_reloc_case("negative_depth", [p], [3], [d], [(110.5, 170.0, 3)], [bits(d, [2])], [0], want_n=1))
    # four matches in four rotation bins (0, 1, 2, 3): ComputeThreeMaxima keeps the first three, the fourth row returns to -1 and the count drops
    ds = [D() for _ in range(4)]
    pts = [at(60.0 + 60 * k, 30.0, 8.0) for k in range(4)]
    keys = [(60.5 + 60 * k, 30.5, 3) for k in range(4)]
    cases.append(_reloc_case("rotation_rejected", pts, [3] * 4, ds, keys, [bits(x, [9]) for x in ds], [0, 1, 2, 3], kf_angles=[0.0, 30.0, 60.0, 90.0],
                             cur_angles=[0.0] * 4, want_n=4, want_ori=([0, 1, 2, -1], 3)))
    for c in cases:
        c.exp = {ori: expect_reloc_pair(oracle, c.cur, c.kf, c.found, c.th, c.orb, ori, cap) for ori in (0, 1)}
        row, n = c.exp[0]
        assert list(row[:c.cur.N]) == c.want and n == c.want_n, (c.name, row[:c.cur.N], n)
        if c.want_ori:
            row, n = c.exp[1]
            assert (list(row[:c.cur.N]), n) == c.want_ori, (c.name, row[:c.cur.N], n)
    return cases


# ---- the loop form --------------------------------------------------------------------------------------------------------------------------------------
SIGMA = (1.0, 2.0, 1.0, 0.5, 1.37, 1.0, 2.0)           # the scale of each key frame's Sim3 pose


def sim3_pose(T, s):
    """Scw = [s R | t]: the decomposition gives Rcw = R, tcw = t / s"""
    S = np.array(T, np.float64)
    S[:3, :3] *= s
    return np.ascontiguousarray(S, f32)


def loop_geom(mp, order, skip):
    return ola.MapPointGeom(mp.world[order], mp.normal[order], mp.maxd[order], mp.mind[order], mp.desc[order], skip=skip)


def expect_loop_frame(oracle, kf, Scw, mp, order, fm, th, cap, n_mp=None):
    """(the row of d_frame_matched after the call over the capacity, nmatches) for one key frame: `order` its list of map indices, fm its row on entry"""
    order = np.asarray(order, np.int64)
    n_mp = mp.n if n_mp is None else n_mp
    fm = np.asarray(fm, np.int32)
    out = fm.copy()
    ok = (order >= 0) & (order < n_mp)                        # (a list index outside the map is left out)
    order = order[ok]
    if kf.N == 0 or len(order) == 0:
        return out, 0
    held = np.zeros(mp.n, bool)
    hv = fm[:kf.N]
    held[hv[(hv >= 0) & (hv < n_mp)]] = True
    n, km, _ = oracle.search_by_projection_sim3(kf, Scw, loop_geom(mp, order, mp.bad[order] | held[order]), hv != -1, int(th))
    took = np.flatnonzero(km >= 0)
    out[took] = order[km[took]]
    return out, int(n)


def make_loop_scene(seed, cap, counts=COUNTS, n_map=1300):
    """a map in the unit of the identity camera and key frames that observe it under Sim3 poses of scale SIGMA; every key frame has its own list of points
    (a shuffled subset: the reference's order is the list's) and holds some matches on entry"""
    rng = np.random.default_rng(seed)
    m = make_map(rng, n_map)
    dist = np.linalg.norm(m.X, axis=1)
    nrm = m.X / dist[:, None] + rng.normal(0, 0.05, m.X.shape)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    maxd = dist * SF8[m.base] * rng.uniform(0.88, 0.99, n_map)
    mp = types.SimpleNamespace(world=np.ascontiguousarray(m.X, f32), normal=np.ascontiguousarray(nrm, f32), maxd=maxd.astype(f32),
                               mind=(maxd / SF8[-1]).astype(f32), desc=m.desc, bad=rng.random(n_map) < 0.05, n=n_map)
    kfs, Scw, lists, fms = [], [], [], []
    for j, n in enumerate(counts):
        T = B.POSES[j % len(B.POSES)]
        kf = observe(rng, m, T, n, jitter=8.0)
        kfs.append(kf)
        Ts = np.array(T)                                      # camera = R X + t is what the decomposition of [s R | s t] gives
        Ts[:3, 3] *= SIGMA[j % len(SIGMA)]
        Scw.append(sim3_pose(Ts, SIGMA[j % len(SIGMA)]))
        pool = np.arange(max(120, int(1.4 * n))) if n else np.arange(50)
        lists.append(rng.permutation(pool)[:max(int(0.8 * len(pool)), 1)].astype(np.int32))
        fm = np.full(cap, FILL, np.int32)
        r = rng.random(n)
        fm[:n] = np.where(r < 0.2, kf.src, np.where(r < 0.25, -2, -1))
        fms.append(fm)
    return types.SimpleNamespace(kfs=kfs, Scw=Scw, lists=lists, fms=fms, mp=mp)


def expect_loop(oracle, s, th, cap, lists=None, n_mp=None):
    lists = s.lists if lists is None else lists
    rows = [expect_loop_frame(oracle, kf, S, s.mp, l, fm, th, cap, n_mp) for kf, S, l, fm in zip(s.kfs, s.Scw, lists, s.fms)]
    return np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.int32)


@functools.lru_cache(maxsize=None)
def scenario_loop_batch(cap):
    """1, loop form: the seven key frames with their lists and pre-matched rows, th = 10 and 6"""
    import oracle_lib as oracle
    s = make_loop_scene(SEED + 2, cap)
    s.exp = {th: expect_loop(oracle, s, th, cap) for th in LOOP_THS}
    n10 = s.exp[10][1]
    assert n10[0] == 0 and 2 * int((n10 >= 20).sum()) >= len(n10), n10      # at least half of the key frames end with 20 or more matches
    assert not np.array_equal(s.exp[10][0], s.exp[6][0])       # (the narrower window changes results)
    assert any((fm >= 0).any() for fm in s.fms) and any((fm == -2).any() for fm in s.fms)
    return s


@functools.lru_cache(maxsize=None)
def scenario_loop_counts(cap):
    """the same kind of scene with the last key frame filled to the capacity (its count will overstate it) and key frame 4 cut to 40 of its 65"""
    import oracle_lib as oracle
    s = make_loop_scene(SEED + 3, cap, counts=COUNTS[:6] + (cap,), n_map=2200)
    s.full = list(s.kfs)
    s.kfs[4] = cut(s.kfs[4], 40)
    s.counts = [None] * 4 + [40, None, cap + 1000]
    s.exp = expect_loop(oracle, s, 10, cap)
    took = s.exp[0][6] != s.fms[6]
    assert took[900:].any() and s.exp[1][4] >= 5 and (s.exp[0][4][40:] == s.fms[4][40:]).all()      # (key points beyond 900 take part; beyond 40 none does)
    return s


def _loop_case(name, pts, levels, pdesc, keys, kdesc, want, fm=None, normals=None, bad=None, interval=None, want_n=None, scale=2.0):
    """one key frame under the pose [scale * I | 0] (camera = world coordinates) with the key points `keys`, against the points pts in list order.
    want: what the key points hold after the call (indices into pts)"""
    n = len(pts)
    P = np.asarray(pts, np.float64).reshape(n, 3)
    iv = [level_interval(np.linalg.norm(p), lv) for p, lv in zip(P, levels)] if interval is None else interval
    nr = P / np.linalg.norm(P, axis=1)[:, None] if normals is None else np.asarray(normals, np.float64)      # (default: PO . Pn = dist3D)
    mp = types.SimpleNamespace(world=np.ascontiguousarray(P, f32), normal=np.ascontiguousarray(nr, f32), maxd=np.asarray([a for a, b in iv], f32),
                               mind=np.asarray([b for a, b in iv], f32), desc=np.ascontiguousarray(np.stack(pdesc), np.uint8),
                               bad=np.zeros(n, bool) if bad is None else np.asarray(bad, bool), n=n)
    kf = key_frame(keys, np.stack(kdesc))
    fm = np.full(kf.N, -1, np.int32) if fm is None else np.asarray(fm, np.int32)
    return types.SimpleNamespace(name=name, kf=kf, mp=mp, Scw=sim3_pose(np.eye(4), scale), fm=fm, want=list(want), want_n=want_n)


@functools.lru_cache(maxsize=None)
def scenario_loop_gates(cap):
    """2, loop form: the gates of fuse_core with `matched` at their edges and the order dependence, each case a key frame with a map of its own"""
    import oracle_lib as oracle
    rng = np.random.default_rng(909)
    D = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    cases = []
    # two points whose best key point is K0 (distances as in the relocalisation case, K1 at 44 / 48 around TH_LOW - 4): the order decides
    d = D()
    p0, k0, p1 = d, bits(d, [0, 1]), bits(d, [2, 3, 4, 5])
    k1 = bits(p1, range(6, 54))                              # dist(P1, K1) = 48, dist(P0, K1) = 52 > TH_LOW
    pts = [at(150.0, 100.0, 8.0), at(151.0, 100.5, 8.0)]
    keys = [(150.5, 100.0, 3), (151.5, 101.0, 3)]
    cases.append(_loop_case("order_first", pts, [3, 3], [p0, p1], keys, [k0, k1], [0, 1], want_n=2))
    cases.append(_loop_case("order_second", pts[::-1], [3, 3], [p1, p0], keys, [k0, k1], [0, -1], want_n=1))
    # the recompute path, as in the relocalisation form
    d = D()
    ks = [bits(d, range(16 * j, 16 * j + j + 1)) for j in range(5)]
    pts = [at(200.0 + 0.5 * j, 150.0, 8.0) for j in range(5)]
    keys = [(199.0 + j, 150.5 - 0.25 * j, 3) for j in range(5)]
    cases.append(_loop_case("recompute", pts, [3] * 5, ks[:4] + [d], keys, ks, [0, 1, 2, 3, 4], want_n=5))
    # a key point closed on entry (it holds a point outside the map, -2) that would have been best; a point in spAlreadyFound (key point 2 holds point 1)
    # and a bad point (2) are left out although key points 3 and 4 wait for them
    ds = [D() for _ in range(3)]
    pts = [at(100.0, 60.0, 8.0), at(200.0, 60.0, 8.0), at(260.0, 60.0, 8.0)]
    keys = [(100.5, 60.0, 3), (101.0, 61.0, 3), (30.0, 200.0, 3), (200.5, 60.0, 3), (260.5, 60.0, 3)]
    kd = [bits(ds[0], [0, 1]), bits(ds[0], range(9)), D(), bits(ds[1], [4]), bits(ds[2], [4])]
    cases.append(_loop_case("closed_found_bad", pts, [3] * 3, ds, keys, kd, [-2, 0, 1, -1, -1], fm=[-2, -1, 1, -1, -1], bad=[False, False, True], want_n=1))
    # KeyFrame::IsInImage is HALF-OPEN: u == minX is inside and the next float below is not; u == maxX is outside and the next float below is inside
    on0, out0 = edge(B._proj, 0, 0.0)
    on1, in1 = edge(B._proj, 0, 320.0)
    in1 = float(np.nextafter(f32(on1), f32(0)))
    while B._proj([in1, 0.0, 5.0])[0] >= f32(320.0):
        in1 = float(np.nextafter(f32(in1), f32(0)))
    pts = [[on0, -1.2, 5.0], [out0, 1.2, 5.0], [on1, -0.4, 5.0], [in1, 0.4, 5.0]]
    assert B._proj(pts[0])[0] == f32(0.0)
    assert B._proj(pts[1])[0] < 0 and B._proj(pts[2])[0] == f32(320.0) and B._proj(pts[3])[0] < f32(320.0)
    ds = [D() for _ in range(4)]
    keys = [(2.0, 72.0, 3), (2.0, 168.0, 3), (314.0, 104.0, 3), (314.0, 136.0, 3)]
    cases.append(_loop_case("bounds_x", pts, [3] * 4, ds, keys, [bits(x, [3]) for x in ds], [0, -1, -1, 3], want_n=2))
    # the depth gate: z < 0 is rejected (this form has one); the decoy sits where a sign-blind projection would land
    d = D()
    cases.append(_loop_case("depth", [[1.0, -1.0, -4.0]], [3], [d], [(110.5, 170.0, 3)], [bits(d, [2])], [-1], want_n=0))
    # the distance interval to the ulp (Ow = 0: dist3D = z on the optical axis)
    lo, hi = f32(f32(0.8) * f32(10.0)), f32(f32(1.2) * f32(6.5))
    for name, zs, iv, level in (("distance_min", (lo, np.nextafter(lo, f32(0))), (8 * B.LEVEL3, 10.0), 3),
                                ("distance_max", (hi, np.nextafter(hi, f32(100))), (6.5, 1.0), 0)):
        for z, taken in zip(zs, (True, False)):
            d = D()
            cases.append(_loop_case(f"{name}_{'in' if taken else 'out'}", [[0.0, 0.0, float(z)]], [level], [d], [(160.5, 120.25, level)], [bits(d, [1])],
                                    [0 if taken else -1], interval=[iv], want_n=int(taken)))
    # the level gate nPredictedLevel - 1 <= octave <= nPredictedLevel at level 0 (octave -1 passes, as in the host form) and at the top level
    for name, level, octs, want in (("level_0", 0, (0, -1, 1, 2), [0, 1, -1, -1]), ("level_top", 7, (5, 6, 7, 4), [-1, 1, 2, -1])):
        ds = [D() for _ in range(4)]
        pts = [at(50.0 + 70 * k, 60.0, 8.0) for k in range(4)]
        keys = [(50.5 + 70 * k, 60.5, o) for k, o in enumerate(octs)]
        cases.append(_loop_case(name, pts, [level] * 4, ds, keys, [bits(x, [5]) for x in ds], want, want_n=sum(w >= 0 for w in want)))
    # a distance equal to TH_LOW is taken, one above it is not
    ds = [D(), D()]
    pts = [at(100.0, 80.0, 8.0), at(200.0, 80.0, 8.0)]
    cases.append(_loop_case("th_low", pts, [3, 3], ds, [(100.5, 80.5, 3), (200.5, 80.5, 2)], [bits(ds[0], range(TH_LOW)), bits(ds[1], range(TH_LOW + 1))],
                            [0, -1], want_n=1))
    # equal distances: the earlier scan position (grid column 30 before 31) wins
    d = D()
    cases.append(_loop_case("tie_scan_order", [at(151.0, 111.0, 8.0)], [3], [d], [(153.0, 110.0, 3), (149.0, 112.0, 3)],
                            [bits(d, [0, 1, 2]), bits(d, [3, 4, 5])], [-1, 0], want_n=1))
    for c in cases:
        c.exp = expect_loop_frame(oracle, c.kf, c.Scw, c.mp, np.arange(c.mp.n), np.concatenate([c.fm, np.full(cap - c.kf.N, FILL, np.int32)]), 10, cap)
        assert list(c.exp[0][:c.kf.N]) == c.want and c.exp[1] == c.want_n, (c.name, c.exp[0][:c.kf.N], c.exp[1])
    return cases
