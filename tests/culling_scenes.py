"""Map snapshots for the KeyFrameCulling / MapPointCulling / TrackedMapPoints tests: a scene holds what an olf_map_graph and an olf_cull_view say about the
points (observations with their slots, isBad(), Observations()) and about the key frames' slots (point, octave, depth, stereo flag), and turns into the
arguments of MapGraph / CullView and into the plain lists tests/culling_reference.py walks.  Hand-worked scenes, each the smallest at which one rule of
src/LocalMapping.cc:632-696 can go wrong and each with its expected answer printed beside it, and seeded random graphs (n_kf <= 300, n_mp <= 300, rows of at
most 2000 slots: the sizes of connections_scenes.py)."""
import copy
import numpy as np

TH_DEPTH = 35.0                                                      # mThDepth of every key frame unless a scene says otherwise
NEAR, FAR = 10.0, 50.0


class CullScene:
    def __init__(self, n_kf):
        self.n_kf = n_kf
        self.kf_mp = [[] for _ in range(n_kf)]                      # per slot: the point, -1 = NULL
        self.kf_oct = [[] for _ in range(n_kf)]
        self.kf_depth = [[] for _ in range(n_kf)]
        self.kf_stereo = [[] for _ in range(n_kf)]
        self.th_depth = [TH_DEPTH] * n_kf
        self.mode = [0] * n_kf
        self.mp_obs = []                                             # per point: [key frame, slot] pairs
        self.mp_bad = []
        self.mp_nobs = []
        self.kf_ml = None                                            # lines, for TrackedMapLines only
        self.ml_bad = None
        self.ml_nobs = None

    @property
    def n_mp(self):
        return len(self.mp_bad)

    def slot(self, kf, point=-1, octave=0, depth=NEAR, stereo=0):
        """one more slot of key frame kf; returns its index"""
        self.kf_mp[kf].append(point); self.kf_oct[kf].append(octave); self.kf_depth[kf].append(depth); self.kf_stereo[kf].append(stereo)
        return len(self.kf_mp[kf]) - 1

    def new_point(self, bad=0):
        self.mp_obs.append([]); self.mp_bad.append(bad); self.mp_nobs.append(0)
        return self.n_mp - 1

    def observe(self, p, kf, octave=0, depth=NEAR, stereo=0):
        """AddMapPoint + AddObservation: a slot of kf holds p and p's observations name it; Observations() grows by 2 for a stereo slot, else by 1"""
        s = self.slot(kf, p, octave, depth, stereo)
        self.mp_obs[p].append([kf, s])
        self.mp_nobs[p] += 2 if stereo else 1
        return s

    def point(self, observers, octave=0, depth=NEAR, stereo=0, bad=0):
        """a point seen by `observers`: key frames, or (key frame, octave, stereo) tuples"""
        p = self.new_point(bad)
        for o in observers:
            kf, oc, st = o if isinstance(o, tuple) else (o, octave, stereo)
            self.observe(p, kf, oc, depth, st)
        return p

    # ---- what the layers under test take -------------------------------------------------------------------------------------------------------------
    def graph(self):
        """the arguments of orb_line_slam_amd.MapGraph"""
        none = [[] for _ in range(self.n_kf)]
        return dict(mp_obs=[[o[0] for o in r] for r in self.mp_obs], mp_bad=list(self.mp_bad), kf_bad=[0] * self.n_kf, kf_mp=copy.deepcopy(self.kf_mp), kf_covis=none,
                    kf_children=none, kf_parent=[-1] * self.n_kf, kf_ml=copy.deepcopy(self.kf_ml), ml_bad=None if self.ml_bad is None else list(self.ml_bad))

    def view(self):
        """the arguments of orb_line_slam_amd.CullView after the graph"""
        return dict(mp_obs_slot=[[o[1] for o in r] for r in self.mp_obs], mp_nobs=list(self.mp_nobs), kf_slot_octave=self.kf_oct, kf_slot_depth=self.kf_depth,
                    kf_slot_stereo=self.kf_stereo, kf_th_depth=self.th_depth, kf_mode=self.mode)

    def world(self):
        """a deep copy as plain lists, for tests/culling_reference.py to walk and to change"""
        return copy.deepcopy(dict(n_kf=self.n_kf, n_mp=self.n_mp, kf_mp=self.kf_mp, kf_oct=self.kf_oct, kf_depth=self.kf_depth, kf_stereo=self.kf_stereo,
                                  th_depth=self.th_depth, mode=self.mode, mp_obs=self.mp_obs, mp_bad=self.mp_bad, mp_nobs=self.mp_nobs))


def expected(decision, n_mps, n_redundant, went_bad=()):
    return dict(decision=list(decision), n_mps=list(n_mps), n_redundant=list(n_redundant), went_bad=list(went_bad))


# ---- the hand-worked scenes ------------------------------------------------------------------------------------------------------------------------------
def loses_redundancy():
    """ten close points observed mono at octave 0 by A = 0, B = 1, C = 2, D = 3; the list is [A, B]"""
    s = CullScene(4)
    for _ in range(10):
        s.point([0, 1, 2, 3])
    return s, [0, 1]


# As the map stands every point has nObs = 4 > 3 and three other observers at octave 0 <= 0 + 1: A and B both see 10 of 10, 10 > 9.0: both redundant by the
# tables.  The reference culls A; every nObs falls to 3 (no point goes bad: 3 > 2), so for B no point passes Observations() > 3: 0 of 10, kept.
LOSES_TABLES = dict(n_mps=[10, 10], n_redundant=[10, 10], redundant=[1, 1])
LOSES_EXPECTED = expected([1, 0], [10, 10], [10, 0])


def gains_redundancy(order):
    """B = 1 holds nine points observed mono by B, C = 2, D = 3, E = 4, and a point q observed by A = 0 (stereo) and B (mono); A holds q and ten points observed
    by A, C, D, E.  order: 'AB' or 'BA'"""
    s = CullScene(5)
    for _ in range(9):
        s.point([1, 2, 3, 4])
    q = s.point([(0, 0, 1), (1, 0, 0)])
    for _ in range(10):
        s.point([0, 2, 3, 4])
    assert s.mp_nobs[q] == 3
    return s, {"AB": [0, 1], "BA": [1, 0]}[order]


# As the map stands: A counts 11 slots, q is not redundant (nObs = 3, not > 3), the ten others are: 10 > 0.9 * 11 = 9.9: redundant.  B counts 10, nine of
# them redundant: 9 > 9.0 is false: kept.  List [A, B]: A is culled, q loses the stereo observation (3 - 2 = 1 <= 2) and goes bad, B is left with 9 of 9:
# culled.  List [B, A]: B is looked at first, 9 of 10: kept; then A, 10 of 11: culled.  q is point 9.
GAINS_TABLES = {"AB": dict(n_mps=[11, 10], n_redundant=[10, 9], redundant=[1, 0]), "BA": dict(n_mps=[10, 11], n_redundant=[9, 10], redundant=[0, 1])}
GAINS_EXPECTED = {"AB": expected([1, 1], [11, 9], [10, 9], [9]), "BA": expected([0, 1], [10, 11], [9, 10], [9])}


BOUNDARY_N = (10, 20, 30, 70, 100)


def boundary(n_mps, n_red):
    """key frame 0 counts n_mps slots of which n_red are redundant (seen mono at octave 0 by 0, 1, 2, 3; the others by 0 and 1 alone); the list is [0]"""
    s = CullScene(4)
    for i in range(n_mps):
        s.point([0, 1, 2, 3] if i < n_red else [(0, 0, 1), (1, 0, 1)])
    return s, [0]


# nRedundantObservations > 0.9 * nMPs in double: 0.9 * 10 = 9.0, 0.9 * 20 = 18.0, 0.9 * 30 = 27.0, 0.9 * 70 = 63.0 and 0.9 * 100 = 90.0 exactly as IEEE doubles
# round them (0.9 is a little above 9/10 as a double, yet each product rounds to the integer), so nRed = 0.9 * nMPs is kept and one more is culled.  The
# points that are not redundant hang by two stereo observations (nObs = 4, one other observer): culling key frame 0 leaves them 2 and they go bad, in slot
# order; the redundant ones fall to 3 and stay.
def boundary_expected(n_mps, n_red):
    culled = n_red > n_mps * 9 // 10
    return expected([1 if culled else 0], [n_mps], [n_red], range(n_red, n_mps) if culled else [])


def octave_rule():
    """key frame 0 holds p at octave 2, q at octave 2 and r at octave 2; each is seen by 0 and by 1, 2, 3.  p's observers sit at octave 3 (own + 1: they count);
    q's at octave 4 (own + 2: they do not); r's observers hold r in TWO slots each, octave 7 first and octave 3 at the slot the observation names: they count.
    Nine more points like p make the row 12 slots.  The list is [0]"""
    s = CullScene(4)
    p = s.point([(0, 2, 0), (1, 3, 0), (2, 3, 0), (3, 3, 0)])
    q = s.point([(0, 2, 0), (1, 4, 0), (2, 4, 0), (3, 4, 0)])
    r = s.new_point()
    s.observe(r, 0, 2)
    for k in (1, 2, 3):
        s.slot(k, r, octave=7)
        s.observe(r, k, 3)
    for _ in range(9):
        s.point([(0, 2, 0), (1, 3, 0), (2, 3, 0), (3, 3, 0)])
    return s, [0]


# 12 slots count; p, r and the nine are redundant (count 3), q is not (count 0): 11 > 10.8: culled.  Every point falls to nObs = 3: none goes bad.
OCTAVE_TABLES = dict(n_mps=[12], n_redundant=[11], redundant=[1], slot_count=[3, 0, 3] + [3] * 9, slot_flags=[3, 1, 3] + [3] * 9)
OCTAVE_EXPECTED = expected([1], [12], [11])


def nobs_boundary(nobs_extra):
    """key frame 0 holds one point (its slot has no observation behind it) that three stereo key frames 1, 2, 3 observe at octave 0: three qualify.  Its
    Observations() is forced to 3 + nobs_extra (3: not redundant, 4: redundant).  The list is [0]"""
    s = CullScene(4)
    p = s.point([(1, 0, 1), (2, 0, 1), (3, 0, 1)])
    s.slot(0, p)
    s.mp_nobs[p] = 3 + nobs_extra
    return s, [0]


# nObs = 3: Observations() > 3 fails, 0 of 1: kept, the count is 3 all the same.  nObs = 4: 1 of 1, 1 > 0.9: culled; key frame 0 is not among the point's
# observations, so nothing is erased.
NOBS_EXPECTED = {0: expected([0], [1], [0]), 1: expected([1], [1], [1])}


def break_irrelevance():
    """key frame 0 holds one point seen by 0 and by seven others at octave 0: the loop breaks at 3, the table holds 7.  The list is [0]"""
    s = CullScene(8)
    s.point(list(range(8)))
    return s, [0]


BREAK_TABLES = dict(n_mps=[1], n_redundant=[1], redundant=[1], slot_count=[7], slot_flags=[3])
BREAK_EXPECTED = expected([1], [1], [1])


def modes(mode_of_a):
    """loses_redundancy with kf_mode[A] = mode_of_a: 1 (mbNotErase) or 2 (mnId == 0)"""
    s, lst = loses_redundancy()
    s.mode[0] = mode_of_a
    return s, lst


# mode 1: A is redundant, SetBadFlag sets mbToBeErased and returns (decision 2); the map does not change, so B still sees 10 of 10 and is culled.
# mode 2: A is skipped at :643 (decision 0, counts 0); B sees 10 of 10 and is culled.
MODES_EXPECTED = {1: expected([2, 1], [10, 10], [10, 10]), 2: expected([0, 1], [0, 10], [0, 10])}


def listed_twice():
    """loses_redundancy with the list [A, A, B]: A is culled once; the second time it is gone (decision 0, counts 0)"""
    s, _ = loses_redundancy()
    return s, [0, 0, 1]


TWICE_EXPECTED = expected([1, 0, 0], [10, 0, 10], [10, 0, 0])


def monocular_depths():
    """key frame 0 holds ten points seen by 0, 1, 2, 3: four close, three far, two at negative depth and one at NaN.  The list is [0]"""
    s = CullScene(4)
    for d in [NEAR] * 4 + [FAR] * 3 + [-1.0] * 2 + [float("nan")]:
        s.point([0, 1, 2, 3], depth=d)
    return s, [0]


# stereo: the far and the negative slots are skipped, the NaN slot counts (both comparisons are false): 5 of 5, culled.  monocular: all ten count: 10 of 10.
MONOCULAR_EXPECTED = {0: expected([1], [5], [5]), 1: expected([1], [10], [10])}


# ---- sizes -----------------------------------------------------------------------------------------------------------------------------------------------
def row_of(n_slots, n_points=97):
    """key frame 0 with a row of n_slots slots over n_points points (a point sits in several slots once the row is longer), each seen by 0 and by three to six
    of the key frames 1 .. 6 at octaves around its own; every seventh slot is NULL"""
    s = CullScene(7)
    pts = []
    for i in range(min(n_slots, n_points)):
        p = s.new_point()
        for k in range(1, 4 + i % 4):
            s.observe(p, k, (i + k) % 4, stereo=(i + k) % 2)
        pts.append(p)
    for i in range(n_slots):
        if i % 7 == 6:
            s.slot(0)
        elif i < len(pts):
            s.observe(pts[i], 0, i % 3, depth=NEAR if i % 5 else FAR, stereo=i % 2)
        else:
            s.slot(0, pts[i % len(pts)], i % 3, NEAR, 0)
    assert len(s.kf_mp[0]) == n_slots
    return s


def observed_by(n_obs):
    """key frame 0 holds one point in a slot without an observation; n_obs other key frames observe it mono, at octaves 0, 1, 2 in turn (the slot's is 0)"""
    s = CullScene(n_obs + 1)
    p = s.point([(k, (k - 1) % 3, 0) for k in range(1, n_obs + 1)])
    s.slot(0, p)
    s.mp_nobs[p] = max(n_obs, 3)                                     # (a point that is not bad has more than 2)
    return s


# ---- random graphs -----------------------------------------------------------------------------------------------------------------------------------------
def random_scene(seed, n_kf, n_mp, max_obs=12, dense=False):
    """a seeded random snapshot: points seen by up to max_obs key frames through slots with octaves 0 - 7, depths around th_depth with negatives and NaNs and
    stereo flags; bad points (whose observation rows stay behind as they were: nobody may read them), NULL slots, points held in a second slot beside the one
    the observation names, and slots held without an observation.  dense: the observers of a point are four or more neighbours, octaves stay within 0 - 2, most slots are
    close and a few points hang by a stereo and a mono observation, so that key frames are redundant, cull each other's support and orphan each other's
    points."""
    rng = np.random.default_rng(seed)
    s = CullScene(n_kf)
    for k in range(n_kf):
        s.th_depth[k] = float(rng.choice([TH_DEPTH, 30.0, 40.0]))
        s.mode[k] = int(rng.choice([0, 0, 0, 0, 0, 0, 1, 2])) if not dense else int(rng.choice([0] * 10 + [1, 2]))

    def depth():
        u = rng.random()
        if dense:
            return float(rng.uniform(1, 30)) if u < 0.95 else FAR
        return float("nan") if u < 0.03 else float(rng.uniform(-5, 0)) if u < 0.1 else float(rng.uniform(0, 70))

    for i in range(n_mp):
        p = s.new_point()
        if dense:
            k = 2 if rng.random() < 0.1 else int(rng.integers(4, max(min(max_obs, n_kf), 4) + 1))
            first = int(rng.integers(0, n_kf))
            kfs = [(first + d) % n_kf for d in range(min(k, n_kf))]
        else:
            k = int(rng.integers(0, min(max_obs, n_kf) + 1))
            kfs = [int(v) for v in rng.permutation(n_kf)[:k]]
        for j, kf in enumerate(kfs):
            if rng.random() < 0.1:
                s.slot(kf)                                           # a NULL slot
            octave = int(rng.integers(0, 8)) if not dense else int(rng.random() < 0.5) + int(rng.random() < 0.04)
            stereo = int(rng.random() < (0.3 if dense else 0.5))
            if dense and k == 2:
                stereo = int(j == 0)                                 # nObs = 3: the point goes bad with either observation
            if rng.random() < 0.05:
                s.slot(kf, p, int(rng.integers(0, 8)), depth(), 0)   # held a second time, before the slot the observation names
            s.observe(p, kf, octave, depth(), stereo)
        if n_kf > len(kfs) and rng.random() < 0.1:
            other = [k for k in range(n_kf) if k not in kfs]
            s.slot(int(rng.choice(other)), p, int(rng.integers(0, 8)), depth(), 0)      # held without an observation
        if s.mp_nobs[p] <= 2 or rng.random() < (0.03 if dense else 0.1):
            s.mp_bad[p] = 1                                          # (EraseObservation would have discarded it)
    return s


def shuffled_list(seed, n_kf):
    """an explicit list: not ascending, one key frame twice"""
    rng = np.random.default_rng(seed)
    lst = [int(v) for v in rng.permutation(n_kf)[:max(n_kf // 2, 1)]]
    return lst + [lst[0]]


def with_lines(s, seed=0, n_ml=20):
    """line slots, flags and observation counts for TrackedMapLines"""
    rng = np.random.default_rng(seed)
    s.kf_ml = [[int(v) for v in rng.integers(-1, n_ml, size=int(rng.integers(0, 30)))] for _ in range(s.n_kf)]
    s.ml_bad = [int(v) for v in rng.random(n_ml) < 0.2]
    s.ml_nobs = [int(v) for v in rng.integers(0, 6, size=n_ml)]
    return s


def recent_points(seed, n, current_kf_id=10):
    """n points of mlpRecentAddedMapPoints as the arrays of olf_map_point_culling, cycling through rows that take each of the five branches, with
    visible == 0 (found 0 and found > 0: NaN and inf fall through) and a ratio of exactly 0.25, followed by random rows"""
    fixed = [  # bad, found, visible, nobs, first_kf_id    -> action (stereo / monocular)
        (1, 5, 5, 9, 10),      # 1
        (0, 1, 5, 9, 10),      # 2: 0.2 < 0.25
        (0, 1, 4, 9, 10),      # 0: 0.25 is not < 0.25, age 0
        (0, 0, 0, 9, 10),      # 0: NaN < 0.25 is false
        (0, 3, 0, 9, 10),      # 0: inf
        (0, 4, 4, 3, 8),       # 3 (stereo: 3 <= 3) / 0 (monocular: 3 <= 2 fails, age 2 < 3)
        (0, 4, 4, 2, 8),       # 3
        (0, 4, 4, 9, 7),       # 4
        (0, 4, 4, 9, 9),       # 0
        (0, 4, 4, 3, 7),       # 3 / 4
        (1, 0, 9, 0, 0),       # 1: bad comes first
        (0, 1, 9, 0, 0),       # 2: the ratio comes before the observations
    ]
    rng = np.random.default_rng(seed)
    rows = [fixed[i] if i < len(fixed) else (int(rng.random() < 0.2), int(rng.integers(0, 40)), int(rng.integers(0, 40)), int(rng.integers(0, 6)),
                                            int(rng.integers(0, current_kf_id + 1))) for i in range(n)]
    cols = list(zip(*rows)) if rows else [()] * 5
    return dict(bad=np.asarray(cols[0], np.uint8), found=np.asarray(cols[1], np.int32), visible=np.asarray(cols[2], np.int32), nobs=np.asarray(cols[3], np.int32),
                first_kf_id=np.asarray(cols[4], np.int64), current_kf_id=current_kf_id)


RECENT_FIXED_ACTIONS = {0: [1, 2, 0, 0, 0, 3, 3, 4, 0, 3, 1, 2], 1: [1, 2, 0, 0, 0, 0, 3, 4, 0, 4, 1, 2]}
