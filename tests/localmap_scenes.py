"""Map snapshots and frame batches for the UpdateLocalMap tests: seeded random graphs and hand-made scenes, each the smallest at which one rule of
src/Tracking.cc:2039-2205 can go wrong.  A scene is a Scene: the arguments of orb_line_slam_amd.MapGraph / localmap_reference.Map (graph()), and per frame
the rows of mvpMapPoints / mvpMapLines as map indices (frame_mp, frame_ml)."""
import numpy as np


class Scene:
    def __init__(self, n_kf, n_mp=0, n_ml=None):
        self.mp_obs = [[] for _ in range(n_mp)]
        self.mp_bad = [0] * n_mp
        self.kf_bad = [0] * n_kf
        self.kf_mp = [[] for _ in range(n_kf)]
        self.kf_covis = [[] for _ in range(n_kf)]
        self.kf_children = [[] for _ in range(n_kf)]
        self.kf_parent = [-1] * n_kf
        self.kf_ml = None if n_ml is None else [[] for _ in range(n_kf)]
        self.ml_bad = None if n_ml is None else [0] * n_ml
        self.frame_mp, self.frame_ml = [], None

    def graph(self):
        return dict(mp_obs=self.mp_obs, mp_bad=self.mp_bad, kf_bad=self.kf_bad, kf_mp=self.kf_mp, kf_covis=self.kf_covis, kf_children=self.kf_children,
                    kf_parent=self.kf_parent, kf_ml=self.kf_ml, ml_bad=self.ml_bad)

    def point(self, kfs, bad=0, slot=True):
        """a new map point observed by `kfs`, appended to each one's slots; returns its index"""
        i = len(self.mp_bad)
        self.mp_obs.append(list(kfs))
        self.mp_bad.append(bad)
        if slot:
            for k in kfs:
                self.kf_mp[k].append(i)
        return i

    def line(self, bad=0):
        i = len(self.ml_bad)
        self.ml_bad.append(bad)
        return i

    def set_parent(self, child, parent):
        self.kf_parent[child] = parent
        self.kf_children[parent].append(child)

    def with_lines_like_points(self):
        """the same scene with every key frame's point slots repeated as line slots (lines i <-> points i) and a frame that also holds its points as lines"""
        self.kf_ml = [list(r) for r in self.kf_mp]
        self.ml_bad = list(self.mp_bad)
        self.frame_ml = [[v if v >= 0 else -1 for v in r] for r in self.frame_mp]
        return self


def voting(n_kf, votes):
    """n_kf key frames, each with one point of its own in slot 0 ... and a frame that gives key frame k votes[k] votes (one more point per vote)"""
    s = Scene(n_kf)
    row = []
    for k in range(n_kf):
        s.point([k])
    for k, v in sorted(votes.items()):
        for _ in range(v):
            row.append(s.point([k]))
    s.frame_mp = [row]
    return s


# ---- the 5-key-frame graph whose answers tests/test_localmap_cpu.py derives on paper ----------------------------------------------------------------
def five_kf():
    s = Scene(5, 6, 3)
    s.mp_obs = [[1, 3], [3], [1], [4], [2], [0]]
    s.mp_bad = [0, 0, 0, 1, 0, 0]
    s.kf_bad = [1, 0, 0, 0, 0]
    s.kf_mp = [[5, 0], [0, -1, 2], [4, 3], [1, 0], [3, 2]]
    s.kf_ml = [[], [1], [2], [1, 0], []]
    s.ml_bad = [0, 0, 1]
    s.kf_covis = [[], [3, 0, 2], [], [1], []]
    s.set_parent(1, 0); s.set_parent(4, 1); s.set_parent(2, 1); s.set_parent(3, 1)      # (children of 1 given as 4, 2, 3: a std::set iterates 2, 3, 4)
    s.frame_mp = [[0, 1, 2, 3, -1], [4], [-1, -2]]
    s.frame_ml = [[2, 0], [], [1]]
    return s


FIVE_KF_EXPECTED = [
    # frame 0: votes kf1 = 2 (points 0, 2), kf3 = 2 (points 0, 1); point 3 is bad and cleared.  First list 1, 3; the tie goes to the lower index.  Member 1:
    # neighbours 3 (stamped), 0 (bad), 2 -> 2; children 2 (stamped now), 3 (stamped), 4 -> 4; parent 0, bad but not tested -> 0, and the loop ends.
    # Points: kf1 0, NULL, 2; kf3 1, (0 seen); kf2 4, (3 bad); kf4 (3 bad), (2 seen); kf0 5, (0 seen).  Lines: kf1 1; kf3 (1 seen), 0; kf2 (2 bad).
    dict(local_kfs=[1, 3, 2, 4, 0], local_points=[0, 2, 1, 4, 5], local_lines=[1, 0], ref_kf=1, n_voted=2, frame_mp=[0, 1, 2, -1, -1], frame_ml=[-1, 0]),
    # frame 1: point 4 votes for kf2.  Member 2: no neighbours, no children, parent 1 -> 1, loop ends.  Points: kf2 4, (3 bad); kf1 0, 2.  Lines: kf2 (2 bad); kf1 1.
    dict(local_kfs=[2, 1], local_points=[4, 0, 2], local_lines=[1], ref_kf=2, n_voted=1, frame_mp=[4], frame_ml=[]),
    # frame 2: holds nothing that votes
    dict(local_kfs=[], local_points=[], local_lines=[], ref_kf=-1, n_voted=0, frame_mp=[-1, -2], frame_ml=[1]),
]


# ---- ties ------------------------------------------------------------------------------------------------------------------------------------------------
def ties(n_equal):
    """n_equal key frames (3, 5[, 6]) with the maximal vote count, a lower one (1) with fewer: the reference key frame is 3"""
    votes = {1: 2, 3: 4, 5: 4, 7: 1}
    if n_equal == 3:
        votes[6] = 4
    return voting(8, votes)


def bad_kf_has_most_votes():
    s = voting(6, {1: 2, 2: 5, 4: 3})
    s.kf_bad[2] = 1
    return s


# ---- the extension loop, one rule each ---------------------------------------------------------------------------------------------------------------
def eleventh_neighbour_free():
    """member 0's first ten neighbours are stamped (1 .. 5) or bad (6 .. 10); the eleventh, 11, is free: nothing is added"""
    s = voting(12, {k: 1 for k in range(6)})
    for k in range(6, 11):
        s.kf_bad[k] = 1
    s.kf_covis[0] = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    return s


def child_after_bad_child():
    """member 2's children: 1 (bad), 4 (stamped), 5, 3 given out of order -- ascending: 1 bad, 3 free -> 3"""
    s = voting(6, {2: 1, 4: 1})
    s.kf_bad[1] = 1
    for c in (5, 1, 4, 3):
        s.set_parent(c, 2)
    return s


def bad_parent():
    s = voting(4, {2: 1})
    s.kf_bad[0] = 1
    s.set_parent(2, 0)
    return s


def parent_at_first_member():
    """members 1, 2, 3: member 1's parent 0 is added and ends the loop, so 2's free neighbour 4 and 3's free child 5 are never added"""
    s = voting(6, {1: 1, 2: 1, 3: 1})
    s.set_parent(1, 0)
    s.kf_covis[2] = [4]
    s.set_parent(5, 3)
    return s


def first_list_of(n_first, n_kf=100):
    """a first list of n_first members (key frames 10 .. 10 + n_first - 1), each with a free neighbour among the rest: at 79 and 80 the loop adds until the list
    holds 81; at 81 it adds nothing"""
    s = voting(n_kf, {10 + k: 1 + (k % 3) for k in range(n_first)})
    free = [k for k in range(n_kf) if not (10 <= k < 10 + n_first)]
    for m in range(n_first):
        s.kf_covis[10 + m] = [free[(m + t) % len(free)] for t in range(3)]
    return s


# ---- positional de-duplication ------------------------------------------------------------------------------------------------------------------------
def _filler(s, kf, n):
    for _ in range(n):
        s.kf_mp[kf].append(s.point([kf], slot=False))


def dup_in_one_kf():
    """key frame 0 holds point X at slots 3 and 7 (after Fuse / Replace); the frame votes for 0"""
    s = Scene(1)
    _filler(s, 0, 3)
    x = s.point([0])                                  # slot 3
    _filler(s, 0, 3)
    s.kf_mp[0].append(x)                              # slot 7
    _filler(s, 0, 2)
    s.frame_mp = [[x]]
    return s


def dup_across_two_kfs(len_a=5, len_b=5, at_a=None, at_b=1):
    """local key frames 0 and 1 with len_a and len_b slots share point X: slot at_a of 0 (default: its last), slot at_b of 1; 1 also holds a point of 0's
    before X and repeats X once more at its end"""
    at_a = len_a - 1 if at_a is None else at_a
    s = Scene(2)
    _filler(s, 0, at_a)
    x = s.point([0, 1], slot=False)
    s.kf_mp[0].append(x)
    _filler(s, 0, len_a - at_a - 1)
    _filler(s, 1, at_b)
    s.kf_mp[1].insert(0, s.kf_mp[0][0])
    s.kf_mp[1].append(x)
    _filler(s, 1, max(len_b - at_b - 3, 0))
    s.kf_mp[1].append(x)
    s.frame_mp = [[x]]
    return s


def dup_straddling(boundary):
    """one key frame holding X on either side of slot `boundary` (and again far behind), followed by a second one that starts with X: with a first key frame of
    boundary + 6 slots, the pair also straddles the boundary when the two are laid end to end"""
    s = Scene(2)
    _filler(s, 0, boundary - 2)
    x = s.point([0, 1], slot=False)
    y = s.point([0, 1], slot=False)
    s.kf_mp[0] += [x, y]                              # slots boundary - 2, boundary - 1
    s.kf_mp[0] += [y, x]                              # slots boundary, boundary + 1
    _filler(s, 0, 3)
    s.kf_mp[0].append(y)
    s.kf_mp[1] += [x, y]
    _filler(s, 1, 4)
    s.frame_mp = [[x]]
    return s


def spread_points(s, n_total):
    """the same scene in a map of n_total points: point i becomes point i * (n_total // n_mp), the points between are seen by nobody.  (A frame's two bitmaps
    live in LDS up to 262144 points and lines together and in scratch beyond: the library takes another path there.)"""
    n = len(s.mp_bad)
    step = n_total // n
    assert step >= 1
    f = lambda v: v * step if v >= 0 else v
    obs, bad = [[] for _ in range(n_total)], [0] * n_total
    for i in range(n):
        obs[i * step], bad[i * step] = s.mp_obs[i], s.mp_bad[i]
    s.mp_obs, s.mp_bad = obs, bad
    s.kf_mp = [[f(v) for v in r] for r in s.kf_mp]
    s.frame_mp = [[f(v) for v in r] for r in s.frame_mp]
    return s


# ---- empty cases -------------------------------------------------------------------------------------------------------------------------------------
def frame_holds_nothing():
    s = voting(3, {1: 1})
    s.frame_mp = [[-1, -1, -2], s.frame_mp[0], []]
    return s


def all_voted_bad():
    s = voting(4, {1: 2, 3: 1})
    s.kf_bad[1] = s.kf_bad[3] = 1
    s.kf_covis[1] = [0]
    return s


# ---- random graphs -------------------------------------------------------------------------------------------------------------------------------------
def random_scene(seed, n_kf, n_mp, n_frames, n_ml=None, max_held=60, max_obs=4, bad=0.1):
    """A map of n_kf key frames in a parent tree with covisibility rows of up to 14, n_mp points seen by 1 .. max_obs key frames each (slots shuffled, with NULLs,
    and now and then a point twice in one key frame), n_ml lines spread the same way; n_frames frames holding between 0 and max_held features each: map points,
    NULLs (-1) and temporal points (-2).  About `bad` of everything is bad."""
    rng = np.random.default_rng(seed)
    s = Scene(n_kf, n_mp, n_ml)
    s.kf_bad = [int(v) for v in rng.random(n_kf) < bad]
    s.mp_bad = [int(v) for v in rng.random(n_mp) < bad]
    for k in range(1, n_kf):
        if rng.random() < 0.85:
            s.set_parent(k, int(rng.integers(0, k)))
    for k in range(n_kf):
        others = [int(v) for v in rng.permutation(n_kf) if v != k]
        s.kf_covis[k] = others[:int(rng.integers(0, 15))]
        rng.shuffle(s.kf_children[k])

    def spread(n_items, rows):
        obs = []
        for i in range(n_items):
            ks = [int(v) for v in rng.choice(n_kf, size=min(int(rng.integers(1, max_obs + 1)), n_kf), replace=False)]
            obs.append(ks)
            for k in ks:
                rows[k].append(i)
                if rng.random() < 0.05:
                    rows[k].append(i)
        for k in range(n_kf):
            rows[k] += [-1] * int(rng.integers(0, 4))
            rng.shuffle(rows[k])
        return obs

    s.mp_obs = spread(n_mp, s.kf_mp)
    if n_ml is not None:
        s.ml_bad = [int(v) for v in rng.random(n_ml) < bad]
        spread(n_ml, s.kf_ml)
        s.frame_ml = []
    for j in range(n_frames):
        n = int(rng.integers(0, max_held + 1)) if j else max_held
        s.frame_mp.append([int(rng.integers(0, n_mp)) if n_mp and rng.random() < 0.8 else int(rng.integers(-2, 0)) for _ in range(n)])
        if n_ml is not None:
            nl = int(rng.integers(0, 20))
            s.frame_ml.append([int(rng.integers(0, n_ml)) if n_ml and rng.random() < 0.8 else -1 for _ in range(nl)])
    return s


def large_scene(seed, n_kf=1500, n_mp=150000, n_frames=256, n_feat=2000, slots=2000):
    """the batch tools/localmap_latency.py times: about `slots` slots per key frame, points seen by neighbouring key frames (a trajectory), frames that hold
    n_feat features of which about 70 % are map points around one place of the trajectory.  Built with numpy: the arguments of MapGraph as arrays."""
    rng = np.random.default_rng(seed)
    home = rng.integers(0, n_kf, n_mp)                               # the key frame a point was created in
    rows = [[] for _ in range(n_kf)]
    obs = [[] for _ in range(n_mp)]
    order = rng.permutation(n_mp)
    per_kf = np.zeros(n_kf, np.int64)
    for i in order:
        for d in range(int(rng.integers(2, 40))):                    # seen by the following key frames while they have room
            k = int(home[i]) + d
            if k >= n_kf or per_kf[k] >= slots:
                break
            rows[k].append(int(i)); obs[i].append(k); per_kf[k] += 1
    s = Scene(n_kf)
    s.mp_obs, s.mp_bad, s.kf_mp = obs, [int(v) for v in rng.random(n_mp) < 0.02], rows
    for k in range(1, n_kf):
        s.set_parent(k, k - 1)
        s.kf_covis[k] = [int(v) for v in range(max(k - 12, 0), k)][::-1]
    by_home = np.argsort(home, kind="stable")
    start = np.searchsorted(home[by_home], np.arange(n_kf + 1))
    for j in range(n_frames):
        k0 = int(rng.integers(40, n_kf))
        near = by_home[start[max(k0 - 40, 0)]:start[k0]]
        held = rng.choice(near, size=min(int(0.7 * n_feat), len(near)), replace=False) if len(near) else np.zeros(0, np.int64)
        row = np.full(n_feat, -1, np.int64)
        row[rng.permutation(n_feat)[:len(held)]] = held
        s.frame_mp.append([int(v) for v in row])
    return s
