"""Map snapshots for the UpdateConnections tests, built on localmap_scenes.Scene: hand-made scenes, each the smallest at which one rule of
src/KeyFrame.cc:446-557 can go wrong, and seeded random graphs.  Only mp_obs, mp_bad and kf_mp matter to the call; the other fields of a Scene stay empty
unless a test fills them."""
import numpy as np
from localmap_scenes import Scene, random_scene


def weighted(n_kf, kf, weights):
    """key frame `kf` shares weights[k] points with key frame k: point i is seen by kf and by every k with weights[k] > i, and sits in the slots of all of them"""
    s = Scene(n_kf)
    for i in range(max(weights.values(), default=0)):
        s.point([kf] + [k for k in sorted(weights) if weights[k] > i])
    return s


# ---- the scenes whose answers tests/test_connections_cpu.py works out by hand -------------------------------------------------------------------------
def three_weights():
    """key frame 0 shares 20 points with 1, 20 with 2, 16 with 3"""
    return weighted(4, 0, {1: 20, 2: 20, 3: 16})


# sort(vPairs) leaves (16, 3), (20, 1), (20, 2); push_front reverses: 2, 1, 3.  `>` at :514 is strict over ascending index: pKFmax = 1.
THREE_WEIGHTS_EXPECTED = dict(connected=[1, 2, 3], weights=[20, 20, 16], ordered=[2, 1, 3], ordered_weights=[20, 20, 16], kf_max=1, w_max=20, n_counted=3)


def all_below_th():
    """key frame 2 shares 3 points with 0, 7 with 1, 7 with 4 and 5 with 5: nobody reaches 15"""
    return weighted(6, 2, {0: 3, 1: 7, 4: 7, 5: 5})


# vPairs is empty after the loop, so it gets the one pair (nmax, pKFmax) = (7, 1): 1 is the first in ascending index to reach 7, and 4 does not exceed it.
ALL_BELOW_TH_EXPECTED = dict(connected=[0, 1, 4, 5], weights=[3, 7, 7, 5], ordered=[1], ordered_weights=[7], kf_max=1, w_max=7, n_counted=4)


def around_th():
    """key frame 0 shares 14 / 15 / 16 points with 1 / 2 / 3"""
    return weighted(4, 0, {1: 14, 2: 15, 3: 16})


# `>= th` at :519 with th = 15: 2 and 3 pass, 1 does not; all three are in KFcounter.
AROUND_TH_EXPECTED = dict(connected=[1, 2, 3], weights=[14, 15, 16], ordered=[3, 2], ordered_weights=[16, 15], kf_max=3, w_max=16, n_counted=3)


def slot_rules():
    """key frame 1's slots: point a (seen by 0, 1, 2), NULL, point b (bad; seen by 1, 2, 3), point c (seen by 1 alone), point a again, point d (seen by 1, 3).
    With th = 1."""
    s = Scene(4)
    a = s.point([0, 1, 2], slot=False)
    b = s.point([1, 2, 3], bad=1, slot=False)
    c = s.point([1], slot=False)
    d = s.point([1, 3], slot=False)
    s.kf_mp[1] = [a, -1, b, c, a, d]
    s.kf_mp[0], s.kf_mp[2], s.kf_mp[3] = [a], [b, a], [d, b]
    return s


# a counts twice: 0 and 2 get 2 each.  b is bad: nothing.  c is seen by 1 alone: the self-observation is skipped, nothing.  d: 3 gets 1.  The NULL slot: nothing.
# sort leaves (1, 3), (2, 0), (2, 2); reversed: 2, 0, 3.  pKFmax = 0, the lower of the two with 2.
SLOT_RULES_EXPECTED = dict(connected=[0, 2, 3], weights=[2, 2, 1], ordered=[2, 0, 3], ordered_weights=[2, 2, 1], kf_max=0, w_max=2, n_counted=3)


def with_lines(s):
    """the same scene with every key frame's point slots repeated as line slots: lines do not vote (:496)"""
    s.kf_ml = [[v if v >= 0 else -1 for v in r] for r in s.kf_mp]
    s.ml_bad = list(s.mp_bad)
    return s


# ---- sizes of the ordered row ------------------------------------------------------------------------------------------------------------------------
def survivors(n):
    """key frame min(3, n) is connected to the n others, with weights 1 .. 5 in no order: at th = 1 the ordered row holds n"""
    kf = min(3, n)
    others = [k for k in range(n + 1) if k != kf]
    return weighted(n + 1, kf, {k: 1 + (k * 7) % 5 for k in others})


def equal_weights(n, kf=1, w=3):
    """n key frames around `kf` with weight w each and one more, the last, with weight 1"""
    others = [k for k in range(n + 1) if k != kf]
    weights = {k: w for k in others}
    weights[n + 1] = 1
    return weighted(n + 2, kf, weights)


def one_point_in_many_slots(n_slots=70000):
    """key frame 0 holds one point, seen by 0 and 1, in every one of n_slots slots: weight n_slots"""
    s = Scene(2)
    x = s.point([0, 1], slot=False)
    s.kf_mp[0] = [x] * n_slots
    s.kf_mp[1] = [x]
    return s


def table_ends(n_kf=8192, kf=100):
    """key frame `kf` sees two points with the first and with the last key frame, one more with the last"""
    s = Scene(n_kf)
    s.point([0, kf, n_kf - 1]); s.point([0, kf, n_kf - 1]); s.point([kf, n_kf - 1])
    return s


# ---- empty cases -----------------------------------------------------------------------------------------------------------------------------------------
def empties():
    """key frame 0: no slots; 1: only bad points; 2: only points it alone sees; 3: NULL slots only; 4: a regular one (shares a point with 1 that is not bad)"""
    s = Scene(5)
    s.kf_mp[1] = [s.point([1, 4], bad=1, slot=False), s.point([1, 2], bad=1, slot=False)]
    s.kf_mp[2] = [s.point([2], slot=False), s.point([2], slot=False)]
    s.kf_mp[3] = [-1, -1, -1]
    s.kf_mp[4] = [s.point([4, 1], slot=False)]
    return s


# ---- random graphs -----------------------------------------------------------------------------------------------------------------------------------------
def random_graph(seed, n_kf, n_mp, n_frames=0, max_obs=12):
    """localmap_scenes.random_scene with points seen by up to max_obs key frames, so that weights reach the thresholds the tests use"""
    return random_scene(seed, n_kf, n_mp, n_frames, max_obs=max_obs, max_held=60)


def shuffled_list(seed, n_kf):
    """an explicit list: not ascending, one key frame twice"""
    rng = np.random.default_rng(seed)
    lst = [int(v) for v in rng.permutation(n_kf)[:max(n_kf // 2, 1)]]
    return lst + [lst[0]]
