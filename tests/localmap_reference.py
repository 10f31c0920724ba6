"""Tracking::UpdateLocalMap restated line by line in Python: the oracle of olf_update_local_map* (tests/test_localmap_cpu.py, tests/test_localmap_gpu.py).

The objects are real objects with real per-object stamps (mnTrackReferenceForFrame), the containers real dicts keyed by key-frame index and iterated in
ascending key: convention C.16 lets ascending index stand for the address order of std::map<KeyFrame*,int> and std::set<KeyFrame*>.  Nothing here
is vectorised or shared with the library's Python wrapper.  Parity unpinned: the reference cannot be run here (its third-party libraries are not vendored),
so every function follows the cited lines by reading."""


class MapPoint:
    """also MapLine: what UpdateLocalMap reads of either"""

    def __init__(self, idx):
        self.idx, self.bad, self.observations, self.mnTrackReferenceForFrame = idx, False, {}, 0

    def isBad(self):
        return self.bad

    def GetObservations(self):
        return dict(self.observations)                # (a copy, as the reference returns one under the lock)


MapLine = MapPoint


class KeyFrame:
    def __init__(self, idx):
        self.idx, self.bad, self.mnTrackReferenceForFrame = idx, False, 0
        self.mvpMapPoints, self.mvpMapLines = [], []  # slots, None = NULL
        self.mvpOrderedConnectedKeyFrames = []
        self.mspChildrens = {}                        # std::set<KeyFrame*>: a dict keyed by index, iterated ascending
        self.mpParent = None

    def isBad(self):
        return self.bad

    def GetMapPointMatches(self):
        return list(self.mvpMapPoints)

    def GetMapLineMatches(self):
        return list(self.mvpMapLines)

    def GetBestCovisibilityKeyFrames(self, N):
        """src/KeyFrame.cc:252-260: the whole list when it is shorter than N, else its first N.  Parity unpinned."""
        if len(self.mvpOrderedConnectedKeyFrames) < N:
            return list(self.mvpOrderedConnectedKeyFrames)
        return list(self.mvpOrderedConnectedKeyFrames[:N])

    def GetChilds(self):
        return [self.mspChildrens[k] for k in sorted(self.mspChildrens)]

    def GetParent(self):
        return self.mpParent


class Frame:
    def __init__(self, mnId, mvpMapPoints, mvpMapLines=()):
        self.mnId = mnId
        self.mvpMapPoints, self.mvpMapLines = list(mvpMapPoints), list(mvpMapLines)
        self.N, self.N_l = len(self.mvpMapPoints), len(self.mvpMapLines)
        self.mpReferenceKF = None


class Tracking:
    """the members UpdateLocalMap reads and writes"""

    def __init__(self):
        self.mCurrentFrame = None
        self.mvpLocalKeyFrames, self.mvpLocalMapPoints, self.mvpLocalMapLines = [], [], []
        self.mpReferenceKF = None
        self.n_voted = 0                              # (not a member: the size of keyframeCounter, for the tests)

    def UpdateLocalMap(self):
        """src/Tracking.cc:2028-2037 (the two Set calls before are for visualisation).  Parity unpinned."""
        self.UpdateLocalKeyFrames()
        self.UpdateLocalPointsAndLines()

    def UpdateLocalPointsAndLines(self):
        """src/Tracking.cc:2039-2078.  Parity unpinned."""
        F = self.mCurrentFrame
        self.mvpLocalMapPoints = []
        self.mvpLocalMapLines = []
        for pKF in self.mvpLocalKeyFrames:
            for pMP in pKF.GetMapPointMatches():
                if pMP is None:
                    continue
                if pMP.mnTrackReferenceForFrame == F.mnId:
                    continue
                if not pMP.isBad():
                    self.mvpLocalMapPoints.append(pMP)
                    pMP.mnTrackReferenceForFrame = F.mnId
            for pML in pKF.GetMapLineMatches():
                if pML is None:
                    continue
                if pML.mnTrackReferenceForFrame == F.mnId:
                    continue
                if not pML.isBad():
                    self.mvpLocalMapLines.append(pML)
                    pML.mnTrackReferenceForFrame = F.mnId

    def UpdateLocalKeyFrames(self):
        """src/Tracking.cc:2080-2205.  Parity unpinned."""
        F = self.mCurrentFrame
        keyframeCounter = {}                          # map<KeyFrame*,int>: keyed by index, iterated ascending (C.16)
        kf_of = {}
        for i in range(F.N):
            if F.mvpMapPoints[i] is not None:
                pMP = F.mvpMapPoints[i]
                if not pMP.isBad():
                    for pKF in pMP.GetObservations().values():
                        keyframeCounter[pKF.idx] = keyframeCounter.get(pKF.idx, 0) + 1
                        kf_of[pKF.idx] = pKF
                else:
                    F.mvpMapPoints[i] = None
        for i in range(F.N_l):
            if F.mvpMapLines[i] is not None:
                pML = F.mvpMapLines[i]
                if not pML.isBad():
                    for _ in pML.GetObservations().values():
                        pass                          # ;//keyframeCounter[it->first]++;   (:2110)
                else:
                    F.mvpMapLines[i] = None
        self.n_voted = len(keyframeCounter)
        if not keyframeCounter:
            return
        max_ = 0
        pKFmax = None
        self.mvpLocalKeyFrames = []                   # clear(); reserve(3 * keyframeCounter.size())
        reserved = 3 * len(keyframeCounter)
        for idx in sorted(keyframeCounter):
            pKF = kf_of[idx]
            if pKF.isBad():
                continue
            if keyframeCounter[idx] > max_:
                max_ = keyframeCounter[idx]
                pKFmax = pKF
            self.mvpLocalKeyFrames.append(pKF)
            pKF.mnTrackReferenceForFrame = F.mnId
        # itEndKF = mvpLocalKeyFrames.end() is taken here, once: the loop visits the first list only.  (The iterators stay valid: no push_back below
        # exceeds the reserve before the parent's, and that one leaves the loop.)
        itEndKF = len(self.mvpLocalKeyFrames)
        itKF = 0
        while itKF != itEndKF:
            if len(self.mvpLocalKeyFrames) > 80:
                break
            pKF = self.mvpLocalKeyFrames[itKF]
            for pNeighKF in pKF.GetBestCovisibilityKeyFrames(10):
                if not pNeighKF.isBad():
                    if pNeighKF.mnTrackReferenceForFrame != F.mnId:
                        self.mvpLocalKeyFrames.append(pNeighKF)
                        pNeighKF.mnTrackReferenceForFrame = F.mnId
                        break
            for pChildKF in pKF.GetChilds():
                if not pChildKF.isBad():
                    if pChildKF.mnTrackReferenceForFrame != F.mnId:
                        self.mvpLocalKeyFrames.append(pChildKF)
                        pChildKF.mnTrackReferenceForFrame = F.mnId
                        break
            pParent = pKF.GetParent()
            if pParent is not None:
                if pParent.mnTrackReferenceForFrame != F.mnId:
                    self.mvpLocalKeyFrames.append(pParent)
                    pParent.mnTrackReferenceForFrame = F.mnId
                    break
            assert len(self.mvpLocalKeyFrames) <= reserved, "a push_back beyond the reserve would invalidate the loop's iterators"
            itKF += 1
        if pKFmax is not None:
            self.mpReferenceKF = pKFmax
            F.mpReferenceKF = self.mpReferenceKF


class Map:
    """The objects of one snapshot, built from the plain lists tests/localmap_scenes.py makes (the arguments of orb_line_slam_amd.MapGraph)."""

    def __init__(self, mp_obs, mp_bad, kf_bad, kf_mp, kf_covis, kf_children, kf_parent, kf_ml=None, ml_bad=None):
        self.kfs = [KeyFrame(k) for k in range(len(kf_bad))]
        self.mps = [MapPoint(i) for i in range(len(mp_bad))]
        self.mls = [MapLine(i) for i in range(len(ml_bad))] if ml_bad is not None else []
        for i, p in enumerate(self.mps):
            p.bad = bool(mp_bad[i])
            p.observations = {int(k): self.kfs[int(k)] for k in mp_obs[i]}
        for i, line in enumerate(self.mls):
            line.bad = bool(ml_bad[i])
        for k, kf in enumerate(self.kfs):
            kf.bad = bool(kf_bad[k])
            kf.mvpMapPoints = [None if int(v) < 0 else self.mps[int(v)] for v in kf_mp[k]]
            if kf_ml is not None:
                kf.mvpMapLines = [None if int(v) < 0 else self.mls[int(v)] for v in kf_ml[k]]
            kf.mvpOrderedConnectedKeyFrames = [self.kfs[int(v)] for v in kf_covis[k]]
            kf.mspChildrens = {int(v): self.kfs[int(v)] for v in kf_children[k]}
            kf.mpParent = None if int(kf_parent[k]) < 0 else self.kfs[int(kf_parent[k])]

    def update_local_map(self, frame_mp, frame_ml=None):
        """UpdateLocalMap for every frame of a batch, each against the snapshot and starting from empty lists (what olf_update_local_map* states for a
        frame without votes).  frame_mp / frame_ml: per frame, map indices, negative = none.  Returns per frame the dict orb_line_slam_amd.UpdateLocalMap
        returns, as plain lists."""
        out = []
        for j, row in enumerate(frame_mp):
            lrow = frame_ml[j] if frame_ml is not None else []
            F = Frame(j + 1, [None if int(v) < 0 else self.mps[int(v)] for v in row], [None if int(v) < 0 else self.mls[int(v)] for v in lrow])
            T = Tracking()
            T.mCurrentFrame = F
            T.UpdateLocalMap()
            clean = [int(v) if int(v) < 0 else (-1 if F.mvpMapPoints[i] is None else int(v)) for i, v in enumerate(row)]
            lclean = [int(v) if int(v) < 0 else (-1 if F.mvpMapLines[i] is None else int(v)) for i, v in enumerate(lrow)]
            out.append({"local_kfs": [k.idx for k in T.mvpLocalKeyFrames], "local_points": [p.idx for p in T.mvpLocalMapPoints],
                        "local_lines": [m.idx for m in T.mvpLocalMapLines], "ref_kf": -1 if T.mpReferenceKF is None else T.mpReferenceKF.idx,
                        "n_voted": T.n_voted, "frame_mp": clean, "frame_ml": lclean if frame_ml is not None else None})
        return out
