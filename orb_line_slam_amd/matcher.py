"""Host-side mirrors of the reference's descriptor matchers on top of the C ABI.

  LineMatcher free functions  include/LineMatcher.h:57-69, src/LineMatcher.cpp:42-150
  ORBmatcher                  include/ORBmatcher.h:37-103 (constants + DescriptorDistance; the searches that
                              need MapPoint state keep their greedy resolution on the host)
All distances are computed on the GPU (csrc/match.hip).  Three sections:
  1. the brute-force matchers over descriptor arrays,
  2. the searches over host views of a frame (FrameView and its kin; class ORBmatcher),
  3. the wrappers of the *_batch_dev / *_pairs_dev entries over device-resident batches (torch tensors).
"""
import numpy as np
from . import _lib
from ._lib import check, lib, ptr

_shared_ctx = None


def _ctx(context=None):
    """matchers are stateless in the reference; they borrow a small context for stream + scratch"""
    global _shared_ctx
    if context is not None:
        return context
    if _shared_ctx is None:
        _shared_ctx = _lib.Context(_lib.default_params(), 640, 480, 1)
    return _shared_ctx


def _call(name, *args):
    """the C ABI entry `name` on args, its return code checked"""
    check(getattr(lib(), name)(*args), name)


# ------------------------------------------------------------------------------------------------------------------
# 1. Brute-force matchers: descriptor arrays in, indices and distances out.
def _desc(d):
    d = np.ascontiguousarray(d, dtype=np.uint8)
    if d.ndim != 2 or (d.shape[0] and d.shape[1] != 32):
        raise ValueError("descriptors must be an (N, 32) uint8 array (cv::Mat N x 32 CV_8U)")
    return d


def knn2(desc1, desc2, context=None):
    """cv::BFMatcher(NORM_HAMMING).knnMatch(desc1, desc2, k=2): (idx0, dist0, dist1) per query row."""
    d1, d2 = _desc(desc1), _desc(desc2)
    n = d1.shape[0]
    idx0, dist0, dist1 = (np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    _call("olf_knn2", _ctx(context).handle, ptr(d1), n, ptr(d2), d2.shape[0], ptr(idx0), ptr(dist0), ptr(dist1))
    return idx0, dist0, dist1


def matchNNR(desc1, desc2, nnr, context=None):
    """src/LineMatcher.cpp:42-62 -> (n_matches, matches_12)"""
    return match(desc1, desc2, nnr, best_lr_matches=False, context=context)


def match(desc1, desc2, nnr, best_lr_matches=True, context=None):
    """match(desc1, desc2, nnr, matches_12), src/LineMatcher.cpp:104-132 -> (n_matches, matches_12).
    best_lr_matches is Config::bestLRMatches() (default true, src/Config.cpp:47)."""
    d1, d2 = _desc(desc1), _desc(desc2)
    m12 = np.full(d1.shape[0], -1, np.int32)
    _call("olf_match_bf", _ctx(context).handle, ptr(d1), d1.shape[0], ptr(d2), d2.shape[0], float(nnr), int(bool(best_lr_matches)), ptr(m12))
    return int((m12 >= 0).sum()), m12


def match_maplines(maplines_desc, frame_desc_l, nnr, context=None):
    """int match(const std::vector<MapLine*>&, Frame&, float nnr, std::vector<int>& matches_12), src/LineMatcher.cpp:64-73: the local map
    lines' descriptors against mDescriptors_Line with matchNNR (the code after the early return there is dead)."""
    return matchNNR(maplines_desc, frame_desc_l, nnr, context)


def distance_matrix(desc1, desc2, context=None):
    """ORB_SLAM2::distance / ORBmatcher::DescriptorDistance over all pairs -> (N1, N2) uint16"""
    d1, d2 = _desc(desc1), _desc(desc2)
    out = np.zeros((d1.shape[0], d2.shape[0]), np.uint16)
    _call("olf_hamming_matrix", _ctx(context).handle, ptr(d1), d1.shape[0], ptr(d2), d2.shape[0], ptr(out))
    return out


def distance(a, b, context=None):
    """int distance(const cv::Mat&, const cv::Mat&), src/LineMatcher.cpp:134-150"""
    return int(distance_matrix(np.asarray(a).reshape(1, 32), np.asarray(b).reshape(1, 32), context)[0, 0])


def ComputeDistinctiveDescriptors(observations, context=None):
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:254-318) / MapLine::ComputeDistinctiveDescriptors (src/MapLine.cc:257-322)
    for a batch of landmarks.  observations: list of (N_p, 32) uint8 arrays (the descriptors observing landmark p, bad key frames already
    dropped).  Returns BestIdx per landmark (-1 where the list is empty: the reference returns early and keeps the old descriptor)."""
    obs = [np.ascontiguousarray(o, np.uint8).reshape(-1, 32) for o in observations]
    offs = np.zeros(len(obs) + 1, np.int32)
    offs[1:] = np.cumsum([len(o) for o in obs])
    desc = np.ascontiguousarray(np.concatenate(obs)) if len(obs) and offs[-1] else np.zeros((0, 32), np.uint8)
    best = np.full(len(obs), -1, np.int32)
    if len(obs):
        _call("olf_distinctive_descriptors", _ctx(context).handle, ptr(desc), ptr(offs), len(obs), ptr(best))
    return best


def _candidate_distances(descQ, lists, descT, context=None):
    """GPU Hamming distances for CSR candidate lists; returns a list of uint16 arrays (one per query)."""
    offs = np.zeros(len(lists) + 1, np.int32)
    offs[1:] = np.cumsum([len(l) for l in lists])
    cand = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32) for l in lists]) if offs[-1] else np.zeros(0, np.int32), np.int32)
    dist = np.zeros(int(offs[-1]), np.uint16)
    dq, dt = _desc(descQ), _desc(descT)
    if len(lists) and offs[-1]:
        _call("olf_match_candidates", _ctx(context).handle, ptr(dq), dq.shape[0], ptr(dt), dt.shape[0], ptr(offs), ptr(cand), ptr(dist))
    return [dist[offs[i]:offs[i + 1]] for i in range(len(lists))]


# ------------------------------------------------------------------------------------------------------------------
# 2. ORBmatcher searches that need Frame / MapPoint state.  The reference walks C++ objects (Frame, KeyFrame, MapPoint*);
# here a frame is a FrameView: plain arrays with the members those functions read.  Host code builds the candidate
# lists (Frame::GetFeaturesInArea / the BoW feature vectors) and replays the greedy, order-dependent resolution exactly
# as the reference does; every descriptor distance comes from the GPU (olf_match_candidates).
class FrameView:
    """The Frame / KeyFrame members read by SearchByProjection (src/ORBmatcher.cc:1330-1472) and SearchByBoW (:161-290).

    mvKeysUn / mvKeys : KEYPOINT_DTYPE arrays;  mDescriptors : (N, 32) uint8;  mvuRight : (N,) float32
    mp_valid[i]  : mvpMapPoints[i] != NULL        mp_world[i] : pMP->GetWorldPos() (float32 x3)
    mp_desc[i]   : pMP->GetDescriptor()           mp_obs[i]   : pMP->Observations() > 0      mp_bad[i] : pMP->isBad()
    mvbOutlier   : (N,) bool                      mTcw : (4, 4) float32
    fx, fy, cx, cy, mbf, mb, mnMinX, mnMaxX, mnMinY, mnMaxY : camera / image bounds;  mvScaleFactors : (nlevels,) float32
    mFeatVec     : {node id: [feature indices]} (DBoW2::FeatureVector), only for SearchByBoW
    """
    FRAME_GRID_COLS, FRAME_GRID_ROWS = 64, 48

    def __init__(self, mvKeysUn, mDescriptors, mvuRight=None, mvScaleFactors=None, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157,
                 mbf=386.1448, bounds=(0.0, 1241.0, 0.0, 376.0), mTcw=None, mFeatVec=None):
        self.mvKeysUn = np.ascontiguousarray(mvKeysUn)
        self.mvKeys = self.mvKeysUn          # identical when the camera has no distortion (src/Frame.cc:601-605)
        self.N = len(self.mvKeysUn)
        self.mDescriptors = np.ascontiguousarray(mDescriptors, np.uint8).reshape(self.N, 32)
        self.mvuRight = np.full(self.N, -1.0, np.float32) if mvuRight is None else np.ascontiguousarray(mvuRight, np.float32)
        self.mvScaleFactors = np.ascontiguousarray(mvScaleFactors if mvScaleFactors is not None else 1.2 ** np.arange(8), np.float32)
        f32 = np.float32
        self.fx, self.fy, self.cx, self.cy, self.mbf = f32(fx), f32(fy), f32(cx), f32(cy), f32(mbf)
        self.mb = f32(self.mbf / self.fx)
        self.mnMinX, self.mnMaxX, self.mnMinY, self.mnMaxY = (f32(v) for v in bounds)
        self.mfGridElementWidthInv = f32(f32(self.FRAME_GRID_COLS) / f32(self.mnMaxX - self.mnMinX))
        self.mfGridElementHeightInv = f32(f32(self.FRAME_GRID_ROWS) / f32(self.mnMaxY - self.mnMinY))
        self.mTcw = np.eye(4, dtype=np.float32) if mTcw is None else np.ascontiguousarray(mTcw, np.float32)
        self.mp_valid = np.zeros(self.N, bool)
        self.mp_world = np.zeros((self.N, 3), np.float32)
        self.mp_desc = np.zeros((self.N, 32), np.uint8)
        self.mp_obs = np.zeros(self.N, bool)
        self.mp_bad = np.zeros(self.N, bool)
        self.mvbOutlier = np.zeros(self.N, bool)
        self.mFeatVec = mFeatVec or {}
        self.AssignFeaturesToGrid()

    def attach_grid(self, offsets, index):
        """Hand the C-backed searches a prebuilt mGrid (frame.assign_features_to_grid / StereoFrontEnd.frame_grid; layout in
        include/orbline_types.h) instead of letting each of them rebuild it from the key points.  attach_grid(None, None) detaches it."""
        self.grid_offsets = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        self.grid_index = None if index is None else np.ascontiguousarray(index, np.int32)

    def AssignFeaturesToGrid(self):
        """src/Frame.cc:334-349 + PosInGrid :572-582 (C round(): half away from zero)"""
        self.mGrid = [[[] for _ in range(self.FRAME_GRID_ROWS)] for _ in range(self.FRAME_GRID_COLS)]
        f32 = np.float32
        for i in range(self.N):
            px = float(f32(f32(self.mvKeysUn["x"][i] - self.mnMinX) * self.mfGridElementWidthInv))
            py = float(f32(f32(self.mvKeysUn["y"][i] - self.mnMinY) * self.mfGridElementHeightInv))
            gx, gy = int(np.floor(abs(px) + 0.5) * np.sign(px)), int(np.floor(abs(py) + 0.5) * np.sign(py))
            if 0 <= gx < self.FRAME_GRID_COLS and 0 <= gy < self.FRAME_GRID_ROWS:
                self.mGrid[gx][gy].append(i)

    def GetFeaturesInArea(self, x, y, r, minLevel=-1, maxLevel=-1):
        """src/Frame.cc:517-570"""
        f32 = np.float32
        x, y, r = f32(x), f32(y), f32(r)
        C, R = self.FRAME_GRID_COLS, self.FRAME_GRID_ROWS
        nMinCellX = max(0, int(np.floor(f32(f32(f32(x - self.mnMinX) - r) * self.mfGridElementWidthInv))))
        if nMinCellX >= C:
            return []
        nMaxCellX = min(C - 1, int(np.ceil(f32(f32(f32(x - self.mnMinX) + r) * self.mfGridElementWidthInv))))
        if nMaxCellX < 0:
            return []
        nMinCellY = max(0, int(np.floor(f32(f32(f32(y - self.mnMinY) - r) * self.mfGridElementHeightInv))))
        if nMinCellY >= R:
            return []
        nMaxCellY = min(R - 1, int(np.ceil(f32(f32(f32(y - self.mnMinY) + r) * self.mfGridElementHeightInv))))
        if nMaxCellY < 0:
            return []
        bCheckLevels = (minLevel > 0) or (maxLevel >= 0)
        out = []
        kx, ky, ko = self.mvKeysUn["x"], self.mvKeysUn["y"], self.mvKeysUn["octave"]
        for ix in range(nMinCellX, nMaxCellX + 1):
            for iy in range(nMinCellY, nMaxCellY + 1):
                for j in self.mGrid[ix][iy]:
                    if bCheckLevels:
                        if ko[j] < minLevel:
                            continue
                        if maxLevel >= 0 and ko[j] > maxLevel:
                            continue
                    if abs(f32(kx[j] - x)) < r and abs(f32(ky[j] - y)) < r:
                        out.append(j)
        return out


class KeyFrameView(FrameView):
    """A FrameView that stands for a KeyFrame* argument (the reference overloads SearchByBoW / SearchByProjection on Frame& / KeyFrame*).
    mp_maxd / mp_mind : (N,) float32, the map points' mfMaxDistance / mfMinDistance (MapPoint::UpdateNormalAndDepth)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.mp_maxd = np.zeros(self.N, np.float32)
        self.mp_mind = np.zeros(self.N, np.float32)


class MapPointView:
    """The MapPoint members read by SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:47-131), gathered by the
    host (mutex-guarded in the reference, src/MapPoint.cc:321-325) into SoA buffers:
    mbTrackInView, isBad : (n,) bool;  mnTrackScaleLevel : (n,) int32;  mTrackViewCos, mTrackProjX, mTrackProjY, mTrackProjXR : (n,) float32;
    descriptor : (n, 32) uint8 (GetDescriptor());  obs : (n,) bool (Observations() > 0)."""

    def __init__(self, descriptor, mTrackProjX, mTrackProjY, mTrackProjXR, mnTrackScaleLevel, mTrackViewCos, mbTrackInView=None, isBad=None,
                 obs=None):
        self.descriptor = np.ascontiguousarray(descriptor, np.uint8).reshape(-1, 32)
        self.n = n = len(self.descriptor)
        f = lambda v: np.ascontiguousarray(v, np.float32).reshape(n)
        self.mTrackProjX, self.mTrackProjY, self.mTrackProjXR, self.mTrackViewCos = f(mTrackProjX), f(mTrackProjY), f(mTrackProjXR), f(mTrackViewCos)
        self.mnTrackScaleLevel = np.ascontiguousarray(mnTrackScaleLevel, np.int32).reshape(n)
        b = lambda v, d: np.full(n, d, bool) if v is None else np.ascontiguousarray(v, bool).reshape(n)
        self.mbTrackInView, self.isBad, self.obs = b(mbTrackInView, True), b(isBad, False), b(obs, True)


class MapPointGeom:
    """The MapPoint members read by the search part of Fuse (src/ORBmatcher.cc:827-948): skip = !pMP || isBad() || IsInKeyFrame(pKF),
    world = GetWorldPos(), normal = GetNormal(), maxd / mind = mfMaxDistance / mfMinDistance, descriptor = GetDescriptor()."""

    def __init__(self, world, normal, maxd, mind, descriptor, skip=None):
        self.descriptor = np.ascontiguousarray(descriptor, np.uint8).reshape(-1, 32)
        self.n = n = len(self.descriptor)
        self.world = np.ascontiguousarray(world, np.float32).reshape(n, 3)
        self.normal = np.ascontiguousarray(normal, np.float32).reshape(n, 3)
        self.maxd, self.mind = np.ascontiguousarray(maxd, np.float32).reshape(n), np.ascontiguousarray(mind, np.float32).reshape(n)
        self.skip = np.zeros(n, bool) if skip is None else np.ascontiguousarray(skip, bool).reshape(n)

    def c_arrays(self):
        """the six arrays as the Fuse family of the C ABI takes them, in its order: skip (one byte each), world, normal, maxd, mind, descriptor"""
        a = np.ascontiguousarray
        return [a(self.skip, np.uint8), a(self.world, np.float32), a(self.normal, np.float32), a(self.maxd, np.float32), a(self.mind, np.float32),
                a(self.descriptor, np.uint8)]


def ComputeThreeMaxima(histo):
    """src/ORBmatcher.cc:1749-1790"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, h in enumerate(histo):
        s = len(h)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif max3 < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def _view_c(v, keep):
    """olf_frame_view of a FrameView / KeyFrameView; every array it points to is appended to `keep` (alive until the call returns).  The bool
    state arrays are passed as they are (one byte per element), so the library's updates land in the view's own arrays."""
    from ._lib import FrameViewC
    c = FrameViewC()

    def p(a, dt=None):
        if a is None:
            return None
        b = np.ascontiguousarray(a if dt is None else np.asarray(a, dt))
        keep.append(b)
        return b.ctypes.data

    def state(name):
        a = getattr(v, name, None)
        if a is None:
            return None
        if not (isinstance(a, np.ndarray) and a.dtype == np.bool_ and a.flags.c_contiguous):
            a = np.ascontiguousarray(a, bool)
            setattr(v, name, a)
        keep.append(a)
        return a.ctypes.data
    c.keys, c.desc, c.uright, c.n = p(v.mvKeysUn), p(v.mDescriptors), p(v.mvuRight, np.float32), v.N
    c.mp_valid, c.mp_obs, c.mp_bad, c.outlier = state("mp_valid"), state("mp_obs"), state("mp_bad"), state("mvbOutlier")
    c.mp_world, c.mp_desc, c.Tcw = p(v.mp_world, np.float32), p(v.mp_desc, np.uint8), p(v.mTcw, np.float32)
    c.fx, c.fy, c.cx, c.cy, c.mbf = float(v.fx), float(v.fy), float(v.cx), float(v.cy), float(v.mbf)
    c.minX, c.maxX, c.minY, c.maxY = float(v.mnMinX), float(v.mnMaxX), float(v.mnMinY), float(v.mnMaxY)
    c.scale_factors, c.n_levels = p(v.mvScaleFactors, np.float32), len(v.mvScaleFactors)
    c.mp_maxd, c.mp_mind = p(getattr(v, "mp_maxd", None), np.float32), p(getattr(v, "mp_mind", None), np.float32)
    nodes = sorted(v.mFeatVec)
    offs = np.zeros(len(nodes) + 1, np.int32)
    offs[1:] = np.cumsum([len(v.mFeatVec[k]) for k in nodes])
    feats = np.array([i for k in nodes for i in v.mFeatVec[k]], np.int32)
    c.fv_nodes, c.fv_offsets, c.fv_features, c.fv_n = p(np.array(nodes, np.int32)), p(offs), p(feats), len(nodes)
    c.grid_offsets, c.grid_index = p(getattr(v, "grid_offsets", None), np.int32), p(getattr(v, "grid_index", None), np.int32)
    return c


def isInFrustum(F, vpMapPoints, viewingCosLimit=0.5):
    """bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit), src/Frame.cc:388-444, for every point of a MapPointGeom (world, normal,
    maxd = mfMaxDistance, mind = mfMinDistance, descriptor) -> olf_is_in_frustum (host arithmetic in the library).  Returns the MapPointView
    that SearchByProjection(Frame, vector<MapPoint*>) reads: mbTrackInView, mnTrackScaleLevel, mTrackViewCos, mTrackProjX / Y / XR."""
    mp = vpMapPoints
    keep = []
    f = _view_c(F, keep)
    inview, level = np.zeros(mp.n, np.uint8), np.zeros(mp.n, np.int32)
    cosv, proj3 = np.zeros(mp.n, np.float32), np.zeros((mp.n, 3), np.float32)
    arrs = mp.c_arrays()[1:5]          # world, normal, maxd, mind
    _call("olf_is_in_frustum", f, mp.n, *(ptr(x) for x in arrs), float(viewingCosLimit), ptr(inview), ptr(level), ptr(cosv), ptr(proj3))
    return MapPointView(mp.descriptor, proj3[:, 0].copy(), proj3[:, 1].copy(), proj3[:, 2].copy(), level, cosv, mbTrackInView=inview.astype(bool),
                        isBad=mp.skip)


def isInFrustum_l(F, lines):
    """bool Frame::isInFrustum_l(MapLine *pML, float viewingCosLimit), src/Frame.cc:446-515, for map lines given as world positions [n, 6] float32 (start,
    then end) -> olf_is_in_frustum_l (host arithmetic in the library).  F: a FrameView (mTcw, the calibration, the bounds).  Returns (mbTrackInView [n]
    bool, proj4 [n, 4] float32 = mTrackProjsX, mTrackProjsY, mTrackProjeX, mTrackProjeY; rows not in view are zero)."""
    keep = []
    f = _view_c(F, keep)
    w = np.ascontiguousarray(lines, np.float32).reshape(-1, 6)
    inview, proj4 = np.zeros(len(w), np.uint8), np.zeros((len(w), 4), np.float32)
    _call("olf_is_in_frustum_l", f, len(w), ptr(w), ptr(inview), ptr(proj4))
    return inview.astype(bool), proj4


def predict_scale_thresholds(scale_factors):
    """olf_predict_scale_thresholds: the ratios mfMaxDistance / dist at which MapPoint::PredictScale (src/MapPoint.cc:414-429) steps, as float32
    [n_levels - 1]; the predicted level of a ratio is the number of thresholds <= it.  Host arithmetic, no device, no context."""
    sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
    thr = np.zeros(max(len(sf) - 1, 0), np.float32)
    _call("olf_predict_scale_thresholds", ptr(sf), len(sf), ptr(thr) if len(thr) else None)
    return thr


def _scale(m, s):
    """cv::Mat (CV_32F) times a scalar: MatExpr scaling, every element times the double factor rounded to float"""
    return (np.asarray(m, np.float32) * np.float32(s)).astype(np.float32)


def _gemv(R, v, t=None, alpha=1.0):
    """alpha * R * v (+ t) on CV_32F operands: double accumulation, one rounding (cv::gemm)"""
    acc = alpha * (np.asarray(R, np.float64) @ np.asarray(v, np.float64))
    if t is not None:
        acc = acc + np.asarray(t, np.float64)
    return acc.astype(np.float32)


def Sim3Decompose(Scw):
    """Scw -> (Rcw, tcw, Ow) as at the top of ORBmatcher::Fuse(pKF, Scw, ...), src/ORBmatcher.cc:985-989"""
    Scw = np.asarray(Scw, np.float32)
    sRcw = Scw[:3, :3]
    scw = np.float32(np.sqrt(np.sum(sRcw[0].astype(np.float64) ** 2)))
    inv = np.float32(1.0 / np.float64(scw))
    Rcw, tcw = _scale(sRcw, inv), _scale(Scw[:3, 3], inv)
    return Rcw, tcw, _gemv(Rcw.T, tcw, alpha=-1.0)


INT_MAX = 2147483647


class ORBmatcher:
    TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30   # src/ORBmatcher.cc:39-41

    def __init__(self, nnratio=0.6, checkOri=True, context=None):
        self.mfNNratio, self.mbCheckOrientation, self._context = float(nnratio), bool(checkOri), context

    @staticmethod
    def DescriptorDistance(a, b):
        return distance(a, b)

    def _search(self, name, *args):
        """the host search `name` on this matcher's context; args from the views on"""
        _call(name, _ctx(self._context).handle, *args)

    def SearchByProjection(self, a, b, *args):
        """The reference overloads SearchByProjection on the second argument: a Frame (:1330; with a trailing map<int,int>& match12 :1474), a
        vector<MapPoint*> (:47) or a KeyFrame* (:1620; with a cv::Mat Scw first :292 -- see SearchByProjectionSim3)."""
        if isinstance(b, KeyFrameView):
            return self._search_by_projection_kf(a, b, *args)
        return self._search_by_projection_frame(a, b, *args)

    def _search_by_projection_frame(self, a, b, th=1.0, bMono=False, match12=None):
        if isinstance(b, MapPointView):
            return self._search_local_map(a, b, th)
        if match12 is not None:
            return self._search_by_projection_match12(a, b, th, bMono, match12)
        return self._search_by_projection(a, b, th, bMono)

    def _search_by_projection(self, CurrentFrame, LastFrame, th, bMono):
        """int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono),
        src/ORBmatcher.cc:1330-1472 -> olf_search_by_projection (host candidate lists and resolution in csrc/search_host.cpp, distances on the
        GPU).  Returns (nmatches, matches) with matches[i2] = index i of the LastFrame map point assigned to CurrentFrame feature i2 (-1 = none);
        CurrentFrame.mp_valid / mp_obs are updated like mvpMapPoints."""
        keep = []
        cur, last = _view_c(CurrentFrame, keep), _view_c(LastFrame, keep)
        matches, n = np.full(CurrentFrame.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_by_projection", cur, last, float(th), int(bool(bMono)), int(bool(self.mbCheckOrientation)), ptr(matches), ptr(n))
        return int(n[0]), matches

    def _search_by_projection_match12(self, CurrentFrame, LastFrame, th, bMono, match12):
        """int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono, map<int,int>& match12),
        src/ORBmatcher.cc:1474-1618 (Tracking::TrackWithMotionModelWithLine, src/Tracking.cc:1296,1302) -> olf_search_by_projection_match12.
        `match12` (a dict) is cleared and filled like the reference's map: key = CurrentFrame feature, value = the FIRST LastFrame feature it was
        matched with; keys in ascending order, as a std::map iterates.  Returns (nmatches, matches) like the four-argument overload."""
        keep = []
        cur, last = _view_c(CurrentFrame, keep), _view_c(LastFrame, keep)
        matches, m12, n = np.full(CurrentFrame.N, -1, np.int32), np.full(CurrentFrame.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_by_projection_match12", cur, last, float(th), int(bool(bMono)), int(bool(self.mbCheckOrientation)), ptr(matches), ptr(m12),
                     ptr(n))
        match12.clear()
        for i2 in np.nonzero(m12 >= 0)[0]:
            match12[int(i2)] = int(m12[i2])
        return int(n[0]), matches

    def _search_local_map(self, F, vpMapPoints, th=1.0):
        """int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th), src/ORBmatcher.cc:47-131
        (Tracking::SearchLocalPoints, every frame) -> olf_search_local_map.  Returns (nmatches, matches) with matches[idx] = index into
        vpMapPoints assigned to feature idx (-1 = none); F.mp_valid / F.mp_obs are updated like F.mvpMapPoints."""
        mp = vpMapPoints
        keep = []
        f = _view_c(F, keep)
        a = np.ascontiguousarray
        proj3 = a(np.stack([mp.mTrackProjX, mp.mTrackProjY, mp.mTrackProjXR], 1), np.float32)
        arrs = [a(mp.mbTrackInView, np.uint8), a(mp.isBad, np.uint8), a(mp.mnTrackScaleLevel, np.int32), a(mp.mTrackViewCos, np.float32), proj3,
                a(mp.descriptor, np.uint8), a(mp.obs, np.uint8)]
        matches, n = np.full(F.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_local_map", f, mp.n, *(ptr(x) for x in arrs), float(th), float(self.mfNNratio), ptr(matches), ptr(n))
        return int(n[0]), matches

    def _search_by_projection_kf(self, CurrentFrame, pKF, sAlreadyFound, th, ORBdist):
        """int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th,
        const int ORBdist), src/ORBmatcher.cc:1620-1747 (relocalisation) -> olf_search_by_projection_kf.  pKF: KeyFrameView with mp_valid /
        mp_bad / mp_world / mp_desc and mp_maxd / mp_mind (mfMaxDistance / mfMinDistance); sAlreadyFound: bool mask over pKF's features.
        Returns (nmatches, matches) with matches[i2] = pKF feature index; CurrentFrame.mp_valid is updated like mvpMapPoints."""
        keep = []
        cur, kf = _view_c(CurrentFrame, keep), _view_c(pKF, keep)
        found = None if sAlreadyFound is None else np.ascontiguousarray(sAlreadyFound, np.uint8)
        matches, n = np.full(CurrentFrame.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_by_projection_kf", cur, kf, None if found is None else ptr(found), float(th), int(ORBdist),
                     int(bool(self.mbCheckOrientation)), ptr(matches), ptr(n))
        return int(n[0]), matches

    def SearchByProjectionSim3(self, pKF, Scw, vpPoints, vpMatched, th):
        """int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th),
        src/ORBmatcher.cc:292-405 (LoopClosing::ComputeSim3, src/LoopClosing.cc:381) -> olf_search_by_projection_sim3.  vpPoints: MapPointView with
        skip = isBad() || (the point is already in vpMatched); vpMatched: bool array over pKF's key points (vpMatched[idx] != NULL), updated in
        place.  Returns (nmatches, matches) with matches[idx] = index into vpPoints that key point idx received (-1 = none)."""
        mp = vpPoints
        keep = []
        kf = _view_c(pKF, keep)
        S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        arrs = mp.c_arrays()
        if not (isinstance(vpMatched, np.ndarray) and vpMatched.dtype == np.bool_ and vpMatched.flags.c_contiguous and len(vpMatched) == pKF.N):
            raise ValueError("vpMatched: a C-contiguous bool array with one entry per key point of pKF (updated in place)")
        matches, n = np.full(pKF.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_by_projection_sim3", kf, ptr(S), mp.n, *(ptr(x) for x in arrs), float(th), vpMatched.ctypes.data, ptr(matches), ptr(n))
        return int(n[0]), matches

    def SearchForInitialization(self, F1, F2, vbPrevMatched, windowSize=10):
        """int ORBmatcher::SearchForInitialization(Frame &F1, Frame &F2, vector<cv::Point2f> &vbPrevMatched, vector<int> &vnMatches12,
        int windowSize), src/ORBmatcher.cc:407-522 (monocular initialisation) -> olf_search_for_initialization.  vbPrevMatched: float32 [N1, 2],
        updated in place like the reference's vector.  Returns (nmatches, vnMatches12)."""
        keep = []
        f1, f2 = _view_c(F1, keep), _view_c(F2, keep)
        if not (isinstance(vbPrevMatched, np.ndarray) and vbPrevMatched.dtype == np.float32 and vbPrevMatched.flags.c_contiguous
                and vbPrevMatched.shape == (F1.N, 2)):
            raise ValueError("vbPrevMatched: contiguous float32 array of shape (F1.N, 2)")
        m, n = np.full(F1.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_for_initialization", f1, f2, ptr(vbPrevMatched), int(windowSize), float(self.mfNNratio), int(bool(self.mbCheckOrientation)),
                     ptr(m), ptr(n))
        return int(n[0]), m

    def SearchByBoW(self, pKF, other):
        """The reference overloads SearchByBoW on the second argument: a Frame (:161) or a KeyFrame* (:524)."""
        return self._search_by_bow_kf(pKF, other) if isinstance(other, KeyFrameView) else self._search_by_bow(pKF, other)

    def _search_by_bow(self, pKF, F):
        """int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches), src/ORBmatcher.cc:161-290 ->
        olf_search_by_bow.  Returns (nmatches, vpMapPointMatches) with vpMapPointMatches[iF] = KF feature index whose map point was matched
        (-1 = none)."""
        keep = []
        kf, f = _view_c(pKF, keep), _view_c(F, keep)
        matched, n = np.full(F.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_by_bow", kf, f, float(self.mfNNratio), int(bool(self.mbCheckOrientation)), ptr(matched), ptr(n))
        return int(n[0]), matched

    def _search_by_bow_kf(self, pKF1, pKF2):
        """int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12), src/ORBmatcher.cc:524-657 (loop closing)
        -> olf_search_by_bow_kf.  Returns (nmatches, vpMatches12) with vpMatches12[idx1] = feature index idx2 of pKF2 whose map point is taken
        (-1 = NULL)."""
        keep = []
        k1, k2 = _view_c(pKF1, keep), _view_c(pKF2, keep)
        m12, n = np.full(pKF1.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_by_bow_kf", k1, k2, float(self.mfNNratio), int(bool(self.mbCheckOrientation)), ptr(m12), ptr(n))
        return int(n[0]), m12

    def SearchForTriangulation(self, pKF1, pKF2, F12, bOnlyStereo, Cw=None):
        """int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs,
        const bool bOnlyStereo), src/ORBmatcher.cc:659-825 (LocalMapping::CreateNewMapPoints) -> olf_search_for_triangulation.  Cw =
        pKF1->GetCameraCenter() (default: from pKF1.mTcw); pKF2.mTcw gives R2w / t2w.  Returns (nmatches, vMatchedPairs) with vMatchedPairs =
        [(idx1, idx2), ...] in idx1 order."""
        keep = []
        k1, k2 = _view_c(pKF1, keep), _view_c(pKF2, keep)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        cw = None if Cw is None else np.ascontiguousarray(Cw, np.float32).reshape(3)
        m12, n = np.full(pKF1.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_for_triangulation", k1, k2, ptr(F), None if cw is None else ptr(cw), int(bool(bOnlyStereo)),
                     int(bool(self.mbCheckOrientation)), ptr(m12), ptr(n))
        return int(n[0]), [(int(i), int(m12[i])) for i in range(pKF1.N) if m12[i] >= 0]

    def FuseSearch(self, pKF, vpMapPoints, th=3.0, Ow=None):
        """The search part of int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th), src/ORBmatcher.cc:827-948
        -> olf_fuse_search: per map point the most similar key point of pKF inside the projection window.  Returns (bestIdx, bestDist) arrays
        (-1 / 256 where a gate rejects the point).  The reference's loop then fuses when bestDist <= TH_LOW (:950-972: Replace / AddObservation
        on the map, host code); that mutation never feeds back into another point's search, so the loop body splits exactly there."""
        mp = vpMapPoints
        keep = []
        kf = _view_c(pKF, keep)
        arrs = mp.c_arrays()
        ow = None if Ow is None else np.ascontiguousarray(Ow, np.float32).reshape(3)
        bi, bd = np.full(mp.n, -1, np.int32), np.full(mp.n, 256, np.int32)
        self._search("olf_fuse_search", kf, mp.n, *(ptr(x) for x in arrs), float(th), None if ow is None else ptr(ow), ptr(bi), ptr(bd))
        return bi, bd

    def FuseSearchSim3(self, pKF, Scw, vpPoints, th):
        """The search part of int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th,
        vector<MapPoint*> &vpReplacePoint), src/ORBmatcher.cc:977-1102 (loop correction) -> olf_fuse_search_sim3: per point the most similar key
        point of pKF inside the projection window under the Sim3 pose, (bestIdx, bestDist), (-1, INT_MAX) where a gate rejects the point.
        vpPoints.skip = isBad() || spAlreadyFound.count(pMP).  The reference then records a replacement / adds the observation when
        bestDist <= TH_LOW (:1086-1099, host code on the map)."""
        mp = vpPoints
        keep = []
        kf = _view_c(pKF, keep)
        S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        arrs = mp.c_arrays()
        bi, bd = np.full(mp.n, -1, np.int32), np.full(mp.n, INT_MAX, np.int32)
        self._search("olf_fuse_search_sim3", kf, ptr(S), mp.n, *(ptr(x) for x in arrs), float(th), ptr(bi), ptr(bd))
        return bi, bd.astype(np.int64)

    def SearchBySim3(self, pKF1, pKF2, vpMatches12, s12, R12, t12, th):
        """int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12,
        const cv::Mat &t12, const float th), src/ORBmatcher.cc:1104-1328 -> olf_search_by_sim3.  pKF1 / pKF2: KeyFrameView (mp_valid, mp_bad,
        mp_world, mp_desc, mp_maxd, mp_mind, mTcw).  vpMatches12: int array over pKF1's features, the index in pKF2 of the feature whose map
        point is already matched (pMP->GetIndexInKeyFrame(pKF2)), -1 for none, or -2 for "matched to a map point that pKF2 does not observe";
        updated in place like the reference's vector.  Returns (nFound, vnMatch1, vnMatch2)."""
        keep = []
        k1, k2 = _view_c(pKF1, keep), _view_c(pKF2, keep)
        m12 = np.ascontiguousarray(vpMatches12, np.int32)
        R, t = np.ascontiguousarray(R12, np.float32).reshape(9), np.ascontiguousarray(t12, np.float32).reshape(3)
        v1, v2, n = np.full(pKF1.N, -1, np.int32), np.full(pKF2.N, -1, np.int32), np.zeros(1, np.int32)
        self._search("olf_search_by_sim3", k1, k2, ptr(m12), float(s12), ptr(R), ptr(t), float(th), ptr(v1), ptr(v2), ptr(n))
        vpMatches12[...] = m12
        return int(n[0]), v1, v2


# ------------------------------------------------------------------------------------------------------------------
# 3. Wrappers of the batched device entries.  The arrays are torch device tensors (or raw device addresses); every entry runs on torch's current
# stream.  Each wrapper checks its arguments (_dev), fills the structures of the C ABI (_track_batch_c / _line_batch_c, the local maps' c()), makes
# the output tensors the caller did not give (_new) and calls the entry (_call_dev).
def _dev(a, dtype=None, what="argument"):
    """device address of a torch tensor (checked: on the GPU, contiguous, of `dtype`), of a raw address (int), or None"""
    if a is None or isinstance(a, int):
        return a
    import torch
    if not (isinstance(a, torch.Tensor) and a.is_cuda and a.is_contiguous() and (dtype is None or a.dtype == dtype)):
        raise TypeError(f"{what}: a contiguous device tensor of {dtype} (or a device address) expected")
    return a.data_ptr()


class _torch_stream:
    """The stream handle that orders a *_dev entry with torch's work: torch's current stream -- or, when that is the default stream (whose handle, 0,
    means "the context's own stream" to the library), the context's stream between two device-wide synchronisations."""

    def __enter__(self):
        import torch
        self.handle = torch.cuda.current_stream().cuda_stream
        if not self.handle:
            torch.cuda.synchronize()
        return self.handle or None

    def __exit__(self, *exc):
        if not self.handle:
            import torch
            torch.cuda.synchronize()
        return False


def _call_dev(name, ctx, *args):
    """the device entry `name` of context ctx on args, on the stream _torch_stream names, its return code checked"""
    with _torch_stream() as s:
        _call(name, ctx.handle, *args, s)


def _new(shape, fill=0, dtype=None):
    """a default output tensor on the device: int32 (or `dtype`), filled with -1, 0, 256 or INT_MAX"""
    import torch
    dtype = torch.int32 if dtype is None else dtype
    return torch.zeros(shape, dtype=dtype, device="cuda") if fill == 0 else torch.full(shape, fill, dtype=dtype, device="cuda")


def _track_batch_c(kps, desc, counts, img_stride, uright, cell_offsets, cell_index, Tcw, camera, bounds, mp_world=None, mp_valid=None, mp_obs=None,
                   outlier=None, mp_desc=None):
    """olf_track_batch (include/orbline.h): the frames of a device-resident batch as the batched point matchers read them.  kps / desc / counts per
    image in the extractor's layout, frame j = image j * img_stride; uright, the grids, Tcw and the per-feature planes mp_* / outlier per frame
    ([n_frames, capacity, ..]); camera = (fx, fy, cx, cy, mbf); bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY).  An entry names the planes it reads; the
    rest may be None."""
    import torch
    tb = _lib.TrackBatchC()
    tb.kps, tb.desc, tb.counts, tb.img_stride = _dev(kps, None, "kps"), _dev(desc, torch.uint8, "desc"), _dev(counts, torch.int32, "counts"), int(img_stride)
    tb.uright, tb.cell_offsets, tb.cell_index = _dev(uright, torch.float32, "uright"), _dev(cell_offsets, torch.int32, "cell_offsets"), _dev(cell_index, torch.int32, "cell_index")
    tb.Tcw, tb.mp_world = _dev(Tcw, torch.float32, "Tcw"), _dev(mp_world, torch.float32, "mp_world")
    tb.mp_valid, tb.mp_obs, tb.outlier = _dev(mp_valid, torch.uint8, "mp_valid"), _dev(mp_obs, torch.uint8, "mp_obs"), _dev(outlier, torch.uint8, "outlier")
    tb.mp_desc = _dev(mp_desc, torch.uint8, "mp_desc")
    tb.fx, tb.fy, tb.cx, tb.cy, tb.mbf = (float(v) for v in camera)
    tb.minX, tb.maxX, tb.minY, tb.maxY = (float(v) for v in bounds)
    return tb


def _line_batch_c(kls, ldesc, lcounts, img_stride, ldisp, Tcw, camera, bounds):
    """olf_line_batch (include/orbline.h): _track_batch_c's counterpart for the batched line matchers"""
    import torch
    lb = _lib.LineBatchC()
    lb.kls, lb.ldesc, lb.lcounts, lb.img_stride = _dev(kls, None, "kls"), _dev(ldesc, torch.uint8, "ldesc"), _dev(lcounts, torch.int32, "lcounts"), int(img_stride)
    lb.ldisp, lb.Tcw = _dev(ldisp, torch.float32, "ldisp"), _dev(Tcw, torch.float32, "Tcw")
    lb.fx, lb.fy, lb.cx, lb.cy = (float(v) for v in camera[:4])
    lb.minX, lb.maxX, lb.minY, lb.maxY = (float(v) for v in bounds)
    return lb


def _cam5(camera):
    """camera = (fx, fy, cx, cy[, mbf]) with the mbf an entry does not read as 0"""
    return tuple(camera) + (0.0,) * (5 - len(tuple(camera)))


class _LocalListsDev:
    """What LocalMapDev and LocalLineMapDev share: optionally every frame's list of map entries as (list_offsets [n_frames + 1], list_index
    [n_entries]) int32 device tensors.  Without lists every frame sees all entries of the map (self.n_map of them) in index order."""
    n_map = 0

    def n_entries(self, n_frames):
        if self.list_offsets is None:
            return int(n_frames) * self.n_map
        return 0 if self.list_index is None else int(self.list_index.shape[0])

    def _lists_c(self, m, n_frames):
        import torch
        m.list_offsets, m.list_index = _dev(self.list_offsets, torch.int32, "list_offsets"), _dev(self.list_index, torch.int32, "list_index")
        m.n_entries = self.n_entries(n_frames)
        return m


class LocalMapDev(_LocalListsDev):
    """olf_local_map (include/orbline.h): the local map a batch of frames is matched against, as device tensors over n_mp points -- world, normal
    [n_mp, 3] float32, maxd / mind [n_mp] float32 (mfMaxDistance / mfMinDistance, unscaled), desc [n_mp, 32] uint8, obs / bad [n_mp] uint8 -- and
    optionally every frame's mvpLocalMapPoints as (list_offsets [n_frames + 1], list_index [n_entries]) int32.  Without lists every frame sees all
    points in index order.  n_mp: the number of points (default: the length of bad)."""
    n_map = property(lambda self: self.n_mp)

    def __init__(self, world, normal, maxd, mind, desc, obs, bad, list_offsets=None, list_index=None, n_mp=None):
        self.world, self.normal, self.maxd, self.mind, self.desc, self.obs, self.bad = world, normal, maxd, mind, desc, obs, bad
        self.list_offsets, self.list_index = list_offsets, list_index
        self.n_mp = int(bad.shape[0]) if n_mp is None else int(n_mp)

    def c(self, n_frames):
        import torch
        m = _lib.LocalMapC()
        m.world, m.normal, m.maxd, m.mind = (_dev(getattr(self, k), torch.float32, k) for k in ("world", "normal", "maxd", "mind"))
        m.desc, m.obs, m.bad = (_dev(getattr(self, k), torch.uint8, k) for k in ("desc", "obs", "bad"))
        m.n_mp = self.n_mp
        return self._lists_c(m, n_frames)


class LocalLineMapDev(_LocalListsDev):
    """olf_local_line_map (include/orbline.h): the map lines a batch of frames is matched against, as device tensors over n_ml lines -- world [n_ml, 6]
    float32 (GetWorldPos(): start, then end), desc [n_ml, 32] uint8, obs / bad [n_ml] uint8 -- and optionally every frame's mvpLocalMapLines as
    (list_offsets [n_frames + 1], list_index [n_entries]) int32.  Without lists every frame sees all lines in index order."""
    n_map = property(lambda self: self.n_ml)

    def __init__(self, world, desc, obs, bad, list_offsets=None, list_index=None, n_ml=None):
        self.world, self.desc, self.obs, self.bad = world, desc, obs, bad
        self.list_offsets, self.list_index = list_offsets, list_index
        self.n_ml = int(bad.shape[0]) if n_ml is None else int(n_ml)

    def c(self, n_frames):
        import torch
        m = _lib.LocalLineMapC()
        m.world = _dev(self.world, torch.float32, "world")
        m.desc, m.obs, m.bad = (_dev(getattr(self, k), torch.uint8, k) for k in ("desc", "obs", "bad"))
        m.n_ml = self.n_ml
        return self._lists_c(m, n_frames)


def unproject_stereo(n_frames, kps, counts, depth, camera, Twc, img_stride=2, out=None, context=None):
    """Frame::UnprojectStereo (src/Frame.cc:1073-1087) for every feature of n_frames device-resident frames: olf_unproject_stereo_dev.  kps / counts in
    the extractor's layout, depth [n_frames, capacity] (mvDepth), camera = (fx, fy, cx, cy), Twc [n_frames, 4, 4] camera-to-world (rows of mRwc | mOw).
    Returns world [n_frames, capacity, 3] float32 on the device ((0, 0, 0) where the reference returns an empty cv::Mat).  torch's current stream."""
    import torch
    ctx = _ctx(context)
    world = _new((int(n_frames), ctx.orb_capacity, 3), 0, torch.float32) if out is None else out
    _call_dev("olf_unproject_stereo_dev", ctx, int(n_frames), int(img_stride), _dev(kps, None, "kps"), _dev(counts, torch.int32, "counts"),
              _dev(depth, torch.float32, "depth"), *(float(v) for v in camera), _dev(Twc, torch.float32, "Twc"), _dev(world, torch.float32, "world"))
    return world


def search_by_projection_batch(n_frames, kps, desc, counts, uright, cell_offsets, cell_index, Tcw, mp_world, camera, bounds, th, bMono=False,
                               checkOri=True, img_stride=2, mp_valid=None, mp_obs=None, outlier=None, mp_desc=None, d_th=None, match12=True, out=None,
                               context=None):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono[, match12]) (src/ORBmatcher.cc:1330-1472, :1474-1618) for the n_frames - 1
    consecutive pairs of a device-resident batch: olf_search_by_projection_batch_dev (include/orbline.h describes every array; csrc/track_batch.hip).
    The arrays are torch device tensors (or raw device addresses) in the extractor's layout -- kps / desc / counts per image, frame j = image
    j * img_stride -- and per-frame planes [n_frames, capacity] for the rest; the context must be the one whose capacity they were made for.
    camera = (fx, fy, cx, cy, mbf); bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY); d_th: float32 [n_frames - 1] per-pair radii (<= 0 skips a pair).
    match12: also return the reference's match12 map as an array.  out = (matches, match12 or None, nmatches): int32 tensors to write into (rows of
    skipped pairs keep what they hold); by default they are made here, filled with -1.  Runs on torch's current stream.
    Returns (matches [n_frames - 1, capacity], match12 or None, nmatches [n_frames - 1]) as device tensors."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    cap, n_pairs = ctx.orb_capacity, max(int(n_frames) - 1, 0)
    tb = _track_batch_c(kps, desc, counts, img_stride, uright, cell_offsets, cell_index, Tcw, camera, bounds, mp_world=mp_world, mp_valid=mp_valid,
                        mp_obs=mp_obs, outlier=outlier, mp_desc=mp_desc)
    if out is None:
        out = (_new((n_pairs, cap), -1), _new((n_pairs, cap), -1) if match12 else None, _new((n_pairs,), -1))
    m, m12, n = out
    _call_dev("olf_search_by_projection_batch_dev", ctx, C.byref(tb), int(n_frames), float(th), _dev(d_th, torch.float32, "d_th"), int(bool(bMono)),
              int(bool(checkOri)), _dev(m, torch.int32, "matches"), _dev(m12, torch.int32, "match12"), _dev(n, torch.int32, "nmatches"))
    return m, m12, n


def search_for_triangulation_batch(voc, n_frames, kps, desc, counts, uright, Tcw, pairs, F12, camera, Cw=None, mp_valid=None, bOnlyStereo=False,
                                   checkOri=True, levelsup=4, img_stride=2, out=None, context=None):
    """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, Cw) (src/ORBmatcher.cc:659-825; LocalMapping::CreateNewMapPoints,
    src/LocalMapping.cc:268) for a list of key-frame pairs of a device-resident batch, Frame::ComputeBoW of every frame included:
    olf_search_for_triangulation_batch_dev (include/orbline.h describes every array; csrc/triangulation_batch.hip).  voc: an ORBVocabulary.  The arrays
    are torch device tensors (or raw device addresses): kps / desc / counts in the extractor's layout (frame j = image j * img_stride), uright and
    mp_valid [n_frames, capacity], Tcw [n_frames, 4, 4]; pairs int32 [n_pairs, 2] = (kf1, kf2) frame indices; F12 float32 [n_pairs, 3, 3], used as
    x1^T F12 x2; Cw float32 [n_pairs, 3] (None: kf1's camera centre from its Tcw); camera = (fx, fy, cx, cy).  mp_valid marks the features that hold a
    map point -- the search takes the others -- so None searches nothing.  out = (matches12, nmatches): int32 tensors to write into (rows of refused
    pairs keep what they hold); by default they are made here, filled with -1 and 0.  Runs on torch's current stream.
    Returns (matches12 [n_pairs, capacity]: idx2 per idx1 or -1, nmatches [n_pairs]) as device tensors."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    n_pairs = int(pairs.shape[0])
    fx, fy, cx, cy = camera
    tb = _track_batch_c(kps, desc, counts, img_stride, uright, None, None, Tcw, (fx, fy, cx, cy, 0.0), (0.0,) * 4, mp_valid=mp_valid)
    if tuple(pairs.shape) != (n_pairs, 2) or F12.numel() != 9 * n_pairs or (Cw is not None and Cw.numel() != 3 * n_pairs):
        raise ValueError("search_for_triangulation_batch: pairs [n_pairs, 2], F12 [n_pairs, 3, 3], Cw [n_pairs, 3]")
    if out is None:
        out = (_new((n_pairs, ctx.orb_capacity), -1), _new((n_pairs,)))
    m, n = out
    _call_dev("olf_search_for_triangulation_batch_dev", ctx, voc._h, C.byref(tb), int(n_frames), n_pairs, _dev(pairs, torch.int32, "pairs"),
              _dev(F12, torch.float32, "F12"), _dev(Cw, torch.float32, "Cw"), int(bool(bOnlyStereo)), int(bool(checkOri)), int(levelsup),
              _dev(m, torch.int32, "matches12"), _dev(n, torch.int32, "nmatches"))
    return out


BOW_KF_FRAME, BOW_KF_KF = 0, 1      # OLF_BOW_KF_FRAME, OLF_BOW_KF_KF (include/orbline.h): the two SearchByBoW overloads of search_by_bow_pairs


def search_by_bow_pairs(voc, n_frames, kps, desc, counts, pairs, mp_valid=None, mp_bad=None, form=BOW_KF_FRAME, nnratio=0.7, checkOri=True, levelsup=4,
                        img_stride=2, out=None, context=None):
    """ORBmatcher::SearchByBoW for a list of pairs of a device-resident batch, Frame::ComputeBoW of every frame included: olf_search_by_bow_pairs_dev
    (include/orbline.h describes every array; csrc/bow_match.hip).  form BOW_KF_FRAME: SearchByBoW(pKF, F, vpMapPointMatches) (src/ORBmatcher.cc:161-290;
    Tracking::TrackReferenceKeyFrame, Tracking::Relocalization), pairs = (pKF, F); form BOW_KF_KF: SearchByBoW(pKF1, pKF2, vpMatches12) (:524-657;
    LoopClosing::ComputeSim3), pairs = (pKF1, pKF2).  voc: an ORBVocabulary.  The arrays are torch device tensors (or raw device addresses): kps / desc /
    counts in the extractor's layout (frame j = image j * img_stride), mp_valid and mp_bad uint8 [n_frames, capacity] (None: every feature holds a
    point / no point is bad), pairs int32 [n_pairs, 2], any order, duplicates allowed.  out = (matches, nmatches): int32 tensors to write into (rows of
    refused pairs keep what they hold); by default they are made here, filled with -1 and 0.  Runs on torch's current stream.
    Returns (matches [n_pairs, capacity], nmatches [n_pairs]) as device tensors: row p is indexed by the feature of F and holds the pKF feature whose
    point it received (BOW_KF_FRAME), or is indexed by idx1 and holds idx2 (BOW_KF_KF); -1 = none."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    n_pairs = int(pairs.shape[0])
    if tuple(pairs.shape) != (n_pairs, 2):
        raise ValueError("search_by_bow_pairs: pairs [n_pairs, 2]")
    tb = _track_batch_c(kps, desc, counts, img_stride, None, None, None, None, (0.0,) * 5, (0.0,) * 4, mp_valid=mp_valid)
    if out is None:
        out = (_new((n_pairs, ctx.orb_capacity), -1), _new((n_pairs,)))
    m, n = out
    _call_dev("olf_search_by_bow_pairs_dev", ctx, voc._h, C.byref(tb), int(n_frames), n_pairs, _dev(pairs, torch.int32, "pairs"),
              _dev(mp_bad, torch.uint8, "mp_bad"), int(form), float(nnratio), int(bool(checkOri)), int(levelsup), _dev(m, torch.int32, "matches"),
              _dev(n, torch.int32, "nmatches"))
    return out


def is_in_frustum_batch(n_frames, Tcw, local_map, camera, bounds, viewingCosLimit=0.5, frame_mp=None, counts=None, img_stride=2, out=None, context=None):
    """Frame::isInFrustum (src/Frame.cc:388-444) for every (frame, local map point) of a device-resident batch, with the bad / already-held tests of
    Tracking::SearchLocalPointsAndLines (src/Tracking.cc:1880-1896, :1921-1924): olf_is_in_frustum_batch_dev (include/orbline.h).  Tcw [n_frames, 4, 4];
    local_map: a LocalMapDev; camera = (fx, fy, cx, cy, mbf); bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY); frame_mp int32 [n_frames, capacity]: the
    frames' mvpMapPoints as map indices (negative: none), counts (extractor layout, with img_stride): their N.  Runs on torch's current stream.
    Returns (in_view uint8, level int32, view_cos float32, proj3 float32 [.., 3]) over the entries (LocalMapDev.n_entries); entries not in view keep
    what `out` held (zeros by default) in the last three."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    ne = local_map.n_entries(n_frames)
    tb = _track_batch_c(None, None, counts, img_stride, None, None, None, Tcw, camera, bounds)
    lm = local_map.c(n_frames)
    if out is None:
        out = (_new((ne,), 0, torch.uint8), _new((ne,)), _new((ne,), 0, torch.float32), _new((ne, 3), 0, torch.float32))
    v, l, c, p = out
    _call_dev("olf_is_in_frustum_batch_dev", ctx, C.byref(tb), int(n_frames), C.byref(lm), _dev(frame_mp, torch.int32, "frame_mp"), float(viewingCosLimit),
              _dev(v, torch.uint8, "in_view"), _dev(l, torch.int32, "level"), _dev(c, torch.float32, "view_cos"), _dev(p, torch.float32, "proj3"))
    return out


def search_local_map_batch(n_frames, kps, desc, counts, uright, cell_offsets, cell_index, Tcw, local_map, camera, bounds, th=1.0, nnratio=0.8,
                           viewingCosLimit=0.5, frame_mp=None, d_th=None, img_stride=2, out=None, context=None):
    """The point half of Tracking::SearchLocalPointsAndLines (src/Tracking.cc:1877-1942) for a device-resident batch: Frame::isInFrustum for every
    (frame, local map point), then ORBmatcher(nnratio).SearchByProjection(F, mvpLocalMapPoints, th) (src/ORBmatcher.cc:47-131) for every frame --
    olf_search_local_map_batch_dev (include/orbline.h describes every array; csrc/local_batch.hip).  The frame arrays are those of
    search_by_projection_batch; local_map: a LocalMapDev; frame_mp int32 [n_frames, capacity]: mvpMapPoints on entry as map indices (negative: none);
    d_th float32 [n_frames]: per-frame radius factors (<= 0 skips a frame, whose rows of `out` keep what they hold).  out = (matches, nmatches).
    Runs on torch's current stream.  Returns (matches [n_frames, capacity]: the map index feature idx received, -1 none; nmatches [n_frames])."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    tb = _track_batch_c(kps, desc, counts, img_stride, uright, cell_offsets, cell_index, Tcw, camera, bounds)
    lm = local_map.c(n_frames)
    if out is None:
        out = (_new((int(n_frames), ctx.orb_capacity), -1), _new((int(n_frames),)))
    m, n = out
    _call_dev("olf_search_local_map_batch_dev", ctx, C.byref(tb), int(n_frames), C.byref(lm), _dev(frame_mp, torch.int32, "frame_mp"), float(viewingCosLimit),
              float(th), _dev(d_th, torch.float32, "d_th"), float(nnratio), _dev(m, torch.int32, "matches"), _dev(n, torch.int32, "nmatches"))
    return out


def fuse_search_batch(n_frames, kps, desc, counts, uright, cell_offsets, cell_index, Tcw, local_map, camera, bounds, th=3.0, Scw=None, Ow=None,
                      frame_mp=None, img_stride=2, out=None, context=None):
    """The search part of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:827-948; LocalMapping::SearchInNeighbors, src/LocalMapping.cc:489,
    :514) -- or, with Scw, of Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:977-1102; LoopClosing::SearchAndFuse, src/LoopClosing.cc:605) -- for every key
    frame of a device-resident batch: olf_fuse_search_batch_dev (include/orbline.h describes every array; csrc/fuse_batch.hip).  The frame arrays are those
    of search_local_map_batch; local_map: a LocalMapDev (obs is not read and may be None) whose lists, if any, are the points each key frame is searched
    for; Scw float32 [n_frames, 4, 4]: the Sim3 poses (Tcw is then not read and may be None); Ow float32 [n_frames, 3]: GetCameraCenter() (None: from
    Tcw; plain form only); frame_mp int32 [n_frames, capacity]: the key frames' mvpMapPoints as map indices (negative: none) -- a point its key frame
    holds is skipped.  out = (best_idx, best_dist, nfused): int32 tensors to write into.  Runs on torch's current stream.
    Returns (best_idx, best_dist) over the entries (LocalMapDev.n_entries; -1 / 256, or -1 / INT_MAX with Scw, where nothing was found) and nfused
    [n_frames]: the entries per key frame with best_idx >= 0 and best_dist <= TH_LOW."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    tb = _track_batch_c(kps, desc, counts, img_stride, uright, cell_offsets, cell_index, Tcw, camera, bounds)
    lm = local_map.c(n_frames)
    if out is None:
        ne = local_map.n_entries(n_frames)
        out = (_new((ne,), -1), _new((ne,), 256 if Scw is None else INT_MAX), _new((int(n_frames),)))
    bi, bd, nf = out
    _call_dev("olf_fuse_search_batch_dev", ctx, C.byref(tb), int(n_frames), C.byref(lm), _dev(frame_mp, torch.int32, "frame_mp"),
              _dev(Scw, torch.float32, "Scw"), _dev(Ow, torch.float32, "Ow"), float(th), _dev(bi, torch.int32, "best_idx"),
              _dev(bd, torch.int32, "best_dist"), _dev(nf, torch.int32, "nfused"))
    return out


def search_by_sim3_pairs(n_frames, kps, desc, counts, cell_offsets, cell_index, Tcw, mp_world, mp_maxd, mp_mind, pairs, s12, R12, t12, camera, bounds,
                         matches12=None, th=7.5, mp_valid=None, mp_bad=None, mp_desc=None, img_stride=2, out=None, context=None):
    """ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1104-1328; LoopClosing::ComputeSim3,
    src/LoopClosing.cc:329) for a list of key-frame pairs of a device-resident batch, each with its own similarity: olf_search_by_sim3_pairs_dev
    (include/orbline.h describes every array; csrc/sim3_batch.hip).  The arrays are torch device tensors (or raw device addresses): kps / desc / counts in
    the extractor's layout (frame j = image j * img_stride), the grids of olf_frame_grid_dev, Tcw [n_frames, 4, 4]; per feature [n_frames, capacity]:
    mp_world [.., 3], mp_maxd / mp_mind float32 (unscaled), mp_valid / mp_bad uint8 (None: every feature holds a point / no point is bad), mp_desc
    [.., 32] uint8 (None: the frame's own descriptors); pairs int32 [n_pairs, 2] = (kf1, kf2), any order, duplicates allowed; s12 [n_pairs], R12
    [n_pairs, 3, 3], t12 [n_pairs, 3] float32; camera = (fx, fy, cx, cy[, mbf]); bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY).  matches12 int32
    [n_pairs, capacity] is vpMatches12 on entry (-1 NULL, >= 0 the index in kf2, -2 a point kf2 does not observe) and is written in place; None: no
    pre-matches, a tensor of -1 is made here.  out = (vn_match1, vn_match2, nfound): int32 tensors to write into, either of the first two None to keep that
    row in context scratch (rows of refused pairs keep what they hold); by default all three are made here.  Runs on torch's current stream.
    Returns (matches12, vn_match1, vn_match2, nfound) as device tensors: row p of matches12 holds per feature of kf1 the agreed feature of kf2 beside the
    pre-matches, vn_match1 / vn_match2 [n_pairs, capacity] the reference's vnMatch1 / vnMatch2 (-1 from N on), nfound [n_pairs] the return values."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    n_pairs, cap = int(pairs.shape[0]), ctx.orb_capacity
    if tuple(pairs.shape) != (n_pairs, 2) or s12.numel() != n_pairs or R12.numel() != 9 * n_pairs or t12.numel() != 3 * n_pairs:
        raise ValueError("search_by_sim3_pairs: pairs [n_pairs, 2], s12 [n_pairs], R12 [n_pairs, 3, 3], t12 [n_pairs, 3]")
    tb = _track_batch_c(kps, desc, counts, img_stride, None, cell_offsets, cell_index, Tcw, _cam5(camera), bounds, mp_world=mp_world, mp_valid=mp_valid,
                        mp_desc=mp_desc)
    if matches12 is None:
        matches12 = _new((n_pairs, cap), -1)
    if out is None:
        out = (_new((n_pairs, cap), -1), _new((n_pairs, cap), -1), _new((n_pairs,)))
    v1, v2, nf = out
    _call_dev("olf_search_by_sim3_pairs_dev", ctx, C.byref(tb), int(n_frames), _dev(mp_bad, torch.uint8, "mp_bad"), _dev(mp_maxd, torch.float32, "mp_maxd"),
              _dev(mp_mind, torch.float32, "mp_mind"), n_pairs, _dev(pairs, torch.int32, "pairs"), _dev(s12, torch.float32, "s12"),
              _dev(R12, torch.float32, "R12"), _dev(t12, torch.float32, "t12"), float(th), _dev(matches12, torch.int32, "matches12"),
              _dev(v1, torch.int32, "vn_match1"), _dev(v2, torch.int32, "vn_match2"), _dev(nf, torch.int32, "nfound"))
    return matches12, v1, v2, nf


def search_by_projection_kf_pairs(n_frames, kps, desc, counts, cell_offsets, cell_index, mp_world, mp_maxd, mp_mind, pairs, camera, bounds, th=10.0,
                                  ORBdist=100, Tcw=None, pair_Tcw=None, cur_valid=None, already_found=None, d_th=None, d_orb_dist=None, checkOri=True,
                                  mp_valid=None, mp_bad=None, mp_desc=None, img_stride=2, out=None, context=None):
    """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1620-1747; Tracking::Relocalization,
    src/Tracking.cc:2322, :2336) for a list of (current frame, key frame) pairs of a device-resident batch, each with its own pose:
    olf_search_by_projection_kf_pairs_dev (include/orbline.h describes every array; csrc/projection_batch.hip).  The arrays are torch device tensors (or
    raw device addresses): kps / desc / counts in the extractor's layout (frame j = image j * img_stride), the grids of olf_frame_grid_dev; per feature
    [n_frames, capacity] in the key-frame role: mp_world [.., 3], mp_maxd / mp_mind float32 (unscaled), mp_valid / mp_bad uint8 (None: every feature
    holds a point / no point is bad), mp_desc [.., 32] uint8 (None: the frame's own descriptors); pairs int32 [n_pairs, 2] = (current frame, key frame).
    pair_Tcw float32 [n_pairs, 4, 4]: the current frame's pose under each candidate (None: Tcw [n_frames, 4, 4] of the current frame); cur_valid uint8
    [n_pairs, capacity]: CurrentFrame.mvpMapPoints[i2] != NULL on entry; already_found uint8 [n_pairs, capacity]: sAlreadyFound over the key frame's
    features; d_th float32 / d_orb_dist int32 [n_pairs]: per-pair values that replace th / ORBdist (d_th <= 0 skips a pair).  camera = (fx, fy, cx,
    cy[, mbf]); bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY).  out = (matches, nmatches): int32 tensors to write into (rows of skipped and refused pairs
    keep what they hold); by default they are made here, filled with -1 and 0.  Runs on torch's current stream.
    Returns (matches [n_pairs, capacity], nmatches [n_pairs]) as device tensors: row p is indexed by the current frame's feature and holds the key-frame
    feature whose point it received in this call (-1: none)."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    n_pairs, cap = int(pairs.shape[0]), ctx.orb_capacity
    if tuple(pairs.shape) != (n_pairs, 2) or (pair_Tcw is not None and pair_Tcw.numel() != 16 * n_pairs):
        raise ValueError("search_by_projection_kf_pairs: pairs [n_pairs, 2], pair_Tcw [n_pairs, 4, 4]")
    tb = _track_batch_c(kps, desc, counts, img_stride, None, cell_offsets, cell_index, Tcw, _cam5(camera), bounds, mp_world=mp_world, mp_valid=mp_valid,
                        mp_desc=mp_desc)
    if out is None:
        out = (_new((n_pairs, cap), -1), _new((n_pairs,)))
    m, n = out
    _call_dev("olf_search_by_projection_kf_pairs_dev", ctx, C.byref(tb), int(n_frames), _dev(mp_bad, torch.uint8, "mp_bad"),
              _dev(mp_maxd, torch.float32, "mp_maxd"), _dev(mp_mind, torch.float32, "mp_mind"), n_pairs, _dev(pairs, torch.int32, "pairs"),
              _dev(pair_Tcw, torch.float32, "pair_Tcw"), _dev(cur_valid, torch.uint8, "cur_valid"), _dev(already_found, torch.uint8, "already_found"),
              float(th), _dev(d_th, torch.float32, "d_th"), int(ORBdist), _dev(d_orb_dist, torch.int32, "d_orb_dist"), int(bool(checkOri)),
              _dev(m, torch.int32, "matches"), _dev(n, torch.int32, "nmatches"))
    return m, n


def search_by_projection_sim3_batch(n_frames, kps, desc, counts, cell_offsets, cell_index, local_map, Scw, frame_matched, camera, bounds, th=10.0, d_th=None,
                                    img_stride=2, out=None, context=None):
    """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:292-405; LoopClosing::ComputeSim3, src/LoopClosing.cc:381) for
    every key frame of a device-resident batch against its list of points: olf_search_by_projection_sim3_batch_dev (include/orbline.h describes every
    array; csrc/projection_batch.hip).  The frame arrays are those of fuse_search_batch (uright and Tcw are not read); local_map: a LocalMapDev (obs is
    not read and may be None) whose lists, if any, are the points each key frame is searched for; Scw float32 [n_frames, 4, 4]: the Sim3 poses;
    frame_matched int32 [n_frames, capacity]: vpMatched as map indices, written in place (in: -1 NULL, >= 0 the map index held, -2 a point outside
    the map; out: additionally the map index each key point received); d_th float32 [n_frames]: per-key-frame radii (<= 0 skips a key frame);
    camera = (fx, fy, cx, cy, mbf).  out = nmatches: an int32 tensor [n_frames] to write into; by default made here, zero.  Runs on torch's current stream.
    Returns (frame_matched, nmatches) as device tensors."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    tb = _track_batch_c(kps, desc, counts, img_stride, None, cell_offsets, cell_index, None, camera, bounds)
    lm = local_map.c(n_frames)
    n = _new((int(n_frames),)) if out is None else out
    _call_dev("olf_search_by_projection_sim3_batch_dev", ctx, C.byref(tb), int(n_frames), C.byref(lm), _dev(Scw, torch.float32, "Scw"),
              _dev(frame_matched, torch.int32, "frame_matched"), float(th), _dev(d_th, torch.float32, "d_th"), _dev(n, torch.int32, "nmatches"))
    return frame_matched, n


def is_in_frustum_l_batch(n_frames, Tcw, local_lines, camera, bounds, frame_ml=None, lcounts=None, img_stride=2, out=None, context=None):
    """Frame::isInFrustum_l (src/Frame.cc:446-515) for every (frame, local map line) of a device-resident batch, with the bad / already-held skips of
    Tracking::SearchLocalPointsAndLines (src/Tracking.cc:1953-1956): olf_is_in_frustum_l_batch_dev (include/orbline.h).  Tcw [n_frames, 4, 4];
    local_lines: a LocalLineMapDev; camera = (fx, fy, cx, cy[, mbf]); bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY); frame_ml int32 [n_frames, capacity]: the
    frames' mvpMapLines as map indices (negative: none), lcounts (extractor layout, with img_stride): their N_l.  Runs on torch's current stream.
    Returns (in_view uint8, proj4 float32 [.., 4]) over the entries; entries not in view keep what `out` held (zeros by default) in proj4."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    ne = local_lines.n_entries(n_frames)
    lb = _line_batch_c(None, None, lcounts, img_stride, None, Tcw, camera, bounds)
    lm = local_lines.c(n_frames)
    if out is None:
        out = (_new((ne,), 0, torch.uint8), _new((ne, 4), 0, torch.float32))
    v, p = out
    _call_dev("olf_is_in_frustum_l_batch_dev", ctx, C.byref(lb), int(n_frames), C.byref(lm), _dev(frame_ml, torch.int32, "frame_ml"),
              _dev(v, torch.uint8, "in_view"), _dev(p, torch.float32, "proj4"))
    return out


def search_local_lines_batch(n_frames, kls, ldesc, lcounts, ldisp, Tcw, local_lines, camera, bounds, nnr, frame_ml=None, img_stride=2, out=None, context=None):
    """The line half of Tracking::SearchLocalPointsAndLines (src/Tracking.cc:1897-1913, :1945-2023) for a device-resident batch: the frustum pass, the
    compaction into mvpLocalMapLines_InFrustum, match() against every frame's own lines, the loop :1976-2016 and n_inliers_ls --
    olf_search_local_lines_batch_dev (include/orbline.h describes every array; csrc/line_batch.hip).  kls / ldesc / lcounts in the extractor's layout,
    ldisp [n_frames, capacity, 2] (mvDisparity_l); nnr = Config::minRatio12L().  out = (in_view, proj4, m12, frame_ml_out, ninliers).  Runs on torch's
    current stream.  Returns (in_view [n_entries] uint8, proj4 [n_entries, 4], m12 [n_entries]: matches_12 at the end per entry, -1 not in view;
    frame_ml_out [n_frames, capacity]: mvpMapLines at the end as map indices; ninliers [n_frames])."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    ne = local_lines.n_entries(n_frames)
    lb = _line_batch_c(kls, ldesc, lcounts, img_stride, ldisp, Tcw, camera, bounds)
    lm = local_lines.c(n_frames)
    if out is None:
        out = (_new((ne,), 0, torch.uint8), _new((ne, 4), 0, torch.float32), _new((ne,), -1), _new((int(n_frames), ctx.line_capacity), -1),
               _new((int(n_frames),)))
    v, p, m, fo, n = out
    _call_dev("olf_search_local_lines_batch_dev", ctx, C.byref(lb), int(n_frames), C.byref(lm), _dev(frame_ml, torch.int32, "frame_ml"), float(nnr),
              _dev(v, torch.uint8, "in_view"), _dev(p, torch.float32, "proj4"), _dev(m, torch.int32, "m12"), _dev(fo, torch.int32, "frame_ml_out"),
              _dev(n, torch.int32, "ninliers"))
    return out


def track_lines_batch(n_frames, kls, ldesc, lcounts, ldisp, last_ml, bounds, nnr, best_lr=True, skip_null=True, gates=True, delta_angle=np.pi / 8.0, pos_frac=0.1,
                      enable=None, img_stride=2, out=None, context=None):
    """The f2f line tracking of Tracking::TrackWithMotionModelWithLine (src/Tracking.cc:1305-1349; the defaults) or TrackReferenceKeyFrameWithLine
    (:976-1020: skip_null=False, gates=False) for the n_frames - 1 consecutive pairs of a device-resident batch: olf_track_lines_batch_dev
    (include/orbline.h).  last_ml int32 [n_frames - 1, capacity]: mvpMapLines of every pair's last frame as ids (negative: NULL); enable int32
    [n_frames - 1] (0: the pair's rows of `out` keep what they hold).  out = (m12, cur_ml, ninliers).  Runs on torch's current stream.  Returns
    (m12 [n_frames - 1, capacity], cur_ml [n_frames - 1, capacity]: the ids the current frame's lines received, -1 none; ninliers [n_frames - 1])."""
    import ctypes as C
    import torch
    ctx = _ctx(context)
    n_pairs = max(int(n_frames) - 1, 0)
    lb = _line_batch_c(kls, ldesc, lcounts, img_stride, ldisp, None, (0.0, 0.0, 0.0, 0.0), bounds)
    if out is None:
        out = (_new((n_pairs, ctx.line_capacity), -1), _new((n_pairs, ctx.line_capacity), -1), _new((n_pairs,)))
    m, cm, n = out
    _call_dev("olf_track_lines_batch_dev", ctx, C.byref(lb), int(n_frames), _dev(last_ml, torch.int32, "last_ml"), float(nnr), int(bool(best_lr)),
              int(bool(skip_null)), int(bool(gates)), float(delta_angle), float(pos_frac), _dev(enable, torch.int32, "enable"), _dev(m, torch.int32, "m12"),
              _dev(cm, torch.int32, "cur_ml"), _dev(n, torch.int32, "ninliers"))
    return out
