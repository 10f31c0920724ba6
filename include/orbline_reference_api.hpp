// orbline_reference_api.hpp -- the reference's OWN call signatures on top of the C ABI, so that the call sites of Tracking.cc need no edit:
//
//   matcher.SearchByProjection(mCurrentFrame, mLastFrame, th, bMono, match12)        src/Tracking.cc:1296,1302   (include/ORBmatcher.h:53; the
//                                                                                    four-argument form :52 as well)
//   matcher.SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches)             src/Tracking.cc:970         (include/ORBmatcher.h:66)
//   matcher.SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th)                 src/Tracking.cc:1941        (include/ORBmatcher.h:48)
//   match(mLastFrame.mDescriptors_Line, mCurrentFrame.mDescriptors_Line, nnr, m12)   src/Tracking.cc:1308, :979  (include/LineMatcher.h:61)
//   match(mvpLocalMapLines, mCurrentFrame, nnr, m12) / matchNNR / distance           src/Tracking.cc:1970        (include/LineMatcher.h:57-63)
//   matchGrid(points1 | lines1, desc1, grid, desc2, [directions2,] w, matches_12)    src/Frame.cc:926            (include/LineMatcher.h:66-69)
//   GridStructure / GridWindow / getLineCoords                                       include/gridStructure.h:33-58
//   StereoFrameFeatures(frame, imLeft, imRight)  = the feature part of Frame::Frame  src/Frame.cc:164-171,199-207
//   FrameGrid(frame)                             = AssignFeaturesToGrid()            src/Frame.cc:215            (:334-349)
//   KeyFrameDatabaseOf<KeyFrame, Frame>          = KeyFrameDatabase                  include/KeyFrameDatabase.h:60-98 (add, erase, clear, the four Detect members)
//   MapGraphOf<KeyFrame, MapPoint, MapLine>, UpdateLocalMap(...)  = Tracking::UpdateLocalMap   src/Tracking.cc:2028-2205
//   KeyFrameCulling<KeyFrame, MapPoint, MapLine>(ctx, mpCurrentKeyFrame, mbMonocular)  = LocalMapping::KeyFrameCulling   src/LocalMapping.cc:632-696
//   and every other ORBmatcher call of the reference: SearchByProjection(cur, pKF, sFound, th, ORBdist) Tracking.cc:2322,2336;
//   SearchForTriangulation LocalMapping.cc:268; Fuse(pKF, vpMapPoints[, th]) LocalMapping.cc:489,514; SearchByBoW(pKF1, pKF2, vpMatches12)
//   LoopClosing.cc:271; SearchBySim3 LoopClosing.cc:329; SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) LoopClosing.cc:381;
//   Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) LoopClosing.cc:605; SearchForInitialization Tracking.cc:628
//
// Everything is a template over the reference's types (Frame, KeyFrame, MapPoint, MapLine, cv::Mat), used only through the public members
// the reference functions themselves read (include/Frame.h:137-260, include/KeyFrame.h, include/MapPoint.h): the header compiles without
// OpenCV -- tests/adaptor_reference_api.cpp instantiates every template with minimal stand-in structs -- and, inside the reference tree,
// binds to the real classes.  A function gathers the members into an olf_frame_view, makes one C-ABI call and scatters the assignments the
// reference function makes (mvpMapPoints[...] = pMP, NULL on a rotation-histogram rejection).
//
// Contexts: the matcher functions run on a small per-thread context (olf_detail::thread_ctx()) -- ORBmatcher objects are stack locals used
// from the Tracking, LocalMapping and LoopClosing threads concurrently (SURVEY 8(b) "Threading"), and a context serves one thread.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <list>
#include <map>
#include <set>
#include <unordered_set>
#include <limits>
#include <mutex>
#include <type_traits>
#include "orbline_adaptor.hpp"

namespace ORB_SLAM2 {

// (AdaptorConfig / ORBLINE_CONFIG -- the Config singleton's accessors read here -- are defined in orbline_adaptor.hpp)

namespace olf_detail {

// one small context per host thread for the matcher calls (their kernels do not depend on the image size; 320 x 240 is about the smallest
// image whose eight pyramid levels all hold a FAST cell)
inline olf_ctx* thread_ctx()
{
    struct Holder { olf_ctx* h = nullptr; ~Holder() { if (h) olf_ctx_destroy(h); } };
    static thread_local Holder t;
    if (!t.h) {
        olf_params p;
        olf_default_params(&p);
        check(olf_ctx_create(&p, 320, 240, 1, &t.h), "olf_ctx_create (matcher context)");
    }
    return t.h;
}

// rows of a continuous N x 32 CV_8U matrix (cv::Mat or anything with rows / cols / data / isContinuous / clone)
template <class MatT> struct DescRows {
    MatT keep;
    const uint8_t* p;
    int n;
    explicit DescRows(const MatT& m) : keep(m.isContinuous() ? m : m.clone()), p(keep.data), n(keep.rows) {}
};

template <class KeyPointVec> const olf_keypoint* keypoints(const KeyPointVec& v)
{
    static_assert(sizeof(typename KeyPointVec::value_type) == sizeof(olf_keypoint), "cv::KeyPoint layout");
    return reinterpret_cast<const olf_keypoint*>(v.data());
}

// DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned int>>) -> CSR
struct FeatVecCSR {
    std::vector<int32_t> nodes, offs, feats;
    template <class FV> explicit FeatVecCSR(const FV& fv)
    {
        offs.push_back(0);
        for (typename FV::const_iterator it = fv.begin(); it != fv.end(); ++it) {
            nodes.push_back((int32_t)it->first);
            for (size_t k = 0; k < it->second.size(); ++k) feats.push_back((int32_t)it->second[k]);
            offs.push_back((int32_t)feats.size());
        }
    }
    void attach(olf_frame_view& v) const { v.fv_nodes = nodes.data(); v.fv_offsets = offs.data(); v.fv_features = feats.data(); v.fv_n = (int32_t)nodes.size(); }
};

// The members of a reference Frame read by the per-frame searches, gathered once (the arrays live as long as the object)
template <class FrameT> struct FrameGather {
    olf_frame_view v;
    std::vector<uint8_t> valid, obs, bad, outlier, mpdesc;
    std::vector<float> world;
    float Tcw[16];
    DescRows<decltype(FrameT::mDescriptors)> desc;
    // with_points: also gather GetWorldPos() / GetDescriptor() of the frame's map points (what SearchByProjection(cur, last) reads of `last`)
    FrameGather(const FrameT& F, bool with_points) : desc(F.mDescriptors)
    {
        v = olf_frame_view();
        const int n = F.N;
        v.keys = keypoints(F.mvKeysUn); v.desc = desc.p; v.uright = F.mvuRight.empty() ? nullptr : F.mvuRight.data(); v.n = n;
        valid.assign(n, 0); obs.assign(n, 0); bad.assign(n, 0); outlier.assign(n, 0);
        if (with_points) { world.assign((size_t)3 * n, 0.f); mpdesc.assign((size_t)32 * n, 0); }
        for (int i = 0; i < n; ++i) {
            auto* pMP = F.mvpMapPoints[i];
            outlier[i] = i < (int)F.mvbOutlier.size() && F.mvbOutlier[i] ? 1 : 0;
            if (!pMP) continue;
            valid[i] = 1; obs[i] = pMP->Observations() > 0 ? 1 : 0; bad[i] = pMP->isBad() ? 1 : 0;
            if (with_points) {
                const auto wp = pMP->GetWorldPos();
                for (int k = 0; k < 3; ++k) world[3 * i + k] = wp.template at<float>(k);
                const auto d = pMP->GetDescriptor();
                std::memcpy(&mpdesc[(size_t)32 * i], d.data, 32);
            }
        }
        v.mp_valid = valid.data(); v.mp_obs = obs.data(); v.mp_bad = bad.data(); v.outlier = outlier.data();
        if (with_points) { v.mp_world = world.data(); v.mp_desc = mpdesc.data(); }
        if (!F.mTcw.empty()) { for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tcw[4 * r + c] = F.mTcw.template at<float>(r, c); v.Tcw = Tcw; }
        v.fx = F.fx; v.fy = F.fy; v.cx = F.cx; v.cy = F.cy; v.mbf = F.mbf;
        v.minX = F.mnMinX; v.maxX = F.mnMaxX; v.minY = F.mnMinY; v.maxY = F.mnMaxY;
        v.scale_factors = F.mvScaleFactors.data(); v.n_levels = F.mnScaleLevels;
    }
};

}  // namespace olf_detail

// ---- ORBmatcher: the member templates declared in orbline_adaptor.hpp -------------------------------------------------------------------------------------
// static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b), include/ORBmatcher.h:44
template <class MatT, class> int ORBmatcher::DescriptorDistance(const MatT& a, const MatT& b)
{
    return distance(static_cast<const uint8_t*>(a.data), static_cast<const uint8_t*>(b.data));
}

// int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono), src/ORBmatcher.cc:1330-1472
template <class FrameT> int ORBmatcher::SearchByProjection(FrameT& CurrentFrame, const FrameT& LastFrame, const float th, const bool bMono)
{
    {
        olf_detail::FrameGather<FrameT> cur(CurrentFrame, false), last(LastFrame, true);
        const std::vector<uint8_t> before = cur.valid;
        std::vector<int32_t> m;
        const int n = SearchByProjection(olf_detail::thread_ctx(), cur.v, last.v, th, bMono, m);
        for (int i2 = 0; i2 < CurrentFrame.N; ++i2) {
            if (m[i2] >= 0) CurrentFrame.mvpMapPoints[i2] = LastFrame.mvpMapPoints[m[i2]];
            else if (before[i2] && !cur.valid[i2]) CurrentFrame.mvpMapPoints[i2] = nullptr;      // assigned, then dropped by the rotation histogram (:1459)
        }
        return n;
    }
}

// int SearchByProjection(Frame &F, const std::vector<MapPoint*> &vpMapPoints, const float th = 3), src/ORBmatcher.cc:47-131
template <class FrameT, class MapPointT> int ORBmatcher::SearchByProjection(FrameT& F, const std::vector<MapPointT*>& vpMapPoints, const float th)
{
    {
        olf_detail::FrameGather<FrameT> f(F, false);
        const int n_mp = (int)vpMapPoints.size();
        std::vector<uint8_t> inView(n_mp, 0), bad(n_mp, 0), observed(n_mp, 0), desc((size_t)32 * n_mp, 0);
        std::vector<int32_t> level(n_mp, 0);
        std::vector<float> viewCos(n_mp, 0.f), proj((size_t)3 * n_mp, 0.f);
        for (int i = 0; i < n_mp; ++i) {
            MapPointT* pMP = vpMapPoints[i];
            if (!pMP) { bad[i] = 1; continue; }            // (the reference dereferences every entry; a null entry can only be skipped)
            inView[i] = pMP->mbTrackInView ? 1 : 0; bad[i] = pMP->isBad() ? 1 : 0; level[i] = pMP->mnTrackScaleLevel; viewCos[i] = pMP->mTrackViewCos;
            proj[3 * i] = pMP->mTrackProjX; proj[3 * i + 1] = pMP->mTrackProjY; proj[3 * i + 2] = pMP->mTrackProjXR;
            observed[i] = pMP->Observations() > 0 ? 1 : 0;
            const auto d = pMP->GetDescriptor();
            std::memcpy(&desc[(size_t)32 * i], d.data, 32);
        }
        TrackedMapPoints t;
        t.n = n_mp; t.mbTrackInView = inView.data(); t.isBad = bad.data(); t.mnTrackScaleLevel = level.data(); t.mTrackViewCos = viewCos.data();
        t.mTrackProjXYR = proj.data(); t.descriptor = desc.data(); t.observed = observed.data();
        std::vector<int32_t> m;
        const int n = SearchByProjection(olf_detail::thread_ctx(), f.v, t, th, m);
        for (int idx = 0; idx < F.N; ++idx) if (m[idx] >= 0) F.mvpMapPoints[idx] = vpMapPoints[m[idx]];
        return n;
    }
}

// int SearchForInitialization(Frame &F1, Frame &F2, std::vector<cv::Point2f> &vbPrevMatched, std::vector<int> &vnMatches12, int windowSize = 10),
// src/ORBmatcher.cc:407-522 (Tracking::MonocularInitialization, src/Tracking.cc:628)
template <class FrameT, class Point2fT> int ORBmatcher::SearchForInitialization(FrameT& F1, FrameT& F2, std::vector<Point2fT>& vbPrevMatched,
                                                                                  std::vector<int>& vnMatches12, int windowSize)
{
    static_assert(sizeof(Point2fT) == 2 * sizeof(float), "cv::Point2f is two floats");
    olf_detail::FrameGather<FrameT> f1(F1, false), f2(F2, false);
    if ((int)vbPrevMatched.size() < F1.N) throw std::runtime_error("SearchForInitialization: vbPrevMatched shorter than F1.mvKeysUn");
    return SearchForInitialization(olf_detail::thread_ctx(), f1.v, f2.v, reinterpret_cast<float*>(vbPrevMatched.data()), vnMatches12, windowSize);
}

// int SearchByBoW(KeyFrame* pKF, Frame &F, std::vector<MapPoint*> &vpMapPointMatches), src/ORBmatcher.cc:161-290
template <class KeyFrameT, class FrameT, class MapPointT> int ORBmatcher::SearchByBoW(KeyFrameT* pKF, FrameT& F, std::vector<MapPointT*>& vpMapPointMatches)
{
    {
        const std::vector<MapPointT*> vpMapPointsKF = pKF->GetMapPointMatches();
        vpMapPointMatches = std::vector<MapPointT*>(F.N, static_cast<MapPointT*>(nullptr));
        olf_frame_view kf = olf_frame_view(), f = olf_frame_view();
        olf_detail::DescRows<decltype(KeyFrameT::mDescriptors)> dk(pKF->mDescriptors);
        olf_detail::DescRows<decltype(FrameT::mDescriptors)> df(F.mDescriptors);
        const int nk = (int)vpMapPointsKF.size();
        std::vector<uint8_t> valid(nk, 0), bad(nk, 0), fvalid(F.N, 0), fobs(F.N, 0);
        for (int i = 0; i < nk; ++i) if (vpMapPointsKF[i]) { valid[i] = 1; bad[i] = vpMapPointsKF[i]->isBad() ? 1 : 0; }
        kf.keys = olf_detail::keypoints(pKF->mvKeysUn); kf.desc = dk.p; kf.n = nk; kf.mp_valid = valid.data(); kf.mp_bad = bad.data();
        f.keys = olf_detail::keypoints(F.mvKeysUn); f.desc = df.p; f.n = F.N; f.mp_valid = fvalid.data(); f.mp_obs = fobs.data();
        const olf_detail::FeatVecCSR ck(pKF->mFeatVec), cf(F.mFeatVec);
        ck.attach(kf); cf.attach(f);
        std::vector<int32_t> m;
        const int n = SearchByBoW(olf_detail::thread_ctx(), kf, f, m);
        for (int iF = 0; iF < F.N; ++iF) if (m[iF] >= 0) vpMapPointMatches[iF] = vpMapPointsKF[m[iF]];
        return n;
    }
}

// ---- the rest of the ORBmatcher surface (include/ORBmatcher.h:37-103): the searches of the relocaliser, LocalMapping and LoopClosing ----------
namespace olf_detail {

// MapPoint::mfMaxDistance / mfMinDistance are protected in the reference (include/MapPoint.h:145-146); the searches need the raw values
// (PredictScale divides mfMaxDistance by the distance, src/MapPoint.cc:397-412).  Inside the reference tree either declare
//     friend struct ORB_SLAM2::olf_detail::MapPointDistances;
// in class MapPoint (one line) -- then the members are read directly -- or nothing: the fall-back inverts the public
// GetMaxDistanceInvariance() = 1.2f * mfMaxDistance / GetMinDistanceInvariance() = 0.8f * mfMinDistance by searching the floats around the
// quotient for one whose product reproduces the returned value (exact except where two neighbouring floats share a product).
struct MapPointDistances {
    template <class MP> static auto maxd(MP* p, int) -> decltype((float)p->mfMaxDistance) { return p->mfMaxDistance; }
    template <class MP> static float maxd(MP* p, long) { return invert(p->GetMaxDistanceInvariance(), 1.2f); }
    template <class MP> static auto mind(MP* p, int) -> decltype((float)p->mfMinDistance) { return p->mfMinDistance; }
    template <class MP> static float mind(MP* p, long) { return invert(p->GetMinDistanceInvariance(), 0.8f); }
    static float invert(float y, float k)
    {
        float x = y / k;
        for (int pass = 0; pass < 2; ++pass) {
            float c = x;
            for (int s = 0; s < 3 && !(k * c == y); ++s) c = std::nextafter(c, pass ? 3.4e38f : -3.4e38f);
            if (k * c == y) return c;
        }
        return x;
    }
};

template <class MatT> void mat4(const MatT& m, float* out16) { for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) out16[4 * r + c] = m.template at<float>(r, c); }

// The members of a reference KeyFrame read by the key-frame searches (include/KeyFrame.h:57-62,92-116,185-231)
template <class KeyFrameT> struct KeyFrameGather {
    typedef typename std::remove_pointer<typename decltype(std::declval<KeyFrameT&>().GetMapPointMatches())::value_type>::type MapPointT;
    olf_frame_view v;
    std::vector<MapPointT*> mps;
    std::vector<uint8_t> valid, obs, bad, mpdesc;
    std::vector<float> world, maxd, mind;
    float Tcw[16];
    DescRows<decltype(KeyFrameT::mDescriptors)> desc;
    FeatVecCSR fv;
    KeyFrameGather(KeyFrameT* pKF, bool with_points) : mps(pKF->GetMapPointMatches()), desc(pKF->mDescriptors), fv(pKF->mFeatVec)
    {
        v = olf_frame_view();
        const int n = (int)mps.size();
        v.keys = keypoints(pKF->mvKeysUn); v.desc = desc.p; v.uright = pKF->mvuRight.empty() ? nullptr : pKF->mvuRight.data(); v.n = n;
        valid.assign(n, 0); obs.assign(n, 0); bad.assign(n, 0);
        if (with_points) { world.assign((size_t)3 * n, 0.f); mpdesc.assign((size_t)32 * n, 0); maxd.assign(n, 0.f); mind.assign(n, 0.f); }
        for (int i = 0; i < n; ++i) {
            MapPointT* pMP = mps[i];
            if (!pMP) continue;
            valid[i] = 1; obs[i] = pMP->Observations() > 0 ? 1 : 0; bad[i] = pMP->isBad() ? 1 : 0;
            if (with_points) {
                const auto wp = pMP->GetWorldPos();
                for (int k = 0; k < 3; ++k) world[3 * i + k] = wp.template at<float>(k);
                const auto d = pMP->GetDescriptor();
                std::memcpy(&mpdesc[(size_t)32 * i], d.data, 32);
                maxd[i] = MapPointDistances::maxd(pMP, 0); mind[i] = MapPointDistances::mind(pMP, 0);
            }
        }
        v.mp_valid = valid.data(); v.mp_obs = obs.data(); v.mp_bad = bad.data();
        if (with_points) { v.mp_world = world.data(); v.mp_desc = mpdesc.data(); v.mp_maxd = maxd.data(); v.mp_mind = mind.data(); }
        mat4(pKF->GetPose(), Tcw); v.Tcw = Tcw;
        v.fx = pKF->fx; v.fy = pKF->fy; v.cx = pKF->cx; v.cy = pKF->cy; v.mbf = pKF->mbf;
        v.minX = (float)pKF->mnMinX; v.maxX = (float)pKF->mnMaxX; v.minY = (float)pKF->mnMinY; v.maxY = (float)pKF->mnMaxY;
        v.scale_factors = pKF->mvScaleFactors.data(); v.n_levels = pKF->mnScaleLevels;
        fv.attach(v);
    }
};

// the members of a list of reference MapPoints read by the two Fuse searches and SearchByProjection(pKF, Scw, ...)
template <class MapPointT> struct PointGather {
    std::vector<uint8_t> skip, desc;
    std::vector<float> world, normal, maxd, mind;
    ORBmatcher::FuseMapPoints m;
    template <class SkipFn> PointGather(const std::vector<MapPointT*>& pts, SkipFn skip_if)
    {
        const size_t n = pts.size();
        skip.assign(n, 1); desc.assign(32 * n, 0); world.assign(3 * n, 0.f); normal.assign(3 * n, 0.f); maxd.assign(n, 0.f); mind.assign(n, 0.f);
        for (size_t i = 0; i < n; ++i) {
            MapPointT* p = pts[i];
            if (!p || skip_if(p)) continue;
            skip[i] = 0;
            const auto w = p->GetWorldPos(); const auto nv = p->GetNormal(); const auto d = p->GetDescriptor();
            for (int k = 0; k < 3; ++k) { world[3 * i + k] = w.template at<float>(k); normal[3 * i + k] = nv.template at<float>(k); }
            std::memcpy(&desc[32 * i], d.data, 32);
            maxd[i] = MapPointDistances::maxd(p, 0); mind[i] = MapPointDistances::mind(p, 0);
        }
        m.n = (int)n; m.skip = skip.data(); m.world = world.data(); m.normal = normal.data(); m.mfMaxDistance = maxd.data(); m.mfMinDistance = mind.data();
        m.descriptor = desc.data();
    }
};
}  // namespace olf_detail

// int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono, map<int,int>& match12),
// src/ORBmatcher.cc:1474-1618 (Tracking::TrackWithMotionModelWithLine, src/Tracking.cc:1296,1302)
template <class FrameT> int ORBmatcher::SearchByProjection(FrameT& CurrentFrame, const FrameT& LastFrame, const float th, const bool bMono, std::map<int, int>& match12)
{
    olf_detail::FrameGather<FrameT> cur(CurrentFrame, false), last(LastFrame, true);
    const std::vector<uint8_t> before = cur.valid;
    std::vector<int32_t> m(CurrentFrame.N, -1), first(CurrentFrame.N, -1);
    int32_t n = 0;
    olf_detail::check(olf_search_by_projection_match12(olf_detail::thread_ctx(), &cur.v, &last.v, th, bMono ? 1 : 0, mbCheckOrientation ? 1 : 0, m.data(),
                                                       first.data(), &n), "olf_search_by_projection_match12");
    match12.clear();
    for (int i2 = 0; i2 < CurrentFrame.N; ++i2) {
        if (m[i2] >= 0) CurrentFrame.mvpMapPoints[i2] = LastFrame.mvpMapPoints[m[i2]];              // the LAST point assigned (:1575)
        else if (before[i2] && !cur.valid[i2]) CurrentFrame.mvpMapPoints[i2] = nullptr;             // dropped by the rotation histogram (:1610)
        if (first[i2] >= 0) match12.insert(match12.end(), std::pair<int, int>(i2, first[i2]));      // the FIRST one inserted (:1577)
    }
    return n;
}

// int SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th, const int ORBdist),
// src/ORBmatcher.cc:1620-1747 (Tracking::Relocalization, src/Tracking.cc:2322,2336)
template <class FrameT, class KeyFrameT, class MapPointT>
int ORBmatcher::SearchByProjection(FrameT& CurrentFrame, KeyFrameT* pKF, const std::set<MapPointT*>& sAlreadyFound, const float th, const int ORBdist)
{
    olf_detail::FrameGather<FrameT> cur(CurrentFrame, false);
    olf_detail::KeyFrameGather<KeyFrameT> kf(pKF, true);
    const std::vector<uint8_t> before = cur.valid;
    std::vector<uint8_t> found(kf.mps.size(), 0);
    for (size_t i = 0; i < kf.mps.size(); ++i) found[i] = kf.mps[i] && sAlreadyFound.count(kf.mps[i]) ? 1 : 0;
    std::vector<int32_t> m;
    const int n = SearchByProjection(olf_detail::thread_ctx(), cur.v, kf.v, found.data(), th, ORBdist, m);
    for (int i2 = 0; i2 < CurrentFrame.N; ++i2) {
        if (m[i2] >= 0) CurrentFrame.mvpMapPoints[i2] = kf.mps[m[i2]];
        else if (before[i2] && !cur.valid[i2]) CurrentFrame.mvpMapPoints[i2] = nullptr;
    }
    return n;
}

// int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th),
// src/ORBmatcher.cc:292-405 (LoopClosing::ComputeSim3, src/LoopClosing.cc:381)
template <class KeyFrameT, class MatT, class MapPointT>
int ORBmatcher::SearchByProjection(KeyFrameT* pKF, MatT Scw, const std::vector<MapPointT*>& vpPoints, std::vector<MapPointT*>& vpMatched, int th)
{
    olf_detail::KeyFrameGather<KeyFrameT> kf(pKF, false);
    std::set<MapPointT*> spAlreadyFound(vpMatched.begin(), vpMatched.end());
    spAlreadyFound.erase(static_cast<MapPointT*>(nullptr));
    const olf_detail::PointGather<MapPointT> pts(vpPoints, [&](MapPointT* p) { return p->isBad() || spAlreadyFound.count(p) != 0; });
    float S[16];
    olf_detail::mat4(Scw, S);
    std::vector<uint8_t> matched(vpMatched.size(), 0);
    for (size_t i = 0; i < vpMatched.size(); ++i) matched[i] = vpMatched[i] ? 1 : 0;
    if ((int)matched.size() != kf.v.n) throw std::runtime_error("SearchByProjection(pKF, Scw, ...): vpMatched must have one entry per key point of pKF");
    std::vector<int32_t> m(kf.v.n, -1);
    int32_t n = 0;
    olf_detail::check(olf_search_by_projection_sim3(olf_detail::thread_ctx(), &kf.v, S, pts.m.n, pts.m.skip, pts.m.world, pts.m.normal, pts.m.mfMaxDistance,
                                                    pts.m.mfMinDistance, pts.m.descriptor, (float)th, matched.data(), m.data(), &n),
                      "olf_search_by_projection_sim3");
    for (int idx = 0; idx < kf.v.n; ++idx) if (m[idx] >= 0) vpMatched[idx] = vpPoints[m[idx]];
    return n;
}

// int SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12), src/ORBmatcher.cc:524-657 (LoopClosing.cc:271)
template <class KeyFrameT, class MapPointT> int ORBmatcher::SearchByBoW(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12)
{
    olf_detail::KeyFrameGather<KeyFrameT> k1(pKF1, false), k2(pKF2, false);
    std::vector<int32_t> m;
    const int n = SearchByBoW(olf_detail::thread_ctx(), KeyFramePair(), k1.v, k2.v, m);
    vpMatches12 = std::vector<MapPointT*>(k1.mps.size(), static_cast<MapPointT*>(nullptr));
    for (size_t i = 0; i < k1.mps.size(); ++i) if (m[i] >= 0) vpMatches12[i] = k2.mps[m[i]];
    return n;
}

// int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t, size_t>> &vMatchedPairs, const bool bOnlyStereo),
// src/ORBmatcher.cc:659-825 (LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:268)
template <class KeyFrameT, class MatT>
int ORBmatcher::SearchForTriangulation(KeyFrameT* pKF1, KeyFrameT* pKF2, MatT F12, std::vector<std::pair<size_t, size_t>>& vMatchedPairs, const bool bOnlyStereo)
{
    olf_detail::KeyFrameGather<KeyFrameT> k1(pKF1, false), k2(pKF2, false);
    float F[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) F[3 * r + c] = F12.template at<float>(r, c);
    const auto Cw = pKF1->GetCameraCenter();
    const float cw[3] = {Cw.template at<float>(0), Cw.template at<float>(1), Cw.template at<float>(2)};
    std::vector<int32_t> m12(k1.v.n, -1);
    int32_t n = 0;
    olf_detail::check(olf_search_for_triangulation(olf_detail::thread_ctx(), &k1.v, &k2.v, F, cw, bOnlyStereo ? 1 : 0, mbCheckOrientation ? 1 : 0, m12.data(), &n),
                      "olf_search_for_triangulation");
    vMatchedPairs.clear();
    vMatchedPairs.reserve(n > 0 ? n : 0);
    for (int i = 0; i < k1.v.n; ++i) if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
    return n;
}

// int Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th = 3.0), src/ORBmatcher.cc:827-975 (LocalMapping.cc:489,514).
// The search of every point runs first (one call); what the reference does with a hit (:950-972: Replace / AddObservation / AddMapPoint) is
// replayed on the reference's own objects in list order.  A hit's (bestIdx, bestDist) depends on nothing that loop changes; whether a point
// is looked at does (isBad() / IsInKeyFrame(pKF) after an earlier Replace or AddObservation), so that gate is evaluated again at its turn.
template <class KeyFrameT, class MapPointT> int ORBmatcher::Fuse(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, const float th)
{
    olf_detail::KeyFrameGather<KeyFrameT> kf(pKF, false);
    const olf_detail::PointGather<MapPointT> pts(vpMapPoints, [&](MapPointT* p) { return p->isBad() || p->IsInKeyFrame(pKF); });
    const auto Ow = pKF->GetCameraCenter();
    const float ow[3] = {Ow.template at<float>(0), Ow.template at<float>(1), Ow.template at<float>(2)};
    std::vector<int32_t> bestIdx(pts.m.n, -1), bestDist(pts.m.n, 256);
    olf_detail::check(olf_fuse_search(olf_detail::thread_ctx(), &kf.v, pts.m.n, pts.m.skip, pts.m.world, pts.m.normal, pts.m.mfMaxDistance, pts.m.mfMinDistance,
                                      pts.m.descriptor, th, ow, bestIdx.data(), bestDist.data()), "olf_fuse_search");
    int nFused = 0;
    for (size_t i = 0; i < vpMapPoints.size(); ++i) {
        MapPointT* pMP = vpMapPoints[i];
        if (!pMP || pts.skip[i] || bestDist[i] > TH_LOW) continue;
        if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        MapPointT* pMPinKF = pKF->GetMapPoint(bestIdx[i]);
        if (pMPinKF) {
            if (!pMPinKF->isBad()) {
                if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                else pMPinKF->Replace(pMP);
            }
        } else {
            pMP->AddObservation(pKF, bestIdx[i]);
            pKF->AddMapPoint(pMP, bestIdx[i]);
        }
        nFused++;
    }
    return nFused;
}

// int Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th, vector<MapPoint*> &vpReplacePoint),
// src/ORBmatcher.cc:977-1102 (LoopClosing::SearchAndFuse, src/LoopClosing.cc:605)
template <class KeyFrameT, class MatT, class MapPointT>
int ORBmatcher::Fuse(KeyFrameT* pKF, MatT Scw, const std::vector<MapPointT*>& vpPoints, float th, std::vector<MapPointT*>& vpReplacePoint)
{
    olf_detail::KeyFrameGather<KeyFrameT> kf(pKF, false);
    const std::set<MapPointT*> spAlreadyFound = pKF->GetMapPoints();
    const olf_detail::PointGather<MapPointT> pts(vpPoints, [&](MapPointT* p) { return p->isBad() || spAlreadyFound.count(p) != 0; });
    float S[16];
    olf_detail::mat4(Scw, S);
    std::vector<int32_t> bestIdx, bestDist;
    FuseSearch(olf_detail::thread_ctx(), kf.v, S, pts.m, th, bestIdx, bestDist);
    int nFused = 0;
    for (size_t iMP = 0; iMP < vpPoints.size(); ++iMP) {
        MapPointT* pMP = vpPoints[iMP];
        if (!pMP || pts.skip[iMP] || bestDist[iMP] > TH_LOW) continue;
        MapPointT* pMPinKF = pKF->GetMapPoint(bestIdx[iMP]);
        if (pMPinKF) { if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF; }
        else { pMP->AddObservation(pKF, bestIdx[iMP]); pKF->AddMapPoint(pMP, bestIdx[iMP]); }
        nFused++;
    }
    return nFused;
}

// int SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12, const cv::Mat &t12,
// const float th), src/ORBmatcher.cc:1104-1328 (LoopClosing::ComputeSim3, src/LoopClosing.cc:329)
template <class KeyFrameT, class MatT, class MapPointT>
int ORBmatcher::SearchBySim3(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches12, const float& s12, const MatT& R12, const MatT& t12, const float th)
{
    olf_detail::KeyFrameGather<KeyFrameT> k1(pKF1, true), k2(pKF2, true);
    const int N1 = k1.v.n;
    std::vector<int32_t> m12(N1, -1);
    for (int i = 0; i < N1 && i < (int)vpMatches12.size(); ++i) {
        MapPointT* pMP = vpMatches12[i];
        if (!pMP) continue;
        const int idx2 = pMP->GetIndexInKeyFrame(pKF2);          // (:1139-1151)
        m12[i] = idx2 >= 0 ? idx2 : -2;
    }
    float R[9], t[3];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R[3 * r + c] = R12.template at<float>(r, c); t[r] = t12.template at<float>(r); }
    const std::vector<int32_t> before = m12;
    const int n = SearchBySim3(olf_detail::thread_ctx(), k1.v, k2.v, m12, s12, R, t, th);
    for (int i1 = 0; i1 < N1; ++i1) if (m12[i1] >= 0 && m12[i1] != before[i1]) vpMatches12[i1] = k2.mps[m12[i1]];      // (:1319)
    return n;
}

// ---- LineMatcher free functions (include/LineMatcher.h:57-69) --------------------------------------------------------------------------
// int distance(const cv::Mat &a, const cv::Mat &b)
template <class MatT, class = typename std::enable_if<std::is_class<MatT>::value>::type> int distance(const MatT& a, const MatT& b) { return distance(static_cast<const uint8_t*>(a.data), static_cast<const uint8_t*>(b.data)); }

// int matchNNR(const cv::Mat &desc1, const cv::Mat &desc2, float nnr, std::vector<int> &matches_12), src/LineMatcher.cpp:42-62
template <class MatT> int matchNNR(const MatT& desc1, const MatT& desc2, float nnr, std::vector<int>& matches_12)
{
    const olf_detail::DescRows<MatT> a(desc1), b(desc2);
    return matchNNR(olf_detail::thread_ctx(), a.p, a.n, b.p, b.n, nnr, matches_12);
}
// int match(const cv::Mat &desc1, const cv::Mat &desc2, float nnr, std::vector<int> &matches_12), src/LineMatcher.cpp:104-132
template <class MatT> int match(const MatT& desc1, const MatT& desc2, float nnr, std::vector<int>& matches_12)
{
    const olf_detail::DescRows<MatT> a(desc1), b(desc2);
    return match(olf_detail::thread_ctx(), a.p, a.n, b.p, b.n, nnr, ORBLINE_CONFIG::bestLRMatches(), matches_12);
}
// int match(const std::vector<MapLine*> &mvpLocalMapLines, Frame &CurrentFrame, float nnr, std::vector<int> &matches_12), src/LineMatcher.cpp:64-73
// (everything after the reference's early `return matchNNR(...)` is dead code)
template <class MapLineT, class FrameT> int match(const std::vector<MapLineT*>& vpLocalMapLines, FrameT& CurrentFrame, float nnr, std::vector<int>& matches_12)
{
    std::vector<uint8_t> d1((size_t)32 * vpLocalMapLines.size());
    for (size_t i = 0; i < vpLocalMapLines.size(); ++i) { const auto d = vpLocalMapLines[i]->GetDescriptor(); std::memcpy(&d1[32 * i], d.data, 32); }
    const olf_detail::DescRows<decltype(FrameT::mDescriptors_Line)> b(CurrentFrame.mDescriptors_Line);
    return matchNNR(olf_detail::thread_ctx(), d1.data(), (int)vpLocalMapLines.size(), b.p, b.n, nnr, matches_12);
}

// ---- include/gridStructure.h:33-58 + src/LineIterator.cpp: the bucket grid of the stereo line matcher, host side ------------------------
// (Frame::ComputeStereoMatches_Lines itself runs on the GPU through olf_stereo_lines / StereoFrameFeatures; these are for callers that
// use the grid matcher directly, with candidate sets that are far too small for a kernel launch.)
typedef std::pair<int, int> point_2d;
typedef std::pair<point_2d, point_2d> line_2d;
struct GridWindow { std::pair<int, int> width, height; };

class GridStructure {
public:
    int rows, cols;
    GridStructure(int rows_, int cols_) : rows(rows_), cols(cols_)
    {
        if (rows <= 0 || cols <= 0) throw std::runtime_error("[GridStructure] invalid dimension");
        grid.assign((size_t)cols * rows, std::list<int>());
    }
    std::list<int>& at(int x, int y) { return (x >= 0 && x < cols && y >= 0 && y < rows) ? grid[(size_t)x * rows + y] : out_of_bounds; }
    void get(int x, int y, const GridWindow& w, std::unordered_set<int>& indices) const
    {
        const int x0 = std::max(0, x - w.width.first), x1 = std::min(cols, x + w.width.second + 1);
        const int y0 = std::max(0, y - w.height.first), y1 = std::min(rows, y + w.height.second + 1);
        for (int cx = x0; cx < x1; ++cx)
            for (int cy = y0; cy < y1; ++cy) { const std::list<int>& c = grid[(size_t)cx * rows + cy]; indices.insert(c.begin(), c.end()); }
    }
    void clear() { for (size_t i = 0; i < grid.size(); ++i) grid[i].clear(); }
private:
    std::vector<std::list<int>> grid;
    std::list<int> out_of_bounds;
};

// void getLineCoords(double x1, double y1, double x2, double y2, std::list<std::pair<int, int>> &line_coords): the cells of the reference's
// double-precision Bresenham walk (src/LineIterator.cpp:34-77), through the library's implementation of it
inline void getLineCoords(double x1, double y1, double x2, double y2, std::list<std::pair<int, int>>& line_coords)
{
    line_coords.clear();
    int32_t n = 0;
    std::vector<int32_t> xy(2 * 4096);
    olf_detail::check(olf_line_coords(x1, y1, x2, y2, xy.data(), 4096, &n), "olf_line_coords");
    for (int i = 0; i < n; ++i) line_coords.push_back(std::make_pair((int)xy[2 * i], (int)xy[2 * i + 1]));
}

namespace olf_detail {
// the candidate loop both matchGrid overloads share (src/LineMatcher.cpp:152-299); keep(i2) is the per-candidate gate of the line overload
template <class MatT, class CandFn, class KeepFn>
int match_grid_core(size_t n1, const MatT& desc1, const MatT& desc2, double ratio, CandFn candidates_of, KeepFn keep, std::vector<int>& matches_12)
{
    const DescRows<MatT> d1(desc1), d2(desc2);
    const bool lr = ORBLINE_CONFIG::bestLRMatches();
    int matches = 0;
    matches_12.resize(d1.n, -1);
    std::vector<int> matches_21, distances;
    if (lr) { matches_21.resize(d2.n, -1); distances.resize(d2.n, std::numeric_limits<int>::max()); }
    for (int i1 = 0; i1 < (int)n1; ++i1) {
        int best_d = std::numeric_limits<int>::max(), best_d2 = std::numeric_limits<int>::max(), best_idx = -1;
        std::unordered_set<int> cand;
        candidates_of(i1, cand);
        for (std::unordered_set<int>::const_iterator it = cand.begin(); it != cand.end(); ++it) {
            const int i2 = *it;
            if (i2 < 0 || i2 >= d2.n || !keep(i1, i2)) continue;
            const int d = distance(d1.p + (size_t)32 * i1, d2.p + (size_t)32 * i2);
            if (lr) { if (d < distances[i2]) { distances[i2] = d; matches_21[i2] = i1; } else continue; }
            if (d < best_d) { best_d2 = best_d; best_d = d; best_idx = i2; }
            else if (d < best_d2) best_d2 = d;
        }
        if (best_d < best_d2 * ratio) { matches_12[i1] = best_idx; ++matches; }
    }
    if (lr)
        for (size_t i1 = 0; i1 < matches_12.size(); ++i1) { int& i2 = matches_12[i1]; if (i2 >= 0 && matches_21[i2] != (int)i1) { i2 = -1; --matches; } }
    return matches;
}
}  // namespace olf_detail

// int matchGrid(const std::vector<point_2d> &points1, const cv::Mat &desc1, const GridStructure &grid, const cv::Mat &desc2, const GridWindow &w, ...)
template <class MatT>
int matchGrid(const std::vector<point_2d>& points1, const MatT& desc1, const GridStructure& grid, const MatT& desc2, const GridWindow& w, std::vector<int>& matches_12)
{
    if ((int)points1.size() != desc1.rows) throw std::runtime_error("[matchGrid] Each point needs a corresponding descriptor!");
    return olf_detail::match_grid_core(points1.size(), desc1, desc2, ORBLINE_CONFIG::minRatio12P(),
                                       [&](int i1, std::unordered_set<int>& c) { grid.get(points1[i1].first, points1[i1].second, w, c); },
                                       [](int, int) { return true; }, matches_12);
}
// int matchGrid(const std::vector<line_2d> &lines1, const cv::Mat &desc1, const GridStructure &grid, const cv::Mat &desc2,
//               const std::vector<std::pair<double, double>> &directions2, const GridWindow &w, std::vector<int> &matches_12), src/LineMatcher.cpp:220-299
template <class MatT>
int matchGrid(const std::vector<line_2d>& lines1, const MatT& desc1, const GridStructure& grid, const MatT& desc2,
              const std::vector<std::pair<double, double>>& directions2, const GridWindow& w, std::vector<int>& matches_12, double min_ratio_12_l = 0.9)
{
    if ((int)lines1.size() != desc1.rows) throw std::runtime_error("[matchGrid] Each line needs a corresponding descriptor!");
    std::vector<std::pair<double, double>> v1(lines1.size());
    for (size_t i = 0; i < lines1.size(); ++i) {
        const point_2d sp = lines1[i].first, ep = lines1[i].second;
        std::pair<double, double> v = std::make_pair((double)(ep.first - sp.first), (double)(ep.second - sp.second));
        const double mag = std::sqrt(v.first * v.first + v.second * v.second);
        v.first /= mag; v.second /= mag;
        v1[i] = v;
    }
    const double sim = ORBLINE_CONFIG::lineSimTh();
    return olf_detail::match_grid_core(lines1.size(), desc1, desc2, min_ratio_12_l,
                                       [&](int i1, std::unordered_set<int>& c) {
                                           grid.get(lines1[i1].first.first, lines1[i1].first.second, w, c);
                                           grid.get(lines1[i1].second.first, lines1[i1].second.second, w, c);
                                       },
                                       [&](int i1, int i2) { return !(std::abs(v1[i1].first * directions2[i2].first + v1[i1].second * directions2[i2].second) < sim); },
                                       matches_12);
}

// ---- void Frame::AssignFeaturesToGrid() (src/Frame.cc:334-349; called by Frame::Frame at :215, after UndistortKeyPoints) ----------------------------------
// Fills F.mGrid[i][j] (std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS], include/Frame.h:228) from olf_frame_grid: reads F.mvKeysUn and
// F.mnMinX .. F.mnMaxY, nothing else.  Every cell is assigned, so a frame that is filled twice does not accumulate.  More than OLF_GRID_MAX_KEYS key
// points throw (OLF_ERR_CAPACITY).  Frame::GetFeaturesInArea then works on the member as in the reference; the searches of this header do not read it --
// a caller that wants them to skip their own rebuild flattens it with olf_detail::GridCSR and attaches that to the view it passes to the C ABI.
template <class FrameT> void FrameGrid(FrameT& F)
{
    const int n = (int)F.mvKeysUn.size();
    std::vector<int32_t> offs(OLF_GRID_CELLS + 1, 0), idx((size_t)(n > 0 ? n : 1));
    olf_detail::check(olf_frame_grid(olf_detail::thread_ctx(), n ? olf_detail::keypoints(F.mvKeysUn) : nullptr, n, (float)F.mnMinX, (float)F.mnMaxX,
                                     (float)F.mnMinY, (float)F.mnMaxY, offs.data(), idx.data()), "olf_frame_grid");
    for (int i = 0; i < OLF_GRID_COLS; ++i)
        for (int j = 0; j < OLF_GRID_ROWS; ++j) {
            const int e = i * OLF_GRID_ROWS + j;
            F.mGrid[i][j].assign(idx.begin() + offs[e], idx.begin() + offs[e + 1]);
        }
}

namespace olf_detail {
// F.mGrid flattened into the two arrays of orbline_types.h ("Frame::mGrid as two arrays"), e.g. for olf_frame_view::grid_offsets / grid_index
struct GridCSR {
    std::vector<int32_t> offs, idx;
    template <class FrameT> explicit GridCSR(const FrameT& F)
    {
        offs.reserve(OLF_GRID_CELLS + 1);
        offs.push_back(0);
        for (int i = 0; i < OLF_GRID_COLS; ++i)
            for (int j = 0; j < OLF_GRID_ROWS; ++j) {
                for (size_t k = 0; k < F.mGrid[i][j].size(); ++k) idx.push_back((int32_t)F.mGrid[i][j][k]);
                offs.push_back((int32_t)idx.size());
            }
    }
    void attach(olf_frame_view& v) const { v.grid_offsets = offs.data(); v.grid_index = idx.data(); }
};
}  // namespace olf_detail

// ---- the feature part of Frame::Frame(imLeft, imRight, ...) (src/Frame.cc:136-221) as one call -------------------------------------------
// Replaces the four extraction threads (:164-171), ComputeStereoMatches (:202) and ComputeStereoMatches_Lines (:205): fills mvKeys,
// mvKeysRight, mDescriptors, mDescriptorsRight, mvuRight, mvDepth, mvKeys_Line, mvKeysRight_Line, mDescriptors_Line, mDescriptorsRight_Line,
// mvDisparity_l, mvle_l, N, N_l of `F`.  The parameters come from the frame's own extractor objects and camera members; the context is
// the left ORB extractor's (one per image size).  Throws like the reference when the two images differ in size (:145-146).
// Config::hasLines() == false (:37 of LineExtractor.cc, :203): no line is extracted or matched -- the key line members come back empty, N_l = 0, and the
// call runs the point half only.  A frame without key points returns like the reference's constructor does (:176-177): N = 0, N_l = the left key lines
// as extracted, and none of the stereo members (mvuRight, mvDepth, mvDisparity_l, mvle_l) is touched.
template <class FrameT, class MatT>
void StereoFrameFeatures(FrameT& F, const MatT& imLeft, const MatT& imRight, const olf_stereo_params* stereo = nullptr)
{
    if (imLeft.rows != imRight.rows || imLeft.cols != imRight.cols) throw std::runtime_error("[StereoFrame] Left and right images have different sizes");
    const int w = imLeft.cols, h = imLeft.rows;
    olf_params p = F.mpORBextractorLeft->params();
    p.line = F.mpLineextractorLeft->params().line;
    if (stereo) p.stereo = *stereo;
    p.stereo.fx = F.fx; p.stereo.bf = F.mbf;
    olf_ctx* ctx = F.mpORBextractorLeft->context(w, h, &p);
    const int cap = olf_orb_capacity(ctx), lcap = olf_line_capacity(ctx);
    const size_t npx = (size_t)w * h;
    std::vector<uint8_t> pair(2 * npx);
    for (int y = 0; y < h; ++y) {                                           // rows may be strided (a cv::Mat ROI)
        std::memcpy(&pair[(size_t)y * w], imLeft.template ptr<uint8_t>(y), w);
        std::memcpy(&pair[npx + (size_t)y * w], imRight.template ptr<uint8_t>(y), w);
    }
    std::vector<olf_keypoint> k((size_t)2 * cap);
    std::vector<uint8_t> d((size_t)2 * cap * 32), ld((size_t)2 * lcap * 32);
    std::vector<float> ur(cap), dep(cap), ldisp((size_t)2 * lcap);
    std::vector<olf_keyline> kl((size_t)2 * lcap);
    std::vector<int32_t> lm(lcap);
    std::vector<double> lle((size_t)3 * lcap);
    int32_t n[2] = {0, 0}, nl[2] = {0, 0};
    const bool lines = ORBLINE_CONFIG::hasLines();
    if (lines) {
        olf_frame_buffers o = {k.data(), d.data(), n, ur.data(), dep.data(), kl.data(), ld.data(), nl, lm.data(), ldisp.data(), lle.data()};
        olf_detail::check(olf_stereo_frames(ctx, pair.data(), 1, &o), "olf_stereo_frames");
    } else
        olf_detail::check(olf_stereo_points(ctx, pair.data(), 1, k.data(), d.data(), n, ur.data(), dep.data()), "olf_stereo_points");
    typedef typename std::remove_reference<decltype(F.mvKeys[0])>::type KP;
    typedef typename std::remove_reference<decltype(F.mvKeys_Line[0])>::type KL;
    static_assert(sizeof(KP) == sizeof(olf_keypoint) && sizeof(KL) == sizeof(olf_keyline), "cv::KeyPoint / KeyLine layout");
    auto fill_kp = [&](std::vector<KP>& dst, const olf_keypoint* src, int cnt) { dst.resize(cnt); if (cnt) std::memcpy((void*)dst.data(), src, (size_t)cnt * sizeof(KP)); };
    auto fill_kl = [&](std::vector<KL>& dst, const olf_keyline* src, int cnt) { dst.resize(cnt); if (cnt) std::memcpy((void*)dst.data(), src, (size_t)cnt * sizeof(KL)); };
    auto fill_mat = [&](MatT& m, const uint8_t* src, int cnt) { m.create(cnt, 32, 0 /* CV_8U */); if (cnt) std::memcpy(m.data, src, (size_t)cnt * 32); };
    fill_kp(F.mvKeys, k.data(), n[0]); fill_kp(F.mvKeysRight, k.data() + cap, n[1]);
    fill_mat(F.mDescriptors, d.data(), n[0]); fill_mat(F.mDescriptorsRight, d.data() + (size_t)cap * 32, n[1]);
    fill_kl(F.mvKeys_Line, kl.data(), nl[0]); fill_kl(F.mvKeysRight_Line, kl.data() + lcap, nl[1]);
    if (lines) { fill_mat(F.mDescriptors_Line, ld.data(), nl[0]); fill_mat(F.mDescriptorsRight_Line, ld.data() + (size_t)lcap * 32, nl[1]); }
    F.N = n[0]; F.N_l = nl[0];
    if (n[0] == 0) return;                                                  // "if(mvKeys.empty()) return;" (src/Frame.cc:176-177)
    F.mvuRight.assign(ur.begin(), ur.begin() + n[0]); F.mvDepth.assign(dep.begin(), dep.begin() + n[0]);
    if (!lines) return;                                                     // (src/Frame.cc:203)
    F.mvDisparity_l.resize(nl[0]); F.mvle_l.resize(nl[0]);
    for (int i = 0; i < nl[0]; ++i) {
        F.mvDisparity_l[i] = std::make_pair(ldisp[2 * i], ldisp[2 * i + 1]);
        for (int c = 0; c < 3; ++c) F.mvle_l[i][c] = lle[3 * i + c];
    }
}

// ---- class KeyFrameDatabase (include/KeyFrameDatabase.h:60-98, src/KeyFrameDatabase.cc) ---------------------------------------------------------------
// The reference's member signatures over the reference's own types; inside the reference tree
//     typedef KeyFrameDatabaseOf<KeyFrame, Frame> KeyFrameDatabase;
// takes the place of the class.  Reads of a key frame / frame: mBowVec, mBowVec_l, mnId, N, N_l, GetConnectedKeyFrames(), GetBestCovisibilityKeyFrames(10) --
// the members the reference's functions read; the covisibility graph and isBad() stay with the caller's classes.  The per-key-frame members the reference
// writes (mnLoopQuery .. mRelocScore_pl) are kept inside the database instead (per slot), so a key frame that is erased and added again starts from the
// constructor's zeros.  Query ids (pKF->mnId, F->mnId) must be > 0 and increase within a family, as the reference's counters make them; anything else
// throws.  The object owns a context and serialises its members with a mutex, as the reference's mMutex does.
template <class KeyFrameT, class FrameT>
class KeyFrameDatabaseOf {
public:
    explicit KeyFrameDatabaseOf(const ORBVocabulary& voc) : db_(nullptr) { create((int)voc.size(), 0, voc.scoring(), 0); }
    KeyFrameDatabaseOf(const ORBVocabulary& voc, const LineVocabulary& voc_l) : db_(nullptr) { create((int)voc.size(), (int)voc_l.size(), voc.scoring(), voc_l.scoring()); }
    ~KeyFrameDatabaseOf() { olf_kfdb_destroy(db_); }
    KeyFrameDatabaseOf(const KeyFrameDatabaseOf&) = delete;
    KeyFrameDatabaseOf& operator=(const KeyFrameDatabaseOf&) = delete;

    void add(KeyFrameT* pKF)                                                  // :46-55
    {
        std::unique_lock<std::mutex> lock(mMutex);
        Vec p(pKF->mBowVec), l(pKF->mBowVec_l);
        int32_t slot = -1;
        olf_detail::check(olf_kfdb_add(db_, p.ids.data(), p.vals.data(), (int)p.ids.size(), l.ids.data(), l.vals.data(), (int)l.ids.size(), &slot), "olf_kfdb_add");
        slot_of_[pKF] = slot;
        kf_of_.resize(slot + 1, nullptr);
        kf_of_[slot] = pKF;
    }
    void erase(KeyFrameT* pKF)                                                // :57-90
    {
        std::unique_lock<std::mutex> lock(mMutex);
        typename std::map<KeyFrameT*, int32_t>::iterator it = slot_of_.find(pKF);
        if (it == slot_of_.end()) return;
        olf_detail::check(olf_kfdb_erase(db_, it->second), "olf_kfdb_erase");
        kf_of_[it->second] = nullptr;
        slot_of_.erase(it);
    }
    void clear()                                                              // :92-98
    {
        std::unique_lock<std::mutex> lock(mMutex);
        olf_detail::check(olf_kfdb_clear(db_), "olf_kfdb_clear");
        slot_of_.clear(); kf_of_.clear();
    }
    std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT* pKF, float minScore) { return detect(OLF_KFDB_LOOP, *pKF, minScore, connected(pKF)); }                 // :107-228
    std::vector<KeyFrameT*> DetectLoopCandidatesWithLine(KeyFrameT* pKF, float minScore) { return detect(OLF_KFDB_LOOP_LINE, *pKF, minScore, connected(pKF)); }    // :230-400
    std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F) { return detect(OLF_KFDB_RELOC, *F, 0.f, std::vector<KeyFrameT*>()); }                        // :402-512
    std::vector<KeyFrameT*> DetectRelocalizationCandidatesWithLine(FrameT* F) { return detect(OLF_KFDB_RELOC_LINE, *F, 0.f, std::vector<KeyFrameT*>()); }           // :514-667
    olf_kfdb* handle() const { return db_; }

private:
    struct Vec {
        std::vector<int32_t> ids; std::vector<double> vals;
        template <class BowVec> explicit Vec(const BowVec& v) { for (typename BowVec::const_iterator it = v.begin(); it != v.end(); ++it) { ids.push_back((int32_t)it->first); vals.push_back(it->second); } }
    };
    void create(int nw_p, int nw_l, int sc_p, int sc_l) { olf_detail::check(olf_kfdb_create(ctx_.get(640, 480), nw_p, nw_l, sc_p, sc_l, &db_), "olf_kfdb_create"); }
    static std::vector<KeyFrameT*> connected(KeyFrameT* pKF)
    {
        const std::set<KeyFrameT*> s = pKF->GetConnectedKeyFrames();
        return std::vector<KeyFrameT*>(s.begin(), s.end());
    }
    template <class QueryT>
    std::vector<KeyFrameT*> detect(int form, QueryT& Q, float minScore, const std::vector<KeyFrameT*>& conn)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int n = (int)kf_of_.size();
        Vec p(Q.mBowVec), l(Q.mBowVec_l);
        const int32_t offp[2] = {0, (int32_t)p.ids.size()}, offl[2] = {0, (int32_t)l.ids.size()};
        const olf_bow_csr qp = {offp, p.ids.data(), p.vals.data()}, ql = {offl, l.ids.data(), l.vals.data()};
        std::vector<int32_t> conn_slots, nb_off(n + 1, 0), nb_slots;
        for (size_t i = 0; i < conn.size(); ++i) { typename std::map<KeyFrameT*, int32_t>::const_iterator it = slot_of_.find(conn[i]); if (it != slot_of_.end()) conn_slots.push_back(it->second); }
        const int32_t conn_off[2] = {0, (int32_t)conn_slots.size()};
        conn_slots.push_back(-1);                                           // (never a null pointer)
        for (int k = 0; k < n; ++k) {
            if (kf_of_[k]) {
                const std::vector<KeyFrameT*> nb = kf_of_[k]->GetBestCovisibilityKeyFrames(10);
                for (size_t i = 0; i < nb.size(); ++i) { typename std::map<KeyFrameT*, int32_t>::const_iterator it = slot_of_.find(nb[i]); nb_slots.push_back(it != slot_of_.end() ? it->second : -1); }
            }
            nb_off[k + 1] = (int32_t)nb_slots.size();
        }
        nb_slots.push_back(-1);
        const int64_t id = (int64_t)Q.mnId;
        const int32_t np = (int32_t)Q.N, nl = (int32_t)Q.N_l;
        std::vector<int32_t> cand((size_t)(n > 0 ? n : 1));
        int32_t cand_off[2] = {0, 0};
        olf_detail::check(olf_kfdb_detect(db_, form, 1, &id, &qp, &ql, &np, &nl, &minScore, conn_off, conn_slots.data(), nb_off.data(), nb_slots.data(), cand_off,
                                          cand.data(), (int)cand.size()), "olf_kfdb_detect");
        std::vector<KeyFrameT*> out;
        for (int i = 0; i < cand_off[1]; ++i) out.push_back(kf_of_[cand[i]]);
        return out;
    }
    olf_detail::Ctx ctx_;
    olf_kfdb* db_;
    std::map<KeyFrameT*, int32_t> slot_of_;
    std::vector<KeyFrameT*> kf_of_;
    std::mutex mMutex;
};

// ---- Tracking::UpdateLocalMap (src/Tracking.cc:2028-2205) over the reference's own types -------------------------------------------------------------------
// MapGraphOf<KeyFrame, MapPoint, MapLine> is one snapshot of the map as olf_update_local_map* reads it (olf_map_graph, orbline_types.h), filled through the
// accessors Tracking itself uses: MapPoint::GetObservations / isBad, KeyFrame::GetMapPointMatches / GetMapLineMatches / GetVectorCovisibleKeyFrames /
// GetChilds / GetParent / isBad, MapLine::isBad.  Key frames are numbered in the order given -- convention C.16: hand them over in the order that is
// to stand for the address order of std::map<KeyFrame*,int> and std::set<KeyFrame*> (the order of creation, mnId, is the natural one); children are sorted by
// that number.  Map points and lines are numbered by their first appearance in the key frames' slots (key-frame order, slot order).  A key frame outside the
// snapshot (an observation, a neighbour, a child, the parent) is left out; a point or line of a frame that no key frame of the snapshot holds is a temporal
// one to the call (-1).  The object owns the arrays; graph() points into them, host pointers for olf_update_local_map.
template <class KeyFrameT, class MapPointT, class MapLineT>
class MapGraphOf {
public:
    explicit MapGraphOf(const std::vector<KeyFrameT*>& kfs) : kfs_(kfs)
    {
        const int n = (int)kfs.size();
        for (int k = 0; k < n; ++k) kf_index_[kfs[k]] = k;
        kf_mp_off_.assign(1, 0); kf_ml_off_.assign(1, 0); covis_off_.assign(1, 0); child_off_.assign(1, 0);
        for (int k = 0; k < n; ++k) {
            KeyFrameT* pKF = kfs[k];
            kf_bad_.push_back(pKF->isBad() ? 1 : 0);
            const std::vector<MapPointT*> vpMPs = pKF->GetMapPointMatches();
            for (size_t i = 0; i < vpMPs.size(); ++i) kf_mp_.push_back(vpMPs[i] ? number(mp_index_, mps_, vpMPs[i]) : -1);
            kf_mp_off_.push_back((int32_t)kf_mp_.size());
            const std::vector<MapLineT*> vpMLs = pKF->GetMapLineMatches();
            for (size_t i = 0; i < vpMLs.size(); ++i) kf_ml_.push_back(vpMLs[i] ? number(ml_index_, mls_, vpMLs[i]) : -1);
            kf_ml_off_.push_back((int32_t)kf_ml_.size());
            const std::vector<KeyFrameT*> vNeighs = pKF->GetVectorCovisibleKeyFrames();
            for (size_t i = 0; i < vNeighs.size(); ++i) { const int c = index_of(vNeighs[i]); if (c >= 0) covis_.push_back(c); }
            covis_off_.push_back((int32_t)covis_.size());
            const std::set<KeyFrameT*> spChilds = pKF->GetChilds();
            std::vector<int32_t> ch;
            for (typename std::set<KeyFrameT*>::const_iterator it = spChilds.begin(); it != spChilds.end(); ++it) { const int c = index_of(*it); if (c >= 0) ch.push_back(c); }
            std::sort(ch.begin(), ch.end());                                // (C.16)
            child_.insert(child_.end(), ch.begin(), ch.end());
            child_off_.push_back((int32_t)child_.size());
            parent_.push_back(index_of(pKF->GetParent()));
        }
        mp_obs_off_.assign(1, 0);
        for (size_t i = 0; i < mps_.size(); ++i) {
            mp_bad_.push_back(mps_[i]->isBad() ? 1 : 0);
            const std::map<KeyFrameT*, size_t> observations = mps_[i]->GetObservations();
            for (typename std::map<KeyFrameT*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it) { const int c = index_of(it->first); if (c >= 0) mp_obs_.push_back(c); }
            mp_obs_off_.push_back((int32_t)mp_obs_.size());
        }
        for (size_t i = 0; i < mls_.size(); ++i) ml_bad_.push_back(mls_[i]->isBad() ? 1 : 0);
        kf_bad_.reserve(n + 1); parent_.reserve(n + 1);                     // (never a null pointer)
        const bool lines = !mls_.empty();
        g_.n_kf = n; g_.n_mp = (int32_t)mps_.size(); g_.n_ml = (int32_t)mls_.size();
        g_.mp_obs_offsets = mp_obs_off_.data(); g_.mp_obs_kf = mp_obs_.data(); g_.mp_bad = mp_bad_.data(); g_.ml_bad = lines ? ml_bad_.data() : nullptr;
        g_.kf_bad = kf_bad_.data(); g_.kf_mp_offsets = kf_mp_off_.data(); g_.kf_mp_index = kf_mp_.data();
        g_.kf_ml_offsets = lines ? kf_ml_off_.data() : nullptr; g_.kf_ml_index = lines ? kf_ml_.data() : nullptr;
        g_.kf_covis_offsets = covis_off_.data(); g_.kf_covis_index = covis_.data(); g_.kf_child_offsets = child_off_.data(); g_.kf_child_index = child_.data();
        g_.kf_parent = parent_.data();
    }
    MapGraphOf(const MapGraphOf&) = delete;
    MapGraphOf& operator=(const MapGraphOf&) = delete;

    const olf_map_graph& graph() const { return g_; }
    KeyFrameT* key_frame(int k) const { return kfs_[k]; }
    MapPointT* map_point(int i) const { return mps_[i]; }

    // What LocalMapping::KeyFrameCulling reads beyond the graph (olf_cull_view, orbline_types.h), beside graph() and parallel to its arrays; filled at the first
    // call, through what KeyFrameCulling itself reads -- mvKeysUn[i].octave, mvDepth[i], mThDepth, mnId, MapPoint::Observations() and the size_t of
    // GetObservations() -- mvuRight[i] as MapPoint::EraseObservation reads it, and mbNotErase, which is protected (include/KeyFrame.h:268): the integrator adds
    //     bool KeyFrame::GetNotErase() { unique_lock<mutex> lock(mMutexConnections); return mbNotErase; }
    // Only a caller of cull_view() needs these members of its types.  Host pointers, owned by the object.
    const olf_cull_view& cull_view()
    {
        if (view_filled_) return v_;
        for (size_t k = 0; k < kfs_.size(); ++k) {
            KeyFrameT* pKF = kfs_[k];
            const int n = kf_mp_off_[k + 1] - kf_mp_off_[k];
            for (int i = 0; i < n; ++i) {
                const int octave = i < (int)pKF->mvKeysUn.size() ? pKF->mvKeysUn[i].octave : 0;
                slot_octave_.push_back((uint8_t)std::min(std::max(octave, 0), 255));
                slot_depth_.push_back(i < (int)pKF->mvDepth.size() ? pKF->mvDepth[i] : -1.0f);
                slot_stereo_.push_back(i < (int)pKF->mvuRight.size() && pKF->mvuRight[i] >= 0 ? 1 : 0);
            }
            th_depth_.push_back(pKF->mThDepth);
            kf_mode_.push_back(pKF->mnId == 0 ? 2 : pKF->GetNotErase() ? 1 : 0);
        }
        for (size_t i = 0; i < mps_.size(); ++i) {
            mp_nobs_.push_back(mps_[i]->Observations());
            const std::map<KeyFrameT*, size_t> observations = mps_[i]->GetObservations();      // (the same keys in the same order as in the constructor)
            for (typename std::map<KeyFrameT*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it) if (index_of(it->first) >= 0) obs_slot_.push_back((int32_t)it->second);
            obs_slot_.resize(mp_obs_off_[i + 1], -1);               // (a map that changed in between: the lengths stay the graph's)
        }
        obs_slot_.reserve(1); mp_nobs_.reserve(1); slot_octave_.reserve(1); slot_depth_.reserve(1); slot_stereo_.reserve(1); th_depth_.reserve(1); kf_mode_.reserve(1);
        v_.mp_obs_slot = obs_slot_.data(); v_.mp_nobs = mp_nobs_.data(); v_.kf_slot_octave = slot_octave_.data(); v_.kf_slot_depth = slot_depth_.data();
        v_.kf_slot_stereo = slot_stereo_.data(); v_.kf_th_depth = th_depth_.data(); v_.kf_mode = kf_mode_.data();
        view_filled_ = true;
        return v_;
    }
    // MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:342-383) for the listed points of the snapshot (a point outside it is passed over), through
    // olf_update_normal_and_depth (c == NULL: the host form, no device) or olf_update_normal_and_depth_points (on the device through context c, whose level
    // table must be the key frames').  Reads GetWorldPos(), GetReferenceKeyFrame(), GetCameraCenter(), mvScaleFactors of the first key frame and cull_view();
    // the observation rows are the std::map's own iteration order.  mNormalVector, mfMaxDistance and mfMinDistance are protected (include/MapPoint.h), so
    // the integrator adds ONE accessor, whose body is the locked block :377-382 with the three values given:
    //     void MapPoint::SetNormalAndDepth(const cv::Mat& normal, float maxDistance, float minDistance);
    // It is called for every listed point the reference would have changed (not bad, observed, reference key frame inside the snapshot).  Returns their number.
    int UpdateNormalAndDepth(olf_ctx* c, const std::vector<MapPointT*>& points)
    {
        const olf_cull_view& v = cull_view();
        const size_t nm = mps_.size(), nk = kfs_.size();
        std::vector<float> world(3 * nm + 1), Ow(3 * nk + 1), normal(3 * nm + 1, 0.0f), maxd(nm + 1, -1.0f), mind(nm + 1, -1.0f), sf;
        std::vector<int32_t> ref(nm + 1, -1), list;
        for (size_t i = 0; i < nm; ++i) {
            const auto w = mps_[i]->GetWorldPos();
            for (int k = 0; k < 3; ++k) world[3 * i + k] = w.template at<float>(k);
            ref[i] = index_of(mps_[i]->GetReferenceKeyFrame());
        }
        for (size_t k = 0; k < nk; ++k) {
            const auto o = kfs_[k]->GetCameraCenter();
            for (int q = 0; q < 3; ++q) Ow[3 * k + q] = o.template at<float>(q);
        }
        for (size_t j = 0; j < points.size(); ++j) { const int i = index_of(points[j]); if (i >= 0 && ref[i] >= 0) list.push_back(i); }
        if (list.empty() || nk == 0) return 0;
        if (!c) {
            for (size_t l = 0; l < kfs_[0]->mvScaleFactors.size(); ++l) sf.push_back(kfs_[0]->mvScaleFactors[l]);
            int32_t status = 0;
            olf_detail::check(olf_update_normal_and_depth(&g_, &v, (int)list.size(), list.data(), world.data(), ref.data(), Ow.data(), sf.data(), (int)sf.size(), normal.data(),
                                                          maxd.data(), mind.data(), &status), "olf_update_normal_and_depth");
        } else
            olf_detail::check(olf_update_normal_and_depth_points(c, &g_, &v, (int)list.size(), list.data(), world.data(), ref.data(), Ow.data(), normal.data(), maxd.data(),
                                                                 mind.data()), "olf_update_normal_and_depth_points");
        int changed = 0;
        std::vector<uint8_t> done(nm + 1, 0);
        for (size_t j = 0; j < list.size(); ++j) {
            const int i = list[j];
            if (done[i] || maxd[i] == -1.0f) continue;              // (left untouched: bad, or without observations)
            done[i] = 1;
            auto n = mps_[i]->GetWorldPos();                         // (a clone: a 3 x 1 CV_32F matrix to fill)
            for (int k = 0; k < 3; ++k) n.template at<float>(k) = normal[3 * i + k];
            mps_[i]->SetNormalAndDepth(n, maxd[i], mind[i]);
            ++changed;
        }
        return changed;
    }
    int index_of(KeyFrameT* p) const { return lookup(kf_index_, p); }
    int index_of(MapPointT* p) const { return lookup(mp_index_, p); }
    int line_index_of(MapLineT* p) const { return lookup(ml_index_, p); }

    // a frame's mvpMapPoints / mvpMapLines as rows of d_frame_mp / d_frame_ml: mp_row [cap], ml_row [lcap] (or NULL), -1 from N / N_l on
    template <class FrameT> void FrameRows(const FrameT& F, int32_t* mp_row, int cap, int32_t* ml_row, int lcap) const
    {
        for (int i = 0; i < cap; ++i) mp_row[i] = i < (int)F.mvpMapPoints.size() && F.mvpMapPoints[i] ? index_of(F.mvpMapPoints[i]) : -1;
        if (ml_row) for (int i = 0; i < lcap; ++i) ml_row[i] = i < (int)F.mvpMapLines.size() && F.mvpMapLines[i] ? line_index_of(F.mvpMapLines[i]) : -1;
    }

    // What UpdateLocalMap leaves behind for frame j of a batch, from the outputs of olf_update_local_map*: the held points and lines that were bad are set to
    // NULL (:2097, :2114; mp_row_in / mp_row_out: the frame's rows before and after, ml rows or NULL); with n_voted[j] == 0 nothing else changes (the
    // reference returns at :2120 and rebuilds its point lists from the key frames it had: the caller's chain); otherwise mvpLocalKeyFrames, mvpLocalMapPoints
    // and mvpLocalMapLines are replaced, and mpReferenceKF and the frame's mpReferenceKF are set when ref_kf[j] >= 0 (:2200-2204).
    template <class FrameT>
    void WriteBack(int j, FrameT& F, const int32_t* mp_row_in, const int32_t* mp_row_out, const int32_t* ml_row_in, const int32_t* ml_row_out, const int32_t* ref_kf,
                   const int32_t* n_voted, const int32_t* kf_offsets, const int32_t* kf_index, const int32_t* mp_offsets, const int32_t* mp_index,
                   const int32_t* ml_offsets, const int32_t* ml_index, std::vector<KeyFrameT*>& mvpLocalKeyFrames, std::vector<MapPointT*>& mvpLocalMapPoints,
                   std::vector<MapLineT*>& mvpLocalMapLines, KeyFrameT*& mpReferenceKF) const
    {
        for (size_t i = 0; i < F.mvpMapPoints.size(); ++i) if (mp_row_in[i] >= 0 && mp_row_out[i] < 0) F.mvpMapPoints[i] = static_cast<MapPointT*>(nullptr);
        if (ml_row_in && ml_row_out) for (size_t i = 0; i < F.mvpMapLines.size(); ++i) if (ml_row_in[i] >= 0 && ml_row_out[i] < 0) F.mvpMapLines[i] = static_cast<MapLineT*>(nullptr);
        if (n_voted[j] == 0) return;
        mvpLocalKeyFrames.clear(); mvpLocalMapPoints.clear(); mvpLocalMapLines.clear();
        for (int e = kf_offsets[j]; e < kf_offsets[j + 1]; ++e) mvpLocalKeyFrames.push_back(kfs_[kf_index[e]]);
        for (int e = mp_offsets[j]; e < mp_offsets[j + 1]; ++e) mvpLocalMapPoints.push_back(mps_[mp_index[e]]);
        for (int e = ml_offsets[j]; e < ml_offsets[j + 1]; ++e) mvpLocalMapLines.push_back(mls_[ml_index[e]]);
        if (ref_kf[j] >= 0) { mpReferenceKF = kfs_[ref_kf[j]]; F.mpReferenceKF = mpReferenceKF; }
    }

private:
    template <class T> static int lookup(const std::map<T*, int32_t>& m, T* p)
    {
        if (!p) return -1;
        typename std::map<T*, int32_t>::const_iterator it = m.find(p);
        return it == m.end() ? -1 : it->second;
    }
    template <class T> static int32_t number(std::map<T*, int32_t>& m, std::vector<T*>& v, T* p)
    {
        typename std::map<T*, int32_t>::const_iterator it = m.find(p);
        if (it != m.end()) return it->second;
        const int32_t i = (int32_t)v.size();
        m[p] = i; v.push_back(p);
        return i;
    }
    std::vector<KeyFrameT*> kfs_; std::vector<MapPointT*> mps_; std::vector<MapLineT*> mls_;
    std::map<KeyFrameT*, int32_t> kf_index_; std::map<MapPointT*, int32_t> mp_index_; std::map<MapLineT*, int32_t> ml_index_;
    std::vector<int32_t> mp_obs_off_, mp_obs_, kf_mp_off_, kf_mp_, kf_ml_off_, kf_ml_, covis_off_, covis_, child_off_, child_, parent_;
    std::vector<uint8_t> mp_bad_, ml_bad_, kf_bad_;
    olf_map_graph g_;
    std::vector<int32_t> obs_slot_, mp_nobs_;
    std::vector<uint8_t> slot_octave_, slot_stereo_, kf_mode_;
    std::vector<float> slot_depth_, th_depth_;
    olf_cull_view v_;
    bool view_filled_ = false;
};

// UpdateLocalMap for one frame through the host form, as Tracking::UpdateLocalMap is called (:2028): the snapshot, the call, the write-back.  Tracking's
// members are passed by reference.  A batch caller uses MapGraphOf, olf_update_local_map[_batch_dev] and WriteBack itself.
template <class KeyFrameT, class MapPointT, class MapLineT, class FrameT>
void UpdateLocalMap(const std::vector<KeyFrameT*>& vpKeyFrames, FrameT& mCurrentFrame, std::vector<KeyFrameT*>& mvpLocalKeyFrames,
                    std::vector<MapPointT*>& mvpLocalMapPoints, std::vector<MapLineT*>& mvpLocalMapLines, KeyFrameT*& mpReferenceKF)
{
    olf_ctx* c = olf_detail::thread_ctx();
    const MapGraphOf<KeyFrameT, MapPointT, MapLineT> G(vpKeyFrames);
    const int cap = olf_orb_capacity(c), lcap = olf_line_capacity(c);
    if ((int)mCurrentFrame.mvpMapPoints.size() > cap || (int)mCurrentFrame.mvpMapLines.size() > lcap) throw std::runtime_error("UpdateLocalMap: the frame holds more features than the context");
    std::vector<int32_t> mp_in(cap), mp_out(cap), ml_in(lcap), ml_out(lcap);
    G.FrameRows(mCurrentFrame, mp_in.data(), cap, ml_in.data(), lcap);
    const int32_t n = (int32_t)mCurrentFrame.mvpMapPoints.size(), nl = (int32_t)mCurrentFrame.mvpMapLines.size();
    const olf_map_graph& g = G.graph();
    std::vector<int32_t> kf_index((size_t)g.n_kf + 1), mp_index((size_t)g.n_mp + 1), ml_index((size_t)g.n_ml + 1);      // (a list holds an item once)
    int32_t ref = -1, voted = 0, kf_off[2], mp_off[2], ml_off[2];
    olf_detail::check(olf_update_local_map(c, &g, 1, 1, &n, &nl, mp_in.data(), g.n_ml ? ml_in.data() : nullptr, mp_out.data(), g.n_ml ? ml_out.data() : nullptr, &ref, &voted,
                                           kf_off, kf_index.data(), g.n_kf, mp_off, mp_index.data(), g.n_mp, ml_off, ml_index.data(), g.n_ml), "olf_update_local_map");
    G.WriteBack(0, mCurrentFrame, mp_in.data(), mp_out.data(), g.n_ml ? ml_in.data() : nullptr, g.n_ml ? ml_out.data() : nullptr, &ref, &voted, kf_off, kf_index.data(),
                mp_off, mp_index.data(), ml_off, ml_index.data(), mvpLocalKeyFrames, mvpLocalMapPoints, mvpLocalMapLines, mpReferenceKF);
}

// ---- KeyFrame::UpdateConnections (src/KeyFrame.cc:446-557) over the reference's own types ----------------------------------------------------------------
// The three members UpdateConnections writes (mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights), mbFirstConnection and mpParent are
// protected (include/KeyFrame.h:235-262), so the integrator adds ONE accessor to KeyFrame whose body is the locked block :541-556 as it stands:
//     void KeyFrame::SetConnections(const std::map<KeyFrame*,int>& KFcounter, const std::vector<KeyFrame*>& vpOrdered, const std::vector<int>& vOrderedWeights)
//     {
//         unique_lock<mutex> lockCon(mMutexConnections);
//         mConnectedKeyFrameWeights = KFcounter;  mvpOrderedConnectedKeyFrames = vpOrdered;  mvOrderedWeights = vOrderedWeights;
//         if(mbFirstConnection && mnId!=0) { mpParent = mvpOrderedConnectedKeyFrames.front();  mpParent->AddChild(this);  mbFirstConnection = false; }
//     }
// ApplyConnections performs, in list order, what the reference does to the objects, from the outputs of olf_update_connections* for `list` (entry j = list[j]):
// the reciprocal AddConnection(this, w) on every key frame of the ordered row (:522, :529; public), in ascending index as the loop :512-524 makes them, then
// the key frame's own members and first-connection parent through SetConnections.  A key frame with n_counted[j] == 0 is left untouched (:501).
template <class KeyFrameT, class MapPointT, class MapLineT>
void ApplyConnections(const MapGraphOf<KeyFrameT, MapPointT, MapLineT>& G, const std::vector<KeyFrameT*>& list, const int32_t* n_counted, const int32_t* conn_offsets,
                      const int32_t* conn_index, const int32_t* conn_weight, const int32_t* covis_offsets, const int32_t* covis_index, const int32_t* covis_weight)
{
    for (size_t j = 0; j < list.size(); ++j) {
        if (n_counted[j] == 0) continue;
        KeyFrameT* pKF = list[j];
        std::map<KeyFrameT*, int> KFcounter;
        for (int e = conn_offsets[j]; e < conn_offsets[j + 1]; ++e) KFcounter[G.key_frame(conn_index[e])] = conn_weight[e];
        std::vector<std::pair<int32_t, int32_t> > reciprocal;        // (index, weight)
        std::vector<KeyFrameT*> vpOrdered;
        std::vector<int> vOrderedWeights;
        for (int e = covis_offsets[j]; e < covis_offsets[j + 1]; ++e) {
            reciprocal.push_back(std::make_pair(covis_index[e], covis_weight[e]));
            vpOrdered.push_back(G.key_frame(covis_index[e]));
            vOrderedWeights.push_back(covis_weight[e]);
        }
        std::sort(reciprocal.begin(), reciprocal.end());
        for (size_t i = 0; i < reciprocal.size(); ++i) G.key_frame(reciprocal[i].first)->AddConnection(pKF, reciprocal[i].second);
        pKF->SetConnections(KFcounter, vpOrdered, vOrderedWeights);
    }
}

// UpdateConnections for every key frame of `list`, each against the snapshot G as it stands, through the host form: the call (a first one sizes the two
// lists), then ApplyConnections.  Every listed key frame must be one of the snapshot's.
template <class KeyFrameT, class MapPointT, class MapLineT>
void UpdateConnections(const MapGraphOf<KeyFrameT, MapPointT, MapLineT>& G, const std::vector<KeyFrameT*>& list, int th = OLF_COVIS_TH)
{
    olf_ctx* c = olf_detail::thread_ctx();
    const int n = (int)list.size();
    std::vector<int32_t> idx(n + 1), n_counted(n + 1), kf_max(n + 1), w_max(n + 1), conn_off(n + 1, 0), covis_off(n + 1, 0), conn(1), conn_w(1), covis(1), covis_w(1);
    for (int j = 0; j < n; ++j) {
        idx[j] = G.index_of(list[j]);
        if (idx[j] < 0) throw std::invalid_argument("UpdateConnections: a listed key frame is not in the snapshot");
    }
    const olf_map_graph& g = G.graph();
    int rc = olf_update_connections(c, &g, n, idx.data(), th, n_counted.data(), kf_max.data(), w_max.data(), conn_off.data(), conn.data(), conn_w.data(), 0, covis_off.data(),
                                    covis.data(), covis_w.data(), 0);
    if (rc == OLF_ERR_CAPACITY && conn_off[n] > 0) {                  // (the offsets are complete whatever the capacities)
        conn.resize(conn_off[n]); conn_w.resize(conn_off[n]); covis.resize(covis_off[n]); covis_w.resize(covis_off[n]);
        rc = olf_update_connections(c, &g, n, idx.data(), th, n_counted.data(), kf_max.data(), w_max.data(), conn_off.data(), conn.data(), conn_w.data(), conn_off[n],
                                    covis_off.data(), covis.data(), covis_w.data(), covis_off[n]);
    }
    olf_detail::check(rc, "olf_update_connections");
    ApplyConnections(G, list, n_counted.data(), conn_off.data(), conn.data(), conn_w.data(), covis_off.data(), covis.data(), covis_w.data());
}

// ---- LocalMapping::KeyFrameCulling (src/LocalMapping.cc:632-696) over the reference's own types ---------------------------------------------------------
// The snapshot KeyFrameCulling needs: the listed key frames first, in their order, then every other key frame that observes a point one of them holds (the
// observer's octave is read, :675).  No order among key frames matters to the result.
template <class KeyFrameT, class MapPointT>
std::vector<KeyFrameT*> CullingSnapshot(const std::vector<KeyFrameT*>& list)
{
    std::vector<KeyFrameT*> kfs;
    std::set<KeyFrameT*> seen;
    for (size_t j = 0; j < list.size(); ++j) if (seen.insert(list[j]).second) kfs.push_back(list[j]);
    const size_t n_listed = kfs.size();
    for (size_t j = 0; j < n_listed; ++j) {
        const std::vector<MapPointT*> vpMapPoints = kfs[j]->GetMapPointMatches();
        for (size_t i = 0; i < vpMapPoints.size(); ++i) {
            if (!vpMapPoints[i] || vpMapPoints[i]->isBad()) continue;
            const std::map<KeyFrameT*, size_t> observations = vpMapPoints[i]->GetObservations();
            for (typename std::map<KeyFrameT*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it) if (seen.insert(it->first).second) kfs.push_back(it->first);
        }
    }
    return kfs;
}

// What the reference does to the objects, from decision [list.size()] of olf_keyframe_culling*: SetBadFlag() on the key frames whose decision is not 0, in
// list order.  SetBadFlag itself sorts out mbNotErase (decision 2: it sets mbToBeErased and returns, src/KeyFrame.cc:637-641), erases the observations,
// lets the points with nObs <= 2 go bad and repairs the spanning tree.
template <class KeyFrameT>
void ApplyKeyFrameCulling(const std::vector<KeyFrameT*>& list, const int32_t* decision)
{
    for (size_t j = 0; j < list.size(); ++j) if (decision[j] != 0) list[j]->SetBadFlag();
}

// KeyFrameCulling as LocalMapping calls it (:84): GetVectorCovisibleKeyFrames() of the current key frame, the snapshot, the host form on context c (NULL:
// the thread's matcher context), then ApplyKeyFrameCulling.  Returns the decisions in list order.
template <class KeyFrameT, class MapPointT, class MapLineT>
std::vector<int32_t> KeyFrameCulling(olf_ctx* c, KeyFrameT* pCurrentKF, bool bMonocular)
{
    const std::vector<KeyFrameT*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
    const int n = (int)vpLocalKeyFrames.size();
    std::vector<int32_t> decision(n + 1, 0), n_mps(n + 1), n_red(n + 1), idx(n + 1);
    if (n == 0) { decision.resize(0); return decision; }
    MapGraphOf<KeyFrameT, MapPointT, MapLineT> G(CullingSnapshot<KeyFrameT, MapPointT>(vpLocalKeyFrames));
    for (int j = 0; j < n; ++j) idx[j] = G.index_of(vpLocalKeyFrames[j]);
    const olf_map_graph& g = G.graph();
    const olf_cull_view& v = G.cull_view();
    olf_detail::check(olf_keyframe_culling(c ? c : olf_detail::thread_ctx(), &g, &v, n, idx.data(), bMonocular ? 1 : 0, decision.data(), n_mps.data(), n_red.data(), nullptr,
                                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "olf_keyframe_culling");
    decision.resize(n);
    ApplyKeyFrameCulling(vpLocalKeyFrames, decision.data());
    return decision;
}

// ---- LocalMapping::ComputeF12 and the triangulation loop of CreateNewMapPoints (src/LocalMapping.cc:536-553, :245-253, :286-431) over the reference's types ----
// c == NULL: the host forms (olf_compute_f12, olf_create_new_map_points; no device); otherwise the pair runs on the device through context c
// (olf_compute_f12_pairs, olf_create_new_map_points_pairs), whose capacity must hold both key frames and whose level table must be theirs.
// ComputeF12 reads GetPose() and fx, fy, cx, cy of pKF1 (mK of both) and returns the reference's matrix type, 3 x 3 CV_32F.
template <class KeyFrameT>
auto ComputeF12(olf_ctx* c, KeyFrameT* pKF1, KeyFrameT* pKF2) -> decltype(pKF1->GetRotation())
{
    float T[32], F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    olf_detail::mat4(pKF1->GetPose(), T);
    olf_detail::mat4(pKF2->GetPose(), T + 16);
    const int32_t pair[2] = {0, 1};
    if (!c) olf_detail::check(olf_compute_f12(T, T + 16, pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy, F), "olf_compute_f12");
    else olf_detail::check(olf_compute_f12_pairs(c, T, 2, pKF1->fx, pKF1->fy, pKF1->cx, pKF1->cy, 1, pair, F), "olf_compute_f12_pairs");
    auto F12 = pKF1->GetRotation();                                  // (a clone: a 3 x 3 CV_32F matrix to fill)
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) F12.template at<float>(r, k) = F[3 * r + k];
    return F12;
}

// What the loop at :286-450 decides for the matches of one neighbour, in the order of vMatchedIndices: code (include/orbline.h: 1 to 3 created, 16 to 23 the
// reference's `continue`s, 0 left out), the point of the created ones, and nnew.  `new MapPoint(x3D, ...)`, AddObservation, AddMapPoint,
// ComputeDistinctiveDescriptors, UpdateNormalAndDepth and the two lists (:434-447) stay the caller's, for the codes 1 to 3 in this order.
struct NewMapPoints {
    std::vector<uint8_t> code;
    std::vector<float> x3D;                                          // three per match
    int nnew = 0;
    bool skipped = false;                                            // the baseline test of :249-253 skipped the neighbour
};
// Reads mvKeysUn, mvuRight, mvDepth, N, GetPose(), fx, fy, cx, cy, mbf, mb and mvScaleFactors of the two key frames.  A match whose idx1 was listed before
// is computed on its own (the row of the C entry holds one idx2 per idx1, so such a list goes down in several calls).
template <class KeyFrameT>
void CreateNewMapPoints(olf_ctx* c, KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<std::pair<size_t, size_t> >& vMatchedIndices, bool bMonocular, NewMapPoints& out)
{
    const int nm = (int)vMatchedIndices.size();
    out.code.assign(nm, 0); out.x3D.assign(3 * (size_t)nm, 0.0f); out.nnew = 0; out.skipped = false;
    const int N1 = (int)pKF1->mvKeysUn.size(), N2 = (int)pKF2->mvKeysUn.size();
    const int cap = c ? olf_orb_capacity(c) : std::max(std::max(N1, N2), 1);
    if (N1 > cap || N2 > cap) throw std::runtime_error("CreateNewMapPoints: the context's capacity does not hold the key frames");
    std::vector<olf_keypoint> kps(2 * (size_t)cap);
    std::vector<float> ur(2 * (size_t)cap, -1.0f), depth(2 * (size_t)cap, -1.0f), sf, x3D(3 * (size_t)cap);
    std::vector<uint8_t> code(cap);
    KeyFrameT* kf[2] = {pKF1, pKF2};
    const int32_t counts[2] = {N1, N2}, pair[2] = {0, 1};
    float T[32];
    for (int j = 0; j < 2; ++j) {
        olf_detail::mat4(kf[j]->GetPose(), T + 16 * j);
        if (counts[j]) std::memcpy(&kps[(size_t)j * cap], olf_detail::keypoints(kf[j]->mvKeysUn), (size_t)counts[j] * sizeof(olf_keypoint));
        for (int i = 0; i < counts[j]; ++i) { ur[(size_t)j * cap + i] = kf[j]->mvuRight[i]; depth[(size_t)j * cap + i] = kf[j]->mvDepth[i]; }
    }
    for (size_t l = 0; l < pKF1->mvScaleFactors.size(); ++l) sf.push_back(pKF1->mvScaleFactors[l]);
    olf_track_batch in;
    std::memset(&in, 0, sizeof in);
    in.kps = kps.data(); in.counts = counts; in.img_stride = 1; in.uright = ur.data(); in.Tcw = T;
    in.fx = pKF1->fx; in.fy = pKF1->fy; in.cx = pKF1->cx; in.cy = pKF1->cy; in.mbf = pKF1->mbf;
    std::vector<uint8_t> taken(nm, 0);
    for (int left = nm; left > 0;) {                                 // one call per round of distinct idx1 (one round for a list as the search returns it)
        std::vector<int32_t> row(cap, -1), who(cap, -1);
        for (int m = 0; m < nm; ++m) {
            const size_t i1 = vMatchedIndices[m].first;
            if (taken[m] || i1 >= (size_t)cap) { if (!taken[m]) { taken[m] = 1; --left; } continue; }
            if (who[i1] >= 0) continue;
            who[i1] = m; row[i1] = vMatchedIndices[m].second < (size_t)cap ? (int32_t)vMatchedIndices[m].second : -1;
            taken[m] = 1; --left;
        }
        int32_t nnew = 0, status = 0;
        if (!c) olf_detail::check(olf_create_new_map_points(&in, cap, 2, depth.data(), pKF2->mb, sf.data(), (int)sf.size(), 1, pair, row.data(), bMonocular ? 1 : 0, x3D.data(),
                                                            code.data(), &nnew, &status), "olf_create_new_map_points");
        else olf_detail::check(olf_create_new_map_points_pairs(c, &in, 2, depth.data(), pKF2->mb, 1, pair, row.data(), bMonocular ? 1 : 0, x3D.data(), code.data(), &nnew),
                               "olf_create_new_map_points_pairs");
        for (int i = 0; i < cap; ++i) {
            if (who[i] < 0) continue;
            out.code[who[i]] = code[i];
            for (int k = 0; k < 3; ++k) out.x3D[3 * (size_t)who[i] + k] = x3D[3 * (size_t)i + k];
        }
        out.nnew += nnew;
    }
    // (a skipped neighbour: every row is 0 and nnew is 0 although there were matches; the test itself is cheap to restate for the flag)
    if (nm && !bMonocular) {
        const auto O1 = pKF1->GetCameraCenter(), O2 = pKF2->GetCameraCenter();
        double s = 0;
        for (int k = 0; k < 3; ++k) { const float d = O2.template at<float>(k) - O1.template at<float>(k); s += (double)d * (double)d; }
        out.skipped = (float)std::sqrt(s) < pKF2->mb;
    }
}

// ---- Optimizer::PoseOptimizationWithLine (src/Optimizer.cc:604-697) over the reference's own types ----------------------------------------------------------
// Reads what the reference reads of the frame -- mvpMapPoints with GetWorldPos(), mvpMapLines with mWorldPos_sP / mWorldPos_eP, mvKeysUn, mvKeysUn_Line,
// mvle_l, mTcw, mTcw_prev (empty: mTcw), DT_cov, the calibration, mvInvLevelSigma2, mvbOutlier, mvbOutlier_Line -- and writes what it writes: mTcw through
// SetPose, DT, DT_cov, DT_cov_eig, err_norm, mvbOutlier, mvbOutlier_Line and n_inliers, n_inliers_pt, n_inliers_ls.  c == NULL: the host form
// (olf_pose_optimization_with_line, no device); otherwise the frame runs on the device through context c, whose capacities must hold the frame and whose
// level table must be the frame's.  params: Config's maxItersRef(), homogTh(), minError(), minErrorChange(), inlierK(), useMotionModel(), hasPoints(),
// hasLines() (NULL: their defaults).  Returns true, as the reference does; *status (or NULL) receives the frame's status word: the cases the reference
// leaves undefined pass the pose through (include/orbline.h).
template <class FrameT>
bool PoseOptimizationWithLine(olf_ctx* c, FrameT* pFrame, const olf_pose_params* params = nullptr, int32_t* status = nullptr)
{
    typedef typename std::remove_const<typename std::remove_reference<decltype(pFrame->mTcw)>::type>::type MatT;
    typedef typename std::remove_reference<decltype(pFrame->mvKeysUn[0])>::type KP;
    typedef typename std::remove_reference<decltype(pFrame->mvKeysUn_Line[0])>::type KL;
    static_assert(sizeof(KP) == sizeof(olf_keypoint) && sizeof(KL) == sizeof(olf_keyline), "cv::KeyPoint / KeyLine layout");
    olf_pose_params p;
    if (params) p = *params; else olf_pose_default_params(&p);
    const int N = (int)pFrame->mvpMapPoints.size(), NL = (int)pFrame->mvpMapLines.size();
    std::vector<int32_t> fmp(N + 1, -1), fml(NL + 1, -1);
    std::vector<float> mpw, mlw;
    std::vector<uint8_t> out(N + 1, 0), outl(NL + 1, 0);
    std::vector<double> lle(3 * (size_t)NL + 3, 0.0);
    for (int i = 0; i < N; ++i) {
        out[i] = pFrame->mvbOutlier[i] ? 1 : 0;
        if (!pFrame->mvpMapPoints[i]) continue;
        const auto wp = pFrame->mvpMapPoints[i]->GetWorldPos();
        fmp[i] = (int32_t)(mpw.size() / 3);
        for (int k = 0; k < 3; ++k) mpw.push_back(wp.template at<float>(k));
    }
    for (int i = 0; i < NL; ++i) {
        outl[i] = pFrame->mvbOutlier_Line[i] ? 1 : 0;
        for (int k = 0; k < 3; ++k) lle[3 * i + k] = pFrame->mvle_l[i][k];
        if (!pFrame->mvpMapLines[i]) continue;
        fml[i] = (int32_t)(mlw.size() / 6);
        for (int k = 0; k < 3; ++k) mlw.push_back((float)pFrame->mvpMapLines[i]->mWorldPos_sP[k]);
        for (int k = 0; k < 3; ++k) mlw.push_back((float)pFrame->mvpMapLines[i]->mWorldPos_eP[k]);
    }
    float Tcw[16], Tprev[16], Tout[16];
    double cov_in[36], DT[16], cov[36], eig[6], err = -1.0;
    olf_detail::mat4(pFrame->mTcw, Tcw);
    const bool has_prev = !pFrame->mTcw_prev.empty();
    if (has_prev) olf_detail::mat4(pFrame->mTcw_prev, Tprev);
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) cov_in[6 * i + j] = pFrame->DT_cov(i, j);
    const int32_t counts[1] = {N}, lcounts[1] = {NL};
    olf_pose_batch in;
    std::memset(&in, 0, sizeof(in));
    in.kps = reinterpret_cast<const olf_keypoint*>(pFrame->mvKeysUn.data()); in.counts = counts;
    in.kls = reinterpret_cast<const olf_keyline*>(pFrame->mvKeysUn_Line.data()); in.lcounts = lcounts; in.img_stride = 1;
    in.lle = lle.data(); in.Tcw = Tcw; in.Tcw_prev = has_prev ? Tprev : nullptr; in.DT_cov_in = cov_in;
    in.fx = pFrame->fx; in.fy = pFrame->fy; in.cx = pFrame->cx; in.cy = pFrame->cy;
    in.frame_mp = fmp.data(); in.mp_world = mpw.data(); in.n_mp = (int32_t)(mpw.size() / 3);
    in.frame_ml = fml.data(); in.ml_world = mlw.data(); in.n_ml = (int32_t)(mlw.size() / 6);
    in.outlier = out.data(); in.outlier_l = outl.data();
    uint8_t good = 0;
    int32_t inl[2] = {0, 0}, iters[4], st = 0;
    const olf_pose_outputs o = {Tout, DT, cov, eig, &err, &good, out.data(), outl.data(), inl, iters, &st};
    if (c) olf_detail::check(olf_pose_optimization_with_line_frame(c, &in, &p, &o), "olf_pose_optimization_with_line_frame");
    else olf_detail::check(olf_pose_optimization_with_line(&in, N, NL, pFrame->mvInvLevelSigma2.data(), (int)pFrame->mvInvLevelSigma2.size(), &p, &o),
                           "olf_pose_optimization_with_line");
    MatT T(4, 4, 5 /* CV_32F */);
    for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) T.template at<float>(r, k) = Tout[4 * r + k];
    pFrame->SetPose(T);
    for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) pFrame->DT(r, k) = DT[4 * r + k];
    for (int i = 0; i < 6; ++i) { pFrame->DT_cov_eig(i) = eig[i]; for (int j = 0; j < 6; ++j) pFrame->DT_cov(i, j) = cov[6 * i + j]; }
    pFrame->err_norm = err;
    for (int i = 0; i < N; ++i) if (pFrame->mvpMapPoints[i]) pFrame->mvbOutlier[i] = out[i] != 0;          // (removeOutliers looks at held features only)
    for (int i = 0; i < NL; ++i) if (pFrame->mvpMapLines[i]) pFrame->mvbOutlier_Line[i] = outl[i] != 0;
    pFrame->n_inliers_pt = inl[0]; pFrame->n_inliers_ls = inl[1]; pFrame->n_inliers = inl[0] + inl[1];
    if (status) *status = st;
    return true;
}

// ---- Optimizer::PoseOptimization (src/Optimizer.cc:239-451) over the reference's own types --------------------------------------------------------------------
// Reads what the reference reads of the frame -- mvpMapPoints with GetWorldPos(), mvKeysUn, mvuRight, mTcw, fx, fy, cx, cy, mbf, mvInvLevelSigma2 -- and
// writes what it writes: mvbOutlier of every held feature and mTcw through SetPose; returns nInitialCorrespondences - nBad.  c == NULL: the host form
// (olf_pose_optimization, no device); otherwise the frame runs on the device through context c (olf_pose_optimization_rows), whose capacity must hold the
// frame and whose level table must be the frame's.  *status (or NULL) receives the row's status word: where the reference is undefined (a depth of 0, a
// non-finite system) the pose is not set, the flags stay as the last completed pass left them and 0 is returned (include/orbline.h).
template <class FrameT>
int PoseOptimization(olf_ctx* c, FrameT* pFrame, int32_t* status = nullptr)
{
    typedef typename std::remove_const<typename std::remove_reference<decltype(pFrame->mTcw)>::type>::type MatT;
    typedef typename std::remove_reference<decltype(pFrame->mvKeysUn[0])>::type KP;
    static_assert(sizeof(KP) == sizeof(olf_keypoint), "cv::KeyPoint layout");
    const int N = (int)pFrame->mvpMapPoints.size();
    const int cap = c ? olf_orb_capacity(c) : N;
    if (N > cap) olf_detail::check(OLF_ERR_CAPACITY, "PoseOptimization: more features than the context's capacity");
    std::vector<olf_keypoint> kps((size_t)cap + 1);
    std::vector<int32_t> fmp((size_t)cap + 1, -1);
    std::vector<float> mpw, ur((size_t)cap + 1, -1.f), chi2((size_t)cap + 1, 0.f);
    std::vector<uint8_t> out((size_t)cap + 1, 0);
    if (N) std::memcpy(kps.data(), pFrame->mvKeysUn.data(), (size_t)N * sizeof(olf_keypoint));
    for (int i = 0; i < N; ++i) {
        ur[i] = pFrame->mvuRight[i];
        if (!pFrame->mvpMapPoints[i]) continue;
        const auto wp = pFrame->mvpMapPoints[i]->GetWorldPos();
        fmp[i] = (int32_t)(mpw.size() / 3);
        for (int k = 0; k < 3; ++k) mpw.push_back(wp.template at<float>(k));
    }
    float Tcw[16], Tout[16];
    olf_detail::mat4(pFrame->mTcw, Tcw);
    const int32_t counts[1] = {N};
    olf_pose_points_batch in;
    std::memset(&in, 0, sizeof(in));
    in.kps = kps.data(); in.counts = counts; in.img_stride = 1; in.uright = ur.data();
    in.fx = pFrame->fx; in.fy = pFrame->fy; in.cx = pFrame->cx; in.cy = pFrame->cy; in.bf = pFrame->mbf;
    in.Tcw = Tcw; in.frame_mp = fmp.data(); in.mp_world = mpw.data(); in.n_mp = (int32_t)(mpw.size() / 3);
    int32_t good = 0, initial = 0, passes = 0, iters[4], st = 0;
    const olf_pose_points_outputs o = {Tout, out.data(), &good, &initial, chi2.data(), &passes, iters, &st};
    if (c) olf_detail::check(olf_pose_optimization_rows(c, &in, 1, 1, &o), "olf_pose_optimization_rows");
    else olf_detail::check(olf_pose_optimization(&in, cap, 1, pFrame->mvInvLevelSigma2.data(), (int)pFrame->mvInvLevelSigma2.size(), &o), "olf_pose_optimization");
    for (int i = 0; i < N; ++i) if (pFrame->mvpMapPoints[i]) pFrame->mvbOutlier[i] = out[i] != 0;
    if (status) *status = st;
    if (initial < 3 || (st & 3)) return 0;                          // :364-365 returns before SetPose; a stopped row leaves the pose alone
    MatT T(4, 4, 5 /* CV_32F */);
    for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) T.template at<float>(r, k) = Tout[4 * r + k];
    pFrame->SetPose(T);
    return good;
}

// ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:2013-2208) over the reference's own types ------------------------------------------------------------------------
// The reference's signature behind the context: reads GetMapPointMatches(), GetPose(), mvKeysUn, mvInvLevelSigma2 and fx, fy, cx, cy of the key frames
// (K1 = K2), isBad(), GetWorldPos() and GetIndexInKeyFrame() of the points, and rotation() / translation() / scale() of g2oS12; nulls the outliers of
// vpMatches1, writes g2oS12 where the reference writes it and returns nIn.  The C entry's per-feature model (a match row of kf2 feature indices) is met by
// laying kf2's matched features out at their kf1 index in a frame of their own.  The start passes through floats (s, the rotation matrix, t), which is what
// LoopClosing::ComputeSim3 builds g2oS12 from (src/LoopClosing.cc:325-327).  c == NULL: the host form (olf_optimize_sim3, no device); otherwise the pair
// runs on the device through context c (olf_optimize_sim3_pairs), whose capacity must hold vpMatches1 and whose level table must be the key frames'.
// *status (or NULL) receives the pair's status word: where the reference is undefined (a depth of 0, a non-finite system) g2oS12 is not written, the
// matches stay as they stood at that moment and 0 is returned (include/orbline.h).
template <class KeyFrameT, class MapPointT, class Sim3T>
int OptimizeSim3(olf_ctx* c, KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12, const float th2, const bool bFixScale,
                 int32_t* status = nullptr)
{
    typedef typename std::remove_const<typename std::remove_reference<decltype(g2oS12.rotation())>::type>::type QuatT;
    typedef typename std::remove_const<typename std::remove_reference<decltype(g2oS12.translation())>::type>::type VecT;
    const int N = (int)vpMatches1.size();
    const int cap = c ? olf_orb_capacity(c) : std::max(N, 1);
    if (N > cap) olf_detail::check(OLF_ERR_CAPACITY, "OptimizeSim3: more matches than the context's capacity");
    const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<olf_keypoint> kps(2 * (size_t)cap);
    std::vector<float> world(6 * (size_t)cap, 0.f), chi2(2 * (size_t)cap, 0.f);
    std::vector<uint8_t> valid(2 * (size_t)cap, 0), bad(2 * (size_t)cap, 0);
    std::vector<int32_t> row((size_t)cap, -1);
    for (int i = 0; i < N; ++i) {
        std::memcpy(&kps[i], olf_detail::keypoints(pKF1->mvKeysUn) + i, sizeof(olf_keypoint));
        MapPointT* pMP1 = i < (int)vpMapPoints1.size() ? vpMapPoints1[i] : nullptr;
        MapPointT* pMP2 = vpMatches1[i];
        if (pMP1) {
            valid[i] = 1; bad[i] = pMP1->isBad() ? 1 : 0;
            const auto X1 = pMP1->GetWorldPos();
            for (int k = 0; k < 3; ++k) world[3 * (size_t)i + k] = X1.template at<float>(k);
        }
        if (!pMP2) continue;
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (i2 < 0) { row[i] = -2; continue; }
        row[i] = i;
        valid[(size_t)cap + i] = 1; bad[(size_t)cap + i] = pMP2->isBad() ? 1 : 0;
        std::memcpy(&kps[(size_t)cap + i], olf_detail::keypoints(pKF2->mvKeysUn) + i2, sizeof(olf_keypoint));
        const auto X2 = pMP2->GetWorldPos();
        for (int k = 0; k < 3; ++k) world[3 * ((size_t)cap + i) + k] = X2.template at<float>(k);
    }
    float T[32];
    olf_detail::mat4(pKF1->GetPose(), T);
    olf_detail::mat4(pKF2->GetPose(), T + 16);
    const int32_t counts[2] = {N, N}, pair[2] = {0, 1};
    olf_track_batch in;
    std::memset(&in, 0, sizeof in);
    in.kps = kps.data(); in.counts = counts; in.img_stride = 1; in.Tcw = T; in.mp_world = world.data(); in.mp_valid = valid.data();
    in.fx = pKF1->fx; in.fy = pKF1->fy; in.cx = pKF1->cx; in.cy = pKF1->cy;
    const double qx = g2oS12.rotation().x(), qy = g2oS12.rotation().y(), qz = g2oS12.rotation().z(), qw = g2oS12.rotation().w();
    const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;                                                 // Quaterniond::toRotationMatrix
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    const float R12[9] = {(float)(1.0 - (tyy + tzz)), (float)(txy - twz), (float)(txz + twy), (float)(txy + twz), (float)(1.0 - (txx + tzz)), (float)(tyz - twx),
                          (float)(txz - twy), (float)(tyz + twx), (float)(1.0 - (txx + tyy))};
    const float t12[3] = {(float)g2oS12.translation()[0], (float)g2oS12.translation()[1], (float)g2oS12.translation()[2]}, s12 = (float)g2oS12.scale();
    double S[8];
    float so, Ro[9], to[3], Scw[16];
    int32_t nin = 0, ncorr = 0, nbad = 0, iters[2] = {0, 0}, st = 0;
    const olf_optimize_sim3_io io = {row.data(), S, &so, Ro, to, Scw, &nin, &ncorr, &nbad, iters, &st, chi2.data()};
    if (c) olf_detail::check(olf_optimize_sim3_pairs(c, &in, 2, bad.data(), 1, pair, &s12, R12, t12, th2, bFixScale ? 1 : 0, nullptr, &io), "olf_optimize_sim3_pairs");
    else olf_detail::check(olf_optimize_sim3(&in, cap, 2, bad.data(), pKF1->mvInvLevelSigma2.data(), (int)pKF1->mvInvLevelSigma2.size(), 0, 1, s12, R12, t12, th2,
                                             bFixScale ? 1 : 0, &io), "olf_optimize_sim3");
    for (int i = 0; i < N; ++i) if (vpMatches1[i] && row[i] == -1) vpMatches1[i] = nullptr;
    if (status) *status = st;
    if ((st & 3) || ncorr - nbad < 10) return 0;                    // :2178-2179 returns before g2oS12 is written; a stopped pair leaves it alone
    g2oS12 = Sim3T(QuatT(S[3], S[0], S[1], S[2]), VecT(S[4], S[5], S[6]), S[7]);
    return nin;
}

// ---- Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) over the reference's own types ---------------------------------------------------------------------
// The reference's members with its signatures: the constructor (pKF1, pKF2, vpMatched12, bFixScale), SetRansacParameters, iterate, find and the three
// GetEstimated*.  It runs over the host form olf_sim3_solver, so a single solver needs no device.  The constructor keeps the correspondences as :62-103 does,
// with the real pMP->GetIndexInKeyFrame(pKF) values; the C entry's per-feature model (indexKF1 = i1) is met by laying the kept correspondences out as the
// features 0 .. N - 1 of two frames of their own.  Reads GetMapPointMatches(), GetPose(), mvKeysUn, mvScaleFactors (mvLevelSigma2 = their squares) and fx,
// fy, cx, cy of the key frames, isBad(), GetWorldPos() and GetIndexInKeyFrame() of the points.  The random stream: the reference draws from
// the global rand() iteration by iteration; here SetRansacParameters draws all max_iterations x 3 values with rand() at once, and an iteration reads its own.
template <class KeyFrameT, class MapPointT>
class Sim3SolverOf {
public:
    typedef decltype(std::declval<KeyFrameT>().GetPose()) MatT;

    Sim3SolverOf(KeyFrameT* pKF1, KeyFrameT* pKF2, const std::vector<MapPointT*>& vpMatched12, const bool bFixScale = true)
        : mpKF1(pKF1), mpKF2(pKF2), mN1((int)vpMatched12.size()), mbFixScale(bFixScale)
    {
        const std::vector<MapPointT*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        std::vector<float> w1, w2;
        for (int i1 = 0; i1 < mN1; i1++) {
            if (!vpMatched12[i1]) continue;
            MapPointT* pMP1 = i1 < (int)vpKeyFrameMP1.size() ? vpKeyFrameMP1[i1] : nullptr;
            MapPointT* pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1), indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            olf_keypoint k1, k2;
            std::memcpy(&k1, olf_detail::keypoints(pKF1->mvKeysUn) + indexKF1, sizeof k1);
            std::memcpy(&k2, olf_detail::keypoints(pKF2->mvKeysUn) + indexKF2, sizeof k2);
            mKeys1.push_back(k1); mKeys2.push_back(k2);
            const auto X1 = pMP1->GetWorldPos(), X2 = pMP2->GetWorldPos();
            for (int k = 0; k < 3; ++k) { w1.push_back(X1.template at<float>(k)); w2.push_back(X2.template at<float>(k)); }
            mvnIndices1.push_back(i1);
        }
        N = (int)mvnIndices1.size();
        mCap = std::max(N, 1);
        mKeys.assign(2 * (size_t)mCap, olf_keypoint());
        mWorld.assign(6 * (size_t)mCap, 0.0f);
        mRow.assign(mCap, -1);
        for (int q = 0; q < N; ++q) {
            mKeys[q] = mKeys1[q]; mKeys[(size_t)mCap + q] = mKeys2[q]; mRow[q] = q;
            for (int k = 0; k < 3; ++k) { mWorld[3 * (size_t)q + k] = w1[3 * (size_t)q + k]; mWorld[3 * ((size_t)mCap + q) + k] = w2[3 * (size_t)q + k]; }
        }
        olf_detail::mat4(pKF1->GetPose(), mT);
        olf_detail::mat4(pKF2->GetPose(), mT + 16);
        for (size_t l = 0; l < pKF1->mvScaleFactors.size(); ++l) mSf.push_back(pKF1->mvScaleFactors[l]);
        mInliers.assign(mCap, 0);
        std::memset(mBestR, 0, sizeof mBestR); std::memset(mBestt, 0, sizeof mBestt); std::memset(mBestT12, 0, sizeof mBestT12);
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mRansac.fix_scale = mbFixScale ? 1 : 0; mRansac.probability = probability; mRansac.min_inliers = minInliers; mRansac.max_iterations = maxIterations;
        mRansac.n_iterations = 0;
        mnIterations = 0;                                            // (:137; mnBestInliers is the constructor's, as in the reference)
        mDraws.resize(3 * (size_t)std::max(maxIterations, 0));
        for (size_t k = 0; k < mDraws.size(); ++k) mDraws[k] = (uint32_t)rand() & 0x7fffffffu;
    }

    MatT iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        olf_track_batch in;
        const int32_t counts[2] = {N, N};
        olf_fill_batch(in, counts);
        mRansac.n_iterations = std::max(nIterations, 0);
        int32_t status = 0;
        const olf_sim3_solver_io io = olf_io();
        olf_detail::check(olf_sim3_solver(&in, mCap, 2, nullptr, mSf.data(), (int)mSf.size(), 0, 1, mRow.data(), &mRansac, mDraws.data(), &io, &status), "olf_sim3_solver");
        return olf_results(bNoMore, vbInliers, nInliers);
    }

    MatT find(std::vector<bool>& vbInliers12, int& nInliers)
    {
        bool bFlag;
        return iterate(mRansac.max_iterations, bFlag, vbInliers12, nInliers);
    }

    MatT GetEstimatedRotation()
    {
        MatT R = mpKF1->GetRotation();                               // (a clone: a 3 x 3 CV_32F matrix to fill)
        for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) R.template at<float>(r, k) = mBestR[3 * r + k];
        return R;
    }
    MatT GetEstimatedTranslation()
    {
        MatT t = mpKF1->GetTranslation();                            // (a clone: 3 x 1 CV_32F)
        for (int r = 0; r < 3; ++r) t.template at<float>(r) = mBestt[r];
        return t;
    }
    float GetEstimatedScale() { return mBests; }

    // ---- what the batched free function below reads and writes (olf_ prefix: not members of the reference's class)
    void olf_fill_batch(olf_track_batch& in, const int32_t* counts) const
    {
        std::memset(&in, 0, sizeof in);
        in.kps = mKeys.data(); in.counts = counts; in.img_stride = 1; in.Tcw = mT; in.mp_world = mWorld.data();
        in.fx = mpKF1->fx; in.fy = mpKF1->fy; in.cx = mpKF1->cx; in.cy = mpKF1->cy;
    }
    olf_sim3_solver_io olf_io()
    {
        const olf_sim3_solver_io io = {&mnIterations, &mnBestInliers, &mBests, mBestR, mBestt, mBestT12, &mAccepted, &mNoMore, &mnInliers, mInliers.data(), &mNCorr, nullptr};
        return io;
    }
    MatT olf_results(bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        bNoMore = mNoMore != 0;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = mAccepted ? mnInliers : 0;
        if (!mAccepted) return MatT();
        for (int q = 0; q < N; ++q) if (mInliers[q]) vbInliers[mvnIndices1[q]] = true;
        MatT T = mpKF1->GetPose();                                   // (a clone: 4 x 4 CV_32F)
        for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) T.template at<float>(r, k) = mBestT12[4 * r + k];
        return T;
    }

    KeyFrameT *mpKF1, *mpKF2;
    int mN1, N = 0, mCap = 1;
    bool mbFixScale;
    olf_sim3_ransac mRansac;
    std::vector<int> mvnIndices1;
    std::vector<olf_keypoint> mKeys1, mKeys2, mKeys;                 // the kept correspondences' key points; both frames at the row length mCap
    std::vector<float> mWorld, mSf;
    std::vector<int32_t> mRow;
    std::vector<uint32_t> mDraws;
    std::vector<uint8_t> mInliers;
    float mT[32];
    int32_t mnIterations = 0, mnBestInliers = 0, mAccepted = 0, mNoMore = 0, mnInliers = 0, mNCorr = 0;
    float mBests = 0.0f, mBestR[9], mBestt[3], mBestT12[16];
};

// One round of LoopClosing::ComputeSim3's loop (src/LoopClosing.cc:286-307) for a vector of candidates: iterate(nIterations, ...) of every solver in one call
// of the device entry (olf_sim3_solver_pairs through context c, whose capacity must hold every solver's correspondences and whose level table must be the
// key frames').  The solvers share their RANSAC parameters, calibration and levels (one ComputeSim3 sets them alike).  Every solver's state advances as its own iterate would
// advance it; vScm[i] is empty unless solver i accepted.
template <class KeyFrameT, class MapPointT>
void Sim3SolversIterate(olf_ctx* c, const std::vector<Sim3SolverOf<KeyFrameT, MapPointT>*>& vpSolvers, int nIterations, std::vector<bool>& vbNoMore,
                        std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers,
                        std::vector<typename Sim3SolverOf<KeyFrameT, MapPointT>::MatT>& vScm)
{
    const size_t n = vpSolvers.size();
    vbNoMore.assign(n, false); vvbInliers.assign(n, std::vector<bool>()); vnInliers.assign(n, 0); vScm.assign(n, typename Sim3SolverOf<KeyFrameT, MapPointT>::MatT());
    if (!n) return;
    const size_t cap = (size_t)olf_orb_capacity(c), mi = (size_t)vpSolvers[0]->mRansac.max_iterations;
    std::vector<olf_keypoint> kps(2 * n * cap);
    std::vector<float> world(6 * n * cap, 0.0f), T(32 * n), s(n), R(9 * n), t(3 * n), T12(16 * n);
    std::vector<int32_t> counts(2 * n), pairs(2 * n), rows(n * cap, -1), done(n), best(n), acc(n), nomore(n), ninl(n), ncorr(n);
    std::vector<uint32_t> draws(3 * n * mi);
    std::vector<uint8_t> inl(n * cap, 0);
    for (size_t i = 0; i < n; ++i) {
        const auto& S = *vpSolvers[i];
        const olf_sim3_ransac &a = S.mRansac, &b = vpSolvers[0]->mRansac;
        if ((size_t)S.N > cap) throw std::runtime_error("Sim3SolversIterate: the context's capacity does not hold a solver's correspondences");
        if (a.fix_scale != b.fix_scale || a.probability != b.probability || a.min_inliers != b.min_inliers || a.max_iterations != b.max_iterations)
            throw std::runtime_error("Sim3SolversIterate: the solvers differ in their RANSAC parameters");
        for (int f = 0; f < 2; ++f) {
            counts[2 * i + f] = S.N; pairs[2 * i + f] = (int32_t)(2 * i + f);
            std::memcpy(&T[16 * (2 * i + f)], S.mT + 16 * f, 64);
            for (int q = 0; q < S.N; ++q) {
                kps[(2 * i + f) * cap + q] = S.mKeys[(size_t)f * S.mCap + q];
                for (int k = 0; k < 3; ++k) world[3 * ((2 * i + f) * cap + q) + k] = S.mWorld[3 * ((size_t)f * S.mCap + q) + k];
            }
        }
        for (int q = 0; q < S.N; ++q) rows[i * cap + q] = q;
        std::memcpy(&draws[3 * i * mi], S.mDraws.data(), 12 * mi);
        done[i] = S.mnIterations; best[i] = S.mnBestInliers; s[i] = S.mBests;
        std::memcpy(&R[9 * i], S.mBestR, 36); std::memcpy(&t[3 * i], S.mBestt, 12); std::memcpy(&T12[16 * i], S.mBestT12, 64);
    }
    olf_track_batch in;
    vpSolvers[0]->olf_fill_batch(in, counts.data());
    in.kps = kps.data(); in.Tcw = T.data(); in.mp_world = world.data();
    olf_sim3_ransac rn = vpSolvers[0]->mRansac;
    rn.n_iterations = std::max(nIterations, 0);
    const olf_sim3_solver_io io = {done.data(), best.data(), s.data(), R.data(), t.data(), T12.data(), acc.data(), nomore.data(), ninl.data(), inl.data(), ncorr.data(), nullptr};
    olf_detail::check(olf_sim3_solver_pairs(c, &in, (int)(2 * n), nullptr, (int)n, pairs.data(), rows.data(), &rn, draws.data(), &io), "olf_sim3_solver_pairs");
    for (size_t i = 0; i < n; ++i) {
        auto& S = *vpSolvers[i];
        S.mnIterations = done[i]; S.mnBestInliers = best[i]; S.mBests = s[i]; S.mAccepted = acc[i]; S.mNoMore = nomore[i]; S.mnInliers = ninl[i]; S.mNCorr = ncorr[i];
        std::memcpy(S.mBestR, &R[9 * i], 36); std::memcpy(S.mBestt, &t[3 * i], 12); std::memcpy(S.mBestT12, &T12[16 * i], 64);
        for (int q = 0; q < S.N; ++q) S.mInliers[q] = inl[i * cap + q];
        bool nm;
        int ni;
        vScm[i] = S.olf_results(nm, vvbInliers[i], ni);
        vbNoMore[i] = nm; vnInliers[i] = ni;
    }
}

// ---- PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) over the reference's own types ------------------------------------------------------------------------
// The reference's members with its signatures: the constructor (F, vpMapPointMatches), SetRansacParameters, iterate and find.  It runs over the host form
// olf_pnp_solver, so a single solver needs no device.  The constructor keeps the correspondences as :79-101 does; the C entry's per-feature model (a row
// from frame feature to key-frame feature) is met by laying the kept correspondences out as the features 0 .. N - 1 of two frames of their own: frame 0
// holds the points, frame 1 the key points.  Reads mvKeysUn, mvScaleFactors (mvLevelSigma2 = their squares) and fx, fy, cx, cy of the frame, isBad() and
// GetWorldPos() of the points.  The random stream: the reference draws from the global rand() iteration by iteration; here
// SetRansacParameters draws all max_iterations x 4 values with rand() at once, and an iteration reads its own (modulo max_iterations, C.26).
template <class FrameT, class MapPointT>
class PnPsolverOf {
public:
    typedef typename std::decay<decltype(std::declval<FrameT>().mTcw)>::type MatT;

    PnPsolverOf(const FrameT& F, const std::vector<MapPointT*>& vpMapPointMatches) : mnMatches((int)vpMapPointMatches.size())
    {
        std::vector<float> w;
        std::vector<olf_keypoint> keys;
        for (int i = 0; i < mnMatches; i++) {
            MapPointT* pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;
            olf_keypoint k;
            std::memcpy(&k, olf_detail::keypoints(F.mvKeysUn) + i, sizeof k);
            keys.push_back(k);
            const auto X = pMP->GetWorldPos();
            for (int c = 0; c < 3; ++c) w.push_back(X.template at<float>(c));
            mvKeyPointIndices.push_back(i);
        }
        N = (int)mvKeyPointIndices.size();
        mCap = std::max(N, 1);
        mKeys.assign(2 * (size_t)mCap, olf_keypoint());
        mWorld.assign(6 * (size_t)mCap, 0.0f);
        mRow.assign(mCap, -1);
        for (int q = 0; q < N; ++q) {
            mKeys[(size_t)mCap + q] = keys[q]; mRow[q] = q;
            for (int c = 0; c < 3; ++c) mWorld[3 * (size_t)q + c] = w[3 * (size_t)q + c];
        }
        for (size_t l = 0; l < F.mvScaleFactors.size(); ++l) mSf.push_back(F.mvScaleFactors[l]);
        fx = F.fx; fy = F.fy; cx = F.cx; cy = F.cy;
        mBestFlags.assign(mCap, 0); mRefinedFlags.assign(mCap, 0); mInliers.assign(mCap, 0);
        std::memset(mBestTcw, 0, sizeof mBestTcw); std::memset(mRefinedTcw, 0, sizeof mRefinedTcw); std::memset(mTcw, 0, sizeof mTcw);
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4, float th2 = 5.991)
    {
        mRansac.probability = probability; mRansac.min_inliers = minInliers; mRansac.max_iterations = maxIterations; mRansac.min_set = minSet;
        mRansac.n_iterations = 0; mRansac.epsilon = epsilon; mRansac.th2 = th2;
        mDraws.resize(4 * (size_t)std::max(maxIterations, 0));
        for (size_t k = 0; k < mDraws.size(); ++k) mDraws[k] = (uint32_t)rand() & 0x7fffffffu;
    }

    MatT iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        olf_track_batch in;
        const int32_t counts[2] = {N, N};
        olf_fill_batch(in, counts);
        mRansac.n_iterations = std::max(nIterations, 0);
        int32_t status = 0;
        const olf_pnp_solver_io io = olf_io();
        olf_detail::check(olf_pnp_solver(&in, mCap, 2, nullptr, mSf.data(), (int)mSf.size(), 0, 1, mRow.data(), &mRansac, mDraws.data(), &io, &status), "olf_pnp_solver");
        return olf_results(bNoMore, vbInliers, nInliers);
    }

    MatT find(std::vector<bool>& vbInliers, int& nInliers)            // iterate(mRansacMaxIts, ...) with the cap SetRansacParameters adjusted to N (:159-163)
    {
        bool bFlag;
        int32_t m = 0, cap = 1;
        olf_detail::check(olf_debug_pnp_solver_parameters(N, &mRansac, &m, &cap), "olf_debug_pnp_solver_parameters");
        return iterate(cap, bFlag, vbInliers, nInliers);
    }

    // ---- what the batched free function below reads and writes (olf_ prefix: not members of the reference's class)
    void olf_fill_batch(olf_track_batch& in, const int32_t* counts) const
    {
        std::memset(&in, 0, sizeof in);
        in.kps = mKeys.data(); in.counts = counts; in.img_stride = 1; in.mp_world = mWorld.data();
        in.fx = fx; in.fy = fy; in.cx = cx; in.cy = cy;
    }
    olf_pnp_solver_io olf_io()
    {
        const olf_pnp_solver_io io = {&mnIterations, &mnBestInliers, mBestTcw, mBestFlags.data(), &mnRefinedInliers, mRefinedTcw, mRefinedFlags.data(), &mAccepted,
                                      &mNoMore, &mnInliers, mInliers.data(), mTcw, &mNCorr, nullptr};
        return io;
    }
    MatT olf_results(bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        bNoMore = mNoMore != 0;
        vbInliers.clear();
        nInliers = mAccepted ? mnInliers : 0;
        if (!mAccepted) return MatT();
        vbInliers = std::vector<bool>(mnMatches, false);
        for (int q = 0; q < N; ++q) if (mInliers[q]) vbInliers[mvKeyPointIndices[q]] = true;
        MatT T(4, 4, 5 /* CV_32F */);
        for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) T.template at<float>(r, k) = mTcw[4 * r + k];
        return T;
    }

    int mnMatches, N = 0, mCap = 1;
    float fx, fy, cx, cy;
    olf_pnp_ransac mRansac;
    std::vector<int> mvKeyPointIndices;
    std::vector<olf_keypoint> mKeys;                                 // both frames at the row length mCap: frame 1 holds the kept key points
    std::vector<float> mWorld, mSf;                                  // frame 0 holds the kept points
    std::vector<int32_t> mRow;
    std::vector<uint32_t> mDraws;
    std::vector<uint8_t> mBestFlags, mRefinedFlags, mInliers;
    int32_t mnIterations = 0, mnBestInliers = 0, mnRefinedInliers = 0, mAccepted = 0, mNoMore = 0, mnInliers = 0, mNCorr = 0;
    float mBestTcw[16], mRefinedTcw[16], mTcw[16];
};

// One round of Tracking::Relocalization's loop (src/Tracking.cc:2267-2308) for a vector of candidates: iterate(nIterations, ...) of every solver in one call
// of the device entry (olf_pnp_solver_pairs through context c, whose capacity must hold every solver's correspondences and whose level table must be the
// frame's).  The solvers share their RANSAC parameters, calibration and levels (one Relocalization sets them alike).  Every solver's state advances as its
// own iterate would advance it; vTcw[i] is empty unless solver i returned a pose.
template <class FrameT, class MapPointT>
void PnPsolversIterate(olf_ctx* c, const std::vector<PnPsolverOf<FrameT, MapPointT>*>& vpSolvers, int nIterations, std::vector<bool>& vbNoMore,
                       std::vector<std::vector<bool> >& vvbInliers, std::vector<int>& vnInliers,
                       std::vector<typename PnPsolverOf<FrameT, MapPointT>::MatT>& vTcw)
{
    const size_t n = vpSolvers.size();
    vbNoMore.assign(n, false); vvbInliers.assign(n, std::vector<bool>()); vnInliers.assign(n, 0); vTcw.assign(n, typename PnPsolverOf<FrameT, MapPointT>::MatT());
    if (!n) return;
    const size_t cap = (size_t)olf_orb_capacity(c), mi = (size_t)vpSolvers[0]->mRansac.max_iterations;
    std::vector<olf_keypoint> kps(2 * n * cap);
    std::vector<float> world(6 * n * cap, 0.0f), bT(16 * n), rT(16 * n), T(16 * n);
    std::vector<int32_t> counts(2 * n), pairs(2 * n), rows(n * cap, -1), done(n), best(n), ref(n), acc(n), nomore(n), ninl(n), ncorr(n);
    std::vector<uint32_t> draws(4 * n * mi);
    std::vector<uint8_t> bf(n * cap, 0), rf(n * cap, 0), inl(n * cap, 0);
    for (size_t i = 0; i < n; ++i) {
        const auto& S = *vpSolvers[i];
        const olf_pnp_ransac &a = S.mRansac, &b = vpSolvers[0]->mRansac;
        if ((size_t)S.N > cap) throw std::runtime_error("PnPsolversIterate: the context's capacity does not hold a solver's correspondences");
        if (a.probability != b.probability || a.min_inliers != b.min_inliers || a.max_iterations != b.max_iterations || a.min_set != b.min_set ||
            a.epsilon != b.epsilon || a.th2 != b.th2)
            throw std::runtime_error("PnPsolversIterate: the solvers differ in their RANSAC parameters");
        for (int f = 0; f < 2; ++f) { counts[2 * i + f] = S.N; pairs[2 * i + f] = (int32_t)(2 * i + f); }
        for (int q = 0; q < S.N; ++q) {
            kps[(2 * i + 1) * cap + q] = S.mKeys[(size_t)S.mCap + q];
            for (int k = 0; k < 3; ++k) world[3 * (2 * i * cap + q) + k] = S.mWorld[3 * (size_t)q + k];
            rows[i * cap + q] = q;
            bf[i * cap + q] = S.mBestFlags[q]; rf[i * cap + q] = S.mRefinedFlags[q];
        }
        std::memcpy(&draws[4 * i * mi], S.mDraws.data(), 16 * mi);
        done[i] = S.mnIterations; best[i] = S.mnBestInliers; ref[i] = S.mnRefinedInliers;
        std::memcpy(&bT[16 * i], S.mBestTcw, 64); std::memcpy(&rT[16 * i], S.mRefinedTcw, 64); std::memcpy(&T[16 * i], S.mTcw, 64);
    }
    olf_track_batch in;
    vpSolvers[0]->olf_fill_batch(in, counts.data());
    in.kps = kps.data(); in.mp_world = world.data();
    olf_pnp_ransac rn = vpSolvers[0]->mRansac;
    rn.n_iterations = std::max(nIterations, 0);
    const olf_pnp_solver_io io = {done.data(), best.data(), bT.data(), bf.data(), ref.data(), rT.data(), rf.data(), acc.data(), nomore.data(), ninl.data(), inl.data(),
                                  T.data(), ncorr.data(), nullptr};
    olf_detail::check(olf_pnp_solver_pairs(c, &in, (int)(2 * n), nullptr, (int)n, pairs.data(), rows.data(), &rn, draws.data(), &io), "olf_pnp_solver_pairs");
    for (size_t i = 0; i < n; ++i) {
        auto& S = *vpSolvers[i];
        S.mnIterations = done[i]; S.mnBestInliers = best[i]; S.mnRefinedInliers = ref[i]; S.mAccepted = acc[i]; S.mNoMore = nomore[i]; S.mnInliers = ninl[i];
        S.mNCorr = ncorr[i];
        std::memcpy(S.mBestTcw, &bT[16 * i], 64); std::memcpy(S.mRefinedTcw, &rT[16 * i], 64); std::memcpy(S.mTcw, &T[16 * i], 64);
        for (int q = 0; q < S.N; ++q) { S.mBestFlags[q] = bf[i * cap + q]; S.mRefinedFlags[q] = rf[i * cap + q]; S.mInliers[q] = inl[i * cap + q]; }
        bool nm;
        int ni;
        vTcw[i] = S.olf_results(nm, vvbInliers[i], ni);
        vbNoMore[i] = nm; vnInliers[i] = ni;
    }
}

// ---- Initializer (include/Initializer.h, src/Initializer.cc) over the reference's own types ---------------------------------------------------------------
// The reference's members with its signatures: the constructor (ReferenceFrame, sigma, iterations) and Initialize.  It runs over the host form
// olf_initializer, so a single initialiser needs no device.  Reads mK and mvKeysUn of both frames.  The two frames are laid out as frames 0 and 1 of a
// batch of their own, at a row length that holds both; vMatches12 is the row as it is.  The random stream: srand(0) once per process
// (DUtils::Random::SeedRandOnce(0), :80), then every Initialize call draws its max_iterations x 8 values with rand() in the reference's order (:82-97).
// The library stores and compares cosines (C.34): olf_parallax() turns the stored cosine of a hypothesis into CheckRT's degrees, on the host.
namespace olf_detail {
inline void seed_rand_once(unsigned seed) { static bool seeded = false; if (!seeded) { srand(seed); seeded = true; } }
}
template <class FrameT>
class InitializerOf {
public:
    InitializerOf(const FrameT& ReferenceFrame, float sigma = 1.0, int iterations = 200)
    {
        fx = ReferenceFrame.mK.template at<float>(0, 0); fy = ReferenceFrame.mK.template at<float>(1, 1);
        cx = ReferenceFrame.mK.template at<float>(0, 2); cy = ReferenceFrame.mK.template at<float>(1, 2);
        olf_copy_keys(ReferenceFrame, mKeys1);
        mParams.sigma = sigma; mParams.max_iterations = iterations; mParams.min_parallax = 1.0f; mParams.min_triangulated = 50;      // :116-118
    }

    template <class MatT, class Point3fT>
    bool Initialize(const FrameT& CurrentFrame, const std::vector<int>& vMatches12, MatT& R21, MatT& t21, std::vector<Point3fT>& vP3D,
                    std::vector<bool>& vbTriangulated)
    {
        olf_prepare(CurrentFrame, vMatches12);
        const size_t cap = mCap;
        std::vector<olf_keypoint> kps(2 * cap);
        std::copy(mKeys1.begin(), mKeys1.end(), kps.begin());
        std::copy(mKeys2.begin(), mKeys2.end(), kps.begin() + cap);
        const int32_t counts[2] = {(int32_t)mKeys1.size(), (int32_t)mKeys2.size()};
        olf_track_batch in;
        olf_fill_batch(in, counts);
        in.kps = kps.data();
        olf_resize(cap);
        const olf_initializer_io io = olf_io(0);
        int32_t status = 0;
        olf_detail::check(olf_initializer(&in, (int)cap, 2, 0, 1, mRow.data(), &mParams, mDraws.data(), &io, &status), "olf_initializer");
        return olf_results(R21, t21, vP3D, vbTriangulated);
    }

    // CheckRT's parallax of hypothesis h in degrees (:901), from the stored cosine
    float olf_parallax(int h) const { return mnGood[h] > 0 ? (float)((double)(std::acos(mCos[h]) * 180.0f) / 3.1415926535897932384626433832795) : 0.0f; }

    // ---- what the batched free function below reads and writes (olf_ prefix: not members of the reference's class)
    static void olf_copy_keys(const FrameT& F, std::vector<olf_keypoint>& keys)
    {
        keys.resize(F.mvKeysUn.size());
        if (!keys.empty()) std::memcpy(keys.data(), olf_detail::keypoints(F.mvKeysUn), keys.size() * sizeof(olf_keypoint));
    }
    void olf_prepare(const FrameT& CurrentFrame, const std::vector<int>& vMatches12)
    {
        olf_copy_keys(CurrentFrame, mKeys2);
        mCap = std::max<size_t>(std::max(mKeys1.size(), mKeys2.size()), 1);
        mRow.assign(mCap, -1);
        for (size_t i = 0; i < vMatches12.size() && i < mKeys1.size(); ++i) mRow[i] = vMatches12[i];
        olf_detail::seed_rand_once(0);
        mDraws.resize(8 * (size_t)std::max(mParams.max_iterations, 0));
        for (size_t k = 0; k < mDraws.size(); ++k) mDraws[k] = (uint32_t)rand() & 0x7fffffffu;
    }
    void olf_fill_batch(olf_track_batch& in, const int32_t* counts) const
    {
        std::memset(&in, 0, sizeof in);
        in.counts = counts; in.img_stride = 1;
        in.fx = fx; in.fy = fy; in.cx = cx; in.cy = cy;
    }
    void olf_resize(size_t cap) { mInlH.assign(cap, 0); mInlF.assign(cap, 0); mTri.assign(cap, 0); mP3D.assign(3 * cap, 0.0f); }
    olf_initializer_io olf_io(size_t)
    {
        const olf_initializer_io io = {&mOk, &mNCorr, &mModel, &mScoreH, &mScoreF, mH21, mF21, mInlH.data(), mInlF.data(), mR21, mt21, mP3D.data(), mTri.data(),
                                       mnGood, mCos, &mHypothesis};
        return io;
    }
    template <class MatT, class Point3fT>
    bool olf_results(MatT& R21, MatT& t21, std::vector<Point3fT>& vP3D, std::vector<bool>& vbTriangulated)
    {
        if (mModel == 2) { R21 = MatT(); t21 = MatT(); }           // ReconstructF empties both before it decides (:501-502)
        if (mOk <= 0) return false;
        R21 = MatT(3, 3, 5 /* CV_32F */); t21 = MatT(3, 1, 5);
        for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) R21.template at<float>(r, k) = mR21[3 * r + k]; t21.template at<float>(r) = mt21[r]; }
        const size_t N1 = mKeys1.size();
        vP3D.resize(N1);
        vbTriangulated = std::vector<bool>(N1, false);
        for (size_t i = 0; i < N1; ++i) { vP3D[i] = Point3fT(mP3D[3 * i], mP3D[3 * i + 1], mP3D[3 * i + 2]); vbTriangulated[i] = mTri[i] != 0; }
        return true;
    }

    float fx, fy, cx, cy;
    olf_initializer_params mParams;
    size_t mCap = 1;
    std::vector<olf_keypoint> mKeys1, mKeys2;
    std::vector<int32_t> mRow;
    std::vector<uint32_t> mDraws;
    std::vector<uint8_t> mInlH, mInlF, mTri;
    std::vector<float> mP3D;
    int32_t mOk = 0, mNCorr = 0, mModel = 0, mHypothesis = -1, mnGood[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float mScoreH = 0, mScoreF = 0, mH21[9], mF21[9], mR21[9], mt21[3], mCos[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// Initialize of every initialiser against its current frame in one call of the device entry (olf_initializer_pairs through context c, whose capacity must
// hold every frame's key points).  The initialisers share sigma, the iteration count and the calibration.  Every initialiser draws as its own Initialize
// would, in the order of the vector; vbOk[i] is the return value and the other outputs are what Initialize would have left.
template <class FrameT, class MatT, class Point3fT>
void InitializersInitialize(olf_ctx* c, const std::vector<InitializerOf<FrameT>*>& vpInitializers, const std::vector<const FrameT*>& vpCurrentFrames,
                            const std::vector<std::vector<int> >& vvMatches12, std::vector<bool>& vbOk, std::vector<MatT>& vR21, std::vector<MatT>& vt21,
                            std::vector<std::vector<Point3fT> >& vvP3D, std::vector<std::vector<bool> >& vvbTriangulated)
{
    const size_t n = vpInitializers.size();
    vbOk.assign(n, false); vR21.assign(n, MatT()); vt21.assign(n, MatT()); vvP3D.assign(n, std::vector<Point3fT>()); vvbTriangulated.assign(n, std::vector<bool>());
    if (!n) return;
    if (vpCurrentFrames.size() != n || vvMatches12.size() != n) throw std::runtime_error("InitializersInitialize: one current frame and one row per initialiser");
    const size_t cap = (size_t)olf_orb_capacity(c), mi = (size_t)vpInitializers[0]->mParams.max_iterations;
    std::vector<olf_keypoint> kps(2 * n * cap);
    std::vector<int32_t> counts(2 * n), pairs(2 * n), rows(n * cap, -1), ok(n), nc(n), model(n), ng(8 * n), hyp(n);
    std::vector<uint32_t> draws(8 * n * mi);
    std::vector<float> sh(n), sf(n), H(9 * n), F(9 * n), R(9 * n), t(3 * n), P(3 * n * cap, 0.0f), cs(8 * n);
    std::vector<uint8_t> iH(n * cap, 0), iF(n * cap, 0), tri(n * cap, 0);
    for (size_t i = 0; i < n; ++i) {
        auto& S = *vpInitializers[i];
        const olf_initializer_params &a = S.mParams, &b = vpInitializers[0]->mParams;
        if (a.sigma != b.sigma || a.max_iterations != b.max_iterations || a.min_parallax != b.min_parallax || a.min_triangulated != b.min_triangulated ||
            S.fx != vpInitializers[0]->fx || S.fy != vpInitializers[0]->fy || S.cx != vpInitializers[0]->cx || S.cy != vpInitializers[0]->cy)
            throw std::runtime_error("InitializersInitialize: the initialisers differ in their parameters or calibration");
        S.olf_prepare(*vpCurrentFrames[i], vvMatches12[i]);
        if (S.mCap > cap) throw std::runtime_error("InitializersInitialize: the context's capacity does not hold a frame's key points");
        std::copy(S.mKeys1.begin(), S.mKeys1.end(), kps.begin() + 2 * i * cap);
        std::copy(S.mKeys2.begin(), S.mKeys2.end(), kps.begin() + (2 * i + 1) * cap);
        counts[2 * i] = (int32_t)S.mKeys1.size(); counts[2 * i + 1] = (int32_t)S.mKeys2.size();
        pairs[2 * i] = (int32_t)(2 * i); pairs[2 * i + 1] = (int32_t)(2 * i + 1);
        std::copy(S.mRow.begin(), S.mRow.end(), rows.begin() + i * cap);
        std::memcpy(&draws[8 * i * mi], S.mDraws.data(), 32 * mi);
    }
    olf_track_batch in;
    vpInitializers[0]->olf_fill_batch(in, counts.data());
    in.kps = kps.data();
    const olf_initializer_io io = {ok.data(), nc.data(), model.data(), sh.data(), sf.data(), H.data(), F.data(), iH.data(), iF.data(), R.data(), t.data(), P.data(),
                                   tri.data(), ng.data(), cs.data(), hyp.data()};
    olf_detail::check(olf_initializer_pairs(c, &in, (int)(2 * n), (int)n, pairs.data(), rows.data(), &vpInitializers[0]->mParams, draws.data(), &io),
                      "olf_initializer_pairs");
    for (size_t i = 0; i < n; ++i) {
        auto& S = *vpInitializers[i];
        const size_t N1 = S.mKeys1.size();
        S.olf_resize(S.mCap);
        S.mOk = ok[i]; S.mNCorr = nc[i]; S.mModel = model[i]; S.mHypothesis = hyp[i]; S.mScoreH = sh[i]; S.mScoreF = sf[i];
        std::memcpy(S.mH21, &H[9 * i], 36); std::memcpy(S.mF21, &F[9 * i], 36); std::memcpy(S.mR21, &R[9 * i], 36); std::memcpy(S.mt21, &t[3 * i], 12);
        std::memcpy(S.mnGood, &ng[8 * i], 32); std::memcpy(S.mCos, &cs[8 * i], 32);
        for (size_t q = 0; q < N1; ++q) {
            S.mInlH[q] = iH[i * cap + q]; S.mInlF[q] = iF[i * cap + q]; S.mTri[q] = tri[i * cap + q];
            for (int k = 0; k < 3; ++k) S.mP3D[3 * q + k] = P[3 * (i * cap + q) + k];
        }
        MatT R21, t21;
        vbOk[i] = S.olf_results(R21, t21, vvP3D[i], vvbTriangulated[i]);
        vR21[i] = R21; vt21[i] = t21;
    }
}

// ---- the landmark loops of Tracking::StereoInitialization, CreateNewKeyFrame and UpdateLastFrame, and Tracking::NeedNewKeyFrame, over the reference's types ----
// What the three loops decide for one frame, through the host form (olf_stereo_landmarks, no context and no device): which features are visited and which
// get a new MapPoint / MapLine, in the reference's order, with the new landmark's geometry.  Creating the objects (new MapPoint, AddObservation,
// AddMapPoint, ComputeDistinctiveDescriptors, mlpTemporalPoints.push_back) stays the caller's, in the order of `created` / `created_l`.
struct StereoLandmarks {
    int nPoints = 0, nLines = 0;                  // the final counters of the two loops
    std::vector<int> visited, created;            // feature indices in visit order; the created subset in creation order (the order of mnId)
    std::vector<int> visited_l, created_l;
    std::vector<float> world, normal;             // [3 k ..]: mWorldPos and mNormalVector of the k-th created point
    std::vector<float> maxd, mind;                // [k]: mfMaxDistance, mfMinDistance
    std::vector<double> world_l;                  // [6 k ..]: sp3D, ep3D of the k-th created line (Frame::backProjection)
    int32_t status = 0;                           // 1 a NaN line depth (no line visited), 4 an octave outside mvScaleFactors
};
namespace olf_detail {
// Reads N, N_l, mvKeysUn, mvKeysUn_Line, mvDepth, mvDisparity_l, mvpMapPoints / mvpMapLines with Observations(), mRwc, mOw, fx, fy, cx, cy, mbf and
// mvScaleFactors of the frame.
template <class FrameT>
StereoLandmarks stereo_landmarks(FrameT& F, int mode, float mThDepth)
{
    typedef typename std::remove_reference<decltype(F.mvKeysUn[0])>::type KP;
    typedef typename std::remove_reference<decltype(F.mvKeysUn_Line[0])>::type KL;
    static_assert(sizeof(KP) == sizeof(olf_keypoint) && sizeof(KL) == sizeof(olf_keyline), "cv::KeyPoint / KeyLine layout");
    const int N = (int)F.N, Nl = (int)F.N_l;
    if (N > OLF_GRID_MAX_KEYS || Nl > OLF_GRID_MAX_KEYS) check(OLF_ERR_CAPACITY, "stereo_landmarks: more than OLF_GRID_MAX_KEYS features");
    const size_t cap = (size_t)N + 1, lcap = (size_t)Nl + 1;
    std::vector<float> depth(cap, -1.f), ldisp(2 * lcap, -1.f);
    std::vector<int32_t> fmp(cap, -1), fml(lcap, -1), nobs, lnobs;
    for (int i = 0; i < N; ++i) {
        depth[i] = F.mvDepth[i];
        if (F.mvpMapPoints[i]) { fmp[i] = (int32_t)nobs.size(); nobs.push_back((int32_t)F.mvpMapPoints[i]->Observations()); }
    }
    for (int i = 0; i < Nl; ++i) {
        ldisp[2 * i] = F.mvDisparity_l[i].first; ldisp[2 * i + 1] = F.mvDisparity_l[i].second;
        if (F.mvpMapLines[i]) { fml[i] = (int32_t)lnobs.size(); lnobs.push_back((int32_t)F.mvpMapLines[i]->Observations()); }
    }
    std::vector<olf_keypoint> kps(cap);
    std::vector<olf_keyline> kls(lcap);
    if (N) std::memcpy(kps.data(), F.mvKeysUn.data(), (size_t)N * sizeof(olf_keypoint));
    if (Nl) std::memcpy(kls.data(), F.mvKeysUn_Line.data(), (size_t)Nl * sizeof(olf_keyline));
    float Twc[16] = {0};
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) Twc[4 * r + k] = F.mRwc.template at<float>(r, k); Twc[4 * r + 3] = F.mOw.template at<float>(r); }
    Twc[15] = 1.f;
    nobs.push_back(0); lnobs.push_back(0);                           // (an array without entries keeps an address)
    const int32_t counts[1] = {N}, lcounts[1] = {Nl};
    olf_landmarks_batch in;
    std::memset(&in, 0, sizeof(in));
    in.kps = kps.data(); in.counts = counts; in.kls = kls.data(); in.lcounts = lcounts; in.img_stride = 1;
    in.depth = depth.data(); in.ldisp = ldisp.data(); in.Twc = Twc; in.frame_mp = fmp.data(); in.frame_ml = fml.data();
    in.mp_nobs = nobs.data(); in.n_mp = (int32_t)nobs.size() - 1; in.ml_nobs = lnobs.data(); in.n_ml = (int32_t)lnobs.size() - 1;
    in.fx = F.fx; in.fy = F.fy; in.cx = F.cx; in.cy = F.cy; in.mbf = F.mbf; in.thDepth = mThDepth;
    int32_t nv[2], nc[2], st = 0;
    std::vector<int32_t> vo(cap), vl(lcap), co(cap), cl(lcap), fo(cap), fl(lcap);
    std::vector<uint8_t> cr(cap), crl(lcap);
    std::vector<float> w(3 * cap), nr(3 * cap), mx(cap), mn(cap), lw(6 * lcap);
    std::vector<double> lwd(6 * lcap);
    const olf_landmarks_outputs o = {nv, nc, vo.data(), vl.data(), co.data(), cl.data(), cr.data(), crl.data(), fo.data(), fl.data(), w.data(), nr.data(), mx.data(),
                                     mn.data(), lwd.data(), lw.data(), &st};
    check(olf_stereo_landmarks(&in, (int)cap, (int)lcap, 1, mode, F.mvScaleFactors.data(), (int)F.mvScaleFactors.size(), &o), "olf_stereo_landmarks");
    StereoLandmarks R;
    R.nPoints = nv[0]; R.nLines = nv[1]; R.status = st;
    for (int q = 0; q < N && vo[q] >= 0; ++q) R.visited.push_back(vo[q]);
    for (int q = 0; q < Nl && vl[q] >= 0; ++q) R.visited_l.push_back(vl[q]);
    for (int k = 0; k < nc[0]; ++k) {
        const int i = co[k];
        R.created.push_back(i);
        for (int c = 0; c < 3; ++c) { R.world.push_back(w[3 * i + c]); R.normal.push_back(nr[3 * i + c]); }
        R.maxd.push_back(mx[i]); R.mind.push_back(mn[i]);
    }
    for (int k = 0; k < nc[1]; ++k) {
        const int i = cl[k];
        R.created_l.push_back(i);
        for (int c = 0; c < 6; ++c) R.world_l.push_back(lwd[6 * i + c]);
    }
    return R;
}
}  // namespace olf_detail

// the loops `for(int i=0; i<mCurrentFrame.N;i++)` and `for(int i=0; i<mCurrentFrame.N_l; ++i)` of Tracking::StereoInitialization, src/Tracking.cc:639-677
template <class FrameT> StereoLandmarks StereoInitializationLandmarks(FrameT& mCurrentFrame) { return olf_detail::stereo_landmarks(mCurrentFrame, OLF_LANDMARKS_INIT, 0.f); }
// the two sorted loops of void Tracking::CreateNewKeyFrame(), src/Tracking.cc:1744-1865
template <class FrameT> StereoLandmarks CreateNewKeyFrameLandmarks(FrameT& mCurrentFrame, float mThDepth) { return olf_detail::stereo_landmarks(mCurrentFrame, OLF_LANDMARKS_KEYFRAME, mThDepth); }
// the two sorted loops of void Tracking::UpdateLastFrame(), src/Tracking.cc:1092-1204, with the early return of :1105-1106
template <class FrameT> StereoLandmarks UpdateLastFrameLandmarks(FrameT& mLastFrame, float mThDepth) { return olf_detail::stereo_landmarks(mLastFrame, OLF_LANDMARKS_LASTFRAME, mThDepth); }

// bool Tracking::NeedNewKeyFrame(), src/Tracking.cc:1606-1725: the tracker's members and what it asks of mpMap, mpReferenceKF and mpLocalMapper ...
struct KeyFrameTest {
    unsigned long mnId = 0;                                   // mCurrentFrame.mnId
    unsigned mnLastKeyFrameId = 0, mnLastRelocFrameId = 0;
    int mMinFrames = 0, mMaxFrames = 0;
    int nKFs = 0;                                             // mpMap->KeyFramesInMap()
    int nRefMatches = 0, nRefMatches_l = 0;                   // mpReferenceKF->TrackedMapPoints(nKFs <= 2 ? 2 : 3), TrackedMapLines(2)
    int mnMatchesInliers = 0, mnMatchesInliers_l = 0;
    bool bLocalMappingIdle = false;                           // mpLocalMapper->AcceptKeyFrames()
    int KeyframesInQueue = 0;
    bool mbOnlyTracking = false, stopped = false, monocular = false;      // stopped: isStopped() || stopRequested(); monocular: mSensor == System::MONOCULAR
};
// ... and what it answers: the return value, whether mpLocalMapper->InterruptBA() is due (:1711), the four counts of :1632-1667, the six conditions
struct KeyFrameDecision {
    bool need = false, interrupt_ba = false;
    int nTrackedClose = 0, nNonTrackedClose = 0, nTrackedClose_l = 0, nNonTrackedClose_l = 0;
    int conditions = 0;                                       // c1a | c1b << 1 | c1c << 2 | c1c_l << 3 | c2 << 4 | c2_l << 5
    int32_t status = 0;                                       // 1: mLastFrame has fewer lines than mCurrentFrame (:1651 reads out of bounds there; not counted)
};
// Reads N, N_l, mvDepth, mvpMapPoints, mvbOutlier, mvpMapLines, mvbOutlier_Line and mbf of mCurrentFrame and mvDisparity_l of mLastFrame (:1651-1652, as
// written).  Through the host form (olf_need_new_keyframe): no context, no device.
template <class FrameT>
KeyFrameDecision NeedNewKeyFrame(const FrameT& mCurrentFrame, const FrameT& mLastFrame, const KeyFrameTest& t, float mThDepth)
{
    const int N = (int)mCurrentFrame.N, Nl = (int)mCurrentFrame.N_l, Nlast = (int)mLastFrame.N_l;
    if (N > OLF_GRID_MAX_KEYS || std::max(Nl, Nlast) > OLF_GRID_MAX_KEYS) olf_detail::check(OLF_ERR_CAPACITY, "NeedNewKeyFrame: more than OLF_GRID_MAX_KEYS features");
    const size_t cap = (size_t)N + 1, lcap = (size_t)std::max(Nl, Nlast) + 1;
    std::vector<float> depth(2 * cap, -1.f), ldisp(4 * lcap, -1.f);                  // two rows: the current frame, then the last one
    std::vector<int32_t> fmp(2 * cap, -1), fml(2 * lcap, -1);
    std::vector<uint8_t> out(2 * cap, 0), out_l(2 * lcap, 0);
    for (int i = 0; i < N; ++i) { depth[i] = mCurrentFrame.mvDepth[i]; fmp[i] = mCurrentFrame.mvpMapPoints[i] ? 0 : -1; out[i] = mCurrentFrame.mvbOutlier[i] ? 1 : 0; }
    for (int i = 0; i < Nl; ++i) { fml[i] = mCurrentFrame.mvpMapLines[i] ? 0 : -1; out_l[i] = mCurrentFrame.mvbOutlier_Line[i] ? 1 : 0; }
    for (int i = 0; i < Nlast; ++i) { ldisp[2 * (lcap + i)] = mLastFrame.mvDisparity_l[i].first; ldisp[2 * (lcap + i) + 1] = mLastFrame.mvDisparity_l[i].second; }
    const int32_t counts[2] = {N, 0}, lcounts[2] = {Nl, Nlast}, ldisp_frame[2] = {1, 1}, nref[2] = {t.nRefMatches, 0}, nref_l[2] = {t.nRefMatches_l, 0};
    const int32_t ninl[4] = {t.mnMatchesInliers, t.mnMatchesInliers_l, 0, 0};
    int32_t rows[2 * OLF_KEYFRAME_ROW] = {(int32_t)(uint32_t)t.mnId, (int32_t)t.mnLastKeyFrameId, (int32_t)t.mnLastRelocFrameId, t.mMinFrames, t.mMaxFrames, t.nKFs,
                                          t.bLocalMappingIdle, t.KeyframesInQueue, t.mbOnlyTracking, t.stopped, t.monocular};
    rows[OLF_KEYFRAME_ROW + 8] = 1;                                  // (the second row is not asked anything: mbOnlyTracking)
    olf_keyframe_test_batch in;
    std::memset(&in, 0, sizeof(in));
    in.counts = counts; in.lcounts = lcounts; in.img_stride = 1; in.depth = depth.data(); in.frame_mp = fmp.data(); in.outlier = out.data();
    in.ldisp = ldisp.data(); in.frame_ml = fml.data(); in.outlier_l = out_l.data(); in.ldisp_frame = ldisp_frame; in.rows = rows;
    in.n_ref_matches = nref; in.n_ref_matches_l = nref_l; in.n_inliers = ninl; in.mbf = mCurrentFrame.mbf; in.thDepth = mThDepth;
    uint8_t need[2], ba[2];
    int32_t cnt[8], cond[2], st[2];
    const olf_keyframe_test_outputs o = {need, ba, cnt, cond, st};
    olf_detail::check(olf_need_new_keyframe(&in, (int)cap, (int)lcap, 2, &o), "olf_need_new_keyframe");
    KeyFrameDecision d;
    d.need = need[0] != 0; d.interrupt_ba = ba[0] != 0; d.nTrackedClose = cnt[0]; d.nNonTrackedClose = cnt[1]; d.nTrackedClose_l = cnt[2]; d.nNonTrackedClose_l = cnt[3];
    d.conditions = cond[0]; d.status = st[0];
    return d;
}

}  // namespace ORB_SLAM2
