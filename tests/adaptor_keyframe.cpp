// adaptor_keyframe.cpp -- ORB_SLAM2::CreateNewKeyFrameLandmarks, UpdateLastFrameLandmarks, StereoInitializationLandmarks and NeedNewKeyFrame
// (include/orbline_reference_api.hpp) against stand-in types with the members the reference's loops read (src/Tracking.cc:639-677, :1092-1204,
// :1606-1725, :1744-1865).  One frame of 180 stereo points (40 close) and 90 stereo lines (12 close), a third of them holding a landmark, half of those
// without observations.  The lists are compared with the loops written out here on std::pair<float,int> and std::sort.  Through the host forms: no device.
// Prints ADAPTOR_KEYFRAME_OK.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>
#include "../include/orbline_reference_api.hpp"

struct Mat {                                                         // the part of cv::Mat the adaptor touches, CV_32F only
    int rows = 0, cols = 0;
    std::vector<float> d;
    Mat() {}
    Mat(int r, int c, int) : rows(r), cols(c), d((size_t)r * c, 0.f) {}
    template <class T> T& at(int r, int c) { return d[(size_t)r * cols + c]; }
    template <class T> const T& at(int r, int c) const { return d[(size_t)r * cols + c]; }
    template <class T> const T& at(int i) const { return d[i]; }
};
struct KeyPoint { float x = 0, y = 0, size = 0, angle = -1, response = 0; int octave = 0, class_id = -1; };
struct KeyLine {
    float angle = 0; int class_id = 0, octave = 0; float pt_x = 0, pt_y = 0, response = 0, size = 0, startPointX = 0, startPointY = 0, endPointX = 0, endPointY = 0,
    sPointInOctaveX = 0, sPointInOctaveY = 0, ePointInOctaveX = 0, ePointInOctaveY = 0, lineLength = 0; int numOfPixels = 0;
};
struct MapPoint { int nObs = 0; int Observations() { return nObs; } };
struct MapLine { int nObs = 0; int Observations() { return nObs; } };
struct Frame {
    int N = 0, N_l = 0;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<KeyLine> mvKeysUn_Line;
    std::vector<float> mvDepth, mvScaleFactors;
    std::vector<std::pair<float, float>> mvDisparity_l;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    std::vector<bool> mvbOutlier, mvbOutlier_Line;
    Mat mRwc, mOw;
    float fx = 435.2f, fy = 435.2f, cx = 367.4f, cy = 252.2f, mbf = 47.9f;
};

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static unsigned lcg = 2024u;
static double uni(double a, double b) { lcg = lcg * 1664525u + 1013904223u; return a + (b - a) * ((lcg >> 8) / 16777216.0); }

// the walk of :1763-1798 on vDepthIdx
template <class Holds>
static void walk(std::vector<std::pair<float, int>> v, float th, int least, Holds holds, std::vector<int>& visited, std::vector<int>& created, int& n)
{
    std::sort(v.begin(), v.end());
    n = 0;
    for (size_t j = 0; j < v.size(); j++) {
        visited.push_back(v[j].second);
        if (!holds(v[j].second)) created.push_back(v[j].second);
        n++;
        if (v[j].first > th && n > least) break;
    }
}

int main()
{
    const float th = 3.85f;
    Frame F;
    F.N = 180; F.N_l = 90;
    float sf = 1.f;
    for (int l = 0; l < 8; ++l) { F.mvScaleFactors.push_back(sf); sf *= 1.2f; }
    F.mRwc = Mat(3, 3, 5); F.mOw = Mat(3, 1, 5);
    const double a = 0.05;
    const float Rm[9] = {(float)std::cos(a), 0.f, (float)std::sin(a), 0.f, 1.f, 0.f, (float)-std::sin(a), 0.f, (float)std::cos(a)};
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) F.mRwc.at<float>(r, k) = Rm[3 * r + k]; F.mOw.d[r] = 0.3f * (r + 1); }
    std::vector<MapPoint> points(180);
    std::vector<MapLine> mlines(90);
    for (int i = 0; i < F.N; ++i) {
        KeyPoint kp;
        kp.x = (float)uni(20, 1200); kp.y = (float)uni(20, 360); kp.octave = i % 8;
        F.mvKeysUn.push_back(kp);
        F.mvDepth.push_back(i % 9 == 4 ? -1.f : (float)(i < 40 ? uni(0.5, 3.8) : uni(3.9, 20)));
        points[i].nObs = i % 6 == 0 ? 0 : 2;
        F.mvpMapPoints.push_back(i % 3 == 0 ? &points[i] : nullptr);
        F.mvbOutlier.push_back(i % 10 == 0);
    }
    for (int i = 0; i < F.N_l; ++i) {
        KeyLine kl;
        kl.startPointX = (float)uni(20, 1200); kl.startPointY = (float)uni(20, 360); kl.endPointX = (float)uni(20, 1200); kl.endPointY = (float)uni(20, 360);
        F.mvKeysUn_Line.push_back(kl);
        const double zf = i < 12 ? uni(0.5, 3.8) : uni(3.9, 15), zn = zf * uni(0.4, 0.95);
        F.mvDisparity_l.push_back(i % 11 == 5 ? std::make_pair(-1.f, -1.f) : i % 2 ? std::make_pair((float)(47.9 / zf), (float)(47.9 / zn))
                                                                                      : std::make_pair((float)(47.9 / zn), (float)(47.9 / zf)));
        mlines[i].nObs = i % 4 == 0 ? 0 : 1;
        F.mvpMapLines.push_back(i % 2 == 0 ? &mlines[i] : nullptr);
        F.mvbOutlier_Line.push_back(i % 7 == 0);
    }
    // the loops, written out
    std::vector<std::pair<float, int>> vp, vl;
    for (int i = 0; i < F.N; i++) if (F.mvDepth[i] > 0) vp.push_back(std::make_pair(F.mvDepth[i], i));
    for (int i = 0; i < F.N_l; i++) {
        const float sz = F.mbf / F.mvDisparity_l[i].first, ez = F.mbf / F.mvDisparity_l[i].second;
        if (sz < 0 || ez < 0) continue;
        vl.push_back(std::make_pair(sz > ez ? sz : ez, i));
    }
    std::vector<int> ev, ec, evl, ecl;
    int en = 0, enl = 0;
    walk(vp, th, 100, [&](int i) { return F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() >= 1; }, ev, ec, en);
    walk(vl, th, 50, [&](int i) { return F.mvpMapLines[i] && F.mvpMapLines[i]->Observations() >= 1; }, evl, ecl, enl);

    const ORB_SLAM2::StereoLandmarks K = ORB_SLAM2::CreateNewKeyFrameLandmarks(F, th);
    expect(K.status == 0 && K.nPoints == en && K.nLines == enl && en == 101 && enl == 51, "the counters of both loops");
    expect(K.visited == ev && K.created == ec && K.visited_l == evl && K.created_l == ecl, "visit and creation lists of CreateNewKeyFrame");
    expect(K.world.size() == 3 * ec.size() && K.maxd.size() == ec.size() && K.world_l.size() == 6 * ecl.size(), "geometry per created landmark");
    bool geo = !ec.empty();
    for (size_t k = 0; k < ec.size() && geo; ++k) {                   // a created point lies at its depth along the ray, and its normal is a unit vector
        const int i = ec[k];
        const double z = F.mvDepth[i], x = (F.mvKeysUn[i].x - F.cx) * z / F.fx, y = (F.mvKeysUn[i].y - F.cy) * z / F.fy;
        for (int r = 0; r < 3; ++r) geo = geo && std::fabs(K.world[3 * k + r] - (Rm[3 * r] * x + Rm[3 * r + 1] * y + Rm[3 * r + 2] * z + F.mOw.d[r])) < 1e-3 * (1 + z);
        const double nn = std::sqrt((double)K.normal[3 * k] * K.normal[3 * k] + (double)K.normal[3 * k + 1] * K.normal[3 * k + 1] + (double)K.normal[3 * k + 2] * K.normal[3 * k + 2]);
        geo = geo && std::fabs(nn - 1) < 1e-5 && K.maxd[k] > K.mind[k] && K.mind[k] > 0;
    }
    expect(geo, "UnprojectStereo, the normal and the distances of the created points");
    bool lgeo = !ecl.empty();
    for (size_t k = 0; k < ecl.size() && lgeo; ++k) {
        const int i = ecl[k];
        const double bd = ((double)F.mbf / F.fx) / F.mvDisparity_l[i].first, P[3] = {bd * (F.mvKeysUn_Line[i].startPointX - F.cx), bd * (F.mvKeysUn_Line[i].startPointY - F.cy), bd * F.fx};
        for (int r = 0; r < 3; ++r) lgeo = lgeo && std::fabs(K.world_l[6 * k + r] - (Rm[3 * r] * P[0] + Rm[3 * r + 1] * P[1] + Rm[3 * r + 2] * P[2] + F.mOw.d[r])) < 1e-6 * (1 + bd * F.fx);      // (mb is the float mbf / fx)
    }
    expect(lgeo, "backProjection of the created lines");

    const ORB_SLAM2::StereoLandmarks U = ORB_SLAM2::UpdateLastFrameLandmarks(F, th);
    expect(U.visited == ev && U.created == ec && U.visited_l == evl && U.created_l == ecl && U.world == K.world && U.maxd == K.maxd, "UpdateLastFrame makes the same lists");
    Frame G = F;
    for (int i = 0; i < G.N; ++i) G.mvDepth[i] = -1.f;
    const ORB_SLAM2::StereoLandmarks U0 = ORB_SLAM2::UpdateLastFrameLandmarks(G, th), K0 = ORB_SLAM2::CreateNewKeyFrameLandmarks(G, th);
    expect(U0.visited_l.empty() && U0.nLines == 0 && K0.visited_l == evl, "no stereo point: UpdateLastFrame returns before its lines, CreateNewKeyFrame does not");
    const ORB_SLAM2::StereoLandmarks I = ORB_SLAM2::StereoInitializationLandmarks(F);
    std::vector<int> ei, eil;
    for (int i = 0; i < F.N; i++) if (F.mvDepth[i] > 0) ei.push_back(i);
    for (int i = 0; i < F.N_l; ++i) if (F.mvDisparity_l[i].first > 0 && F.mvDisparity_l[i].second > 0) eil.push_back(i);
    expect(I.created == ei && I.created_l == eil && I.visited == ei, "StereoInitialization creates every stereo feature in index order");

    // NeedNewKeyFrame: the counts written out, and the decision of a tracker that lost most of its matches
    int tc = 0, nc = 0, tcl = 0, ncl = 0;
    for (int i = 0; i < F.N; i++) if (F.mvDepth[i] > 0 && F.mvDepth[i] < th) { if (F.mvpMapPoints[i] && !F.mvbOutlier[i]) tc++; else nc++; }
    for (int i = 0; i < F.N_l; i++) {
        float minz = F.mbf / F.mvDisparity_l[i].first, maxz = F.mbf / F.mvDisparity_l[i].second;
        if (minz > maxz) std::swap(minz, maxz);
        if (minz > 0 && maxz < th) { if (F.mvpMapLines[i] && !F.mvbOutlier_Line[i]) ++tcl; else ++ncl; }
    }
    ORB_SLAM2::KeyFrameTest t;
    t.mnId = 100; t.mnLastKeyFrameId = 90; t.mMaxFrames = 30; t.nKFs = 5; t.nRefMatches = 100; t.nRefMatches_l = 100; t.mnMatchesInliers = 20; t.mnMatchesInliers_l = 80;
    ORB_SLAM2::KeyFrameDecision d = ORB_SLAM2::NeedNewKeyFrame(F, F, t, th);
    expect(d.nTrackedClose == tc && d.nNonTrackedClose == nc && d.nTrackedClose_l == tcl && d.nNonTrackedClose_l == ncl && tc + nc > 20 && tcl + ncl > 5, "the four counts");
    expect(d.conditions == (4 | 16) && d.need && d.interrupt_ba && d.status == 0, "c1c and c2 with local mapping busy and an empty queue: InterruptBA, then true");
    t.KeyframesInQueue = 3;
    d = ORB_SLAM2::NeedNewKeyFrame(F, F, t, th);
    expect(!d.need && d.interrupt_ba, "three key frames queued");
    t.bLocalMappingIdle = true;
    d = ORB_SLAM2::NeedNewKeyFrame(F, F, t, th);
    expect(d.need && !d.interrupt_ba && d.conditions == (2 | 4 | 16), "local mapping idle");
    Frame L = F;
    L.N_l = 30; L.mvDisparity_l.resize(30);
    d = ORB_SLAM2::NeedNewKeyFrame(F, L, t, th);
    expect(d.status == 1 && d.nTrackedClose_l + d.nNonTrackedClose_l <= tcl + ncl, "a shorter last frame: the lines it lacks are not counted");
    if (failures) return 1;
    std::printf("ADAPTOR_KEYFRAME_OK\n");
    return 0;
}
