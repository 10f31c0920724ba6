// adaptor_newpoints.cpp -- ORB_SLAM2::ComputeF12, CreateNewMapPoints and MapGraphOf::UpdateNormalAndDepth (include/orbline_reference_api.hpp) against stand-in
// types: two key frames 0.5 m apart (sideways and forward) that see five points -- one to triangulate, one stereo point whose parallax is below its stereo angle (UnprojectStereo of
// key frame 1), one far mono point (low parallax), one wrong match (rejected), and a second match on an idx1 already listed.
//   without an argument  the host forms, no device.  Prints ADAPTOR_NEWPOINTS_OK.
//   with "device"        the same through the thread's context on the device, and every result compared bit for bit with the host forms'.
// The stand-in MapPoint provides the one accessor the integrator adds (SetNormalAndDepth).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../include/orbline_reference_api.hpp"

struct Mat {                                                         // the part of cv::Mat the adaptor touches, CV_32F only
    int rows = 0, cols = 0;
    std::vector<float> d;
    Mat() {}
    Mat(int r, int c) : rows(r), cols(c), d((size_t)r * c, 0.f) {}
    template <class T> T& at(int r, int c) { return d[(size_t)r * cols + c]; }
    template <class T> const T& at(int r, int c) const { return d[(size_t)r * cols + c]; }
    template <class T> T& at(int i) { return d[i]; }
    template <class T> const T& at(int i) const { return d[i]; }
};
struct KeyPoint { float x = 0, y = 0, size = 31, angle = 0, response = 0; int octave = 0, class_id = -1; };
struct KeyFrame;
struct MapLine { bool isBad() { return false; } };
struct MapPoint {
    Mat w = Mat(3, 1), normal = Mat(3, 1);
    KeyFrame* ref = nullptr;
    std::map<KeyFrame*, size_t> mObservations;
    bool bad = false;
    float maxd = -5.f, mind = -5.f;
    int calls = 0;
    bool isBad() { return bad; }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    int Observations() { return (int)mObservations.size(); }
    Mat GetWorldPos() { return w; }
    KeyFrame* GetReferenceKeyFrame() { return ref; }
    void SetNormalAndDepth(const Mat& n, float maxDistance, float minDistance) { normal = n; maxd = maxDistance; mind = minDistance; ++calls; }
};
struct KeyFrame {
    long unsigned int mnId = 1;
    float mThDepth = 35.f, fx = 200.f, fy = 200.f, cx = 160.f, cy = 120.f, mbf = 40.f, mb = 0.2f;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvDepth, mvScaleFactors;
    std::vector<MapPoint*> mvpMapPoints;
    Mat Tcw = Mat(4, 4);
    KeyFrame() { for (int i = 0; i < 4; ++i) Tcw.at<float>(i, i) = 1.f; float s = 1.f; for (int l = 0; l < 8; ++l) { mvScaleFactors.push_back(s); s = (float)((double)s * (double)1.2f); } }
    Mat GetPose() { return Tcw; }
    Mat GetRotation() { Mat R(3, 3); for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R.at<float>(r, c) = Tcw.at<float>(r, c); return R; }
    Mat GetCameraCenter() { Mat o(3, 1); for (int r = 0; r < 3; ++r) { float s = 0; for (int k = 0; k < 3; ++k) s += Tcw.at<float>(k, r) * Tcw.at<float>(k, 3); o.at<float>(r) = -s; } return o; }
    bool isBad() { return false; }
    bool GetNotErase() { return false; }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<MapLine*> GetMapLineMatches() { return std::vector<MapLine*>(); }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return std::vector<KeyFrame*>(); }
    std::set<KeyFrame*> GetChilds() { return std::set<KeyFrame*>(); }
    KeyFrame* GetParent() { return nullptr; }
    // feature i: the projection of world point X (with a pixel offset), octave, stereo or not
    size_t see(const double* X, int octave, bool stereo, float dy = 0.f)
    {
        const double x = X[0] + Tcw.at<float>(0, 3), y = X[1] + Tcw.at<float>(1, 3), z = X[2] + Tcw.at<float>(2, 3);      // (identity rotations)
        KeyPoint k;
        k.x = (float)(fx * x / z + cx); k.y = (float)(fy * y / z + cy) + dy; k.octave = octave;
        mvKeysUn.push_back(k);
        mvDepth.push_back(stereo ? (float)z : -1.f);
        mvuRight.push_back(stereo ? k.x - mbf / (float)z : -1.f);
        mvpMapPoints.push_back(nullptr);
        return mvKeysUn.size() - 1;
    }
};

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static bool same_bits(const float* a, const float* b, size_t n) { return std::memcmp(a, b, 4 * n) == 0; }
typedef ORB_SLAM2::MapGraphOf<KeyFrame, MapPoint, MapLine> Graph;

int main(int argc, char** argv)
{
    const bool device = argc > 1 && !std::strcmp(argv[1], "device");
    olf_ctx* ctx = device ? ORB_SLAM2::olf_detail::thread_ctx() : nullptr;
    KeyFrame kf1, kf2;
    kf2.Tcw.at<float>(0, 3) = -0.3f; kf2.Tcw.at<float>(2, 3) = -0.4f; // 0.5 m from kf1: 0.3 to the right, 0.4 forward
    const double P[4][3] = {{0.4, -0.2, 6.0}, {-0.3, 0.1, 40.0}, {1.0, 0.5, 600.0}, {0.2, 0.3, 5.0}};
    std::vector<std::pair<size_t, size_t> > matches;
    matches.push_back(std::make_pair(kf1.see(P[0], 2, false), kf2.see(P[0], 2, false)));       // mono - mono with parallax: triangulated
    matches.push_back(std::make_pair(kf1.see(P[1], 1, true), kf2.see(P[1], 1, false)));        // stereo in kf1, its parallax below its stereo angle: UnprojectStereo
    matches.push_back(std::make_pair(kf1.see(P[2], 0, false), kf2.see(P[2], 0, false)));       // far, mono: low parallax
    matches.push_back(std::make_pair(kf1.see(P[3], 0, false), kf2.see(P[3], 0, false, 25.f))); // 25 px off the epipolar line: rejected
    matches.push_back(std::make_pair(matches[0].first, matches[3].second));                    // idx1 of match 0 again, with another idx2
    kf1.mb = kf2.mb = 0.45f; kf1.mbf = kf2.mbf = 90.f;               // the stereo angle of point 1 (0.45 / 40) is above its parallax (0.3 / 40), the baseline above mb
    kf1.mvuRight[1] = kf1.mvKeysUn[1].x - kf1.mbf / kf1.mvDepth[1];

    // ---- ComputeF12 ----
    const Mat F12 = ORB_SLAM2::ComputeF12(ctx, &kf1, &kf2);
    float F[9];
    expect(olf_compute_f12(kf1.Tcw.d.data(), kf2.Tcw.d.data(), 200.f, 200.f, 160.f, 120.f, F) == OLF_OK && same_bits(F, F12.d.data(), 9), "ComputeF12 equals olf_compute_f12");
    const KeyPoint &a = kf1.mvKeysUn[0], &b = kf2.mvKeysUn[0];
    const double l[3] = {a.x * F[0] + a.y * F[3] + F[6], a.x * F[1] + a.y * F[4] + F[7], a.x * F[2] + a.y * F[5] + F[8]};
    expect(std::fabs(l[0] * b.x + l[1] * b.y + l[2]) / std::sqrt(l[0] * l[0] + l[1] * l[1]) < 1e-2, "ComputeF12: a true correspondence lies on its epipolar line");

    // ---- CreateNewMapPoints ----
    ORB_SLAM2::NewMapPoints out, host;
    ORB_SLAM2::CreateNewMapPoints(ctx, &kf1, &kf2, matches, false, out);
    ORB_SLAM2::CreateNewMapPoints(nullptr, &kf1, &kf2, matches, false, host);
    expect(out.code == host.code && out.nnew == host.nnew && same_bits(out.x3D.data(), host.x3D.data(), out.x3D.size()), "CreateNewMapPoints: the device equals the host form");
    expect(out.code.size() == 5 && out.code[0] == 1 && out.code[1] == 2 && out.code[2] == 16 && out.code[3] >= 16 && out.code[4] >= 16, "CreateNewMapPoints: the codes");
    expect(out.nnew == 2 && !out.skipped, "CreateNewMapPoints: nnew");
    if (failures) std::printf("codes %d %d %d %d %d, nnew %d, x3D %g %g %g | %g %g %g\n", out.code[0], out.code[1], out.code[2], out.code[3], out.code[4], out.nnew, out.x3D[0], out.x3D[1],
                              out.x3D[2], out.x3D[3], out.x3D[4], out.x3D[5]);
    bool near = true;
    for (int k = 0; k < 3; ++k) near = near && std::fabs(out.x3D[k] - P[0][k]) < 2e-2 && std::fabs(out.x3D[3 + k] - P[1][k]) < 2e-2 && out.x3D[6 + k] == 0.f;
    expect(near, "CreateNewMapPoints: the triangulated and the unprojected point");
    kf2.mb = 0.6f;                                                   // baseline 0.5 < mb: the neighbour is skipped
    ORB_SLAM2::CreateNewMapPoints(ctx, &kf1, &kf2, matches, false, out);
    expect(out.nnew == 0 && out.skipped && out.code == std::vector<uint8_t>(5, 0), "CreateNewMapPoints: the baseline test");
    ORB_SLAM2::CreateNewMapPoints(ctx, &kf1, &kf2, matches, true, out);
    expect(out.nnew == 2 && !out.skipped, "CreateNewMapPoints: monocular leaves the baseline test out");

    // ---- UpdateNormalAndDepth: the two created points as map points, a bad one and one outside the list ----
    MapPoint mp[4];
    for (int i = 0; i < 4; ++i) {
        const int m = i < 2 ? i : 0;
        for (int k = 0; k < 3; ++k) mp[i].w.at<float>(k) = host.x3D[3 * m + k] + (i >= 2 ? 1.f : 0.f);
        mp[i].mObservations[&kf1] = matches[m].first; mp[i].mObservations[&kf2] = matches[m].second;
        mp[i].ref = &kf1;
    }
    mp[2].bad = true;
    kf1.mvpMapPoints[0] = &mp[0]; kf1.mvpMapPoints[1] = &mp[1]; kf1.mvpMapPoints[2] = &mp[2]; kf1.mvpMapPoints[3] = &mp[3];
    std::vector<KeyFrame*> kfs;
    kfs.push_back(&kf1); kfs.push_back(&kf2);
    std::vector<MapPoint*> list;
    list.push_back(&mp[1]); list.push_back(&mp[0]); list.push_back(&mp[2]); list.push_back(&mp[1]);
    Graph G(kfs);
    expect(G.UpdateNormalAndDepth(ctx, list) == 2, "UpdateNormalAndDepth: two points change");
    expect(mp[0].calls == 1 && mp[1].calls == 1 && mp[2].calls == 0 && mp[3].calls == 0 && mp[2].maxd == -5.f && mp[3].maxd == -5.f, "UpdateNormalAndDepth: the bad and the unlisted point are untouched");
    for (int i = 0; i < 2; ++i) {
        double n[3] = {0, 0, 0}, d1 = 0;
        KeyFrame* obs[2] = {&kf1, &kf2};
        for (int j = 0; j < 2; ++j) {
            const Mat o = obs[j]->GetCameraCenter();
            double v[3], s = 0;
            for (int k = 0; k < 3; ++k) { v[k] = mp[i].w.at<float>(k) - o.at<float>(k); s += v[k] * v[k]; }
            for (int k = 0; k < 3; ++k) n[k] += v[k] / std::sqrt(s) / 2;
            if (j == 0) d1 = std::sqrt(s);
        }
        const float sf = kf1.mvScaleFactors[kf1.mvKeysUn[matches[i].first].octave];
        bool ok = std::fabs(mp[i].maxd - d1 * sf) < 1e-4 * d1 && std::fabs(mp[i].mind - d1 * sf / kf1.mvScaleFactors[7]) < 1e-4 * d1;
        for (int k = 0; k < 3; ++k) ok = ok && std::fabs(mp[i].normal.at<float>(k) - n[k]) < 1e-5;
        expect(ok, "UpdateNormalAndDepth: normal, mfMaxDistance, mfMinDistance");
    }
    if (device) {
        const Mat n0 = mp[0].normal, n1 = mp[1].normal;
        const float m0 = mp[0].maxd, m1 = mp[1].mind;
        Graph H(kfs);
        expect(H.UpdateNormalAndDepth(nullptr, list) == 2 && same_bits(n0.d.data(), mp[0].normal.d.data(), 3) && same_bits(n1.d.data(), mp[1].normal.d.data(), 3) &&
               m0 == mp[0].maxd && m1 == mp[1].mind, "UpdateNormalAndDepth: the device equals the host form");
    }
    if (failures) return 1;
    std::printf("ADAPTOR_NEWPOINTS_OK\n");
    return 0;
}
