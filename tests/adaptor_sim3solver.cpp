// adaptor_sim3solver.cpp -- ORB_SLAM2::Sim3SolverOf and Sim3SolversIterate (include/orbline_reference_api.hpp) against stand-in types: two key frames see 40
// points under a similarity (scale 2, 0.3 rad about z, a translation); key frame 2 holds them in reversed order, so GetIndexInKeyFrame(pKF2) differs from
// i1; one match is NULL, one point is bad and one is not observed by key frame 2 (index -1), which leaves 37 correspondences.
//   without an argument  the host form, no device: SetRansacParameters(0.99, 20, 300), iterate(5, ...) until it returns a similarity.  Prints
//                        ADAPTOR_SIM3SOLVER_OK.
//   with "device"        a second pair of solvers with the same rand() stream through Sim3SolversIterate on the thread's context, compared bit for bit
//                        with the host form's.
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
    bool empty() const { return d.empty(); }
    template <class T> T& at(int r, int c) { return d[(size_t)r * cols + c]; }
    template <class T> const T& at(int r, int c) const { return d[(size_t)r * cols + c]; }
    template <class T> T& at(int i) { return d[i]; }
    template <class T> const T& at(int i) const { return d[i]; }
};
struct KeyPoint { float x = 0, y = 0, size = 31, angle = 0, response = 0; int octave = 0, class_id = -1; };
struct KeyFrame;
struct MapPoint {
    Mat w = Mat(3, 1);
    bool bad = false;
    std::map<KeyFrame*, int> index;
    bool isBad() { return bad; }
    Mat GetWorldPos() { return w; }
    int GetIndexInKeyFrame(KeyFrame* pKF) { return index.count(pKF) ? index[pKF] : -1; }
};
struct KeyFrame {
    float fx = 200.f, fy = 200.f, cx = 160.f, cy = 120.f;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    std::vector<MapPoint*> mvpMapPoints;
    Mat Tcw = Mat(4, 4);
    KeyFrame() { for (int i = 0; i < 4; ++i) Tcw.at<float>(i, i) = 1.f; float s = 1.f; for (int l = 0; l < 8; ++l) { mvScaleFactors.push_back(s); s = (float)((double)s * (double)1.2f); } }
    Mat GetPose() { return Tcw; }
    Mat GetRotation() { Mat R(3, 3); for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R.at<float>(r, c) = Tcw.at<float>(r, c); return R; }
    Mat GetTranslation() { Mat t(3, 1); for (int r = 0; r < 3; ++r) t.at<float>(r) = Tcw.at<float>(r, 3); return t; }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
};
typedef ORB_SLAM2::Sim3SolverOf<KeyFrame, MapPoint> Solver;

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float unit(uint32_t& s) { return (float)lcg(s) / 16777216.0f; }

int main(int argc, char** argv)
{
    const bool device = argc > 1 && !std::strcmp(argv[1], "device");
    const int n = 40;
    const float c = std::cos(0.3f), s = std::sin(0.3f), scale = 2.f, t[3] = {0.2f, -0.1f, 0.3f};
    KeyFrame kf1, kf2;
    std::vector<MapPoint> p1(n), p2(n);
    std::vector<MapPoint*> matched(n, nullptr);
    uint32_t seed = 99u;
    kf1.mvKeysUn.resize(n); kf2.mvKeysUn.resize(n); kf1.mvpMapPoints.resize(n); kf2.mvpMapPoints.resize(n);
    for (int i = 0; i < n; ++i) {
        const float z = 3.f + 6.f * unit(seed), x2[3] = {(unit(seed) - 0.5f) * z, (unit(seed) - 0.5f) * z * 0.7f, z};
        const int j = n - 1 - i;                                     // the feature of key frame 2 that holds point i
        for (int k = 0; k < 3; ++k) p2[i].w.at<float>(k) = x2[k];
        p1[i].w.at<float>(0) = scale * (c * x2[0] - s * x2[1]) + t[0];
        p1[i].w.at<float>(1) = scale * (s * x2[0] + c * x2[1]) + t[1];
        p1[i].w.at<float>(2) = scale * x2[2] + t[2];
        p1[i].index[&kf1] = i; p2[i].index[&kf2] = j;
        kf1.mvpMapPoints[i] = &p1[i]; kf2.mvpMapPoints[j] = &p2[i];
        kf1.mvKeysUn[i].octave = i % 8; kf2.mvKeysUn[j].octave = (i / 3) % 8;
        matched[i] = &p2[i];
    }
    matched[7] = nullptr; p1[11].bad = true; p2[20].index.clear();   // three entries that are no correspondence

    srand(7);
    Solver solver(&kf1, &kf2, matched, false);
    solver.SetRansacParameters(0.99, 20, 300);
    expect(solver.N == 37, "37 correspondences are kept");
    bool bNoMore = false;
    std::vector<bool> vbInliers;
    int nInliers = 0, calls = 0;
    Mat Scm;
    while (Scm.empty() && !bNoMore && calls < 60) { Scm = solver.iterate(5, bNoMore, vbInliers, nInliers); ++calls; }
    expect(!Scm.empty() && Scm.rows == 4 && nInliers == 37 && (int)vbInliers.size() == n, "iterate returns a similarity with every correspondence an inlier");
    int set = 0;
    for (int i = 0; i < n; ++i) set += vbInliers[i] ? 1 : 0;
    expect(set == 37 && !vbInliers[7] && !vbInliers[11] && !vbInliers[20], "the flags are scattered to i1");
    const Mat R = solver.GetEstimatedRotation(), tt = solver.GetEstimatedTranslation();
    expect(std::fabs(solver.GetEstimatedScale() - scale) < 1e-3f && std::fabs(R.at<float>(0, 0) - c) < 1e-3f && std::fabs(R.at<float>(1, 0) - s) < 1e-3f &&
           std::fabs(tt.at<float>(2) - t[2]) < 1e-2f && tt.rows == 3, "GetEstimatedRotation / Translation / Scale");
    expect(std::fabs(Scm.at<float>(0, 0) - scale * c) < 2e-3f && Scm.at<float>(3, 3) == 1.f, "the returned matrix is T12");

    // find() on a new solver with the same stream gives the same similarity; 10 correspondences end with bNoMore
    srand(7);
    Solver again(&kf1, &kf2, matched, false);
    again.SetRansacParameters(0.99, 20, 300);
    std::vector<bool> vb2;
    int n2 = 0;
    const Mat S2 = again.find(vb2, n2);
    expect(!S2.empty() && n2 == nInliers && vb2 == vbInliers && !std::memcmp(S2.d.data(), Scm.d.data(), 64), "find() equals the windows of 5");
    std::vector<MapPoint*> few(matched);
    for (int i = 10; i < n; ++i) few[i] = nullptr;
    Solver small(&kf1, &kf2, few, true);
    small.SetRansacParameters(0.99, 20, 300);
    const Mat S3 = small.iterate(5, bNoMore, vb2, n2);
    expect(S3.empty() && bNoMore && n2 == 0 && small.N == 9, "below minInliers: bNoMore at once");

    if (device) {
        olf_ctx* ctx = ORB_SLAM2::olf_detail::thread_ctx();
        srand(7);
        Solver d1(&kf1, &kf2, matched, false);
        d1.SetRansacParameters(0.99, 20, 300);
        Solver d2(&kf1, &kf2, few, false);
        d2.SetRansacParameters(0.99, 20, 300);
        std::vector<Solver*> solvers;
        solvers.push_back(&d1); solvers.push_back(&d2);
        std::vector<bool> noMore;
        std::vector<std::vector<bool> > inl;
        std::vector<int> ni;
        std::vector<Mat> scm;
        int rounds = 0;
        do { ORB_SLAM2::Sim3SolversIterate(ctx, solvers, 5, noMore, inl, ni, scm); ++rounds; } while (scm[0].empty() && !noMore[0] && rounds < 60);
        expect(rounds == calls && !scm[0].empty() && ni[0] == nInliers && inl[0] == vbInliers && !std::memcmp(scm[0].d.data(), Scm.d.data(), 64) &&
               d1.GetEstimatedScale() == solver.GetEstimatedScale(), "Sim3SolversIterate: the device equals the host form");
        expect(scm[1].empty() && noMore[1] && ni[1] == 0, "Sim3SolversIterate: the small solver ends with bNoMore");
    }
    if (failures) return 1;
    std::printf("ADAPTOR_SIM3SOLVER_OK\n");
    return 0;
}
