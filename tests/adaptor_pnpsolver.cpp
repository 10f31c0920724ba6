// adaptor_pnpsolver.cpp -- ORB_SLAM2::PnPsolverOf and PnPsolversIterate (include/orbline_reference_api.hpp) against stand-in types: a frame of 40 key
// points sees 40 map points under a pose (0.3 rad about z, a translation), 30 of the key points noise-free projections and 7 displaced by 50 pixels; one
// match is NULL and two points are bad, which leaves 37 correspondences.
//   without an argument  the host form, no device: SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), iterate(5, ...) until it returns a pose, find() on a
//                        new solver with the same stream, a solver below the minimum.  Prints ADAPTOR_PNPSOLVER_OK.
//   with "device"        a second pair of solvers with the same rand() stream through PnPsolversIterate on the thread's context, compared bit for bit
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
    Mat(int r, int c, int /* type */ = 5) : rows(r), cols(c), d((size_t)r * c, 0.f) {}
    bool empty() const { return d.empty(); }
    template <class T> T& at(int r, int c) { return d[(size_t)r * cols + c]; }
    template <class T> const T& at(int r, int c) const { return d[(size_t)r * cols + c]; }
    template <class T> T& at(int i) { return d[i]; }
    template <class T> const T& at(int i) const { return d[i]; }
};
struct KeyPoint { float x = 0, y = 0, size = 31, angle = 0, response = 0; int octave = 0, class_id = -1; };
struct MapPoint {
    Mat w = Mat(3, 1);
    bool bad = false;
    bool isBad() { return bad; }
    Mat GetWorldPos() { return w; }
};
struct Frame {
    float fx = 200.f, fy = 200.f, cx = 160.f, cy = 120.f;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    Mat mTcw;
    Frame() { float s = 1.f; for (int l = 0; l < 8; ++l) { mvScaleFactors.push_back(s); s = (float)((double)s * (double)1.2f); } }
};
typedef ORB_SLAM2::PnPsolverOf<Frame, MapPoint> Solver;

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float unit(uint32_t& s) { return (float)lcg(s) / 16777216.0f; }

int main(int argc, char** argv)
{
    const bool device = argc > 1 && !std::strcmp(argv[1], "device");
    const int n = 40;
    const float c = std::cos(0.3f), s = std::sin(0.3f), t[3] = {0.2f, -0.1f, 0.3f};
    Frame F;
    std::vector<MapPoint> pts(n);
    std::vector<MapPoint*> matches(n, nullptr);
    uint32_t seed = 99u;
    F.mvKeysUn.resize(n);
    for (int i = 0; i < n; ++i) {
        const float z = 3.f + 6.f * unit(seed), xw[3] = {(unit(seed) - 0.5f) * z, (unit(seed) - 0.5f) * z * 0.7f, z};
        for (int k = 0; k < 3; ++k) pts[i].w.at<float>(k) = xw[k];
        const double xc = (double)c * xw[0] - (double)s * xw[1] + t[0], yc = (double)s * xw[0] + (double)c * xw[1] + t[1], zc = (double)xw[2] + t[2];
        F.mvKeysUn[i].x = (float)(200.0 * xc / zc + 160.0) + (i % 5 == 4 && i < 35 ? 50.f : 0.f);
        F.mvKeysUn[i].y = (float)(200.0 * yc / zc + 120.0);
        F.mvKeysUn[i].octave = i % 8;
        matches[i] = &pts[i];
    }
    matches[7] = nullptr; pts[11].bad = true; pts[20].bad = true;    // three entries that are no correspondence

    srand(7);
    Solver solver(F, matches);
    solver.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
    expect(solver.N == 37, "37 correspondences are kept");
    bool bNoMore = false;
    std::vector<bool> vbInliers;
    int nInliers = 0, calls = 0;
    Mat Tcw;
    while (Tcw.empty() && !bNoMore && calls < 60) { Tcw = solver.iterate(5, bNoMore, vbInliers, nInliers); ++calls; }
    expect(!Tcw.empty() && Tcw.rows == 4 && nInliers >= 27 && (int)vbInliers.size() == n, "iterate returns a pose");
    int set = 0;
    for (int i = 0; i < n; ++i) set += vbInliers[i] ? 1 : 0;
    expect(set == nInliers && !vbInliers[7] && !vbInliers[11] && !vbInliers[20] && !vbInliers[4], "the flags are scattered to the frame's features");
    if (!bNoMore)
        expect(std::fabs(Tcw.at<float>(0, 0) - c) < 1e-3f && std::fabs(Tcw.at<float>(1, 0) - s) < 1e-3f && std::fabs(Tcw.at<float>(2, 3) - t[2]) < 1e-2f &&
               Tcw.at<float>(3, 3) == 1.f, "the returned matrix is the pose");

    // find() on a new solver with the same stream gives the same pose; 9 correspondences end with bNoMore
    srand(7);
    Solver again(F, matches);
    again.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
    std::vector<bool> vb2;
    int n2 = 0;
    const Mat T2 = again.find(vb2, n2);
    expect(!T2.empty() && n2 == nInliers && vb2 == vbInliers && !std::memcmp(T2.d.data(), Tcw.d.data(), 64), "find() equals the windows of 5");
    std::vector<MapPoint*> few(matches);
    for (int i = 10; i < n; ++i) few[i] = nullptr;
    Solver small(F, few);
    small.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
    const Mat T3 = small.iterate(5, bNoMore, vb2, n2);
    expect(T3.empty() && bNoMore && n2 == 0 && small.N == 9 && vb2.empty(), "below minInliers: bNoMore at once");

    if (device) {
        olf_ctx* ctx = ORB_SLAM2::olf_detail::thread_ctx();
        srand(7);
        Solver d1(F, matches);
        d1.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        Solver d2(F, few);
        d2.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        std::vector<Solver*> solvers;
        solvers.push_back(&d1); solvers.push_back(&d2);
        std::vector<bool> noMore;
        std::vector<std::vector<bool> > inl;
        std::vector<int> ni;
        std::vector<Mat> tcw;
        int rounds = 0;
        do { ORB_SLAM2::PnPsolversIterate(ctx, solvers, 5, noMore, inl, ni, tcw); ++rounds; } while (tcw[0].empty() && !noMore[0] && rounds < 60);
        expect(rounds == calls && !tcw[0].empty() && ni[0] == nInliers && inl[0] == vbInliers && !std::memcmp(tcw[0].d.data(), Tcw.d.data(), 64) &&
               d1.mnIterations == solver.mnIterations, "PnPsolversIterate: the device equals the host form");
        expect(tcw[1].empty() && noMore[1] && ni[1] == 0, "PnPsolversIterate: the small solver ends with bNoMore");
    }
    if (failures) return 1;
    std::printf("ADAPTOR_PNPSOLVER_OK\n");
    return 0;
}
