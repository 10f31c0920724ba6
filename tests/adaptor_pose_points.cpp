// adaptor_pose_points.cpp -- ORB_SLAM2::PoseOptimization (include/orbline_reference_api.hpp) against stand-in types with the members the reference's
// Optimizer::PoseOptimization reads and writes (src/Optimizer.cc:239-451).  One frame: 40 points at 3-12 m seen exactly by a camera 4 cm and 0.3 degrees
// from the pose the frame starts with, every third one monocular; features 5 and 17 hold nothing, point 9 is seen 40 pixels off.  The optimiser must bring
// the pose to the true one, flag point 9 and nothing else, and return 37.
//   without an argument  through the host form (no device).  Prints ADAPTOR_POSE_POINTS_OK.
//   with "device"        through olf_pose_optimization_rows on a context made for the frame; the same checks.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../include/orbline_reference_api.hpp"

struct Mat {                                                         // the part of cv::Mat the adaptor touches, CV_32F only
    int rows = 0, cols = 0;
    std::vector<float> d;
    Mat() {}
    Mat(int r, int c, int) : rows(r), cols(c), d((size_t)r * c, 0.f) {}
    bool empty() const { return d.empty(); }
    template <class T> T& at(int r, int c) { return d[(size_t)r * cols + c]; }
    template <class T> const T& at(int r, int c) const { return d[(size_t)r * cols + c]; }
    template <class T> const T& at(int i) const { return d[i]; }
};
struct KeyPoint { float x = 0, y = 0, size = 0, angle = -1, response = 0; int octave = 0, class_id = -1; };
struct MapPoint { Mat w; Mat GetWorldPos() { return w; } };
struct Frame {
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<bool> mvbOutlier;
    Mat mTcw;
    float fx = 250.f, fy = 250.f, cx = 160.f, cy = 120.f, mbf = 25.f;
    int poses_set = 0;
    void SetPose(const Mat& T) { mTcw = T; ++poses_set; }
};

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static unsigned lcg = 12345u;
static double uni(double a, double b) { lcg = lcg * 1664525u + 1013904223u; return a + (b - a) * ((lcg >> 8) / 16777216.0); }

int main(int argc, char** argv)
{
    const bool device = argc > 1 && !std::strcmp(argv[1], "device");
    const double a = 0.3 * 3.14159265358979323846 / 180.0;
    const double Tt[12] = {std::cos(a), 0, std::sin(a), 0.04, 0, 1, 0, 0.0, -std::sin(a), 0, std::cos(a), 0.01};
    Frame F;
    F.mvInvLevelSigma2.resize(8);
    float sf = 1.f;
    for (int l = 0; l < 8; ++l) { F.mvInvLevelSigma2[l] = 1.0f / (sf * sf); sf = (float)(sf * 1.2); }
    F.mTcw = Mat(4, 4, 5);
    for (int i = 0; i < 4; ++i) F.mTcw.at<float>(i, i) = 1.f;
    std::vector<MapPoint> points(40);
    for (int i = 0; i < 40; ++i) {
        const double z = uni(3, 12), X[3] = {uni(-0.5, 0.5) * z, uni(-0.35, 0.35) * z, z};
        points[i].w = Mat(3, 1, 5);
        for (int k = 0; k < 3; ++k) points[i].w.at<float>(k, 0) = (float)X[k];
        const double Xf[3] = {(double)(float)X[0], (double)(float)X[1], (double)(float)X[2]};
        const double P[3] = {Tt[0] * Xf[0] + Tt[1] * Xf[1] + Tt[2] * Xf[2] + Tt[3], Tt[4] * Xf[0] + Tt[5] * Xf[1] + Tt[6] * Xf[2] + Tt[7], Tt[8] * Xf[0] + Tt[9] * Xf[1] + Tt[10] * Xf[2] + Tt[11]};
        KeyPoint kp;
        kp.x = (float)(160.0 + 250.0 * P[0] / P[2]) + (i == 9 ? 40.f : 0.f); kp.y = (float)(120.0 + 250.0 * P[1] / P[2]); kp.octave = i % 8;
        F.mvKeysUn.push_back(kp);
        F.mvuRight.push_back(i % 3 == 0 ? -1.f : (float)(160.0 + 250.0 * P[0] / P[2] - 25.0 / P[2]));
        F.mvpMapPoints.push_back(i == 5 || i == 17 ? nullptr : &points[i]);
        F.mvbOutlier.push_back(i == 17 || i == 20);                   // a stale flag: kept where nothing is held, cleared where a point is
    }
    olf_ctx* ctx = nullptr;
    if (device) {
        olf_params p;
        olf_default_params(&p);
        p.orb.nfeatures = 236;
        expect(olf_ctx_create(&p, 320, 240, 2, &ctx) == OLF_OK, "olf_ctx_create");
    }
    int32_t status = -1;
    const int good = ORB_SLAM2::PoseOptimization(ctx, &F, &status);
    expect(status == 0 && F.poses_set == 1, "the frame ran through");
    bool near = F.mTcw.rows == 4 && F.mTcw.cols == 4;
    for (int r = 0; r < 3 && near; ++r) for (int c = 0; c < 4; ++c) near = near && std::fabs(F.mTcw.at<float>(r, c) - Tt[4 * r + c]) < 1e-4;
    expect(near, "SetPose received the true pose");
    int flagged = 0;
    for (int i = 0; i < 40; ++i) flagged += F.mvpMapPoints[i] && F.mvbOutlier[i];
    expect(F.mvbOutlier[9] && flagged == 1 && F.mvbOutlier[17] && !F.mvbOutlier[20], "point 9 alone is flagged; a feature that holds nothing keeps its flag");
    expect(good == 37, "nInitialCorrespondences - nBad");

    // fewer than three correspondences: 0, no SetPose, the held flags cleared (:364-365)
    Frame G = F;
    G.poses_set = 0;
    for (int i = 2; i < 40; ++i) G.mvpMapPoints[i] = nullptr;
    G.mvbOutlier[0] = true;
    expect(ORB_SLAM2::PoseOptimization(ctx, &G, &status) == 0 && status == 0 && G.poses_set == 0 && !G.mvbOutlier[0] && G.mvbOutlier[9], "two correspondences");
    if (ctx) olf_ctx_destroy(ctx);
    if (failures) return 1;
    std::printf("ADAPTOR_POSE_POINTS_OK\n");
    return 0;
}
