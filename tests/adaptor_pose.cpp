// adaptor_pose.cpp -- ORB_SLAM2::PoseOptimizationWithLine (include/orbline_reference_api.hpp) against stand-in types with the members the reference's
// Optimizer::PoseOptimizationWithLine reads and writes (src/Optimizer.cc:604-697).  One frame: 40 points and 12 segments at 3-12 m seen exactly by a
// camera that moved 4 cm and 0.3 degrees since the previous frame, the prior being the previous pose; features 5 and 17 hold nothing, point 9 is seen
// 40 pixels off.  The optimiser must bring the pose from 4 cm off to within a millimetre of the true one (its ten rounds a pass do not converge further), flag point 9 and nothing that holds nothing, and count the rest.
//   without an argument  through the host form (no device).  Prints ADAPTOR_POSE_OK.
//   with "device"        through olf_pose_optimization_with_line_frame on a context made for the frame; the same checks.
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
template <int R, int C> struct Mx {                                  // Eigen::Matrix<double, R, C> as far as it is read and written
    double v[R * C] = {0};
    double& operator()(int r, int c) { return v[r * C + c]; }
    double& operator()(int i) { return v[i]; }
    double& operator[](int i) { return v[i]; }
};
struct KeyPoint { float x = 0, y = 0, size = 0, angle = -1, response = 0; int octave = 0, class_id = -1; };
struct KeyLine { float angle = 0; int class_id = 0, octave = 0; float pt_x = 0, pt_y = 0, response = 0, size = 0, startPointX = 0, startPointY = 0, endPointX = 0, endPointY = 0,
                 sPointInOctaveX = 0, sPointInOctaveY = 0, ePointInOctaveX = 0, ePointInOctaveY = 0, lineLength = 0; int numOfPixels = 0; };
struct MapPoint { Mat w; Mat GetWorldPos() { return w; } };
struct MapLine { Mx<3, 1> mWorldPos_sP, mWorldPos_eP; };
struct Frame {
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<KeyLine> mvKeysUn_Line;
    std::vector<Mx<3, 1>> mvle_l;
    std::vector<bool> mvbOutlier, mvbOutlier_Line;
    std::vector<float> mvInvLevelSigma2;
    Mat mTcw, mTcw_prev;
    Mx<4, 4> DT;
    Mx<6, 6> DT_cov;
    Mx<6, 1> DT_cov_eig;
    double err_norm = 0;
    int n_inliers = 0, n_inliers_pt = 0, n_inliers_ls = 0;
    float fx = 250.f, fy = 250.f, cx = 160.f, cy = 120.f;
    void SetPose(const Mat& T) { mTcw = T; }
};

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static unsigned lcg = 12345u;
static double uni(double a, double b) { lcg = lcg * 1664525u + 1013904223u; return a + (b - a) * ((lcg >> 8) / 16777216.0); }

int main(int argc, char** argv)
{
    const bool device = argc > 1 && !std::strcmp(argv[1], "device");
    // the previous pose is the identity; the true pose: a rotation of 0.3 degrees about y and 4 cm along x
    const double a = 0.3 * 3.14159265358979323846 / 180.0;
    const double Tt[12] = {std::cos(a), 0, std::sin(a), 0.04, 0, 1, 0, 0.0, -std::sin(a), 0, std::cos(a), 0.01};
    auto see = [&](const double* X, double* uv) {
        const double P[3] = {Tt[0] * X[0] + Tt[1] * X[1] + Tt[2] * X[2] + Tt[3], Tt[4] * X[0] + Tt[5] * X[1] + Tt[6] * X[2] + Tt[7], Tt[8] * X[0] + Tt[9] * X[1] + Tt[10] * X[2] + Tt[11]};
        uv[0] = 160.0 + 250.0 * P[0] / P[2]; uv[1] = 120.0 + 250.0 * P[1] / P[2];
    };
    Frame F;
    F.mvInvLevelSigma2.resize(8);
    float sf = 1.f;
    for (int l = 0; l < 8; ++l) { F.mvInvLevelSigma2[l] = 1.0f / (sf * sf); sf = (float)(sf * 1.2); }
    F.mTcw_prev = Mat(4, 4, 5);
    for (int i = 0; i < 4; ++i) F.mTcw_prev.at<float>(i, i) = 1.f;
    F.mTcw = F.mTcw_prev;
    std::vector<MapPoint> points(40);
    std::vector<MapLine> lines(12);
    for (int i = 0; i < 40; ++i) {
        const double z = uni(3, 12), X[3] = {uni(-0.5, 0.5) * z, uni(-0.35, 0.35) * z, z};
        double uv[2];
        points[i].w = Mat(3, 1, 5);
        for (int k = 0; k < 3; ++k) points[i].w.at<float>(k, 0) = (float)X[k];
        const double Xf[3] = {(double)(float)X[0], (double)(float)X[1], (double)(float)X[2]};
        see(Xf, uv);
        KeyPoint kp;
        kp.x = (float)uv[0] + (i == 9 ? 40.f : 0.f); kp.y = (float)uv[1]; kp.octave = i % 8;
        F.mvKeysUn.push_back(kp);
        F.mvpMapPoints.push_back(i == 5 || i == 17 ? nullptr : &points[i]);
        F.mvbOutlier.push_back(i == 17);                               // a stale flag on a feature that holds nothing stays as it is
    }
    for (int i = 0; i < 12; ++i) {
        const double zs = uni(3, 12), ze = uni(3, 12), S[3] = {uni(-0.4, 0.0) * zs, uni(-0.3, 0.0) * zs, zs}, E[3] = {uni(0.05, 0.4) * ze, uni(0.05, 0.3) * ze, ze};
        double s[2], e[2];
        for (int k = 0; k < 3; ++k) { lines[i].mWorldPos_sP[k] = (double)(float)S[k]; lines[i].mWorldPos_eP[k] = (double)(float)E[k]; }
        see(lines[i].mWorldPos_sP.v, s); see(lines[i].mWorldPos_eP.v, e);
        KeyLine kl;
        kl.startPointX = (float)s[0]; kl.startPointY = (float)s[1]; kl.endPointX = (float)e[0]; kl.endPointY = (float)e[1]; kl.octave = i % 8;
        F.mvKeysUn_Line.push_back(kl);
        const double sx = kl.startPointX, sy = kl.startPointY, ex = kl.endPointX, ey = kl.endPointY;      // mvle_l, src/Frame.cc:939-941
        const double l[3] = {sy - ey, ex - sx, sx * ey - sy * ex}, n = std::sqrt(l[0] * l[0] + l[1] * l[1]);
        Mx<3, 1> le;
        for (int k = 0; k < 3; ++k) le[k] = l[k] / n;
        F.mvle_l.push_back(le);
        F.mvpMapLines.push_back(i == 5 ? nullptr : &lines[i]);
        F.mvbOutlier_Line.push_back(false);
    }
    olf_ctx* ctx = nullptr;
    if (device) {
        olf_params p;
        olf_default_params(&p);
        p.orb.nfeatures = 300; p.line.lsd_nfeatures = 150;
        expect(olf_ctx_create(&p, 320, 240, 2, &ctx) == OLF_OK, "olf_ctx_create");
    }
    int32_t status = -1;
    expect(ORB_SLAM2::PoseOptimizationWithLine(ctx, &F, nullptr, &status), "PoseOptimizationWithLine returns true");
    expect(status == 0, "the frame ran through");
    bool near = F.mTcw.rows == 4 && F.mTcw.cols == 4;
    for (int r = 0; r < 3 && near; ++r) for (int c = 0; c < 4; ++c) near = near && std::fabs(F.mTcw.at<float>(r, c) - Tt[4 * r + c]) < 1e-3;
    expect(near, "SetPose received the true pose");
    expect(std::fabs(F.DT(0, 3) + 0.04) < 5e-4 && std::fabs(F.DT(0, 0) - std::cos(a)) < 1e-5 && F.DT(3, 3) == 1.0, "DT is the inverse of the motion");
    expect(F.mvbOutlier[9] && F.mvbOutlier[17] && !F.mvbOutlier[5], "point 9 is flagged; the features that hold nothing keep their flags");
    int flagged = 0, lflagged = 0;
    for (int i = 0; i < 40; ++i) flagged += F.mvpMapPoints[i] && F.mvbOutlier[i];
    for (int i = 0; i < 12; ++i) lflagged += F.mvpMapLines[i] && F.mvbOutlier_Line[i];
    expect(F.n_inliers_pt == 38 - flagged && F.n_inliers_ls == 11 - lflagged && F.n_inliers == F.n_inliers_pt + F.n_inliers_ls, "n_inliers count the held features that are not flagged");
    expect(F.err_norm >= 0.0 && F.err_norm < 1.0 && F.DT_cov_eig(0) > 0.0 && F.DT_cov_eig(5) >= F.DT_cov_eig(0) && F.DT_cov(0, 0) > 0.0, "err_norm, DT_cov and its eigenvalues are set");

    // an empty previous pose is the pose itself (:613-614): the motion prior is the identity and the result is relative to mTcw
    Frame G = F;
    G.mTcw = F.mTcw_prev; G.mTcw_prev = Mat();
    for (size_t i = 0; i < G.mvbOutlier.size(); ++i) G.mvbOutlier[i] = false;
    expect(ORB_SLAM2::PoseOptimizationWithLine(ctx, &G, nullptr, &status) && status == 0, "empty mTcw_prev");
    near = true;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) near = near && std::fabs(G.mTcw.at<float>(r, c) - Tt[4 * r + c]) < 1e-3;
    expect(near, "empty mTcw_prev: the true pose again");

    // a frame that holds nothing stops with status 1 and keeps its pose
    Frame E = F;
    for (size_t i = 0; i < E.mvpMapPoints.size(); ++i) E.mvpMapPoints[i] = nullptr;
    for (size_t i = 0; i < E.mvpMapLines.size(); ++i) E.mvpMapLines[i] = nullptr;
    const Mat before = E.mTcw;
    expect(ORB_SLAM2::PoseOptimizationWithLine(ctx, &E, nullptr, &status) && status == 1 && E.mTcw.d == before.d && E.err_norm == -1.0 && E.n_inliers == 0, "a frame that holds nothing");
    if (ctx) olf_ctx_destroy(ctx);
    if (failures) return 1;
    std::printf("ADAPTOR_POSE_OK\n");
    return 0;
}
