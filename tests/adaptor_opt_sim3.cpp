// adaptor_opt_sim3.cpp -- ORB_SLAM2::OptimizeSim3 (include/orbline_reference_api.hpp) against stand-in types with the members the reference's
// Optimizer::OptimizeSim3 reads and writes (src/Optimizer.cc:2013-2208).  Two key frames: 40 points of kf2 at 3-12 m seen exactly in both images under
// S12 = (s 1.25, a rotation of 2 degrees about y, t = (0.6, -0.3, 0.4)); the start is 2 % of scale, half a degree and 3 cm off.  Match 5 is NULL, match 9's
// point is 45 pixels off in image 2, match 17's point is not observed by kf2 and match 21's kf1 point is bad.  The optimiser must bring S12 to the true one,
// null match 9 and nothing else, and return 36.
//   without an argument  through the host form (no device).  Prints ADAPTOR_OPT_SIM3_OK.
//   with "device"        through olf_optimize_sim3_pairs on a context made for the key frames; the same checks.
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
struct KeyFrame;
struct MapPoint {
    Mat w;
    bool bad = false;
    KeyFrame* kf = nullptr;
    int idx = -1;
    Mat GetWorldPos() { return w; }
    bool isBad() { return bad; }
    int GetIndexInKeyFrame(KeyFrame* p) { return p == kf ? idx : -1; }
};
struct KeyFrame {
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    Mat Tcw;
    float fx = 250.f, fy = 250.f, cx = 160.f, cy = 120.f;
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    Mat GetPose() { return Tcw; }
};
struct Quat {                                                        // Eigen::Quaterniond's constructor order and accessors
    double qw, qx, qy, qz;
    Quat(double w_, double x_, double y_, double z_) : qw(w_), qx(x_), qy(y_), qz(z_) {}
    double x() const { return qx; } double y() const { return qy; } double z() const { return qz; } double w() const { return qw; }
};
struct Vec3 {
    double v[3];
    Vec3(double a, double b, double c) { v[0] = a; v[1] = b; v[2] = c; }
    double operator[](int i) const { return v[i]; }
};
struct Sim3 {                                                        // g2o::Sim3
    Quat r; Vec3 t; double s;
    Sim3(const Quat& r_, const Vec3& t_, double s_) : r(r_), t(t_), s(s_) {}
    const Quat& rotation() const { return r; }
    const Vec3& translation() const { return t; }
    const double& scale() const { return s; }
};

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static unsigned lcg = 4321u;
static double uni(double a, double b) { lcg = lcg * 1664525u + 1013904223u; return a + (b - a) * ((lcg >> 8) / 16777216.0); }
static Quat quat_y(double deg) { const double h = 0.5 * deg * 3.14159265358979323846 / 180.0; return Quat(std::cos(h), 0.0, std::sin(h), 0.0); }

int main(int argc, char** argv)
{
    const bool device = argc > 1 && !std::strcmp(argv[1], "device");
    const int N = 40;
    const double a = 2.0 * 3.14159265358979323846 / 180.0, s_true = 1.25, t_true[3] = {0.6, -0.3, 0.4};
    KeyFrame K1, K2;
    float sf = 1.f;
    for (int l = 0; l < 8; ++l) { K1.mvInvLevelSigma2.push_back(1.0f / (sf * sf)); sf = (float)(sf * 1.2); }
    K2.mvInvLevelSigma2 = K1.mvInvLevelSigma2;
    K1.Tcw = Mat(4, 4, 5); K2.Tcw = Mat(4, 4, 5);
    for (int i = 0; i < 4; ++i) { K1.Tcw.at<float>(i, i) = 1.f; K2.Tcw.at<float>(i, i) = 1.f; }      // both poses the identity: world = camera frame
    std::vector<MapPoint> p1(N), p2(N);
    std::vector<MapPoint*> matches(N);
    K2.mvKeysUn.resize(N + 3);
    for (int i = 0; i < N; ++i) {
        const double z = uni(3, 12), X2[3] = {uni(-0.5, 0.5) * z, uni(-0.35, 0.35) * z, z};
        const double X2f[3] = {(double)(float)X2[0], (double)(float)X2[1], (double)(float)X2[2]};
        const double X1[3] = {s_true * (std::cos(a) * X2f[0] + std::sin(a) * X2f[2]) + t_true[0], s_true * X2f[1] + t_true[1],
                              s_true * (-std::sin(a) * X2f[0] + std::cos(a) * X2f[2]) + t_true[2]};
        p1[i].w = Mat(3, 1, 5); p2[i].w = Mat(3, 1, 5);
        for (int k = 0; k < 3; ++k) { p1[i].w.at<float>(k, 0) = (float)X1[k]; p2[i].w.at<float>(k, 0) = (float)X2[k]; }
        const int i2 = (i * 7 + 3) % N + 3;                          // where kf2 observes the point
        p1[i].kf = &K1; p1[i].idx = i; p2[i].kf = &K2; p2[i].idx = i == 17 ? -1 : i2;
        KeyPoint k1, k2;
        k1.x = (float)(160.0 + 250.0 * X1[0] / X1[2]); k1.y = (float)(120.0 + 250.0 * X1[1] / X1[2]); k1.octave = i % 8;
        k2.x = (float)(160.0 + 250.0 * X2f[0] / X2f[2]) + (i == 9 ? 45.f : 0.f); k2.y = (float)(120.0 + 250.0 * X2f[1] / X2f[2]); k2.octave = (i + 3) % 8;
        K1.mvKeysUn.push_back(k1);
        K2.mvKeysUn[i2] = k2;
        K1.mvpMapPoints.push_back(&p1[i]);
        matches[i] = i == 5 ? nullptr : &p2[i];
    }
    p1[21].bad = true;
    // the start: S12 = dS * S_true with dS = (1.02, half a degree about y, 3 cm)
    const Quat qt = quat_y(2.0), qd = quat_y(0.5);
    const Quat q0(qd.qw * qt.qw - qd.qy * qt.qy, 0.0, qd.qw * qt.qy + qd.qy * qt.qw, 0.0);
    const double b = 0.5 * 3.14159265358979323846 / 180.0;
    Sim3 S12(q0, Vec3(1.02 * (std::cos(b) * t_true[0] + std::sin(b) * t_true[2]) + 0.02, 1.02 * t_true[1] - 0.02, 1.02 * (-std::sin(b) * t_true[0] + std::cos(b) * t_true[2]) + 0.01),
             1.02 * s_true);
    olf_ctx* ctx = nullptr;
    if (device) {
        olf_params p;
        olf_default_params(&p);
        p.orb.nfeatures = 236;
        expect(olf_ctx_create(&p, 320, 240, 2, &ctx) == OLF_OK, "olf_ctx_create");
    }
    int32_t status = -1;
    std::vector<MapPoint*> m = matches;
    const int nIn = ORB_SLAM2::OptimizeSim3(ctx, &K1, &K2, m, S12, 10.f, false, &status);
    expect(status == 0, "the pair ran through");
    expect(nIn == 36, "nIn");
    int nulled = 0;
    for (int i = 0; i < N; ++i) nulled += matches[i] && !m[i];
    expect(!m[9] && nulled == 1 && m[17] == matches[17] && m[21] == matches[21] && !m[5], "match 9 alone is nulled; entries that are no correspondence keep their value");
    expect(std::fabs(S12.scale() - s_true) < 1e-3 && std::fabs(S12.translation()[0] - t_true[0]) < 2e-3 && std::fabs(S12.translation()[1] - t_true[1]) < 2e-3 &&
           std::fabs(S12.translation()[2] - t_true[2]) < 2e-3 && std::fabs(S12.rotation().y() - qt.qy) < 1e-4 && std::fabs(S12.rotation().w() - qt.qw) < 1e-4,
           "g2oS12 received the true similarity");

    // fewer than ten correspondences: 0 and g2oS12 as it was (:2178-2179)
    std::vector<MapPoint*> few = matches;
    for (int i = 8; i < N; ++i) few[i] = nullptr;
    Sim3 S0(q0, Vec3(0.5, -0.25, 0.5), 1.3);
    expect(ORB_SLAM2::OptimizeSim3(ctx, &K1, &K2, few, S0, 10.f, true, &status) == 0 && status == 0 && S0.scale() == 1.3 && S0.translation()[0] == 0.5, "seven correspondences");
    if (ctx) olf_ctx_destroy(ctx);
    if (failures) return 1;
    std::printf("ADAPTOR_OPT_SIM3_OK\n");
    return 0;
}
