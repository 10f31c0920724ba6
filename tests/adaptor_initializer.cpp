// adaptor_initializer.cpp -- ORB_SLAM2::InitializerOf and InitializersInitialize (include/orbline_reference_api.hpp) against stand-in types: a reference
// frame of 112 key points and a current frame of 105 see 100 common points of a general scene under a known motion (0.05 rad about y, a translation
// along x), noise-free.
//   without an argument  the host form, no device: Initialize returns true with the motion, the points and the flags by reference feature; a second
//                        frame pair below eight matches returns false.  Prints ADAPTOR_INITIALIZER_OK.
//   with "device"        two more initialisers through InitializersInitialize on the thread's context, compared bit for bit with the host form's (the
//                        rand() stream is replayed: the adaptor seeds once per process and draws per call).
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
struct Point3f { float x, y, z; Point3f() : x(0), y(0), z(0) {} Point3f(float a, float b, float c) : x(a), y(b), z(c) {} };
struct Frame {
    Mat mK = Mat(3, 3);
    std::vector<KeyPoint> mvKeysUn;
    Frame() { mK.at<float>(0, 0) = 200.f; mK.at<float>(1, 1) = 200.f; mK.at<float>(0, 2) = 160.f; mK.at<float>(1, 2) = 120.f; mK.at<float>(2, 2) = 1.f; }
};
typedef ORB_SLAM2::InitializerOf<Frame> Initializer;

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float unit(uint32_t& s) { return (float)lcg(s) / 16777216.0f; }

int main(int argc, char** argv)
{
    const bool device = argc > 1 && !std::strcmp(argv[1], "device");
    const int N1 = 112, N2 = 105, N = 100;
    const float c = std::cos(0.05f), s = std::sin(0.05f), t[3] = {0.5f, 0.02f, 0.05f};
    Frame F1, F2;
    uint32_t seed = 99u;
    F1.mvKeysUn.resize(N1); F2.mvKeysUn.resize(N2);
    for (int i = 0; i < N1; ++i) { F1.mvKeysUn[i].x = 320.f * unit(seed); F1.mvKeysUn[i].y = 240.f * unit(seed); }
    for (int i = 0; i < N2; ++i) { F2.mvKeysUn[i].x = 320.f * unit(seed); F2.mvKeysUn[i].y = 240.f * unit(seed); }
    std::vector<int> matches(N1, -1);
    for (int q = 0; q < N; ++q) {
        const int i = q + q / 9, v = N2 - 1 - q;
        const float z = 3.f + 6.f * unit(seed), X[3] = {(unit(seed) - 0.5f) * z, (unit(seed) - 0.5f) * z * 0.7f, z};
        const double xc = (double)c * X[0] + (double)s * X[2] + t[0], yc = (double)X[1] + t[1], zc = -(double)s * X[0] + (double)c * X[2] + t[2];
        F1.mvKeysUn[i].x = (float)(200.0 * X[0] / X[2] + 160.0); F1.mvKeysUn[i].y = (float)(200.0 * X[1] / X[2] + 120.0);
        F2.mvKeysUn[v].x = (float)(200.0 * xc / zc + 160.0); F2.mvKeysUn[v].y = (float)(200.0 * yc / zc + 120.0);
        matches[i] = v;
    }

    Initializer init(F1, 1.0, 200);
    Mat R21, t21;
    std::vector<Point3f> vP3D;
    std::vector<bool> vbTriangulated;
    const bool ok = init.Initialize(F2, matches, R21, t21, vP3D, vbTriangulated);
    expect(ok && init.mNCorr == N && init.mModel == 2, "Initialize returns true from the fundamental matrix");
    expect(R21.rows == 3 && R21.cols == 3 && t21.rows == 3 && t21.cols == 1 && (int)vP3D.size() == N1 && (int)vbTriangulated.size() == N1, "the outputs have the reference's shapes");
    const float tn = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    if (ok)
        expect(std::fabs(R21.at<float>(0, 0) - c) < 1e-3f && std::fabs(R21.at<float>(0, 2) - s) < 1e-3f && std::fabs(t21.at<float>(0) - t[0] / tn) < 1e-2f &&
               std::fabs(t21.at<float>(2) - t[2] / tn) < 1e-2f, "the motion is recovered");
    int set = 0;
    for (int i = 0; i < N1 && ok; ++i) { set += vbTriangulated[i] ? 1 : 0; if (vbTriangulated[i]) expect(matches[i] >= 0 && vP3D[i].z > 0.f, "a triangulated feature is a match in front of the camera"); }
    expect(set >= 90 && ok && !vbTriangulated[9] && vP3D[9].z == 0.f, "the flags and points are by reference feature");
    expect(ok && init.mHypothesis >= 0 && init.olf_parallax(init.mHypothesis) > 1.0f && init.olf_parallax(init.mHypothesis) < 20.f, "the parallax in degrees comes from the stored cosine");

    std::vector<int> few(matches);
    for (int i = 7; i < N1; ++i) few[i] = -1;
    Mat R2, t2;
    std::vector<Point3f> p2;
    std::vector<bool> b2;
    expect(!init.Initialize(F2, few, R2, t2, p2, b2) && R2.empty() && init.mNCorr == 7, "fewer than eight matches: false");

    if (device) {
        // the host form again on the stream as it stands now, then the same draws through the device: rand() is replayed by re-seeding
        olf_ctx* ctx = ORB_SLAM2::olf_detail::thread_ctx();
        srand(5);
        Initializer h1(F1, 1.0, 200), h2(F1, 1.0, 200);
        Mat Ra, ta, Rb, tb;
        std::vector<Point3f> pa, pb;
        std::vector<bool> ba, bb;
        const bool oka = h1.Initialize(F2, matches, Ra, ta, pa, ba), okb = h2.Initialize(F2, few, Rb, tb, pb, bb);
        srand(5);
        Initializer d1(F1, 1.0, 200), d2(F1, 1.0, 200);
        std::vector<Initializer*> inits;
        inits.push_back(&d1); inits.push_back(&d2);
        std::vector<const Frame*> cur(2, &F2);
        std::vector<std::vector<int> > rows;
        rows.push_back(matches); rows.push_back(few);
        std::vector<bool> vok;
        std::vector<Mat> vR, vt;
        std::vector<std::vector<Point3f> > vp;
        std::vector<std::vector<bool> > vb;
        ORB_SLAM2::InitializersInitialize(ctx, inits, cur, rows, vok, vR, vt, vp, vb);
        expect(vok[0] == oka && oka && !std::memcmp(vR[0].d.data(), Ra.d.data(), 36) && !std::memcmp(vt[0].d.data(), ta.d.data(), 12) && vb[0] == ba &&
               !std::memcmp(vp[0].data(), pa.data(), sizeof(Point3f) * pa.size()) && d1.mScoreF == h1.mScoreF && d1.mHypothesis == h1.mHypothesis,
               "InitializersInitialize: the device equals the host form");
        expect(vok[1] == okb && !okb && vR[1].empty(), "InitializersInitialize: the pair below eight matches returns false");
    }
    if (failures) return 1;
    std::printf("ADAPTOR_INITIALIZER_OK\n");
    return 0;
}
