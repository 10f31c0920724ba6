// pose_host_main.cpp -- the host forms of the pose optimiser (csrc/pose_host.cpp over pose_terms.hpp) as a stand-alone program, so that they can run under
// AddressSanitizer / UBSan in a process of their own (tests/test_pose_cpu.py builds it with -fsanitize=address,undefined).  Two frames written out as
// arrays (tests/pose_scenes.py: make_scene(501, 8, 4, extra_points=2, extra_lines=1) and make_scene(431, 5, 0), whose five points all become outliers, so
// the frame stops with status 1); the rows are allocated at exactly their lengths, so a read or write past a count is an error the sanitizer reports.
// Prints POSE_HOST_OK.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../include/orbline.h"

namespace olf { void set_error(const std::string& s) { std::printf("error: %s\n", s.c_str()); } }

// scene a: 10 key points, 5 key lines
static const float a_kp_xy[] = {299.062042f, 135.907852f, 239.511566f, 82.5613022f, 150.564789f, 165.852249f, 182.384094f, 88.2677994f, 118.724899f, 66.4105148f, 145.959091f, 140.795807f, 20.1198406f, 199.939301f, 267.773895f, 185.471176f, 105.083565f, 40.9221725f, 75.8043365f, 168.118591f};
static const int a_kp_octave[] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1};
static const float a_kl_ends[] = {88.1430893f, 105.447624f, 88.1430893f, 161.058914f, 96.8821716f, 51.2053032f, 158.611282f, 51.2053032f, 100.602341f, 118.064667f, 128.514008f, 153.441483f, 77.9445267f, 61.668045f, 77.9445267f, 103.079781f, 153.981567f, 137.012146f, 191.372772f, 137.012146f};
static const int a_kl_octave[] = {0, 1, 2, 3, 4};
static const double a_lle[] = {-1, 0, 88.143089294433594, 0, 1, -51.205303192138672, -0.78507050644452325, 0.61940640932342628, 5.8499192630988235, -1, 0, 77.944526672363281, 0, 1, -137.01214599609375};
static const float a_Tcw[] = {0.985631764f, 0.16714485f, 0.0243432671f, -0.943362296f, -0.168835387f, 0.979153752f, 0.11292699f, 0.521766543f, -0.00496063661f, -0.115414433f, 0.993305027f, 0.306262761f, 0.f, 0.f, 0.f, 1.f};
static const float a_Tcw_prev[] = {0.984453738f, 0.17377831f, 0.0255330931f, -0.966927171f, -0.175568417f, 0.977843106f, 0.114011399f, 0.517675698f, -0.00515465159f, -0.116721749f, 0.993151307f, 0.311810255f, 0.f, 0.f, 0.f, 1.f};
static const int a_frame_mp[] = {0, 1, 2, 3, 4, 5, 6, -1, 7, -1};
static const float a_mp_world[] = {5.15512514f, 0.0285696071f, 7.48478556f, 5.80557871f, -3.29544115f, 13.6166868f, 0.259152085f, 0.39943853f, 11.4841061f, 1.37146986f, -1.06514812f, 2.94689226f, -0.2522268f, -3.72052693f, 8.9618454f, 0.294151008f, -0.789331675f, 10.414979f, -2.0658443f, 0.249225199f, 4.81021547f, -0.00568374805f, -3.111449f, 5.41287994f};
static const int a_frame_ml[] = {-1, 0, 1, 2, 3};
static const float a_ml_world[] = {0.296965986f, -1.77605355f, 2.93766713f, 1.14608753f, -1.77981532f, 3.31977248f, -1.69084382f, -2.19684649f, 10.71311f, -0.199058041f, -0.34970215f, 7.81830549f, -2.30120945f, -4.86519289f, 10.6244507f, -2.68292546f, -3.06145453f, 11.0227938f, 0.528716564f, -0.937611699f, 11.4336395f, 2.55485511f, -0.689946711f, 13.544837f};
static const unsigned char a_want_outlier[] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static const unsigned char a_want_outlier_l[] = {0, 0, 0, 0, 0};
static const int a_n = 10, a_nl = 5, a_n_mp = 8, a_n_ml = 4, a_want_status = 0, a_want_inliers[2] = {8, 4};
static const double a_want_err = 0.17893468521084618;

// scene b: 5 key points, 0 key lines
static const float b_kp_xy[] = {238.071075f, 70.964859f, 296.926025f, 197.555847f, 188.317291f, 50.1275749f, 47.0547256f, 129.118179f, 24.8010426f, 113.57534f};
static const int b_kp_octave[] = {0, 1, 2, 3, 4};
static const float b_kl_ends[] = {0};
static const int b_kl_octave[] = {0};
static const double b_lle[] = {0};
static const float b_Tcw[] = {0.981562674f, -0.188960344f, 0.0287864823f, 1.04341972f, 0.191123411f, 0.968268991f, -0.16101855f, -0.736969233f, 0.00255306228f, 0.163551569f, 0.986531496f, 0.507344544f, 0.f, 0.f, 0.f, 1.f};
static const float b_Tcw_prev[] = {0.981490493f, -0.189939976f, 0.0244800542f, 0.997164845f, 0.191338599f, 0.967139781f, -0.167422041f, -0.732320487f, 0.00812450238f, 0.169007123f, 0.985581338f, 0.498268813f, 0.f, 0.f, 0.f, 1.f};
static const int b_frame_mp[] = {0, 1, 2, 3, 4};
static const float b_mp_world[] = {2.29064059f, -0.154920459f, 10.981451f, 3.47398305f, 3.41291666f, 6.15431309f, -0.481487513f, 0.101414837f, 5.0985899f, -5.6310873f, 3.91704726f, 10.0579243f, -7.93228388f, 4.07475233f, 12.4019785f};
static const int b_frame_ml[] = {0};
static const float b_ml_world[] = {0};
static const unsigned char b_want_outlier[] = {1, 1, 1, 1, 1};
static const unsigned char b_want_outlier_l[] = {0};
static const int b_n = 5, b_nl = 0, b_n_mp = 5, b_n_ml = 0, b_want_status = 1, b_want_inliers[2] = {0, 0};
static const double b_want_err = -1;

static const float inv_level_sigma2[] = {1.f, 0.694444418f, 0.482253075f, 0.334897906f, 0.232567981f, 0.161505535f, 0.112156615f, 0.0778865293f};

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

struct Outputs {
    float Tcw[16]; double DT[16], cov[36], eig[6], err; uint8_t good; int32_t inl[2], iters[4], status;
    std::vector<uint8_t> out, outl;
};

static void run(int n, int nl, const float* kp_xy, const int* kp_octave, const float* kl_ends, const int* kl_octave, const double* lle, const float* Tcw,
                const float* Tcw_prev, const int* frame_mp, const float* mp_world, int n_mp, const int* frame_ml, const float* ml_world, int n_ml, Outputs* o)
{
    std::vector<olf_keypoint> kps(n);
    std::vector<olf_keyline> kls(nl);
    for (int i = 0; i < n; ++i) { std::memset(&kps[i], 0, sizeof(olf_keypoint)); kps[i].x = kp_xy[2 * i]; kps[i].y = kp_xy[2 * i + 1]; kps[i].octave = kp_octave[i]; }
    for (int i = 0; i < nl; ++i) {
        std::memset(&kls[i], 0, sizeof(olf_keyline));
        kls[i].startPointX = kl_ends[4 * i]; kls[i].startPointY = kl_ends[4 * i + 1]; kls[i].endPointX = kl_ends[4 * i + 2]; kls[i].endPointY = kl_ends[4 * i + 3];
        kls[i].octave = kl_octave[i];
    }
    std::vector<int32_t> fmp(frame_mp, frame_mp + n), fml(frame_ml, frame_ml + nl);
    std::vector<double> le(lle, lle + 3 * nl);
    std::vector<float> mpw(mp_world, mp_world + 3 * n_mp), mlw(ml_world, ml_world + 6 * n_ml);
    const int32_t counts[1] = {n}, lcounts[1] = {nl};
    olf_pose_batch in;
    std::memset(&in, 0, sizeof(in));
    in.kps = kps.data(); in.counts = counts; in.kls = kls.data(); in.lcounts = lcounts; in.img_stride = 1; in.lle = le.data();
    in.Tcw = Tcw; in.Tcw_prev = Tcw_prev; in.fx = 250.f; in.fy = 250.f; in.cx = 160.f; in.cy = 120.f;
    in.frame_mp = fmp.data(); in.mp_world = mpw.data(); in.n_mp = n_mp; in.frame_ml = fml.data(); in.ml_world = mlw.data(); in.n_ml = n_ml;
    o->out.assign(n, 7); o->outl.assign(nl, 7);
    olf_pose_outputs out = {o->Tcw, o->DT, o->cov, o->eig, &o->err, &o->good, o->out.data(), o->outl.data(), o->inl, o->iters, &o->status};
    olf_pose_params p;
    olf_pose_default_params(&p);
    CHECK(olf_pose_optimization_with_line(&in, n, nl, inv_level_sigma2, 8, &p, &out) == OLF_OK);

    // the loops after the call, on the rows it wrote: mode 0 on a copy, mode 1 on another
    for (int mode = 0; mode < 2; ++mode) {
        std::vector<int32_t> hp(fmp), hl(fml);
        std::vector<uint8_t> fo(o->out), fl(o->outl), obs(n_mp, 1), lobs(n_ml, 1);
        olf_discard_batch d;
        std::memset(&d, 0, sizeof(d));
        d.counts = counts; d.lcounts = lcounts; d.img_stride = 1; d.frame_mp = hp.data(); d.frame_ml = hl.data(); d.outlier = fo.data(); d.outlier_l = fl.data();
        d.mp_obs = obs.data(); d.ml_obs = lobs.data(); d.n_mp = n_mp; d.n_ml = n_ml;
        int32_t nm[2] = {-1, -1}, st = -1;
        CHECK(olf_discard_outliers(&d, n, nl, mode, 0, 1, nm, &st) == OLF_OK);
        CHECK(st == 0 && nm[0] == o->inl[0] && nm[1] == o->inl[1]);
        for (int i = 0; i < n; ++i) CHECK((hp[i] < 0) == (fmp[i] < 0 || o->out[i]));
        for (int i = 0; i < nl; ++i) CHECK((hl[i] < 0) == (fml[i] < 0 || o->outl[i]));
    }
}

int main()
{
    Outputs a, b;
    run(a_n, a_nl, a_kp_xy, a_kp_octave, a_kl_ends, a_kl_octave, a_lle, a_Tcw, a_Tcw_prev, a_frame_mp, a_mp_world, a_n_mp, a_frame_ml, a_ml_world, a_n_ml, &a);
    CHECK(a.status == a_want_status && a.inl[0] == a_want_inliers[0] && a.inl[1] == a_want_inliers[1]);
    CHECK(std::fabs(a.err - a_want_err) <= 1e-9 * std::fabs(a_want_err));
    for (int i = 0; i < a_n; ++i) CHECK(a.out[i] == a_want_outlier[i]);
    for (int i = 0; i < a_nl; ++i) CHECK(a.outl[i] == a_want_outlier_l[i]);
    for (int i = 0; i < 16; ++i) CHECK(std::isfinite(a.DT[i]) && std::isfinite(a.Tcw[i]));

    run(b_n, b_nl, b_kp_xy, b_kp_octave, b_kl_ends, b_kl_octave, b_lle, b_Tcw, b_Tcw_prev, b_frame_mp, b_mp_world, b_n_mp, b_frame_ml, b_ml_world, b_n_ml, &b);
    CHECK(b.status == b_want_status && b.status == 1 && b.inl[0] == 0 && b.inl[1] == 0 && b.err == -1.0 && b.good == 0);
    for (int i = 0; i < b_n; ++i) CHECK(b.out[i] == b_want_outlier[i]);
    for (int i = 0; i < 16; ++i) CHECK(b.Tcw[i] == b_Tcw[i] && b.DT[i] == (i % 5 == 0 ? 1.0 : 0.0));      // the pose goes through unchanged
    for (int i = 0; i < 36; ++i) CHECK(b.cov[i] == 0.0);

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("POSE_HOST_OK\n");
    return 0;
}
