// optsim3_host_main.cpp -- the host form of Optimizer::OptimizeSim3 (csrc/optsim3_host.cpp over optsim3_terms.hpp) as a stand-alone program, so that it can
// run under AddressSanitizer and UBSan without a Python process around it.  Pairs of 0, 1, 9, 12, 64 and 300 correspondences (every seventh entry is
// none, one gross outlier from 12 on), rows exactly as long as the count, both scale modes, a refused pair, a depth of 0, an octave outside the levels and
// the numeric Jacobian's debug entry.  Prints OPTSIM3_HOST_OK.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../include/orbline.h"

namespace olf { void set_error(const std::string&) {} }              // (the library's error slot; this program links the host source alone)

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static unsigned lcg = 77u;
static double uni(double a, double b) { lcg = lcg * 1664525u + 1013904223u; return a + (b - a) * ((lcg >> 8) / 16777216.0); }

int main()
{
    float sig[8], sf = 1.f;
    for (int l = 0; l < 8; ++l) { sig[l] = 1.0f / (sf * sf); sf = (float)(sf * 1.2); }
    const double s_true = 1.2, t_true[3] = {0.5, -0.4, 0.3};
    const int sizes[6] = {0, 1, 9, 12, 64, 300};
    for (int n : sizes) for (int fix = 0; fix < 2; ++fix) {
        // two key frames with identity poses, rows exactly n long: feature i of kf1 matches feature n - 1 - i of kf2
        std::vector<olf_keypoint> kps(2 * (size_t)n);
        std::vector<float> world(2 * 3 * (size_t)n, 0.f), chi2(2 * (size_t)n);
        std::vector<int32_t> m((size_t)n, -1);
        const int32_t counts[2] = {n, n};
        int corr = 0;
        for (int i = 0; i < n; ++i) {
            const int j = n - 1 - i;
            const double z = uni(3, 12), X2[3] = {uni(-0.5, 0.5) * z, uni(-0.35, 0.35) * z, z};
            for (int k = 0; k < 3; ++k) { world[3 * ((size_t)n + j) + k] = (float)X2[k]; world[3 * (size_t)i + k] = (float)((fix ? 1.0 : s_true) * (double)(float)X2[k] + t_true[k]); }
            const float* P1 = &world[3 * (size_t)i];
            const float* P2 = &world[3 * ((size_t)n + j)];
            std::memset(&kps[i], 0, sizeof(olf_keypoint)); std::memset(&kps[(size_t)n + j], 0, sizeof(olf_keypoint));
            kps[i].x = (float)(160.0 + 250.0 * P1[0] / P1[2]) + (i == 4 && n >= 12 ? 50.f : 0.f); kps[i].y = (float)(120.0 + 250.0 * P1[1] / P1[2]); kps[i].octave = i % 8;
            kps[(size_t)n + j].x = (float)(160.0 + 250.0 * P2[0] / P2[2]); kps[(size_t)n + j].y = (float)(120.0 + 250.0 * P2[1] / P2[2]); kps[(size_t)n + j].octave = (i + 5) % 8;
            if (i % 7 != 3) { m[i] = j; ++corr; }
        }
        float T[32];
        std::memset(T, 0, sizeof T);
        for (int f = 0; f < 2; ++f) for (int i = 0; i < 4; ++i) T[16 * f + 5 * i] = 1.f;
        olf_track_batch in;
        std::memset(&in, 0, sizeof(in));
        in.kps = kps.data(); in.counts = counts; in.img_stride = 1; in.Tcw = T; in.mp_world = world.data(); in.fx = 250.f; in.fy = 250.f; in.cx = 160.f; in.cy = 120.f;
        const float R12[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t12[3] = {(float)t_true[0] + 0.02f, (float)t_true[1] - 0.01f, (float)t_true[2] + 0.02f};
        const float s12 = fix ? 1.0f : (float)(s_true * 1.02);
        double S[8];
        float so, Ro[9], to[3], Scw[16];
        int32_t nin = -7, ncorr = -7, nbad = -7, iters[2], status = -7;
        std::vector<int32_t> row = m;
        olf_optimize_sim3_io io = {row.data(), S, &so, Ro, to, Scw, &nin, &ncorr, &nbad, iters, &status, chi2.data()};
        CHECK(olf_optimize_sim3(&in, n, 2, nullptr, sig, 8, 0, 1, s12, R12, t12, 10.f, fix, &io) == OLF_OK);
        CHECK(ncorr == corr && status == 0);
        if (corr < 10) { CHECK(nin == 0 && S[7] == (double)s12 && S[4] == (double)t12[0] && S[3] == 1.0); }
        else if (n >= 64) {
            CHECK(nbad == 1 && row[4] == -1 && nin == corr - 1 && iters[1] > 0);
            CHECK(std::fabs(S[7] - (fix ? 1.0 : s_true)) < 1e-3 && std::fabs(S[4] - t_true[0]) < 2e-3 && std::fabs(S[6] - t_true[2]) < 2e-3);
            CHECK(std::fabs(Scw[3] - (float)S[4]) < 1e-6f && Scw[15] == 1.f);
            for (int i = 0; i < n; ++i) CHECK(row[i] == (i == 4 ? -1 : m[i]));
        }
        if (n == 64 && !fix) {
            row = m;
            CHECK(olf_optimize_sim3(&in, n, 2, nullptr, sig, 8, 1, 1, s12, R12, t12, 10.f, fix, &io) == OLF_OK && nin == -1 && status == 2048 && row == m);
            CHECK(olf_optimize_sim3(&in, n, 2, nullptr, sig, 8, 0, 2, s12, R12, t12, 10.f, fix, &io) == OLF_OK && nin == -1 && status == 2048);
            CHECK(olf_optimize_sim3(&in, n, 2, nullptr, sig, 8, 0, 1, s12, R12, t12, 0.f, fix, &io) == OLF_ERR_INVALID);
            kps[9].octave = 8;                                         // outside the levels: left out
            CHECK(olf_optimize_sim3(&in, n, 2, nullptr, sig, 8, 0, 1, s12, R12, t12, 10.f, fix, &io) == OLF_OK && status == 4 && ncorr == corr - 1 && row[9] == m[9]);
            kps[9].octave = 1;
            row = m;
            const float t0[3] = {0.f, 0.f, 0.f};
            world[3 * ((size_t)n + m[6]) + 2] = 0.f;                   // a depth of exactly 0 under the identity
            CHECK(olf_optimize_sim3(&in, n, 2, nullptr, sig, 8, 0, 1, 1.0f, R12, t0, 10.f, fix, &io) == OLF_OK && status == 1 && nin == 0 && S[7] == 1.0 && S[4] == 0.0 && row == m);
        }
    }
    const double S12[8] = {0.01, -0.02, 0.015, 0.9996, 0.3, -0.2, 0.1, 1.2}, cam[4] = {250, 250, 160, 120}, X[3] = {0.4, -0.3, 5.0}, obs[2] = {170.0, 110.0};
    double J[14], J6[14];
    CHECK(olf_debug_optimize_sim3_jacobian(S12, 0, cam, X, obs, 1, J) == OLF_OK && olf_debug_optimize_sim3_jacobian(S12, 1, cam, X, obs, 1, J6) == OLF_OK);
    CHECK(J[3] != 0.0 && J[6] != 0.0 && J6[6] == 0.0 && J6[13] == 0.0);
    CHECK(olf_debug_optimize_sim3_jacobian(nullptr, 0, cam, X, obs, 0, J) == OLF_ERR_INVALID);
    CHECK(olf_optimize_sim3(nullptr, 0, 1, nullptr, sig, 8, 0, 1, 1.f, nullptr, nullptr, 10.f, 0, nullptr) == OLF_ERR_INVALID);
    std::printf("OPTSIM3_HOST_OK\n");
    return 0;
}
