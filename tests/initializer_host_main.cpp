// initializer_host_main.cpp -- the host form of the initialiser (csrc/initializer_host.cpp over initializer_terms.hpp) as a stand-alone program, so that
// it can run under AddressSanitizer / UBSan in a process of its own (tests/test_initializer_cpu.py builds it with -fsanitize=address,undefined).  Two
// frames at a row length of 120: 100 noise-free correspondences of a general scene under a known motion (0.05 rad about y, a translation along x), 112
// and 105 key points.  Every array is allocated at exactly its length, so a read or write past a count is an error the sanitizer reports.  The pair must
// initialise from the fundamental matrix with the motion recovered; then a row of 7 correspondences must leave everything but ok, model and
// n_correspondences; then a refused pair and a bad argument.  Prints "initializer_host_main ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../include/orbline.h"

namespace olf { void set_error(const std::string& s) { std::printf("error: %s\n", s.c_str()); } }

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 1; }      // below 2^31
static float unit(uint32_t& s) { return (float)(lcg(s) >> 7) / 16777216.0f; }

#define CHECK(c) do { if (!(c)) { std::printf("failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

int main()
{
    const int cap = 120, N1 = 112, N2 = 105, N = 100, its = 40;
    uint32_t seed = 4321u;
    std::vector<olf_keypoint> kps((size_t)2 * cap);
    std::memset(kps.data(), 0, kps.size() * sizeof(olf_keypoint));
    std::vector<int32_t> counts = {N1, N2}, row(cap, -1);
    const float c = std::cos(0.05f), s = std::sin(0.05f), t[3] = {0.5f, 0.02f, 0.05f};
    for (int i = 0; i < cap; ++i) {                                  // unmatched key points anywhere in the image
        kps[i].x = 320.f * unit(seed); kps[i].y = 240.f * unit(seed);
        kps[cap + i].x = 320.f * unit(seed); kps[cap + i].y = 240.f * unit(seed);
    }
    for (int q = 0; q < N; ++q) {
        const int i = q + q / 9, v = N2 - 1 - q;                     // reference feature i sees what current feature v sees
        const float z = 3.f + 6.f * unit(seed), X[3] = {(unit(seed) - 0.5f) * z, (unit(seed) - 0.5f) * z * 0.7f, z};
        const double xc = (double)c * X[0] + (double)s * X[2] + t[0], yc = (double)X[1] + t[1], zc = -(double)s * X[0] + (double)c * X[2] + t[2];
        kps[i].x = (float)(200.0 * X[0] / X[2] + 160.0); kps[i].y = (float)(200.0 * X[1] / X[2] + 120.0);
        kps[cap + v].x = (float)(200.0 * xc / zc + 160.0); kps[cap + v].y = (float)(200.0 * yc / zc + 120.0);
        row[i] = v;
    }
    row[9] = N2 + 2; row[N1] = 3;                                   // a value beyond N2 and a row entry beyond N1: no correspondences
    std::vector<uint32_t> draws((size_t)its * 8);
    for (auto& d : draws) d = lcg(seed);

    olf_track_batch in;
    std::memset(&in, 0, sizeof in);
    in.kps = kps.data(); in.counts = counts.data(); in.img_stride = 1;
    in.fx = in.fy = 200.f; in.cx = 160.f; in.cy = 120.f;
    olf_initializer_params P = {1.0f, its, 1.0f, 50};
    int32_t ok = 9, ncorr = 9, model = 9, hyp = 9, status = 0;
    float sH = -7.f, sF = -7.f, H[9], F[9], R[9], tt[3], cosv[8];
    int32_t ng[8];
    std::vector<uint8_t> iH(cap, 77), iF(cap, 77), tri(cap, 77);
    std::vector<float> P3D((size_t)3 * cap, -7.f);
    olf_initializer_io io = {&ok, &ncorr, &model, &sH, &sF, H, F, iH.data(), iF.data(), R, tt, P3D.data(), tri.data(), ng, cosv, &hyp};
    CHECK(olf_initializer(&in, cap, 2, 0, 1, row.data(), &P, draws.data(), &io, &status) == OLF_OK && status == 0);
    CHECK(ncorr == N && ok == 1 && model == 2 && hyp >= 0 && hyp < 4 && ng[hyp] == N && sF > sH);
    CHECK(std::fabs(R[0] - c) < 1e-3f && std::fabs(R[2] - s) < 1e-3f && std::fabs(R[4] - 1.f) < 1e-3f);
    const float tn = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    CHECK(std::fabs(tt[0] - t[0] / tn) < 1e-2f && std::fabs(tt[1] - t[1] / tn) < 1e-2f && std::fabs(tt[2] - t[2] / tn) < 1e-2f);
    int set = 0;
    for (int i = 0; i < N1; ++i) { CHECK(tri[i] <= 1 && iF[i] <= 1 && iH[i] <= 1); set += tri[i]; if (tri[i]) CHECK(row[i] >= 0 && row[i] < N2); }
    for (int i = N1; i < cap; ++i) CHECK(tri[i] == 77 && iF[i] == 77 && iH[i] == 77 && P3D[3 * i] == -7.f);
    CHECK(set >= 90 && !tri[9] && P3D[3 * 9] == 0.f && P3D[2] > 0.f);

    // 7 correspondences: only ok, model and n_correspondences are written
    std::vector<int32_t> few(row);
    for (int i = 7; i < cap; ++i) few[i] = -1;
    ok = 9; model = 9; hyp = 9; sH = -7.f;
    CHECK(olf_initializer(&in, cap, 2, 0, 1, few.data(), &P, draws.data(), &io, &status) == OLF_OK && status == 0);
    CHECK(ncorr == 7 && ok == 0 && model == 0 && hyp == 9 && sH == -7.f);
    // a refused pair and a bad argument
    CHECK(olf_initializer(&in, cap, 2, 1, 1, row.data(), &P, draws.data(), &io, &status) == OLF_OK && status == 2048 && ok == -1);
    P.sigma = 0.f;
    CHECK(olf_initializer(&in, cap, 2, 0, 1, row.data(), &P, draws.data(), &io, &status) == OLF_ERR_INVALID);
    std::printf("initializer_host_main ok\n");
    return 0;
}
