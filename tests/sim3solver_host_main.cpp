// sim3solver_host_main.cpp -- the host form of the Sim3 solver (csrc/sim3solver_host.cpp over sim3solver_terms.hpp) as a stand-alone program, so that it
// can run under AddressSanitizer / UBSan in a process of its own (tests/test_sim3solver_cpu.py builds it with -fsanitize=address,undefined).  Two key
// frames at capacity 40 see 37 points under a known similarity (scale 2, a rotation of 0.3 rad, a translation); three row entries are no correspondence.
// Every array is allocated at exactly its length, so a read or write past a count is an error the sanitizer reports.  The solver runs in windows of 5
// until it accepts; then a row with 10 correspondences must end with no_more and an untouched state.  Prints "sim3solver_host_main ok".
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
    const int cap = 40, n_frames = 2, max_its = 300;
    uint32_t seed = 12345u;
    std::vector<olf_keypoint> kps((size_t)n_frames * cap);
    std::memset(kps.data(), 0, kps.size() * sizeof(olf_keypoint));
    std::vector<int32_t> counts = {cap, cap}, row(cap);
    std::vector<float> Tcw(32, 0.f), world((size_t)n_frames * cap * 3);
    std::vector<uint8_t> valid((size_t)n_frames * cap, 1), bad((size_t)n_frames * cap, 0);
    for (int f = 0; f < 2; ++f) for (int k = 0; k < 4; ++k) Tcw[16 * f + 5 * k] = 1.f;
    const float c = std::cos(0.3f), s = std::sin(0.3f), scale = 2.f, t[3] = {0.2f, -0.1f, 0.3f};
    for (int i = 0; i < cap; ++i) {
        const float z = 3.f + 6.f * unit(seed), x2[3] = {(unit(seed) - 0.5f) * z, (unit(seed) - 0.5f) * z * 0.7f, z};
        const int j = cap - 1 - i;                                   // feature j of frame 1 holds the point of feature i of frame 0
        for (int k = 0; k < 3; ++k) world[3 * (cap + j) + k] = x2[k];
        // X1 = scale * Rz(0.3) * X2 + t
        world[3 * i] = scale * (c * x2[0] - s * x2[1]) + t[0];
        world[3 * i + 1] = scale * (s * x2[0] + c * x2[1]) + t[1];
        world[3 * i + 2] = scale * x2[2] + t[2];
        row[i] = j;
        kps[i].octave = i % 8; kps[cap + j].octave = (i / 3) % 8;
    }
    row[7] = -1; bad[11] = 1; valid[cap + (cap - 1 - 20)] = 0;       // three entries that are no correspondence
    float sf[8] = {1.f};
    for (int l = 1; l < 8; ++l) sf[l] = sf[l - 1] * 1.2f;
    std::vector<uint32_t> draws((size_t)max_its * 3);
    for (auto& d : draws) d = lcg(seed);

    olf_track_batch in;
    std::memset(&in, 0, sizeof in);
    in.kps = kps.data(); in.counts = counts.data(); in.img_stride = 1; in.Tcw = Tcw.data(); in.mp_world = world.data(); in.mp_valid = valid.data();
    in.fx = in.fy = 200.f; in.cx = 160.f; in.cy = 120.f;
    olf_sim3_ransac R = {0, 0.99, 20, max_its, 5};
    int32_t done = 0, best = 0, accepted = 0, no_more = 0, n_inliers = 0, n_corr = 0, status = 0;
    float bs = 0, bR[9] = {0}, bt[3] = {0}, bT[16] = {0};
    std::vector<uint8_t> inliers(cap, 99);
    std::vector<int32_t> cnt(max_its, -7);
    olf_sim3_solver_io io = {&done, &best, &bs, bR, bt, bT, &accepted, &no_more, &n_inliers, inliers.data(), &n_corr, cnt.data()};
    for (int call = 0; call < 60 && !accepted && !no_more; ++call)
        CHECK(olf_sim3_solver(&in, cap, n_frames, bad.data(), sf, 8, 0, 1, row.data(), &R, draws.data(), &io, &status) == OLF_OK && status == 0);
    CHECK(n_corr == 37 && accepted == 1 && n_inliers == 37 && best == 37 && done >= 1);
    CHECK(std::fabs(bs - scale) < 1e-3f && std::fabs(bR[0] - c) < 1e-3f && std::fabs(bR[3] - s) < 1e-3f && std::fabs(bt[2] - t[2]) < 1e-2f);
    int set = 0;
    for (int i = 0; i < cap; ++i) { CHECK(inliers[i] <= 1); set += inliers[i]; }
    CHECK(set == 37 && !inliers[7] && !inliers[11] && !inliers[20]);
    for (int j = 0; j < max_its; ++j) CHECK(j < done ? cnt[j] >= 0 : cnt[j] == -7);

    // 10 correspondences: below min_inliers
    for (int i = 10; i < cap; ++i) row[i] = -1;
    row[7] = cap - 1 - 7;
    done = best = 0; accepted = 7; no_more = 0; bs = 5.f;
    CHECK(olf_sim3_solver(&in, cap, n_frames, nullptr, sf, 8, 0, 1, row.data(), &R, draws.data(), &io, &status) == OLF_OK);
    CHECK(n_corr == 10 && accepted == 0 && no_more == 1 && n_inliers == 0 && done == 0 && best == 0 && bs == 5.f);
    // a refused pair and a bad argument
    CHECK(olf_sim3_solver(&in, cap, n_frames, nullptr, sf, 8, 1, 1, row.data(), &R, draws.data(), &io, &status) == OLF_OK && status == 2048 && n_inliers == -1);
    R.min_inliers = 2;
    CHECK(olf_sim3_solver(&in, cap, n_frames, nullptr, sf, 8, 0, 1, row.data(), &R, draws.data(), &io, &status) == OLF_ERR_INVALID);
    std::printf("sim3solver_host_main ok\n");
    return 0;
}
