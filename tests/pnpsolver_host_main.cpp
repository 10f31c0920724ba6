// pnpsolver_host_main.cpp -- the host form of the PnP solver (csrc/pnpsolver_host.cpp over pnpsolver_terms.hpp) as a stand-alone program, so that it can
// run under AddressSanitizer / UBSan in a process of its own (tests/test_pnpsolver_cpu.py builds it with -fsanitize=address,undefined).  A key frame and a
// frame at capacity 40: 37 row entries are correspondences, 30 of them noise-free projections under a known pose (a rotation of 0.3 rad about z, a
// translation) and 7 displaced by 50 pixels; three row entries are no correspondence.  Every array is allocated at exactly its length, so a read or write
// past a count is an error the sanitizer reports.  The solver runs in windows of 5 until it returns a pose, is resumed once, then a row with 9
// correspondences must end with no_more and an untouched state.  Prints "pnpsolver_host_main ok".
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
    uint32_t seed = 4321u;
    std::vector<olf_keypoint> kps((size_t)n_frames * cap);
    std::memset(kps.data(), 0, kps.size() * sizeof(olf_keypoint));
    std::vector<int32_t> counts = {cap, cap}, row(cap);
    std::vector<float> world((size_t)n_frames * cap * 3, 0.f);
    std::vector<uint8_t> valid((size_t)n_frames * cap, 1), bad((size_t)n_frames * cap, 0);
    const float c = std::cos(0.3f), s = std::sin(0.3f), t[3] = {0.2f, -0.1f, 0.3f};
    for (int i = 0; i < cap; ++i) {                                  // frame 0 is the key frame, frame 1 the lost frame
        const int v = cap - 1 - i;                                   // frame feature i sees the point of key-frame feature v
        const float z = 3.f + 6.f * unit(seed), xw[3] = {(unit(seed) - 0.5f) * z, (unit(seed) - 0.5f) * z * 0.7f, z};
        for (int k = 0; k < 3; ++k) world[3 * v + k] = xw[k];
        const double xc = (double)c * xw[0] - (double)s * xw[1] + t[0], yc = (double)s * xw[0] + (double)c * xw[1] + t[1], zc = (double)xw[2] + t[2];
        kps[cap + i].x = (float)(200.0 * xc / zc + 160.0) + (i % 5 == 4 && i < 35 ? 50.f : 0.f);
        kps[cap + i].y = (float)(200.0 * yc / zc + 120.0);
        kps[cap + i].octave = i % 8;
        row[i] = v;
    }
    row[7] = -1; bad[cap - 1 - 11] = 1; valid[cap - 1 - 20] = 0;     // three entries that are no correspondence
    float sf[8] = {1.f};
    for (int l = 1; l < 8; ++l) sf[l] = sf[l - 1] * 1.2f;
    std::vector<uint32_t> draws((size_t)max_its * 4);
    for (auto& d : draws) d = lcg(seed);

    olf_track_batch in;
    std::memset(&in, 0, sizeof in);
    in.kps = kps.data(); in.counts = counts.data(); in.img_stride = 1; in.mp_world = world.data(); in.mp_valid = valid.data();
    in.fx = in.fy = 200.f; in.cx = 160.f; in.cy = 120.f;
    olf_pnp_ransac R = {0.99, 10, max_its, 4, 5, 0.5f, 5.991f};
    int32_t done = 0, best = 0, refined = 0, accepted = 0, no_more = 0, n_inliers = 0, n_corr = 0, status = 0;
    float bT[16] = {0}, rT[16] = {0}, T[16] = {0};
    std::vector<uint8_t> bf(cap, 0), rf(cap, 0), inliers(cap, 99);
    std::vector<int32_t> cnt(max_its, -7);
    olf_pnp_solver_io io = {&done, &best, bT, bf.data(), &refined, rT, rf.data(), &accepted, &no_more, &n_inliers, inliers.data(), T, &n_corr, cnt.data()};
    CHECK(olf_pnp_solver(&in, cap, n_frames, bad.data(), sf, 8, 0, 1, row.data(), &R, draws.data(), &io, &status) == OLF_OK && (status & ~32768) == 0);
    CHECK(n_corr == 37 && accepted == 1 && done >= 1);
    if (!no_more) {                                                  // Refine accepted: the 30 inliers less the two that are no correspondence
        CHECK(n_inliers == refined && n_inliers >= 27);
        CHECK(std::fabs(T[0] - c) < 1e-3f && std::fabs(T[4] - s) < 1e-3f && std::fabs(T[11] - t[2]) < 1e-2f);
    }
    int set = 0;
    for (int i = 0; i < cap; ++i) { CHECK(inliers[i] <= 1); set += inliers[i]; }
    CHECK(set == n_inliers && !inliers[7] && !inliers[11] && !inliers[20]);
    const int first = done;
    CHECK(olf_pnp_solver(&in, cap, n_frames, bad.data(), sf, 8, 0, 1, row.data(), &R, draws.data(), &io, &status) == OLF_OK);      // resumed
    CHECK(done > first && accepted == 1);

    // 9 correspondences: below min_inliers
    for (int i = 9; i < cap; ++i) row[i] = -1;
    row[7] = cap - 1 - 7;
    done = best = 0; accepted = 7; no_more = 0; bT[0] = 5.f;
    CHECK(olf_pnp_solver(&in, cap, n_frames, nullptr, sf, 8, 0, 1, row.data(), &R, draws.data(), &io, &status) == OLF_OK);
    CHECK(n_corr == 9 && accepted == 0 && no_more == 1 && n_inliers == 0 && done == 0 && best == 0 && bT[0] == 5.f);
    // a refused pair and a bad argument
    CHECK(olf_pnp_solver(&in, cap, n_frames, nullptr, sf, 8, 1, 1, row.data(), &R, draws.data(), &io, &status) == OLF_OK && status == 2048 && n_inliers == -1);
    R.min_set = 3;
    CHECK(olf_pnp_solver(&in, cap, n_frames, nullptr, sf, 8, 0, 1, row.data(), &R, draws.data(), &io, &status) == OLF_ERR_INVALID);
    std::printf("pnpsolver_host_main ok\n");
    return 0;
}
