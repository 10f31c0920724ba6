// posepoints_host_main.cpp -- the host form of Optimizer::PoseOptimization (csrc/posepoints_host.cpp over posepoints_terms.hpp) as a stand-alone program, so
// that it can run under AddressSanitizer and UBSan without a Python process around it.  Frames of 0, 2, 9, 64 and 300 features (every fifth holds nothing,
// kinds interleaved, one gross outlier from 9 on), rows exactly as long as the count, a pair row, a refused pair, an inactive row, a depth of 0, an index
// past the map.  Prints POSEPOINTS_HOST_OK.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../include/orbline.h"

namespace olf { void set_error(const std::string&) {} }              // (the library's error slot; this program links the host source alone)

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static unsigned lcg = 99u;
static double uni(double a, double b) { lcg = lcg * 1664525u + 1013904223u; return a + (b - a) * ((lcg >> 8) / 16777216.0); }

int main()
{
    float sig[8], sf = 1.f;
    for (int l = 0; l < 8; ++l) { sig[l] = 1.0f / (sf * sf); sf = (float)(sf * 1.2); }
    const int sizes[5] = {0, 2, 9, 64, 300};
    for (int n : sizes) {
        // two frames: frame 1 carries the features, frame 0 is the "key frame" whose plane of mp_world the pair row indexes
        std::vector<olf_keypoint> kps(2 * (size_t)n);
        std::vector<float> ur(2 * (size_t)n, -1.f), world(2 * 3 * (size_t)n, 0.f), chi2((size_t)n);
        std::vector<int32_t> fmp((size_t)n, -1);
        std::vector<uint8_t> out((size_t)n);
        const int32_t counts[2] = {n, n};
        for (int i = 0; i < n; ++i) {
            const double z = uni(3, 12), X[3] = {uni(-0.5, 0.5) * z, uni(-0.35, 0.35) * z, z};
            for (int k = 0; k < 3; ++k) world[3 * i + k] = (float)X[k];
            const double P[3] = {(double)world[3 * i] + 0.03, (double)world[3 * i + 1], (double)world[3 * i + 2] - 0.02};
            olf_keypoint& kp = kps[(size_t)n + i];
            std::memset(&kp, 0, sizeof(kp));
            kp.x = (float)(160.0 + 250.0 * P[0] / P[2]) + (i == 4 ? 50.f : 0.f); kp.y = (float)(120.0 + 250.0 * P[1] / P[2]); kp.octave = i % 8;
            if (i % 3) ur[(size_t)n + i] = (float)(160.0 + 250.0 * P[0] / P[2] - 25.0 / P[2]);
            if (i % 5 != 3) fmp[i] = i;
        }
        float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, Tout[16];
        const int32_t pairs[2] = {0, 1};
        olf_pose_points_batch in;
        std::memset(&in, 0, sizeof(in));
        in.kps = kps.data(); in.counts = counts; in.img_stride = 1; in.uright = ur.data(); in.fx = 250.f; in.fy = 250.f; in.cx = 160.f; in.cy = 120.f; in.bf = 25.f;
        in.Tcw = Tcw; in.frame_mp = fmp.data(); in.mp_world = world.data(); in.n_mp = 2 * n; in.pairs = pairs;
        int32_t good = -7, initial = -7, passes = -7, iters[4], status = -7;
        const olf_pose_points_outputs o = {Tout, out.data(), &good, &initial, chi2.data(), &passes, iters, &status};
        CHECK(olf_pose_optimization(&in, n, 2, sig, 8, &o) == OLF_OK);
        int held = 0;
        for (int i = 0; i < n; ++i) held += fmp[i] >= 0;
        CHECK(initial == held && status == 0);
        if (held < 3) { CHECK(good == 0 && passes == 0 && !std::memcmp(Tout, Tcw, sizeof(Tcw))); }
        else {
            CHECK(passes == (held < 10 ? 1 : 4));                     // (seven edges with a gross outlier among them: one pass, wherever it ends)
            if (n >= 64) CHECK(out[4] == 1 && good == held - 1 && std::fabs(Tout[3] - 0.03f) < 1e-3f && std::fabs(Tout[11] + 0.02f) < 1e-3f);
        }
        if (n == 64) {
            const int32_t refused[2] = {1, 1}, idle[1] = {0};
            in.pairs = refused;
            CHECK(olf_pose_optimization(&in, n, 2, sig, 8, &o) == OLF_OK && good == -1 && status == 2048);
            in.pairs = pairs; in.row_active = idle;
            CHECK(olf_pose_optimization(&in, n, 2, sig, 8, &o) == OLF_OK && good == -1 && status == 0);
            in.row_active = nullptr;
            fmp[7] = 2 * n;                                            // past the map
            CHECK(olf_pose_optimization(&in, n, 2, sig, 8, &o) == OLF_OK && (status & 512) && initial == held - 1);
            fmp[7] = 7;
            world[3 * 9 + 2] = 0.f;                                    // a depth of exactly 0 at the input pose
            CHECK(olf_pose_optimization(&in, n, 2, sig, 8, &o) == OLF_OK && status == 1 && good == 0 && !std::memcmp(Tout, Tcw, sizeof(Tcw)));
        }
    }
    CHECK(olf_pose_optimization(nullptr, 0, 1, sig, 8, nullptr) == OLF_ERR_INVALID);
    std::printf("POSEPOINTS_HOST_OK\n");
    return 0;
}
