// keyframe_host_main.cpp -- the host forms of the key-frame step (orb_line_slam_amd/csrc/keyframe_host.cpp) as a stand-alone program, for a build under
// -fsanitize=address,undefined (tests/test_keyframe_cpu.py): every plane is a heap array of exactly the size the entry may touch, so a read or write past
// a row ends the run.  Rows: empty, one feature, full rows, counts beyond the capacity, NaN and infinite depths, held indices outside the map, octaves
// outside the levels, all three modes, with and without the optional planes.  Prints KEYFRAME_HOST_OK.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>
#include "../include/orbline.h"

namespace olf { void set_error(const std::string&) {} }              // (the library's is api.cpp)

static unsigned lcg = 7u;
static double uni(double a, double b) { lcg = lcg * 1664525u + 1013904223u; return a + (b - a) * ((lcg >> 8) / 16777216.0); }
static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }

int main()
{
    const int cap = 137, lcap = 61, n = 7, stride = 2, n_mp = 9, n_ml = 5;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<olf_keypoint> kps((size_t)n * stride * cap);
    std::vector<olf_keyline> kls((size_t)n * stride * lcap);
    std::vector<int32_t> counts(n * stride, 1 << 30), lcounts(n * stride, -(1 << 30));
    std::vector<float> depth((size_t)n * cap), ldisp((size_t)2 * n * lcap), Twc(16 * n, 0.f), sf(8);
    std::vector<int32_t> fmp((size_t)n * cap), fml((size_t)n * lcap), nobs(n_mp), lnobs(n_ml), base(n), base_l(n);
    std::vector<uint8_t> outl((size_t)n * cap), outl_l((size_t)n * lcap);
    const int row_counts[n] = {0, 1, cap, cap + 50, 100, 101, 64}, row_lcounts[n] = {0, 1, lcap, lcap + 9, 50, 51, 30};
    for (int l = 0; l < 8; ++l) sf[l] = (float)std::pow(1.2, l);
    for (int k = 0; k < n_mp; ++k) nobs[k] = k % 3;
    for (int k = 0; k < n_ml; ++k) lnobs[k] = k % 2;
    for (int j = 0; j < n; ++j) {
        counts[j * stride] = row_counts[j]; lcounts[j * stride] = row_lcounts[j];
        base[j] = 1000 * j; base_l[j] = 500 * j;
        for (int r = 0; r < 4; ++r) Twc[16 * j + 5 * r] = 1.f;
        Twc[16 * j + 3] = 0.5f * j;
        for (int i = 0; i < cap; ++i) {
            olf_keypoint& kp = kps[((size_t)j * stride) * cap + i];
            kp.x = (float)uni(0, 1200); kp.y = (float)uni(0, 370); kp.octave = i % 13 == 0 ? 9 : i % 8;
            depth[(size_t)j * cap + i] = i % 17 == 3 ? -1.f : i % 29 == 5 ? inf : i % 31 == 7 ? nan : i % 37 == 11 ? 0.f : (float)uni(0.3, 12);
            fmp[(size_t)j * cap + i] = i % 3 == 0 ? -1 : i % 23 == 1 ? n_mp + i : i % n_mp;
            outl[(size_t)j * cap + i] = i % 5 == 0;
        }
        for (int i = 0; i < lcap; ++i) {
            olf_keyline& kl = kls[((size_t)j * stride) * lcap + i];
            kl.startPointX = (float)uni(0, 1200); kl.startPointY = (float)uni(0, 370); kl.endPointX = (float)uni(0, 1200); kl.endPointY = (float)uni(0, 370);
            float* d = &ldisp[2 * ((size_t)j * lcap + i)];
            d[0] = i % 7 == 2 ? -1.f : i % 19 == 4 ? 0.f : i % 23 == 6 ? -0.f : (float)uni(3, 90);
            d[1] = i % 11 == 3 ? -1.f : j == 6 && i == 12 ? nan : (float)uni(3, 90);
            fml[(size_t)j * lcap + i] = i % 2 ? -1 : i % 13 == 0 ? n_ml + 1 : i % n_ml;
            outl_l[(size_t)j * lcap + i] = i % 4 == 0;
        }
    }
    olf_landmarks_batch in = {};
    in.kps = kps.data(); in.counts = counts.data(); in.kls = kls.data(); in.lcounts = lcounts.data(); in.img_stride = stride;
    in.depth = depth.data(); in.ldisp = ldisp.data(); in.Twc = Twc.data();
    in.fx = 435.2f; in.fy = 435.2f; in.cx = 367.4f; in.cy = 252.2f; in.mbf = 47.9f; in.thDepth = 3.85f;
    std::vector<int32_t> nv(2 * n), nc(2 * n), vo((size_t)n * cap), vl((size_t)n * lcap), co((size_t)n * cap), cl((size_t)n * lcap), fo((size_t)n * cap), fl((size_t)n * lcap), st(n);
    std::vector<uint8_t> cr((size_t)n * cap), crl((size_t)n * lcap);
    std::vector<float> w((size_t)3 * n * cap), nr((size_t)3 * n * cap), mx((size_t)n * cap), mn((size_t)n * cap), lw((size_t)6 * n * lcap);
    std::vector<double> lwd((size_t)6 * n * lcap);
    olf_landmarks_outputs o = {nv.data(), nc.data(), vo.data(), vl.data(), co.data(), cl.data(), cr.data(), crl.data(), fo.data(), fl.data(), w.data(), nr.data(), mx.data(),
                               mn.data(), lwd.data(), lw.data(), st.data()};
    for (int pass = 0; pass < 2; ++pass) {
        for (int mode = 0; mode < 3; ++mode) {
            expect(olf_stereo_landmarks(&in, cap, lcap, n, mode, sf.data(), 8, &o) == OLF_OK, "olf_stereo_landmarks");
            for (int j = 0; j < n; ++j) {
                int made = 0;
                for (int i = 0; i < cap; ++i) made += cr[(size_t)j * cap + i];
                expect(made == nc[2 * j] && nc[2 * j] <= nv[2 * j] && nv[2 * j] <= (row_counts[j] < cap ? row_counts[j] : cap), "the point counters of a row");
                expect(nc[2 * j + 1] <= nv[2 * j + 1] && nv[2 * j + 1] <= (row_lcounts[j] < lcap ? row_lcounts[j] : lcap), "the line counters of a row");
            }
            if (mode) expect((st[6] & 1) && nv[13] == 0 && !(st[5] & 1), "a NaN line depth empties the row's lines and sets bit 1");
            expect((st[2] & 4) != 0, "an octave outside the levels sets bit 4");
            if (pass && mode) expect((st[2] & 2) != 0, "a held index outside the map sets bit 2");
        }
        // second pass: with the held entries, the observation counts and the bases; without the double plane
        in.frame_mp = fmp.data(); in.frame_ml = fml.data(); in.mp_nobs = nobs.data(); in.n_mp = n_mp; in.ml_nobs = lnobs.data(); in.n_ml = n_ml;
        in.new_base_mp = base.data(); in.new_base_ml = base_l.data();
        o.ml_world_d = nullptr;
    }
    expect(olf_stereo_landmarks(&in, cap, lcap, n, 3, sf.data(), 8, &o) == OLF_ERR_INVALID && olf_stereo_landmarks(&in, cap, lcap, -1, 0, sf.data(), 8, &o) == OLF_ERR_INVALID,
           "an unknown mode and a negative count are refused");
    expect(olf_stereo_landmarks(&in, 8193, lcap, 0, 0, sf.data(), 8, &o) == OLF_ERR_CAPACITY, "more than OLF_GRID_MAX_KEYS key points");

    std::vector<int32_t> rows((size_t)OLF_KEYFRAME_ROW * n, 0), nref(n, 100), nref_l(n, 100), ninl(2 * n, 20), lf(n);
    for (int j = 0; j < n; ++j) {
        int32_t* r = &rows[(size_t)OLF_KEYFRAME_ROW * j];
        r[0] = 100 + j; r[1] = 90; r[4] = 30; r[5] = j; r[6] = j & 1; r[7] = j % 4; r[10] = j == 3;
        lf[j] = j - 1;
    }
    olf_keyframe_test_batch kin = {};
    kin.counts = counts.data(); kin.lcounts = lcounts.data(); kin.img_stride = stride; kin.depth = depth.data(); kin.ldisp = ldisp.data(); kin.rows = rows.data();
    kin.n_ref_matches = nref.data(); kin.n_ref_matches_l = nref_l.data(); kin.n_inliers = ninl.data(); kin.mbf = 47.9f; kin.thDepth = 3.85f;
    std::vector<uint8_t> need(n), ba(n);
    std::vector<int32_t> cnt(4 * n), cond(n), kst(n);
    const olf_keyframe_test_outputs ko = {need.data(), ba.data(), cnt.data(), cond.data(), kst.data()};
    expect(olf_need_new_keyframe(&kin, cap, lcap, n, &ko) == OLF_OK, "olf_need_new_keyframe without the optional planes");
    expect(cnt[4 * 2] == 0 && cnt[4 * 2 + 1] > 0 && cnt[4 * 3 + 1] == 0, "nothing is held: every close point is untracked; a monocular row counts nothing");
    kin.frame_mp = fmp.data(); kin.frame_ml = fml.data(); kin.outlier = outl.data(); kin.outlier_l = outl_l.data(); kin.ldisp_frame = lf.data();
    expect(olf_need_new_keyframe(&kin, cap, lcap, n, &ko) == OLF_OK, "olf_need_new_keyframe with every plane");
    expect(kst[0] == 0 && kst[1] == 1 && kst[2] == 1 && kst[4] == 0, "rows that read a shorter frame's disparities set bit 1");
    expect(olf_need_new_keyframe(&kin, cap, lcap, -1, &ko) == OLF_ERR_INVALID && olf_need_new_keyframe(nullptr, cap, lcap, 1, &ko) == OLF_ERR_INVALID, "argument checks");
    if (failures) return 1;
    std::printf("KEYFRAME_HOST_OK\n");
    return 0;
}
