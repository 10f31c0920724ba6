// initializer_host.cpp -- the host form of initializer_batch.hip: olf_initializer, one Initializer::Initialize (src/Initializer.cc:44-121) over host
// pointers, no context and no device.  The arithmetic is initializer_terms.hpp, the text the kernel runs; the loops are FindHomography, FindFundamental,
// ReconstructH / ReconstructF and CheckRT as written.  Here too: the checks of the parameter and io blocks that every form shares, and C.34's cosine
// thresholds, found with this machine's libm for the host form and the device entry alike.
#include <algorithm>
#include <vector>
#include "initializer_terms.hpp"
#include "solver_args.hpp"
#include "olf_internal.hpp"
#include "../../include/orbline.h"

using namespace olf;

namespace olf {

bool ini_params_ok(const olf_initializer_params* P)
{
    return P && P->sigma > 0.0f && ini_finite(P->sigma) && P->max_iterations >= 1 && P->min_triangulated >= 0 && ini_finite(P->min_parallax);
}
bool ini_io_ok(const olf_initializer_io* io)
{
    return io && io->ok && io->n_correspondences && io->model && io->score_H && io->score_F && io->H21 && io->F21 && io->inliers_H && io->inliers_F && io->R21 &&
           io->t21 && io->P3D && io->triangulated && io->n_good && io->cos_parallax && io->hypothesis;
}

// floats in ascending order as unsigned integers, and back
static uint32_t ord_of(float f) { const uint32_t u = f2bits(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
static float of_ord(uint32_t o) { return bits2f((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// C.34: the largest float cosine in [-1, 1] whose parallax passes `> min_parallax` (strict) or `>= min_parallax`; NaN when none does.  By bisection
// over the floats' bit patterns; the comparison has to be monotone over the 256 floats on either side of the answer.
bool ini_cos_threshold(float min_parallax, bool strict, float* out)
{
    auto pred = [&](uint32_t o) { const float d = ini_parallax_degrees(of_ord(o)); return strict ? d > min_parallax : d >= min_parallax; };
    uint32_t lo = ord_of(-1.0f), hi = ord_of(1.0f);
    const uint32_t first = lo, last = hi;
    if (!pred(lo)) { *out = bits2f(0x7fc00000u); return true; }
    if (pred(hi)) lo = hi;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pred(mid)) lo = mid; else hi = mid;
    }
    for (uint32_t k = 1; k <= 256; ++k) {
        if (lo >= first + k && !pred(lo - k)) return false;
        if (lo + k <= last && pred(lo + k)) return false;
    }
    *out = of_ord(lo);
    return true;
}

}  // namespace olf

extern "C" int olf_debug_initializer_cos_thresholds(float min_parallax, float* cos_gt, float* cos_ge)
{
    if (!cos_gt || !cos_ge || !ini_finite(min_parallax) || !ini_cos_threshold(min_parallax, true, cos_gt) || !ini_cos_threshold(min_parallax, false, cos_ge)) {
        set_error("olf_debug_initializer_cos_thresholds: bad argument, or acosf is not monotone around the threshold");
        return OLF_ERR_INVALID;
    }
    return OLF_OK;
}

extern "C" int olf_debug_initializer_sample(int N, const uint32_t* draws8, int32_t* idx8)
{
    if (N < 8 || !draws8 || !idx8) { set_error("olf_debug_initializer_sample: bad argument"); return OLF_ERR_INVALID; }
    int idx[8];
    ransac_sample<8>(N, draws8, idx);
    for (int k = 0; k < 8; ++k) idx8[k] = idx[k];
    return OLF_OK;
}

extern "C" int olf_initializer(const olf_track_batch* in, int capacity, int n_frames, int ref, int cur, const int32_t* matches, const olf_initializer_params* prm,
                               const uint32_t* draws, const olf_initializer_io* io, int32_t* status)
{
    const char* who = "olf_initializer";
    bool ok = in && status && capacity >= 0 && n_frames >= 0 && matches && draws && ini_params_ok(prm) && ini_io_ok(io);
    ok = ok && (!n_frames || (in->kps && in->counts && in->img_stride >= 1));
    float cos_gt = 0, cos_ge = 0;
    ok = ok && ini_cos_threshold(prm->min_parallax, true, &cos_gt) && ini_cos_threshold(prm->min_parallax, false, &cos_ge);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    *status = 0;
    if (!(ref >= 0 && ref < n_frames && cur >= 0 && cur < n_frames && ref != cur)) { *status = STATUS_PAIR; *io->ok = -1; return OLF_OK; }
    const size_t cap = (size_t)capacity;
    const int N1 = clampi(in->counts[(size_t)ref * in->img_stride], 0, capacity), N2 = clampi(in->counts[(size_t)cur * in->img_stride], 0, capacity);
    const olf_keypoint* kp1 = in->kps + (size_t)ref * in->img_stride * cap;
    const olf_keypoint* kp2 = in->kps + (size_t)cur * in->img_stride * cap;
    const IniCam K = {in->fx, in->fy, in->cx, in->cy};
    // mvMatches12 (:51-63)
    const int room = N1 > 0 ? N1 : 1;
    std::vector<float> st((size_t)INI_WORDS * room);
    const IniPlanes P = {st.data(), room};
    int N = 0;
    for (int i = 0; i < N1; ++i) {
        const int v = matches[i];
        if (!s3_is_match(v, N2)) continue;
        st[N] = kp1[i].x; st[(size_t)room + N] = kp1[i].y; st[(size_t)2 * room + N] = kp2[v].x; st[(size_t)3 * room + N] = kp2[v].y;
        P.feat(N) = i;
        P.flags(N) = 0;
        ++N;
    }
    *io->n_correspondences = N;
    *io->ok = 0; *io->model = 0;
    if (N < 8) return OLF_OK;                                        // C.33
    IniNorm n1, n2;
    ini_normalize_axis(kp1, N1, 0, &n1.mx, &n1.sx); ini_normalize_axis(kp1, N1, 1, &n1.my, &n1.sy);
    ini_normalize_axis(kp2, N2, 0, &n2.mx, &n2.sx); ini_normalize_axis(kp2, N2, 1, &n2.my, &n2.sy);
    const float invSigmaSquare = ini_inv_sigma_square(prm->sigma);
    // FindHomography (:124-172) and FindFundamental (:175-223)
    std::vector<float> wf((size_t)INI_WS_F);
    std::vector<double> wd((size_t)INI_WS_D);
    IniWs e = {wf.data(), wd.data(), 1};
    float SH = 0, SF = 0, H21[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, H12[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, F21[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // (no score: zeros)
    bool anyH = false, anyF = false;
    for (int it = 0; it < prm->max_iterations; ++it) {
        int idx[8];
        ransac_sample<8>(N, draws + 8 * (size_t)it, idx);
        float Hi[9], Hinv[9], Fi[9];
        ini_fit_h(e, P, idx, n1, n2, Hi, Hinv);
        const float sh = ini_score_h(P, N, Hi, Hinv, invSigmaSquare);
        if (sh > SH) { SH = sh; anyH = true; for (int k = 0; k < 9; ++k) { H21[k] = Hi[k]; H12[k] = Hinv[k]; } }
        float sf = 0;
        if (ini_fit_f(e, P, idx, n1, n2, Fi)) sf = ini_score_f(P, N, Fi, invSigmaSquare);
        else *status |= STATUS_INI_DEGENERATE;
        if (sf > SF) { SF = sf; anyF = true; for (int k = 0; k < 9; ++k) F21[k] = Fi[k]; }
    }
    *io->score_H = SH; *io->score_F = SF;
    if (anyH) for (int k = 0; k < 9; ++k) io->H21[k] = H21[k];
    if (anyF) for (int k = 0; k < 9; ++k) io->F21[k] = F21[k];
    for (int i = 0; i < N1; ++i) { io->inliers_H[i] = 0; io->inliers_F[i] = 0; }
    for (int q = 0; q < N; ++q) {
        float c[4], s = 0;
        P.load(q, c);
        const int f = (anyH && ini_check_h(H21, H12, c, invSigmaSquare, s) ? 1 : 0) | (anyF && ini_check_f(F21, c, invSigmaSquare, s) ? 2 : 0);
        P.flags(q) = f;
        io->inliers_H[P.feat(q)] = f & 1; io->inliers_F[P.feat(q)] = (f >> 1) & 1;
    }
    // the model (:112-118) and its motion hypotheses
    const bool useH = ini_choose_h(SH, SF);
    const int bit = useH ? 1 : 2;
    *io->model = useH ? 1 : 2;
    for (int h = 0; h < 8; ++h) { io->n_good[h] = 0; io->cos_parallax[h] = 0.0f; }
    *io->hypothesis = -1;
    int Nin = 0;
    for (int q = 0; q < N; ++q) Nin += (P.flags(q) & bit) ? 1 : 0;
    float Rs[72], ts[24];
    const int flags = useH ? ini_hypotheses_h(e, H21, K, Rs, ts) : ini_hypotheses_f(e, F21, K, Rs, ts);
    if (flags < 0) return OLF_OK;                                    // :597-600
    if (flags & 2) *status |= STATUS_INI_DEGENERATE;
    const int nh = useH ? 8 : 4;
    const float th2 = ini_th2(prm->sigma);
    int nGood[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float cosv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> keys;
    for (int h = 0; h < nh; ++h) {                                   // CheckRT (:798-907)
        IniPose Hp;
        ini_pose_prepare(K, Rs + 9 * h, ts + 3 * h, Hp);
        keys.clear();
        for (int q = 0; q < N; ++q) {
            if (!(P.flags(q) & bit)) continue;
            float c[4], p3d[3], cp = 0;
            P.load(q, c);
            if (!ini_check_point(K, Hp, c, th2, p3d, cp)) continue;
            P.cosv(q) = cp;
            if (cp != cp) *status |= STATUS_INI_NAN;
            keys.push_back(((uint64_t)ini_cos_key(cp) << 32) | (uint32_t)q);
        }
        nGood[h] = (int)keys.size();
        if (nGood[h] > 0) {                                          // C.35
            std::sort(keys.begin(), keys.end());
            cosv[h] = P.cosv((int)(uint32_t)keys[(size_t)std::min(50, nGood[h] - 1)]);
        }
        io->n_good[h] = nGood[h]; io->cos_parallax[h] = cosv[h];
    }
    const int chosen = useH ? ini_decide_h(nGood, cosv, Nin, prm->min_triangulated, cos_ge, 0.0f >= prm->min_parallax)
                            : ini_decide_f(nGood, cosv, Nin, prm->min_triangulated, cos_gt, 0.0f > prm->min_parallax);
    if (chosen < 0) return OLF_OK;
    *io->hypothesis = chosen;
    *io->ok = 1;
    for (int k = 0; k < 9; ++k) io->R21[k] = Rs[9 * chosen + k];
    for (int k = 0; k < 3; ++k) io->t21[k] = ts[3 * chosen + k];
    for (int i = 0; i < N1; ++i) { io->triangulated[i] = 0; for (int k = 0; k < 3; ++k) io->P3D[3 * (size_t)i + k] = 0.0f; }
    IniPose Hp;
    ini_pose_prepare(K, Rs + 9 * chosen, ts + 3 * chosen, Hp);
    for (int q = 0; q < N; ++q) {
        if (!(P.flags(q) & bit)) continue;
        float c[4], p3d[3], cp = 0;
        P.load(q, c);
        const int code = ini_check_point(K, Hp, c, th2, p3d, cp);
        if (!code) continue;
        const size_t i = (size_t)P.feat(q);
        for (int k = 0; k < 3; ++k) io->P3D[3 * i + k] = p3d[k];
        io->triangulated[i] = code == 3;
    }
    return OLF_OK;
}
