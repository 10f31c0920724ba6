// newpoints_host.cpp -- the host forms of newpoints_batch.hip: olf_compute_f12 (LocalMapping::ComputeF12, src/LocalMapping.cc:536-553) and
// olf_update_normal_and_depth (MapPoint::UpdateNormalAndDepth, src/MapPoint.cc:342-383).  Host pointers, no context and no device; the arithmetic is
// newpoints_terms.hpp, the text the kernels run.
#include "newpoints_terms.hpp"
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_compute_f12(const float* Tcw1, const float* Tcw2, float fx, float fy, float cx, float cy, float* F12)
{
    if (!Tcw1 || !Tcw2 || !F12) { set_error("olf_compute_f12: bad argument"); return OLF_ERR_INVALID; }
    const float cam[4] = {fx, fy, cx, cy};
    f12_compute(Tcw1, Tcw2, cam, F12);
    return OLF_OK;
}

// the loop of k_create_new_map_points (newpoints_batch.hip), pair by pair and slot by slot
extern "C" int olf_create_new_map_points(const olf_track_batch* in, int capacity, int n_frames, const float* depth, float mb, const float* scale_factors, int n_levels,
                                         int n_pairs, const int32_t* pairs, const int32_t* matches12, int monocular, float* x3D, uint8_t* code, int32_t* nnew,
                                         int32_t* status)
{
    const char* who = "olf_create_new_map_points";
    bool ok = in && status && capacity >= 0 && n_frames >= 0 && n_pairs >= 0 && scale_factors && n_levels >= 1 && n_levels <= OLF_MAX_LEVELS;
    ok = ok && (!n_pairs || (pairs && matches12 && x3D && code && nnew));
    ok = ok && (!n_pairs || !n_frames || (in->kps && in->counts && in->img_stride >= 1 && in->uright && in->Tcw && depth));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    const NewPointCam K = new_point_cam(in->fx, in->fy, in->cx, in->cy, in->mbf, mb, n_levels > 1 ? scale_factors[1] : 1.0f);
    const size_t cap = (size_t)capacity;
    int bits = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const int f1 = pairs[2 * (size_t)p], f2 = pairs[2 * (size_t)p + 1];
        if (!(f1 >= 0 && f1 < n_frames && f2 >= 0 && f2 < n_frames && f1 != f2)) { bits |= STATUS_PAIR; nnew[p] = -1; continue; }
        KfPose P1, P2;
        kf_pose(in->Tcw + 16 * (size_t)f1, P1);
        kf_pose(in->Tcw + 16 * (size_t)f2, P2);
        const bool skip = !monocular && np_short_baseline(P1, P2, K.mb);
        const int N1 = skip ? 0 : np_count(in->counts[(size_t)f1 * in->img_stride], capacity), N2 = np_count(in->counts[(size_t)f2 * in->img_stride], capacity);
        const olf_keypoint* kp1 = in->kps + (size_t)f1 * in->img_stride * cap;
        const olf_keypoint* kp2 = in->kps + (size_t)f2 * in->img_stride * cap;
        const size_t row = (size_t)p * cap, r1 = (size_t)f1 * cap, r2 = (size_t)f2 * cap;
        int created = 0;
        for (int i = 0; i < capacity; ++i) {
            float x[3] = {0.f, 0.f, 0.f};
            int c = NP_NONE;
            const int idx2 = i < N1 ? matches12[row + i] : -1;
            if ((unsigned)idx2 < (unsigned)N2) {
                const olf_keypoint &a = kp1[i], &b = kp2[idx2];
                if ((unsigned)a.octave < (unsigned)n_levels && (unsigned)b.octave < (unsigned)n_levels)
                    c = np_create_point(P1, P2, K, a.x, a.y, in->uright[r1 + i], depth[r1 + i], scale_factors[a.octave], b.x, b.y, in->uright[r2 + idx2],
                                        depth[r2 + idx2], scale_factors[b.octave], x);
                else bits |= STATUS_OCTAVE;
            }
            const bool made = c >= NP_TRIANGULATED && c <= NP_UNPROJECT_2;
            code[row + i] = (uint8_t)c;
            for (int k = 0; k < 3; ++k) x3D[3 * (row + i) + k] = made ? x[k] : 0.f;
            created += made;
        }
        nnew[p] = created;
    }
    *status = bits;
    return OLF_OK;
}

extern "C" int olf_update_normal_and_depth(const olf_map_graph* g, const olf_cull_view* v, int n_points, const int32_t* points, const float* mp_world,
                                           const int32_t* mp_ref_kf, const float* kf_Ow, const float* scale_factors, int n_levels, float* normal, float* maxd,
                                           float* mind, int32_t* status)
{
    const char* who = "olf_update_normal_and_depth";
    size_t n_obs = 0, n_slots = 0;
    bool ok = g && v && status && n_points >= 0 && g->n_kf >= 0 && g->n_mp >= 0 && scale_factors && n_levels >= 1 && n_levels <= OLF_MAX_LEVELS;
    ok = ok && csr_ok(g->mp_obs_offsets, g->mp_obs_kf, g->n_mp, &n_obs) && csr_ok(g->kf_mp_offsets, (const int32_t*)v->kf_slot_octave, g->n_kf, &n_slots);
    ok = ok && (v->mp_obs_slot || !n_obs) && ((g->mp_bad && mp_world && mp_ref_kf && normal && maxd && mind) || !g->n_mp) && (kf_Ow || !g->n_kf);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    NormalDepthView A;
    A.n_kf = g->n_kf; A.n_mp = g->n_mp; A.n_levels = n_levels;
    for (int k = 0; k < OLF_MAX_LEVELS; ++k) A.sf[k] = k < n_levels ? scale_factors[k] : 1.0f;
    A.obs_off = g->mp_obs_offsets; A.obs_kf = g->mp_obs_kf; A.obs_slot = v->mp_obs_slot; A.kmp_off = g->kf_mp_offsets; A.ref_kf = mp_ref_kf;
    A.mp_bad = g->mp_bad; A.slot_octave = v->kf_slot_octave;
    A.world = mp_world; A.Ow = kf_Ow; A.normal = normal; A.maxd = maxd; A.mind = mind;
    int bits = 0;
    for (int i = 0; i < n_points; ++i) normal_depth_point(A, points ? points[i] : i, &bits);
    *status = bits;
    return OLF_OK;
}
