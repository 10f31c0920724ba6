// newpoints_api.cpp -- the host-pointer forms of newpoints_batch.hip that run on the device: olf_compute_f12_pairs, olf_create_new_map_points_pairs and
// olf_update_normal_and_depth_points.  Each checks what the device form leaves to its caller (the shape of the CSR pairs it reads), stages the arrays and
// the outputs in one carve -- the outputs are uploaded first, so what the device leaves untouched comes back as it went in -- and runs the same kernels.
// (The forms that compute on the host, without a context, are newpoints_host.cpp.)
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_compute_f12_pairs(olf_ctx* c, const float* Tcw, int n_frames, float fx, float fy, float cx, float cy, int n_pairs, const int32_t* pairs, float* F12)
{
    const char* who = "olf_compute_f12_pairs";
    if (!c || n_frames < 0 || n_pairs < 0 || (n_frames && !Tcw) || (n_pairs && (!pairs || !F12))) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n_pairs == 0) return OLF_OK;
    const size_t nf = (size_t)n_frames, np = (size_t)n_pairs;
    float *d_T, *d_F;
    int32_t* d_pairs;
    HostCall h(c, who);
    h.add(&d_T, 16 * nf + 1); h.add(&d_F, 9 * np); h.add(&d_pairs, 2 * np);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(d_T, Tcw, 64 * nf)); OLF_TRY(h.up(d_F, F12, 36 * np)); OLF_TRY(h.up(d_pairs, pairs, 8 * np));
    olf_track_batch in = {};
    in.Tcw = d_T; in.fx = fx; in.fy = fy; in.cx = cx; in.cy = cy;
    OLF_TRY(olf_compute_f12_pairs_dev(c, &in, n_frames, n_pairs, d_pairs, d_F, h.stream()));
    OLF_TRY(h.down(F12, d_F, 36 * np));
    return h.finish_status();
}

extern "C" int olf_create_new_map_points_pairs(olf_ctx* c, const olf_track_batch* in, int n_frames, const float* depth, float mb, int n_pairs, const int32_t* pairs,
                                               const int32_t* matches12, int monocular, float* x3D, uint8_t* code, int32_t* nnew)
{
    const char* who = "olf_create_new_map_points_pairs";
    bool ok = c && in && n_frames >= 0 && n_pairs >= 0 && (!n_pairs || (pairs && matches12 && x3D && code && nnew));
    ok = ok && (!n_frames || (in->kps && in->counts && in->img_stride >= 1 && in->uright && in->Tcw && depth));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n_pairs == 0) return OLF_OK;
    const size_t cap = (size_t)olf_orb_capacity(c), nf = (size_t)n_frames, ni = nf * (size_t)in->img_stride, np = (size_t)n_pairs;
    olf_keypoint* d_kps;
    int32_t *d_counts, *d_pairs, *d_m12, *d_nnew;
    float *d_ur, *d_depth, *d_T, *d_x;
    uint8_t* d_code;
    HostCall h(c, who);
    h.add(&d_kps, ni * cap + 1); h.add(&d_counts, ni + 1); h.add(&d_ur, nf * cap + 1); h.add(&d_depth, nf * cap + 1); h.add(&d_T, 16 * nf + 1);
    h.add(&d_pairs, 2 * np); h.add(&d_m12, np * cap); h.add(&d_x, 3 * np * cap); h.add(&d_nnew, np); h.add(&d_code, np * cap);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(d_kps, in->kps, ni * cap * sizeof(olf_keypoint))); OLF_TRY(h.up(d_counts, in->counts, ni * 4)); OLF_TRY(h.up(d_ur, in->uright, nf * cap * 4));
    OLF_TRY(h.up(d_depth, depth, nf * cap * 4)); OLF_TRY(h.up(d_T, in->Tcw, 64 * nf)); OLF_TRY(h.up(d_pairs, pairs, 8 * np)); OLF_TRY(h.up(d_m12, matches12, np * cap * 4));
    OLF_TRY(h.up(d_x, x3D, 12 * np * cap)); OLF_TRY(h.up(d_code, code, np * cap)); OLF_TRY(h.up(d_nnew, nnew, 4 * np));
    olf_track_batch d = *in;
    d.kps = d_kps; d.counts = d_counts; d.uright = d_ur; d.Tcw = d_T;
    OLF_TRY(olf_create_new_map_points_batch_dev(c, &d, n_frames, d_depth, mb, n_pairs, d_pairs, d_m12, monocular, d_x, d_code, d_nnew, h.stream()));
    OLF_TRY(h.down(x3D, d_x, 12 * np * cap)); OLF_TRY(h.down(code, d_code, np * cap)); OLF_TRY(h.down(nnew, d_nnew, 4 * np));
    return h.finish_status();
}

extern "C" int olf_update_normal_and_depth_points(olf_ctx* c, const olf_map_graph* g, const olf_cull_view* v, int n_points, const int32_t* points, const float* mp_world,
                                                  const int32_t* mp_ref_kf, const float* kf_Ow, float* normal, float* maxd, float* mind)
{
    const char* who = "olf_update_normal_and_depth_points";
    size_t n_obs = 0, n_slots = 0;
    bool ok = c && g && v && n_points >= 0 && g->n_kf >= 0 && g->n_mp >= 0;
    ok = ok && csr_ok(g->mp_obs_offsets, g->mp_obs_kf, g->n_mp, &n_obs) && csr_ok(g->kf_mp_offsets, (const int32_t*)v->kf_slot_octave, g->n_kf, &n_slots);
    ok = ok && (v->mp_obs_slot || !n_obs) && ((g->mp_bad && mp_world && mp_ref_kf && normal && maxd && mind) || !g->n_mp) && (kf_Ow || !g->n_kf);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n_points == 0) return OLF_OK;
    const size_t nm = (size_t)g->n_mp, nk = (size_t)g->n_kf, npt = (size_t)n_points;
    int32_t *d_obs_off, *d_obs_kf, *d_obs_slot, *d_kmp_off, *d_ref, *d_points = nullptr;
    uint8_t *d_bad, *d_oct;
    float *d_world, *d_Ow, *d_normal, *d_maxd, *d_mind;
    HostCall h(c, who);
    h.add(&d_obs_off, nm + 1); h.add(&d_obs_kf, n_obs + 1); h.add(&d_obs_slot, n_obs + 1); h.add(&d_kmp_off, nk + 1); h.add(&d_ref, nm + 1);
    if (points) h.add(&d_points, npt);
    h.add(&d_world, 3 * nm + 1); h.add(&d_Ow, 3 * nk + 1); h.add(&d_normal, 3 * nm + 1); h.add(&d_maxd, nm + 1); h.add(&d_mind, nm + 1);
    h.add(&d_bad, nm + 1); h.add(&d_oct, n_slots + 1);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(d_obs_off, g->mp_obs_offsets, (nm + 1) * 4)); OLF_TRY(h.up(d_obs_kf, g->mp_obs_kf, n_obs * 4)); OLF_TRY(h.up(d_obs_slot, v->mp_obs_slot, n_obs * 4));
    OLF_TRY(h.up(d_kmp_off, g->kf_mp_offsets, (nk + 1) * 4)); OLF_TRY(h.up(d_ref, mp_ref_kf, nm * 4));
    if (points) OLF_TRY(h.up(d_points, points, npt * 4));
    OLF_TRY(h.up(d_world, mp_world, 12 * nm)); OLF_TRY(h.up(d_Ow, kf_Ow, 12 * nk)); OLF_TRY(h.up(d_normal, normal, 12 * nm)); OLF_TRY(h.up(d_maxd, maxd, 4 * nm));
    OLF_TRY(h.up(d_mind, mind, 4 * nm)); OLF_TRY(h.up(d_bad, g->mp_bad, nm)); OLF_TRY(h.up(d_oct, v->kf_slot_octave, n_slots));
    olf_map_graph d = {};
    olf_cull_view dv = {};
    d.n_kf = g->n_kf; d.n_mp = g->n_mp;
    d.mp_obs_offsets = d_obs_off; d.mp_obs_kf = d_obs_kf; d.mp_bad = d_bad; d.kf_mp_offsets = d_kmp_off;
    dv.mp_obs_slot = d_obs_slot; dv.kf_slot_octave = d_oct;
    OLF_TRY(olf_update_normal_and_depth_dev(c, &d, &dv, n_points, d_points, d_world, d_ref, d_Ow, d_normal, d_maxd, d_mind, h.stream()));
    OLF_TRY(h.down(normal, d_normal, 12 * nm)); OLF_TRY(h.down(maxd, d_maxd, 4 * nm)); OLF_TRY(h.down(mind, d_mind, 4 * nm));
    return h.finish_status();
}
