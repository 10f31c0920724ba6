// initializer_api.cpp -- the host-pointer form of initializer_batch.hip that runs on the device: olf_initializer_pairs.  It stages the arrays and the
// outputs in one carve -- the outputs are uploaded first, so what the device leaves untouched (a refused pair, a row's tail, H21 of a RANSAC without a
// score, R21 / t21 / P3D of a pair that did not initialise) comes back as it went in -- and runs the same kernel.  (The form that computes on the host is
// initializer_host.cpp.)
#include "solver_args.hpp"
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_initializer_pairs(olf_ctx* c, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* pairs, const int32_t* matches,
                                     const olf_initializer_params* prm, const uint32_t* draws, const olf_initializer_io* io)
{
    const char* who = "olf_initializer_pairs";
    bool ok = c && in && io && n_frames >= 0 && n_pairs >= 0 && ini_params_ok(prm);
    ok = ok && (!n_pairs || (pairs && matches && draws && ini_io_ok(io)));
    ok = ok && (!n_frames || (in->kps && in->counts && in->img_stride >= 1));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n_pairs == 0) return OLF_OK;
    const size_t cap = (size_t)olf_orb_capacity(c), ni = (size_t)n_frames * (size_t)in->img_stride, np = (size_t)n_pairs, mi = (size_t)prm->max_iterations;
    olf_keypoint* d_kps;
    int32_t *d_counts, *d_pairs, *d_m, *d_ok, *d_nc, *d_model, *d_ng, *d_hyp;
    float *d_sh, *d_sf, *d_H, *d_F, *d_R, *d_t, *d_P, *d_cos;
    uint8_t *d_iH, *d_iF, *d_tri;
    uint32_t* d_draws;
    HostCall h(c, who);
    h.add(&d_kps, ni * cap + 1); h.add(&d_counts, ni + 1); h.add(&d_pairs, 2 * np); h.add(&d_m, np * cap); h.add(&d_draws, 8 * np * mi);
    h.add(&d_ok, np); h.add(&d_nc, np); h.add(&d_model, np); h.add(&d_sh, np); h.add(&d_sf, np); h.add(&d_H, 9 * np); h.add(&d_F, 9 * np);
    h.add(&d_R, 9 * np); h.add(&d_t, 3 * np); h.add(&d_P, 3 * np * cap + 1); h.add(&d_ng, 8 * np); h.add(&d_cos, 8 * np); h.add(&d_hyp, np);
    h.add(&d_iH, np * cap + 1); h.add(&d_iF, np * cap + 1); h.add(&d_tri, np * cap + 1);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(d_kps, in->kps, ni * cap * sizeof(olf_keypoint))); OLF_TRY(h.up(d_counts, in->counts, ni * 4));
    OLF_TRY(h.up(d_pairs, pairs, 8 * np)); OLF_TRY(h.up(d_m, matches, 4 * np * cap)); OLF_TRY(h.up(d_draws, draws, 32 * np * mi));
    OLF_TRY(h.up(d_ok, io->ok, 4 * np)); OLF_TRY(h.up(d_nc, io->n_correspondences, 4 * np)); OLF_TRY(h.up(d_model, io->model, 4 * np));
    OLF_TRY(h.up(d_sh, io->score_H, 4 * np)); OLF_TRY(h.up(d_sf, io->score_F, 4 * np)); OLF_TRY(h.up(d_H, io->H21, 36 * np)); OLF_TRY(h.up(d_F, io->F21, 36 * np));
    OLF_TRY(h.up(d_R, io->R21, 36 * np)); OLF_TRY(h.up(d_t, io->t21, 12 * np)); OLF_TRY(h.up(d_P, io->P3D, 12 * np * cap));
    OLF_TRY(h.up(d_ng, io->n_good, 32 * np)); OLF_TRY(h.up(d_cos, io->cos_parallax, 32 * np)); OLF_TRY(h.up(d_hyp, io->hypothesis, 4 * np));
    OLF_TRY(h.up(d_iH, io->inliers_H, np * cap)); OLF_TRY(h.up(d_iF, io->inliers_F, np * cap)); OLF_TRY(h.up(d_tri, io->triangulated, np * cap));
    olf_track_batch d = *in;
    d.kps = d_kps; d.counts = d_counts;
    const olf_initializer_io dio = {d_ok, d_nc, d_model, d_sh, d_sf, d_H, d_F, d_iH, d_iF, d_R, d_t, d_P, d_tri, d_ng, d_cos, d_hyp};
    OLF_TRY(olf_initializer_pairs_dev(c, &d, n_frames, n_pairs, d_pairs, d_m, prm, d_draws, &dio, h.stream()));
    OLF_TRY(h.down(io->ok, d_ok, 4 * np)); OLF_TRY(h.down(io->n_correspondences, d_nc, 4 * np)); OLF_TRY(h.down(io->model, d_model, 4 * np));
    OLF_TRY(h.down(io->score_H, d_sh, 4 * np)); OLF_TRY(h.down(io->score_F, d_sf, 4 * np)); OLF_TRY(h.down(io->H21, d_H, 36 * np)); OLF_TRY(h.down(io->F21, d_F, 36 * np));
    OLF_TRY(h.down(io->R21, d_R, 36 * np)); OLF_TRY(h.down(io->t21, d_t, 12 * np)); OLF_TRY(h.down(io->P3D, d_P, 12 * np * cap));
    OLF_TRY(h.down(io->n_good, d_ng, 32 * np)); OLF_TRY(h.down(io->cos_parallax, d_cos, 32 * np)); OLF_TRY(h.down(io->hypothesis, d_hyp, 4 * np));
    OLF_TRY(h.down(io->inliers_H, d_iH, np * cap)); OLF_TRY(h.down(io->inliers_F, d_iF, np * cap)); OLF_TRY(h.down(io->triangulated, d_tri, np * cap));
    return h.finish_status();
}
