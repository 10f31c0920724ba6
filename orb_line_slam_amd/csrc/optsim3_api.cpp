// optsim3_api.cpp -- olf_optimize_sim3_pairs: the host-pointer form of optsim3_batch.hip that runs on the device.  It stages the pairs' arrays at the
// context's capacity in one carve (the in / out rows and the outputs are uploaded first, so what the kernel leaves untouched comes back as it went in),
// runs the batched kernel on the context's stream and brings the outputs back.  (The form that needs no device is optsim3_host.cpp.)
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_optimize_sim3_pairs(olf_ctx* c, const olf_track_batch* in, int n_frames, const uint8_t* mp_bad, int n_pairs, const int32_t* pairs,
                                       const float* s12, const float* R12, const float* t12, float th2, int fix_scale, const int32_t* row_active,
                                       const olf_optimize_sim3_io* io)
{
    const char* who = "olf_optimize_sim3_pairs";
    bool ok = c && in && io && n_pairs >= 0 && n_frames >= 0 && th2 > 0.f;
    ok = ok && (!n_pairs || (pairs && s12 && R12 && t12 && in->kps && in->counts && in->img_stride >= 1 && in->Tcw && in->mp_world));
    ok = ok && (!n_pairs || (io->matches12 && io->S12_out && io->s12_out && io->R12_out && io->t12_out && io->Scw_out && io->n_inliers && io->n_correspondences &&
                             io->n_bad_first && io->iters && io->status && io->chi2));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    const size_t cap = (size_t)olf_orb_capacity(c), P = (size_t)n_pairs, F = (size_t)n_frames;
    const size_t images = F ? (F - 1) * (size_t)in->img_stride + 1 : 0;

    olf_keypoint* d_kps;
    int32_t *d_counts, *d_pairs, *d_act, *d_m, *d_nin, *d_nc, *d_nb, *d_iters, *d_status;
    float *d_Tcw, *d_mpw, *d_s, *d_R, *d_t, *d_so, *d_Ro, *d_to, *d_Scw, *d_chi2;
    double* d_S;
    uint8_t *d_valid, *d_bad;
    HostCall h(c, who);
    h.add(&d_S, P * 8);
    h.add(&d_kps, images * cap); h.add(&d_counts, images); h.add(&d_Tcw, F * 16); h.add(&d_mpw, F * cap * 3); h.add(&d_valid, F * cap); h.add(&d_bad, F * cap);
    h.add(&d_pairs, P * 2); h.add(&d_act, P); h.add(&d_s, P); h.add(&d_R, P * 9); h.add(&d_t, P * 3); h.add(&d_m, P * cap);
    h.add(&d_so, P); h.add(&d_Ro, P * 9); h.add(&d_to, P * 3); h.add(&d_Scw, P * 16); h.add(&d_nin, P); h.add(&d_nc, P); h.add(&d_nb, P); h.add(&d_iters, P * 2);
    h.add(&d_status, P); h.add(&d_chi2, P * cap * 2);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    if (n_pairs == 0) return h.finish();

    OLF_TRY(h.up(d_kps, in->kps, images * cap * sizeof(olf_keypoint))); OLF_TRY(h.up(d_counts, in->counts, images * 4)); OLF_TRY(h.up(d_Tcw, in->Tcw, F * 64));
    OLF_TRY(h.up(d_mpw, in->mp_world, F * cap * 12));
    if (in->mp_valid) OLF_TRY(h.up(d_valid, in->mp_valid, F * cap));
    if (mp_bad) OLF_TRY(h.up(d_bad, mp_bad, F * cap));
    if (row_active) OLF_TRY(h.up(d_act, row_active, P * 4));
    OLF_TRY(h.up(d_pairs, pairs, P * 8)); OLF_TRY(h.up(d_s, s12, P * 4)); OLF_TRY(h.up(d_R, R12, P * 36)); OLF_TRY(h.up(d_t, t12, P * 12));
    OLF_TRY(h.up(d_m, io->matches12, P * cap * 4)); OLF_TRY(h.up(d_S, io->S12_out, P * 64)); OLF_TRY(h.up(d_so, io->s12_out, P * 4)); OLF_TRY(h.up(d_Ro, io->R12_out, P * 36));
    OLF_TRY(h.up(d_to, io->t12_out, P * 12)); OLF_TRY(h.up(d_Scw, io->Scw_out, P * 64)); OLF_TRY(h.up(d_nin, io->n_inliers, P * 4));
    OLF_TRY(h.up(d_nc, io->n_correspondences, P * 4)); OLF_TRY(h.up(d_nb, io->n_bad_first, P * 4)); OLF_TRY(h.up(d_iters, io->iters, P * 8));
    OLF_TRY(h.up(d_status, io->status, P * 4)); OLF_TRY(h.up(d_chi2, io->chi2, P * cap * 8));

    olf_track_batch d = *in;
    d.kps = d_kps; d.counts = d_counts; d.Tcw = d_Tcw; d.mp_world = d_mpw; d.mp_valid = in->mp_valid ? d_valid : nullptr;
    d.desc = nullptr; d.uright = nullptr; d.cell_offsets = nullptr; d.cell_index = nullptr; d.mp_obs = nullptr; d.outlier = nullptr; d.mp_desc = nullptr;
    const olf_optimize_sim3_io dio = {d_m, d_S, d_so, d_Ro, d_to, d_Scw, d_nin, d_nc, d_nb, d_iters, d_status, d_chi2};
    OLF_TRY(olf_optimize_sim3_pairs_dev(c, &d, n_frames, mp_bad ? d_bad : nullptr, n_pairs, d_pairs, d_s, d_R, d_t, th2, fix_scale, row_active ? d_act : nullptr,
                                        &dio, h.stream()));
    OLF_TRY(h.down(io->matches12, d_m, P * cap * 4)); OLF_TRY(h.down(io->S12_out, d_S, P * 64)); OLF_TRY(h.down(io->s12_out, d_so, P * 4));
    OLF_TRY(h.down(io->R12_out, d_Ro, P * 36)); OLF_TRY(h.down(io->t12_out, d_to, P * 12)); OLF_TRY(h.down(io->Scw_out, d_Scw, P * 64));
    OLF_TRY(h.down(io->n_inliers, d_nin, P * 4)); OLF_TRY(h.down(io->n_correspondences, d_nc, P * 4)); OLF_TRY(h.down(io->n_bad_first, d_nb, P * 4));
    OLF_TRY(h.down(io->iters, d_iters, P * 8)); OLF_TRY(h.down(io->status, d_status, P * 4)); OLF_TRY(h.down(io->chi2, d_chi2, P * cap * 8));
    return h.finish_status();
}
