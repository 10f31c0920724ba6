// pose_api.cpp -- the host-pointer forms of pose_batch.hip that run on the device: olf_pose_optimization_with_line_frame and olf_discard_outliers_frame.
// Each stages one frame's rows at the context's capacities in one carve, runs the batched kernel on a batch of one and brings the outputs back.  (The forms
// that need no device are pose_host.cpp.)
#include <algorithm>
#include <vector>
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_pose_optimization_with_line_frame(olf_ctx* c, const olf_pose_batch* in, const olf_pose_params* params, const olf_pose_outputs* o)
{
    const char* who = "olf_pose_optimization_with_line_frame";
    bool ok = c && in && params && o && in->counts && in->lcounts && in->Tcw && in->n_mp >= 0 && in->n_ml >= 0 && (in->mp_world || !in->n_mp) && (in->ml_world || !in->n_ml);
    ok = ok && o->Tcw_out && o->DT && o->DT_cov && o->DT_cov_eig && o->err_norm && o->good && o->n_inliers && o->iters && o->status;
    const int cap = c ? olf_orb_capacity(c) : 0, lcap = c ? olf_line_capacity(c) : 0;
    const int n = ok ? in->counts[0] : 0, nl = ok ? in->lcounts[0] : 0;
    ok = ok && n >= 0 && nl >= 0 && ((in->kps && in->frame_mp && o->outlier_out) || !n) && ((in->kls && in->lle && in->frame_ml && o->outlier_l_out) || !nl);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n > cap || nl > lcap) { set_error(std::string(who) + ": more features than the context's capacities"); return OLF_ERR_CAPACITY; }

    const size_t nm = (size_t)in->n_mp, nml = (size_t)in->n_ml;
    olf_keypoint* d_kps; olf_keyline* d_kls;
    int32_t *d_counts, *d_lcounts, *d_fmp, *d_fml, *d_off, *d_offl, *d_inl, *d_iters, *d_status;
    double *d_lle, *d_cov_in, *d_DT, *d_cov, *d_eig, *d_err;
    float *d_Tcw, *d_Tprev, *d_mpw, *d_mlw, *d_Tout;
    uint8_t *d_out, *d_outl, *d_good;
    HostCall h(c, who);
    h.add(&d_kps, (size_t)cap); h.add(&d_kls, (size_t)lcap); h.add(&d_counts, 1); h.add(&d_lcounts, 1); h.add(&d_lle, 3 * (size_t)lcap); h.add(&d_Tcw, 16); h.add(&d_Tprev, 16);
    h.add(&d_cov_in, 36); h.add(&d_fmp, (size_t)cap); h.add(&d_fml, (size_t)lcap); h.add(&d_off, 1); h.add(&d_offl, 1); h.add(&d_mpw, 3 * nm); h.add(&d_mlw, 6 * nml);
    h.add(&d_out, (size_t)cap); h.add(&d_outl, (size_t)lcap); h.add(&d_Tout, 16); h.add(&d_DT, 16); h.add(&d_cov, 36); h.add(&d_eig, 6); h.add(&d_err, 1); h.add(&d_good, 1);
    h.add(&d_inl, 2); h.add(&d_iters, 4); h.add(&d_status, 1);
    OLF_TRY(h.bind(SCRATCH_STAGE));

    const int32_t off = in->mp_index_offset ? in->mp_index_offset[0] : 0, offl = in->ml_index_offset ? in->ml_index_offset[0] : 0;
    std::vector<uint8_t> flags((size_t)std::max(n, 1), 0), lflags((size_t)std::max(nl, 1), 0);
    if (in->outlier) std::copy(in->outlier, in->outlier + n, flags.begin());
    if (in->outlier_l) std::copy(in->outlier_l, in->outlier_l + nl, lflags.begin());
    OLF_TRY(h.up(d_kps, in->kps, (size_t)n * sizeof(olf_keypoint))); OLF_TRY(h.up(d_kls, in->kls, (size_t)nl * sizeof(olf_keyline)));
    OLF_TRY(h.up(d_counts, in->counts, 4)); OLF_TRY(h.up(d_lcounts, in->lcounts, 4)); OLF_TRY(h.up(d_lle, in->lle, (size_t)nl * 24));
    OLF_TRY(h.up(d_Tcw, in->Tcw, 64));
    if (in->Tcw_prev) OLF_TRY(h.up(d_Tprev, in->Tcw_prev, 64));
    if (in->DT_cov_in) OLF_TRY(h.up(d_cov_in, in->DT_cov_in, 288));
    OLF_TRY(h.up(d_fmp, in->frame_mp, (size_t)n * 4)); OLF_TRY(h.up(d_fml, in->frame_ml, (size_t)nl * 4)); OLF_TRY(h.up(d_off, &off, 4)); OLF_TRY(h.up(d_offl, &offl, 4));
    OLF_TRY(h.up(d_mpw, in->mp_world, nm * 12)); OLF_TRY(h.up(d_mlw, in->ml_world, nml * 24));
    OLF_TRY(h.up(d_out, flags.data(), (size_t)n)); OLF_TRY(h.up(d_outl, lflags.data(), (size_t)nl));

    olf_pose_batch d = *in;
    d.kps = d_kps; d.counts = d_counts; d.kls = d_kls; d.lcounts = d_lcounts; d.img_stride = 1; d.lle = d_lle; d.Tcw = d_Tcw; d.Tcw_prev = in->Tcw_prev ? d_Tprev : nullptr;
    d.DT_cov_in = in->DT_cov_in ? d_cov_in : nullptr; d.frame_mp = d_fmp; d.mp_index_offset = d_off; d.mp_world = d_mpw; d.frame_ml = d_fml; d.ml_index_offset = d_offl;
    d.ml_world = d_mlw; d.outlier = d_out; d.outlier_l = d_outl;                    // (the flags go in and come out in one row each)
    const olf_pose_outputs dout = {d_Tout, d_DT, d_cov, d_eig, d_err, d_good, d_out, d_outl, d_inl, d_iters, d_status};
    OLF_TRY(olf_pose_optimization_with_line_batch_dev(c, &d, 1, params, &dout, h.stream()));
    OLF_TRY(h.down(o->Tcw_out, d_Tout, 64)); OLF_TRY(h.down(o->DT, d_DT, 128)); OLF_TRY(h.down(o->DT_cov, d_cov, 288)); OLF_TRY(h.down(o->DT_cov_eig, d_eig, 48));
    OLF_TRY(h.down(o->err_norm, d_err, 8)); OLF_TRY(h.down(o->good, d_good, 1)); OLF_TRY(h.down(o->n_inliers, d_inl, 8)); OLF_TRY(h.down(o->iters, d_iters, 16));
    OLF_TRY(h.down(o->status, d_status, 4));
    if (n) OLF_TRY(h.down(o->outlier_out, d_out, (size_t)n));
    if (nl) OLF_TRY(h.down(o->outlier_l_out, d_outl, (size_t)nl));
    return h.finish_status();
}

extern "C" int olf_discard_outliers_frame(olf_ctx* c, const olf_discard_batch* io, int mode, int only_tracking, int stereo, int32_t* n_matches)
{
    const char* who = "olf_discard_outliers_frame";
    bool ok = c && io && n_matches && (mode == 0 || mode == 1) && io->counts && io->lcounts && io->n_mp >= 0 && io->n_ml >= 0;
    const int cap = c ? olf_orb_capacity(c) : 0, lcap = c ? olf_line_capacity(c) : 0;
    const int n = ok ? io->counts[0] : 0, nl = ok ? io->lcounts[0] : 0;
    ok = ok && n >= 0 && nl >= 0 && ((io->frame_mp && io->outlier) || !n) && ((io->frame_ml && io->outlier_l) || !nl);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n > cap || nl > lcap) { set_error(std::string(who) + ": more features than the context's capacities"); return OLF_ERR_CAPACITY; }
    const size_t nm = (size_t)io->n_mp, nml = (size_t)io->n_ml;
    int32_t *d_counts, *d_lcounts, *d_fmp, *d_fml, *d_off, *d_offl, *d_nm;
    uint8_t *d_out, *d_outl, *d_obs = nullptr, *d_lobs = nullptr;
    HostCall h(c, who);
    h.add(&d_counts, 1); h.add(&d_lcounts, 1); h.add(&d_fmp, (size_t)cap); h.add(&d_fml, (size_t)lcap); h.add(&d_out, (size_t)cap); h.add(&d_outl, (size_t)lcap);
    h.add(&d_off, 1); h.add(&d_offl, 1); h.add(&d_nm, 2);
    if (io->mp_obs) h.add(&d_obs, nm);
    if (io->ml_obs) h.add(&d_lobs, nml);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    const int32_t off = io->mp_index_offset ? io->mp_index_offset[0] : 0, offl = io->ml_index_offset ? io->ml_index_offset[0] : 0;
    OLF_TRY(h.up(d_counts, io->counts, 4)); OLF_TRY(h.up(d_lcounts, io->lcounts, 4)); OLF_TRY(h.up(d_fmp, io->frame_mp, (size_t)n * 4)); OLF_TRY(h.up(d_fml, io->frame_ml, (size_t)nl * 4));
    OLF_TRY(h.up(d_out, io->outlier, (size_t)n)); OLF_TRY(h.up(d_outl, io->outlier_l, (size_t)nl)); OLF_TRY(h.up(d_off, &off, 4)); OLF_TRY(h.up(d_offl, &offl, 4));
    if (io->mp_obs) OLF_TRY(h.up(d_obs, io->mp_obs, nm));
    if (io->ml_obs) OLF_TRY(h.up(d_lobs, io->ml_obs, nml));
    olf_discard_batch d = *io;
    d.counts = d_counts; d.lcounts = d_lcounts; d.img_stride = 1; d.frame_mp = d_fmp; d.frame_ml = d_fml; d.outlier = d_out; d.outlier_l = d_outl; d.mp_index_offset = d_off;
    d.ml_index_offset = d_offl; d.mp_obs = d_obs; d.ml_obs = d_lobs;
    OLF_TRY(olf_discard_outliers_batch_dev(c, &d, 1, mode, only_tracking, stereo, d_nm, h.stream()));
    if (n) { OLF_TRY(h.down(io->frame_mp, d_fmp, (size_t)n * 4)); OLF_TRY(h.down(io->outlier, d_out, (size_t)n)); }
    if (nl) { OLF_TRY(h.down(io->frame_ml, d_fml, (size_t)nl * 4)); OLF_TRY(h.down(io->outlier_l, d_outl, (size_t)nl)); }
    OLF_TRY(h.down(n_matches, d_nm, 8));
    return h.finish_status();
}
