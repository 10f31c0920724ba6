// posepoints_api.cpp -- olf_pose_optimization_rows: the host-pointer form of posepoints_batch.hip that runs on the device.  It stages the rows' arrays at
// the context's capacity in one carve (the outputs are uploaded first, so a row the kernel leaves untouched comes back as it went in), runs the batched
// kernel on the context's stream and brings the outputs back.  (The form that needs no device is posepoints_host.cpp.)
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_pose_optimization_rows(olf_ctx* c, const olf_pose_points_batch* in, int n_rows, int n_frames, const olf_pose_points_outputs* o)
{
    const char* who = "olf_pose_optimization_rows";
    bool ok = c && in && o && n_rows >= 0 && n_frames >= 0 && in->n_mp >= 0 && in->img_stride >= 1 && (in->pairs || n_rows <= n_frames);
    ok = ok && in->kps && in->counts && in->uright && in->Tcw && in->frame_mp && (in->mp_world || !in->n_mp);
    ok = ok && o->Tcw_out && o->outlier_out && o->n_good && o->n_initial && o->chi2 && o->passes && o->iters && o->status;
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    const size_t cap = (size_t)olf_orb_capacity(c), R = (size_t)n_rows, F = (size_t)n_frames, nm = (size_t)in->n_mp;
    const size_t images = F ? (F - 1) * (size_t)in->img_stride + 1 : 0;

    olf_keypoint* d_kps;
    int32_t *d_counts, *d_fmp, *d_off, *d_pairs, *d_act, *d_good, *d_init, *d_passes, *d_iters, *d_status;
    float *d_ur, *d_Tcw, *d_mpw, *d_Tout, *d_chi2;
    uint8_t* d_out;
    HostCall h(c, who);
    h.add(&d_kps, images * cap); h.add(&d_counts, images); h.add(&d_ur, F * cap); h.add(&d_Tcw, R * 16); h.add(&d_fmp, R * cap); h.add(&d_mpw, nm * 3);
    h.add(&d_off, R); h.add(&d_pairs, R * 2); h.add(&d_act, R); h.add(&d_Tout, R * 16); h.add(&d_out, R * cap); h.add(&d_good, R); h.add(&d_init, R);
    h.add(&d_chi2, R * cap); h.add(&d_passes, R); h.add(&d_iters, R * 4); h.add(&d_status, R);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    if (n_rows == 0) return h.finish();

    OLF_TRY(h.up(d_kps, in->kps, images * cap * sizeof(olf_keypoint))); OLF_TRY(h.up(d_counts, in->counts, images * 4)); OLF_TRY(h.up(d_ur, in->uright, F * cap * 4));
    OLF_TRY(h.up(d_Tcw, in->Tcw, R * 64)); OLF_TRY(h.up(d_fmp, in->frame_mp, R * cap * 4)); OLF_TRY(h.up(d_mpw, in->mp_world, nm * 12));
    if (in->mp_index_offset) OLF_TRY(h.up(d_off, in->mp_index_offset, R * 4));
    if (in->pairs) OLF_TRY(h.up(d_pairs, in->pairs, R * 8));
    if (in->row_active) OLF_TRY(h.up(d_act, in->row_active, R * 4));
    OLF_TRY(h.up(d_Tout, o->Tcw_out, R * 64)); OLF_TRY(h.up(d_out, o->outlier_out, R * cap)); OLF_TRY(h.up(d_good, o->n_good, R * 4)); OLF_TRY(h.up(d_init, o->n_initial, R * 4));
    OLF_TRY(h.up(d_chi2, o->chi2, R * cap * 4)); OLF_TRY(h.up(d_passes, o->passes, R * 4)); OLF_TRY(h.up(d_iters, o->iters, R * 16)); OLF_TRY(h.up(d_status, o->status, R * 4));

    olf_pose_points_batch d = *in;
    d.kps = d_kps; d.counts = d_counts; d.uright = d_ur; d.Tcw = d_Tcw; d.frame_mp = d_fmp; d.mp_world = d_mpw;
    d.mp_index_offset = in->mp_index_offset ? d_off : nullptr; d.pairs = in->pairs ? d_pairs : nullptr; d.row_active = in->row_active ? d_act : nullptr;
    const olf_pose_points_outputs dout = {d_Tout, d_out, d_good, d_init, d_chi2, d_passes, d_iters, d_status};
    OLF_TRY(olf_pose_optimization_batch_dev(c, &d, n_rows, n_frames, &dout, h.stream()));
    OLF_TRY(h.down(o->Tcw_out, d_Tout, R * 64)); OLF_TRY(h.down(o->outlier_out, d_out, R * cap)); OLF_TRY(h.down(o->n_good, d_good, R * 4));
    OLF_TRY(h.down(o->n_initial, d_init, R * 4)); OLF_TRY(h.down(o->chi2, d_chi2, R * cap * 4)); OLF_TRY(h.down(o->passes, d_passes, R * 4));
    OLF_TRY(h.down(o->iters, d_iters, R * 16)); OLF_TRY(h.down(o->status, d_status, R * 4));
    return h.finish_status();
}
