// keyframe_api.cpp -- the host-pointer forms of keyframe_batch.hip that run on the device: olf_stereo_landmarks_frames and olf_need_new_keyframe_frames.
// Each stages its caller's arrays and its outputs in one carve, runs the device entry on the context's stream and brings the outputs back.  Every output
// slot of a frame is written by the kernels, so the outputs are not uploaded.  (The forms that compute on the host, without a context, are
// keyframe_host.cpp.)
#include "keyframe_terms.hpp"
#include "staging.hpp"

using namespace olf;

namespace {
// a staged array: its device region, and the copy up where the caller gave one (an optional input stays NULL on the device too)
template <class T>
struct Staged {
    T* dev = nullptr;
    const T* host;
    size_t n;
    Staged(HostCall& h, const T* host_, size_t n_) : host(host_), n(n_) { if (host) h.add(&dev, n + 1); }
    int up(HostCall& h) { return host ? h.up(dev, host, n * sizeof(T)) : OLF_OK; }
    int down(HostCall& h, T* to) { return to ? h.down(to, dev, n * sizeof(T)) : OLF_OK; }
};
}  // namespace

extern "C" int olf_stereo_landmarks_frames(olf_ctx* c, const olf_landmarks_batch* in, int n_frames, int mode, const olf_landmarks_outputs* out)
{
    const char* who = "olf_stereo_landmarks_frames";
    if (!c || !lm_args_ok(in, n_frames, mode, out)) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n_frames == 0) return OLF_OK;
    const size_t cap = (size_t)olf_orb_capacity(c), lcap = (size_t)olf_line_capacity(c), nf = (size_t)n_frames, ni = nf * (size_t)in->img_stride;
    HostCall h(c, who);
    Staged<olf_keypoint> kps(h, in->kps, ni * cap);
    Staged<olf_keyline> kls(h, in->kls, ni * lcap);
    Staged<int32_t> counts(h, in->counts, ni), lcounts(h, in->lcounts, ni), fmp(h, in->frame_mp, nf * cap), fml(h, in->frame_ml, nf * lcap);
    Staged<int32_t> nobs(h, in->mp_nobs, (size_t)in->n_mp), lnobs(h, in->ml_nobs, (size_t)in->n_ml), bmp(h, in->new_base_mp, nf), bml(h, in->new_base_ml, nf);
    Staged<float> depth(h, in->depth, nf * cap), ldisp(h, in->ldisp, 2 * nf * lcap), Twc(h, in->Twc, 16 * nf);
    Staged<int32_t> o_nv(h, out->n_visited, 2 * nf), o_nc(h, out->n_created, 2 * nf), o_vo(h, out->visit_order, nf * cap), o_vl(h, out->visit_order_l, nf * lcap);
    Staged<int32_t> o_co(h, out->created_order, nf * cap), o_cl(h, out->created_order_l, nf * lcap), o_fp(h, out->frame_mp_out, nf * cap);
    Staged<int32_t> o_fl(h, out->frame_ml_out, nf * lcap), o_st(h, out->status, nf);
    Staged<uint8_t> o_cr(h, out->created, nf * cap), o_crl(h, out->created_l, nf * lcap);
    Staged<float> o_w(h, out->mp_world, 3 * nf * cap), o_n(h, out->mp_normal, 3 * nf * cap), o_max(h, out->mp_maxd, nf * cap), o_min(h, out->mp_mind, nf * cap);
    Staged<float> o_lw(h, out->ml_world, 6 * nf * lcap);
    Staged<double> o_lwd(h, out->ml_world_d, 6 * nf * lcap);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(kps.up(h)); OLF_TRY(kls.up(h)); OLF_TRY(counts.up(h)); OLF_TRY(lcounts.up(h)); OLF_TRY(fmp.up(h)); OLF_TRY(fml.up(h)); OLF_TRY(nobs.up(h));
    OLF_TRY(lnobs.up(h)); OLF_TRY(bmp.up(h)); OLF_TRY(bml.up(h)); OLF_TRY(depth.up(h)); OLF_TRY(ldisp.up(h)); OLF_TRY(Twc.up(h));
    olf_landmarks_batch d = *in;
    d.kps = kps.dev; d.kls = kls.dev; d.counts = counts.dev; d.lcounts = lcounts.dev; d.frame_mp = fmp.dev; d.frame_ml = fml.dev; d.mp_nobs = nobs.dev;
    d.ml_nobs = lnobs.dev; d.new_base_mp = bmp.dev; d.new_base_ml = bml.dev; d.depth = depth.dev; d.ldisp = ldisp.dev; d.Twc = Twc.dev;
    const olf_landmarks_outputs o = {o_nv.dev, o_nc.dev, o_vo.dev, o_vl.dev, o_co.dev, o_cl.dev, o_cr.dev, o_crl.dev, o_fp.dev, o_fl.dev, o_w.dev, o_n.dev, o_max.dev,
                                     o_min.dev, o_lwd.dev, o_lw.dev, o_st.dev};
    OLF_TRY(olf_stereo_landmarks_batch_dev(c, &d, n_frames, mode, &o, h.stream()));
    OLF_TRY(o_nv.down(h, out->n_visited)); OLF_TRY(o_nc.down(h, out->n_created)); OLF_TRY(o_vo.down(h, out->visit_order)); OLF_TRY(o_vl.down(h, out->visit_order_l));
    OLF_TRY(o_co.down(h, out->created_order)); OLF_TRY(o_cl.down(h, out->created_order_l)); OLF_TRY(o_fp.down(h, out->frame_mp_out));
    OLF_TRY(o_fl.down(h, out->frame_ml_out)); OLF_TRY(o_st.down(h, out->status)); OLF_TRY(o_cr.down(h, out->created)); OLF_TRY(o_crl.down(h, out->created_l));
    OLF_TRY(o_w.down(h, out->mp_world)); OLF_TRY(o_n.down(h, out->mp_normal)); OLF_TRY(o_max.down(h, out->mp_maxd)); OLF_TRY(o_min.down(h, out->mp_mind));
    OLF_TRY(o_lw.down(h, out->ml_world)); OLF_TRY(o_lwd.down(h, out->ml_world_d));
    return h.finish();
}

extern "C" int olf_need_new_keyframe_frames(olf_ctx* c, const olf_keyframe_test_batch* in, int n_frames, const olf_keyframe_test_outputs* out)
{
    const char* who = "olf_need_new_keyframe_frames";
    if (!c || !kf_args_ok(in, n_frames, out)) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n_frames == 0) return OLF_OK;
    const size_t cap = (size_t)olf_orb_capacity(c), lcap = (size_t)olf_line_capacity(c), nf = (size_t)n_frames, ni = nf * (size_t)in->img_stride;
    HostCall h(c, who);
    Staged<int32_t> counts(h, in->counts, ni), lcounts(h, in->lcounts, ni), fmp(h, in->frame_mp, nf * cap), fml(h, in->frame_ml, nf * lcap), lf(h, in->ldisp_frame, nf);
    Staged<int32_t> rows(h, in->rows, KF_ROW * nf), nref(h, in->n_ref_matches, nf), nrefl(h, in->n_ref_matches_l, nf), ninl(h, in->n_inliers, 2 * nf);
    Staged<float> depth(h, in->depth, nf * cap), ldisp(h, in->ldisp, 2 * nf * lcap);
    Staged<uint8_t> outl(h, in->outlier, nf * cap), outl_l(h, in->outlier_l, nf * lcap), o_need(h, out->need, nf), o_int(h, out->interrupt_ba, nf);
    Staged<int32_t> o_cnt(h, out->counts, 4 * nf), o_cond(h, out->conditions, nf), o_st(h, out->status, nf);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(counts.up(h)); OLF_TRY(lcounts.up(h)); OLF_TRY(fmp.up(h)); OLF_TRY(fml.up(h)); OLF_TRY(lf.up(h)); OLF_TRY(rows.up(h)); OLF_TRY(nref.up(h));
    OLF_TRY(nrefl.up(h)); OLF_TRY(ninl.up(h)); OLF_TRY(depth.up(h)); OLF_TRY(ldisp.up(h)); OLF_TRY(outl.up(h)); OLF_TRY(outl_l.up(h));
    olf_keyframe_test_batch d = *in;
    d.counts = counts.dev; d.lcounts = lcounts.dev; d.frame_mp = fmp.dev; d.frame_ml = fml.dev; d.ldisp_frame = lf.dev; d.rows = rows.dev; d.n_ref_matches = nref.dev;
    d.n_ref_matches_l = nrefl.dev; d.n_inliers = ninl.dev; d.depth = depth.dev; d.ldisp = ldisp.dev; d.outlier = outl.dev; d.outlier_l = outl_l.dev;
    const olf_keyframe_test_outputs o = {o_need.dev, o_int.dev, o_cnt.dev, o_cond.dev, o_st.dev};
    OLF_TRY(olf_need_new_keyframe_batch_dev(c, &d, n_frames, &o, h.stream()));
    OLF_TRY(o_need.down(h, out->need)); OLF_TRY(o_int.down(h, out->interrupt_ba)); OLF_TRY(o_cnt.down(h, out->counts)); OLF_TRY(o_cond.down(h, out->conditions));
    OLF_TRY(o_st.down(h, out->status));
    return h.finish();
}
