// pnpsolver_api.cpp -- the host-pointer form of pnpsolver_batch.hip that runs on the device: olf_pnp_solver_pairs.  It stages the arrays, the carried
// state and the outputs in one carve -- the outputs are uploaded first, so what the device leaves untouched (a refused pair, a row's tail, counts of
// iterations not evaluated, the pose of a call that returns none) comes back as it went in -- and runs the same kernel.  (The form that computes on the
// host is pnpsolver_host.cpp.)
#include "solver_args.hpp"
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_pnp_solver_pairs(olf_ctx* c, const olf_track_batch* in, int n_frames, const uint8_t* mp_bad, int n_pairs, const int32_t* pairs,
                                    const int32_t* matches, const olf_pnp_ransac* R, const uint32_t* draws, const olf_pnp_solver_io* io)
{
    const char* who = "olf_pnp_solver_pairs";
    bool ok = c && in && io && n_frames >= 0 && n_pairs >= 0 && pnp_ransac_ok(R);
    ok = ok && (!n_pairs || (pairs && matches && draws && pnp_io_ok(io)));
    ok = ok && (!n_frames || (in->kps && in->counts && in->img_stride >= 1 && in->mp_world));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n_pairs == 0) return OLF_OK;
    const size_t cap = (size_t)olf_orb_capacity(c), nf = (size_t)n_frames, ni = nf * (size_t)in->img_stride, np = (size_t)n_pairs, mi = (size_t)R->max_iterations;
    olf_keypoint* d_kps;
    int32_t *d_counts, *d_pairs, *d_m, *d_done, *d_best, *d_ref, *d_acc, *d_nomore, *d_ninl, *d_ncorr, *d_cnt = nullptr;
    float *d_world, *d_bT, *d_rT, *d_T;
    uint8_t *d_valid = nullptr, *d_bad = nullptr, *d_bf, *d_rf, *d_inl;
    uint32_t* d_draws;
    HostCall h(c, who);
    h.add(&d_kps, ni * cap + 1); h.add(&d_counts, ni + 1); h.add(&d_world, 3 * nf * cap + 1);
    h.add(&d_pairs, 2 * np); h.add(&d_m, np * cap); h.add(&d_draws, 4 * np * mi);
    h.add(&d_done, np); h.add(&d_best, np); h.add(&d_ref, np); h.add(&d_bT, 16 * np); h.add(&d_rT, 16 * np); h.add(&d_T, 16 * np);
    h.add(&d_acc, np); h.add(&d_nomore, np); h.add(&d_ninl, np); h.add(&d_ncorr, np);
    if (io->counts) h.add(&d_cnt, np * mi);
    h.add(&d_bf, np * cap); h.add(&d_rf, np * cap); h.add(&d_inl, np * cap);
    if (in->mp_valid) h.add(&d_valid, nf * cap + 1);
    if (mp_bad) h.add(&d_bad, nf * cap + 1);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(d_kps, in->kps, ni * cap * sizeof(olf_keypoint))); OLF_TRY(h.up(d_counts, in->counts, ni * 4));
    OLF_TRY(h.up(d_world, in->mp_world, 12 * nf * cap)); OLF_TRY(h.up(d_pairs, pairs, 8 * np)); OLF_TRY(h.up(d_m, matches, 4 * np * cap));
    OLF_TRY(h.up(d_draws, draws, 16 * np * mi));
    OLF_TRY(h.up(d_done, io->iterations_done, 4 * np)); OLF_TRY(h.up(d_best, io->best_inliers, 4 * np)); OLF_TRY(h.up(d_ref, io->refined_inliers, 4 * np));
    OLF_TRY(h.up(d_bT, io->best_Tcw, 64 * np)); OLF_TRY(h.up(d_rT, io->refined_Tcw, 64 * np)); OLF_TRY(h.up(d_T, io->Tcw, 64 * np));
    OLF_TRY(h.up(d_acc, io->accepted, 4 * np)); OLF_TRY(h.up(d_nomore, io->no_more, 4 * np)); OLF_TRY(h.up(d_ninl, io->n_inliers, 4 * np));
    OLF_TRY(h.up(d_ncorr, io->n_correspondences, 4 * np));
    OLF_TRY(h.up(d_bf, io->best_flags, np * cap)); OLF_TRY(h.up(d_rf, io->refined_flags, np * cap)); OLF_TRY(h.up(d_inl, io->inliers, np * cap));
    if (d_cnt) OLF_TRY(h.up(d_cnt, io->counts, 4 * np * mi));
    if (d_valid) OLF_TRY(h.up(d_valid, in->mp_valid, nf * cap));
    if (d_bad) OLF_TRY(h.up(d_bad, mp_bad, nf * cap));
    olf_track_batch d = *in;
    d.kps = d_kps; d.counts = d_counts; d.mp_world = d_world; d.mp_valid = d_valid;
    const olf_pnp_solver_io dio = {d_done, d_best, d_bT, d_bf, d_ref, d_rT, d_rf, d_acc, d_nomore, d_ninl, d_inl, d_T, d_ncorr, d_cnt};
    OLF_TRY(olf_pnp_solver_pairs_dev(c, &d, n_frames, d_bad, n_pairs, d_pairs, d_m, R, d_draws, &dio, h.stream()));
    OLF_TRY(h.down(io->iterations_done, d_done, 4 * np)); OLF_TRY(h.down(io->best_inliers, d_best, 4 * np)); OLF_TRY(h.down(io->refined_inliers, d_ref, 4 * np));
    OLF_TRY(h.down(io->best_Tcw, d_bT, 64 * np)); OLF_TRY(h.down(io->refined_Tcw, d_rT, 64 * np)); OLF_TRY(h.down(io->Tcw, d_T, 64 * np));
    OLF_TRY(h.down(io->accepted, d_acc, 4 * np)); OLF_TRY(h.down(io->no_more, d_nomore, 4 * np)); OLF_TRY(h.down(io->n_inliers, d_ninl, 4 * np));
    OLF_TRY(h.down(io->n_correspondences, d_ncorr, 4 * np));
    OLF_TRY(h.down(io->best_flags, d_bf, np * cap)); OLF_TRY(h.down(io->refined_flags, d_rf, np * cap)); OLF_TRY(h.down(io->inliers, d_inl, np * cap));
    if (d_cnt) OLF_TRY(h.down(io->counts, d_cnt, 4 * np * mi));
    return h.finish_status();
}
