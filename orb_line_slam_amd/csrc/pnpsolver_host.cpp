// pnpsolver_host.cpp -- the host form of pnpsolver_batch.hip: olf_pnp_solver, one PnPsolver (src/PnPsolver.cc) over host pointers, no context and no
// device.  The arithmetic is pnpsolver_terms.hpp, the text the kernel runs; the loop is PnPsolver::iterate as written (:165-258) with Refine (:260-305)
// run when the best set changes and its outcome carried (Refine is a function of the best set alone) -- the kernel takes the window as a scan, and the
// tests hold the two against each other and both against a literal restatement.
#include <vector>
#include "pnpsolver_terms.hpp"
#include "solver_args.hpp"
#include "olf_internal.hpp"
#include "../../include/orbline.h"

using namespace olf;

namespace olf {
bool pnp_ransac_ok(const olf_pnp_ransac* R)
{
    return R && R->min_inliers >= 1 && R->max_iterations >= 1 && R->n_iterations >= 0 && R->probability > 0.0 && R->probability < 1.0 && R->min_set == 4 &&
           R->epsilon > 0.0f && R->epsilon <= 1.0f && R->th2 > 0.0f;
}
bool pnp_io_ok(const olf_pnp_solver_io* io)
{
    return io && io->iterations_done && io->best_inliers && io->best_Tcw && io->best_flags && io->refined_inliers && io->refined_Tcw && io->refined_flags &&
           io->accepted && io->no_more && io->n_inliers && io->inliers && io->Tcw && io->n_correspondences;
}
}

extern "C" int olf_debug_pnp_solver_parameters(int N, const olf_pnp_ransac* R, int32_t* min_inliers, int32_t* cap)
{
    if (N < 0 || !pnp_ransac_ok(R) || !min_inliers || !cap) { set_error("olf_debug_pnp_solver_parameters: bad argument"); return OLF_ERR_INVALID; }
    int m, c;
    pnp_parameters(N, R->probability, R->min_inliers, R->max_iterations, R->min_set, R->epsilon, &m, &c);
    *min_inliers = m; *cap = c;
    return OLF_OK;
}

extern "C" int olf_pnp_solver(const olf_track_batch* in, int capacity, int n_frames, const uint8_t* mp_bad, const float* scale_factors, int n_levels, int kf,
                              int frame, const int32_t* matches, const olf_pnp_ransac* R, const uint32_t* draws, const olf_pnp_solver_io* io, int32_t* status)
{
    const char* who = "olf_pnp_solver";
    bool ok = in && status && capacity >= 0 && n_frames >= 0 && scale_factors && n_levels >= 1 && n_levels <= OLF_MAX_LEVELS && matches && draws;
    ok = ok && pnp_ransac_ok(R) && pnp_io_ok(io);
    ok = ok && (!n_frames || (in->kps && in->counts && in->img_stride >= 1 && in->mp_world));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    *status = 0;
    if (!(kf >= 0 && kf < n_frames && frame >= 0 && frame < n_frames && kf != frame)) { *status = STATUS_PAIR; *io->n_inliers = -1; return OLF_OK; }
    const size_t cap = (size_t)capacity, rk = (size_t)kf * cap;
    const int Nf = clampi(in->counts[(size_t)frame * in->img_stride], 0, capacity), Nk = clampi(in->counts[(size_t)kf * in->img_stride], 0, capacity);
    const olf_keypoint* kpf = in->kps + (size_t)frame * in->img_stride * cap;
    const double cam[4] = {(double)in->fx, (double)in->fy, (double)in->cx, (double)in->cy};
    // the constructor (:67-110) and mvMaxError (:154-156)
    const int room = Nf > 0 ? Nf : 1;
    std::vector<float> st((size_t)6 * room);
    std::vector<int> feat((size_t)room), list((size_t)room);
    int N = 0;
    for (int i = 0; i < Nf; ++i) {
        io->inliers[i] = 0;                                          // vbInliers.clear(), :168
        const int v = matches[i];
        if (!s3_is_match(v, Nk)) continue;
        if (in->mp_valid && !in->mp_valid[rk + v]) continue;
        if (mp_bad && mp_bad[rk + v]) continue;
        const int o = kpf[i].octave;
        if (!((unsigned)o < (unsigned)n_levels)) { *status |= STATUS_OCTAVE; continue; }
        for (int k = 0; k < 3; ++k) st[(size_t)k * room + N] = in->mp_world[3 * (rk + v) + k];
        st[(size_t)3 * room + N] = kpf[i].x; st[(size_t)4 * room + N] = kpf[i].y;
        st[(size_t)5 * room + N] = pnp_max_error(scale_factors[o], R->th2);
        feat[N++] = i;
    }
    const PnpPlanes P = {st.data(), room};
    *io->n_correspondences = N;
    *io->accepted = 0; *io->no_more = 0; *io->n_inliers = 0;
    int min_eff, cap_its;
    pnp_parameters(N, R->probability, R->min_inliers, R->max_iterations, R->min_set, R->epsilon, &min_eff, &cap_its);
    if (N < min_eff) { *io->no_more = 1; return OLF_OK; }            // :173-177
    int it = clampi(*io->iterations_done, 0, 1 << 30), best = *io->best_inliers, cur = 0;
    const int n_iterations = R->n_iterations < R->max_iterations ? R->n_iterations : R->max_iterations;
    std::vector<uint8_t> flags((size_t)N);
    std::vector<double> ws((size_t)PNP_WS);
    double Rm[9], tv[3];
    while (it < cap_its || cur < n_iterations) {                     // :182, an OR
        ++cur;
        const int j = it++, slot = j % R->max_iterations;            // C.26
        int idx[4];
        ransac_sample<4>(N, draws + 4 * (size_t)slot, idx);
        PnpSeqEnv e = {ws.data(), 1, P, idx[0], idx[1], idx[2], idx[3]};
        pnp_compute_pose(e, cam);
        int n = 0;
        if (pnp_result(e, Rm, tv)) {
            for (int q = 0; q < N; ++q) { flags[q] = P.inlier(q, Rm, tv, cam); n += flags[q]; }
        } else *status |= STATUS_PNP_DEGENERATE;
        if (io->counts) io->counts[slot] = n;
        if (n < min_eff) continue;                                   // :209
        if (n > best) {                                              // :212-224
            best = n;
            *io->best_inliers = n;
            pnp_tcw(Rm, tv, io->best_Tcw);
            int m = 0;
            for (int q = 0; q < N; ++q) { io->best_flags[feat[q]] = flags[q]; if (flags[q]) list[m++] = q; }
            // Refine (:260-305) of the new best set, its outcome carried
            PnpHostBlockEnv b = {ws.data(), P, list.data(), m};
            pnp_compute_pose(b, cam);
            double Rr[9], tr[3];
            int nr = 0;
            const bool full = pnp_result(b, Rr, tr);
            if (!full) *status |= STATUS_PNP_DEGENERATE;
            for (int q = 0; q < N; ++q) { const uint8_t f = full && P.inlier(q, Rr, tr, cam); io->refined_flags[feat[q]] = f; nr += f; }
            *io->refined_inliers = nr;
            pnp_tcw(Rr, tr, io->refined_Tcw);
        }
        if (*io->refined_inliers > min_eff) {                        // :226-236, :292
            *io->iterations_done = it;
            *io->accepted = 1;
            *io->n_inliers = *io->refined_inliers;
            for (int q = 0; q < N; ++q) io->inliers[feat[q]] = io->refined_flags[feat[q]];
            for (int k = 0; k < 16; ++k) io->Tcw[k] = io->refined_Tcw[k];
            return OLF_OK;
        }
    }
    *io->iterations_done = it;
    *io->no_more = 1;                                                // :241-243: the loop ends at or beyond the cap only
    if (best >= min_eff) {                                           // :244-254
        *io->accepted = 1;
        *io->n_inliers = best;
        for (int q = 0; q < N; ++q) io->inliers[feat[q]] = io->best_flags[feat[q]];
        for (int k = 0; k < 16; ++k) io->Tcw[k] = io->best_Tcw[k];
    }
    return OLF_OK;
}
