// sim3solver_host.cpp -- the host form of sim3solver_batch.hip: olf_sim3_solver, one Sim3Solver (src/Sim3Solver.cc) over host pointers, no context and no
// device.  The arithmetic is sim3solver_terms.hpp, the text the kernel runs; the loop is Sim3Solver::iterate as written (:140-207) -- the kernel takes the
// window as a scan, and the tests hold the two against each other.
#include <vector>
#include "sim3solver_terms.hpp"
#include "solver_args.hpp"
#include "olf_internal.hpp"
#include "../../include/orbline.h"

using namespace olf;

namespace {
struct Corr { float X1[3], X2[3], p1[2], p2[2], g1, g2; int i1; };
}

namespace olf {
bool sim3_ransac_ok(const olf_sim3_ransac* R)
{
    return R && R->min_inliers >= 3 && R->max_iterations >= 1 && R->n_iterations >= 0 && R->probability > 0.0 && R->probability < 1.0;
}
bool sim3_io_ok(const olf_sim3_solver_io* io)
{
    return io && io->iterations_done && io->best_inliers && io->best_s && io->best_R && io->best_t && io->best_T12 && io->accepted && io->no_more &&
           io->n_inliers && io->inliers && io->n_correspondences;
}
}

extern "C" int olf_debug_sim3_solver_gate(float scale_factor, uint64_t* gate)
{
    if (!gate) { set_error("olf_debug_sim3_solver_gate: bad argument"); return OLF_ERR_INVALID; }
    *gate = (uint64_t)s3_gate_int(scale_factor);
    return OLF_OK;
}

extern "C" int olf_debug_sim3_solver_cap(int N, double probability, int min_inliers, int max_iterations, int32_t* cap)
{
    if (!cap || N < 0 || min_inliers < 3 || max_iterations < 1 || !(probability > 0.0 && probability < 1.0)) { set_error("olf_debug_sim3_solver_cap: bad argument"); return OLF_ERR_INVALID; }
    *cap = s3_iteration_cap(N, probability, min_inliers, max_iterations);
    return OLF_OK;
}

extern "C" int olf_sim3_solver(const olf_track_batch* in, int capacity, int n_frames, const uint8_t* mp_bad, const float* scale_factors, int n_levels, int kf1,
                               int kf2, const int32_t* matches12, const olf_sim3_ransac* R, const uint32_t* draws, const olf_sim3_solver_io* io, int32_t* status)
{
    const char* who = "olf_sim3_solver";
    bool ok = in && status && capacity >= 0 && n_frames >= 0 && scale_factors && n_levels >= 1 && n_levels <= OLF_MAX_LEVELS && matches12 && draws;
    ok = ok && sim3_ransac_ok(R) && sim3_io_ok(io);
    ok = ok && (!n_frames || (in->kps && in->counts && in->img_stride >= 1 && in->Tcw && in->mp_world));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    *status = 0;
    if (!(kf1 >= 0 && kf1 < n_frames && kf2 >= 0 && kf2 < n_frames && kf1 != kf2)) { *status = STATUS_PAIR; *io->n_inliers = -1; return OLF_OK; }
    const size_t cap = (size_t)capacity, r1 = (size_t)kf1 * cap, r2 = (size_t)kf2 * cap;
    const int N1 = clampi(in->counts[(size_t)kf1 * in->img_stride], 0, capacity), N2 = clampi(in->counts[(size_t)kf2 * in->img_stride], 0, capacity);
    const olf_keypoint* kp1 = in->kps + (size_t)kf1 * in->img_stride * cap;
    const olf_keypoint* kp2 = in->kps + (size_t)kf2 * in->img_stride * cap;
    const float cam[4] = {in->fx, in->fy, in->cx, in->cy};
    // the constructor (:37-112)
    std::vector<Corr> cs;
    cs.reserve((size_t)N1);
    for (int i1 = 0; i1 < N1; ++i1) {
        io->inliers[i1] = 0;                                         // vbInliers = vector<bool>(mN1, false), :143
        const int v = matches12[i1];
        if (!s3_is_match(v, N2)) continue;
        if (in->mp_valid && !(in->mp_valid[r1 + i1] && in->mp_valid[r2 + v])) continue;
        if (mp_bad && (mp_bad[r1 + i1] || mp_bad[r2 + v])) continue;
        const int o1 = kp1[i1].octave, o2 = kp2[v].octave;
        if (!((unsigned)o1 < (unsigned)n_levels && (unsigned)o2 < (unsigned)n_levels)) { *status |= STATUS_OCTAVE; continue; }
        Corr c;
        rot_apply(in->Tcw + 16 * (size_t)kf1, in->mp_world + 3 * (r1 + i1), 1.0f, c.X1);
        rot_apply(in->Tcw + 16 * (size_t)kf2, in->mp_world + 3 * (r2 + v), 1.0f, c.X2);
        s3_image(c.X1, cam, c.p1);
        s3_image(c.X2, cam, c.p2);
        c.g1 = s3_gate(scale_factors[o1]); c.g2 = s3_gate(scale_factors[o2]);
        c.i1 = i1;
        cs.push_back(c);
    }
    const int N = (int)cs.size();
    *io->n_correspondences = N;
    *io->accepted = 0; *io->no_more = 0; *io->n_inliers = 0;
    if (N < R->min_inliers) { *io->no_more = 1; return OLF_OK; }      // :146-150
    const int cap_its = s3_iteration_cap(N, R->probability, R->min_inliers, R->max_iterations);
    int it = clampi(*io->iterations_done, 0, R->max_iterations), best = *io->best_inliers, cur = 0;
    std::vector<uint8_t> flags((size_t)N);
    while (it < cap_its && cur < R->n_iterations) {                  // :158
        ++cur;
        const int j = it++;
        int idx[3];
        ransac_sample<3>(N, draws + 3 * (size_t)j, idx);
        float P1[3][3], P2[3][3];
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) { P1[k][c] = cs[idx[k]].X1[c]; P2[k][c] = cs[idx[k]].X2[c]; }
        S3Hyp H;
        s3_fit(P1, P2, R->fix_scale != 0, H);
        int n = 0;
        for (int q = 0; q < N; ++q) {
            const Corr& c = cs[q];
            flags[q] = s3_inlier(H.T12, H.T21, cam, c.X1, c.X2, c.p1, c.p2, c.g1, c.g2);
            n += flags[q];
        }
        if (io->counts) io->counts[j] = n;
        if (n >= best) {                                             // :183-190
            best = n;
            *io->best_inliers = n;
            *io->best_s = H.s;
            for (int k = 0; k < 9; ++k) io->best_R[k] = H.R[k];
            for (int k = 0; k < 3; ++k) io->best_t[k] = H.t[k];
            for (int k = 0; k < 16; ++k) io->best_T12[k] = H.T12[k];
            if (n > R->min_inliers) {                                // :192-199
                *io->iterations_done = it;
                *io->accepted = 1;
                *io->n_inliers = n;
                for (int q = 0; q < N; ++q) if (flags[q]) io->inliers[cs[q].i1] = 1;
                return OLF_OK;
            }
        }
    }
    *io->iterations_done = it;
    if (it >= cap_its) *io->no_more = 1;                             // :203-204
    return OLF_OK;
}
