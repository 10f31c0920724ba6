// optsim3_host.cpp -- olf_optimize_sim3: int Optimizer::OptimizeSim3 (src/Optimizer.cc:2013-2208) for one key-frame pair on the host.  Plain C++ doubles,
// every sum in the order of the reference's _activeEdges (e12_i, e21_i for ascending i), no context and no device: the definition the kernel of
// optsim3_batch.hip is read against.  The Sim3 algebra, the edges' terms, the numeric Jacobian, the Levenberg loop and the driver are optsim3_terms.hpp /
// g2o_levenberg.hpp, shared with the kernel; this file owns the graph construction (:2066-2145) and the loops over a pair's correspondences.
#include <math.h>
#include <string>
#include <vector>
#include "optsim3_terms.hpp"
#include "../../include/orbline.h"

namespace olf { void set_error(const std::string& s); }

using namespace olf;
using namespace olf::optsim3;

namespace {

struct Corr { double P1[3], P2[3], obs1[2], obs2[2], w1, w2, e[4]; int i1; uint8_t f; };

struct HostOps {
    Cam c;
    double delta = 0.0;
    std::vector<Corr> cs;                                            // the correspondences in ascending i1
    int32_t* matches = nullptr;
    float* chi2 = nullptr;

    int n_edges() const { return (int)cs.size(); }
    int n_active() const { int k = 0; for (const Corr& q : cs) k += !(q.f & C_OUT); return k; }
    bool errors(const VertexSim3& v, bool, double* chi)
    {
        Sim3 inv;
        sim3_inverse(v.est, &inv);
        double s = 0.0;
        bool ok = true;
        for (Corr& q : cs) if (!(q.f & C_OUT)) {
            if (!corr_errors(c, v.est, inv, q.P1, q.P2, q.obs1, q.obs2, q.e)) { ok = false; continue; }
            s = s + edge_robust_chi2(q.e, q.w1, delta);
            s = s + edge_robust_chi2(q.e + 2, q.w2, delta);
        }
        *chi = s;
        return ok;
    }
    bool system(const VertexSim3& v, bool, double* S)
    {
        Sim3 pert[N_PERT];
        for (int k = 0; k < 14; ++k) perturbed(v, k, &pert[k], &pert[14 + k]);
        bool ok = true;
        for (int k = 0; k < N_SUMS; ++k) S[k] = 0.0;
        for (Corr& q : cs) if (!(q.f & C_OUT)) ok = corr_quadratic_form(c, pert, q.P1, q.P2, q.obs1, q.obs2, q.e, q.w1, q.w2, delta, S) && ok;
        return ok;
    }
    int check(double th2)
    {
        int bad = 0;
        for (Corr& q : cs) if (!(q.f & C_OUT)) {
            const double a = edge_chi2(q.e, q.w1), b = edge_chi2(q.e + 2, q.w2);
            chi2[2 * q.i1] = (float)a; chi2[2 * q.i1 + 1] = (float)b;
            if (a > th2 || b > th2) { q.f |= C_OUT; matches[q.i1] = -1; ++bad; }
        }
        return bad;
    }
};

inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace

extern "C" int olf_optimize_sim3(const olf_track_batch* in, int capacity, int n_frames, const uint8_t* mp_bad, const float* inv_level_sigma2, int n_levels,
                                 int kf1, int kf2, float s12, const float* R12, const float* t12, float th2, int fix_scale, const olf_optimize_sim3_io* io)
{
    const char* who = "olf_optimize_sim3";
    bool ok = in && io && capacity >= 0 && n_frames >= 0 && n_levels >= 0 && n_levels <= OLF_MAX_LEVELS && (inv_level_sigma2 || !n_levels) && R12 && t12 && th2 > 0.f;
    ok = ok && io->S12_out && io->s12_out && io->R12_out && io->t12_out && io->Scw_out && io->n_inliers && io->n_correspondences && io->n_bad_first &&
         io->iters && io->status && ((io->matches12 && io->chi2) || !capacity);
    ok = ok && (!n_frames || (in->counts && in->img_stride >= 1 && in->Tcw && ((in->kps && in->mp_world) || !capacity)));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    *io->status = 0;
    if (!(kf1 >= 0 && kf1 < n_frames && kf2 >= 0 && kf2 < n_frames && kf1 != kf2)) { *io->status = 2048; *io->n_inliers = -1; return OLF_OK; }
    const size_t cap = (size_t)capacity, r1 = (size_t)kf1 * cap, r2 = (size_t)kf2 * cap;
    const int N1 = clampi(in->counts[(size_t)kf1 * in->img_stride], 0, capacity), N2 = clampi(in->counts[(size_t)kf2 * in->img_stride], 0, capacity);
    const olf_keypoint* kp1 = in->kps + (size_t)kf1 * in->img_stride * cap;
    const olf_keypoint* kp2 = in->kps + (size_t)kf2 * in->img_stride * cap;

    HostOps ops;
    ops.c = {(double)in->fx, (double)in->fy, (double)in->cx, (double)in->cy};
    ops.delta = (double)sqrtf(th2);                                  // const float deltaHuber = sqrt(th2), :2062
    ops.matches = io->matches12; ops.chi2 = io->chi2;
    int status = 0;
    for (int i = 0; i < 2 * capacity; ++i) io->chi2[i] = 0.f;
    for (int i1 = 0; i1 < N1; ++i1) {                                // :2066-2145
        const int v = io->matches12[i1];
        if (!((unsigned)v < (unsigned)N2)) continue;
        if (in->mp_valid && !(in->mp_valid[r1 + i1] && in->mp_valid[r2 + v])) continue;
        if (mp_bad && (mp_bad[r1 + i1] || mp_bad[r2 + v])) continue;
        const int o1 = kp1[i1].octave, o2 = kp2[v].octave;
        if (!((unsigned)o1 < (unsigned)n_levels && (unsigned)o2 < (unsigned)n_levels)) { status |= ST_OCTAVE; continue; }
        Corr q;
        cam_point(in->Tcw + 16 * (size_t)kf1, in->mp_world + 3 * (r1 + i1), q.P1);
        cam_point(in->Tcw + 16 * (size_t)kf2, in->mp_world + 3 * (r2 + v), q.P2);
        q.obs1[0] = (double)kp1[i1].x; q.obs1[1] = (double)kp1[i1].y;
        q.obs2[0] = (double)kp2[v].x; q.obs2[1] = (double)kp2[v].y;
        q.w1 = (double)inv_level_sigma2[o1]; q.w2 = (double)inv_level_sigma2[o2];
        for (int k = 0; k < 4; ++k) q.e[k] = 0.0;
        q.i1 = i1; q.f = C_HELD;
        ops.cs.push_back(q);
    }
    Sim3 S12;
    sim3_from_floats(s12, R12, t12, &S12);
    Result r;
    run_pair(ops, S12, fix_scale != 0, (double)th2, &r);
    double R[9];
    quat_to_mat3(r.S12.q, R);
    for (int k = 0; k < 4; ++k) io->S12_out[k] = r.S12.q[k];
    for (int k = 0; k < 3; ++k) { io->S12_out[4 + k] = r.S12.t[k]; io->t12_out[k] = (float)r.S12.t[k]; }
    io->S12_out[7] = r.S12.s;
    *io->s12_out = (float)r.S12.s;
    for (int k = 0; k < 9; ++k) io->R12_out[k] = (float)R[k];
    sim3_scw(r.S12, in->Tcw + 16 * (size_t)kf2, io->Scw_out);
    *io->n_inliers = r.n_inliers; *io->n_correspondences = r.n_correspondences; *io->n_bad_first = r.n_bad_first;
    io->iters[0] = r.iters[0]; io->iters[1] = r.iters[1];
    *io->status = status | r.status;
    return OLF_OK;
}

// tests: the numeric Jacobian of one edge at an estimate.  S12 [8] = q (x, y, z, w), t, s; cam = fx, fy, cx, cy; X [3] the fixed point (P2c for e12, P1c
// for the inverse edge), obs [2]; J [2][7] row-major.  OLF_ERR_INVALID: a NULL pointer, or a depth of exactly 0 at a perturbed estimate.
extern "C" int olf_debug_optimize_sim3_jacobian(const double* S12, int fix_scale, const double* cam, const double* X, const double* obs, int inverse, double* J)
{
    if (!S12 || !cam || !X || !obs || !J) { set_error("olf_debug_optimize_sim3_jacobian: bad argument"); return OLF_ERR_INVALID; }
    VertexSim3 v;
    for (int k = 0; k < 4; ++k) v.est.q[k] = S12[k];
    for (int k = 0; k < 3; ++k) v.est.t[k] = S12[4 + k];
    v.est.s = S12[7];
    v.fix_scale = fix_scale != 0;
    Sim3 pert[N_PERT];
    for (int k = 0; k < 14; ++k) perturbed(v, k, &pert[k], &pert[14 + k]);
    const Cam c = {cam[0], cam[1], cam[2], cam[3]};
    double Jm[2][7];
    if (!edge_numeric_jacobian(c, inverse ? pert + 14 : pert, X, obs, Jm)) { set_error("olf_debug_optimize_sim3_jacobian: a depth of 0"); return OLF_ERR_INVALID; }
    for (int r = 0; r < 2; ++r) for (int d = 0; d < 7; ++d) J[r * 7 + d] = Jm[r][d];
    return OLF_OK;
}
