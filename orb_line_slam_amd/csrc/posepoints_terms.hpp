// posepoints_terms.hpp -- int Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:239-451) stated once for the host form (posepoints_host.cpp) and the
// batched kernel (posepoints_batch.hip): everything the reference executes through g2o for this graph -- one free VertexSE3Expmap, one
// EdgeSE3ProjectXYZOnlyPose or EdgeStereoSE3ProjectXYZOnlyPose per held feature, Huber kernels, OptimizationAlgorithmLevenberg over a BlockSolver with
// LinearSolverDense -- in plain C++ doubles, no Eigen, built with -ffp-contract=off on both sides.  What differs between the host and the device is only
// who sums: the drivers are templates over `Ops`, which owns the edges of one row (a serial loop on the host, a workgroup on the device, where every lane
// runs the driver on the same values and so takes the same branches).
//
// What is restated (Thirdparty/g2o/g2o/...):
//   types/types_six_dof_expmap.{h,cpp}   computeError and linearizeOplus of the two ...OnlyPose edges, VertexSE3Expmap::oplusImpl
//   types/se3quat.h, se3_ops.hpp         the constructor's normalizeRotation, map, exp (with its theta < 1e-5 branch), operator*, to_homogeneous_matrix
//   core/base_edge.h, base_unary_edge.hpp:43-72    chi2, constructQuadraticForm with rho[1] on b and on omega
// The Levenberg loop, Eigen's LDLT, the Huber kernel and the row status bits ST_DEPTH / ST_NOT_FINITE / ST_OCTAVE are g2o_levenberg.hpp; the matrix and
// quaternion pieces are dense_math.hpp.
//
// Conventions where the reference's build decides: an Eigen fixed-size product sums over k in ascending order and is formed before it
// is added to its destination; Quaterniond * Vector3d, the generic quaternion product and a quaternion's norm are dense_math.hpp's; LDLT is
// g2o_levenberg.hpp's.
//
// Beside what g2o_levenberg.hpp defines (a depth of exactly 0: ST_DEPTH; an H, b, step or estimate that is not finite: ST_NOT_FINITE; a failed LDLT), two
// things the reference leaves undefined, or that cannot happen through its call sites, are defined here:
//   - a stopped row returns Tcw_out = Tcw, its flags as they stood at that moment, n_good = 0 and the passes it completed;
//   - a pass whose active set is empty: g2o's initializeOptimization leaves the vertex out and optimize() returns before its first iteration; carrying the
//     algebra through instead (H = 0, b = 0, lambda = 0, LDLT of a zero matrix is "positive" with x = 0, rho = 0 / 1e-3 = 0: rejected, pop(), Terminate) ends
//     at the same place.  Either way the estimate is toSE3Quat(mTcw), iters = 0, and every edge -- all are flagged -- is classified with its error there.
#pragma once
#include "dense_math.hpp"
#include "g2o_levenberg.hpp"

namespace olf {
namespace posepoints {

using namespace dense;
using namespace levenberg;

enum { E_HELD = 1, E_OUT = 2, E_STEREO = 4 };                     // an edge's byte: holds a point, mvbOutlier (= level 1), the stereo kind

struct Cam { double fx, fy, cx, cy, bf; };
struct Se3 { double q[4], t[3]; };                                // g2o::SE3Quat: _r as x, y, z, w and _t

// Converter::toSE3Quat (src/Converter.cc:37-47): the floats widen, SE3Quat(R, t) normalises (quat_from_mat4)
PT_HD void se3_from_tcw(const float* Tcw, Se3* s)
{
    double T[16];
    for (int i = 0; i < 16; ++i) T[i] = (double)Tcw[i];
    quat_from_mat4(T, s->q);
    s->t[0] = T[3]; s->t[1] = T[7]; s->t[2] = T[11];
}
// SE3Quat::map, se3quat.h:217-220: _r * xyz + _t
PT_HD void se3_map(const Se3& s, const double* X, double* o)
{
    double r[3];
    quat_rotate(s.q, X, r);
    for (int i = 0; i < 3; ++i) o[i] = r[i] + s.t[i];
}
// SE3Quat::exp, se3quat.h:223-257: update = (omega, upsilon)
PT_HD void se3_exp(const double* u, Se3* s)
{
    const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]};
    const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
    double Om[9], OO[9], R[9], V[9];
    skew3(om, Om);
    mat3_mul(Om, Om, OO);
    if (theta < 0.00001) {
        for (int i = 0; i < 9; ++i) { R[i] = (((i % 4 == 0) ? 1.0 : 0.0) + Om[i]) + OO[i]; V[i] = R[i]; }
    } else {
        const double a = sin(theta) / theta, b = (1.0 - cos(theta)) / (theta * theta), c = (theta - sin(theta)) / pow(theta, 3.0);
        for (int i = 0; i < 9; ++i) {
            const double I = (i % 4 == 0) ? 1.0 : 0.0;
            R[i] = (I + a * Om[i]) + b * OO[i];
            V[i] = (I + b * Om[i]) + c * OO[i];
        }
    }
    double T[16];
    mat4_identity(T);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T[i * 4 + j] = R[i * 3 + j];
    quat_from_mat4(T, s->q);                                        // SE3Quat(Quaterniond(R), V * upsilon) normalises
    mat3_vec(V, up, s->t);
}
// SE3Quat::operator*, se3quat.h:104-110
PT_HD void se3_mul(const Se3& a, const Se3& b, Se3* o)
{
    double r[3], q[4];
    quat_rotate(a.q, b.t, r);
    quat_mul(a.q, b.q, q);
    for (int i = 0; i < 3; ++i) o->t[i] = a.t[i] + r[i];
    quat_normalize_positive(q);
    for (int i = 0; i < 4; ++i) o->q[i] = q[i];
}
PT_HD bool se3_finite(const Se3& s)
{
    bool ok = true;
    for (int i = 0; i < 4; ++i) ok = ok && finite_d(s.q[i]);
    for (int i = 0; i < 3; ++i) ok = ok && finite_d(s.t[i]);
    return ok;
}
// the vertex of this problem, as the Levenberg driver sees one: oplusImpl (types_six_dof_expmap.h:73-76) is SE3Quat::exp(update) * estimate
struct VertexSE3 {
    enum { D = 6 };
    Se3 est;
    PT_HD void oplus(const double* x) { Se3 e, r; se3_exp(x, &e); se3_mul(e, est, &r); est = r; }
    PT_HD bool finite() const { return se3_finite(est); }
};
// Converter::toCvMat(SE3Quat) (src/Converter.cc:51-55): to_homogeneous_matrix, every entry rounded to float
PT_HD void se3_to_tcw(const Se3& s, float* Tcw)
{
    double R[9];
    quat_to_mat3(s.q, R);
    for (int i = 0; i < 16; ++i) Tcw[i] = (i % 5 == 0) ? 1.f : 0.f;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Tcw[i * 4 + j] = (float)R[i * 3 + j]; Tcw[i * 4 + 3] = (float)s.t[i]; }
}

// ---- one edge ------------------------------------------------------------------------------------------------------------------------------------------
// Huber: delta is the float the reference forms (const float deltaMono = sqrt(5.991), :273-274) widened; dsqr = delta * delta (robust_kernel_impl.cpp:65-69)
PT_HD double huber_delta(bool stereo) { return stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991); }
PT_HD float chi2_threshold(bool stereo) { return stereo ? 7.815f : 5.991f; }        // chi2Mono / chi2Stereo, :369-370 (the same in all four passes)

// computeError (types_six_dof_expmap.h:153-157, :184-188) with cam_project (.cpp:290-306): obs - projection.  The stereo edge forms 1 / z in FLOAT
// (`const float invz = 1.0f / trans_xyz[2]`: a double quotient rounded to float).  false: the depth is exactly 0, nothing is written.
PT_HD bool edge_error(const Cam& c, const Se3& est, const double* Xw, const double* obs, bool stereo, double* e)
{
    double P[3];
    se3_map(est, Xw, P);
    if (P[2] == 0.0) return false;
    if (stereo) {
        const double invz = (double)(float)(1.0 / P[2]);
        const double u = (P[0] * invz) * c.fx + c.cx, v = (P[1] * invz) * c.fy + c.cy;
        e[0] = obs[0] - u; e[1] = obs[1] - v; e[2] = obs[2] - (u - c.bf * invz);
    } else {
        e[0] = obs[0] - ((P[0] / P[2]) * c.fx + c.cx); e[1] = obs[1] - ((P[1] / P[2]) * c.fy + c.cy); e[2] = 0.0;
    }
    return true;
}
// chi2 (base_edge.h:58-61): _error.dot(information * _error) with information = Identity * invSigma2
PT_HD double edge_chi2(const double* e, double w, bool stereo)
{
    double s = e[0] * (w * e[0]) + e[1] * (w * e[1]);
    if (stereo) s = s + e[2] * (w * e[2]);
    return s;
}
// what activeRobustChi2 (sparse_optimizer.cpp:100-114) adds for an edge
PT_HD double edge_robust_chi2(const double* e, double w, bool stereo, bool robust)
{
    const double chi = edge_chi2(e, w, stereo);
    if (!robust) return chi;
    double r0, r1;
    huber(chi, huber_delta(stereo), &r0, &r1);
    return r0;
}
// linearizeOplus (.cpp:266-288, :335-364) at est and constructQuadraticForm (base_unary_edge.hpp:43-72) with the edge's CURRENT _error e, added into
// S[27]: the 21 entries of H's lower triangle (row by row: 00, 10, 11, 20, ...) and the 6 of -b.  Each product is formed, then added.
// false: depth 0.
PT_HD bool edge_quadratic_form(const Cam& c, const Se3& est, const double* Xw, const double* e, double w, bool stereo, bool robust, double* S)
{
    double P[3], J[3][6];
    se3_map(est, Xw, P);
    if (P[2] == 0.0) return false;
    const double x = P[0], y = P[1], invz = 1.0 / P[2], invz_2 = invz * invz;
    J[0][0] = ((x * y) * invz_2) * c.fx;
    J[0][1] = (-(1.0 + ((x * x) * invz_2))) * c.fx;
    J[0][2] = (y * invz) * c.fx;
    J[0][3] = (-invz) * c.fx;
    J[0][4] = 0.0;
    J[0][5] = (x * invz_2) * c.fx;
    J[1][0] = (1.0 + ((y * y) * invz_2)) * c.fy;
    J[1][1] = (((-x) * y) * invz_2) * c.fy;
    J[1][2] = ((-x) * invz) * c.fy;
    J[1][3] = 0.0;
    J[1][4] = (-invz) * c.fy;
    J[1][5] = (y * invz_2) * c.fy;
    const int D = stereo ? 3 : 2;
    if (stereo) {
        J[2][0] = J[0][0] - ((c.bf * y) * invz_2);
        J[2][1] = J[0][1] + ((c.bf * x) * invz_2);
        J[2][2] = J[0][2];
        J[2][3] = J[0][3];
        J[2][4] = 0.0;
        J[2][5] = J[0][5] - c.bf * invz_2;
    }
    double rho1 = 1.0;
    if (robust) { double r0; huber(edge_chi2(e, w, stereo), huber_delta(stereo), &r0, &rho1); }
    const double ww = robust ? rho1 * w : w;                        // robustInformation (base_edge.h:96-102): rho[1] * _information
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {                              // (A^T * weightedOmega) * A at (i, j)
            double s = (J[0][i] * ww) * J[0][j] + (J[1][i] * ww) * J[1][j];
            if (D == 3) s = s + (J[2][i] * ww) * J[2][j];
            S[k] = S[k] + s;
            ++k;
        }
    for (int i = 0; i < 6; ++i) {                                   // ((rho[1] * A^T) * omega) * _error at i
        double s = robust ? ((rho1 * J[0][i]) * w) * e[0] + ((rho1 * J[1][i]) * w) * e[1] : (J[0][i] * w) * e[0] + (J[1][i] * w) * e[1];
        if (D == 3) s = s + (robust ? ((rho1 * J[2][i]) * w) * e[2] : (J[2][i] * w) * e[2]);
        S[21 + i] = S[21 + i] + s;
    }
    return true;
}

// ---- the four passes and the epilogue, src/Optimizer.cc:364-450 ---------------------------------------------------------------------------------------------
// Ops, beyond errors() and system() of lm_optimize (g2o_levenberg.hpp):
//       int  n_edges()                        nInitialCorrespondences = optimizer.edges().size(): the held features
//       int  n_active()                       edges of level 0
//       bool classify(const Se3& est, int* n_bad)      :382-438 for every edge: a flagged one gets computeError at est first, an unflagged one is read with
//                                             the _error the last errors() left; chi2 in float against the float threshold; false: a depth of 0
struct Result {
    float Tcw[16];
    int n_good, n_initial, passes, iters[4], status;
};
template <class Ops>
PT_HD void run_row(Ops& ops, const float* Tcw, Result* o)
{
    o->n_initial = ops.n_edges();
    o->n_good = 0; o->passes = 0; o->status = 0;
    for (int p = 0; p < 4; ++p) o->iters[p] = 0;
    for (int i = 0; i < 16; ++i) o->Tcw[i] = Tcw[i];
    if (o->n_initial < 3) return;                                   // :364-365
    VertexSE3 v;
    int n_bad = 0;
    bool robust = true, alive = true;
    for (int it = 0; it < 4; ++it) {
        se3_from_tcw(Tcw, &v.est);                                  // :377
        if (!v.finite()) { o->status |= ST_NOT_FINITE; alive = false; break; }
        if (ops.n_active() > 0) {
            const int n = lm_optimize(ops, v, 10, robust, &o->status);
            if (n == LM_STOP) { alive = false; break; }
            o->iters[it] = n;
        }
        if (!ops.classify(v.est, &n_bad)) { o->status |= ST_DEPTH; alive = false; break; }
        o->passes = it + 1;
        if (it == 2) robust = false;                                // setRobustKernel(0), :407-408
        if (o->n_initial < 10) break;                               // optimizer.edges().size() < 10, :440-441
    }
    if (!alive) return;
    se3_to_tcw(v.est, o->Tcw);                                      // :445-448
    o->n_good = o->n_initial - n_bad;
}

}  // namespace posepoints
}  // namespace olf
