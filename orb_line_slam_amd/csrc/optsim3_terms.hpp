// optsim3_terms.hpp -- int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:2013-2208) stated once for the host form
// (optsim3_host.cpp) and the batched kernel (optsim3_batch.hip): one free VertexSim3Expmap, per correspondence one EdgeSim3ProjectXYZ (e12) and one
// EdgeInverseSim3ProjectXYZ (e21) against fixed points, Huber kernels, OptimizationAlgorithmLevenberg over LinearSolverDense -- in plain C++ doubles, no
// Eigen, built with -ffp-contract=off on both sides.  The Levenberg loop (lm_optimize<V, Ops>), Eigen's LDLT (ldlt_solve<7>), the Huber kernel and the
// row status bits are g2o_levenberg.hpp, the quaternion and 3 x 3 pieces dense_math.hpp; what is stated here is what is specific to this graph.
//
// What is restated (Thirdparty/g2o/g2o/...):
//   types/sim3.h                          the Vector7d constructor with its four branches, map, inverse, operator* (no normalisation anywhere)
//   types/types_seven_dof_expmap.h        VertexSim3Expmap::oplusImpl (update[6] = 0 is written INTO the caller's array), cam_map1 / cam_map2, the two computeError
//   core/base_binary_edge.hpp:55-204      the NUMERIC linearizeOplus of the Sim3 vertex (the edges have no analytic Jacobian; the points are fixed) and
//                                         constructQuadraticForm's robust branch
//
// Conventions (with C.27's): the 14 perturbed estimates Sim3(+-1e-9 e_d) * estimate and their inverses depend on the vertex alone, so they
// are formed once per linearisation (perturbed()) and every edge reads them -- the same bits as g2o's per-edge oplus / pop; an edge's _error is not touched
// by its linearisation (g2o restores it).  -omega * _error is (-(w e)), exactly; the sums carry -b, whose terms are the exact negatives of b's.
// information * _error with information = Identity * invSigma2 is w e per component (the zero off-diagonal adds nothing).
//
// Defined here, not by the reference, with g2o_levenberg.hpp: a depth of exactly 0 at any evaluation, the perturbed ones included (ST_DEPTH), and an H,
// b, step or estimate that is not finite (ST_NOT_FINITE) stop the pair: S12_out = the input, the matches as they stood, n_inliers = 0.  An empty graph:
// optimize() returns at once, nothing is bad, 0 - 0 < 10 returns 0.
#pragma once
#include "dense_math.hpp"
#include "g2o_levenberg.hpp"

namespace olf {
namespace optsim3 {

using namespace dense;
using namespace levenberg;

enum { C_HELD = 1, C_OUT = 2 };                                     // a correspondence's byte: both edges are in the graph; both were removed
enum { N_H = 28, N_SUMS = 35, N_PERT = 28 };                        // H's lower triangle, + 7 of -b; 14 perturbed estimates and their 14 inverses

struct Cam { double fx, fy, cx, cy; };                              // _focal_length / _principle_point: K's floats widened (K1 = K2 here)
struct Sim3 { double q[4], t[3], s; };                              // g2o::Sim3: r as x, y, z, w (not normalised), t, s

// Sim3(const Matrix3d& R, const Vector3d& t, double s) of floats (:2038 through LoopClosing.cc:325-327 and Converter::toMatrix3d / toVector3d)
PT_HD void sim3_from_floats(float s, const float* R, const float* t, Sim3* o)
{
    double M[9];
    for (int i = 0; i < 9; ++i) M[i] = (double)R[i];
    quat_of_rotation(M, 3, o->q);
    for (int i = 0; i < 3; ++i) o->t[i] = (double)t[i];
    o->s = (double)s;
}
// P3D1c = R1w * P3D1w + t1w (:2085, :2093): float cv::Mat arithmetic under C.12 -- the three products summed in float, the t term added in double, one
// rounding -- then widened (Converter::toVector3d).  The statement is rot_apply's (search_math.hpp, what sim3solver_host.cpp runs for Sim3Solver.cc's same
// expression), spelled here because this header also builds without the HIP headers.
PT_HD void cam_point(const float* T, const float* P, double* o)
{
    for (int r = 0; r < 3; ++r) {
        const float d = T[4 * r] * P[0] + T[4 * r + 1] * P[1] + T[4 * r + 2] * P[2];
        o[r] = (double)(float)((double)d + (double)1.0f * (double)T[4 * r + 3]);
    }
}
// Sim3(const Vector7d& update), sim3.h:70-142: update = (omega, upsilon, sigma)
PT_HD void sim3_exp(const double* u, Sim3* o)
{
    const double om[3] = {u[0], u[1], u[2]}, up[3] = {u[3], u[4], u[5]}, sigma = u[6];
    const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
    double Om[9], O2[9], R[9], W[9], A, B, C;
    skew3(om, Om);
    const double s = exp(sigma);
    mat3_mul(Om, Om, O2);
    const double eps = 0.00001;
    const bool small = theta < eps;
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (small) { A = 1. / 2.; B = 1. / 6.; }
        else {
            const double theta2 = theta * theta;
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (small) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta), b = s * cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2;
        }
    }
    if (small) {
        for (int i = 0; i < 9; ++i) R[i] = (((i % 4 == 0) ? 1.0 : 0.0) + Om[i]) + O2[i];
    } else {
        const double ra = sin(theta) / theta, rb = (1.0 - cos(theta)) / (theta * theta);
        for (int i = 0; i < 9; ++i) R[i] = (((i % 4 == 0) ? 1.0 : 0.0) + ra * Om[i]) + rb * O2[i];
    }
    quat_of_rotation(R, 3, o->q);
    for (int i = 0; i < 9; ++i) W[i] = (A * Om[i] + B * O2[i]) + C * ((i % 4 == 0) ? 1.0 : 0.0);
    mat3_vec(W, up, o->t);
    o->s = s;
}
// Sim3::map, :144-146: s * (r * xyz) + t
PT_HD void sim3_map(const Sim3& S, const double* X, double* o)
{
    double r[3];
    quat_rotate(S.q, X, r);
    for (int i = 0; i < 3; ++i) o[i] = S.s * r[i] + S.t[i];
}
// Sim3::inverse, :233-236: Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
PT_HD void sim3_inverse(const Sim3& S, Sim3* o)
{
    const double qc[4] = {-S.q[0], -S.q[1], -S.q[2], S.q[3]}, f = -1. / S.s;
    const double ft[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
    double r[3];
    quat_rotate(qc, ft, r);
    for (int i = 0; i < 4; ++i) o->q[i] = qc[i];
    for (int i = 0; i < 3; ++i) o->t[i] = r[i];
    o->s = 1. / S.s;
}
// Sim3::operator*, :266-272
PT_HD void sim3_mul(const Sim3& a, const Sim3& b, Sim3* o)
{
    double q[4], r[3];
    quat_mul(a.q, b.q, q);
    quat_rotate(a.q, b.t, r);
    for (int i = 0; i < 3; ++i) o->t[i] = a.s * r[i] + a.t[i];
    for (int i = 0; i < 4; ++i) o->q[i] = q[i];
    o->s = a.s * b.s;
}
PT_HD bool sim3_finite(const Sim3& S)
{
    bool ok = finite_d(S.s);
    for (int i = 0; i < 4; ++i) ok = ok && finite_d(S.q[i]);
    for (int i = 0; i < 3; ++i) ok = ok && finite_d(S.t[i]);
    return ok;
}
// the vertex as the Levenberg driver sees it: oplusImpl (types_seven_dof_expmap.h:60-69).  x is the solver's array: with _fix_scale its seventh entry is
// zero from here on, which computeScale then reads.
struct VertexSim3 {
    enum { D = 7 };
    Sim3 est;
    int fix_scale;
    PT_HD void oplus(double* x)
    {
        if (fix_scale) x[6] = 0.0;
        Sim3 e, r;
        sim3_exp(x, &e);
        sim3_mul(e, est, &r);
        est = r;
    }
    PT_HD bool finite() const { return sim3_finite(est); }
};
// perturbed estimate k of a linearisation (base_binary_edge.hpp:181-194): d = k / 2, +1e-9 for even k and -1e-9 for odd, through oplus; and its inverse
PT_HD void perturbed(const VertexSim3& v, int k, Sim3* fwd, Sim3* inv)
{
    const double delta = 1e-9;
    double add[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    add[k >> 1] = (k & 1) ? -delta : delta;
    VertexSim3 p = v;
    p.oplus(add);
    *fwd = p.est;
    sim3_inverse(p.est, inv);
}
// Converter::toCvMat(Sim3) (src/Converter.cc:57-63) of gScm * Sim3(R2w, t2w, 1.0) (src/LoopClosing.cc:339-341): s * R, t, rounded to float
PT_HD void sim3_scw(const Sim3& S12, const float* T2w, float* Scw)
{
    double M[16], R[9];
    for (int i = 0; i < 16; ++i) M[i] = (double)T2w[i];
    Sim3 w, r;
    quat_of_rotation(M, 4, w.q);
    w.t[0] = M[3]; w.t[1] = M[7]; w.t[2] = M[11];
    w.s = 1.0;
    sim3_mul(S12, w, &r);
    quat_to_mat3(r.q, R);
    for (int i = 0; i < 16; ++i) Scw[i] = (i == 15) ? 1.f : 0.f;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Scw[i * 4 + j] = (float)(r.s * R[i * 3 + j]); Scw[i * 4 + 3] = (float)r.t[i]; }
}

// ---- one edge ------------------------------------------------------------------------------------------------------------------------------------------
// computeError of either edge (types_seven_dof_expmap.h:138-145, :160-167): obs - cam_map(project(S.map(X))), S the estimate (e12, X = P2c) or its
// inverse (e21, X = P1c).  false: the depth is exactly 0, nothing is written.
PT_HD bool edge_error(const Cam& c, const Sim3& S, const double* X, const double* obs, double* e)
{
    double P[3];
    sim3_map(S, X, P);
    if (P[2] == 0.0) return false;
    e[0] = obs[0] - ((P[0] / P[2]) * c.fx + c.cx);
    e[1] = obs[1] - ((P[1] / P[2]) * c.fy + c.cy);
    return true;
}
// chi2 (base_edge.h:58-61)
PT_HD double edge_chi2(const double* e, double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }
// what activeRobustChi2 adds for an edge
PT_HD double edge_robust_chi2(const double* e, double w, double delta)
{
    double r0, r1;
    huber(edge_chi2(e, w), delta, &r0, &r1);
    return r0;
}
// linearizeOplus (base_binary_edge.hpp:176-200): column d = (1 / (2 * 1e-9)) * (error at perturbed 2 d - error at perturbed 2 d + 1).  P: the 14 perturbed
// estimates (e12) or their inverses (e21).  false: a depth of 0.
PT_HD bool edge_numeric_jacobian(const Cam& c, const Sim3* P, const double* X, const double* obs, double (*J)[7])
{
    const double delta = 1e-9;
    const double scalar = 1.0 / (2 * delta);
    for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        if (!edge_error(c, P[2 * d], X, obs, ep)) return false;
        if (!edge_error(c, P[2 * d + 1], X, obs, em)) return false;
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
    return true;
}
// constructQuadraticForm, the robust branch with `from` fixed (base_binary_edge.hpp:91-113), with the edge's CURRENT _error e, added into S[35]
PT_HD void edge_quadratic_form(const double (*J)[7], const double* e, double w, double delta, double* S)
{
    double r0, r1;
    huber(edge_chi2(e, w), delta, &r0, &r1);
    const double ww = r1 * w;                                       // robustInformation: rho[1] * _information
    const double n0 = (w * e[0]) * r1, n1 = (w * e[1]) * r1;        // -omega_r
    int k = 0;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j <= i; ++j) {                              // (B^T * weightedOmega) * B at (i, j)
            S[k] = S[k] + ((J[0][i] * ww) * J[0][j] + (J[1][i] * ww) * J[1][j]);
            ++k;
        }
    for (int i = 0; i < 7; ++i) S[N_H + i] = S[N_H + i] + (J[0][i] * n0 + J[1][i] * n1);
}
// both edges of correspondence i, e12 first: what errors() and system() of an Ops do per correspondence.  e [4]: e12's _error, e21's.
PT_HD bool corr_errors(const Cam& c, const Sim3& est, const Sim3& inv, const double* P1, const double* P2, const double* obs1, const double* obs2, double* e)
{
    double t[4];
    if (!edge_error(c, est, P2, obs1, t)) return false;
    if (!edge_error(c, inv, P1, obs2, t + 2)) return false;
    for (int i = 0; i < 4; ++i) e[i] = t[i];
    return true;
}
PT_HD bool corr_quadratic_form(const Cam& c, const Sim3* pert, const double* P1, const double* P2, const double* obs1, const double* obs2, const double* e,
                               double w1, double w2, double delta, double* S)
{
    double J[2][7];
    if (!edge_numeric_jacobian(c, pert, P2, obs1, J)) return false;
    edge_quadratic_form(J, e, w1, delta, S);
    if (!edge_numeric_jacobian(c, pert + 14, P1, obs2, J)) return false;
    edge_quadratic_form(J, e + 2, w2, delta, S);
    return true;
}

// ---- the driver, src/Optimizer.cc:2147-2207 ----------------------------------------------------------------------------------------------------------------
// Ops:  int  n_edges()                        nCorrespondences
//       int  n_active()                       correspondences whose edges are still in the graph
//       bool errors(const VertexSim3&, bool, double* chi), bool system(const VertexSim3&, bool, double* S)      as lm_optimize asks (S[35])
//       int  check(double th2)                :2153-2170 / :2187-2201 for every correspondence still in the graph, with the _error the last errors() left:
//                                             chi2 of either edge above th2 removes both and nulls the match; returns how many
struct Result {
    Sim3 S12;
    int n_inliers, n_correspondences, n_bad_first, iters[2], status;
};
template <class Ops>
PT_HD void run_pair(Ops& ops, const Sim3& S12, int fix_scale, double th2, Result* o)
{
    o->S12 = S12;
    o->n_inliers = 0; o->n_bad_first = 0; o->iters[0] = 0; o->iters[1] = 0; o->status = 0;
    o->n_correspondences = ops.n_edges();
    VertexSim3 v;
    v.est = S12; v.fix_scale = fix_scale;
    if (!v.finite()) { o->status |= ST_NOT_FINITE; return; }
    if (ops.n_active() > 0) {                                       // :2148-2149
        const int n = lm_optimize(ops, v, 5, true, &o->status);
        if (n == LM_STOP) return;
        o->iters[0] = n;
    }
    const int n_bad = ops.check(th2);                               // :2152-2170
    o->n_bad_first = n_bad;
    const int more = n_bad > 0 ? 10 : 5;
    if (o->n_correspondences - n_bad < 10) return;                  // :2178-2179: g2oS12 is not written
    const int n = lm_optimize(ops, v, more, true, &o->status);      // :2183-2184: from the current estimate, lambda anew
    if (n == LM_STOP) return;
    o->iters[1] = n;
    o->n_inliers = (o->n_correspondences - n_bad) - ops.check(th2); // :2186-2201
    o->S12 = v.est;                                                 // :2204-2205
}

}  // namespace optsim3
}  // namespace olf
