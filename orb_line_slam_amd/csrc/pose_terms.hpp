// pose_terms.hpp -- Optimizer::PoseOptimizationWithLine (src/Optimizer.cc:604-697, the branch that executes) stated once for the host form
// (pose_host.cpp) and the batched kernel (pose_batch.hip): the per-feature terms, the small dense pieces and the driver of the four passes.  Plain C++
// over doubles, no Eigen; built with -ffp-contract=off on both sides, so for the same DT a feature's J, r and w are the same bits on the host and on the
// device.  What differs between the two is only who sums: the driver is a template over `Ops`, which owns the features of one frame and delivers the 28
// sums, the robust scales and the outlier update (a serial loop in pose_host.cpp, a workgroup in pose_batch.hip, where every lane runs the driver on the
// same values and so takes the same branches).
//
// Conventions where the reference's build decides: sqrt(mvInvLevelSigma2[octave]) is the C function on the widened float (C.6, conv_libm_float = 0);
// vector / scalar divides every coefficient (Eigen 3.2+, conv_eigen_recip = 0); an Eigen product sums over k in ascending order.
// The 4 x 4, 3 x 3 and quaternion pieces and the PT_HD marker are dense_math.hpp; what is here belongs to this optimiser alone.
#pragma once
#include <string.h>
#include "dense_math.hpp"

namespace olf {
namespace pose {

using namespace dense;

enum { ST_NO_FEATURE = 1, ST_NOT_FINITE = 2, ST_OCTAVE = 4 };      // the frame's own status word
enum { N_SUMS = 28 };                                              // 21 of H's upper triangle (row by row), 6 of g, 1 of e

struct Cfg {
    int max_iters;
    double homog_th, min_error, min_error_change, inlier_k;
    int use_motion_model, has_points, has_lines;
    double fx, fy, cx, cy;
};

struct Result {
    float Tcw[16];
    double DT[16], cov[36], eig[6], err;
    int good, status, iters[4];
};

// the ordered 64-bit pattern of a residual (>= 0 or NaN): its order is the order of the values, every NaN is one pattern above the infinities
PT_HD uint64_t key_of(double r)
{
    if (r != r) return 0x7ff8000000000000ull;
    uint64_t u;
    __builtin_memcpy(&u, &r, 8);
    return u & 0x7fffffffffffffffull;
}
PT_HD double value_of(uint64_t k) { double r; __builtin_memcpy(&r, &k, 8); return r; }
// residues[i] = fabsf(residues[i] - median), src/Auxiliar.cc:413: the deviation rounded to float
PT_HD double mad_dev(double r, double median) { return (double)fabsf((float)(r - median)); }

// ---- se(3) ---------------------------------------------------------------------------------------------------------------------------------------------
// expmap_se3, src/Auxiliar.cc:124-144: x = (t, w)
PT_HD void expmap_se3(const double* x, double* T)
{
    const double w[3] = {x[3], x[4], x[5]};
    double t[3] = {x[0], x[1], x[2]}, R[9], Om[9], OO[9];
    const double theta = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    skew3(w, Om);
    if (theta < 0.00001) {
        mat3_mul(Om, Om, OO);
        for (int i = 0; i < 9; ++i) R[i] = (((i % 4 == 0) ? 1.0 : 0.0) + Om[i]) + OO[i];
        mat3_vec(R, t, t);
    } else {
        double s[9], ss[9], V[9];
        for (int i = 0; i < 9; ++i) s[i] = Om[i] / theta;
        mat3_mul(s, s, ss);
        const double sn = sin(theta), c1 = 1.0 - cos(theta), ts = theta - sn;
        for (int i = 0; i < 9; ++i) {
            const double I = (i % 4 == 0) ? 1.0 : 0.0;
            R[i] = (I + s[i] * sn) + ss[i] * c1;
            V[i] = (I + (s[i] * c1) / theta) + (ss[i] * ts) / theta;
        }
        mat3_vec(V, t, t);
    }
    mat4_identity(T);
    for (int i = 0; i < 3; ++i) { T[i * 4] = R[i * 3]; T[i * 4 + 1] = R[i * 3 + 1]; T[i * 4 + 2] = R[i * 3 + 2]; T[i * 4 + 3] = t[i]; }
}
// logmap_se3 (src/Auxiliar.cc:146-152): g2o::SE3Quat(R, t).log() with the halves swapped, so x = (upsilon, omega).  The constructor goes through a
// normalised quaternion with w >= 0 (se3quat.h:58-60, :280-285) and log() through its rotation matrix again (:178-215).
PT_HD void logmap_se3(const double* T, double* x)
{
    double q[4], R[9];                                              // x, y, z, w
    quat_from_mat4(T, q);
    quat_to_mat3(q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    double om[3], Om[9], OO[9], Vi[9];
    if (d > 0.99999) {
        for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
        skew3(om, Om);
        mat3_mul(Om, Om, OO);
        for (int i = 0; i < 9; ++i) Vi[i] = (((i % 4 == 0) ? 1.0 : 0.0) - 0.5 * Om[i]) + (1. / 12.) * OO[i];
    } else {
        const double theta = acos(d), f = theta / (2.0 * sqrt(1.0 - d * d));
        for (int i = 0; i < 3; ++i) om[i] = f * dR[i];
        skew3(om, Om);
        mat3_mul(Om, Om, OO);
        const double c = (1.0 - theta / (2.0 * tan(theta / 2.0))) / (theta * theta);
        for (int i = 0; i < 9; ++i) Vi[i] = (((i % 4 == 0) ? 1.0 : 0.0) - 0.5 * Om[i]) + c * OO[i];
    }
    const double t[3] = {T[3], T[7], T[11]};
    mat3_vec(Vi, t, x);
    x[3] = om[0]; x[4] = om[1]; x[5] = om[2];
}

// ---- 6 x 6, row-major ------------------------------------------------------------------------------------------------------------------------------
// x = H^-1 g by Householder QR with column pivoting, as Eigen's ColPivHouseholderQR<Matrix6d>(H).solve(g): the pivot is the column of the largest
// remaining norm, a column counts as zero below (epsilon * largest column norm)^2 * (6 - k) / 6, and the solution uses the pivots before the first such
// column.  *log_abs_det = sum log |R_kk| (logAbsDeterminant()).
PT_HD void solve6_qr(const double* H, const double* g, double* x, double* log_abs_det)
{
    double A[36], b[6];
    int perm[6];
    for (int i = 0; i < 36; ++i) A[i] = H[i];
    for (int i = 0; i < 6; ++i) { b[i] = g[i]; perm[i] = i; }
    double maxn = 0.0;
    for (int j = 0; j < 6; ++j) {
        double s = 0.0;
        for (int i = 0; i < 6; ++i) s = s + A[i * 6 + j] * A[i * 6 + j];
        maxn = max_d(maxn, s);
    }
    const double eps = 2.220446049250313e-16, th = (maxn * eps) * eps / 6.0;
    int rank = 6;
    double lad = 0.0;
    for (int k = 0; k < 6; ++k) {
        int p = k;
        double big = -1.0;
        for (int j = k; j < 6; ++j) {
            double s = 0.0;
            for (int i = k; i < 6; ++i) s = s + A[i * 6 + j] * A[i * 6 + j];
            if (s > big) { big = s; p = j; }
        }
        if (rank == 6 && big < th * (double)(6 - k)) rank = k;
        if (p != k) {
            for (int i = 0; i < 6; ++i) { const double t = A[i * 6 + k]; A[i * 6 + k] = A[i * 6 + p]; A[i * 6 + p] = t; }
            const int t = perm[k]; perm[k] = perm[p]; perm[p] = t;
        }
        double tail = 0.0;
        for (int i = k + 1; i < 6; ++i) tail = tail + A[i * 6 + k] * A[i * 6 + k];
        const double c0 = A[k * 6 + k];
        double beta = c0, tau = 0.0, v[6];
        if (tail > 2.2250738585072014e-308) {
            beta = sqrt(c0 * c0 + tail);
            if (c0 >= 0.0) beta = -beta;
            for (int i = k + 1; i < 6; ++i) v[i] = A[i * 6 + k] / (c0 - beta);
            tau = (beta - c0) / beta;
        } else {
            for (int i = k + 1; i < 6; ++i) v[i] = 0.0;
        }
        A[k * 6 + k] = beta;
        for (int i = k + 1; i < 6; ++i) A[i * 6 + k] = 0.0;
        for (int j = k + 1; j < 6; ++j) {
            double s = A[k * 6 + j];
            for (int i = k + 1; i < 6; ++i) s = s + v[i] * A[i * 6 + j];
            s = s * tau;
            A[k * 6 + j] = A[k * 6 + j] - s;
            for (int i = k + 1; i < 6; ++i) A[i * 6 + j] = A[i * 6 + j] - s * v[i];
        }
        {
            double s = b[k];
            for (int i = k + 1; i < 6; ++i) s = s + v[i] * b[i];
            s = s * tau;
            b[k] = b[k] - s;
            for (int i = k + 1; i < 6; ++i) b[i] = b[i] - s * v[i];
        }
        lad = lad + log(fabs(beta));
    }
    double y[6];
    for (int i = 0; i < 6; ++i) y[i] = 0.0;
    for (int i = rank - 1; i >= 0; --i) {
        double s = b[i];
        for (int j = i + 1; j < rank; ++j) s = s - A[i * 6 + j] * y[j];
        y[i] = s / A[i * 6 + i];
    }
    for (int i = 0; i < 6; ++i) x[perm[i]] = y[i];
    *log_abs_det = lad;
}
// H.inverse(): LU with partial pivoting (Eigen's PartialPivLU for a 6 x 6), column by column of the identity
PT_HD void inverse6(const double* H, double* Hi)
{
    double A[36];
    int piv[6];
    for (int i = 0; i < 36; ++i) A[i] = H[i];
    for (int k = 0; k < 6; ++k) {
        int p = k;
        double big = fabs(A[k * 6 + k]);
        for (int i = k + 1; i < 6; ++i) if (fabs(A[i * 6 + k]) > big) { big = fabs(A[i * 6 + k]); p = i; }
        piv[k] = p;
        if (p != k) for (int j = 0; j < 6; ++j) { const double t = A[k * 6 + j]; A[k * 6 + j] = A[p * 6 + j]; A[p * 6 + j] = t; }
        for (int i = k + 1; i < 6; ++i) {
            const double f = A[i * 6 + k] / A[k * 6 + k];
            A[i * 6 + k] = f;
            for (int j = k + 1; j < 6; ++j) A[i * 6 + j] = A[i * 6 + j] - f * A[k * 6 + j];
        }
    }
    for (int c = 0; c < 6; ++c) {
        double y[6];
        for (int i = 0; i < 6; ++i) y[i] = (i == c) ? 1.0 : 0.0;
        for (int k = 0; k < 6; ++k) if (piv[k] != k) { const double t = y[k]; y[k] = y[piv[k]]; y[piv[k]] = t; }
        for (int i = 1; i < 6; ++i) { double s = y[i]; for (int j = 0; j < i; ++j) s = s - A[i * 6 + j] * y[j]; y[i] = s; }
        for (int i = 5; i >= 0; --i) { double s = y[i]; for (int j = i + 1; j < 6; ++j) s = s - A[i * 6 + j] * y[j]; y[i] = s / A[i * 6 + i]; }
        for (int i = 0; i < 6; ++i) Hi[i * 6 + c] = y[i];
    }
}
// eigenvalues of the symmetric matrix the lower triangle of M states (what SelfAdjointEigenSolver reads), ascending: cyclic Jacobi
PT_HD void eig6_sym(const double* M, double* w)
{
    double A[36];
    for (int i = 0; i < 6; ++i) for (int j = 0; j <= i; ++j) { A[i * 6 + j] = M[i * 6 + j]; A[j * 6 + i] = M[i * 6 + j]; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 6; ++i) { diag = diag + A[i * 7] * A[i * 7]; for (int j = i + 1; j < 6; ++j) off = off + A[i * 6 + j] * A[i * 6 + j]; }
        if (!(off > 1e-40 * diag)) break;                            // (a NaN ends the loop too)
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                const double apq = A[p * 6 + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * 7] - A[p * 7]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 6; ++k) {
                    const double akp = A[k * 6 + p], akq = A[k * 6 + q];
                    A[k * 6 + p] = c * akp - s * akq; A[k * 6 + q] = s * akp + c * akq;
                }
                for (int k = 0; k < 6; ++k) {
                    const double apk = A[p * 6 + k], aqk = A[q * 6 + k];
                    A[p * 6 + k] = c * apk - s * aqk; A[q * 6 + k] = s * apk + c * aqk;
                }
            }
    }
    for (int i = 0; i < 6; ++i) w[i] = A[i * 7];
    for (int i = 1; i < 6; ++i) { const double v = w[i]; int j = i - 1; while (j >= 0 && w[j] > v) { w[j + 1] = w[j]; --j; } w[j + 1] = v; }
}

// ---- per-feature terms ------------------------------------------------------------------------------------------------------------------------------
// Rlw * Xw + tlw, src/Optimizer.cc:642, :654-655 (and DR * P + Dt of every evaluation)
PT_HD void transform3(const double* T, const double* P, double* o)
{
    for (int i = 0; i < 3; ++i) o[i] = ((T[i * 4] * P[0] + T[i * 4 + 1] * P[1]) + T[i * 4 + 2] * P[2]) + T[i * 4 + 3];
}
// Frame::projection, src/Frame.cc:1099-1106
PT_HD void project(const Cfg& c, const double* P, double* uv)
{
    uv[0] = c.cx + c.fx * P[0] / P[2];
    uv[1] = c.cy + c.fy * P[1] / P[2];
}
PT_HD double cauchy(double r) { return 1.0 / (1.0 + r * r); }                       // robustWeightCauchy, src/Auxiliar.cc:568
// the six-entry row of :982-988 / :1041-1047 for a camera-frame point g and the pair (a, b) = (dx, dy) or (lx, ly)
PT_HD void jac_row(const Cfg& c, const double* g, double a, double b, double* J)
{
    const double gx = g[0], gy = g[1], gz = g[2];
    const double gz2 = gz * gz;
    const double fgz2 = c.fx / max_d(c.homog_th, gz2);
    J[0] = +fgz2 * a * gz;
    J[1] = +fgz2 * b * gz;
    J[2] = -fgz2 * (gx * a + gy * b);
    J[3] = -fgz2 * (gx * gy * a + gy * gy * b + gz * gz * b);
    J[4] = +fgz2 * (gx * gx * a + gz * gz * a + gx * gy * b);
    J[5] = +fgz2 * (gx * gz * b - gy * gz * a);
}
// the point's projection error norm under DT (what removeOutliers and the robust pre-pass take) and, with J, its Jacobian row (:962-989)
PT_HD double point_term(const Cfg& c, const double* DT, const double* Pprev, double ox, double oy, double* J)
{
    double P[3], uv[2];
    transform3(DT, Pprev, P);
    project(c, P, uv);
    const double dx = uv[0] - ox, dy = uv[1] - oy;
    const double n = sqrt(dx * dx + dy * dy);
    if (J) {
        jac_row(c, P, dx, dy, J);
        const double d = max_d(c.homog_th, n);
        for (int i = 0; i < 6; ++i) J[i] = J[i] / d;
    }
    return n;
}
// Frame::lineSegmentOverlap, src/Frame.cc:1108-1209
PT_HD double overlap_ladder(double ls, double le)
{
    const double lmin = min_d(ls, le), lmax = max_d(ls, le);
    if (lmin < 0.0 && lmax > 1.0) return 1.0;
    if (lmax < 0.0 || lmin > 1.0) return 0.0;
    if (lmin < 0.0) return lmax;
    if (lmax > 1.0) return 1.0 - lmin;
    return lmax - lmin;
}
PT_HD double line_segment_overlap(const double* so, const double* eo, const double* sp, const double* ep, int* branch)
{
    if (fabs(so[0] - eo[0]) < 1.0) {                                // vertical
        if (branch) *branch = 0;
        const double l1 = eo[1] - so[1];
        return overlap_ladder((sp[1] - so[1]) / l1, (ep[1] - so[1]) / l1);
    }
    if (fabs(so[1] - eo[1]) < 1.0) {                                // horizontal
        if (branch) *branch = 1;
        const double l0 = eo[0] - so[0];
        return overlap_ladder((sp[0] - so[0]) / l0, (ep[0] - so[0]) / l0);
    }
    if (branch) *branch = 2;
    const double l0 = eo[0] - so[0];
    const double a = so[1] - eo[1], b = eo[0] - so[0], c = so[0] * eo[1] - eo[0] * so[1];
    const double lxy = 1.0 / (a * a + b * b);
    const double sx = (b * (b * sp[0] - a * sp[1]) - a * c) * lxy;
    const double ex = (b * (b * ep[0] - a * ep[1]) - a * c) * lxy;
    return overlap_ladder((sx - so[0]) / l0, (ex - so[0]) / l0);
}
// a line's error norm under DT and, with J, its Jacobian row and overlap (:1016-1077); Lprev = start, end; le = mvle_l[i]; obs = the key line's end points
PT_HD double line_term(const Cfg& c, const double* DT, const double* Lprev, const double* le, const double* obs, double* J, double* overlap)
{
    double sP[3], eP[3], sp[2], ep[2];
    transform3(DT, Lprev, sP);
    transform3(DT, Lprev + 3, eP);
    project(c, sP, sp);
    project(c, eP, ep);
    const double ds = le[0] * sp[0] + le[1] * sp[1] + le[2];
    const double de = le[0] * ep[0] + le[1] * ep[1] + le[2];
    const double n = sqrt(ds * ds + de * de);
    if (J) {
        double Js[6], Je[6];
        jac_row(c, sP, le[0], le[1], Js);
        jac_row(c, eP, le[0], le[1], Je);
        const double d = max_d(c.homog_th, n);
        for (int i = 0; i < 6; ++i) J[i] = (Js[i] * ds + Je[i] * de) / d;
        *overlap = line_segment_overlap(obs, obs + 2, sp, ep, nullptr);
    }
    return n;
}
// H += J J^T w, g += J r w, e += r r w (:1001-1003) into S: H's upper triangle row by row, g, e
PT_HD void add_term(double* S, const double* J, double r, double w)
{
    int k = 0;
    for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) { S[k] = S[k] + J[i] * J[j] * w; ++k; }
    for (int i = 0; i < 6; ++i) S[21 + i] = S[21 + i] + J[i] * r * w;
    S[27] = S[27] + r * r * w;
}
// one point's / line's contribution to the sums of optimizeFunctions (robust = 0, sq = sqrt(mvInvLevelSigma2[octave])) or optimizeFunctionsRobust
// (robust = 1, s = s_p / s_l)
PT_HD void accumulate_point(const Cfg& c, const double* DT, const double* Pprev, double ox, double oy, int robust, double sq, double s, double* S)
{
    double J[6];
    const double n = point_term(c, DT, Pprev, ox, oy, J);
    const double r = robust ? n : n * sq;
    const double w = cauchy(robust ? r / s : r);
    add_term(S, J, r, w);
}
PT_HD void accumulate_line(const Cfg& c, const double* DT, const double* Lprev, const double* le, const double* obs, int robust, double sq, double s, double* S)
{
    double J[6], ov;
    const double n = line_term(c, DT, Lprev, le, obs, J, &ov);
    const double r = robust ? n : n * sq;
    double w = cauchy(robust ? r / s : r);
    w = w * ov;
    add_term(S, J, r, w);
}
// the scale of the residuals of optimizeFunctionsRobust from a MAD (:1171-1208)
PT_HD double clamp_scale(double s) { const double lo = 0.0001, hi = sqrt(7.815); if (s < lo) s = lo; if (s > hi) s = hi; return s; }
// the mean of vector_mean_stdv_mad (src/Auxiliar.cc:417-439) from its two sums; n > 0
PT_HD double mad_mean(double sum_below, int k, double sum_all, int n) { return k >= (int)(0.2 * (double)n) ? sum_below / (double)k : sum_all / (double)n; }
// removeOutliers' decision for one residual (:517-529)
PT_HD bool is_outlier(double res, double mean, double th) { return fabs(res - mean) > th; }

// ---- the four passes and the epilogue ----------------------------------------------------------------------------------------------------------------
// Ops:  void prepare(const double* Tlw)                       previous-frame positions of every held feature
//       void sums(const double* DT, int robust, double s_p, double s_l, double* S, int* n)   S[N_SUMS] over the active features (H_p + H_l in one), their number
//       void robust_scales(const double* DT, double* s_p, double* s_l)                        1.4826 * MAD of the active features' error norms, 0 without any
//       void remove_outliers(const double* DT)
template <class Ops>
PT_HD bool evaluate(Ops& ops, const double* DT, int robust, double* H, double* g, double* err, int* status, bool first)
{
    double S[N_SUMS], sp = 1.0, sl = 1.0;
    int n = 0;
    if (robust) { ops.robust_scales(DT, &sp, &sl); sp = clamp_scale(sp); sl = clamp_scale(sl); }
    ops.sums(DT, robust, sp, sl, S, &n);
    if (first && n == 0) { *status |= ST_NO_FEATURE; return false; }
    bool ok = true;
    for (int i = 0; i < N_SUMS; ++i) ok = ok && finite_d(S[i]);
    if (!ok) { *status |= ST_NOT_FINITE; return false; }
    int k = 0;
    for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) { H[i * 6 + j] = S[k]; H[j * 6 + i] = S[k]; ++k; }
    for (int i = 0; i < 6; ++i) g[i] = S[21 + i];
    *err = S[27] / (double)n;
    return true;
}
PT_HD bool step(const double* inc, double* DT, int* status)
{
    double E[16], Ei[16];
    expmap_se3(inc, E);
    inverse_se3(E, Ei);
    mat4_mul(DT, Ei, DT);
    if (!mat4_finite(DT)) { *status |= ST_NOT_FINITE; return false; }
    return true;
}
// gaussNewtonOptimization (:779-816); false: the frame stops (status says why)
template <class Ops>
PT_HD bool gauss_newton(Ops& ops, const Cfg& c, double* DT, double* cov, double* err_out, int* iters_out, int* status)
{
    double H[36], g[6], inc[6], err = 0.0, err_prev = 999999999.9, lad;
    int iters;
    for (iters = 0; iters < c.max_iters; iters++) {
        if (!evaluate(ops, DT, 0, H, g, &err, status, iters == 0)) return false;
        ++*iters_out;
        if (err > err_prev) {
            if (iters > 0) break;
            *err_out = -1.0;
            return true;
        }
        if (err < c.min_error || fabs(err - err_prev) < c.min_error_change) break;
        solve6_qr(H, g, inc, &lad);
        if (!step(inc, DT, status)) return false;
        if (sqrt((inc[0] * inc[0] + inc[1] * inc[1]) + inc[2] * inc[2]) < c.min_error_change &&
            sqrt((inc[3] * inc[3] + inc[4] * inc[4]) + inc[5] * inc[5]) < c.min_error_change)
            break;
        err_prev = err;
    }
    inverse6(H, cov);
    *err_out = err;
    return true;
}
// gaussNewtonOptimizationRobust (:818-865)
template <class Ops>
PT_HD bool gauss_newton_robust(Ops& ops, const Cfg& c, double* DT, double* cov, double* err_out, int* iters_out, int* status)
{
    double H[36], g[6], inc[6], DT0[16], err = 0.0, err_prev = 999999999.9, lad;
    bool good = true;
    for (int i = 0; i < 16; ++i) DT0[i] = DT[i];
    for (int iters = 0; iters < c.max_iters; iters++) {
        if (!evaluate(ops, DT, 1, H, g, &err, status, iters == 0)) return false;
        ++*iters_out;
        if (fabs(err - err_prev) < c.min_error_change || err < c.min_error) break;
        solve6_qr(H, g, inc, &lad);
        if (lad < 0.0) { good = false; break; }
        if (!step(inc, DT, status)) return false;
        double n2 = 0.0;
        for (int i = 0; i < 6; ++i) n2 = n2 + inc[i] * inc[i];
        if (sqrt(n2) < c.min_error_change) break;
        err_prev = err;
    }
    if (good) {
        inverse6(H, cov);
        *err_out = err;
    } else {
        for (int i = 0; i < 16; ++i) DT[i] = DT0[i];
        *err_out = -1.0;
        for (int i = 0; i < 36; ++i) cov[i] = (i % 7 == 0) ? 1.0 : 0.0;
    }
    return true;
}
// Tcw, Tcw_prev: row-major float 4 x 4 (Tcw_prev never NULL here: the caller passes Tcw for an empty one, :613-614); cov_in [36] or NULL for zeros
template <class Ops>
PT_HD void run_frame(Ops& ops, const Cfg& c, const float* Tcw, const float* Tcw_prev, const double* cov_in, Result* o)
{
    double T[16], Tp[16], Tpi[16], DT0[16], DT[16], cov[36], err = -1.0;
    for (int i = 0; i < 16; ++i) { T[i] = (double)Tcw[i]; Tp[i] = (double)Tcw_prev[i]; }
    for (int i = 12; i < 16; ++i) { T[i] = (i == 15) ? 1.0 : 0.0; Tp[i] = T[i]; }       // Converter::toMatrix4d writes the last row itself
    inverse_se3(Tp, Tpi);
    if (c.use_motion_model) mat4_mul(T, Tpi, DT0); else mat4_identity(DT0);
    for (int i = 0; i < 36; ++i) cov[i] = cov_in ? cov_in[i] : 0.0;
    ops.prepare(Tp);
    o->status = 0; o->good = 0;
    for (int p = 0; p < 4; ++p) o->iters[p] = 0;
    bool alive = mat4_finite(DT0);
    if (!alive) o->status |= ST_NOT_FINITE;
    for (int p = 0; p < 4 && alive; ++p) {                           // :665-679
        for (int i = 0; i < 16; ++i) DT[i] = DT0[i];
        alive = (p == 2) ? gauss_newton_robust(ops, c, DT, cov, &err, &o->iters[p], &o->status) : gauss_newton(ops, c, DT, cov, &err, &o->iters[p], &o->status);
        if (alive) ops.remove_outliers(DT);
    }
    if (!alive) {                                                    // defined here, not by the reference: the pose goes through unchanged
        for (int i = 0; i < 16; ++i) o->Tcw[i] = Tcw[i];
        mat4_identity(o->DT);
        for (int i = 0; i < 36; ++i) o->cov[i] = 0.0;
        for (int i = 0; i < 6; ++i) o->eig[i] = 0.0;
        o->err = -1.0;
        return;
    }
    eig6_sym(cov, o->eig);                                          // isGoodSolution, :453-466 (its value is ignored by the reference)
    o->good = !(o->eig[0] < 0.0 || o->eig[5] > 1.0 || err < 0.0 || err > 1.0 || !mat4_finite(DT));
    double x[6], Ti[16], Twc[16];
    inverse_se3(DT, Ti);                                            // :684
    logmap_se3(Ti, x);
    expmap_se3(x, o->DT);
    mat4_mul(Tpi, o->DT, Twc);                                       // :686-687
    logmap_se3(Twc, x);
    expmap_se3(x, Twc);
    float f[16];                                                    // Converter::toInvCvMat(toCvMat(Twc)): a float matrix, -R^T t summed in double
    for (int i = 0; i < 16; ++i) f[i] = (float)Twc[i];
    for (int i = 0; i < 16; ++i) o->Tcw[i] = (i % 5 == 0) ? 1.f : 0.f;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o->Tcw[i * 4 + j] = f[j * 4 + i];
        const double s = ((double)f[0 * 4 + i] * (double)f[3] + (double)f[1 * 4 + i] * (double)f[7]) + (double)f[2 * 4 + i] * (double)f[11];
        o->Tcw[i * 4 + 3] = (float)(-s);
    }
    for (int i = 0; i < 36; ++i) o->cov[i] = cov[i];
    o->err = err;
}

}  // namespace pose
}  // namespace olf
