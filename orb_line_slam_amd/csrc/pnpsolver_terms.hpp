// pnpsolver_terms.hpp -- the arithmetic of PnPsolver (src/PnPsolver.cc) that the host form (pnpsolver_host.cpp) and the kernel (pnpsolver_batch.hip) both
// run: the parameters of SetRansacParameters as a function of N (:121-157), EPnP's
// compute_pose with everything it calls (:375-950) and the inlier test of one correspondence (:308-339).  One text for both sides; every file that includes
// it is built with -ffp-contract=off (C.4) and the rounded operations are spelled through device_math.hpp.  All of compute_pose is double, as written.
//
// How one text serves a lane that fits four points, a workgroup that fits a thousand, and the host: compute_pose is written against an environment E.
//   e.at(k)            word k of the fit's workspace of PNP_WS doubles (a plain array on the host, lane-interleaved LDS in the kernel): every array
//                      of the reference that is indexed at run time lives there, so a fit holds no indexed array in registers
//   e.n(), e.point()   the correspondences of the fit: the four sampled ones, or the best set's
//   e.sum<K>(off, f)   K sums over the correspondences, f(i, acc) adding correspondence i's terms with acc.add(k, v); the results at workspace off
//   e.single(f)        what one thread does between two sums
// pws, us, alphas and pcs of the reference are not kept: a term recomputes its correspondence's alphas and pcs from the workspace, which gives the same
// bits.  pw0 of estimate_R_and_t (:585-588) is cws[0] of choose_control_points (:378-384): the same sum in the same order, divided by the same n.
// THE ORDER OF A SUM OVER CORRESPONDENCES (the centroid, PW0^t PW0, M^t M, pc0, ABt, the reprojection error) is the environment's:
//   PnpSeqEnv    i = 0 .. n - 1 into one accumulator that starts at +0: the reference's order, right for the four-point fits
//   blocked      (Refine, n up to the capacity) PNP_THREADS partial sums, partial t taking i = t, t + PNP_THREADS, .. ascending from +0; the 64 partials
//                of a wave are added as a balanced tree of neighbours (t + 1, then + 2, .. + 32); the PNP_THREADS / 64 wave sums are added in ascending order
//                to the first.  PnpHostBlockEnv replays it; the kernel produces it with a butterfly per wave (IEEE addition commutes).
// New conventions:
//   C.23  cvSVD / cvSolve(CV_SVD) / cvInvert(CV_SVD) on double matrices follow C.19's OpenCV without LAPACK: JacobiSVDImpl_<double> on the transposed
//         matrix -- cyclic sweeps over the row pairs, at most max(m, 30) of them, a pair skipped at |p| <= 10 DBL_EPSILON sqrt(a b), every operation in
//         double, hypot spelled sqrt(p p + beta beta) as in C.19 -- singular values ordered descending by a selection that takes the first of equal
//         maxima, the rows with them; a row is normalised by 1 / norm where norm > DBL_MIN and multiplied by 0 otherwise.  cvSolve and cvInvert add
//         SVBkSb: singular values at or below 2 DBL_EPSILON times their sum are skipped.  The three constants are restated from OpenCV 3.4's
//         modules/core/src/lapack.cpp and could not be verified where this was written.
//   C.24  OpenCV fills a row whose norm is <= DBL_MIN from a fixed-seed generator and re-orthogonalises it.  That is not restated: where such a row is
//         read as a vector (the PCA of choose_control_points, M^t M, ABt) the hypothesis is DEGENERATE: it counts no inlier, Refine on it fails, and
//         STATUS_PNP_DEGENERATE is set.  Under cvSolve / cvInvert such a row belongs to a skipped singular value and is not read.
//   C.25  qr_solve's `eta == 0` return (:887-891) leaves x as it is, which in the reference's first Gauss-Newton round is uninitialised: x starts at 0.
//   C.26  the loop of iterate (:182) goes on while mnIterations < cap OR nCurrentIterations < n_iterations, so iterations beyond max_iterations exist:
//         iteration j reads draws[j % max_iterations] and writes counts[j % max_iterations].
// The sample of an iteration is ransac_sample<4> and a row value's test s3_is_match, both of ransac_terms.hpp (shared with sim3solver_terms.hpp, of which
// nothing else is needed here: that header is not included).
#pragma once
#include "ransac_terms.hpp"

// OLF_HD on a member function (device_math.hpp's host form is `static inline`, which a member cannot be)
#if defined(__HIPCC__)
#define OLF_HDM __host__ __device__ __forceinline__
#else
#define OLF_HDM inline
#endif

namespace olf {

constexpr int PNP_WORDS = 8;                       // 4-byte words a correspondence keeps: the 3-D point, the 2-D point, mvMaxError, its feature, the best set's list
constexpr int PNP_THREADS = 256, PNP_WAVES = 4;    // the blocked order's shape (the kernel's workgroup)
constexpr int STATUS_PNP_DEGENERATE = 32768;

// the workspace of one fit, in doubles
constexpr int W_AT = 0;                            // 12 x 12: M^t M, then Ut
constexpr int W_SA = 144, W_SV = 174, W_SW = 199;  // the small SVDs: At (at most 5 x 6), V (at most 5 x 5), the singular values (also the 12)
constexpr int W_CWS = 211, W_CI = 223;             // cws[4][3], cc_inv[9]
constexpr int W_L = 232, W_RHO = 292, W_BETAS = 298;   // l_6x10, rho[6], Betas[1..3][4]
constexpr int W_SUM = 232;                         // the 78 sums of M^t M's upper triangle, before l_6x10 exists
constexpr int W_CCS = 310, W_PC0 = 322, W_S9 = 325;    // ccs[4][3], pc0[3], up to nine sums
constexpr int W_R = 334, W_T = 361, W_ERR = 370;   // Rs[1..3][9], ts[1..3][3], rep_errors[1..3]
constexpr int W_GN = 373, W_B = 415;               // gauss_newton's a[24] b[6] x[4] A1[4] A2[4]; the solution of cvSolve (at most 5)
constexpr int W_FLAG = 420, W_CHOICE = 421;        // 1.0: degenerate (C.24); the chosen N - 1
constexpr int PNP_WS = 422;

// ---- SetRansacParameters (:121-157) as a function of N alone, through the host's libm (host only: the kernel reads the table its caller built).
// N < the effective minimum never iterates and gets the cap 1.  A quotient beyond max_iterations, or a NaN, is max_iterations.
inline void pnp_parameters(int N, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, int* min_eff, int* cap)
{
    int nMin = (int)((float)N * epsilon);
    if (nMin < min_inliers) nMin = min_inliers;
    if (nMin < min_set) nMin = min_set;
    *min_eff = nMin;
    int its = 1;
    if (N > nMin) {
        float e = epsilon;
        if (e < (float)nMin / N) e = (float)nMin / N;
        const double v = ceil(log(1 - probability) / log(1 - pow((double)e, 3)));
        its = v < (double)max_iterations ? (v > 0 ? (int)v : 0) : max_iterations;      // (a NaN compares false: max_iterations)
    }
    const int capped = its < max_iterations ? its : max_iterations;
    *cap = capped > 1 ? capped : 1;
}

// mvMaxError[i] = mvSigma2[i] * th2 with mvSigma2 = mvLevelSigma2[octave] = sf * sf, all float (:90, :156)
OLF_HD float pnp_max_error(float sf, float th2) { return f_mul(f_mul(sf, sf), th2); }

// ---- C.23: the singular value decomposition of the N x M matrix At(i, k) = e.at(oA + i * M + k) (the transposed operand), in place.  Afterwards row i
// is the i-th left singular vector of the operand, e.at(oW + i) its singular value, row i of V (e.at(oV + i * N + k), when WANT_V) the right one.
// Returns false when a row's norm is <= DBL_MIN (C.24).
template <int M, int N, bool WANT_V, class E>
OLF_HD bool pnp_jacobi_svd(E& e, int oA, int oV, int oW)
{
    const double eps = 2.220446049250313e-16 * 10, minval = 2.2250738585072014e-308;
    for (int i = 0; i < N; ++i) {
        double sd = 0;
        for (int k = 0; k < M; ++k) { const double t = e.at(oA + i * M + k); sd = d_add(sd, d_mul(t, t)); }
        e.at(oW + i) = sd;
        if (WANT_V) for (int k = 0; k < N; ++k) e.at(oV + i * N + k) = i == k ? 1.0 : 0.0;
    }
    const int max_iter = M > 30 ? M : 30;
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
        for (int i = 0; i < N - 1; ++i)
            for (int j = i + 1; j < N; ++j) {
                double a = e.at(oW + i), p = 0, b = e.at(oW + j);
                for (int k = 0; k < M; ++k) p = d_add(p, d_mul(e.at(oA + i * M + k), e.at(oA + j * M + k)));
                if (fabs(p) <= d_mul(eps, d_sqrt(d_mul(a, b)))) continue;
                p = d_mul(p, 2.0);
                const double beta = d_sub(a, b), gamma = d_sqrt(d_add(d_mul(p, p), d_mul(beta, beta)));
                double c, s;
                if (beta < 0) {
                    const double delta = d_mul(d_sub(gamma, beta), 0.5);
                    s = d_sqrt(d_div(delta, gamma));
                    c = d_div(p, d_mul(d_mul(gamma, s), 2.0));
                } else {
                    c = d_sqrt(d_div(d_add(gamma, beta), d_mul(gamma, 2.0)));
                    s = d_div(p, d_mul(d_mul(gamma, c), 2.0));
                }
                a = 0; b = 0;
                for (int k = 0; k < M; ++k) {
                    const double x = e.at(oA + i * M + k), y = e.at(oA + j * M + k);
                    const double t0 = d_add(d_mul(c, x), d_mul(s, y)), t1 = d_add(d_mul(-s, x), d_mul(c, y));
                    e.at(oA + i * M + k) = t0; e.at(oA + j * M + k) = t1;
                    a = d_add(a, d_mul(t0, t0)); b = d_add(b, d_mul(t1, t1));
                }
                e.at(oW + i) = a; e.at(oW + j) = b;
                changed = true;
                if (WANT_V)
                    for (int k = 0; k < N; ++k) {
                        const double x = e.at(oV + i * N + k), y = e.at(oV + j * N + k);
                        e.at(oV + i * N + k) = d_add(d_mul(c, x), d_mul(s, y));
                        e.at(oV + j * N + k) = d_add(d_mul(-s, x), d_mul(c, y));
                    }
            }
        if (!changed) break;
    }
    for (int i = 0; i < N; ++i) {
        double sd = 0;
        for (int k = 0; k < M; ++k) { const double t = e.at(oA + i * M + k); sd = d_add(sd, d_mul(t, t)); }
        e.at(oW + i) = d_sqrt(sd);
    }
    for (int i = 0; i < N - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < N; ++k) if (e.at(oW + j) < e.at(oW + k)) j = k;
        if (i != j) {
            { const double t = e.at(oW + i); e.at(oW + i) = e.at(oW + j); e.at(oW + j) = t; }
            for (int k = 0; k < M; ++k) { const double t = e.at(oA + i * M + k); e.at(oA + i * M + k) = e.at(oA + j * M + k); e.at(oA + j * M + k) = t; }
            if (WANT_V) for (int k = 0; k < N; ++k) { const double t = e.at(oV + i * N + k); e.at(oV + i * N + k) = e.at(oV + j * N + k); e.at(oV + j * N + k) = t; }
        }
    }
    bool full = true;
    for (int i = 0; i < N; ++i) {
        const double sd = e.at(oW + i);
        if (sd <= minval) full = false;
        const double s = sd > minval ? d_div(1.0, sd) : 0.0;
        for (int k = 0; k < M; ++k) e.at(oA + i * M + k) = d_mul(e.at(oA + i * M + k), s);
    }
    return full;
}

// SVBkSb's threshold over the N singular values at oW
template <int N, class E>
OLF_HD double pnp_sv_threshold(E& e, int oW)
{
    double th = 0;
    for (int i = 0; i < N; ++i) th = d_add(th, e.at(oW + i));
    return d_mul(th, 2.220446049250313e-16 * 2);
}

// cvSolve(L_6xK, Rho, B, CV_SVD) (:681, :712, :746): column c of L_6xK is column (APPROX == 1 ? {0, 1, 3, 6}[c] : c) of l_6x10; the solution at W_B
template <int K, int APPROX, class E>
OLF_HD void pnp_solve_betas(E& e)
{
    for (int c = 0; c < K; ++c) {
        const int col = APPROX == 1 ? (c == 2 ? 3 : c == 3 ? 6 : c) : c;
        for (int r = 0; r < 6; ++r) e.at(W_SA + c * 6 + r) = e.at(W_L + r * 10 + col);
    }
    pnp_jacobi_svd<6, K, true>(e, W_SA, W_SV, W_SW);
    const double threshold = pnp_sv_threshold<K>(e, W_SW);
    for (int j = 0; j < K; ++j) e.at(W_B + j) = 0.0;
    for (int i = 0; i < K; ++i) {
        double wi = e.at(W_SW + i);
        if (fabs(wi) <= threshold) continue;
        wi = d_div(1.0, wi);
        double s = 0;
        for (int j = 0; j < 6; ++j) s = d_add(s, d_mul(e.at(W_SA + i * 6 + j), e.at(W_RHO + j)));
        s = d_mul(s, wi);
        for (int j = 0; j < K; ++j) e.at(W_B + j) = d_add(e.at(W_B + j), d_mul(s, e.at(W_SV + i * K + j)));
    }
}

// gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838) and qr_solve (:860-950), on W_GN; C.25
template <class E>
OLF_HD void pnp_gauss_newton(E& e, double* betas)
{
    const int oa = W_GN, ob = W_GN + 24, ox = W_GN + 30, o1 = W_GN + 34, o2 = W_GN + 38, nr = 6, nc = 4;
    for (int i = 0; i < 4; ++i) e.at(ox + i) = 0.0;
    for (int round = 0; round < 5; ++round) {
        const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
        for (int i = 0; i < 6; ++i) {
            double L[10];
#pragma unroll
            for (int k = 0; k < 10; ++k) L[k] = e.at(W_L + i * 10 + k);
            e.at(oa + i * 4 + 0) = d_add(d_add(d_add(d_mul(d_mul(2.0, L[0]), b0), d_mul(L[1], b1)), d_mul(L[3], b2)), d_mul(L[6], b3));
            e.at(oa + i * 4 + 1) = d_add(d_add(d_add(d_mul(L[1], b0), d_mul(d_mul(2.0, L[2]), b1)), d_mul(L[4], b2)), d_mul(L[7], b3));
            e.at(oa + i * 4 + 2) = d_add(d_add(d_add(d_mul(L[3], b0), d_mul(L[4], b1)), d_mul(d_mul(2.0, L[5]), b2)), d_mul(L[8], b3));
            e.at(oa + i * 4 + 3) = d_add(d_add(d_add(d_mul(L[6], b0), d_mul(L[7], b1)), d_mul(L[8], b2)), d_mul(d_mul(2.0, L[9]), b3));
            double q = d_mul(d_mul(L[0], b0), b0);
            q = d_add(q, d_mul(d_mul(L[1], b0), b1)); q = d_add(q, d_mul(d_mul(L[2], b1), b1)); q = d_add(q, d_mul(d_mul(L[3], b0), b2));
            q = d_add(q, d_mul(d_mul(L[4], b1), b2)); q = d_add(q, d_mul(d_mul(L[5], b2), b2)); q = d_add(q, d_mul(d_mul(L[6], b0), b3));
            q = d_add(q, d_mul(d_mul(L[7], b1), b3)); q = d_add(q, d_mul(d_mul(L[8], b2), b3)); q = d_add(q, d_mul(d_mul(L[9], b3), b3));
            e.at(ob + i) = d_sub(e.at(W_RHO + i), q);
        }
        // qr_solve
        bool singular = false;
        for (int k = 0; k < nc && !singular; ++k) {
            const int kk = oa + k * nc + k;
            double eta = fabs(e.at(kk));
            for (int i = k + 1, at = kk; i < nr; ++i, at += nc) { const double elt = fabs(e.at(at)); if (eta < elt) eta = elt; }      // (:881-885 as written: the pointer trails the row by one)
            if (eta == 0) { e.at(o1 + k) = 0.0; e.at(o2 + k) = 0.0; singular = true; break; }
            double sum = 0;
            const double inv_eta = d_div(1.0, eta);
            for (int i = k, at = kk; i < nr; ++i, at += nc) { const double v = d_mul(e.at(at), inv_eta); e.at(at) = v; sum = d_add(sum, d_mul(v, v)); }
            double sigma = d_sqrt(sum);
            if (e.at(kk) < 0) sigma = -sigma;
            e.at(kk) = d_add(e.at(kk), sigma);
            e.at(o1 + k) = d_mul(sigma, e.at(kk));
            e.at(o2 + k) = d_mul(-eta, sigma);
            for (int j = k + 1; j < nc; ++j) {
                double s2 = 0;
                for (int i = k, at = kk; i < nr; ++i, at += nc) s2 = d_add(s2, d_mul(e.at(at), e.at(at + j - k)));
                const double tau = d_div(s2, e.at(o1 + k));
                for (int i = k, at = kk; i < nr; ++i, at += nc) e.at(at + j - k) = d_sub(e.at(at + j - k), d_mul(tau, e.at(at)));
            }
        }
        if (!singular) {
            for (int j = 0; j < nc; ++j) {
                const int jj = oa + j * nc + j;
                double tau = 0;
                for (int i = j, at = jj; i < nr; ++i, at += nc) tau = d_add(tau, d_mul(e.at(at), e.at(ob + i)));
                tau = d_div(tau, e.at(o1 + j));
                for (int i = j, at = jj; i < nr; ++i, at += nc) e.at(ob + i) = d_sub(e.at(ob + i), d_mul(tau, e.at(at)));
            }
            e.at(ox + nc - 1) = d_div(e.at(ob + nc - 1), e.at(o2 + nc - 1));
            for (int i = nc - 2; i >= 0; --i) {
                double sum = 0;
                for (int j = i + 1; j < nc; ++j) sum = d_add(sum, d_mul(e.at(oa + i * nc + j), e.at(ox + j)));
                e.at(ox + i) = d_div(d_sub(e.at(ob + i), sum), e.at(o2 + i));
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) betas[i] = d_add(betas[i], e.at(ox + i));
    }
}

OLF_HD double pnp_dot3(const double* a, const double* b) { return d_add(d_add(d_mul(a[0], b[0]), d_mul(a[1], b[1])), d_mul(a[2], b[2])); }

// alphas of one correspondence (:423-433) from cws[0] and cc_inv
template <class E>
OLF_HD void pnp_alphas(E& e, const double* X, double* a)
{
    const double d0 = d_sub(X[0], e.at(W_CWS)), d1 = d_sub(X[1], e.at(W_CWS + 1)), d2 = d_sub(X[2], e.at(W_CWS + 2));
#pragma unroll
    for (int j = 0; j < 3; ++j)
        a[1 + j] = d_add(d_add(d_mul(e.at(W_CI + 3 * j), d0), d_mul(e.at(W_CI + 3 * j + 1), d1)), d_mul(e.at(W_CI + 3 * j + 2), d2));
    a[0] = d_sub(d_sub(d_sub(1.0, a[1]), a[2]), a[3]);
}
// pcs of one correspondence (:468-474)
template <class E>
OLF_HD void pnp_pc(E& e, const double* a, double* pc)
{
#pragma unroll
    for (int j = 0; j < 3; ++j)
        pc[j] = d_add(d_add(d_add(d_mul(a[0], e.at(W_CCS + j)), d_mul(a[1], e.at(W_CCS + 3 + j))), d_mul(a[2], e.at(W_CCS + 6 + j))), d_mul(a[3], e.at(W_CCS + 9 + j)));
}

// compute_pose (:477-525).  cam = fu, fv, uc, vc.  Leaves Rs, ts and rep_errors of the three variants, the chosen one at W_CHOICE and C.24's flag at W_FLAG.
template <class E>
OLF_HD void pnp_compute_pose(E& e, const double* cam)
{
    const double dn = (double)e.n();
    const double fu = cam[0], fv = cam[1], uc = cam[2], vc = cam[3];
    // choose_control_points (:375-409)
    e.template sum<3>(W_S9, [&](int i, auto& acc) {
        double X[3], u[2];
        e.point(i, X, u);
        acc.add(0, X[0]); acc.add(1, X[1]); acc.add(2, X[2]);
    });
    e.single([&]() {
        e.at(W_FLAG) = 0.0;
        for (int j = 0; j < 3; ++j) e.at(W_CWS + j) = d_div(e.at(W_S9 + j), dn);
    });
    e.template sum<6>(W_S9, [&](int i, auto& acc) {
        double X[3], u[2];
        e.point(i, X, u);
        const double d0 = d_sub(X[0], e.at(W_CWS)), d1 = d_sub(X[1], e.at(W_CWS + 1)), d2 = d_sub(X[2], e.at(W_CWS + 2));
        acc.add(0, d_mul(d0, d0)); acc.add(1, d_mul(d0, d1)); acc.add(2, d_mul(d0, d2));
        acc.add(3, d_mul(d1, d1)); acc.add(4, d_mul(d1, d2)); acc.add(5, d_mul(d2, d2));
    });
    e.single([&]() {
        const double s00 = e.at(W_S9), s01 = e.at(W_S9 + 1), s02 = e.at(W_S9 + 2), s11 = e.at(W_S9 + 3), s12 = e.at(W_S9 + 4), s22 = e.at(W_S9 + 5);
        e.at(W_SA + 0) = s00; e.at(W_SA + 1) = s01; e.at(W_SA + 2) = s02;
        e.at(W_SA + 3) = s01; e.at(W_SA + 4) = s11; e.at(W_SA + 5) = s12;
        e.at(W_SA + 6) = s02; e.at(W_SA + 7) = s12; e.at(W_SA + 8) = s22;
        if (!pnp_jacobi_svd<3, 3, true>(e, W_SA, W_SV, W_SW)) e.at(W_FLAG) = 1.0;
        for (int i = 1; i < 4; ++i) {
            const double k = d_sqrt(d_div(e.at(W_SW + i - 1), dn));
            for (int j = 0; j < 3; ++j) e.at(W_CWS + 3 * i + j) = d_add(e.at(W_CWS + j), d_mul(k, e.at(W_SA + 3 * (i - 1) + j)));
        }
        // compute_barycentric_coordinates (:411-421): cc[3 i + j - 1] = cws[j][i] - cws[0][i]; its transpose is the SVD's operand
        for (int a = 0; a < 3; ++a)
            for (int k = 0; k < 3; ++k) e.at(W_SA + 3 * a + k) = d_sub(e.at(W_CWS + 3 * (a + 1) + k), e.at(W_CWS + k));
        pnp_jacobi_svd<3, 3, true>(e, W_SA, W_SV, W_SW);
        const double threshold = pnp_sv_threshold<3>(e, W_SW);
        for (int k = 0; k < 9; ++k) e.at(W_CI + k) = 0.0;
        for (int i = 0; i < 3; ++i) {
            double wi = e.at(W_SW + i);
            if (fabs(wi) <= threshold) continue;
            wi = d_div(1.0, wi);
            for (int r = 0; r < 3; ++r)
                for (int j = 0; j < 3; ++j)
                    e.at(W_CI + 3 * r + j) = d_add(e.at(W_CI + 3 * r + j), d_mul(e.at(W_SV + 3 * i + r), d_mul(e.at(W_SA + 3 * i + j), wi)));
        }
    });
    // fill_M (:436-451) and cvMulTransposed(M, MtM, 1): the upper triangle, rows 2 i and 2 i + 1 of M in turn
    e.template sum<78>(W_SUM, [&](int i, auto& acc) {
        double X[3], u[2], a[4];
        e.point(i, X, u);
        pnp_alphas(e, X, a);
        double M1[12], M2[12];
        const double du = d_sub(uc, u[0]), dv = d_sub(vc, u[1]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            M1[3 * k] = d_mul(a[k], fu); M1[3 * k + 1] = 0.0; M1[3 * k + 2] = d_mul(a[k], du);
            M2[3 * k] = 0.0; M2[3 * k + 1] = d_mul(a[k], fv); M2[3 * k + 2] = d_mul(a[k], dv);
        }
        int t = 0;
#pragma unroll
        for (int r = 0; r < 12; ++r)
#pragma unroll
            for (int c = r; c < 12; ++c, ++t) { acc.add(t, d_mul(M1[r], M1[c])); acc.add(t, d_mul(M2[r], M2[c])); }
    });
    e.single([&]() {
        int t = 77;
        for (int r = 11; r >= 0; --r)
            for (int c = 11; c >= r; --c, --t) { const double v = e.at(W_SUM + t); e.at(W_AT + 12 * r + c) = v; e.at(W_AT + 12 * c + r) = v; }
        if (!pnp_jacobi_svd<12, 12, false>(e, W_AT, 0, W_SW)) e.at(W_FLAG) = 1.0;
        // compute_L_6x10 (:760-800): v[i] = row 11 - i of ut
        for (int r = 0, a = 0, b = 1; r < 6; ++r) {
            double dv[4][3];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) dv[i][k] = d_sub(e.at(W_AT + 12 * (11 - i) + 3 * a + k), e.at(W_AT + 12 * (11 - i) + 3 * b + k));
            const int o = W_L + 10 * r;
            e.at(o + 0) = pnp_dot3(dv[0], dv[0]); e.at(o + 1) = d_mul(2.0, pnp_dot3(dv[0], dv[1])); e.at(o + 2) = pnp_dot3(dv[1], dv[1]);
            e.at(o + 3) = d_mul(2.0, pnp_dot3(dv[0], dv[2])); e.at(o + 4) = d_mul(2.0, pnp_dot3(dv[1], dv[2])); e.at(o + 5) = pnp_dot3(dv[2], dv[2]);
            e.at(o + 6) = d_mul(2.0, pnp_dot3(dv[0], dv[3])); e.at(o + 7) = d_mul(2.0, pnp_dot3(dv[1], dv[3])); e.at(o + 8) = d_mul(2.0, pnp_dot3(dv[2], dv[3]));
            e.at(o + 9) = pnp_dot3(dv[3], dv[3]);
            if (++b > 3) { ++a; b = a + 1; }
        }
        // compute_rho (:802-810)
        for (int r = 0, a = 0, b = 1; r < 6; ++r) {
            const double x = d_sub(e.at(W_CWS + 3 * a), e.at(W_CWS + 3 * b)), y = d_sub(e.at(W_CWS + 3 * a + 1), e.at(W_CWS + 3 * b + 1)),
                         z = d_sub(e.at(W_CWS + 3 * a + 2), e.at(W_CWS + 3 * b + 2));
            e.at(W_RHO + r) = d_add(d_add(d_mul(x, x), d_mul(y, y)), d_mul(z, z));
            if (++b > 3) { ++a; b = a + 1; }
        }
        double bt[4];
        // find_betas_approx_1 (:667-694)
        pnp_solve_betas<4, 1>(e);
        {
            const double b0 = e.at(W_B), b1 = e.at(W_B + 1), b2 = e.at(W_B + 2), b3 = e.at(W_B + 3);
            if (b0 < 0) { bt[0] = d_sqrt(-b0); bt[1] = d_div(-b1, bt[0]); bt[2] = d_div(-b2, bt[0]); bt[3] = d_div(-b3, bt[0]); }
            else { bt[0] = d_sqrt(b0); bt[1] = d_div(b1, bt[0]); bt[2] = d_div(b2, bt[0]); bt[3] = d_div(b3, bt[0]); }
        }
        pnp_gauss_newton(e, bt);
#pragma unroll
        for (int k = 0; k < 4; ++k) e.at(W_BETAS + k) = bt[k];
        // find_betas_approx_2 (:699-726)
        pnp_solve_betas<3, 2>(e);
        {
            const double b0 = e.at(W_B), b1 = e.at(W_B + 1), b2 = e.at(W_B + 2);
            if (b0 < 0) { bt[0] = d_sqrt(-b0); bt[1] = b2 < 0 ? d_sqrt(-b2) : 0.0; }
            else { bt[0] = d_sqrt(b0); bt[1] = b2 > 0 ? d_sqrt(b2) : 0.0; }
            if (b1 < 0) bt[0] = -bt[0];
            bt[2] = 0.0; bt[3] = 0.0;
        }
        pnp_gauss_newton(e, bt);
#pragma unroll
        for (int k = 0; k < 4; ++k) e.at(W_BETAS + 4 + k) = bt[k];
        // find_betas_approx_3 (:731-758)
        pnp_solve_betas<5, 3>(e);
        {
            const double b0 = e.at(W_B), b1 = e.at(W_B + 1), b2 = e.at(W_B + 2), b3 = e.at(W_B + 3);
            if (b0 < 0) { bt[0] = d_sqrt(-b0); bt[1] = b2 < 0 ? d_sqrt(-b2) : 0.0; }
            else { bt[0] = d_sqrt(b0); bt[1] = b2 > 0 ? d_sqrt(b2) : 0.0; }
            if (b1 < 0) bt[0] = -bt[0];
            bt[2] = d_div(b3, bt[0]); bt[3] = 0.0;
        }
        pnp_gauss_newton(e, bt);
#pragma unroll
        for (int k = 0; k < 4; ++k) e.at(W_BETAS + 8 + k) = bt[k];
    });
    // compute_R_and_t of the three variants (:651-662)
    for (int v = 0; v < 3; ++v) {
        e.single([&]() {
            // compute_ccs (:453-464)
            for (int k = 0; k < 12; ++k) e.at(W_CCS + k) = 0.0;
            for (int i = 0; i < 4; ++i)
                for (int k = 0; k < 12; ++k) e.at(W_CCS + k) = d_add(e.at(W_CCS + k), d_mul(e.at(W_BETAS + 4 * v + i), e.at(W_AT + 12 * (11 - i) + k)));
            // solve_for_sign (:636-649): the first correspondence's depth
            double X[3], u[2], a[4], pc[3];
            e.point(0, X, u);
            pnp_alphas(e, X, a);
            pnp_pc(e, a, pc);
            if (pc[2] < 0.0) for (int k = 0; k < 12; ++k) e.at(W_CCS + k) = -e.at(W_CCS + k);
        });
        // estimate_R_and_t (:569-627)
        e.template sum<3>(W_S9, [&](int i, auto& acc) {
            double X[3], u[2], a[4], pc[3];
            e.point(i, X, u);
            pnp_alphas(e, X, a);
            pnp_pc(e, a, pc);
            acc.add(0, pc[0]); acc.add(1, pc[1]); acc.add(2, pc[2]);
        });
        e.single([&]() { for (int j = 0; j < 3; ++j) e.at(W_PC0 + j) = d_div(e.at(W_S9 + j), dn); });
        e.template sum<9>(W_S9, [&](int i, auto& acc) {
            double X[3], u[2], a[4], pc[3];
            e.point(i, X, u);
            pnp_alphas(e, X, a);
            pnp_pc(e, a, pc);
            const double w0 = d_sub(X[0], e.at(W_CWS)), w1 = d_sub(X[1], e.at(W_CWS + 1)), w2 = d_sub(X[2], e.at(W_CWS + 2));
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double c = d_sub(pc[j], e.at(W_PC0 + j));
                acc.add(3 * j, d_mul(c, w0)); acc.add(3 * j + 1, d_mul(c, w1)); acc.add(3 * j + 2, d_mul(c, w2));
            }
        });
        e.single([&]() {
            for (int a = 0; a < 3; ++a)
                for (int k = 0; k < 3; ++k) e.at(W_SA + 3 * a + k) = e.at(W_S9 + 3 * k + a);
            if (!pnp_jacobi_svd<3, 3, true>(e, W_SA, W_SV, W_SW)) e.at(W_FLAG) = 1.0;
            // R[i][j] = dot(abt_u + 3 i, abt_v + 3 j): U[i][k] is At(k, i), V[j][k] is Vt(k, j)
            double R[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    R[3 * i + j] = d_add(d_add(d_mul(e.at(W_SA + i), e.at(W_SV + j)), d_mul(e.at(W_SA + 3 + i), e.at(W_SV + 3 + j))), d_mul(e.at(W_SA + 6 + i), e.at(W_SV + 6 + j)));
            double det = d_mul(d_mul(R[0], R[4]), R[8]);
            det = d_add(det, d_mul(d_mul(R[1], R[5]), R[6]));
            det = d_add(det, d_mul(d_mul(R[2], R[3]), R[7]));
            det = d_sub(det, d_mul(d_mul(R[2], R[4]), R[6]));
            det = d_sub(det, d_mul(d_mul(R[1], R[3]), R[8]));
            det = d_sub(det, d_mul(d_mul(R[0], R[5]), R[7]));
            if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            const double pw0[3] = {e.at(W_CWS), e.at(W_CWS + 1), e.at(W_CWS + 2)};
#pragma unroll
            for (int k = 0; k < 9; ++k) e.at(W_R + 9 * v + k) = R[k];
            e.at(W_T + 3 * v) = d_sub(e.at(W_PC0), pnp_dot3(R, pw0));
            e.at(W_T + 3 * v + 1) = d_sub(e.at(W_PC0 + 1), pnp_dot3(R + 3, pw0));
            e.at(W_T + 3 * v + 2) = d_sub(e.at(W_PC0 + 2), pnp_dot3(R + 6, pw0));
        });
        // reprojection_error (:550-567)
        e.template sum<1>(W_S9, [&](int i, auto& acc) {
            double X[3], u[2], R[9];
            e.point(i, X, u);
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = e.at(W_R + 9 * v + k);
            const double Xc = d_add(pnp_dot3(R, X), e.at(W_T + 3 * v)), Yc = d_add(pnp_dot3(R + 3, X), e.at(W_T + 3 * v + 1));
            const double inv_Zc = d_div(1.0, d_add(pnp_dot3(R + 6, X), e.at(W_T + 3 * v + 2)));
            const double ue = d_add(uc, d_mul(d_mul(fu, Xc), inv_Zc)), ve = d_add(vc, d_mul(d_mul(fv, Yc), inv_Zc));
            const double du = d_sub(u[0], ue), dv = d_sub(u[1], ve);
            acc.add(0, d_sqrt(d_add(d_mul(du, du), d_mul(dv, dv))));
        });
        e.single([&]() { e.at(W_ERR + v) = d_div(e.at(W_S9), dn); });
    }
    e.single([&]() {
        int N = 0;
        if (e.at(W_ERR + 1) < e.at(W_ERR)) N = 1;
        if (e.at(W_ERR + 2) < e.at(W_ERR + N)) N = 2;
        e.at(W_CHOICE) = (double)N;
    });
}

// CheckInliers for one correspondence (:314-337) with its mixed widths: Xc, Yc, invZc double sums rounded to float; ue, ve double; distX, distY, error2
// float; strict <.  R, t: mRi, mti.  Every comparison with a NaN is false.
OLF_HD bool pnp_inlier(const double* R, const double* t, const double* cam, const float* X, const float* u, float max_error)
{
    const double x = X[0], y = X[1], z = X[2];
    const float Xc = (float)d_add(d_add(d_add(d_mul(R[0], x), d_mul(R[1], y)), d_mul(R[2], z)), t[0]);
    const float Yc = (float)d_add(d_add(d_add(d_mul(R[3], x), d_mul(R[4], y)), d_mul(R[5], z)), t[1]);
    const float invZc = (float)d_div(1.0, d_add(d_add(d_add(d_mul(R[6], x), d_mul(R[7], y)), d_mul(R[8], z)), t[2]));
    const double ue = d_add(cam[2], d_mul(d_mul(cam[0], (double)Xc), (double)invZc)), ve = d_add(cam[3], d_mul(d_mul(cam[1], (double)Yc), (double)invZc));
    const float distX = (float)d_sub((double)u[0], ue), distY = (float)d_sub((double)u[1], ve);
    const float error2 = f_add(f_mul(distX, distX), f_mul(distY, distY));
    return error2 < max_error;
}

// mBestTcw / mRefinedTcw (:217-223, :294-300): eye(4, 4) with R and t converted to float
OLF_HD void pnp_tcw(const double* R, const double* t, float* T)
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[3 * i + j];
        T[4 * i + 3] = (float)t[i];
        T[12 + i] = 0.0f;
    }
    T[15] = 1.0f;
}

// The correspondences of a solver as planes of `cap` words: 0-2 the 3-D point, 3-4 the 2-D point, 5 mvMaxError, 6 the frame feature (int), 7 the list of
// the best set (int: position q of its k-th member).
struct PnpPlanes {
    const float* st;
    int cap;
    OLF_HDM void load(int q, double* X, double* u) const
    {
        X[0] = (double)st[q]; X[1] = (double)st[(size_t)cap + q]; X[2] = (double)st[(size_t)2 * cap + q];
        u[0] = (double)st[(size_t)3 * cap + q]; u[1] = (double)st[(size_t)4 * cap + q];
    }
    OLF_HDM bool inlier(int q, const double* R, const double* t, const double* cam) const
    {
        const float X[3] = {st[q], st[(size_t)cap + q], st[(size_t)2 * cap + q]}, u[2] = {st[(size_t)3 * cap + q], st[(size_t)4 * cap + q]};
        return pnp_inlier(R, t, cam, X, u, st[(size_t)5 * cap + q]);
    }
};

// the environment of a four-point fit: one thread, the reference's order.  The workspace word k is base[k * stride].
struct PnpSeqEnv {
    double* base;
    int stride;
    PnpPlanes P;
    int i0, i1, i2, i3;
    struct Acc {
        PnpSeqEnv& e;
        int off;
        OLF_HDM void add(int k, double v) { e.at(off + k) = d_add(e.at(off + k), v); }
    };
    OLF_HDM double& at(int k) { return base[(size_t)k * stride]; }
    OLF_HDM int n() const { return 4; }
    OLF_HDM void point(int i, double* X, double* u) const { P.load(i == 0 ? i0 : i == 1 ? i1 : i == 2 ? i2 : i3, X, u); }
    template <int K, class F>
    OLF_HDM void sum(int off, F f)
    {
        for (int k = 0; k < K; ++k) at(off + k) = 0.0;
        Acc acc{*this, off};
        for (int i = 0; i < 4; ++i) f(i, acc);
    }
    template <class F>
    OLF_HDM void single(F f) { f(); }
};

// the chosen pose of a finished compute_pose; false: the hypothesis is degenerate (C.24)
template <class E>
OLF_HD bool pnp_result(E& e, double* R, double* t)
{
    const int v = (int)e.at(W_CHOICE);
    for (int k = 0; k < 9; ++k) R[k] = e.at(W_R + 9 * v + k);
    for (int k = 0; k < 3; ++k) t[k] = e.at(W_T + 3 * v + k);
    return e.at(W_FLAG) == 0.0;
}

// the environment of Refine on the host: the blocked order, replayed (see the head of this file)
struct PnpHostBlockEnv {
    double* base;
    PnpPlanes P;
    const int* list;
    int count;
    template <int K>
    struct Acc {
        double part[K];
        void add(int k, double v) { part[k] = d_add(part[k], v); }
    };
    double& at(int k) { return base[k]; }
    int n() const { return count; }
    void point(int i, double* X, double* u) const { P.load(list[i], X, u); }
    template <int K, class F>
    void sum(int off, F f)
    {
        static thread_local Acc<K> acc[PNP_THREADS];
        for (int t = 0; t < PNP_THREADS; ++t)
            for (int k = 0; k < K; ++k) acc[t].part[k] = 0.0;
        for (int i = 0; i < count; ++i) f(i, acc[i % PNP_THREADS]);
        for (int k = 0; k < K; ++k) {
            double total = 0;
            for (int w = 0; w < PNP_WAVES; ++w) {
                double v[64];
                for (int l = 0; l < 64; ++l) v[l] = acc[64 * w + l].part[k];
                for (int d = 1; d < 64; d <<= 1)
                    for (int l = 0; l < 64; l += 2 * d) v[l] = d_add(v[l], v[l + d]);
                total = w == 0 ? v[0] : d_add(total, v[0]);
            }
            base[off + k] = total;
        }
    }
    template <class F>
    void single(F f) { f(); }
};

}  // namespace olf
