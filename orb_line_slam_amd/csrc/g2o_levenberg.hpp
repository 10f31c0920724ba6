// g2o_levenberg.hpp -- what g2o runs around a graph with ONE free vertex, whatever its edges are: OptimizationAlgorithmLevenberg over a BlockSolver with
// LinearSolverDense (Eigen::LDLT of the one block), and the Huber kernel.  Stated once for posepoints_terms.hpp (a 6-dimensional VertexSE3Expmap) and
// optsim3_terms.hpp (a 7-dimensional VertexSim3Expmap), host and device.  Plain C++ doubles, no Eigen, no HIP header, -ffp-contract=off on both sides.
//
// What is restated (Thirdparty/g2o/g2o/...):
//   core/optimization_algorithm_levenberg.cpp:61-189, sparse_optimizer.cpp:354-419, block_solver.hpp   the loop, lambda, the stop rules
//   solvers/linear_solver_dense.h        Eigen::LDLT<MatrixXd> and isPositive()
//   core/robust_kernel_impl.cpp:65-91    RobustKernelHuber
//
// Conventions: LDLT is Eigen 3.3's unblocked in-place form on the LOWER triangle (the one block of the problem is copied whole, and
// Eigen::LDLT reads the lower half): the pivot is the first largest |diagonal| of what remains, a column whose pivot is exactly zero is not scaled,
// isPositive() is "no negative pivot was seen", and solve() sets a component whose |D| <= DBL_MIN to zero.
//
// Defined here, not by the reference: a depth of exactly 0 at an evaluation stops the row (ST_DEPTH), and so does an H, b, step or estimate that is not
// finite (ST_NOT_FINITE).  A failed LDLT: g2o applies the solver's previous x again and sets tempChi = DBL_MAX; that is followed literally (x is zero at an
// optimisation's start).
#pragma once
#include <float.h>
#include "dense_math.hpp"

namespace olf {
namespace levenberg {

enum { ST_DEPTH = 1, ST_NOT_FINITE = 2, ST_OCTAVE = 4 };          // a row's own status word (the host forms add 512 / 2048 of the context's)

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1]
PT_HD void huber(double e, double delta, double* rho0, double* rho1)
{
    const double dsqr = delta * delta;
    if (e <= dsqr) { *rho0 = e; *rho1 = 1.0; }
    else { const double sq = sqrt(e); *rho0 = (2.0 * sq) * delta - dsqr; *rho1 = delta / sq; }
}

// ---- Eigen::LDLT<MatrixXd> of a D x D matrix and its solve (what LinearSolverDense calls) ------------------------------------------------------------------
// A: row-major, only the lower triangle is read.  Returns isPositive(); x is written only then (linear_solver_dense.h:107-112).
template <int D>
PT_HD bool ldlt_solve(const double* A, const double* b, double* x)
{
    double M[D * D], tmp[D], y[D];
    int tr[D];
    for (int i = 0; i < D; ++i) for (int j = 0; j < D; ++j) M[i * D + j] = j <= i ? A[i * D + j] : 0.0;
    int sign = 0;                                                   // ZeroSign; 1 PositiveSemiDef, -1 NegativeSemiDef, 2 Indefinite
    bool all_zero = false;
    for (int k = 0; k < D; ++k) {
        int p = k;
        double big = fabs(M[k * D + k]);
        for (int i = k + 1; i < D; ++i) if (fabs(M[i * D + i]) > big) { big = fabs(M[i * D + i]); p = i; }
        tr[k] = p;
        if (p != k) {
            for (int j = 0; j < k; ++j) { const double t = M[k * D + j]; M[k * D + j] = M[p * D + j]; M[p * D + j] = t; }
            for (int i = p + 1; i < D; ++i) { const double t = M[i * D + k]; M[i * D + k] = M[i * D + p]; M[i * D + p] = t; }
            { const double t = M[k * D + k]; M[k * D + k] = M[p * D + p]; M[p * D + p] = t; }
            for (int i = k + 1; i < p; ++i) { const double t = M[i * D + k]; M[i * D + k] = M[p * D + i]; M[p * D + i] = t; }
        }
        if (k > 0) {
            for (int j = 0; j < k; ++j) tmp[j] = M[j * D + j] * M[k * D + j];
            double s = M[k * D] * tmp[0];
            for (int j = 1; j < k; ++j) s = s + M[k * D + j] * tmp[j];
            M[k * D + k] = M[k * D + k] - s;
            for (int i = k + 1; i < D; ++i) {
                double r = M[i * D] * tmp[0];
                for (int j = 1; j < k; ++j) r = r + M[i * D + j] * tmp[j];
                M[i * D + k] = M[i * D + k] - r;
            }
        }
        const double akk = M[k * D + k];
        const bool valid = fabs(akk) > 0.0;
        if (k == 0 && !valid) { for (int j = 0; j < D; ++j) tr[j] = j; all_zero = true; break; }      // the whole diagonal is zero: ZeroSign
        if (valid) for (int i = k + 1; i < D; ++i) M[i * D + k] = M[i * D + k] / akk;
        if (sign == 1) { if (akk < 0.0) sign = 2; }
        else if (sign == -1) { if (akk > 0.0) sign = 2; }
        else if (sign == 0) { if (akk > 0.0) sign = 1; else if (akk < 0.0) sign = -1; }
    }
    if (!(sign == 1 || sign == 0)) return false;
    for (int i = 0; i < D; ++i) y[i] = b[i];
    for (int k = 0; k < D; ++k) if (tr[k] != k) { const double t = y[k]; y[k] = y[tr[k]]; y[tr[k]] = t; }
    if (!all_zero) for (int j = 0; j < D; ++j) for (int i = j + 1; i < D; ++i) y[i] = y[i] - M[i * D + j] * y[j];          // L^-1, column by column
    for (int i = 0; i < D; ++i) y[i] = fabs(M[i * D + i]) > DBL_MIN ? y[i] / M[i * D + i] : 0.0;                            // D^-1
    if (!all_zero)
        for (int i = D - 2; i >= 0; --i) {                                                                                  // L^-T, row by row
            double s = M[(i + 1) * D + i] * y[i + 1];
            for (int j = i + 2; j < D; ++j) s = s + M[j * D + i] * y[j];
            y[i] = y[i] - s;
        }
    for (int k = D - 1; k >= 0; --k) if (tr[k] != k) { const double t = y[k]; y[k] = y[tr[k]]; y[tr[k]] = t; }
    for (int i = 0; i < D; ++i) x[i] = y[i];
    return true;
}

// ---- OptimizationAlgorithmLevenberg over one vertex of dimension V::D --------------------------------------------------------------------------------------
// V:    enum { D };  void oplus(double* x) (oplusImpl: x is the solver's array, which a vertex may write);  bool finite() const;  copyable (push / pop)
// Ops:  bool errors(const V& v, bool robust, double* chi)      computeActiveErrors at v (every active edge's _error is replaced) and activeRobustChi2;
//                                                               false: a depth of 0 (the stored errors are then unspecified, the row stops)
//       bool system(const V& v, bool robust, double* S)        buildSystem: S[D (D + 1) / 2 + D], H's lower triangle row by row and -b, over the active edges
// Returns the iterations done, or LM_STOP with the reason in *status.
enum { LM_STOP = -1 };
template <class V, class Ops>
PT_HD int lm_optimize(Ops& ops, V& v, int iterations, bool robust, int* status)
{
    enum { D = V::D, NH = D * (D + 1) / 2 };
    double lambda = -1.0, ni = 2.0, x[D], H[D * D], Hl[D * D], b[D], S[NH + D];
    int n_bad = 0, done = 0;
    for (int i = 0; i < D; ++i) x[i] = 0.0;
    for (int it = 0; it < iterations; ++it) {                       // SparseOptimizer::optimize, sparse_optimizer.cpp:376-414
        // ---- OptimizationAlgorithmLevenberg::solve(it), optimization_algorithm_levenberg.cpp:61-164
        double cur, tmp;
        if (!ops.errors(v, robust, &cur)) { *status |= ST_DEPTH; return LM_STOP; }
        const double ini = cur;
        if (!ops.system(v, robust, S)) { *status |= ST_DEPTH; return LM_STOP; }
        bool ok = true;
        for (int i = 0; i < NH + D; ++i) ok = ok && dense::finite_d(S[i]);
        if (!ok) { *status |= ST_NOT_FINITE; return LM_STOP; }
        int k = 0;
        for (int i = 0; i < D; ++i) for (int j = 0; j <= i; ++j) { H[i * D + j] = S[k]; H[j * D + i] = S[k]; ++k; }
        for (int i = 0; i < D; ++i) b[i] = -S[NH + i];
        if (it == 0) {                                              // computeLambdaInit, :166-180
            double md = 0.0;
            for (int j = 0; j < D; ++j) md = dense::max_d(fabs(H[j * D + j]), md);
            lambda = 1e-5 * md; ni = 2.0; n_bad = 0;
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            const V backup = v;                                     // push()
            for (int i = 0; i < D * D; ++i) Hl[i] = H[i];
            for (int i = 0; i < D; ++i) Hl[i * D + i] = Hl[i * D + i] + lambda;      // setLambda; restoreDiagonal is H itself
            const bool ok2 = ldlt_solve<D>(Hl, b, x);
            for (int i = 0; i < D; ++i) ok = ok && dense::finite_d(x[i]);
            if (!ok) { *status |= ST_NOT_FINITE; return LM_STOP; }
            v.oplus(x);
            if (!v.finite()) { v = backup; *status |= ST_NOT_FINITE; return LM_STOP; }
            if (!ops.errors(v, robust, &tmp)) { v = backup; *status |= ST_DEPTH; return LM_STOP; }
            if (!ok2) tmp = DBL_MAX;
            rho = cur - tmp;
            double scale = 0.0;                                     // computeScale, :182-189
            for (int j = 0; j < D; ++j) scale = scale + x[j] * (lambda * x[j] + b[j]);
            scale = scale + 1e-3;
            rho = rho / scale;
            if (rho > 0.0 && dense::finite_d(tmp)) {
                double alpha = 1.0 - pow(2.0 * rho - 1.0, 3.0);
                alpha = dense::min_d(alpha, 2. / 3.);
                lambda = lambda * dense::max_d(1. / 3., alpha);
                ni = 2.0;
                cur = tmp;
            } else {
                lambda = lambda * ni;
                ni = ni * 2.0;
                v = backup;                                         // pop(): the vertex comes back, the edges keep the errors of the rejected estimate
            }
            qmax++;
        } while (rho < 0.0 && qmax < 10);
        ++done;
        if (qmax == 10 || rho == 0.0) break;                        // Terminate
        if ((ini - cur) * 1e3 < ini) n_bad++; else n_bad = 0;
        if (n_bad >= 3) break;
    }
    return done;
}

}  // namespace levenberg
}  // namespace olf
