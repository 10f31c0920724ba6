// sim3solver_terms.hpp -- the arithmetic of Sim3Solver (src/Sim3Solver.cc) that the host form (sim3solver_host.cpp) and the kernel (sim3solver_batch.hip)
// both run: the correspondence of one match row entry (:62-109), the integer gates (:87-88, include/Sim3Solver.h:78-79), Horn's fit (:226-337) and the
// inlier test of one correspondence (:340-364, :382-403); the sample of one iteration from its three draws (:163-177) is ransac_sample<3> of
// ransac_terms.hpp, shared with pnpsolver_terms.hpp.  One text for both sides; every file
// that includes it is built with -ffp-contract=off (C.4) and the rounded operations are spelled through device_math.hpp.  cv::Mat products follow C.12
// (plain product: float sums, alpha and the C term in double, one rounding; transposed operand: double accumulation) and C.17 (Mat / scalar); new here:
//   C.20  the random stream is the caller's: draws[iteration][3], raw rand() values below 2^31; draw k of an iteration picks position
//         (int)(((double)r / 2147483648.0) * (N - k)) of the indices still available (DUtils::Random::RandomInt with glibc's RAND_MAX)
//   C.21  cv::eigen of the symmetric 4 x 4 float matrix is a cyclic Jacobi iteration in float (OpenCV's rotation formulas and its own hypot, pairs
//         (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), a pair skipped at |p| <= FLT_EPSILON, at most 30 sweeps), eigenvalues then ordered descending, the first
//         of equal maxima first; row 0 is the quaternion, whose sign does not matter
//   C.22  R12 from the quaternion by the double-angle identities in double, cos = (q0^2 - |v|^2) / |q|^2, sin = 2 q0 |v| / |q|^2, then Rodrigues'
//         c I + (1 - c) r r^T + s [r]x with r = v / |v|, each element rounded once: no libm on either side.  |v| == 0 divides 0 by 0 as the reference
//         does: every element of R is NaN and the iteration counts no inlier.
#pragma once
#include "ransac_terms.hpp"
#include "search_math.hpp"

namespace olf {

constexpr int S3_WORDS = 13;                       // 4-byte words a correspondence keeps: X1c, X2c (3 each), its two images (2 each), two gates, i1

// the float square root, correctly rounded on both sides: sqrtf, as lbd.hip takes it under C.6 (hip's __fsqrt_rn is the native 1-ulp instruction)
OLF_HD float s3_sqrtf(float a) { return sqrtf(a); }

// mvnMaxError (:87-88): the double product 9.210 * sigmaSquare truncated to size_t, compared as float (err < maxErr converts the integer);
// sigmaSquare = mvLevelSigma2[octave] = sf * sf in float
OLF_HD unsigned long long s3_gate_int(float sf) { return (unsigned long long)d_mul(9.210, (double)f_mul(sf, sf)); }
OLF_HD float s3_gate(float sf) { return (float)s3_gate_int(sf); }

// FromCameraToImage / the tail of Project (:396-401, :417-421): invz = 1 / z, x * invz, fx * x + cx in float, as written.  cam = fx, fy, cx, cy
OLF_HD void s3_image(const float* X, const float* cam, float* uv)
{
    const float invz = f_div(1.0f, X[2]);
    const float x = f_mul(X[0], invz), y = f_mul(X[1], invz);
    uv[0] = f_add(f_mul(cam[0], x), cam[2]);
    uv[1] = f_add(f_mul(cam[1], y), cam[3]);
}

OLF_HD float s3_hypot(float a, float b)             // OpenCV's own hypot<float> (modules/core/src/lapack.cpp)
{
    a = fabsf(a); b = fabsf(b);
    if (a > b) { b = f_div(b, a); return f_mul(a, s3_sqrtf(f_add(1.0f, f_mul(b, b)))); }
    if (b > 0) { a = f_div(a, b); return f_mul(b, s3_sqrtf(f_add(1.0f, f_mul(a, a)))); }
    return 0.0f;
}

// C.21: the eigenvector of the largest eigenvalue of the symmetric matrix
//   | n[0] n[1] n[2] n[3] |
//   |      n[4] n[5] n[6] |
//   |           n[7] n[8] |
//   |                n[9] |
// All indices are static after unrolling: A, V and W stay in registers on the device.
OLF_HD void s3_eigen4(const float* n, float* q)
{
    float A[4][4] = {{n[0], n[1], n[2], n[3]}, {n[1], n[4], n[5], n[6]}, {n[2], n[5], n[7], n[8]}, {n[3], n[6], n[8], n[9]}};
    float V[4][4], W[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) V[i][k] = i == k ? 1.0f : 0.0f;
        W[i] = A[i][i];
    }
    const float eps = 1.1920928955078125e-7f;                        // FLT_EPSILON
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool changed = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int l = k + 1; l < 4; ++l) {
                const float p = A[k][l];
                if (!(fabsf(p) > eps)) continue;                     // (a NaN pivot ends its pair as in the reference: |p| <= eps is false there, but
                                                                     //  every later value is NaN either way and the fit counts no inlier)
                const float y = f_mul(f_sub(W[l], W[k]), 0.5f);
                float t = f_add(fabsf(y), s3_hypot(p, y));
                float s = s3_hypot(p, t);
                const float c = f_div(t, s);
                s = f_div(p, s); t = f_mul(f_div(p, t), p);
                if (y < 0) { s = -s; t = -t; }
                A[k][l] = 0.0f;
                W[k] = f_sub(W[k], t); W[l] = f_add(W[l], t);
#define OLF_S3_ROT(v0, v1) { const float a0 = v0, b0 = v1; v0 = f_sub(f_mul(a0, c), f_mul(b0, s)); v1 = f_add(f_mul(a0, s), f_mul(b0, c)); }
#pragma unroll
                for (int i = 0; i < 4; ++i) {                        // the upper triangle's entries of rows and columns k and l
                    if (i < k) OLF_S3_ROT(A[i][k], A[i][l])
                    else if (i > k && i < l) OLF_S3_ROT(A[k][i], A[i][l])
                    else if (i > l) OLF_S3_ROT(A[k][i], A[l][i])
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) OLF_S3_ROT(V[k][i], V[l][i])
#undef OLF_S3_ROT
                changed = true;
            }
        }
        if (!changed) break;
    }
    // the row of the largest eigenvalue, the first of equal maxima (a NaN never wins a comparison)
    int m = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i) if (W[m] < W[i]) m = i;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = m == 0 ? V[0][i] : m == 1 ? V[1][i] : m == 2 ? V[2][i] : V[3][i];
}

// C.22
OLF_HD void s3_rotation(const float* q, float* R)
{
    const double q0 = q[0], v0 = q[1], v1 = q[2], v2 = q[3];
    const double vv = d_add(d_add(d_mul(v0, v0), d_mul(v1, v1)), d_mul(v2, v2)), nv = d_sqrt(vv);
    const double qq = d_add(d_mul(q0, q0), vv);
    const double c = d_div(d_sub(d_mul(q0, q0), vv), qq), s = d_div(d_mul(d_mul(2.0, q0), nv), qq), c1 = d_sub(1.0, c);
    const double r[3] = {d_div(v0, nv), d_div(v1, nv), d_div(v2, nv)};          // 0 / 0 at the identity, as vec / norm(vec) of the reference
    const double rx[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = i == j ? c : 0.0;
            R[3 * i + j] = (float)d_add(d_add(d, d_mul(c1, d_mul(r[i], r[j]))), d_mul(s, rx[3 * i + j]));
        }
}

// one hypothesis: mR12i, mt12i, ms12i, mT12i and mT21i (4 x 4 row-major; only the first three rows are read)
struct S3Hyp { float s, R[9], t[3], T12[16], T21[16]; };

// Sim3Solver::ComputeSim3 (:226-337).  P1, P2: the three sampled points of set 1 and set 2, [point][coordinate]
OLF_HD void s3_fit(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, S3Hyp& H)
{
    // ComputeCentroid (:215-224): the row sums in double, stored as float; C / P.cols by C.17; Pr = P - C in float.  Pr[coordinate][point]
    const float third = recip_f32(3.0);
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
    for (int r = 0; r < 3; ++r) {
        O1[r] = f_mul((float)d_add(d_add((double)P1[0][r], (double)P1[1][r]), (double)P1[2][r]), third);
        O2[r] = f_mul((float)d_add(d_add((double)P2[0][r], (double)P2[1][r]), (double)P2[2][r]), third);
        for (int k = 0; k < 3; ++k) { Pr1[r][k] = f_sub(P1[k][r], O1[r]); Pr2[r][k] = f_sub(P2[k][r], O2[r]); }
    }
    // M = Pr2 * Pr1.t(): a transposed operand, double accumulation, one rounding (C.12)
    float M[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc = d_add(acc, d_mul((double)Pr2[i][k], (double)Pr1[j][k]));
            M[i][j] = (float)acc;
        }
    // the ten terms in double from the float elements, stored as float (:247-265)
    const double m00 = M[0][0], m01 = M[0][1], m02 = M[0][2], m10 = M[1][0], m11 = M[1][1], m12 = M[1][2], m20 = M[2][0], m21 = M[2][1], m22 = M[2][2];
    const float n[10] = {(float)d_add(d_add(m00, m11), m22), (float)d_sub(m12, m21), (float)d_sub(m20, m02), (float)d_sub(m01, m10),
                         (float)d_sub(d_sub(m00, m11), m22), (float)d_add(m01, m10), (float)d_add(m20, m02),
                         (float)d_sub(d_add(-m00, m11), m22), (float)d_add(m12, m21), (float)d_add(d_sub(-m00, m11), m22)};
    float q[4];
    s3_eigen4(n, q);
    s3_rotation(q, H.R);
    // P3 = R * Pr2, a plain product (C.12); s = Pr1.dot(P3) / sum(P3^2): double sums over the float products / squares in row-major order (:288-311)
    if (!fix_scale) {
        double nom = 0, den = 0;
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) {
                const float p3 = f_add(f_add(f_mul(H.R[3 * i], Pr2[0][k]), f_mul(H.R[3 * i + 1], Pr2[1][k])), f_mul(H.R[3 * i + 2], Pr2[2][k]));
                nom = d_add(nom, d_mul((double)Pr1[i][k], (double)p3));
                den = d_add(den, (double)f_mul(p3, p3));
            }
        H.s = (float)d_div(nom, den);
    } else H.s = 1.0f;
    // t = O1 - s * R * O2: the plain product's float sum, alpha = -s and the C term O1 in double, one rounding (:316)
    for (int r = 0; r < 3; ++r) H.t[r] = (float)d_add(d_mul(-(double)H.s, (double)dot3_small(H.R + 3 * r, O2)), (double)O1[r]);
    // T12 = [s R | t], T21 = [(1.0 / s) R.t() | -sRinv * t] (:321-336)
    const double sinv = d_div(1.0, (double)H.s);
    float sRinv[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { H.T12[4 * i + j] = f_mul(H.s, H.R[3 * i + j]); sRinv[3 * i + j] = (float)d_mul((double)H.R[3 * j + i], sinv); }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) H.T21[4 * i + j] = sRinv[3 * i + j];
        H.T12[4 * i + 3] = H.t[i];
        H.T21[4 * i + 3] = (float)d_mul(-1.0, (double)dot3_small(sRinv + 3 * i, H.t));
        H.T12[12 + i] = 0.0f; H.T21[12 + i] = 0.0f;
    }
    H.T12[15] = 1.0f; H.T21[15] = 1.0f;
}

// CheckInliers for one correspondence (:343-356): set 2 by T12 into image 1, set 1 by T21 into image 2; dist.dot(dist) is a double sum rounded to float;
// every comparison with a NaN is false
OLF_HD bool s3_inlier(const float* T12, const float* T21, const float* cam, const float* X1, const float* X2, const float* p1, const float* p2, float g1, float g2)
{
    float Q[3], uv[2];
    rot_apply(T12, X2, 1.0f, Q);
    s3_image(Q, cam, uv);
    const float a0 = f_sub(p1[0], uv[0]), a1 = f_sub(p1[1], uv[1]);
    const float err1 = (float)d_add(d_mul((double)a0, (double)a0), d_mul((double)a1, (double)a1));
    rot_apply(T21, X1, 1.0f, Q);
    s3_image(Q, cam, uv);
    const float b0 = f_sub(uv[0], p2[0]), b1 = f_sub(uv[1], p2[1]);
    const float err2 = (float)d_add(d_mul((double)b0, (double)b0), d_mul((double)b1, (double)b1));
    return err1 < g1 && err2 < g2;
}

// The cap of SetRansacParameters (:114-138) as a function of N alone, through the host's libm (host only: the kernel reads the table its caller built).
// N < min_inliers never iterates and gets 1.  A quotient beyond max_iterations (the reference converts it to int, which is undefined from 2^31 on) is
// max_iterations.
inline int s3_iteration_cap(int N, double probability, int min_inliers, int max_iterations)
{
    int its = 1;
    if (N > min_inliers) {
        const float epsilon = (float)min_inliers / N;
        const double v = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        its = v < (double)max_iterations ? (int)v : max_iterations;
    }
    const int capped = its < max_iterations ? its : max_iterations;
    return capped > 1 ? capped : 1;
}

}  // namespace olf
