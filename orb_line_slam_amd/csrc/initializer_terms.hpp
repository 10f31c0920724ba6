// initializer_terms.hpp -- the arithmetic of Initializer (src/Initializer.cc) that the host form (initializer_host.cpp) and the kernel
// (initializer_batch.hip) both run: Normalize (:749-795), ComputeH21 / ComputeF21 (:226-303), CheckHomography / CheckFundamental (:305-468), the motion
// hypotheses of ReconstructF with DecomposeE (:470-570, :909-929) and of ReconstructH (:572-732), one correspondence of CheckRT with Triangulate (:734-747,
// :798-907) and the decisions behind the counts.  One text for both sides; every file that includes it is built with -ffp-contract=off (C.4): products,
// sums and differences are plain operators, quotients and roots go through device_math.hpp (f_div, d_div, d_sqrt).  The cv::Mat products are C.12's
// (mat3_mul_small, dot3_small, r3_apply), Mat / scalar is C.17 (recip_f32), the 3 x 3 cv::invert and cv::determinant are C.18's closed forms, and the
// 4 x 4 decomposition of Triangulate IS newpoints_terms.hpp's jacobi_null4 (C.19): there is no second one.
//
// How one text serves a lane that fits eight points and the host: a fit is written against a workspace E
//   e.at(k)    float word k of the fit's workspace of INI_WS_F floats (a plain array on the host, lane-interleaved LDS in the kernel)
//   e.dat(k)   double word k of its INI_WS_D doubles: the squared norms JacobiSVDImpl_ keeps in double
// so a fit holds no run-time indexed array in registers.  A SUM OVER CORRESPONDENCES (the scores of CheckHomography / CheckFundamental) is one
// accumulator walking q = 0 .. N - 1 from +0 in the reference's order: ini_score_h / ini_score_f, one thread per hypothesis on both sides.  What one
// thread does between two such walks is plain code of the caller.
// New conventions, all behind OpenCV and unpinned like C.12:
//   C.30  cv::SVDecomp / cv::SVD::compute of a CV_32F matrix is OpenCV 3.4's JacobiSVDImpl_<float> without LAPACK at every shape -- ini_jacobi_svd,
//         C.19's constants: rows of the n x m operand At (m >= n: the transposed matrix, or the matrix itself where it has fewer rows than columns) are
//         rotated pair by pair in cyclic sweeps, at most max(m, 30) of them, a pair skipped at |p| <= 2 FLT_EPSILON sqrt(a b); norms and dot products are
//         double sums of double products, c and s are rounded to float, rotated entries are float; singular values descending by a selection that takes
//         the first of equal maxima; a row is normalised by (float)(1 / norm) where norm > FLT_MIN.  16 x 9 (ComputeH21): At is 9 rows of 16 and vt is
//         the accumulated V, vt.row(8) needs no fill.  8 x 9 (ComputeF21): At is A itself, vt.row(k < 8) its normalised rows and vt.row(8) C.31's fill.
//         3 x 3 (Fpre, ReconstructH's A, DecomposeE): u = At^t, vt = V.
//   C.31  the row of a zero singular value (norm <= FLT_MIN, or a row beyond n), UNVERIFIED, restated from memory of OpenCV 3.4's lapack.cpp: one
//         RNG(0x12345678) per decomposition, state s -> (uint32)s * 4164903690 + (s >> 32), next() its low word; element k = +-(float)(1. / m), plus
//         where next() & 256; two rounds of: for each earlier row j, sd = the double sum of the FLOAT products row[k] * rowj[k], row[k] = (float)(row[k] -
//         sd * rowj[k]), asum = the float sum of |row[k]|, row *= (asum > 100 eps ? 1 / asum : 0); then the double norm.  OpenCV repeats this while the
//         norm stays <= FLT_MIN; here at most INI_FILL_ATTEMPTS times, then the row is scaled by 0 and the decomposition reports it.  In ComputeF21 a
//         give-up, or one of A's own eight rows at norm <= FLT_MIN, makes the hypothesis DEGENERATE in C.24's sense: it scores 0 and bit 32768 is set.
//   C.32  Normalize sums over ALL key points of a frame sequentially in float from +0; the Check* functions add th - chiSquare sequentially in float
//         over the correspondences in ascending reference feature; everything in them is float but 1.0 / x, a double quotient rounded to float.  The best
//         hypothesis of a RANSAC is the first of the maxima under strict >; a NaN score never wins.
//   C.33  quirks, kept or defined: FindFundamental sizes its flags from an empty vector (:178), so with no F iteration above 0 the flags are all false;
//         N < 8 (undefined in the reference) is ok = 0, model = 0; RH = SH / (SH + SF) may be NaN, then F is tried; 0.7 * maxGood, 0.9 * N and
//         0.75 * bestGood are double products compared with ints; `-R.t() * t` is alpha = -1 on the plain product of the materialised transpose;
//         `K.t() * F21` and `u * W.t()` take cv::gemm's generic path (double accumulation, one rounding).
//   C.34  parallax = acos(c) * 180 / CV_PI -- acosf, a float product with 180, a double quotient, stored to float -- is only ever compared with
//         min_parallax (> in ReconstructF, >= in ReconstructH): the entry finds on the host, with the host's libm, the largest float cosine for which
//         each comparison holds (ini_cos_threshold, initializer_host.cpp) and both sides compare cosines.  nGood == 0 is parallax = 0, compared directly.
//         cos_parallax is what is stored, never degrees: the Python wrapper and the adaptor convert on the host.
//   C.35  sort(vCosParallax)[min(50, n - 1)] is a selection.  The order is by value with -0 = +0, a NaN (a zero distance; undefined under std::sort)
//         LAST, equal values by ascending correspondence; a NaN among the good cosines sets bit 65536.
#pragma once
#include "ransac_terms.hpp"
#include "newpoints_terms.hpp"

// OLF_HD on a member function (device_math.hpp's host form is `static inline`, which a member cannot be)
#ifndef OLF_HDM
#if defined(__HIPCC__)
#define OLF_HDM __host__ __device__ __forceinline__
#else
#define OLF_HDM inline
#endif
#endif

namespace olf {

constexpr int STATUS_INI_DEGENERATE = 32768, STATUS_INI_NAN = 65536;
constexpr int INI_WORDS = 8;                 // 4-byte words a correspondence keeps: u1 v1 u2 v2, its reference feature, a cosine, CheckRT's code, its flags
constexpr int INI_THREADS = 256, INI_WAVES = 4;
constexpr int INI_FILL_ATTEMPTS = 4;         // C.31
constexpr int INI_WS_A = 0, INI_WS_V = 144;  // At (9 x 16, or 9 x 9 and the 3 x 3 behind it at INI_WS_A3); V (9 x 9, or 3 x 3)
constexpr int INI_WS_A3 = 81;
constexpr int INI_WS_F = 225, INI_WS_D = 9;

// the workspace of one fit: word k of slot `this` among `stride` interleaved ones
struct IniWs {
    float* f;
    double* d;
    int stride;
    OLF_HDM float& at(int k) { return f[(size_t)k * stride]; }
    OLF_HDM double& dat(int k) { return d[(size_t)k * stride]; }
};

OLF_HD float ini_sqrtf(float x) { return (float)d_sqrt((double)x); }      // std::sqrt(float): the double root rounded again is the correctly rounded float root
OLF_HD bool ini_finite(float x) { return x - x == 0.0f; }

// ---- C.30 / C.31.  At: N1 rows of M floats at e.at(oA + i * M + k), the first N the operand's; V (WANT_V): N x N at oV; the squared norms at e.dat(0 .. N).
// WANT_U: the rows of At are ordered with the singular values, normalised, and rows of a zero singular value filled (i < N1).  w (or NULL): the N
// singular values as floats.  Returns bit 0: one of the N rows had norm <= FLT_MIN; bit 1: a fill gave up.
template <int M, int N, int N1, bool WANT_V, bool WANT_U, class E>
OLF_HD int ini_jacobi_svd(E& e, int oA, int oV, float* w)
{
    const float eps = 1.1920928955078125e-7f * 2;
    const double minval = 1.1754943508222875e-38;
    for (int i = 0; i < N; ++i) {
        double sd = 0;
        for (int k = 0; k < M; ++k) { const double t = (double)e.at(oA + i * M + k); sd += t * t; }
        e.dat(i) = sd;
        if (WANT_V) for (int k = 0; k < N; ++k) e.at(oV + i * N + k) = i == k ? 1.0f : 0.0f;
    }
    const int max_iter = M > 30 ? M : 30;
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
        for (int i = 0; i < N - 1; ++i)
            for (int j = i + 1; j < N; ++j) {
                double a = e.dat(i), p = 0, b = e.dat(j);
                for (int k = 0; k < M; ++k) p += (double)e.at(oA + i * M + k) * (double)e.at(oA + j * M + k);
                if (fabs(p) <= (double)eps * d_sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = d_sqrt(p * p + beta * beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)d_sqrt(d_div(delta, gamma));
                    c = (float)d_div(p, gamma * (double)s * 2);
                } else {
                    c = (float)d_sqrt(d_div(gamma + beta, gamma * 2));
                    s = (float)d_div(p, gamma * (double)c * 2);
                }
                a = 0; b = 0;
                for (int k = 0; k < M; ++k) {
                    const float x = e.at(oA + i * M + k), y = e.at(oA + j * M + k);
                    const float t0 = c * x + s * y, t1 = -s * x + c * y;
                    e.at(oA + i * M + k) = t0; e.at(oA + j * M + k) = t1;
                    a += (double)t0 * (double)t0; b += (double)t1 * (double)t1;
                }
                e.dat(i) = a; e.dat(j) = b;
                changed = true;
                if (WANT_V)
                    for (int k = 0; k < N; ++k) {
                        const float x = e.at(oV + i * N + k), y = e.at(oV + j * N + k);
                        e.at(oV + i * N + k) = c * x + s * y;
                        e.at(oV + j * N + k) = -s * x + c * y;
                    }
            }
        if (!changed) break;
    }
    for (int i = 0; i < N; ++i) {
        double sd = 0;
        for (int k = 0; k < M; ++k) { const double t = (double)e.at(oA + i * M + k); sd += t * t; }
        e.dat(i) = d_sqrt(sd);
    }
    for (int i = 0; i < N - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < N; ++k) if (e.dat(j) < e.dat(k)) j = k;
        if (i != j) {
            { const double t = e.dat(i); e.dat(i) = e.dat(j); e.dat(j) = t; }
            if (WANT_U) for (int k = 0; k < M; ++k) { const float t = e.at(oA + i * M + k); e.at(oA + i * M + k) = e.at(oA + j * M + k); e.at(oA + j * M + k) = t; }
            if (WANT_V) for (int k = 0; k < N; ++k) { const float t = e.at(oV + i * N + k); e.at(oV + i * N + k) = e.at(oV + j * N + k); e.at(oV + j * N + k) = t; }
        }
    }
    if (w) for (int i = 0; i < N; ++i) w[i] = (float)e.dat(i);
    int flags = 0;
    if (!WANT_U) return flags;
    uint64_t rng = 0x12345678u;
    for (int i = 0; i < N1; ++i) {
        double sd = i < N ? e.dat(i) : 0.0;
        if (i < N && sd <= minval) flags |= 1;
        for (int ii = 0; ii < INI_FILL_ATTEMPTS && sd <= minval; ++ii) {
            const float val0 = (float)d_div(1., (double)M);
            for (int k = 0; k < M; ++k) {
                rng = (uint64_t)(uint32_t)rng * 4164903690u + (rng >> 32);
                e.at(oA + i * M + k) = ((uint32_t)rng & 256u) != 0 ? val0 : -val0;
            }
            for (int iter = 0; iter < 2; ++iter)
                for (int j = 0; j < i; ++j) {
                    sd = 0;
                    for (int k = 0; k < M; ++k) sd += (double)(e.at(oA + i * M + k) * e.at(oA + j * M + k));
                    float asum = 0;
                    for (int k = 0; k < M; ++k) {
                        const float t = (float)((double)e.at(oA + i * M + k) - sd * (double)e.at(oA + j * M + k));
                        e.at(oA + i * M + k) = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100.0f ? f_div(1.0f, asum) : 0.0f;
                    for (int k = 0; k < M; ++k) e.at(oA + i * M + k) = e.at(oA + i * M + k) * asum;
                }
            sd = 0;
            for (int k = 0; k < M; ++k) { const double t = (double)e.at(oA + i * M + k); sd += t * t; }
            sd = d_sqrt(sd);
        }
        if (!(sd > minval)) flags |= 2;
        const float s = (float)(sd > minval ? d_div(1., sd) : 0.);
        for (int k = 0; k < M; ++k) e.at(oA + i * M + k) = e.at(oA + i * M + k) * s;
    }
    return flags;
}

// the 3 x 3 decomposition of A (row-major) with u and vt, on the fit's workspace (INI_WS_A3, INI_WS_V); returns ini_jacobi_svd's flags
template <class E>
OLF_HD int ini_svd3(E& e, const float* A, float* w, float* u, float* vt)
{
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) e.at(INI_WS_A3 + 3 * i + k) = A[3 * k + i];
    const int flags = ini_jacobi_svd<3, 3, 3, true, true>(e, INI_WS_A3, INI_WS_V, w);
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) { u[3 * i + k] = e.at(INI_WS_A3 + 3 * k + i); vt[3 * i + k] = e.at(INI_WS_V + 3 * i + k); }
    return flags;
}

// cv::determinant of a 3 x 3 CV_32F matrix: in double, C.18's form
OLF_HD double ini_det3(const float* s)
{
    const double m0 = s[0], m1 = s[1], m2 = s[2], m3 = s[3], m4 = s[4], m5 = s[5], m6 = s[6], m7 = s[7], m8 = s[8];
    return m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6) + m2 * (m3 * m7 - m4 * m6);
}

// ---- Normalize (:749-795) of one axis of one frame's key points: the mean and the scale (C.32)
struct IniNorm { float mx, my, sx, sy; };
OLF_HD void ini_normalize_axis(const olf_keypoint* kp, int n, int axis, float* mean, float* scale)
{
    float m = 0;
    for (int i = 0; i < n; ++i) m += axis ? kp[i].y : kp[i].x;
    m = f_div(m, (float)n);
    float dev = 0;
    for (int i = 0; i < n; ++i) dev += fabsf((axis ? kp[i].y : kp[i].x) - m);
    dev = f_div(dev, (float)n);
    *mean = m;
    *scale = (float)d_div(1.0, (double)dev);
}
OLF_HD void ini_T(const IniNorm& n, float* T)
{
    T[0] = n.sx; T[1] = 0.0f; T[2] = -n.mx * n.sx;
    T[3] = 0.0f; T[4] = n.sy; T[5] = -n.my * n.sy;
    T[6] = 0.0f; T[7] = 0.0f; T[8] = 1.0f;
}

// The correspondences of a pair as planes of `cap` words: 0-3 u1 v1 u2 v2 (mvKeys1[first].pt, mvKeys2[second].pt), 4 the reference feature (int),
// 5 CheckRT's cosine, 6 CheckRT's code (int), 7 the flags (int: bit 0 the best H's, bit 1 the best F's)
struct IniPlanes {
    float* st;
    int cap;
    OLF_HDM void load(int q, float* c) const { c[0] = st[q]; c[1] = st[(size_t)cap + q]; c[2] = st[(size_t)2 * cap + q]; c[3] = st[(size_t)3 * cap + q]; }
    OLF_HDM int& feat(int q) const { return reinterpret_cast<int*>(st + (size_t)4 * cap)[q]; }
    OLF_HDM float& cosv(int q) const { return st[(size_t)5 * cap + q]; }
    OLF_HDM int& code(int q) const { return reinterpret_cast<int*>(st + (size_t)6 * cap)[q]; }
    OLF_HDM int& flags(int q) const { return reinterpret_cast<int*>(st + (size_t)7 * cap)[q]; }
};

// ---- CheckHomography (:305-388) / CheckFundamental (:390-468) for one correspondence: what it adds to the score, and bIn
OLF_HD bool ini_check_h(const float* H21, const float* H12, const float* c, float invSigmaSquare, float& score)
{
    const float th = 5.991f;
    const float u1 = c[0], v1 = c[1], u2 = c[2], v2 = c[3];
    bool bIn = true;
    const float w2in1inv = (float)d_div(1.0, (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score += th - chiSquare1;
    const float w1in2inv = (float)d_div(1.0, (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score += th - chiSquare2;
    return bIn;
}
OLF_HD bool ini_check_f(const float* F, const float* c, float invSigmaSquare, float& score)
{
    const float th = 3.841f, thScore = 5.991f;
    const float u1 = c[0], v1 = c[1], u2 = c[2], v2 = c[3];
    bool bIn = true;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = f_div(num2 * num2, a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score += thScore - chiSquare1;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = f_div(num1 * num1, a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score += thScore - chiSquare2;
    return bIn;
}
OLF_HD float ini_inv_sigma_square(float sigma) { return (float)d_div(1.0, (double)(sigma * sigma)); }

// the sequential scores (C.32)
OLF_HD float ini_score_h(const IniPlanes& P, int N, const float* H21, const float* H12, float invSigmaSquare)
{
    float score = 0;
    for (int q = 0; q < N; ++q) { float c[4]; P.load(q, c); ini_check_h(H21, H12, c, invSigmaSquare, score); }
    return score;
}
OLF_HD float ini_score_f(const IniPlanes& P, int N, const float* F, float invSigmaSquare)
{
    float score = 0;
    for (int q = 0; q < N; ++q) { float c[4]; P.load(q, c); ini_check_f(F, c, invSigmaSquare, score); }
    return score;
}

// ---- one iteration of FindHomography (:150-163): ComputeH21 of the eight sampled correspondences, H21i = T2inv * Hn * T1, H12i = H21i.inv()
template <class E>
OLF_HD void ini_fit_h(E& e, const IniPlanes& P, const int* idx, const IniNorm& n1, const IniNorm& n2, float* H21, float* H12)
{
    for (int i = 0; i < 8; ++i) {
        float c[4];
        P.load(idx[i], c);
        const float u1 = (c[0] - n1.mx) * n1.sx, v1 = (c[1] - n1.my) * n1.sy, u2 = (c[2] - n2.mx) * n2.sx, v2 = (c[3] - n2.my) * n2.sy;
        const float r0[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, -u2 * u1, -u2 * v1, -u2};
#pragma unroll
        for (int k = 0; k < 9; ++k) { e.at(INI_WS_A + k * 16 + 2 * i) = r0[k]; e.at(INI_WS_A + k * 16 + 2 * i + 1) = r1[k]; }
    }
    ini_jacobi_svd<16, 9, 9, true, false>(e, INI_WS_A, INI_WS_V, (float*)nullptr);
    float Hn[9], T1[9], T2[9], T2inv[9], M[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Hn[k] = e.at(INI_WS_V + 72 + k);
    ini_T(n1, T1); ini_T(n2, T2);
    inv3_f32(T2, T2inv);
    mat3_mul_small(T2inv, Hn, M);
    mat3_mul_small(M, T1, H21);
    inv3_f32(H21, H12);
}

// one iteration of FindFundamental (:201-212): ComputeF21, F21i = T2t * Fn * T1.  false: degenerate (C.31)
template <class E>
OLF_HD bool ini_fit_f(E& e, const IniPlanes& P, const int* idx, const IniNorm& n1, const IniNorm& n2, float* F21)
{
    for (int i = 0; i < 8; ++i) {
        float c[4];
        P.load(idx[i], c);
        const float u1 = (c[0] - n1.mx) * n1.sx, v1 = (c[1] - n1.my) * n1.sy, u2 = (c[2] - n2.mx) * n2.sx, v2 = (c[3] - n2.my) * n2.sy;
        const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0f};
#pragma unroll
        for (int k = 0; k < 9; ++k) e.at(INI_WS_A + i * 9 + k) = r[k];
    }
    for (int k = 0; k < 9; ++k) e.at(INI_WS_A + 72 + k) = 0.0f;
    const int flags = ini_jacobi_svd<9, 8, 9, false, true>(e, INI_WS_A, INI_WS_V, (float*)nullptr);
    float Fpre[9], w[3], u[9], vt[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Fpre[k] = e.at(INI_WS_A + 72 + k);
    ini_svd3(e, Fpre, w, u, vt);
    const float D[9] = {w[0], 0.0f, 0.0f, 0.0f, w[1], 0.0f, 0.0f, 0.0f, 0.0f};
    float M[9], Fn[9], T1[9], T2[9];
    mat3_mul_small(u, D, M);
    mat3_mul_small(M, vt, Fn);
    ini_T(n1, T1); ini_T(n2, T2);
    const float T2t[9] = {T2[0], T2[3], T2[6], T2[1], T2[4], T2[7], T2[2], T2[5], T2[8]};
    mat3_mul_small(T2t, Fn, M);
    mat3_mul_small(M, T1, F21);
    return flags == 0;
}

// RH = SH / (SH + SF); RH > 0.40 (:112-115): a NaN tries F (C.33)
OLF_HD bool ini_choose_h(float SH, float SF) { return (double)f_div(SH, SH + SF) > 0.40; }

// ---- a motion hypothesis as CheckRT prepares it (:803-826): P2 = K * [R | t] (C.12), O2 = -R.t() * t (C.33)
struct IniCam { float fx, fy, cx, cy; };
struct IniPose { float R[9], t[3], P2[12], O2[3]; };
OLF_HD void ini_pose_prepare(const IniCam& K, const float* R, const float* t, IniPose& o)
{
    const float Km[9] = {K.fx, 0.0f, K.cx, 0.0f, K.fy, K.cy, 0.0f, 0.0f, 1.0f};
    for (int k = 0; k < 9; ++k) o.R[k] = R[k];
    for (int k = 0; k < 3; ++k) o.t[k] = t[k];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            const float b0 = c < 3 ? R[c] : t[0], b1 = c < 3 ? R[3 + c] : t[1], b2 = c < 3 ? R[6 + c] : t[2];
            o.P2[4 * r + c] = Km[3 * r] * b0 + Km[3 * r + 1] * b1 + Km[3 * r + 2] * b2;
        }
    for (int r = 0; r < 3; ++r) {
        const float t0 = R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2];
        o.O2[r] = (float)((double)t0 * -1.0);
    }
}

// One correspondence of CheckRT's loop (:830-894) with Triangulate (:734-747).  Returns 0: not counted; 1: counted (nGood, vCosParallax and vP3D take
// it); 3: counted and vbGood.  p3d and cosParallax are written when counted.
OLF_HD int ini_check_point(const IniCam& K, const IniPose& H, const float* c, float th2, float* p3d, float& cosParallax)
{
    const float P1[12] = {K.fx, 0.0f, K.cx, 0.0f, 0.0f, K.fy, K.cy, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    float A[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        A[0][k] = c[0] * P1[8 + k] - P1[k];
        A[1][k] = c[1] * P1[8 + k] - P1[4 + k];
        A[2][k] = c[2] * H.P2[8 + k] - H.P2[k];
        A[3][k] = c[3] * H.P2[8 + k] - H.P2[4 + k];
    }
    float v4[4], x[3];
    jacobi_null4(A, v4);
    const float inv = recip_f32((double)v4[3]);
    for (int k = 0; k < 3; ++k) x[k] = v4[k] * inv;
    if (!ini_finite(x[0]) || !ini_finite(x[1]) || !ini_finite(x[2])) return 0;
    // Check parallax
    const float normal1[3] = {x[0] - 0.0f, x[1] - 0.0f, x[2] - 0.0f};
    const float dist1 = norm3_f32(normal1);
    const float normal2[3] = {x[0] - H.O2[0], x[1] - H.O2[1], x[2] - H.O2[2]};
    const float dist2 = norm3_f32(normal2);
    double dot = 0;
    for (int k = 0; k < 3; ++k) dot += (double)normal1[k] * (double)normal2[k];
    const float cosP = (float)d_div(dot, (double)(dist1 * dist2));
    // Check depth in front of first camera (only if enough parallax, as "infinite" points can easily go to negative depth)
    if (x[2] <= 0 && (double)cosP < 0.99998) return 0;
    float x2[3];
    r3_apply(H.R, x, H.t, x2);
    if (x2[2] <= 0 && (double)cosP < 0.99998) return 0;
    // Check reprojection error in first image
    const float invZ1 = (float)d_div(1.0, (double)x[2]);
    const float im1x = K.fx * x[0] * invZ1 + K.cx, im1y = K.fy * x[1] * invZ1 + K.cy;
    const float squareError1 = (im1x - c[0]) * (im1x - c[0]) + (im1y - c[1]) * (im1y - c[1]);
    if (squareError1 > th2) return 0;
    // Check reprojection error in second image
    const float invZ2 = (float)d_div(1.0, (double)x2[2]);
    const float im2x = K.fx * x2[0] * invZ2 + K.cx, im2y = K.fy * x2[1] * invZ2 + K.cy;
    const float squareError2 = (im2x - c[2]) * (im2x - c[2]) + (im2y - c[3]) * (im2y - c[3]);
    if (squareError2 > th2) return 0;
    cosParallax = cosP;
    p3d[0] = x[0]; p3d[1] = x[1]; p3d[2] = x[2];
    return (double)cosP < 0.99998 ? 3 : 1;
}
OLF_HD float ini_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }

// C.35: the key a cosine is ordered by
OLF_HD uint32_t ini_cos_key(float c)
{
    if (c != c) return 0xffffffffu;
    if (c == 0.0f) c = 0.0f;
    const uint32_t u = f2bits(c);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- the motion hypotheses of ReconstructF (:479-497) with DecomposeE (:909-929): Rs [4][9], ts [4][3] in the order (R1, t) (R2, t) (R1, -t) (R2, -t).
// Returns ini_jacobi_svd's flags.
template <class E>
OLF_HD int ini_hypotheses_f(E& e, const float* F21, const IniCam& K, float* Rs, float* ts)
{
    const float Km[9] = {K.fx, 0.0f, K.cx, 0.0f, K.fy, K.cy, 0.0f, 0.0f, 1.0f};
    float M[9], E21[9], w[3], u[9], vt[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc += (double)Km[3 * k + i] * (double)F21[3 * k + j];
            M[3 * i + j] = (float)acc;
        }
    mat3_mul_small(M, Km, E21);
    const int flags = ini_svd3(e, E21, w, u, vt);
    float t[3] = {u[2], u[5], u[8]};
    const float inv = recip_f32(norm3(t));
    for (int k = 0; k < 3; ++k) t[k] = t[k] * inv;
    const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float R1[9], R2[9];
    mat3_mul_small(u, W, M);
    mat3_mul_small(M, vt, R1);
    if (ini_det3(R1) < 0) for (int k = 0; k < 9; ++k) R1[k] = R1[k] * -1.0f + 0.0f;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc += (double)u[3 * i + k] * (double)W[3 * j + k];
            M[3 * i + j] = (float)acc;
        }
    mat3_mul_small(M, vt, R2);
    if (ini_det3(R2) < 0) for (int k = 0; k < 9; ++k) R2[k] = R2[k] * -1.0f + 0.0f;
    for (int h = 0; h < 4; ++h) {
        for (int k = 0; k < 9; ++k) Rs[9 * h + k] = (h & 1) ? R2[k] : R1[k];
        for (int k = 0; k < 3; ++k) ts[3 * h + k] = h < 2 ? t[k] : t[k] * -1.0f + 0.0f;
    }
    return flags;
}

// what ReconstructF decides from the four counts (:499-569).  cosv[h]: C.35's cosine of hypothesis h; cos_gt: C.34's threshold of `parallax >
// minParallax`; zero_gt: 0 > minParallax.  N: the set flags.  Returns the chosen hypothesis, or -1.
OLF_HD int ini_decide_f(const int* nGood, const float* cosv, int N, int minTriangulated, float cos_gt, bool zero_gt)
{
    int maxGood = nGood[0];
    for (int h = 1; h < 4; ++h) if (nGood[h] > maxGood) maxGood = nGood[h];
    const int n09 = (int)(0.9 * N);
    const int nMinGood = n09 > minTriangulated ? n09 : minTriangulated;
    int nsimilar = 0;
    for (int h = 0; h < 4; ++h) if ((double)nGood[h] > 0.7 * maxGood) nsimilar++;
    // If there is not a clear winner or not enough triangulated points reject initialization
    if (maxGood < nMinGood || nsimilar > 1) return -1;
    for (int h = 0; h < 4; ++h)
        if (maxGood == nGood[h]) return (nGood[h] > 0 ? cosv[h] <= cos_gt : zero_gt) ? h : -1;
    return -1;
}

// ---- the motion hypotheses of ReconstructH (:584-686): Rs [8][9], ts [8][3].  Returns -1 when the d1 / d2, d2 / d3 gate fails (:597), else
// ini_jacobi_svd's flags.
template <class E>
OLF_HD int ini_hypotheses_h(E& e, const float* H21, const IniCam& K, float* Rs, float* ts)
{
    const float Km[9] = {K.fx, 0.0f, K.cx, 0.0f, K.fy, K.cy, 0.0f, 0.0f, 1.0f};
    float invK[9], M[9], A[9], w[3], U[9], Vt[9];
    inv3_f32(Km, invK);
    mat3_mul_small(invK, H21, M);
    mat3_mul_small(M, Km, A);
    const int flags = ini_svd3(e, A, w, U, Vt);
    const float s = (float)(ini_det3(U) * ini_det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)f_div(d1, d2) < 1.00001 || (double)f_div(d2, d3) < 1.00001) return -1;
    // n'=[x1 0 x3] 4 posibilities e1=e3=1, e1=1 e3=-1, e1=-1 e3=1, e1=e3=-1
    const float aux1 = ini_sqrtf(f_div(d1 * d1 - d2 * d2, d1 * d1 - d3 * d3));
    const float aux3 = ini_sqrtf(f_div(d2 * d2 - d3 * d3, d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    // case d'=d2
    const float aux_stheta = f_div(ini_sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)), (d1 + d3) * d2);
    const float ctheta = f_div(d2 * d2 + d1 * d3, (d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    // case d'=-d2
    const float aux_sphi = f_div(ini_sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)), (d1 - d3) * d2);
    const float cphi = f_div(d1 * d3 - d2 * d2, (d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    for (int h = 0; h < 8; ++h) {
        const int i = h & 3;
        float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, tp[3];
        float scale;
        if (h < 4) {
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            tp[0] = x1[i]; tp[1] = 0.0f; tp[2] = -x3[i];
            scale = d1 - d3;
        } else {
            Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.0f; Rp[6] = sphi[i]; Rp[8] = -cphi;
            tp[0] = x1[i]; tp[1] = 0.0f; tp[2] = x3[i];
            scale = d1 + d3;
        }
        // R = s * U * Rp * Vt: alpha = s on the first plain product, applied in double (C.12)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const float t0 = U[3 * r] * Rp[c] + U[3 * r + 1] * Rp[3 + c] + U[3 * r + 2] * Rp[6 + c];
                M[3 * r + c] = (float)((double)t0 * (double)s);
            }
        mat3_mul_small(M, Vt, Rs + 9 * h);
        for (int k = 0; k < 3; ++k) tp[k] = tp[k] * scale + 0.0f;      // tp *= d1 -+ d3
        float t[3];
        for (int r = 0; r < 3; ++r) t[r] = dot3_small(U + 3 * r, tp);
        const float inv = recip_f32(norm3(t));
        for (int k = 0; k < 3; ++k) ts[3 * h + k] = t[k] * inv;
    }
    return flags;
}

// what ReconstructH decides from the eight counts (:689-731).  cos_ge: C.34's threshold of `bestParallax >= minParallax`; zero_ge: 0 >= minParallax
// (bestGood > minTriangulated >= 0 makes the best count positive wherever the answer is yes, so zero_ge decides nothing but is kept for the form).
OLF_HD int ini_decide_h(const int* nGood, const float* cosv, int N, int minTriangulated, float cos_ge, bool zero_ge)
{
    int bestGood = 0, secondBestGood = 0, best = -1;
    for (int h = 0; h < 8; ++h) {
        if (nGood[h] > bestGood) { secondBestGood = bestGood; bestGood = nGood[h]; best = h; }
        else if (nGood[h] > secondBestGood) secondBestGood = nGood[h];
    }
    if (best < 0) return -1;                                         // bestParallax = -1 >= minParallax with bestGood = 0 > minTriangulated never holds
    const bool parallax_ok = nGood[best] > 0 ? cosv[best] <= cos_ge : zero_ge;
    if ((double)secondBestGood < 0.75 * bestGood && parallax_ok && bestGood > minTriangulated && (double)bestGood > 0.9 * N) return best;
    return -1;
}

// the degrees of a stored cosine (C.34), host only: what the Python wrapper and the adaptor do with cos_parallax
inline float ini_parallax_degrees(float c) { return (float)((double)(acosf(c) * 180.0f) / 3.1415926535897932384626433832795); }

}  // namespace olf
