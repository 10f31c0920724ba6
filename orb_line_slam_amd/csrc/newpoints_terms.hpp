// newpoints_terms.hpp -- the arithmetic the host forms (newpoints_host.cpp) and the kernels (newpoints_batch.hip) of the map-producing entries both run:
// LocalMapping::ComputeF12 (src/LocalMapping.cc:536-553) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:342-383).  One text for both sides; every
// file that includes it is built with -ffp-contract=off (C.4).  The cv::Mat products are those of search_math.hpp (C.12); new here:
//   C.17  cv::Mat / scalar is a scaling by the double reciprocal rounded to float, (float)(1.0 / (double)s) (recip_f32, search_math.hpp): normali / cv::norm(normali) (the norm stays
//         a double: cv::norm returns one) and normal / n (an int, widened)
//   C.18  cv::invert of a 3 x 3 CV_32F matrix is the closed-form adjugate: determinant and cofactors in double, times the double 1 / det, one rounding
//         per element (the float sibling of C.13's form); a zero determinant gives the zero matrix
// Both sit behind the un-vendored OpenCV and are unpinned like C.12.
#pragma once
#include "search_math.hpp"
#include "olf_internal.hpp"

namespace olf {

// C.18
OLF_HD void inv3_f32(const float* s, float* out)
{
    const double m0 = s[0], m1 = s[1], m2 = s[2], m3 = s[3], m4 = s[4], m5 = s[5], m6 = s[6], m7 = s[7], m8 = s[8];
    double d = m0 * (m4 * m8 - m5 * m7) - m1 * (m3 * m8 - m5 * m6) + m2 * (m3 * m7 - m4 * m6);
    if (d == 0.) { for (int k = 0; k < 9; ++k) out[k] = 0.0f; return; }
    d = d_div(1., d);
    out[0] = (float)((m4 * m8 - m5 * m7) * d); out[1] = (float)((m2 * m7 - m1 * m8) * d); out[2] = (float)((m1 * m5 - m2 * m4) * d);
    out[3] = (float)((m5 * m6 - m3 * m8) * d); out[4] = (float)((m0 * m8 - m2 * m6) * d); out[5] = (float)((m2 * m3 - m0 * m5) * d);
    out[6] = (float)((m3 * m7 - m4 * m6) * d); out[7] = (float)((m1 * m6 - m0 * m7) * d); out[8] = (float)((m0 * m4 - m1 * m3) * d);
}

// a plain 3 x 3 product, cv::gemm's small-matrix path (C.12): ((a0 * b0 + a1 * b1) + a2 * b2) in float
OLF_HD void mat3_mul_small(const float* A, const float* B, float* C)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

// LocalMapping::ComputeF12 (:536-553).  T1, T2: the 4 x 4 poses of pKF1 and pKF2, row-major; cam = fx, fy, cx, cy of both (mK); F12 [9] row-major.
//   R12 = R1w * R2w.t()                 a transposed operand: the generic path, double accumulation, one rounding
//   t12 = -R1w * R2w.t() * t2w + t1w    ((-R1w) * R2w.t()) is evaluated first, alpha = -1 applied to the double sum: the negated R12 exactly; then a
//                                       plain product with t1w as the C term (rot_apply's form)
//   K1.t().inv() * t12x * R12 * K2.inv()   left to right, three plain products; the two inverses by C.18
OLF_HD void f12_compute(const float* T1, const float* T2, const float* cam, float* F12)
{
    float R12[9], M[9], t12[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0;
            for (int k = 0; k < 3; ++k) acc += (double)T1[4 * i + k] * (double)T2[4 * j + k];
            R12[3 * i + j] = (float)acc;
            M[3 * i + j] = (float)(-1.0 * acc);
        }
    const float t2w[3] = {T2[3], T2[7], T2[11]};
    for (int i = 0; i < 3; ++i) t12[i] = (float)((double)dot3_small(M + 3 * i, t2w) + (double)T1[4 * i + 3]);
    const float t12x[9] = {0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f};      // SkewSymmetricMatrix, :698-703
    const float K1t[9] = {cam[0], 0.0f, 0.0f, 0.0f, cam[1], 0.0f, cam[2], cam[3], 1.0f};
    const float K2[9] = {cam[0], 0.0f, cam[2], 0.0f, cam[1], cam[3], 0.0f, 0.0f, 1.0f};
    float K1ti[9], K2i[9], A[9], B[9];
    inv3_f32(K1t, K1ti);
    inv3_f32(K2, K2i);
    mat3_mul_small(K1ti, t12x, A);
    mat3_mul_small(A, R12, B);
    mat3_mul_small(B, K2i, F12);
}

// ---- LocalMapping::CreateNewMapPoints, the body after the search (src/LocalMapping.cc:245-253, :286-431) ------------------------------------------------------
// the codes of olf_create_new_map_points*: what became of a match
enum NewPointCode : int {
    NP_NONE = 0, NP_TRIANGULATED = 1, NP_UNPROJECT_1 = 2, NP_UNPROJECT_2 = 3,
    NP_LOW_PARALLAX = 16, NP_W_ZERO = 17, NP_Z1 = 18, NP_Z2 = 19, NP_REPROJ_1 = 20, NP_REPROJ_2 = 21, NP_ZERO_DIST = 22, NP_SCALE_RATIO = 23
};

// The right singular vector of the smallest singular value of a 4 x 4 float matrix, as cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) gives vt.row(3)
// in an OpenCV built without LAPACK (C.19): the one-sided (Hestenes) Jacobi iteration on the transposed matrix -- rows of At are orthogonalised pair by
// pair in cyclic sweeps (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), at most 30 of them, a pair being skipped when |p| <= 2 FLT_EPSILON sqrt(a b); the squared
// norms and the dot product are double sums of float terms, the rotation's c and s are rounded to float, the rotated entries are float products and
// sums; a sweep without a rotation ends the iteration.  The singular values are then ordered descending by a selection that takes the first of equal
// maxima, the rows of V with them.  gamma = hypot(2p, a - b) is spelled sqrt(p p + beta beta) so that host and device run the same operations.  All
// indices are static after unrolling: A, V and W stay in registers on the device.
OLF_HD void jacobi_null4(const float (&A)[4][4], float* v4)
{
    float At[4][4], V[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { At[i][k] = A[k][i]; V[i][k] = i == k ? 1.0f : 0.0f; sd += (double)At[i][k] * (double)At[i][k]; }
        W[i] = sd;
    }
    const float eps = 1.1920928955078125e-7f * 2;                    // FLT_EPSILON * 2
    for (int iter = 0; iter < 30; ++iter) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i + 1; j < 4; ++j) {
                double a = W[i], p = 0, b = W[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) p += (double)At[i][k] * (double)At[j][k];
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
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float t0 = c * At[i][k] + s * At[j][k], t1 = -s * At[i][k] + c * At[j][k];
                    At[i][k] = t0; At[j][k] = t1;
                    a += (double)t0 * (double)t0; b += (double)t1 * (double)t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float t0 = c * V[i][k] + s * V[j][k], t1 = -s * V[i][k] + c * V[j][k];
                    V[i][k] = t0; V[j][k] = t1;
                }
            }
        }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) sd += (double)At[i][k] * (double)At[i][k];
        W[i] = d_sqrt(sd);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                    // position i takes the first maximum of W[i ..]
        int j = i;
        double best = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) if (best < W[k]) { j = k; best = W[k]; }
#pragma unroll
        for (int k = i + 1; k < 4; ++k)
            if (j == k) {
                const double tw = W[i]; W[i] = W[k]; W[k] = tw;
#pragma unroll
                for (int q = 0; q < 4; ++q) { const float tv = V[i][q]; V[i][q] = V[k][q]; V[k][q] = tv; }
            }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) v4[q] = V[3][q];
}

// KeyFrame::SetPose (src/KeyFrame.cc:148-162) of a 4 x 4 pose: Rcw, tcw, and Ow = -Rwc * tcw on the materialised transpose Rwc = Rcw.t(): a plain product
// (cv::gemm's small-matrix path, C.12), alpha = -1 applied to the float sum in double -- not Frame's -mRcw.t() * mtcw (camera_centre)
struct KfPose { float R[9], t[3], Ow[3]; };
OLF_HD void kf_pose(const float* Tcw, KfPose& P)
{
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) P.R[3 * r + k] = Tcw[4 * r + k]; P.t[r] = Tcw[4 * r + 3]; }
    for (int r = 0; r < 3; ++r) {
        const float t0 = P.R[r] * P.t[0] + P.R[3 + r] * P.t[1] + P.R[6 + r] * P.t[2];
        P.Ow[r] = (float)((double)t0 * -1.0);
    }
}
// cv::norm(Ow2 - Ow1) < pKF2->mb, :245-252
OLF_HD bool np_short_baseline(const KfPose& P1, const KfPose& P2, float mb)
{
    return dist3_f32(P2.Ow, P1.Ow) < mb;
}

// the calibration of both key frames as the loop reads it: invfx = 1.0f / fx formed once in float (src/Frame.cc:188-189, copied by the KeyFrame);
// ratio_factor = 1.5f * mfScaleFactor (:232)
struct NewPointCam { float fx, fy, cx, cy, invfx, invfy, mbf, mb, ratio_factor; };
inline NewPointCam new_point_cam(float fx, float fy, float cx, float cy, float mbf, float mb, float scale_factor)
{
    return {fx, fy, cx, cy, 1.0f / fx, 1.0f / fy, mbf, mb, 1.5f * scale_factor};
}
// a frame's key-point count inside [0, cap] whatever it holds
inline int np_count(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:793-809) for a feature with z > 0: Twc.rowRange(0,3).colRange(0,3) * x3Dc + Twc.rowRange(0,3).col(3) with
// Twc = [Rwc | Ow] of kf_pose -- unproject_stereo_point (search_math.hpp), the routine of olf_unproject_stereo_dev, on that Twc
OLF_HD void np_unproject(const KfPose& P, const NewPointCam& K, float u, float v, float z, float* x3D)
{
    float Twc[12];
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) Twc[4 * r + k] = P.R[3 * k + r]; Twc[4 * r + 3] = P.Ow[r]; }
    unproject_stereo_point(u, v, z, K.cx, K.cy, K.invfx, K.invfy, Twc, x3D);
}
// Rcw.row(r).dot(x3Dt) + tcw.at<float>(r) (:354-365): Mat::dot is a double sum, the float is added in double, the assignment rounds once
OLF_HD float np_row_dot(const KfPose& P, int r, const float* x)
{
    double acc = 0;
    for (int k = 0; k < 3; ++k) acc += (double)P.R[3 * r + k] * (double)x[k];
    return (float)(acc + (double)P.t[r]);
}
// the reprojection gate of one key frame (:362-413): true = rejected.  ur >= 0: the stereo form with mpCurrentKeyFrame->mbf for both key frames (:380,
// :406, as written); sigma2 = mvLevelSigma2[octave] = sf * sf in float; the float sum is compared with the double product
OLF_HD bool np_reproj_fails(const KfPose& P, const NewPointCam& K, const float* x3D, float z, float kx, float ky, float ur, float sf)
{
    const float sigmaSquare = sf * sf;
    const float x = np_row_dot(P, 0, x3D), y = np_row_dot(P, 1, x3D);
    const float invz = recip_f32((double)z);
    const float u = K.fx * x * invz + K.cx, v = K.fy * y * invz + K.cy;
    const float errX = u - kx, errY = v - ky;
    if (!(ur >= 0)) return (double)(errX * errX + errY * errY) > 5.991 * (double)sigmaSquare;
    const float u_r = u - K.mbf * invz;
    const float errX_r = u_r - ur;
    return (double)(errX * errX + errY * errY + errX_r * errX_r) > 7.8 * (double)sigmaSquare;
}

// One match of the loop at :286-450: key point 1 (x, y, mvuRight, mvDepth, mvScaleFactors[octave]) of the current key frame P1, key point 2 of the
// neighbour P2.  Returns the code; x3D is written for the codes 1 to 3 (and holds the candidate for the rejections behind it).
//   xn = ((x - cx) * invfx, (y - cy) * invfy, 1); ray = Rwc * xn, a plain product on the materialised transpose (C.12)
//   cosParallaxRays = (float)(ray1.dot(ray2) / (cv::norm(ray1) * cv::norm(ray2))), all of it in double
//   cosParallaxStereo = cos(2 * atan2(mb / 2, depth)): the float overloads (using namespace std), glibc's atan2f and cosf as device_math.hpp restates
//     them for both sides; only compared, never stored
//   A.row(0) = xn1[0] * Tcw1.row(2) - Tcw1.row(0): a float product and a float difference per element; x3D = vt.row(3) / w by C.17
OLF_HD int np_create_point(const KfPose& P1, const KfPose& P2, const NewPointCam& K, float x1, float y1, float ur1, float depth1, float sf1,
                                                        float x2, float y2, float ur2, float depth2, float sf2, float* x3D)
{
    const bool bStereo1 = ur1 >= 0, bStereo2 = ur2 >= 0;
    const float xn1[3] = {(x1 - K.cx) * K.invfx, (y1 - K.cy) * K.invfy, 1.0f};
    const float xn2[3] = {(x2 - K.cx) * K.invfx, (y2 - K.cy) * K.invfy, 1.0f};
    float ray1[3], ray2[3];
    for (int r = 0; r < 3; ++r) {
        ray1[r] = P1.R[r] * xn1[0] + P1.R[3 + r] * xn1[1] + P1.R[6 + r] * xn1[2];
        ray2[r] = P2.R[r] * xn2[0] + P2.R[3 + r] * xn2[1] + P2.R[6 + r] * xn2[2];
    }
    double dot = 0, n1 = 0, n2 = 0;
    for (int k = 0; k < 3; ++k) { dot += (double)ray1[k] * (double)ray2[k]; n1 += (double)ray1[k] * (double)ray1[k]; n2 += (double)ray2[k] * (double)ray2[k]; }
    const float cosParallaxRays = (float)d_div(dot, d_sqrt(n1) * d_sqrt(n2));
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = glibc_cosf(2 * glibc_atan2f(K.mb / 2, depth1));
    else if (bStereo2) cosParallaxStereo2 = glibc_cosf(2 * glibc_atan2f(K.mb / 2, depth2));
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;      // std::min(a, b): b < a ? b : a

    int code;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        float A[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float r2a = k < 3 ? P1.R[6 + k] : P1.t[2], r0a = k < 3 ? P1.R[k] : P1.t[0], r1a = k < 3 ? P1.R[3 + k] : P1.t[1];
            const float r2b = k < 3 ? P2.R[6 + k] : P2.t[2], r0b = k < 3 ? P2.R[k] : P2.t[0], r1b = k < 3 ? P2.R[3 + k] : P2.t[1];
            A[0][k] = xn1[0] * r2a - r0a;
            A[1][k] = xn1[1] * r2a - r1a;
            A[2][k] = xn2[0] * r2b - r0b;
            A[3][k] = xn2[1] * r2b - r1b;
        }
        float v4[4];
        jacobi_null4(A, v4);
        if (v4[3] == 0) return NP_W_ZERO;
        const float inv = recip_f32((double)v4[3]);
        for (int k = 0; k < 3; ++k) x3D[k] = v4[k] * inv;
        code = NP_TRIANGULATED;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        np_unproject(P1, K, x1, y1, depth1, x3D);
        code = NP_UNPROJECT_1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        np_unproject(P2, K, x2, y2, depth2, x3D);
        code = NP_UNPROJECT_2;
    } else
        return NP_LOW_PARALLAX;      // No stereo and very low parallax

    // Check triangulation in front of cameras
    const float z1 = np_row_dot(P1, 2, x3D);
    if (z1 <= 0) return NP_Z1;
    const float z2 = np_row_dot(P2, 2, x3D);
    if (z2 <= 0) return NP_Z2;
    // Check reprojection error
    if (np_reproj_fails(P1, K, x3D, z1, x1, y1, ur1, sf1)) return NP_REPROJ_1;
    if (np_reproj_fails(P2, K, x3D, z2, x2, y2, ur2, sf2)) return NP_REPROJ_2;
    // Check scale consistency
    const float dist1 = dist3_f32(x3D, P1.Ow), dist2 = dist3_f32(x3D, P2.Ow);
    if (dist1 == 0 || dist2 == 0) return NP_ZERO_DIST;
    const float ratioDist = f_div(dist2, dist1);
    const float ratioOctave = f_div(sf1, sf2);
    if (ratioDist * K.ratio_factor < ratioOctave || ratioDist > ratioOctave * K.ratio_factor) return NP_SCALE_RATIO;
    return code;
}

// What MapPoint::UpdateNormalAndDepth reads and writes of a map snapshot (olf_map_graph + olf_cull_view + the three position arrays), device or host
// pointers alike.
struct NormalDepthView {
    int n_kf, n_mp, n_levels;
    const int *obs_off, *obs_kf, *obs_slot, *kmp_off, *ref_kf;
    const uint8_t *mp_bad, *slot_octave;
    const float *world, *Ow;
    float *normal, *maxd, *mind;
    float sf[OLF_MAX_LEVELS];                                        // mvScaleFactors
};

// MapPoint::UpdateNormalAndDepth (:342-383) of point p.  The normal is summed over the observation row in row order, sequentially in float (:362-369;
// std::map<KeyFrame*, size_t> iterates in address order: C.15 is rows ascending, the caller's choice); normali / cv::norm(normali) and normal / n by
// C.17.  The level is the octave at the slot observations[pRefKF] (:373): the row's entry that names the reference key frame, or -- when none does --
// slot 0, which std::map::operator[] inserts.  A bad point (:350) or an empty row (:357) leaves the point untouched.
// Malformed input is left out, never dereferenced: an observation whose key frame is outside [0, n_kf) or whose slot is outside that key frame's row
// (bit 4096) does not enter the sum, n or the search for the reference's slot; a point none of whose observations is left counts as an empty row.  A
// reference key frame outside [0, n_kf) or the slot read for the level outside the reference's row (4096), or a level outside [0, n_levels) (256),
// leaves the point untouched; so does a point index outside [0, n_mp) (512).
OLF_HD void normal_depth_point(const NormalDepthView& a, int p, int* status)
{
    if ((unsigned)p >= (unsigned)a.n_mp) { status_raise(status, STATUS_POINT_INDEX); return; }
    if (a.mp_bad[p]) return;
    int b, e;
    csr_row(a.obs_off, a.n_mp, p, b, e);
    if (b == e) return;
    const int ref = a.ref_kf[p];
    if ((unsigned)ref >= (unsigned)a.n_kf) { status_raise(status, STATUS_KF_INDEX); return; }
    const float P[3] = {a.world[3 * (size_t)p], a.world[3 * (size_t)p + 1], a.world[3 * (size_t)p + 2]};
    float nv[3] = {0.0f, 0.0f, 0.0f};
    int n = 0, ref_slot = 0;
    bool named = false;
    for (int o = b; o < e; ++o) {
        const int kf = a.obs_kf[o], slot = a.obs_slot[o];
        if ((unsigned)kf >= (unsigned)a.n_kf) { status_raise(status, STATUS_KF_INDEX); continue; }
        int rb, re;
        csr_row(a.kmp_off, a.n_kf, kf, rb, re);
        if ((unsigned)slot >= (unsigned)(re - rb)) { status_raise(status, STATUS_KF_INDEX); continue; }
        if (kf == ref && !named) { named = true; ref_slot = slot; }
        float d[3];
        for (int k = 0; k < 3; ++k) d[k] = P[k] - a.Ow[3 * (size_t)kf + k];
        const float inv = recip_f32(norm3(d));
        for (int k = 0; k < 3; ++k) nv[k] = nv[k] + d[k] * inv;
        ++n;
    }
    if (n == 0) return;
    int rb, re;
    csr_row(a.kmp_off, a.n_kf, ref, rb, re);
    if ((unsigned)ref_slot >= (unsigned)(re - rb)) { status_raise(status, STATUS_KF_INDEX); return; }
    const int level = a.slot_octave[rb + ref_slot];
    if (level >= a.n_levels) { status_raise(status, STATUS_OCTAVE); return; }
    const float dist = dist3_f32(P, a.Ow + 3 * (size_t)ref);
    const float maxd = dist * a.sf[level];                           // :379
    a.maxd[p] = maxd;
    a.mind[p] = f_div(maxd, a.sf[a.n_levels - 1]);                   // :380
    const float invn = recip_f32((double)n);                         // :381
    for (int k = 0; k < 3; ++k) a.normal[3 * (size_t)p + k] = nv[k] * invn;
}

}  // namespace olf
