// search_math.hpp -- the arithmetic the host searches (search_host.cpp) and the batched device matchers (track_batch.hip, local_batch.hip, bow_match.hip,
// triangulation_batch.hip, fuse_batch.hip, sim3_batch.hip, projection_batch.hip) both run: the cv::Mat products of convention C.12, the rotation histogram
// of ORBmatcher, the gate of SearchForTriangulation, the gates of the two Fuse forms, the transforms and point gate of SearchBySim3 and the point gate of
// the relocalisation SearchByProjection.  One text for both sides; every file that includes it is built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>
#include "device_math.hpp"
#include "../../include/orbline_types.h"

namespace olf {

constexpr int HISTO_LENGTH = 30;                                       // src/ORBmatcher.cc:41

// cv::Mat products of CV_32F operands (convention C.12): a plain product A*b (+ c) of inner length 3 takes cv::gemm's
// small-matrix path (flags == 0, 2 <= len <= 4): the three products are summed in float, alpha and the C term are applied in double and the
// result is rounded once.  Products with a transposed operand (A.t()*b) take the generic path: double accumulation, one rounding.
OLF_HD float dot3_small(const float* a, const float* b)
{
    float t = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];        // ((a0*b0 + a1*b1) + a2*b2) in float, no contraction (-ffp-contract=off)
    return t;
}
// cv::Mat / scalar (convention C.17): a scaling by the double reciprocal rounded to float
OLF_HD float recip_f32(double s) { return (float)d_div(1.0, s); }
// cv::norm of a 3-vector of floats: the squares summed in double, the double root; norm3_f32 and dist3_f32 (cv::norm(a - b), the differences formed
// in float) round it once to the float the reference assigns it to
OLF_HD double norm3(const float* v) { return d_sqrt((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1] + (double)v[2] * (double)v[2]); }
OLF_HD float norm3_f32(const float* v) { return (float)norm3(v); }
OLF_HD float dist3_f32(const float* a, const float* b) { const float d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; return norm3_f32(d); }
OLF_HD void rot_apply(const float* T, const float* v, float alpha_t, float* out)     // R * v + alpha_t * t, T = 4x4 row-major
{
    for (int r = 0; r < 3; ++r) out[r] = (float)((double)dot3_small(T + 4 * r, v) + (double)alpha_t * (double)T[4 * r + 3]);
}
OLF_HD void camera_centre(const float* Tcw, float* Ow)                 // -Rcw.t() * tcw
{
    for (int r = 0; r < 3; ++r) {
        double acc = 0;
        for (int k = 0; k < 3; ++k) acc += (double)Tcw[4 * k + r] * (double)Tcw[4 * k + 3];
        Ow[r] = (float)(-acc);
    }
}

// Frame::UnprojectStereo / KeyFrame::UnprojectStereo (src/Frame.cc:1073-1087, src/KeyFrame.cc:793-809) of a feature with z > 0: x = (u - cx) * z * invfx left
// to right in float, then Rwc * x3Dc + Ow under C.12.  Twc: rows of mRwc | mOw, row-major with a row stride of 4
OLF_HD void unproject_stereo_point(float u, float v, float z, float cx, float cy, float invfx, float invfy, const float* Twc, float* out)
{
    const float x3Dc[3] = {(u - cx) * z * invfx, (v - cy) * z * invfy, z};
    rot_apply(Twc, x3Dc, 1.0f, out);
}

// One endpoint of Frame::isInFrustum_l (src/Frame.cc:456-479, :480-503) -- the first half of Frame::isInFrustum (:394-412): mRcw * p + mtcw under C.12, the
// depth gate, the projection and the CLOSED image bounds.  cam = fx, fy, cx, cy; bounds = mnMinX, mnMaxX, mnMinY, mnMaxY.  false: uv is not written.
// (The point forms, olf_is_in_frustum and k_local_frustum, keep their own spelling of these six lines: they go on to use PcZ's reciprocal for
// mTrackProjXR, and k_local_frustum is held to the instructions it compiled to when it was measured.)
OLF_HD bool project_closed(const float* Tcw, const float* P, const float* cam, const float* bounds, float* uv)
{
    float Pc[3];
    rot_apply(Tcw, P, 1.0f, Pc);
    const float PcX = Pc[0], PcY = Pc[1], PcZ = Pc[2];
    if (PcZ < 0.0f) return false;
    const float invz = f_div(1.0f, PcZ);
    const float u = cam[0] * PcX * invz + cam[2], v = cam[1] * PcY * invz + cam[3];
    if (u < bounds[0] || u > bounds[1]) return false;
    if (v < bounds[2] || v > bounds[3]) return false;
    uv[0] = u; uv[1] = v;
    return true;
}

// The gates of the line trackers (src/Tracking.cc:1324-1344, :995-1015, :2000-2012), literally: the differences are formed in float, widened to double and
// compared with a strict '>'; deltaWidth = (mnMaxX - mnMinX) * frac is a float difference times a double.
OLF_HD bool line_turned(float angle_cur, float angle_last, double delta_angle)
{
    double theta = (double)f_sub(angle_cur, angle_last);
    if (theta < -M_PI) theta += 2 * M_PI;
    else if (theta > M_PI) theta -= 2 * M_PI;
    return fabs(theta) > delta_angle;
}
OLF_HD bool line_moved(const olf_keyline& cur, float sX, float sY, float eX, float eY, double delta_width, double delta_height)
{
    return (double)fabsf(f_sub(cur.startPointX, sX)) > delta_width || (double)fabsf(f_sub(cur.endPointX, eX)) > delta_width ||
           (double)fabsf(f_sub(cur.startPointY, sY)) > delta_height || (double)fabsf(f_sub(cur.endPointY, eY)) > delta_height;
}
// mvDisparity_l[i2].first < 0 || .second < 0 (:1319, :990, :1979): a line without a stereo match takes no map line
OLF_HD bool line_is_mono(const float* ldisp, int i2) { return ldisp[2 * (size_t)i2] < 0 || ldisp[2 * (size_t)i2 + 1] < 0; }

// a frame's FeatureVector as bow_match.hip sorts it, (node << 16 | feature index) ascending: the first position with a[p] >= key
OLF_HD int bm_lower_bound(const unsigned long long* a, int n, unsigned long long key)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}

// The candidate gate of ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:659-825), one text for olf_search_for_triangulation (search_host.cpp) and
// k_search_for_triangulation (triangulation_batch.hip).
// The epipole in the second image (:666-676): C2 = R2w * Cw + t2w under C.12, invz = 1.0f / C2z as one float division, ex = fx * C2x * invz + cx.
OLF_HD void tri_epipole(const float* Tcw2, const float* Cw, float fx, float fy, float cx, float cy, float& ex, float& ey)
{
    float C2[3];
    rot_apply(Tcw2, Cw, 1.0f, C2);
    const float invz = f_div(1.0f, C2[2]);
    ex = fx * C2[0] * invz + cx; ey = fy * C2[1] * invz + cy;
}
// distex * distex + distey * distey < 100 * pKF2->mvScaleFactors[kp2.octave] (:749-755, both features mono): the candidate lies too close to the epipole
OLF_HD bool tri_near_epipole(float ex, float ey, float x2, float y2, float sf)
{
    const float distex = ex - x2, distey = ey - y2;
    return distex * distex + distey * distey < 100 * sf;
}
// ORBmatcher::CheckDistEpipolarLine (:142-161): the line l = x1^T F12 of key point 1 in image 2 (F12 row-major) ...
OLF_HD void tri_epiline(const float* F12, float x1, float y1, float* l)
{
    l[0] = x1 * F12[0] + y1 * F12[3] + F12[6];
    l[1] = x1 * F12[1] + y1 * F12[4] + F12[7];
    l[2] = x1 * F12[2] + y1 * F12[5] + F12[8];
}
// ... and the test of key point 2 against it: den == 0 fails, dsqr = num * num / den in float, dsqr < 3.84 * sigma2 in double, mvLevelSigma2[l] = mvScaleFactor[l]^2
OLF_HD bool tri_epiline_ok(const float* l, float x2, float y2, float sf)
{
    const float num = l[0] * x2 + l[1] * y2 + l[2];
    const float den = l[0] * l[0] + l[1] * l[1];
    if (den == 0) return false;
    const float dsqr = f_div(num * num, den);
    const float sigma2 = sf * sf;
    return dsqr < 3.84 * sigma2;
}

// alpha * R * v (+ t), cv::gemm on a 3x3 R9 (row-major).  transposed: R9 holds the transpose of the matrix the reference multiplies with .t() -> generic path
OLF_HD void r3_apply(const float* R9, const float* v, const float* t3, float* out, double alpha = 1.0, bool transposed = false)
{
    for (int r = 0; r < 3; ++r) {
        double acc = 0;
        if (transposed) for (int k = 0; k < 3; ++k) acc += (double)R9[3 * r + k] * (double)v[k];
        else acc = (double)dot3_small(R9 + 3 * r, v);
        out[r] = (float)(alpha * acc + (t3 ? (double)t3[r] : 0.0));
    }
}

// The search part of the two ORBmatcher::Fuse forms (src/ORBmatcher.cc:827-948, :977-1102), one text for fuse_core (search_host.cpp) and the kernels of
// fuse_batch.hip: the Sim3 decomposition, the gates on a map point, the gates on a key point of its window.
// Decompose Scw (:301-305, :985-989): scw = sqrt(row0 . row0); Rcw = sRcw / scw, tcw = Scw.col(3) / scw (a cv::Mat divided by a scalar is a scaling by
// the double 1/scw rounded to float); Ow = -Rcw.t() * tcw
OLF_HD void sim3_decompose(const float* Scw, float* R, float* t, float* ow)
{
    const float scw = norm3_f32(Scw);
    const float inv = recip_f32((double)scw);
    float Rt[9];
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) { R[3 * r + k] = Scw[4 * r + k] * inv; Rt[3 * k + r] = R[3 * r + k]; } t[r] = Scw[4 * r + 3] * inv; }
    r3_apply(Rt, t, nullptr, ow, -1.0, true);
}
// A map point against a key frame (:855-894, :1011-1050): p3Dc = Rcw * p + tcw (C.12), the depth gate, invz = 1 / z (one rounding to float: the double
// quotient rounded again gives the same float), x = p3Dc[0] * invz, u = fx * x + cx, KeyFrame::IsInImage (HALF-OPEN), ur = u - mbf * invz, the distance
// interval, the 60 degree gate in double.  cam = fx, fy, cx, cy, mbf; bounds = mnMinX, mnMaxX, mnMinY, mnMaxY.  true: uvr = (u, v, ur) and dist3D are
// written; the level is the caller's (predict_scale on the host, fuse_level below on the device).
OLF_HD bool fuse_point_gate(const float* Rcw9, const float* tcw3, const float* Ow3, const float* p3Dw, const float* normal,
                                                         float maxd, float mind, const float* cam, const float* bounds, float* uvr, float& dist3D)
{
    float p3Dc[3];
    r3_apply(Rcw9, p3Dw, tcw3, p3Dc);
    // Depth must be positive
    if (p3Dc[2] < 0.0f) return false;
    const float invz = f_div(1.0f, p3Dc[2]);
    const float x = p3Dc[0] * invz, y = p3Dc[1] * invz;
    const float u = cam[0] * x + cam[2], v = cam[1] * y + cam[3];
    // Point must be inside the image
    if (!(u >= bounds[0] && u < bounds[1] && v >= bounds[2] && v < bounds[3])) return false;
    const float ur = u - cam[4] * invz;
    const float maxDistance = 1.2f * maxd, minDistance = 0.8f * mind;
    float PO[3]; double dot = 0;
    for (int k = 0; k < 3; ++k) { PO[k] = p3Dw[k] - Ow3[k]; dot += (double)PO[k] * (double)normal[k]; }
    dist3D = norm3_f32(PO);
    // Depth must be inside the scale pyramid of the image
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    // Viewing angle must be less than 60 deg
    if (dot < 0.5 * dist3D) return false;
    uvr[0] = u; uvr[1] = v; uvr[2] = ur;
    return true;
}
// MapPoint::PredictScale from the table of olf_predict_scale_thresholds: the number of thresholds <= mfMaxDistance / dist3D
OLF_HD int fuse_level(float maxd, float dist3D, const float* thr, int nlevels)
{
    const float ratio = f_div(maxd, dist3D);
    int lv = 0;
    for (int k = 0; k + 1 < nlevels; ++k) lv += thr[k] <= ratio ? 1 : 0;
    return lv;
}
// the level gate on a key point of the window (:905-908, :1061-1064)
OLF_HD bool fuse_level_ok(int kpLevel, int nPredictedLevel) { return !(kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel); }
// the chi-square gate of the plain form (:910-933): invSigma2 = 1.0f / (sf * sf) (mvInvLevelSigma2, src/ORBextractor.cc:434-436), e2 summed in float left
// to right, the product compared in double; a key point with mvuRight >= 0 -- 0 included -- takes the stereo test.  sf = mvScaleFactors[kpLevel]
OLF_HD bool fuse_chi2_ok(const float* uvr, float kpx, float kpy, float kpur, float sf)
{
    const float sigma2 = sf * sf;
    const float invSigma2 = f_div(1.0f, sigma2);
    const float ex = uvr[0] - kpx, ey = uvr[1] - kpy;
    if (kpur >= 0) {
        // Check reprojection error in stereo
        const float er = uvr[2] - kpur;
        const float e2 = ex * ex + ey * ey + er * er;
        if (e2 * invSigma2 > 7.8) return false;
    } else {
        const float e2 = ex * ex + ey * ey;
        if (e2 * invSigma2 > 5.99) return false;
    }
    return true;
}

// ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1104-1328), one text for olf_search_by_sim3 (search_host.cpp) and the kernels of sim3_batch.hip.
// Transformation between cameras (:1121-1123): sR12 = s12 * R12; sR21 = (1.0 / s12) * R12.t() -- the double reciprocal rounded to float scales the
// transpose; t21 = -sR21 * t12 (a plain product, cv::gemm's small-matrix path, alpha = -1 applied in double).  All row-major.
OLF_HD void sim3_pair_transforms(float s12, const float* R12, const float* t12, float* sR12, float* sR21, float* t21)
{
    const float inv = recip_f32((double)s12);
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) { sR12[3 * r + k] = s12 * R12[3 * r + k]; sR21[3 * r + k] = inv * R12[3 * k + r]; }
    r3_apply(sR21, t12, nullptr, t21, -1.0);
}
// A map point of the source key frame against the other one (:1160-1185, :1240-1265): p3Dc1 = Rsw * p3Dw + tsw (C.12), p3Dc2 = sR * p3Dc1 + t, the depth
// gate (z == 0 fails through the infinite quotient), invz = 1.0 / z (the double quotient rounded to float), x = p3Dc2[0] * invz, u = fx * x + cx,
// KeyFrame::IsInImage (HALF-OPEN), dist3D = cv::norm(p3Dc2) (a double sum, its double root, one rounding), the CLOSED distance interval.
// Tsw = the source key frame's 4 x 4 pose; cam = fx, fy, cx, cy; bounds = mnMinX, mnMaxX, mnMinY, mnMaxY.  true: uv = (u, v) and dist3D are written;
// the level is the caller's (predict_scale on the host, fuse_level on the device).
OLF_HD bool sim3_point_gate(const float* Tsw, const float* p3Dw, const float* sR9, const float* t3, float maxd, float mind,
                                                         const float* cam, const float* bounds, float* uv, float& dist3D)
{
    float pa[3], pb[3];
    rot_apply(Tsw, p3Dw, 1.0f, pa);
    r3_apply(sR9, pa, t3, pb);
    // Depth must be positive
    if (pb[2] < 0.0f) return false;
    const float invz = (float)d_div(1.0, (double)pb[2]);
    const float x = pb[0] * invz, y = pb[1] * invz;
    const float u = cam[0] * x + cam[2], v = cam[1] * y + cam[3];
    // Point must be inside the image
    if (!(u >= bounds[0] && u < bounds[1] && v >= bounds[2] && v < bounds[3])) return false;
    const float maxDistance = 1.2f * maxd, minDistance = 0.8f * mind;
    dist3D = norm3_f32(pb);
    // Depth must be inside the scale invariance region
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    uv[0] = u; uv[1] = v;
    return true;
}

// ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1620-1747), one text for
// olf_search_by_projection_kf (search_host.cpp) and k_proj_gate (projection_batch.hip).  A map point of the key frame against the current frame
// (:1651-1677): x3Dc = Rcw * x3Dw + tcw (C.12), invzc = 1.0 / z (the double quotient rounded to float) WITH NO SIGN TEST -- the reference has none, so a
// point behind the camera that lands inside the bounds goes on --, u = fx * xc * invzc + cx, the CLOSED image bounds, dist3D = cv::norm(x3Dw - Ow)
// (float differences, a double sum, its double root, one rounding), the CLOSED distance interval.  cam = fx, fy, cx, cy; bounds = mnMinX, mnMaxX,
// mnMinY, mnMaxY; Ow3 = -Rcw.t() * tcw (camera_centre).  true: uv = (u, v) and dist3D are written; the level is the caller's (predict_scale on the
// host, fuse_level on the device).
OLF_HD bool reloc_point_gate(const float* Tcw, const float* Ow3, const float* x3Dw, float maxd, float mind, const float* cam,
                                                          const float* bounds, float* uv, float& dist3D)
{
    float x3Dc[3];
    rot_apply(Tcw, x3Dw, 1.0f, x3Dc);
    const float xc = x3Dc[0], yc = x3Dc[1];
    const float invzc = (float)d_div(1.0, (double)x3Dc[2]);
    const float u = cam[0] * xc * invzc + cam[2], v = cam[1] * yc * invzc + cam[3];
    if (u < bounds[0] || u > bounds[1]) return false;
    if (v < bounds[2] || v > bounds[3]) return false;
    // Compute predicted scale level
    dist3D = dist3_f32(x3Dw, Ow3);
    const float maxDistance = 1.2f * maxd, minDistance = 0.8f * mind;
    // Depth must be inside the scale pyramid of the image
    if (dist3D < minDistance || dist3D > maxDistance) return false;
    uv[0] = u; uv[1] = v;
    return true;
}

// the rotation bin of a match (src/ORBmatcher.cc:1434-1441 and its siblings); angles outside [0, 360) give a bin outside [0, HISTO_LENGTH)
OLF_HD int rot_bin(float angle1, float angle2)
{
    float rot = angle1 - angle2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / HISTO_LENGTH));
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// ORBmatcher::ComputeThreeMaxima, src/ORBmatcher.cc:1749-1790, on the sizes of the HISTO_LENGTH bins
OLF_HD void three_maxima(const int* counts, int& ind1, int& ind2, int& ind3)
{
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = counts[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if (max3 < 0.1f * (float)max1) i3 = -1;
    ind1 = i1; ind2 = i2; ind3 = i3;
}

}  // namespace olf
