// host_geometry.cpp -- the host entries of the C ABI that feed or follow a search but are none themselves and touch no device: the frustum tests
// (olf_is_in_frustum, olf_is_in_frustum_l), the line assignment loops of tracking (olf_local_lines_assign, olf_track_lines_assign), the thresholds of
// MapPoint::PredictScale (olf_predict_scale_thresholds) and the grid walk of a line (olf_line_coords).  They need no context.  The searches themselves are
// in search_host.cpp.  Float expressions are written as the reference writes them (float unless a double literal promotes them); cv::Mat products of
// CV_32F operands accumulate in double and round once; the library is built with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include "../../include/orbline.h"
#include "olf_internal.hpp"
#include "predict_scale.hpp"
#include "search_math.hpp"

using namespace olf;

extern "C" {

int olf_is_in_frustum(const olf_frame_view* f, int n_mp, const float* world, const float* normal, const float* maxd, const float* mind,
                      float viewing_cos_limit, uint8_t* track_in_view, int32_t* track_scale_level, float* track_view_cos, float* track_proj3)
{
    if (!f || !f->Tcw || !f->scale_factors || f->n_levels < 1 || n_mp < 0 ||
        (n_mp && (!world || !normal || !maxd || !mind || !track_in_view || !track_scale_level || !track_view_cos || !track_proj3))) {
        set_error("olf_is_in_frustum: bad argument"); return OLF_ERR_INVALID;
    }
    float Ow[3];
    camera_centre(f->Tcw, Ow);                                   // mOw, Frame::UpdatePoseMatrices (src/Frame.cc:380-386)
    const float logSF = log_scale_factor(f->scale_factors, f->n_levels);
    for (int i = 0; i < n_mp; ++i) {
        track_in_view[i] = 0;
        const float* P = world + 3 * (size_t)i;
        // 3D in camera coordinates
        float Pc[3];
        rot_apply(f->Tcw, P, 1.0f, Pc);
        const float PcX = Pc[0], PcY = Pc[1], PcZ = Pc[2];
        // Check positive depth
        if (PcZ < 0.0f) continue;
        // Project in image and check it is not outside
        const float invz = 1.0f / PcZ;
        const float u = f->fx * PcX * invz + f->cx, v = f->fy * PcY * invz + f->cy;
        if (u < f->minX || u > f->maxX) continue;
        if (v < f->minY || v > f->maxY) continue;
        // Check distance is in the scale invariance region of the MapPoint
        const float maxDistance = 1.2f * maxd[i], minDistance = 0.8f * mind[i];
        float PO[3]; double nrm = 0, dot = 0;
        for (int k = 0; k < 3; ++k) { PO[k] = P[k] - Ow[k]; nrm += (double)PO[k] * (double)PO[k]; dot += (double)PO[k] * (double)normal[3 * (size_t)i + k]; }
        const float dist = (float)std::sqrt(nrm);
        if (dist < minDistance || dist > maxDistance) continue;
        // Check viewing angle
        const float viewCos = (float)(dot / dist);
        if (viewCos < viewing_cos_limit) continue;
        // Predict scale in the image; data used by the tracking
        track_scale_level[i] = predict_scale(maxd[i], dist, logSF, f->n_levels);
        track_in_view[i] = 1;
        track_proj3[3 * (size_t)i] = u; track_proj3[3 * (size_t)i + 1] = v; track_proj3[3 * (size_t)i + 2] = u - f->mbf * invz;
        track_view_cos[i] = viewCos;
    }
    return OLF_OK;
}

// bool Frame::isInFrustum_l(MapLine *pML, float viewingCosLimit), src/Frame.cc:446-515: both end points through project_closed (search_math.hpp), the start
// point first.  mnTrackangle (:512) is read by commented-out code only (src/Tracking.cc:1991-1997) and is not produced.
int olf_is_in_frustum_l(const olf_frame_view* f, int n_ml, const float* world6, uint8_t* in_view, float* proj4)
{
    if (!f || !f->Tcw || n_ml < 0 || (n_ml && (!world6 || !in_view || !proj4))) { set_error("olf_is_in_frustum_l: bad argument"); return OLF_ERR_INVALID; }
    const float cam[4] = {f->fx, f->fy, f->cx, f->cy}, bounds[4] = {f->minX, f->maxX, f->minY, f->maxY};
    for (int i = 0; i < n_ml; ++i) {
        in_view[i] = 0;
        float s[2], e[2];
        if (!project_closed(f->Tcw, world6 + 6 * (size_t)i, cam, bounds, s)) continue;
        if (!project_closed(f->Tcw, world6 + 6 * (size_t)i + 3, cam, bounds, e)) continue;
        in_view[i] = 1;                                       // mbTrackInView; mTrackProjsX, mTrackProjsY, mTrackProjeX, mTrackProjeY
        float* p = proj4 + 4 * (size_t)i;
        p[0] = s[0]; p[1] = s[1]; p[2] = e[0]; p[3] = e[1];
    }
    return OLF_OK;
}

// The loop of Tracking::SearchLocalPointsAndLines over matches_12 (src/Tracking.cc:1974-2016) and n_inliers_ls (:2021-2023) for one frame.
int olf_local_lines_assign(int n_in_view, int32_t* m12, const int32_t* map_index, const float* proj4, const olf_keyline* kls, int n_lines, const float* ldisp,
                           float minX, float maxX, float minY, float maxY, int n_ml, const uint8_t* obs, int32_t* frame_ml, int32_t* n_inliers)
{
    if (n_in_view < 0 || n_lines < 0 || n_ml < 0 || !n_inliers || (n_in_view && (!m12 || !map_index || !proj4 || !obs)) || (n_lines && (!kls || !ldisp || !frame_ml))) {
        set_error("olf_local_lines_assign: bad argument"); return OLF_ERR_INVALID;
    }
    for (int i1 = 0; i1 < n_in_view; ++i1)
        if (m12[i1] >= n_lines || map_index[i1] < 0 || map_index[i1] >= n_ml) { set_error("olf_local_lines_assign: index out of range"); return OLF_ERR_INVALID; }
    for (int i2 = 0; i2 < n_lines; ++i2)
        if (frame_ml[i2] >= n_ml) { set_error("olf_local_lines_assign: a held map line outside the map"); return OLF_ERR_INVALID; }
    const double deltaWidth = (double)(maxX - minX) * 0.1, deltaHeight = (double)(maxY - minY) * 0.1;
    for (int i1 = 0; i1 < n_in_view; ++i1) {
        const int i2 = m12[i1];
        if (i2 < 0) continue;
        if (line_is_mono(ldisp, i2)) continue;
        if (frame_ml[i2] >= 0 && obs[frame_ml[i2]]) continue;               // mvpMapLines[i2]->Observations() > 0, :1981-1983
        const float* p = proj4 + 4 * (size_t)i1;                            // mTrackProjsX, sY, eX, eY of mvpLocalMapLines_InFrustum[i1]
        if (line_moved(kls[i2], p[0], p[1], p[2], p[3], deltaWidth, deltaHeight)) { m12[i1] = -1; continue; }
        frame_ml[i2] = map_index[i1];
    }
    int n = 0;
    for (int i2 = 0; i2 < n_lines; ++i2) n += frame_ml[i2] >= 0 ? 1 : 0;
    *n_inliers = n;
    return OLF_OK;
}

// The frame-to-frame line tracking of Tracking::TrackWithMotionModelWithLine (src/Tracking.cc:1305-1349; skip_null = 1, gates = 1, pos_frac = 0.1) and
// of TrackReferenceKeyFrameWithLine (:976-1020; skip_null = 0, gates = 0: `if(false)`, 0.3 unused) behind match(): the fill with NULL, the loop, n_inliers_ls.
int olf_track_lines_assign(int n_last, int32_t* m12, const olf_keyline* kls_last, const int32_t* last_ml, int n_cur, const olf_keyline* kls_cur,
                           const float* ldisp_cur, float minX, float maxX, float minY, float maxY, int skip_null, int gates, double delta_angle, double pos_frac,
                           int32_t* cur_ml, int32_t* n_inliers)
{
    if (n_last < 0 || n_cur < 0 || !n_inliers || (n_last && (!m12 || !last_ml || (gates && !kls_last))) || (n_cur && (!ldisp_cur || !cur_ml || (gates && !kls_cur)))) {
        set_error("olf_track_lines_assign: bad argument"); return OLF_ERR_INVALID;
    }
    for (int i1 = 0; i1 < n_last; ++i1)
        if (m12[i1] >= n_cur) { set_error("olf_track_lines_assign: index out of range"); return OLF_ERR_INVALID; }
    std::fill(cur_ml, cur_ml + n_cur, -1);
    const double deltaWidth = (double)(maxX - minX) * pos_frac, deltaHeight = (double)(maxY - minY) * pos_frac;
    int n = 0;
    for (int i1 = 0; i1 < n_last; ++i1) {
        if (skip_null && last_ml[i1] < 0) continue;
        const int i2 = m12[i1];
        if (i2 < 0) continue;
        if (line_is_mono(ldisp_cur, i2)) continue;
        if (gates) {
            if (line_turned(kls_cur[i2].angle, kls_last[i1].angle, delta_angle)) { m12[i1] = -1; continue; }
            const olf_keyline& l = kls_last[i1];
            if (line_moved(kls_cur[i2], l.startPointX, l.startPointY, l.endPointX, l.endPointY, deltaWidth, deltaHeight)) { m12[i1] = -1; continue; }
        }
        cur_ml[i2] = last_ml[i1] < 0 ? -1 : last_ml[i1];
        ++n;
    }
    *n_inliers = n;
    return OLF_OK;
}

// The ratios at which predict_scale steps, found on predict_scale itself: thr[k - 1] = the smallest positive float whose level is >= k.  The level is a
// non-decreasing function of the ratio wherever ceil(logf(ratio) / logSF) is (a property of the libm in use, checked around every threshold below), so
// "the number of thresholds <= ratio" is the level.
int olf_predict_scale_thresholds(const float* scale_factors, int n_levels, float* thr)
{
    if (!scale_factors || n_levels < 1 || n_levels > OLF_MAX_LEVELS || (n_levels > 1 && !thr)) { set_error("olf_predict_scale_thresholds: bad argument"); return OLF_ERR_INVALID; }
    const float logSF = log_scale_factor(scale_factors, n_levels);
    if (!(logSF > 0.f)) { set_error("olf_predict_scale_thresholds: the scale factor must exceed 1"); return OLF_ERR_INVALID; }
    auto level = [&](uint32_t bits) { float r; std::memcpy(&r, &bits, 4); return predict_scale(r, 1.0f, logSF, n_levels); };      // (r / 1.0f == r)
    constexpr uint32_t kMinPos = 0x00000001u, kMaxFinite = 0x7f7fffffu, kNear = 4096;
    for (int k = 1; k < n_levels; ++k) {
        uint32_t lo = kMinPos, hi = kMaxFinite;          // positive floats order as their bit patterns do
        if (level(lo) >= k || level(hi) < k) { set_error("olf_predict_scale_thresholds: level " + std::to_string(k) + " has no threshold"); return OLF_ERR_INVALID; }
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (level(mid) >= k) hi = mid; else lo = mid;
        }
        const int below = level(lo), above = level(hi);
        for (uint32_t d = 1; d < kNear; ++d) {
            const bool okLo = lo - kMinPos < d || level(lo - d) == below, okHi = kMaxFinite - hi < d || level(hi + d) == above;
            if (!okLo || !okHi) { set_error("olf_predict_scale_thresholds: the level is not monotone around the threshold of level " + std::to_string(k)); return OLF_ERR_INVALID; }
        }
        std::memcpy(&thr[k - 1], &hi, 4);
    }
    return OLF_OK;
}

// getLineCoords (src/gridStructure.cpp:33-41): the cells visited by the reference's double-precision Bresenham walk (src/LineIterator.cpp:34-77),
// host arithmetic -- the same walk csrc/linematch.hip makes on the device for the stereo line matcher.  xy: (x, y) pairs; *n receives the
// number of cells (which may exceed cap; only cap pairs are written).
int olf_line_coords(double x1, double y1, double x2, double y2, int32_t* xy, int cap, int32_t* n)
{
    if (!xy || !n || cap < 0) { set_error("olf_line_coords: bad argument"); return OLF_ERR_INVALID; }
    const bool steep = std::fabs(y2 - y1) > std::fabs(x2 - x1);
    if (steep) { std::swap(x1, y1); std::swap(x2, y2); }
    if (x1 > x2) { std::swap(x1, x2); std::swap(y1, y2); }
    const double dx = x2 - x1, dy = std::fabs(y2 - y1);
    double error = dx / 2.0;
    const int ystep = (y1 < y2) ? 1 : -1;
    int y = (int)y1, count = 0;
    const int maxX = (int)x2;
    for (int x = (int)x1; x <= maxX; ++x) {
        if (count < cap) { xy[2 * count] = steep ? y : x; xy[2 * count + 1] = steep ? x : y; }
        ++count;
        error -= dy;
        if (error < 0) { y += ystep; error += dx; }
        if (x == 2147483647) break;
    }
    *n = count;
    return OLF_OK;
}

}  // extern "C"
