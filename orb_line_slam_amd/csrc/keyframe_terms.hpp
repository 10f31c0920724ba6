// keyframe_terms.hpp -- what the host forms (keyframe_host.cpp) and the kernels (keyframe_batch.hip) of the key-frame step both run: the selection of
// Tracking::StereoInitialization (src/Tracking.cc:639-677), CreateNewKeyFrame (:1744-1865) and UpdateLastFrame (:1092-1204), the landmarks they create, and
// the counts and the decision of Tracking::NeedNewKeyFrame (:1606-1725).  One text for both sides; every file that includes it is built with
// -ffp-contract=off (C.4).  The point arithmetic is search_math.hpp (C.12, C.17: the terms newpoints_terms.hpp states); new here:
//   C.29  Frame::backProjection (src/Frame.cc:1089-1098) in double: bd = (double)mb / (double)disp with mb the float mbf / fx as Frame forms it; bd * (u - cx)
//         with the float operands widened; Converter::toMatrix3d(mRwc) * P + Converter::toVector3d(mOw) as an Eigen fixed-size product, summed over k
//         ascending (the convention of pose_terms.hpp), the translation added last; Converter::toCvMat rounds each double to float once.
// It sits behind the un-vendored Eigen and is unpinned like C.12.
#pragma once
#include "newpoints_terms.hpp"
#include "../../include/orbline.h"

namespace olf {

enum { LM_INIT = 0, LM_KEYFRAME = 1, LM_LASTFRAME = 2 };             // OLF_LANDMARKS_*
enum { LM_ST_NAN_DEPTH = 1, LM_ST_HELD_INDEX = 2, LM_ST_OCTAVE = 4 };      // a frame's own status word
constexpr int LM_MIN_POINTS = 100, LM_MIN_LINES = 50;                // `nPoints>100` (:1796, :1142), `nLines>50` (:1862, :1202)
constexpr unsigned long long LM_KEY_PAD = ~0ull;

// pair<float,int>(z, i) under operator< as one unsigned word.  Every z that enters is > 0, +inf, or (lines: mbf / +-inf) a zero of either sign: positive
// floats and +inf order as their bit patterns, and both zeros compare equal, so they share the pattern 0 and the index decides.
OLF_HD unsigned long long lm_key(float z, int i) { return ((unsigned long long)(z == 0 ? 0u : f2bits(z)) << 32) | (unsigned)i; }
OLF_HD int lm_key_index(unsigned long long key) { return (int)(unsigned)(key & 0xffffffffu); }

// a point enters vDepthIdx when z > 0 (:1751-1755, :1098-1102; :642 in INIT mode)
OLF_HD bool lm_point_enters(float z) { return z > 0; }
// a line (:1806-1813, :1149-1156): sz = mbf / disparity in float, `if(sz<0||ez<0) continue; z = sz>ez?sz:ez`.  INIT mode (:657): both disparities > 0,
// and no depth is formed.  nan: the depth that would be sorted is NaN.
OLF_HD bool lm_line_enters(int mode, float mbf, float d0, float d1, float& z, bool& nan)
{
    nan = false; z = 0.f;
    if (mode == LM_INIT) return d0 > 0 && d1 > 0;
    const float sz = f_div(mbf, d0), ez = f_div(mbf, d1);
    if (sz < 0 || ez < 0) return false;
    z = sz > ez ? sz : ez;
    nan = z != z;
    return true;
}
// the entries the walk visits of n sorted ones, n_close of them with !(z > thDepth): it breaks behind the first entry j (0-based) with z > thDepth and
// j + 1 > least, which in ascending order is j = max(n_close, least)
OLF_HD int lm_prefix(int n, int n_close, int least)
{
    const int j = n_close > least ? n_close : least;
    return j + 1 < n ? j + 1 : n;
}
// does a visited feature get a new landmark (:1769-1776, :1119-1125)?  held: its entry of mvpMapPoints / mvpMapLines; an index outside the map counts as
// NULL and raises bit 2.  INIT mode creates without looking.
OLF_HD bool lm_creates(int mode, int held, int n_map, const int* __restrict__ nobs, int& bits)
{
    if (mode == LM_INIT || held < 0) return true;
    if (held >= n_map) { bits |= LM_ST_HELD_INDEX; return true; }
    return nobs[held] < 1;
}

struct LandmarkCam { float cx, cy, invfx, invfy, fx, mb; };
// invfx = 1.0f / fx (src/Frame.cc:188-189), mb = mbf / fx (:191), both in float
inline LandmarkCam landmark_cam(float fx, float fy, float cx, float cy, float mbf) { return {cx, cy, 1.0f / fx, 1.0f / fy, fx, mbf / fx}; }

// A created point: x3D = Frame::UnprojectStereo (unproject_stereo_point, the routine of olf_unproject_stereo_dev); then with Ow = column 3 of Twc
//   LASTFRAME   MapPoint(Pos, pMap, pFrame, idxF) (src/MapPoint.cc:64-76): mNormalVector = (Pos - Ow) / cv::norm(.) (C.17)
//   otherwise   UpdateNormalAndDepth (:342-383) with the one observation: normal = zeros + normali / cv::norm(normali), then / n with n = 1 -- the sum
//               turns a -0 component into +0, the constructor keeps it
// dist = (float)cv::norm(Pos - Ow); mfMaxDistance = dist * mvScaleFactors[level]; mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1].  A level
// outside [0, n_levels) raises bit 4 and gives 0 for both.
OLF_HD void lm_point(int mode, const olf_keypoint& kp, float z, const LandmarkCam& K, const float* Twc, const float* sf, int n_levels, float* world, float* normal,
                     float& maxd, float& mind, int& bits)
{
    unproject_stereo_point(kp.x, kp.y, z, K.cx, K.cy, K.invfx, K.invfy, Twc, world);
    const float Ow[3] = {Twc[3], Twc[7], Twc[11]};
    float d[3];
    for (int k = 0; k < 3; ++k) d[k] = world[k] - Ow[k];
    const float inv = recip_f32(norm3(d));
    if (mode == LM_LASTFRAME) for (int k = 0; k < 3; ++k) normal[k] = d[k] * inv;
    else {
        const float invn = recip_f32(1.0);
        for (int k = 0; k < 3; ++k) normal[k] = (0.0f + d[k] * inv) * invn;
    }
    maxd = 0.f; mind = 0.f;
    if ((unsigned)kp.octave >= (unsigned)n_levels) { bits |= LM_ST_OCTAVE; return; }
    const float dist = dist3_f32(world, Ow);
    maxd = dist * sf[kp.octave];
    mind = f_div(maxd, sf[n_levels - 1]);
}

// C.29: one endpoint
OLF_HD void lm_back_projection(float u, float v, float disp, const LandmarkCam& K, const float* Twc, double* out)
{
    const double bd = d_div((double)K.mb, (double)disp);
    const double P[3] = {bd * ((double)u - (double)K.cx), bd * ((double)v - (double)K.cy), bd * (double)K.fx};
    for (int r = 0; r < 3; ++r) {
        double acc = (double)Twc[4 * r] * P[0];
        acc = acc + (double)Twc[4 * r + 1] * P[1];
        acc = acc + (double)Twc[4 * r + 2] * P[2];
        out[r] = acc + (double)Twc[4 * r + 3];
    }
}
// a created line: both endpoints in double, and their float copies
OLF_HD void lm_line(const olf_keyline& kl, float d0, float d1, const LandmarkCam& K, const float* Twc, double* wd, float* wf)
{
    lm_back_projection(kl.startPointX, kl.startPointY, d0, K, Twc, wd);
    lm_back_projection(kl.endPointX, kl.endPointY, d1, K, Twc, wd + 3);
    for (int k = 0; k < 6; ++k) wf[k] = (float)wd[k];
}

// ---- Tracking::NeedNewKeyFrame --------------------------------------------------------------------------------------------------------------------------
enum { KF_ID, KF_LAST_KF_ID, KF_LAST_RELOC_ID, KF_MIN_FRAMES, KF_MAX_FRAMES, KF_NKFS, KF_IDLE, KF_QUEUE, KF_ONLY_TRACKING, KF_STOPPED, KF_MONOCULAR, KF_ROW };
enum { KF_ST_LDISP_RANGE = 1 };
// :1641-1647: 0 none, 1 tracked, 2 not tracked
OLF_HD int kf_point_class(float z, float thDepth, bool held, bool outlier)
{
    if (!(z > 0 && z < thDepth)) return 0;
    return held && !outlier ? 1 : 2;
}
// :1651-1665
OLF_HD int kf_line_class(float mbf, float d0, float d1, float thDepth, bool held, bool outlier)
{
    float minz = f_div(mbf, d0), maxz = f_div(mbf, d1);
    if (minz > maxz) { const float tmp = minz; minz = maxz; maxz = tmp; }
    if (!(minz > 0 && maxz < thDepth)) return 0;
    return held && !outlier ? 1 : 2;
}
// :1609-1724 behind the counts, in the reference's types: mCurrentFrame.mnId is a long unsigned, mnLastKeyFrameId and mnLastRelocFrameId are unsigned and
// their sum with the int mMaxFrames / mMinFrames wraps at 32 bits before it is widened; nKFs, the match counts and the queue length are int; the 0.25
// comparisons are int against double, the thRefRatio ones int against float.  cnt = nTrackedClose, nNonTrackedClose, nTrackedClose_l, nNonTrackedClose_l.
// Returns the decision; interrupt: mpLocalMapper->InterruptBA() was called (:1711); cond: the six conditions, 0 when an early return came first.
OLF_HD bool kf_need_new_keyframe(const int* __restrict__ row, int nRefMatches, int nRefMatches_l, int mnMatchesInliers, int mnMatchesInliers_l, const int* cnt,
                                 int& interrupt, int& cond)
{
    interrupt = 0; cond = 0;
    const bool monocular = row[KF_MONOCULAR] != 0;
    if (row[KF_ONLY_TRACKING]) return false;
    if (row[KF_STOPPED]) return false;
    const int nKFs = row[KF_NKFS], mMaxFrames = row[KF_MAX_FRAMES], mMinFrames = row[KF_MIN_FRAMES];
    const unsigned long long mnId = (unsigned long long)(unsigned)row[KF_ID];
    const unsigned mnLastKeyFrameId = (unsigned)row[KF_LAST_KF_ID], mnLastRelocFrameId = (unsigned)row[KF_LAST_RELOC_ID];
    if (mnId < (unsigned long long)(mnLastRelocFrameId + (unsigned)mMaxFrames) && nKFs > mMaxFrames) return false;
    const bool bLocalMappingIdle = row[KF_IDLE] != 0;
    const bool bNeedToInsertClose = (cnt[0] < 100) && (cnt[1] > 70);
    const bool bNeedToInsertClose_l = (cnt[2] < 20) && (cnt[3] > 100);
    float thRefRatio = 0.75f, thRefRatio_l = 0.75f;
    if (nKFs < 2) { thRefRatio = 0.4f; thRefRatio_l = 0.4f; }
    if (monocular) thRefRatio = 0.9f;
    const bool c1a = mnId >= (unsigned long long)(mnLastKeyFrameId + (unsigned)mMaxFrames);
    const bool c1b = mnId >= (unsigned long long)(mnLastKeyFrameId + (unsigned)mMinFrames) && bLocalMappingIdle;
    const bool c1c = !monocular && ((double)mnMatchesInliers < (double)nRefMatches * 0.25 || bNeedToInsertClose);
    const bool c1c_l = !monocular && ((double)mnMatchesInliers_l < (double)nRefMatches_l * 0.25 || bNeedToInsertClose_l);
    const bool c2 = ((float)mnMatchesInliers < (float)nRefMatches * thRefRatio || bNeedToInsertClose) && mnMatchesInliers > 15;
    const bool c2_l = ((float)mnMatchesInliers_l < (float)nRefMatches_l * thRefRatio_l || bNeedToInsertClose_l) && mnMatchesInliers_l > 10;
    cond = (int)c1a | (int)c1b << 1 | (int)c1c << 2 | (int)c1c_l << 3 | (int)c2 << 4 | (int)c2_l << 5;
    if ((c1a || c1b || c1c || c1c_l) && (c2 || c2_l)) {
        if (bLocalMappingIdle) return true;
        interrupt = 1;
        if (!monocular) return row[KF_QUEUE] < 3;
        return false;
    }
    return false;
}

// the checks both forms of each entry make of their caller's structs
inline bool lm_args_ok(const olf_landmarks_batch* in, int n_frames, int mode, const olf_landmarks_outputs* o)
{
    bool ok = in && o && n_frames >= 0 && mode >= LM_INIT && mode <= LM_LASTFRAME && in->img_stride >= 1 && in->n_mp >= 0 && in->n_ml >= 0;
    ok = ok && in->kps && in->counts && in->kls && in->lcounts && in->depth && in->ldisp && in->Twc;
    ok = ok && (!in->frame_mp || !in->n_mp || in->mp_nobs) && (!in->frame_ml || !in->n_ml || in->ml_nobs);
    ok = ok && o->n_visited && o->n_created && o->visit_order && o->visit_order_l && o->created_order && o->created_order_l && o->created && o->created_l;
    return ok && o->frame_mp_out && o->frame_ml_out && o->mp_world && o->mp_normal && o->mp_maxd && o->mp_mind && o->ml_world && o->status;
}
inline bool kf_args_ok(const olf_keyframe_test_batch* in, int n_frames, const olf_keyframe_test_outputs* o)
{
    bool ok = in && o && n_frames >= 0 && in->img_stride >= 1 && in->counts && in->lcounts && in->depth && in->ldisp && in->rows;
    ok = ok && in->n_ref_matches && in->n_ref_matches_l && in->n_inliers;
    return ok && o->need && o->interrupt_ba && o->counts && o->conditions && o->status;
}

}  // namespace olf
