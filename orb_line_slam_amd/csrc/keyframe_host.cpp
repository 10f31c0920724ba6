// keyframe_host.cpp -- the host forms of keyframe_batch.hip: olf_stereo_landmarks (Tracking::StereoInitialization, CreateNewKeyFrame and UpdateLastFrame,
// src/Tracking.cc:639-677, :1744-1865, :1092-1204) and olf_need_new_keyframe (Tracking::NeedNewKeyFrame, :1606-1725).  Host pointers, no context and no
// device; the arithmetic and the rules are keyframe_terms.hpp, the text the kernels run.  The sort is std::sort on the keys: they are unique, so any correct
// sort gives the reference's order.
#include <algorithm>
#include <string>
#include <vector>
#include "keyframe_terms.hpp"

using namespace olf;

namespace {

// what one half (points or lines) of one frame shares: the walk over the sorted keys and the planes it fills
struct HalfOut {
    int32_t *n_visited, *n_created, *visit_order, *created_order, *frame_out;
    uint8_t* created;
};

// keys: the entries of vDepthIdx, already in visit order; visits the first n_visit of them.  make(i): the geometry of a created feature.
template <class Make>
void walk(const std::vector<unsigned long long>& keys, int n_visit, int mode, const int32_t* held_row, int n_map, const int32_t* nobs, int new_base, int cap,
          const HalfOut& o, int& bits, Make make)
{
    for (int i = 0; i < cap; ++i) { o.visit_order[i] = -1; o.created_order[i] = -1; o.created[i] = 0; o.frame_out[i] = held_row ? held_row[i] : -1; }
    int k = 0;
    for (int q = 0; q < n_visit; ++q) {
        const int i = lm_key_index(keys[q]);
        o.visit_order[q] = i;
        if (!lm_creates(mode, held_row ? held_row[i] : -1, n_map, nobs, bits)) continue;
        o.created_order[k] = i;
        o.created[i] = 1;
        o.frame_out[i] = new_base + k;
        make(i);
        ++k;
    }
    *o.n_visited = n_visit;
    *o.n_created = k;
}

}  // namespace

extern "C" int olf_stereo_landmarks(const olf_landmarks_batch* in, int capacity, int line_capacity, int n_frames, int mode, const float* scale_factors, int n_levels,
                                    const olf_landmarks_outputs* out)
{
    const char* who = "olf_stereo_landmarks";
    const bool ok = lm_args_ok(in, n_frames, mode, out) && capacity >= 0 && line_capacity >= 0 && scale_factors && n_levels >= 1 && n_levels <= OLF_MAX_LEVELS;
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (capacity > OLF_GRID_MAX_KEYS || line_capacity > OLF_GRID_MAX_KEYS) { set_error(std::string(who) + ": more than OLF_GRID_MAX_KEYS features per frame"); return OLF_ERR_CAPACITY; }
    const LandmarkCam K = landmark_cam(in->fx, in->fy, in->cx, in->cy, in->mbf);
    const size_t cap = (size_t)capacity, lcap = (size_t)line_capacity;
    std::vector<unsigned long long> keys;
    for (int j = 0; j < n_frames; ++j) {
        const size_t img = (size_t)j * in->img_stride, row = (size_t)j * cap, lrow = (size_t)j * lcap;
        const float* Twc = in->Twc + 16 * (size_t)j;
        int bits = 0;
        // ---- points
        const int N = np_count(in->counts[img], capacity);
        const olf_keypoint* kps = in->kps + img * cap;
        const float* depth = in->depth + row;
        keys.clear();
        int n_close = 0;
        for (int i = 0; i < N; ++i) if (lm_point_enters(depth[i])) { keys.push_back(lm_key(depth[i], i)); n_close += !(depth[i] > in->thDepth); }
        const bool no_point = keys.empty();
        int n_visit = (int)keys.size();
        if (mode != LM_INIT) { std::sort(keys.begin(), keys.end()); n_visit = lm_prefix(n_visit, n_close, LM_MIN_POINTS); }
        for (size_t i = 0; i < cap; ++i) {
            for (int k = 0; k < 3; ++k) { out->mp_world[3 * (row + i) + k] = 0.f; out->mp_normal[3 * (row + i) + k] = 0.f; }
            out->mp_maxd[row + i] = 0.f; out->mp_mind[row + i] = 0.f;
        }
        const HalfOut po = {out->n_visited + 2 * j, out->n_created + 2 * j, out->visit_order + row, out->created_order + row, out->frame_mp_out + row, out->created + row};
        walk(keys, n_visit, mode, in->frame_mp ? in->frame_mp + row : nullptr, in->n_mp, in->mp_nobs, in->new_base_mp ? in->new_base_mp[j] : in->n_mp, capacity, po, bits,
             [&](int i) {
                 lm_point(mode, kps[i], depth[i], K, Twc, scale_factors, n_levels, out->mp_world + 3 * (row + i), out->mp_normal + 3 * (row + i), out->mp_maxd[row + i],
                          out->mp_mind[row + i], bits);
             });
        // ---- lines
        const int Nl = np_count(in->lcounts[img], line_capacity);
        const olf_keyline* kls = in->kls + img * lcap;
        const float* ldisp = in->ldisp + 2 * lrow;
        keys.clear();
        n_close = 0;
        bool any_nan = false;
        for (int i = 0; i < Nl; ++i) {
            float z; bool nan;
            if (!lm_line_enters(mode, in->mbf, ldisp[2 * i], ldisp[2 * i + 1], z, nan)) continue;
            keys.push_back(lm_key(z, i));
            n_close += !(z > in->thDepth);
            any_nan |= nan;
        }
        n_visit = (int)keys.size();
        if (mode != LM_INIT) { std::sort(keys.begin(), keys.end()); n_visit = lm_prefix(n_visit, n_close, LM_MIN_LINES); }
        if (mode == LM_LASTFRAME && no_point) n_visit = 0;           // :1105-1106: the lines are not looked at
        else if (any_nan) { bits |= LM_ST_NAN_DEPTH; n_visit = 0; }
        for (size_t i = 0; i < 6 * lcap; ++i) { out->ml_world[6 * lrow + i] = 0.f; if (out->ml_world_d) out->ml_world_d[6 * lrow + i] = 0.0; }
        const HalfOut lo = {out->n_visited + 2 * j + 1, out->n_created + 2 * j + 1, out->visit_order_l + lrow, out->created_order_l + lrow, out->frame_ml_out + lrow,
                            out->created_l + lrow};
        walk(keys, n_visit, mode, in->frame_ml ? in->frame_ml + lrow : nullptr, in->n_ml, in->ml_nobs, in->new_base_ml ? in->new_base_ml[j] : in->n_ml, line_capacity, lo,
             bits, [&](int i) {
                 double wd[6];
                 lm_line(kls[i], ldisp[2 * i], ldisp[2 * i + 1], K, Twc, wd, out->ml_world + 6 * (lrow + i));
                 if (out->ml_world_d) for (int k = 0; k < 6; ++k) out->ml_world_d[6 * (lrow + i) + k] = wd[k];
             });
        out->status[j] = bits;
    }
    return OLF_OK;
}

extern "C" int olf_need_new_keyframe(const olf_keyframe_test_batch* in, int capacity, int line_capacity, int n_frames, const olf_keyframe_test_outputs* out)
{
    const char* who = "olf_need_new_keyframe";
    if (!kf_args_ok(in, n_frames, out) || capacity < 0 || line_capacity < 0) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (capacity > OLF_GRID_MAX_KEYS || line_capacity > OLF_GRID_MAX_KEYS) { set_error(std::string(who) + ": more than OLF_GRID_MAX_KEYS features per frame"); return OLF_ERR_CAPACITY; }
    const size_t cap = (size_t)capacity, lcap = (size_t)line_capacity;
    for (int j = 0; j < n_frames; ++j) {
        const size_t img = (size_t)j * in->img_stride, row = (size_t)j * cap, lrow = (size_t)j * lcap;
        const int32_t* r = in->rows + (size_t)KF_ROW * j;
        int cnt[4] = {0, 0, 0, 0}, bits = 0;
        if (!r[KF_MONOCULAR]) {
            const int N = np_count(in->counts[img], capacity), Nl = np_count(in->lcounts[img], line_capacity);
            for (int i = 0; i < N; ++i) {
                const int c = kf_point_class(in->depth[row + i], in->thDepth, in->frame_mp && in->frame_mp[row + i] >= 0, in->outlier && in->outlier[row + i]);
                if (c) ++cnt[c - 1];
            }
            const int lf = in->ldisp_frame ? in->ldisp_frame[j] : j;
            const int Nd = lf >= 0 && lf < n_frames ? np_count(in->lcounts[(size_t)lf * in->img_stride], line_capacity) : 0;
            for (int i = 0; i < Nl; ++i) {
                if (i >= Nd) { bits |= KF_ST_LDISP_RANGE; continue; }
                const float* d = in->ldisp + 2 * ((size_t)lf * lcap + i);
                const int c = kf_line_class(in->mbf, d[0], d[1], in->thDepth, in->frame_ml && in->frame_ml[lrow + i] >= 0, in->outlier_l && in->outlier_l[lrow + i]);
                if (c) ++cnt[1 + c];
            }
        }
        int interrupt, cond;
        const bool need = kf_need_new_keyframe(r, in->n_ref_matches[j], in->n_ref_matches_l[j], in->n_inliers[2 * (size_t)j], in->n_inliers[2 * (size_t)j + 1], cnt, interrupt, cond);
        out->need[j] = need ? 1 : 0;
        out->interrupt_ba[j] = (uint8_t)interrupt;
        for (int k = 0; k < 4; ++k) out->counts[4 * (size_t)j + k] = cnt[k];
        out->conditions[j] = cond;
        out->status[j] = bits;
    }
    return OLF_OK;
}
