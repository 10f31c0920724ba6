// search_host.cpp -- host side of the ORBmatcher searches behind the C ABI, and nothing else: the every-frame ones (olf_search_by_projection[_match12],
// olf_search_for_initialization, olf_search_by_bow, olf_search_local_map) and the relocalisation / LocalMapping / LoopClosing ones
// (olf_search_by_projection_kf, olf_search_by_bow_kf, olf_search_for_triangulation, olf_fuse_search, olf_fuse_search_sim3,
// olf_search_by_projection_sim3, olf_search_by_sim3).  The host entries that feed them without searching (olf_is_in_frustum and its kin) are in
// host_geometry.cpp.  Split of the reference's loops, as SURVEY 8(b) / App. C.7 prescribe:
//   1. candidate generation on the host, exactly as the reference walks them (Frame::GetFeaturesInArea over the 64 x 48 grid,
//      src/Frame.cc:517-570; the merge of two DBoW2 feature vectors, src/ORBmatcher.cc:176-203),
//   2. every DescriptorDistance of the search in one k_match_candidates launch (match.hip),
//   3. the reference's greedy resolution, which depends on the map points assigned so far, on the host in the reference's order.
// What the searches share is stated once at the top: Grid (1), bow_queries (1), Batch (2), RotHist (the rejection that ends 3) and the argument tests.
// Map mutations (MapPoint::Replace / AddObservation in the Fuse functions) stay with the caller: they never feed back into a search.
// Float expressions are written as the reference writes them (src/ORBmatcher.cc, float unless a double literal promotes them); cv::Mat
// products of CV_32F operands accumulate in double and round once; the library is built with -ffp-contract=off.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/orbline.h"
#include "olf_internal.hpp"
#include "predict_scale.hpp"
#include "search_math.hpp"

namespace {
using namespace olf;
constexpr int TH_HIGH = 100, TH_LOW = 50;                             // src/ORBmatcher.cc:39-40 (HISTO_LENGTH: search_math.hpp)
constexpr int GRID_COLS = OLF_GRID_COLS, GRID_ROWS = OLF_GRID_ROWS;      // FRAME_GRID_COLS / FRAME_GRID_ROWS, include/Frame.h:51-52

// Frame::mGrid (src/Frame.cc:334-349) as one index array (layout: include/orbline_types.h): the features of cell (ix, iy) are
// item[cell[ix * GRID_ROWS + iy]] .. [+1), in feature order -- the order push_back gives them in the reference.  A view that carries a prebuilt grid
// (grid_offsets / grid_index, e.g. from olf_frame_grid) is walked as it is once checked (ok == false: the search returns OLF_ERR_INVALID); otherwise the
// grid is built here from the key points.
struct Grid {
    const olf_frame_view& f;
    float wInv, hInv;
    std::vector<int> built_cell, built_item;
    const int32_t* cell;
    const int32_t* item;
    bool ok = true;
    explicit Grid(const olf_frame_view& fr) : f(fr)
    {
        wInv = static_cast<float>(GRID_COLS) / (f.maxX - f.minX);      // mfGridElementWidthInv, src/Frame.cc:186-187
        hInv = static_cast<float>(GRID_ROWS) / (f.maxY - f.minY);
        if (f.grid_offsets || f.grid_index) {
            cell = f.grid_offsets; item = f.grid_index;
            ok = grid_is_valid(cell, item, f.n);
            return;
        }
        std::vector<int> where((size_t)std::max(f.n, 0));
        built_cell.assign(GRID_COLS * GRID_ROWS + 1, 0);
        for (int i = 0; i < f.n; ++i) {                                 // PosInGrid, src/Frame.cc:572-582
            const int posX = (int)std::round((f.keys[i].x - f.minX) * wInv), posY = (int)std::round((f.keys[i].y - f.minY) * hInv);
            where[i] = (posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS) ? -1 : posX * GRID_ROWS + posY;
            if (where[i] >= 0) ++built_cell[where[i] + 1];
        }
        for (int c = 0; c < GRID_COLS * GRID_ROWS; ++c) built_cell[c + 1] += built_cell[c];
        built_item.resize(built_cell.back());
        std::vector<int> fill(built_cell.begin(), built_cell.end() - 1);
        for (int i = 0; i < f.n; ++i) if (where[i] >= 0) built_item[fill[where[i]]++] = i;
        cell = built_cell.data(); item = built_item.data();
    }
    // Frame::GetFeaturesInArea: appends the indices to `out`, returns how many
    int area(float x, float y, float r, int minLevel, int maxLevel, std::vector<int>& out) const
    {
        const int nMinCellX = std::max(0, (int)std::floor((x - f.minX - r) * wInv));
        if (nMinCellX >= GRID_COLS) return 0;
        const int nMaxCellX = std::min(GRID_COLS - 1, (int)std::ceil((x - f.minX + r) * wInv));
        if (nMaxCellX < 0) return 0;
        const int nMinCellY = std::max(0, (int)std::floor((y - f.minY - r) * hInv));
        if (nMinCellY >= GRID_ROWS) return 0;
        const int nMaxCellY = std::min(GRID_ROWS - 1, (int)std::ceil((y - f.minY + r) * hInv));
        if (nMaxCellY < 0) return 0;
        const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
        const size_t before = out.size();
        for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
            // the cells (ix, nMinCellY .. nMaxCellY) are adjacent in `cell`
            for (int p = cell[ix * GRID_ROWS + nMinCellY]; p < cell[ix * GRID_ROWS + nMaxCellY + 1]; ++p) {
                const int j = item[p];
                const olf_keypoint& kp = f.keys[j];
                if (bCheckLevels) {
                    if (kp.octave < minLevel) continue;
                    if (maxLevel >= 0 && kp.octave > maxLevel) continue;
                }
                const float distx = kp.x - x, disty = kp.y - y;
                if (std::fabs(distx) < r && std::fabs(disty) < r) out.push_back(j);
            }
        }
        return (int)(out.size() - before);
    }
};

// the queries of one search: descriptor rows gathered contiguously, CSR candidate lists, distances from the GPU
struct Batch {
    std::vector<uint8_t> descQ;
    std::vector<int> offs{0}, cand, owner;
    std::vector<uint16_t> dist;
    void add(int who, const uint8_t* d) { owner.push_back(who); descQ.insert(descQ.end(), d, d + 32); offs.push_back((int)cand.size()); }
    int run(olf_ctx* c, const uint8_t* descT, int nT)
    {
        dist.assign(cand.size(), 0);
        if (owner.empty() || cand.empty()) return OLF_OK;
        return olf_match_candidates(c, descQ.data(), (int)owner.size(), descT, nT, offs.data(), cand.data(), dist.data());
    }
};

// The reference's rotHist (src/ORBmatcher.cc:1434-1441 and its siblings): the matches of a search by rotation bin, and the rejection that ends the
// search -- every match outside the three fullest bins (ORBmatcher::ComputeThreeMaxima on the sizes of the vectors) is undone, bin by bin and within a
// bin in the order the matches were made; `undo` takes one index and does the search's own reset.
struct RotHist {
    std::vector<int> rotHist[HISTO_LENGTH];
    void add(float angle1, float angle2, int idx) { rotHist[rot_bin(angle1, angle2)].push_back(idx); }
    template <class Undo>
    void reject(int check_orientation, Undo&& undo) const
    {
        if (!check_orientation) return;
        int counts[HISTO_LENGTH], ind1, ind2, ind3;
        for (int i = 0; i < HISTO_LENGTH; i++) counts[i] = (int)rotHist[i].size();
        three_maxima(counts, ind1, ind2, ind3);
        for (int b = 0; b < HISTO_LENGTH; b++) {
            if (b == ind1 || b == ind2 || b == ind3) continue;
            for (int idx : rotHist[b]) undo(idx);
        }
    }
};

// merge of two DBoW2 feature vectors: calls f(a, b) for every node present in both; the two ordered maps are walked in step (:176-203, :537-543, :683-689)
template <class F>
void for_common_nodes(const olf_frame_view& A, const olf_frame_view& B, F&& f)
{
    int a = 0, b = 0;
    while (a < A.fv_n && b < B.fv_n) {
        if (A.fv_nodes[a] == B.fv_nodes[b]) { f(a, b); ++a; ++b; }
        else if (A.fv_nodes[a] < B.fv_nodes[b]) ++a;
        else ++b;
    }
}

// The queries of the three searches that walk two feature vectors: every feature of A under a common node that `eligible` lets through, against all of
// B's features under that node.  false: a feature index of A lies outside A (that feature is left out).
template <class E>
bool bow_queries(const olf_frame_view& A, const olf_frame_view& B, Batch& q, E&& eligible)
{
    bool inside = true;
    for_common_nodes(A, B, [&](int a, int b) {
        for (int p = A.fv_offsets[a]; p < A.fv_offsets[a + 1]; ++p) {
            const int idxA = A.fv_features[p];
            if (idxA < 0 || idxA >= A.n) { inside = false; continue; }
            if (!eligible(idxA)) continue;
            q.cand.insert(q.cand.end(), B.fv_features + B.fv_offsets[b], B.fv_features + B.fv_offsets[b + 1]);
            q.add(idxA, A.desc + 32 * (size_t)idxA);
        }
    });
    return inside;
}
// the candidates are features of B
bool cand_inside(const Batch& q, const olf_frame_view& B)
{
    for (int idxB : q.cand) if (idxB < 0 || idxB >= B.n) return false;
    return true;
}

// (rot_bin; dot3_small, rot_apply, camera_centre -- convention C.12; r3_apply; sim3_decompose, sim3_pair_transforms, sim3_point_gate: search_math.hpp)
// (predict_scale: predict_scale.hpp)
float log_scale_factor(const olf_frame_view& f) { return olf::log_scale_factor(f.scale_factors, f.n_levels); }

// ---- the argument tests --------------------------------------------------------------------------------------------------------------------------
int bad_grid() { set_error("the view's grid_offsets / grid_index do not describe its n features (orbline_types.h: Frame::mGrid as two arrays)"); return OLF_ERR_INVALID; }
bool bad_view(const olf_frame_view* f, bool needs_pose)
{
    return !f || f->n < 0 || (f->n && (!f->keys || !f->desc)) || (needs_pose && !f->Tcw);
}
// views whose scale tables are indexed by a predicted pyramid level (MapPoint::PredictScale) or by a key point's octave
bool bad_levels(const olf_frame_view* f) { return f->n_levels < 1 || f->n_levels > OLF_MAX_LEVELS || !f->scale_factors; }
// a feature vector that is named but not there; and one that is that or has a negative length
bool fv_missing(const olf_frame_view* v) { return v->fv_n && (!v->fv_nodes || !v->fv_offsets || !v->fv_features); }
bool bad_fv(const olf_frame_view* v) { return v->fv_n < 0 || fv_missing(v); }
// the state planes of a key frame whose map points are projected: mp_valid, mp_bad and the points' position, descriptor and distance range
bool bad_kf_points(const olf_frame_view* k) { return k->n && (!k->mp_valid || !k->mp_bad || !k->mp_world || !k->mp_desc || !k->mp_maxd || !k->mp_mind); }
// the arrays of a list of map points (the Fuse family)
bool bad_points(int n_mp, const float* world, const float* normal, const float* maxd, const float* mind, const uint8_t* desc)
{
    return n_mp && (!world || !normal || !maxd || !mind || !desc);
}

// Both SearchByProjection(Frame, Frame) overloads: src/ORBmatcher.cc:1330-1472 and, with match12, :1474-1618.  match12 models the reference's
// map<int, int>: match12.insert(pair(bestIdx2, i)) keeps the FIRST last-frame index a current feature was matched with (:1577; a feature whose
// new map point has no observations can be matched again, and mvpMapPoints[bestIdx2] = pMP then keeps the last one), match12.erase(idx) on a
// rotation-histogram rejection (:1612).
int search_by_projection_frames(olf_ctx* c, const olf_frame_view* cur, const olf_frame_view* last, float th, int bMono, int check_orientation,
                                int32_t* matches, int32_t* match12, int32_t* nmatches)
{
    if (!c || bad_view(cur, true) || bad_view(last, true) || !matches || !nmatches || !cur->scale_factors || !cur->mp_valid || !cur->mp_obs ||
        (cur->n && !cur->uright) || (last->n && (!last->mp_valid || !last->mp_world || !last->mp_desc || !last->mp_obs))) {
        set_error("olf_search_by_projection: bad argument"); return OLF_ERR_INVALID;
    }
    for (int i = 0; i < cur->n; ++i) matches[i] = -1;
    if (match12) for (int i = 0; i < cur->n; ++i) match12[i] = -1;
    *nmatches = 0;
    const float mb = cur->mbf / cur->fx;
    // twc = -Rcw.t() * tcw;  tlc = Rlw * twc + tlw                                   (:1341-1349)
    float twc[3], tlc[3];
    camera_centre(cur->Tcw, twc);
    rot_apply(last->Tcw, twc, 1.0f, tlc);
    const bool bForward = tlc[2] > mb && !bMono, bBackward = -tlc[2] > mb && !bMono;

    const Grid grid(*cur);
    if (!grid.ok) return bad_grid();
    Batch q;
    struct Meta { float u, invzc, radius; };
    std::vector<Meta> meta;
    for (int i = 0; i < last->n; ++i) {
        if (!last->mp_valid[i]) continue;
        if (last->outlier && last->outlier[i]) continue;
        float x3Dc[3];
        rot_apply(cur->Tcw, last->mp_world + 3 * (size_t)i, 1.0f, x3Dc);
        const float xc = x3Dc[0], yc = x3Dc[1];
        const float invzc = (float)(1.0 / x3Dc[2]);
        if (invzc < 0) continue;
        const float u = cur->fx * xc * invzc + cur->cx, v = cur->fy * yc * invzc + cur->cy;
        if (u < cur->minX || u > cur->maxX) continue;
        if (v < cur->minY || v > cur->maxY) continue;
        const int nLastOctave = last->keys[i].octave;
        if (nLastOctave < 0 || nLastOctave >= cur->n_levels) { set_error("olf_search_by_projection: octave outside mvScaleFactors"); return OLF_ERR_INVALID; }
        const float radius = th * cur->scale_factors[nLastOctave];
        int got;
        if (bForward) got = grid.area(u, v, radius, nLastOctave, -1, q.cand);
        else if (bBackward) got = grid.area(u, v, radius, 0, nLastOctave, q.cand);
        else got = grid.area(u, v, radius, nLastOctave - 1, nLastOctave + 1, q.cand);
        if (!got) continue;
        q.add(i, last->mp_desc + 32 * (size_t)i);
        meta.push_back({u, invzc, radius});
    }
    OLF_TRY(q.run(c, cur->desc, cur->n));

    RotHist hist;
    int n = 0;
    for (size_t k = 0; k < q.owner.size(); ++k) {
        const int i = q.owner[k];
        const Meta& m = meta[k];
        int bestDist = 256, bestIdx2 = -1;
        for (int p = q.offs[k]; p < q.offs[k + 1]; ++p) {
            const int i2 = q.cand[p];
            if (cur->mp_valid[i2] && cur->mp_obs[i2]) continue;
            if (cur->uright[i2] > 0) {
                const float ur = m.u - cur->mbf * m.invzc;
                const float er = std::fabs(ur - cur->uright[i2]);
                if (er > m.radius) continue;
            }
            const int dist = q.dist[p];
            if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; }
        }
        if (bestDist <= TH_HIGH) {
            cur->mp_valid[bestIdx2] = 1;
            cur->mp_obs[bestIdx2] = last->mp_obs[i];
            matches[bestIdx2] = i;
            if (match12 && match12[bestIdx2] < 0) match12[bestIdx2] = i;
            n++;
            if (check_orientation) hist.add(last->keys[i].angle, cur->keys[bestIdx2].angle, bestIdx2);
        }
    }
    hist.reject(check_orientation, [&](int j) { cur->mp_valid[j] = 0; matches[j] = -1; if (match12) match12[j] = -1; n--; });
    *nmatches = n;
    return OLF_OK;
}

// per map point: gates, window, candidates.  Rcw9 / tcw3 / Ow3: camera pose; stereo_gate: the chi-square test of the plain Fuse.
int fuse_core(olf_ctx* c, const char* who, const olf_frame_view* kf, const float* Rcw9, const float* tcw3, const float* Ow3, int n_mp,
              const uint8_t* skip, const float* world, const float* normal, const float* maxd, const float* mind, const uint8_t* desc, float th,
              bool stereo_gate, int none_dist, int32_t* best_idx, int32_t* best_dist, uint8_t* matched = nullptr, int32_t* kf_match = nullptr,
              int32_t* nmatches = nullptr)
{
    // matched != nullptr: SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:292-405) -- key points that hold a match are
    // skipped (:378), a point whose best distance is <= TH_LOW takes its key point at once (:397-401), so later points see it taken
    if (bad_levels(kf)) { set_error(std::string(who) + ": n_levels / scale_factors missing"); return OLF_ERR_INVALID; }
    const float logSF = log_scale_factor(*kf);
    const Grid grid(*kf);
    if (!grid.ok) return bad_grid();
    Batch q;
    struct Meta { float uvr[3]; int level; };
    std::vector<Meta> meta;
    int taken = 0;
    const float cam[5] = {kf->fx, kf->fy, kf->cx, kf->cy, kf->mbf}, bounds[4] = {kf->minX, kf->maxX, kf->minY, kf->maxY};
    for (int i = 0; i < n_mp; ++i) {
        if (best_idx) { best_idx[i] = -1; best_dist[i] = none_dist; }
        if (skip && skip[i]) continue;
        // the gates on the point (fuse_point_gate, search_math.hpp)
        Meta m;
        float dist3D;
        if (!fuse_point_gate(Rcw9, tcw3, Ow3, world + 3 * (size_t)i, normal + 3 * (size_t)i, maxd[i], mind[i], cam, bounds, m.uvr, dist3D)) continue;
        m.level = predict_scale(maxd[i], dist3D, logSF, kf->n_levels);
        const float radius = th * kf->scale_factors[m.level];
        if (!grid.area(m.uvr[0], m.uvr[1], radius, -1, -1, q.cand)) continue;
        q.add(i, desc + 32 * (size_t)i);
        meta.push_back(m);
    }
    const int rc = q.run(c, kf->desc, kf->n);
    if (rc != OLF_OK) return rc;
    for (size_t k = 0; k < q.owner.size(); ++k) {
        const Meta& m = meta[k];
        int bestDist = none_dist, bestIdx = -1;
        for (int p = q.offs[k]; p < q.offs[k + 1]; ++p) {
            const int idx = q.cand[p];
            if (matched && matched[idx]) continue;
            const olf_keypoint& kp = kf->keys[idx];
            const int kpLevel = kp.octave;
            if (!fuse_level_ok(kpLevel, m.level)) continue;
            if (stereo_gate) {
                if (kpLevel < 0 || kpLevel >= kf->n_levels) { set_error(std::string(who) + ": octave outside mvScaleFactors"); return OLF_ERR_INVALID; }
                if (!fuse_chi2_ok(m.uvr, kp.x, kp.y, kf->uright[idx], kf->scale_factors[kpLevel])) continue;
            }
            const int dist = q.dist[p];
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
        }
        if (best_idx) { best_idx[q.owner[k]] = bestIdx; best_dist[q.owner[k]] = bestDist; }
        if (matched && bestDist <= TH_LOW) { matched[bestIdx] = 1; kf_match[bestIdx] = q.owner[k]; ++taken; }
    }
    if (nmatches) *nmatches = taken;
    return OLF_OK;
}
}  // namespace

extern "C" {

// ---- the every-frame searches ---------------------------------------------------------------------------------------------------------------------

int olf_search_by_projection(olf_ctx* c, const olf_frame_view* cur, const olf_frame_view* last, float th, int bMono, int check_orientation,
                             int32_t* matches, int32_t* nmatches)
{
    return search_by_projection_frames(c, cur, last, th, bMono, check_orientation, matches, nullptr, nmatches);
}

int olf_search_by_projection_match12(olf_ctx* c, const olf_frame_view* cur, const olf_frame_view* last, float th, int bMono, int check_orientation,
                                     int32_t* matches, int32_t* match12, int32_t* nmatches)
{
    if (!match12) { set_error("olf_search_by_projection_match12: bad argument"); return OLF_ERR_INVALID; }
    return search_by_projection_frames(c, cur, last, th, bMono, check_orientation, matches, match12, nmatches);
}

int olf_search_for_initialization(olf_ctx* c, const olf_frame_view* f1, const olf_frame_view* f2, float* prev_matched, int window_size, float nnratio,
                                  int check_orientation, int32_t* matches12, int32_t* nmatches)
{
    if (!c || bad_view(f1, false) || bad_view(f2, false) || !matches12 || !nmatches || (f1->n && !prev_matched)) {
        set_error("olf_search_for_initialization: bad argument"); return OLF_ERR_INVALID;
    }
    for (int i = 0; i < f1->n; ++i) matches12[i] = -1;
    *nmatches = 0;
    // candidate lists: GetFeaturesInArea(vbPrevMatched[i1], windowSize, level1, level1) for the level-0 key points of F1   (:421-429)
    const Grid grid(*f2);
    if (!grid.ok) return bad_grid();
    Batch q;
    for (int i1 = 0; i1 < f1->n; ++i1) {
        const int level1 = f1->keys[i1].octave;
        if (level1 > 0) continue;
        if (!grid.area(prev_matched[2 * i1], prev_matched[2 * i1 + 1], (float)window_size, level1, level1, q.cand)) continue;
        q.add(i1, f1->desc + 32 * (size_t)i1);
    }
    OLF_TRY(q.run(c, f2->desc, f2->n));
    // the resolution depends on the matches made so far (vMatchedDistance): replayed in F1 order                             (:431-486)
    std::vector<int> matchedDistance((size_t)f2->n, INT_MAX), matches21((size_t)f2->n, -1);
    RotHist hist;
    int n = 0;
    for (size_t k = 0; k < q.owner.size(); ++k) {
        const int i1 = q.owner[k];
        int bestDist = INT_MAX, bestDist2 = INT_MAX, bestIdx2 = -1;
        for (int p = q.offs[k]; p < q.offs[k + 1]; ++p) {
            const int i2 = q.cand[p], dist = q.dist[p];
            if (matchedDistance[i2] <= dist) continue;
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; }
            else if (dist < bestDist2) bestDist2 = dist;
        }
        if (bestDist <= TH_LOW && (float)bestDist < (float)bestDist2 * nnratio) {
            if (matches21[bestIdx2] >= 0) { matches12[matches21[bestIdx2]] = -1; n--; }
            matches12[i1] = bestIdx2;
            matches21[bestIdx2] = i1;
            matchedDistance[bestIdx2] = bestDist;
            n++;
            if (check_orientation) hist.add(f1->keys[i1].angle, f2->keys[bestIdx2].angle, i1);
        }
    }
    hist.reject(check_orientation, [&](int idx1) { if (matches12[idx1] >= 0) { matches12[idx1] = -1; n--; } });      // (a later match may already have undone it)
    for (int i1 = 0; i1 < f1->n; ++i1)                                                       // "Update prev matched"          (:516-519)
        if (matches12[i1] >= 0) { prev_matched[2 * i1] = f2->keys[matches12[i1]].x; prev_matched[2 * i1 + 1] = f2->keys[matches12[i1]].y; }
    *nmatches = n;
    return OLF_OK;
}

int olf_search_by_bow(olf_ctx* c, const olf_frame_view* kf, const olf_frame_view* f, float nnratio, int check_orientation, int32_t* matched,
                      int32_t* nmatches)
{
    if (!c || bad_view(kf, false) || bad_view(f, false) || !matched || !nmatches || (kf->n && (!kf->mp_valid || !kf->mp_bad)) || fv_missing(kf) ||
        fv_missing(f)) {
        set_error("olf_search_by_bow: bad argument"); return OLF_ERR_INVALID;
    }
    for (int i = 0; i < f->n; ++i) matched[i] = -1;
    *nmatches = 0;
    // only nodes present in both contribute (:176-203, :273-281)
    Batch q;
    if (!bow_queries(*kf, *f, q, [&](int realIdxKF) { return kf->mp_valid[realIdxKF] && !kf->mp_bad[realIdxKF]; })) {
        set_error("olf_search_by_bow: feature index outside the key frame"); return OLF_ERR_INVALID;
    }
    OLF_TRY(q.run(c, f->desc, f->n));

    RotHist hist;
    int n = 0;
    for (size_t k = 0; k < q.owner.size(); ++k) {
        const int realIdxKF = q.owner[k];
        int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
        for (int p = q.offs[k]; p < q.offs[k + 1]; ++p) {
            const int realIdxF = q.cand[p];
            if (realIdxF < 0 || realIdxF >= f->n) { set_error("olf_search_by_bow: feature index outside the frame"); return OLF_ERR_INVALID; }
            if (matched[realIdxF] >= 0) continue;
            const int dist = q.dist[p];
            if (dist < bestDist1) { bestDist2 = bestDist1; bestDist1 = dist; bestIdxF = realIdxF; }
            else if (dist < bestDist2) bestDist2 = dist;
        }
        if (bestDist1 <= TH_LOW) {
            if (static_cast<float>(bestDist1) < nnratio * static_cast<float>(bestDist2)) {
                matched[bestIdxF] = realIdxKF;
                if (check_orientation) hist.add(kf->keys[realIdxKF].angle, f->keys[bestIdxF].angle, bestIdxF);
                n++;
            }
        }
    }
    hist.reject(check_orientation, [&](int j) { matched[j] = -1; n--; });
    *nmatches = n;
    return OLF_OK;
}

int olf_search_local_map(olf_ctx* c, const olf_frame_view* f, int n_mp, const uint8_t* track_in_view, const uint8_t* bad,
                         const int32_t* track_scale_level, const float* track_view_cos, const float* track_proj3, const uint8_t* mp_desc,
                         const uint8_t* mp_obs, float th, float nnratio, int32_t* matches, int32_t* nmatches)
{
    if (!c || bad_view(f, false) || n_mp < 0 || !matches || !nmatches || !f->scale_factors || !f->mp_valid || !f->mp_obs || (f->n && !f->uright) ||
        (n_mp && (!track_in_view || !bad || !track_scale_level || !track_view_cos || !track_proj3 || !mp_desc || !mp_obs))) {
        set_error("olf_search_local_map: bad argument"); return OLF_ERR_INVALID;
    }
    for (int i = 0; i < f->n; ++i) matches[i] = -1;
    *nmatches = 0;
    const bool bFactor = th != 1.0;
    const Grid grid(*f);
    if (!grid.ok) return bad_grid();
    Batch q;
    std::vector<float> radii;
    for (int iMP = 0; iMP < n_mp; ++iMP) {
        if (!track_in_view[iMP]) continue;
        if (bad[iMP]) continue;
        const int nPredictedLevel = track_scale_level[iMP];
        if (nPredictedLevel < 0 || nPredictedLevel >= f->n_levels) { set_error("olf_search_local_map: scale level outside mvScaleFactors"); return OLF_ERR_INVALID; }
        float r = track_view_cos[iMP] > 0.998 ? 2.5f : 4.0f;            // RadiusByViewingCos, :133-139
        if (bFactor) r *= th;
        const float rs = r * f->scale_factors[nPredictedLevel];
        if (!grid.area(track_proj3[3 * (size_t)iMP], track_proj3[3 * (size_t)iMP + 1], rs, nPredictedLevel - 1, nPredictedLevel, q.cand)) continue;
        q.add(iMP, mp_desc + 32 * (size_t)iMP);
        radii.push_back(rs);
    }
    OLF_TRY(q.run(c, f->desc, f->n));

    int n = 0;
    for (size_t k = 0; k < q.owner.size(); ++k) {
        const int iMP = q.owner[k];
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
        for (int p = q.offs[k]; p < q.offs[k + 1]; ++p) {
            const int idx = q.cand[p];
            if (f->mp_valid[idx] && f->mp_obs[idx]) continue;
            if (f->uright[idx] > 0) {
                const float er = std::fabs(track_proj3[3 * (size_t)iMP + 2] - f->uright[idx]);
                if (er > radii[k]) continue;
            }
            const int dist = q.dist[p];
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = f->keys[idx].octave; bestIdx = idx; }
            else if (dist < bestDist2) { bestLevel2 = f->keys[idx].octave; bestDist2 = dist; }
        }
        // Apply ratio to second match (only if best and second are in the same scale level)
        if (bestDist <= TH_HIGH) {
            if (bestLevel == bestLevel2 && bestDist > nnratio * bestDist2) continue;
            f->mp_valid[bestIdx] = 1;
            f->mp_obs[bestIdx] = mp_obs[iMP];
            matches[bestIdx] = iMP;
            n++;
        }
    }
    *nmatches = n;
    return OLF_OK;
}

// ---- LocalMapping / LoopClosing / relocalisation searches ------------------------------------------------------------------------

int olf_search_by_projection_kf(olf_ctx* c, const olf_frame_view* cur, const olf_frame_view* kf, const uint8_t* already_found, float th,
                                int orb_dist, int check_orientation, int32_t* matches, int32_t* nmatches)
{
    if (!c || bad_view(cur, true) || bad_view(kf, false) || !matches || !nmatches || !cur->scale_factors || !cur->mp_valid || bad_kf_points(kf)) {
        set_error("olf_search_by_projection_kf: bad argument"); return OLF_ERR_INVALID;
    }
    if (bad_levels(cur)) { set_error("olf_search_by_projection_kf: n_levels / scale_factors missing"); return OLF_ERR_INVALID; }
    for (int i = 0; i < cur->n; ++i) matches[i] = -1;
    *nmatches = 0;
    float Ow[3];
    camera_centre(cur->Tcw, Ow);
    const float logSF = log_scale_factor(*cur);
    const Grid grid(*cur);
    if (!grid.ok) return bad_grid();
    Batch q;
    const float cam[4] = {cur->fx, cur->fy, cur->cx, cur->cy}, bounds[4] = {cur->minX, cur->maxX, cur->minY, cur->maxY};
    for (int i = 0; i < kf->n; ++i) {
        if (!kf->mp_valid[i]) continue;
        if (kf->mp_bad[i] || (already_found && already_found[i])) continue;
        // the gates on the point (reloc_point_gate, search_math.hpp)
        float uv[2], dist3D;
        if (!reloc_point_gate(cur->Tcw, Ow, kf->mp_world + 3 * (size_t)i, kf->mp_maxd[i], kf->mp_mind[i], cam, bounds, uv, dist3D)) continue;
        const int nPredictedLevel = predict_scale(kf->mp_maxd[i], dist3D, logSF, cur->n_levels);
        // Search in a window
        const float radius = th * cur->scale_factors[nPredictedLevel];
        if (!grid.area(uv[0], uv[1], radius, nPredictedLevel - 1, nPredictedLevel + 1, q.cand)) continue;
        q.add(i, kf->mp_desc + 32 * (size_t)i);
    }
    OLF_TRY(q.run(c, cur->desc, cur->n));
    RotHist hist;
    int n = 0;
    for (size_t k = 0; k < q.owner.size(); ++k) {
        const int i = q.owner[k];
        int bestDist = 256, bestIdx2 = -1;
        for (int p = q.offs[k]; p < q.offs[k + 1]; ++p) {
            const int i2 = q.cand[p];
            if (cur->mp_valid[i2]) continue;
            const int dist = q.dist[p];
            if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; }
        }
        if (bestDist <= orb_dist) {
            cur->mp_valid[bestIdx2] = 1;
            matches[bestIdx2] = i;
            n++;
            if (check_orientation) hist.add(kf->keys[i].angle, cur->keys[bestIdx2].angle, bestIdx2);
        }
    }
    hist.reject(check_orientation, [&](int j) { cur->mp_valid[j] = 0; matches[j] = -1; n--; });
    *nmatches = n;
    return OLF_OK;
}

int olf_search_by_bow_kf(olf_ctx* c, const olf_frame_view* kf1, const olf_frame_view* kf2, float nnratio, int check_orientation,
                         int32_t* matches12, int32_t* nmatches)
{
    if (!c || bad_view(kf1, false) || bad_view(kf2, false) || !matches12 || !nmatches || bad_fv(kf1) || bad_fv(kf2) ||
        (kf1->n && (!kf1->mp_valid || !kf1->mp_bad)) || (kf2->n && (!kf2->mp_valid || !kf2->mp_bad))) {
        set_error("olf_search_by_bow_kf: bad argument"); return OLF_ERR_INVALID;
    }
    for (int i = 0; i < kf1->n; ++i) matches12[i] = -1;
    *nmatches = 0;
    Batch q;
    const bool inside1 = bow_queries(*kf1, *kf2, q, [&](int idx1) { return kf1->mp_valid[idx1] && !kf1->mp_bad[idx1]; });
    if (!inside1 || !cand_inside(q, *kf2)) { set_error("olf_search_by_bow_kf: feature index outside its key frame"); return OLF_ERR_INVALID; }
    OLF_TRY(q.run(c, kf2->desc, kf2->n));
    std::vector<uint8_t> vbMatched2((size_t)std::max(kf2->n, 0), 0);
    RotHist hist;
    int n = 0;
    for (size_t k = 0; k < q.owner.size(); ++k) {
        const int idx1 = q.owner[k];
        int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256;
        for (int p = q.offs[k]; p < q.offs[k + 1]; ++p) {
            const int idx2 = q.cand[p];
            if (vbMatched2[idx2] || !kf2->mp_valid[idx2]) continue;
            if (kf2->mp_bad[idx2]) continue;
            const int dist = q.dist[p];
            if (dist < bestDist1) { bestDist2 = bestDist1; bestDist1 = dist; bestIdx2 = idx2; }
            else if (dist < bestDist2) bestDist2 = dist;
        }
        if (bestDist1 < TH_LOW) {
            if (static_cast<float>(bestDist1) < nnratio * static_cast<float>(bestDist2)) {
                matches12[idx1] = bestIdx2;
                vbMatched2[bestIdx2] = 1;
                if (check_orientation) hist.add(kf1->keys[idx1].angle, kf2->keys[bestIdx2].angle, idx1);
                n++;
            }
        }
    }
    hist.reject(check_orientation, [&](int j) { matches12[j] = -1; n--; });
    *nmatches = n;
    return OLF_OK;
}

int olf_search_for_triangulation(olf_ctx* c, const olf_frame_view* kf1, const olf_frame_view* kf2, const float* F12, const float* Cw,
                                 int only_stereo, int check_orientation, int32_t* matches12, int32_t* nmatches)
{
    if (!c || bad_view(kf1, !Cw) || bad_view(kf2, true) || !F12 || !matches12 || !nmatches || bad_fv(kf1) || bad_fv(kf2) || !kf2->scale_factors ||
        (kf1->n && (!kf1->mp_valid || !kf1->uright)) || (kf2->n && (!kf2->mp_valid || !kf2->uright))) {
        set_error("olf_search_for_triangulation: bad argument"); return OLF_ERR_INVALID;
    }
    for (int i = 0; i < kf1->n; ++i) matches12[i] = -1;
    *nmatches = 0;
    // Compute epipole in second image (:666-676)
    float cw[3], ex, ey;
    if (Cw) std::memcpy(cw, Cw, sizeof(cw)); else camera_centre(kf1->Tcw, cw);
    tri_epipole(kf2->Tcw, cw, kf2->fx, kf2->fy, kf2->cx, kf2->cy, ex, ey);
    Batch q;
    const bool inside1 = bow_queries(*kf1, *kf2, q, [&](int idx1) {
        // If there is already a MapPoint skip
        if (kf1->mp_valid[idx1]) return false;
        const bool bStereo1 = kf1->uright[idx1] >= 0;
        if (only_stereo) if (!bStereo1) return false;
        return true;
    });
    if (!inside1 || !cand_inside(q, *kf2)) { set_error("olf_search_for_triangulation: feature index outside its key frame"); return OLF_ERR_INVALID; }
    OLF_TRY(q.run(c, kf2->desc, kf2->n));
    RotHist hist;
    int n = 0;
    for (size_t k = 0; k < q.owner.size(); ++k) {
        const int idx1 = q.owner[k];
        const bool bStereo1 = kf1->uright[idx1] >= 0;
        const olf_keypoint& kp1 = kf1->keys[idx1];
        int bestDist = TH_LOW, bestIdx2 = -1;
        for (int p = q.offs[k]; p < q.offs[k + 1]; ++p) {
            const int idx2 = q.cand[p];
            // If we have already matched or there is a MapPoint skip (vbMatched2 is never set in the reference)
            if (kf2->mp_valid[idx2]) continue;
            const bool bStereo2 = kf2->uright[idx2] >= 0;
            if (only_stereo) if (!bStereo2) continue;
            const int dist = q.dist[p];
            if (dist > TH_LOW || dist > bestDist) continue;
            const olf_keypoint& kp2 = kf2->keys[idx2];
            if (kp2.octave < 0 || kp2.octave >= kf2->n_levels) { set_error("olf_search_for_triangulation: octave outside mvScaleFactors"); return OLF_ERR_INVALID; }
            const float sf2 = kf2->scale_factors[kp2.octave];
            if (!bStereo1 && !bStereo2 && tri_near_epipole(ex, ey, kp2.x, kp2.y, sf2)) continue;
            // CheckDistEpipolarLine (:142-161): search_math.hpp
            float l[3];
            tri_epiline(F12, kp1.x, kp1.y, l);
            if (tri_epiline_ok(l, kp2.x, kp2.y, sf2)) { bestIdx2 = idx2; bestDist = dist; }
        }
        if (bestIdx2 >= 0) {
            matches12[idx1] = bestIdx2;
            n++;
            if (check_orientation) hist.add(kp1.angle, kf2->keys[bestIdx2].angle, idx1);
        }
    }
    hist.reject(check_orientation, [&](int j) { matches12[j] = -1; n--; });
    *nmatches = n;
    return OLF_OK;
}

int olf_fuse_search(olf_ctx* c, const olf_frame_view* kf, int n_mp, const uint8_t* skip, const float* world, const float* normal,
                    const float* maxd, const float* mind, const uint8_t* desc, float th, const float* Ow, int32_t* best_idx, int32_t* best_dist)
{
    if (!c || bad_view(kf, true) || n_mp < 0 || !best_idx || !best_dist || !kf->scale_factors || (kf->n && !kf->uright) ||
        bad_points(n_mp, world, normal, maxd, mind, desc)) { set_error("olf_fuse_search: bad argument"); return OLF_ERR_INVALID; }
    float R[9], t[3], ow[3];
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) R[3 * r + k] = kf->Tcw[4 * r + k]; t[r] = kf->Tcw[4 * r + 3]; }
    if (Ow) std::memcpy(ow, Ow, sizeof(ow)); else camera_centre(kf->Tcw, ow);
    return fuse_core(c, "olf_fuse_search", kf, R, t, ow, n_mp, skip, world, normal, maxd, mind, desc, th, true, 256, best_idx, best_dist);
}

int olf_fuse_search_sim3(olf_ctx* c, const olf_frame_view* kf, const float* Scw, int n_mp, const uint8_t* skip, const float* world,
                         const float* normal, const float* maxd, const float* mind, const uint8_t* desc, float th, int32_t* best_idx,
                         int32_t* best_dist)
{
    if (!c || bad_view(kf, false) || !Scw || n_mp < 0 || !best_idx || !best_dist || !kf->scale_factors ||
        bad_points(n_mp, world, normal, maxd, mind, desc)) { set_error("olf_fuse_search_sim3: bad argument"); return OLF_ERR_INVALID; }
    float R[9], t[3], ow[3];
    sim3_decompose(Scw, R, t, ow);
    return fuse_core(c, "olf_fuse_search_sim3", kf, R, t, ow, n_mp, skip, world, normal, maxd, mind, desc, th, false, 2147483647, best_idx,
                     best_dist);
}

int olf_search_by_projection_sim3(olf_ctx* c, const olf_frame_view* kf, const float* Scw, int n_mp, const uint8_t* skip, const float* world,
                                  const float* normal, const float* maxd, const float* mind, const uint8_t* desc, float th, uint8_t* matched,
                                  int32_t* matches, int32_t* nmatches)
{
    if (!c || bad_view(kf, false) || !Scw || n_mp < 0 || !matched || !matches || !nmatches || !kf->scale_factors ||
        bad_points(n_mp, world, normal, maxd, mind, desc)) { set_error("olf_search_by_projection_sim3: bad argument"); return OLF_ERR_INVALID; }
    float R[9], t[3], ow[3];
    sim3_decompose(Scw, R, t, ow);
    for (int i = 0; i < kf->n; ++i) matches[i] = -1;
    return fuse_core(c, "olf_search_by_projection_sim3", kf, R, t, ow, n_mp, skip, world, normal, maxd, mind, desc, th, false, 256, nullptr, nullptr,
                     matched, matches, nmatches);
}

int olf_search_by_sim3(olf_ctx* c, const olf_frame_view* kf1, const olf_frame_view* kf2, int32_t* matches12, float s12, const float* R12,
                       const float* t12, float th, int32_t* vn_match1, int32_t* vn_match2, int32_t* nfound)
{
    if (!c || bad_view(kf1, true) || bad_view(kf2, true) || !matches12 || !R12 || !t12 || !vn_match1 || !vn_match2 || !nfound ||
        !kf1->scale_factors || !kf2->scale_factors || bad_kf_points(kf1) || bad_kf_points(kf2)) {
        set_error("olf_search_by_sim3: bad argument"); return OLF_ERR_INVALID;
    }
    if (bad_levels(kf1) || bad_levels(kf2)) { set_error("olf_search_by_sim3: n_levels / scale_factors missing"); return OLF_ERR_INVALID; }
    const int N1 = kf1->n, N2 = kf2->n;
    // Transformation between cameras (:1123-1125)
    float sR12[9], sR21[9], t21[3];
    sim3_pair_transforms(s12, R12, t12, sR12, sR21, t21);
    std::vector<uint8_t> already1((size_t)N1, 0), already2((size_t)N2, 0);
    for (int i = 0; i < N1; i++) {
        if (matches12[i] != -1) {
            already1[i] = 1;
            const int idx2 = matches12[i];
            if (idx2 >= 0 && idx2 < N2) already2[idx2] = 1;
        }
    }
    const float logSF = log_scale_factor(*kf1);
    for (int dir = 0; dir < 2; ++dir) {
        // dir 0: the map points of KF1 into KF2 (:1157-1232); dir 1: those of KF2 into KF1 (:1235-1309)
        const olf_frame_view &src = dir ? *kf2 : *kf1, &dst = dir ? *kf1 : *kf2;
        const std::vector<uint8_t>& already = dir ? already2 : already1;
        const float *sR = dir ? sR12 : sR21, *t = dir ? t12 : t21;
        int32_t* out = dir ? vn_match2 : vn_match1;
        for (int i = 0; i < src.n; ++i) out[i] = -1;
        const Grid grid(dst);
        if (!grid.ok) return bad_grid();
        Batch q;
        std::vector<int> levels;
        for (int i = 0; i < src.n; ++i) {
            if (!src.mp_valid[i] || already[i]) continue;
            if (src.mp_bad[i]) continue;
            // (the projection and the gates on the point: sim3_point_gate, search_math.hpp)
            const float cam[4] = {dst.fx, dst.fy, dst.cx, dst.cy}, bounds[4] = {dst.minX, dst.maxX, dst.minY, dst.maxY};
            float uv[2], dist3D;
            if (!sim3_point_gate(src.Tcw, src.mp_world + 3 * (size_t)i, sR, t, src.mp_maxd[i], src.mp_mind[i], cam, bounds, uv, dist3D)) continue;
            const float u = uv[0], v = uv[1];
            const int nPredictedLevel = predict_scale(src.mp_maxd[i], dist3D, logSF, dst.n_levels);
            const float radius = th * dst.scale_factors[nPredictedLevel];
            if (!grid.area(u, v, radius, -1, -1, q.cand)) continue;
            q.add(i, src.mp_desc + 32 * (size_t)i);
            levels.push_back(nPredictedLevel);
        }
        OLF_TRY(q.run(c, dst.desc, dst.n));
        for (size_t k = 0; k < q.owner.size(); ++k) {
            int bestDist = 2147483647, bestIdx = -1;
            for (int p = q.offs[k]; p < q.offs[k + 1]; ++p) {
                const int idx = q.cand[p];
                const int oct = dst.keys[idx].octave;
                if (oct < levels[k] - 1 || oct > levels[k]) continue;
                const int dist = q.dist[p];
                if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
            }
            if (bestDist <= TH_HIGH) out[q.owner[k]] = bestIdx;
        }
    }
    // Check agreement
    int found = 0;
    for (int i1 = 0; i1 < N1; i1++) {
        const int idx2 = vn_match1[i1];
        if (idx2 >= 0 && vn_match2[idx2] == i1) { matches12[i1] = idx2; found++; }
    }
    *nfound = found;
    return OLF_OK;
}

}  // extern "C"
