// adaptor_localmap.cpp -- MapGraphOf<KeyFrame, MapPoint, MapLine> and its write-back (include/orbline_reference_api.hpp) against stand-in types, on the CPU:
// the five-key-frame graph of tests/localmap_scenes.py (five_kf), with the key frames laid out so that their address order is the REVERSE of the order given
// (a std::set<KeyFrame*> then iterates the children backwards and the adaptor has to sort them: convention C.16), one key frame outside the snapshot, and the
// outputs of frame 0 as tests/localmap_scenes.py derives them (FIVE_KF_EXPECTED), renumbered as the adaptor numbers points and lines: by first appearance in
// the key frames' slots.  Prints ADAPTOR_LOCALMAP_OK.  ORB_SLAM2::UpdateLocalMap is instantiated, not run: it needs a device.
#include <cstdio>
#include <cstdlib>
#include "../include/orbline_reference_api.hpp"

struct KeyFrame;
struct MapPoint {
    bool bad = false;
    std::map<KeyFrame*, size_t> obs;
    bool isBad() { return bad; }
    std::map<KeyFrame*, size_t> GetObservations() { return obs; }
};
struct MapLine {
    bool bad = false;
    bool isBad() { return bad; }
};
struct KeyFrame {
    bool bad = false;
    std::vector<MapPoint*> mps;
    std::vector<MapLine*> mls;
    std::vector<KeyFrame*> covis;
    std::set<KeyFrame*> childs;
    KeyFrame* parent = nullptr;
    bool isBad() { return bad; }
    std::vector<MapPoint*> GetMapPointMatches() { return mps; }
    std::vector<MapLine*> GetMapLineMatches() { return mls; }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return covis; }
    std::set<KeyFrame*> GetChilds() { return childs; }
    KeyFrame* GetParent() { return parent; }
};
struct Frame {
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    KeyFrame* mpReferenceKF = nullptr;
};

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static bool same(const int32_t* a, std::initializer_list<int> want)
{
    size_t i = 0;
    for (int w : want) if (a[i++] != w) return false;
    return true;
}
static bool same8(const uint8_t* a, std::initializer_list<int> want)
{
    size_t i = 0;
    for (int w : want) if (a[i++] != w) return false;
    return true;
}

int main(int argc, char**)
{
    KeyFrame pool[6];
    KeyFrame* kf[5] = {&pool[4], &pool[3], &pool[2], &pool[1], &pool[0]};      // ascending index = descending address
    KeyFrame* outside = &pool[5];
    MapPoint p[6];
    MapLine l[3];
    p[0].obs[kf[1]] = 0; p[0].obs[kf[3]] = 1; p[1].obs[kf[3]] = 0; p[1].obs[outside] = 7; p[2].obs[kf[1]] = 2; p[3].obs[kf[4]] = 0; p[4].obs[kf[2]] = 0; p[5].obs[kf[0]] = 0;
    p[3].bad = true; l[2].bad = true; kf[0]->bad = true;
    kf[0]->mps = {&p[5], &p[0]}; kf[1]->mps = {&p[0], nullptr, &p[2]}; kf[2]->mps = {&p[4], &p[3]}; kf[3]->mps = {&p[1], &p[0]}; kf[4]->mps = {&p[3], &p[2]};
    kf[1]->mls = {&l[1]}; kf[2]->mls = {&l[2]}; kf[3]->mls = {&l[1], &l[0]};
    kf[1]->covis = {kf[3], kf[0], kf[2]}; kf[3]->covis = {kf[1], outside};
    kf[0]->childs = {kf[1]}; kf[1]->childs = {kf[4], kf[2], kf[3]};
    kf[1]->parent = kf[0]; kf[2]->parent = kf[1]; kf[3]->parent = kf[1]; kf[4]->parent = kf[1];

    typedef ORB_SLAM2::MapGraphOf<KeyFrame, MapPoint, MapLine> Graph;
    const Graph G(std::vector<KeyFrame*>(kf, kf + 5));
    const olf_map_graph& g = G.graph();
    expect(g.n_kf == 5 && g.n_mp == 6 && g.n_ml == 3, "sizes");
    // points by first appearance: p5, p0, p2, p4, p3, p1; lines: l1, l2, l0
    expect(G.index_of(&p[5]) == 0 && G.index_of(&p[0]) == 1 && G.index_of(&p[2]) == 2 && G.index_of(&p[4]) == 3 && G.index_of(&p[3]) == 4 && G.index_of(&p[1]) == 5, "point numbers");
    expect(G.line_index_of(&l[1]) == 0 && G.line_index_of(&l[2]) == 1 && G.line_index_of(&l[0]) == 2, "line numbers");
    expect(G.index_of(outside) == -1 && G.index_of(kf[3]) == 3, "key-frame numbers");
    expect(same(g.kf_mp_offsets, {0, 2, 5, 7, 9, 11}) && same(g.kf_mp_index, {0, 1, 1, -1, 2, 3, 4, 5, 1, 4, 2}), "kf_mp");
    expect(same(g.kf_ml_offsets, {0, 0, 1, 2, 4, 4}) && same(g.kf_ml_index, {0, 1, 0, 2}), "kf_ml");
    expect(same(g.mp_obs_offsets, {0, 1, 3, 4, 5, 6, 7}), "mp_obs_offsets");
    // (inside a point the order is that of the std::map, here descending index: irrelevant to the call)
    expect(same(g.mp_obs_kf, {0, 3, 1, 1, 2, 4, 3}) || same(g.mp_obs_kf, {0, 1, 3, 1, 2, 4, 3}), "mp_obs_kf (the key frame outside is left out)");
    expect(same8(g.mp_bad, {0, 0, 0, 0, 1, 0}) && same8(g.ml_bad, {0, 1, 0}) && same8(g.kf_bad, {1, 0, 0, 0, 0}), "bad flags");
    expect(same(g.kf_covis_offsets, {0, 0, 3, 3, 4, 4}) && same(g.kf_covis_index, {3, 0, 2, 1}), "covisibility (its own order; the key frame outside is left out)");
    expect(same(g.kf_child_offsets, {0, 1, 4, 4, 4, 4}) && same(g.kf_child_index, {1, 2, 3, 4}), "children ascend by number although their addresses descend");
    expect(same(g.kf_parent, {-1, 0, 1, 1, 1}), "parents");

    Frame F;
    MapPoint temporal;
    F.mvpMapPoints = {&p[0], &p[1], &p[2], &p[3], nullptr, &temporal};
    F.mvpMapLines = {&l[2], &l[0]};
    int32_t mp_in[8], ml_in[4];
    G.FrameRows(F, mp_in, 8, ml_in, 4);
    expect(same(mp_in, {1, 5, 2, 4, -1, -1, -1, -1}) && same(ml_in, {1, 2, -1, -1}), "frame rows (a point no key frame holds is a temporal one: -1)");

    // frame 0 of FIVE_KF_EXPECTED in the adaptor's numbers
    const int32_t mp_out[8] = {1, 5, 2, -1, -1, -1, -1, -1}, ml_out[4] = {-1, 2, -1, -1};
    const int32_t ref[2] = {1, -1}, voted[2] = {2, 0}, kf_off[3] = {0, 5, 5}, kf_idx[5] = {1, 3, 2, 4, 0}, mp_off[3] = {0, 5, 5}, mp_idx[5] = {1, 2, 5, 3, 0}, ml_off[3] = {0, 2, 2},
                  ml_idx[2] = {0, 2};
    std::vector<KeyFrame*> localKFs(1, outside);
    std::vector<MapPoint*> localMPs;
    std::vector<MapLine*> localMLs;
    KeyFrame* refKF = nullptr;
    G.WriteBack(0, F, mp_in, mp_out, ml_in, ml_out, ref, voted, kf_off, kf_idx, mp_off, mp_idx, ml_off, ml_idx, localKFs, localMPs, localMLs, refKF);
    expect(localKFs == std::vector<KeyFrame*>({kf[1], kf[3], kf[2], kf[4], kf[0]}), "mvpLocalKeyFrames");
    expect(localMPs == std::vector<MapPoint*>({&p[0], &p[2], &p[1], &p[4], &p[5]}), "mvpLocalMapPoints");
    expect(localMLs == std::vector<MapLine*>({&l[1], &l[0]}), "mvpLocalMapLines");
    expect(refKF == kf[1] && F.mpReferenceKF == kf[1], "mpReferenceKF");
    expect(F.mvpMapPoints[3] == nullptr && F.mvpMapPoints[0] == &p[0] && F.mvpMapPoints[5] == &temporal && F.mvpMapLines[0] == nullptr && F.mvpMapLines[1] == &l[0], "the bad ones are cleared, nothing else");
    // a frame without votes leaves the members as they are (:2120)
    G.WriteBack(1, F, mp_out, mp_out, ml_out, ml_out, ref, voted, kf_off, kf_idx, mp_off, mp_idx, ml_off, ml_idx, localKFs, localMPs, localMLs, refKF);
    expect(localKFs.size() == 5 && localMPs.size() == 5 && localMLs.size() == 2 && refKF == kf[1], "n_voted == 0 changes nothing");

    if (argc > 100) ORB_SLAM2::UpdateLocalMap<KeyFrame, MapPoint, MapLine>(std::vector<KeyFrame*>(kf, kf + 5), F, localKFs, localMPs, localMLs, refKF);      // (instantiated only)
    if (failures) return 1;
    std::printf("ADAPTOR_LOCALMAP_OK\n");
    return 0;
}
