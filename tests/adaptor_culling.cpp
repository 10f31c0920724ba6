// adaptor_culling.cpp -- ORB_SLAM2::KeyFrameCulling, ApplyKeyFrameCulling, CullingSnapshot and MapGraphOf::cull_view (include/orbline_reference_api.hpp)
// against stand-in types whose SetBadFlag / EraseObservation are the reference's (src/KeyFrame.cc:631-649, src/MapPoint.cc:123-180).  Two scenes of
// tests/culling_scenes.py, each as the covisible key frames [A, B] of a current key frame:
//   loses redundancy  ten points seen mono by A, B, C, D: A is culled, every nObs falls to 3, B is kept
//   gains redundancy  B holds nine points seen by B, C, D, E and q (A stereo, B mono); A holds q and ten points seen by A, C, D, E: A is culled, q goes bad,
//                     B is left with 9 of 9 and is culled
//   without an argument  the snapshot, the view, olf_keyframe_culling_replay on the tables worked out by hand (LOSES_TABLES, GAINS_TABLES and the counts
//                        beside them), ApplyKeyFrameCulling; no device is needed.  Prints ADAPTOR_CULLING_OK.
//   with "device"        KeyFrameCulling itself: the host form on the device, then the same checks.
// The stand-in KeyFrame provides the one accessor the integrator adds (GetNotErase).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../include/orbline_reference_api.hpp"

struct KeyFrame;
struct MapPoint {
    bool bad = false;
    int nObs = 0;
    std::map<KeyFrame*, size_t> mObservations;
    bool isBad() { return bad; }
    std::map<KeyFrame*, size_t> GetObservations() { return mObservations; }
    int Observations() { return nObs; }
    void AddObservation(KeyFrame* pKF, size_t idx);
    void EraseObservation(KeyFrame* pKF);
    void SetBadFlag();
};
struct MapLine {
    bool isBad() { return false; }
};
struct KeyPoint { int octave = 0; };
struct KeyFrame {
    long unsigned int mnId = 1;
    float mThDepth = 35.0f;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    bool mbNotErase = false, mbToBeErased = false, mbBad = false;
    bool isBad() { return mbBad; }
    bool GetNotErase() { return mbNotErase; }
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<MapLine*> GetMapLineMatches() { return std::vector<MapLine*>(); }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::set<KeyFrame*> GetChilds() { return std::set<KeyFrame*>(); }
    KeyFrame* GetParent() { return nullptr; }
    void EraseMapPointMatch(const size_t& idx) { mvpMapPoints[idx] = nullptr; }
    size_t hold(MapPoint* pMP, bool stereo)
    {
        mvpMapPoints.push_back(pMP); mvKeysUn.push_back(KeyPoint()); mvDepth.push_back(10.0f); mvuRight.push_back(stereo ? 5.0f : -1.0f);
        return mvpMapPoints.size() - 1;
    }
    void SetBadFlag()                                               // src/KeyFrame.cc:631-649; the spanning tree is left out
    {
        if (mnId == 0) return;
        else if (mbNotErase) { mbToBeErased = true; return; }
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
        mbBad = true;
    }
};
void MapPoint::AddObservation(KeyFrame* pKF, size_t idx)
{
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    if (pKF->mvuRight[idx] >= 0) nObs += 2; else nObs++;
}
void MapPoint::EraseObservation(KeyFrame* pKF)
{
    bool bBad = false;
    if (mObservations.count(pKF)) {
        int idx = mObservations[pKF];
        if (pKF->mvuRight[idx] >= 0) nObs -= 2; else nObs--;
        mObservations.erase(pKF);
        if (nObs <= 2) bBad = true;
    }
    if (bBad) SetBadFlag();
}
void MapPoint::SetBadFlag()
{
    std::map<KeyFrame*, size_t> obs = mObservations;
    bad = true;
    mObservations.clear();
    for (std::map<KeyFrame*, size_t>::iterator mit = obs.begin(); mit != obs.end(); mit++) mit->first->EraseMapPointMatch(mit->second);
}

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }
static void see(MapPoint& p, KeyFrame& kf, bool stereo = false) { p.AddObservation(&kf, kf.hold(&p, stereo)); }

typedef ORB_SLAM2::MapGraphOf<KeyFrame, MapPoint, MapLine> Graph;

// the tables by hand -> replay -> the objects; or, on the device, the whole call
static std::vector<int32_t> cull(bool device, KeyFrame& current, const int32_t* t_mps, const int32_t* t_red, const int32_t* row_off, const int32_t* count, const uint8_t* flags)
{
    if (device) return ORB_SLAM2::KeyFrameCulling<KeyFrame, MapPoint, MapLine>(nullptr, &current, false);
    const std::vector<KeyFrame*> list = current.GetVectorCovisibleKeyFrames();
    Graph G(ORB_SLAM2::CullingSnapshot<KeyFrame, MapPoint>(list));
    std::vector<int32_t> idx, decision(list.size()), n_mps(list.size()), n_red(list.size());
    for (size_t j = 0; j < list.size(); ++j) idx.push_back(G.index_of(list[j]));
    const int rc = olf_keyframe_culling_replay(&G.graph(), &G.cull_view(), (int)list.size(), idx.data(), t_mps, t_red, row_off, count, flags, decision.data(), n_mps.data(),
                                               n_red.data(), nullptr, nullptr, nullptr, nullptr);
    expect(rc == OLF_OK, "olf_keyframe_culling_replay");
    ORB_SLAM2::ApplyKeyFrameCulling(list, decision.data());
    return decision;
}

int main(int argc, char** argv)
{
    const bool device = argc > 1 && !std::strcmp(argv[1], "device");
    {   // ---- loses redundancy ----
        KeyFrame kf[5];                                              // A, B, C, D and the current key frame
        MapPoint p[10];
        for (int i = 0; i < 10; ++i) for (int k = 0; k < 4; ++k) see(p[i], kf[k]);
        kf[4].mvpOrderedConnectedKeyFrames = {&kf[0], &kf[1]};
        const int32_t t_mps[2] = {10, 10}, t_red[2] = {10, 10}, row_off[3] = {0, 10, 20};
        int32_t count[20];
        uint8_t flags[20];
        for (int i = 0; i < 20; ++i) { count[i] = 3; flags[i] = 3; }
        {
            Graph G(ORB_SLAM2::CullingSnapshot<KeyFrame, MapPoint>(kf[4].GetVectorCovisibleKeyFrames()));
            const olf_cull_view& v = G.cull_view();
            expect(G.graph().n_kf == 4 && G.graph().n_mp == 10 && G.graph().mp_obs_offsets[10] == 40, "the snapshot holds A, B and the observers C, D");
            expect(v.mp_nobs[0] == 4 && v.mp_obs_slot[0] == 0 && v.mp_obs_slot[39] == 9 && v.kf_slot_octave[0] == 0 && v.kf_slot_depth[0] == 10.0f && v.kf_slot_stereo[0] == 0 &&
                   v.kf_th_depth[0] == 35.0f && v.kf_mode[0] == 0, "the view of the snapshot");
        }
        const std::vector<int32_t> decision = cull(device, kf[4], t_mps, t_red, row_off, count, flags);
        expect(decision == std::vector<int32_t>({1, 0}), "loses redundancy: A is culled, B is kept");
        expect(kf[0].isBad() && !kf[1].isBad() && !kf[2].isBad(), "loses redundancy: SetBadFlag ran on A alone");
        bool three = true;
        for (int i = 0; i < 10; ++i) three = three && p[i].Observations() == 3 && !p[i].isBad() && !p[i].mObservations.count(&kf[0]);
        expect(three, "loses redundancy: every point is left with three observations");
    }
    {   // ---- gains redundancy, with A protected first: mbNotErase gives decision 2 and changes nothing ----
        KeyFrame kf[6];                                              // A, B, C, D, E and the current key frame
        MapPoint b[9], q, a[10];
        for (int i = 0; i < 9; ++i) for (int k = 1; k < 5; ++k) see(b[i], kf[k]);
        see(q, kf[0], true); see(q, kf[1]);
        for (int i = 0; i < 10; ++i) { see(a[i], kf[0]); for (int k = 2; k < 5; ++k) see(a[i], kf[k]); }
        kf[5].mvpOrderedConnectedKeyFrames = {&kf[0], &kf[1]};
        const int32_t t_mps[2] = {11, 10}, t_red[2] = {10, 9}, row_off[3] = {0, 11, 21};
        int32_t count[21];
        uint8_t flags[21];
        for (int i = 0; i < 21; ++i) { count[i] = 3; flags[i] = 3; }
        count[0] = 1; flags[0] = 1; count[20] = 1; flags[20] = 1;   // q: A's first slot, B's last
        kf[0].mbNotErase = true;
        std::vector<int32_t> decision = cull(device, kf[5], t_mps, t_red, row_off, count, flags);
        expect(decision == std::vector<int32_t>({2, 0}) && kf[0].mbToBeErased && !kf[0].isBad() && !q.isBad() && q.Observations() == 3, "mbNotErase: decision 2, the map is as it was");
        kf[0].mbNotErase = false;
        decision = cull(device, kf[5], t_mps, t_red, row_off, count, flags);
        expect(decision == std::vector<int32_t>({1, 1}), "gains redundancy: A is culled, then B");
        expect(kf[0].isBad() && kf[1].isBad() && q.isBad() && kf[1].mvpMapPoints[9] == nullptr, "gains redundancy: q went bad and left B's slot");
        expect(b[0].Observations() == 3 && a[0].Observations() == 3 && !b[0].isBad() && !a[0].isBad(), "gains redundancy: the other points keep three observations");
    }
    if (failures) return 1;
    std::printf("ADAPTOR_CULLING_OK\n");
    return 0;
}
