// adaptor_connections.cpp -- ORB_SLAM2::ApplyConnections and ORB_SLAM2::UpdateConnections (include/orbline_reference_api.hpp) against stand-in types: the
// four key frames of tests/connections_scenes.py (slot_rules) and a fifth without slots, with th = 1.  Listed: key frames 1, 3 and 4, in that order.
//   without an argument  ApplyConnections on the outputs as tests/connections_scenes.py derives them (SLOT_RULES_EXPECTED for key frame 1; key frame 3 holds
//                        d, seen by 1 and 3, and b, which is bad: 1 gets 1); no device is needed.  Prints ADAPTOR_CONNECTIONS_OK.
//   with "device"        UpdateConnections itself: the snapshot, the host form on the device, then the same checks.
// The stand-in KeyFrame provides the one accessor the integrator adds (SetConnections, whose body is src/KeyFrame.cc:541-556).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../include/orbline_reference_api.hpp"

struct KeyFrame;
struct MapPoint {
    bool bad = false;
    std::map<KeyFrame*, size_t> obs;
    bool isBad() { return bad; }
    std::map<KeyFrame*, size_t> GetObservations() { return obs; }
};
struct MapLine {
    bool isBad() { return false; }
};
struct KeyFrame {
    long unsigned int mnId = 0;
    std::vector<MapPoint*> mps;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = true;
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens;
    int n_add_connection = 0;
    bool isBad() { return false; }
    std::vector<MapPoint*> GetMapPointMatches() { return mps; }
    std::vector<MapLine*> GetMapLineMatches() { return std::vector<MapLine*>(); }
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::set<KeyFrame*> GetChilds() { return mspChildrens; }
    KeyFrame* GetParent() { return mpParent; }
    void AddChild(KeyFrame* pKF) { mspChildrens.insert(pKF); }
    void AddConnection(KeyFrame* pKF, const int& weight) { mConnectedKeyFrameWeights[pKF] = weight; ++n_add_connection; }      // (UpdateBestCovisibles left out)
    void SetConnections(const std::map<KeyFrame*, int>& KFcounter, const std::vector<KeyFrame*>& vpOrdered, const std::vector<int>& vOrderedWeights)
    {
        mConnectedKeyFrameWeights = KFcounter;
        mvpOrderedConnectedKeyFrames = vpOrdered;
        mvOrderedWeights = vOrderedWeights;
        if (mbFirstConnection && mnId != 0) {
            mpParent = mvpOrderedConnectedKeyFrames.front();
            mpParent->AddChild(this);
            mbFirstConnection = false;
        }
    }
};

static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++failures; } }

int main(int argc, char** argv)
{
    KeyFrame kf[5];
    MapPoint a, b, c, d;
    for (int k = 0; k < 5; ++k) kf[k].mnId = k;
    a.obs[&kf[0]] = 0; a.obs[&kf[1]] = 0; a.obs[&kf[2]] = 1;
    b.obs[&kf[1]] = 2; b.obs[&kf[2]] = 0; b.obs[&kf[3]] = 1; b.bad = true;
    c.obs[&kf[1]] = 3;
    d.obs[&kf[1]] = 5; d.obs[&kf[3]] = 0;
    kf[0].mps = {&a}; kf[1].mps = {&a, nullptr, &b, &c, &a, &d}; kf[2].mps = {&b, &a}; kf[3].mps = {&d, &b};
    std::vector<KeyFrame*> all;
    for (int k = 0; k < 5; ++k) all.push_back(&kf[k]);
    const std::vector<KeyFrame*> list = {&kf[1], &kf[3], &kf[4]};

    typedef ORB_SLAM2::MapGraphOf<KeyFrame, MapPoint, MapLine> Graph;
    const Graph G(all);
    if (argc > 1 && !std::strcmp(argv[1], "device")) {
        ORB_SLAM2::UpdateConnections(G, list, 1);
    } else {
        const int32_t n_counted[3] = {3, 1, 0}, conn_off[4] = {0, 3, 4, 4}, conn_idx[4] = {0, 2, 3, 1}, conn_w[4] = {2, 2, 1, 1};
        const int32_t covis_off[4] = {0, 3, 4, 4}, covis_idx[4] = {2, 0, 3, 1}, covis_w[4] = {2, 2, 1, 1};
        ORB_SLAM2::ApplyConnections(G, list, n_counted, conn_off, conn_idx, conn_w, covis_off, covis_idx, covis_w);
        if (argc > 100) ORB_SLAM2::UpdateConnections(G, list);      // (instantiated with its default threshold)
    }

    // key frame 1: its own members, then key frame 3's reciprocal edge (weight 1, as it had)
    expect(kf[1].mvpOrderedConnectedKeyFrames == std::vector<KeyFrame*>({&kf[2], &kf[0], &kf[3]}) && kf[1].mvOrderedWeights == std::vector<int>({2, 2, 1}), "ordered row of key frame 1");
    expect(kf[1].mConnectedKeyFrameWeights == std::map<KeyFrame*, int>({{&kf[0], 2}, {&kf[2], 2}, {&kf[3], 1}}), "weights of key frame 1");
    expect(kf[1].mpParent == &kf[2] && !kf[1].mbFirstConnection && kf[2].mspChildrens.count(&kf[1]) == 1, "first connection: the parent of key frame 1 is the head of its row");
    expect(kf[1].n_add_connection == 1, "key frame 1 received one reciprocal edge, key frame 3's");
    // key frame 3: key frame 1's reciprocal edge first, then its own members replace the map
    expect(kf[3].mvpOrderedConnectedKeyFrames == std::vector<KeyFrame*>({&kf[1]}) && kf[3].mvOrderedWeights == std::vector<int>({1}), "ordered row of key frame 3");
    expect(kf[3].mConnectedKeyFrameWeights == std::map<KeyFrame*, int>({{&kf[1], 1}}) && kf[3].mpParent == &kf[1] && kf[1].mspChildrens.count(&kf[3]) == 1, "members of key frame 3");
    // the others: reciprocal edges only
    expect(kf[0].mConnectedKeyFrameWeights == std::map<KeyFrame*, int>({{&kf[1], 2}}) && kf[0].mvpOrderedConnectedKeyFrames.empty() && kf[0].mbFirstConnection, "key frame 0");
    expect(kf[2].mConnectedKeyFrameWeights == std::map<KeyFrame*, int>({{&kf[1], 2}}) && kf[2].mbFirstConnection && kf[2].mpParent == nullptr, "key frame 2");
    // key frame 4: KFcounter is empty, :501
    expect(kf[4].mbFirstConnection && kf[4].mConnectedKeyFrameWeights.empty() && kf[4].mpParent == nullptr && kf[4].n_add_connection == 0, "n_counted == 0 leaves the key frame untouched");

    if (failures) return 1;
    std::printf("ADAPTOR_CONNECTIONS_OK\n");
    return 0;
}
