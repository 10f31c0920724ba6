// connections_host_walk.cpp -- a plain C++ restatement of KeyFrame::UpdateConnections (src/KeyFrame.cc:446-557) with the reference's data structures, for
// tools/connections_latency.py to time beside the device entry: objects on the heap, a std::map<KeyFrame*, size_t> of observations per map point that is
// copied as GetObservations() copies it, a std::map<KeyFrame*, int> KFcounter, sort(vPairs) and the two std::lists.  The reciprocal AddConnection calls and the
// member writes are left out (the device entry leaves them to its caller too).  One host thread.  The tool compiles it with -O3 into a shared object.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <list>
#include <map>
#include <vector>

namespace {

struct KF;
struct MP {
    bool bad = false;
    std::map<KF*, size_t> mObservations;
    std::map<KF*, size_t> GetObservations() const { return mObservations; }
};
struct KF {
    long unsigned int mnId = 0;
    std::vector<MP*> mvpMapPoints;
};
struct Map {
    std::vector<KF*> kfs;
    std::vector<MP*> mps;
};

}  // namespace

extern "C" {

// the graph as olf_map_graph holds it (mp_obs_*, mp_bad, kf_mp_*), made into objects
void* cw_create(int n_kf, int n_mp, const int32_t* mp_obs_offsets, const int32_t* mp_obs_kf, const uint8_t* mp_bad, const int32_t* kf_mp_offsets, const int32_t* kf_mp_index)
{
    Map* m = new Map;
    for (int k = 0; k < n_kf; ++k) { m->kfs.push_back(new KF); m->kfs[k]->mnId = k; }
    for (int i = 0; i < n_mp; ++i) {
        m->mps.push_back(new MP);
        m->mps[i]->bad = mp_bad[i] != 0;
        for (int o = mp_obs_offsets[i]; o < mp_obs_offsets[i + 1]; ++o) m->mps[i]->mObservations[m->kfs[mp_obs_kf[o]]] = (size_t)o;
    }
    for (int k = 0; k < n_kf; ++k)
        for (int s = kf_mp_offsets[k]; s < kf_mp_offsets[k + 1]; ++s) m->kfs[k]->mvpMapPoints.push_back(kf_mp_index[s] >= 0 ? m->mps[kf_mp_index[s]] : nullptr);
    return m;
}

void cw_destroy(void* h)
{
    Map* m = (Map*)h;
    for (KF* k : m->kfs) delete k;
    for (MP* p : m->mps) delete p;
    delete m;
}

// UpdateConnections of the listed key frames, one after the other; returns the sum of the ordered rows' lengths and, in *check, of their weights
long cw_update_connections(void* h, const int32_t* list, int n_list, int th, long* check)
{
    Map* m = (Map*)h;
    long total = 0, sum = 0;
    for (int j = 0; j < n_list; ++j) {
        KF* self = m->kfs[list[j]];
        std::map<KF*, int> KFcounter;
        const std::vector<MP*> vpMP = self->mvpMapPoints;
        for (MP* pMP : vpMP) {
            if (!pMP) continue;
            if (pMP->bad) continue;
            const std::map<KF*, size_t> observations = pMP->GetObservations();
            for (std::map<KF*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit) {
                if (mit->first->mnId == self->mnId) continue;
                KFcounter[mit->first]++;
            }
        }
        if (KFcounter.empty()) continue;
        int nmax = 0;
        KF* pKFmax = nullptr;
        std::vector<std::pair<int, KF*> > vPairs;
        vPairs.reserve(KFcounter.size());
        for (std::map<KF*, int>::iterator mit = KFcounter.begin(); mit != KFcounter.end(); ++mit) {
            if (mit->second > nmax) { nmax = mit->second; pKFmax = mit->first; }
            if (mit->second >= th) vPairs.push_back(std::make_pair(mit->second, mit->first));
        }
        if (vPairs.empty()) vPairs.push_back(std::make_pair(nmax, pKFmax));
        std::sort(vPairs.begin(), vPairs.end());
        std::list<KF*> lKFs;
        std::list<int> lWs;
        for (size_t i = 0; i < vPairs.size(); ++i) { lKFs.push_front(vPairs[i].second); lWs.push_front(vPairs[i].first); }
        const std::vector<KF*> ordered(lKFs.begin(), lKFs.end());
        const std::vector<int> weights(lWs.begin(), lWs.end());
        total += (long)ordered.size();
        for (int w : weights) sum += w;
    }
    *check = sum;
    return total;
}

}  // extern "C"
