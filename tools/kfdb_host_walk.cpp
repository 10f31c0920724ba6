// kfdb_host_walk.cpp -- a plain C++ restatement of the reference's own place-recognition walk, for tools/kfdb_latency.py to time beside the device entries:
// KeyFrameDatabase::add and the two relocalisation forms (src/KeyFrameDatabase.cc:46-55, :402-667) with the reference's data structures -- a std::list per
// word as the inverted file, std::map BowVectors, the per-key-frame members -- and L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).
// One host thread.  The tool compiles it with -O3 into a shared object; key frames are returned by index.
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <vector>

namespace {

typedef std::map<unsigned, double> BowVector;

struct KF {
    int index;
    BowVector mBowVec, mBowVec_l;
    long mnRelocQuery = 0, mnRelocQuery_l = 0;
    int mnRelocWords = 0, mnRelocWords_l = 0;
    float mRelocScore = 0, mRelocScore_l = 0, mRelocScore_pl = 0;
    std::vector<KF*> best;          // GetBestCovisibilityKeyFrames(10)
};

struct DB {
    std::vector<std::list<KF*>> inv, inv_l;
    std::vector<KF*> kfs;
};

double score(const BowVector& v1, const BowVector& v2)
{
    BowVector::const_iterator a = v1.begin(), b = v2.begin();
    double s = 0;
    while (a != v1.end() && b != v2.end()) {
        if (a->first == b->first) { s += std::fabs(a->second - b->second) - std::fabs(a->second) - std::fabs(b->second); ++a; ++b; }
        else if (a->first < b->first) a = v1.lower_bound(b->first);
        else b = v2.lower_bound(a->first);
    }
    return -s / 2.0;
}

BowVector bow(const int32_t* ids, const double* vals, int n)
{
    BowVector v;
    for (int i = 0; i < n; ++i) v.insert(v.end(), BowVector::value_type((unsigned)ids[i], vals[i]));
    return v;
}

int retain(const std::list<std::pair<float, KF*>>& acc, float best, int32_t* out)
{
    const float minScoreToRetain = 0.75f * best;
    std::set<KF*> added;
    int n = 0;
    for (const auto& e : acc)
        if (e.first > minScoreToRetain && !added.count(e.second)) { out[n++] = e.second->index; added.insert(e.second); }
    return n;
}

}  // namespace

extern "C" {

void* hw_create(int n_words, int n_words_l)
{
    DB* d = new DB;
    d->inv.resize(n_words); d->inv_l.resize(n_words_l);
    return d;
}

void hw_destroy(void* h)
{
    DB* d = (DB*)h;
    for (KF* k : d->kfs) delete k;
    delete d;
}

int hw_add(void* h, const int32_t* ids, const double* vals, int n, const int32_t* ids_l, const double* vals_l, int n_l)
{
    DB* d = (DB*)h;
    KF* k = new KF;
    k->index = (int)d->kfs.size();
    k->mBowVec = bow(ids, vals, n); k->mBowVec_l = bow(ids_l, vals_l, n_l);
    for (const auto& e : k->mBowVec) d->inv[e.first].push_back(k);
    for (const auto& e : k->mBowVec_l) d->inv_l[e.first].push_back(k);
    d->kfs.push_back(k);
    return k->index;
}

void hw_set_neighbours(void* h, int kf, const int32_t* nb, int n)
{
    DB* d = (DB*)h;
    d->kfs[kf]->best.clear();
    for (int i = 0; i < n; ++i) if (nb[i] >= 0) d->kfs[kf]->best.push_back(d->kfs[nb[i]]);
}

// DetectRelocalizationCandidates, :402-512
int hw_reloc(void* h, long id, const int32_t* ids, const double* vals, int n, int32_t* out)
{
    DB* d = (DB*)h;
    const BowVector q = bow(ids, vals, n);
    std::list<KF*> sharing;
    for (const auto& e : q)
        for (KF* k : d->inv[e.first]) {
            if (k->mnRelocQuery != id) { k->mnRelocWords = 0; k->mnRelocQuery = id; sharing.push_back(k); }
            k->mnRelocWords++;
        }
    if (sharing.empty()) return 0;
    int maxCommonWords = 0;
    for (KF* k : sharing) if (k->mnRelocWords > maxCommonWords) maxCommonWords = k->mnRelocWords;
    const int minCommonWords = maxCommonWords * 0.8f;
    std::list<std::pair<float, KF*>> scored, acc;
    for (KF* k : sharing)
        if (k->mnRelocWords > minCommonWords) { const float si = score(q, k->mBowVec); k->mRelocScore = si; scored.push_back(std::make_pair(si, k)); }
    if (scored.empty()) return 0;
    float bestAcc = 0;
    for (const auto& e : scored) {
        float bestScore = e.first, accScore = bestScore;
        KF* bestKF = e.second;
        for (KF* k2 : e.second->best) {
            if (k2->mnRelocQuery != id) continue;
            accScore += k2->mRelocScore;
            if (k2->mRelocScore > bestScore) { bestKF = k2; bestScore = k2->mRelocScore; }
        }
        acc.push_back(std::make_pair(accScore, bestKF));
        if (accScore > bestAcc) bestAcc = accScore;
    }
    return retain(acc, bestAcc, out);
}

// DetectRelocalizationCandidatesWithLine, :514-667 (the std::set in index order: the index stands for the address)
int hw_reloc_line(void* h, long id, const int32_t* ids, const double* vals, int n, const int32_t* ids_l, const double* vals_l, int n_l, int np, int nl,
                  int32_t* out)
{
    DB* d = (DB*)h;
    const BowVector q = bow(ids, vals, n), ql = bow(ids_l, vals_l, n_l);
    std::list<KF*> sharing, sharing_l;
    for (const auto& e : q)
        for (KF* k : d->inv[e.first]) {
            if (k->mnRelocQuery != id) { k->mnRelocWords = 0; k->mnRelocQuery = id; sharing.push_back(k); }
            k->mnRelocWords++;
        }
    for (const auto& e : ql)
        for (KF* k : d->inv_l[e.first]) {
            if (k->mnRelocQuery_l != id) { k->mnRelocWords_l = 0; k->mnRelocQuery_l = id; sharing_l.push_back(k); }
            k->mnRelocWords_l++;
        }
    if (sharing.empty() && sharing_l.empty()) return 0;
    int maxCommonWords = 0, maxCommonWords_l = 0;
    for (KF* k : sharing) if (k->mnRelocWords > maxCommonWords) maxCommonWords = k->mnRelocWords;
    for (KF* k : sharing_l) if (k->mnRelocWords_l > maxCommonWords_l) maxCommonWords_l = k->mnRelocWords_l;
    const int minCommonWords = maxCommonWords * 0.8f, minCommonWords_l = maxCommonWords_l * 0.8f;
    auto by_index = [](const KF* a, const KF* b) { return a->index < b->index; };
    std::set<KF*, decltype(by_index)> both(by_index);
    for (KF* k : sharing) if (k->mnRelocWords > minCommonWords) both.insert(k);
    for (KF* k : sharing_l) if (k->mnRelocWords_l > minCommonWords_l) both.insert(k);
    std::list<std::pair<float, KF*>> scored, acc;
    for (KF* k : both) {
        const float spi = score(q, k->mBowVec), sli = score(ql, k->mBowVec_l);
        k->mRelocScore = spi; k->mRelocScore_l = sli; k->mRelocScore_pl = (spi * np + sli * nl) / (np + nl);
        scored.push_back(std::make_pair(k->mRelocScore_pl, k));
    }
    if (scored.empty()) return 0;
    float bestAcc = 0;
    for (const auto& e : scored) {
        float bestScore = e.first, accScore = bestScore;
        KF* bestKF = e.second;
        for (KF* k2 : e.second->best) {
            if (!(k2->mnRelocQuery == id && k2->mnRelocQuery_l == id)) continue;
            accScore += k2->mRelocScore_pl;
            if (k2->mRelocScore_pl > bestScore) { bestKF = k2; bestScore = k2->mRelocScore_pl; }
        }
        acc.push_back(std::make_pair(accScore, bestKF));
        if (accScore > bestAcc) bestAcc = accScore;
    }
    return retain(acc, bestAcc, out);
}

}  // extern "C"
