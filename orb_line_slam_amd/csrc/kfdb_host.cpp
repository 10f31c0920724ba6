// kfdb_host.cpp -- the sequential, stateful half of KeyFrameDatabase's four Detect members (src/KeyFrameDatabase.cc:107-667): everything behind the walk of
// the inverted file and the calls of mpVoc->score, whose results arrive as tables (kfdb.hip).  Plain host C++: no HIP header and no HIP call, so that
// tests/kfdb_select_main.cpp links it into a stand-alone program.
//
// What the tables stand for.  For query q and slot k, common[q][k] is the value mnLoopWords / mnRelocWords has after the walk and first[q][k] the word at
// which the walk met k first.  "pKFi->mnRelocQuery == F->mnId" after the walk is "common > 0"; in the loop forms "mnLoopQuery == pKF->mnId" is "common > 0 and
// k is not connected to the query" (:124-131).  lKFsSharingWords is in first-encounter order: ascending (first, slot), the slot being the position in the
// word's posting list.  The std::set of the WithLine forms iterates in ascending slot.
#include <algorithm>
#include "kfdb.hpp"

namespace olf {

namespace {

struct Row { const int32_t *common, *first; const double* score; };
Row row_of(const olf_kfdb_tables* t, int q, int n_slots)
{
    const size_t o = (size_t)q * n_slots;
    return {t->common + o, t->first + o, t->score + o};
}

// lKFsSharingWords (:110-135, :404-425) and the thresholds behind it (:144-151, :431-438): the list in order, minCommonWords
int sharing_list(const Row& r, int n_slots, const std::vector<uint8_t>* connected, std::vector<int32_t>& list)
{
    list.clear();
    for (int k = 0; k < n_slots; ++k) if (r.common[k] > 0 && !(connected && (*connected)[k])) list.push_back(k);
    std::sort(list.begin(), list.end(), [&](int32_t a, int32_t b) { return r.first[a] != r.first[b] ? r.first[a] < r.first[b] : a < b; });
    int maxCommonWords = 0;
    for (int32_t k : list) if (r.common[k] > maxCommonWords) maxCommonWords = r.common[k];
    return (int)(maxCommonWords * 0.8f);
}

// (spi*np+sli*nl)/(np+nl) in float, :338, :609
float combined(float spi, float sli, int np, int nl) { return (spi * np + sli * nl) / (np + nl); }

struct Scored { float score; int32_t kf; };

// :206-224, :378-396, :492-509, :647-664
void retain(const std::vector<Scored>& acc, float bestAccScore, std::vector<uint8_t>& added, std::vector<int32_t>& cand)
{
    const float minScoreToRetain = 0.75f * bestAccScore;
    const size_t base = cand.size();
    for (const Scored& s : acc) {
        if (s.score > minScoreToRetain && !added[s.kf]) { cand.push_back(s.kf); added[s.kf] = 1; }
    }
    for (size_t i = base; i < cand.size(); ++i) added[cand[i]] = 0;
}

}  // namespace

int kfdb_select(const SelectArgs& a, bool has_lines, KfdbState& st_io, std::vector<int32_t>& cand_off, std::vector<int32_t>& cand)
{
    const bool loop = a.form == OLF_KFDB_LOOP || a.form == OLF_KFDB_LOOP_LINE;
    const bool line = a.form == OLF_KFDB_LOOP_LINE || a.form == OLF_KFDB_RELOC_LINE;
    const int n = a.n_slots;
    {
        int64_t last = loop ? st_io.last_loop_id : st_io.last_reloc_id;
        for (int q = 0; q < a.n_queries; ++q) {
            if (a.query_ids[q] <= last) { set_error("olf_kfdb_select: a query id must be > 0 and greater than every earlier query id of its family"); return OLF_ERR_INVALID; }
            last = a.query_ids[q];
        }
        for (int i = 0; i < a.nb_off[n]; ++i) if (a.nb_slots[i] >= n) { set_error("olf_kfdb_select: a neighbour slot is >= n_slots"); return OLF_ERR_INVALID; }
    }
    KfdbState& st = st_io;
    cand.clear();
    cand_off.assign(a.n_queries + 1, 0);
    std::vector<uint8_t> connected(n), added(n, 0), inP(n), inL(n);
    std::vector<int32_t> lP, lL;
    std::vector<Scored> lScoreAndMatch, lAcc;
    std::vector<float> pl(n);
    for (int q = 0; q < a.n_queries; ++q) {
        (loop ? st.last_loop_id : st.last_reloc_id) = a.query_ids[q];
        cand_off[q + 1] = (int32_t)cand.size();
        if (line && !has_lines) continue;                                   // :232-235, :516-519
        const Row rp = row_of(a.tp, q, n);
        const std::vector<uint8_t>* conn = nullptr;
        if (loop) {                                                         // spConnectedKeyFrames, :109, :237
            std::fill(connected.begin(), connected.end(), 0);
            if (a.conn_off) for (int i = a.conn_off[q]; i < a.conn_off[q + 1]; ++i) if (a.conn_slots[i] >= 0 && a.conn_slots[i] < n) connected[a.conn_slots[i]] = 1;
            conn = &connected;
        }
        const int minCommonWords = sharing_list(rp, n, conn, lP);
        const float minScore = loop ? a.min_score[q] : 0.f;
        lScoreAndMatch.clear();
        lAcc.clear();
        float bestAccScore = loop ? minScore : 0.f;                         // :176, :347, :462, :617
        if (!line) {
            if (lP.empty()) continue;                                       // :138, :427
            for (int32_t k : lP) {                                          // :156-170, :445-456
                if (rp.common[k] > minCommonWords) {
                    const float si = (float)rp.score[k];
                    if (loop) { if (si >= minScore) lScoreAndMatch.push_back({si, k}); }
                    else { st.reloc_score[k] = si; lScoreAndMatch.push_back({si, k}); }
                }
            }
            for (const Scored& s : lScoreAndMatch) {                        // :179-204, :465-490
                float bestScore = s.score, accScore = s.score;
                int32_t pBestKF = s.kf;
                for (int i = a.nb_off[s.kf]; i < a.nb_off[s.kf + 1]; ++i) {
                    const int32_t k2 = a.nb_slots[i];
                    if (k2 < 0) continue;
                    float s2;
                    if (loop) {                                             // :190: scored in this very query
                        if (!(rp.common[k2] > 0 && !connected[k2] && rp.common[k2] > minCommonWords)) continue;
                        s2 = (float)rp.score[k2];
                    } else {                                                // :476: shares a word; mRelocScore may be an earlier query's, or the constructor's 0
                        if (!(rp.common[k2] > 0)) continue;
                        s2 = st.reloc_score[k2];
                    }
                    accScore += s2;
                    if (s2 > bestScore) { pBestKF = k2; bestScore = s2; }
                }
                lAcc.push_back({accScore, pBestKF});
                if (accScore > bestAccScore) bestAccScore = accScore;
            }
        } else {
            const Row rl = row_of(a.tl, q, n);
            const int minCommonWords_l = sharing_list(rl, n, conn, lL);
            if (lP.empty() && lL.empty()) continue;                         // :287, :562
            std::fill(inP.begin(), inP.end(), 0);
            std::fill(inL.begin(), inL.end(), 0);
            for (int32_t k : lP) inP[k] = 1;
            for (int32_t k : lL) inL[k] = 1;
            const int np = a.np[q], nl = a.nl[q];
            for (int32_t k = 0; k < n; ++k) {                               // sKFsSharingWords_pl in set order, :307-341, :582-611
                if (!((inP[k] && rp.common[k] > minCommonWords) || (inL[k] && rl.common[k] > minCommonWords_l))) continue;
                const float spi = (float)rp.score[k], sli = (float)rl.score[k];
                pl[k] = combined(spi, sli, np, nl);
                if (loop) { if (pl[k] > minScore) lScoreAndMatch.push_back({pl[k], k}); }
                else {
                    st.reloc_score[k] = spi; st.reloc_score_l[k] = sli; st.reloc_score_pl[k] = pl[k];
                    lScoreAndMatch.push_back({pl[k], k});
                }
            }
            for (const Scored& s : lScoreAndMatch) {                        // :350-376, :620-645
                float bestScore = s.score, accScore = s.score;
                int32_t pBestKF = s.kf;
                for (int i = a.nb_off[s.kf]; i < a.nb_off[s.kf + 1]; ++i) {
                    const int32_t k2 = a.nb_slots[i];
                    if (k2 < 0) continue;
                    float s2;
                    if (loop) {                                             // :361-362: in both lists above both thresholds, hence scored in this query
                        if (!(inP[k2] && rp.common[k2] > minCommonWords && inL[k2] && rl.common[k2] > minCommonWords_l)) continue;
                        s2 = pl[k2];
                    } else {                                                // :631
                        if (!(inP[k2] && inL[k2])) continue;
                        s2 = st.reloc_score_pl[k2];
                    }
                    accScore += s2;
                    if (s2 > bestScore) { pBestKF = k2; bestScore = s2; }
                }
                lAcc.push_back({accScore, pBestKF});
                if (accScore > bestAccScore) bestAccScore = accScore;
            }
        }
        retain(lAcc, bestAccScore, added, cand);
        cand_off[q + 1] = (int32_t)cand.size();
    }
    return OLF_OK;
}

}  // namespace olf

extern "C" {

int olf_kfdb_select(olf_kfdb* db, int form, int n_queries, const int64_t* query_ids, const int32_t* np, const int32_t* nl, const float* min_score,
                    const int32_t* conn_off, const int32_t* conn_slots, const int32_t* nb_off, const int32_t* nb_slots, int n_slots,
                    const olf_kfdb_tables* tp, const olf_kfdb_tables* tl, int32_t* cand_off, int32_t* cand_slots, int cand_capacity)
{
    const bool loop = form == OLF_KFDB_LOOP || form == OLF_KFDB_LOOP_LINE, line = form == OLF_KFDB_LOOP_LINE || form == OLF_KFDB_RELOC_LINE;
    auto whole = [](const olf_kfdb_tables* t) { return t && t->common && t->first && t->score; };
    if (!db || form < OLF_KFDB_LOOP || form > OLF_KFDB_RELOC_LINE || n_queries < 0 || n_slots < 0 || cand_capacity < 0 || !cand_off || !nb_off ||
        (cand_capacity > 0 && !cand_slots) || (conn_off && !conn_slots) ||
        (n_queries > 0 && (!query_ids || (loop && !min_score) || (line && (!np || !nl)) || (n_slots > 0 && (!whole(tp) || (line && !whole(tl))))))) {
        olf::set_error("olf_kfdb_select: bad argument"); return OLF_ERR_INVALID;
    }
    if (n_slots != db->n_slots) { olf::set_error("olf_kfdb_select: n_slots is not the database's"); return OLF_ERR_INVALID; }
    if (nb_off[0] != 0) { olf::set_error("olf_kfdb_select: nb_off must start at 0"); return OLF_ERR_INVALID; }
    for (int k = 0; k < n_slots; ++k) if (nb_off[k + 1] < nb_off[k]) { olf::set_error("olf_kfdb_select: nb_off must not decrease"); return OLF_ERR_INVALID; }
    if (nb_off[n_slots] > 0 && !nb_slots) { olf::set_error("olf_kfdb_select: bad argument"); return OLF_ERR_INVALID; }
    if (conn_off) for (int q = 0; q < n_queries; ++q) if (conn_off[q] < 0 || conn_off[q + 1] < conn_off[q]) { olf::set_error("olf_kfdb_select: conn_off must not decrease"); return OLF_ERR_INVALID; }
    const olf::SelectArgs a = {form, n_queries, query_ids, np, nl, min_score, conn_off, conn_slots, nb_off, nb_slots, n_slots, tp, tl};
    olf::KfdbState st = db->st;
    std::vector<int32_t> off, cand;
    const int rc = olf::kfdb_select(a, db->v[1].n_words > 0, st, off, cand);
    if (rc != OLF_OK) return rc;
    if (cand.size() > (size_t)cand_capacity) { olf::set_error("olf_kfdb_select: more candidates than cand_capacity"); return OLF_ERR_CAPACITY; }
    db->st = st;
    std::copy(off.begin(), off.end(), cand_off);
    std::copy(cand.begin(), cand.end(), cand_slots);
    return OLF_OK;
}

int olf_kfdb_size(const olf_kfdb* db, int32_t* n_slots, int32_t* n_live)
{
    if (!db) { olf::set_error("olf_kfdb_size: null database"); return OLF_ERR_INVALID; }
    if (n_slots) *n_slots = db->n_slots;
    if (n_live) *n_live = db->n_live;
    return OLF_OK;
}

int olf_kfdb_state(const olf_kfdb* db, float* reloc_score, float* reloc_score_l, float* reloc_score_pl)
{
    if (!db) { olf::set_error("olf_kfdb_state: null database"); return OLF_ERR_INVALID; }
    if (reloc_score) std::copy(db->st.reloc_score.begin(), db->st.reloc_score.end(), reloc_score);
    if (reloc_score_l) std::copy(db->st.reloc_score_l.begin(), db->st.reloc_score_l.end(), reloc_score_l);
    if (reloc_score_pl) std::copy(db->st.reloc_score_pl.begin(), db->st.reloc_score_pl.end(), reloc_score_pl);
    return OLF_OK;
}

}  // extern "C"
