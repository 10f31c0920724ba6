// culling_host.cpp -- olf_keyframe_culling_replay: the sequential rest of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:632-696) on the host, from the
// tables of olf_keyframe_culling_tables_dev (culling_batch.hip).  The tables say what every listed key frame sees in the map as it stands; the replay walks
// the list in order and, after every key frame it culls, changes the later ones' counts as KeyFrame::SetBadFlag (src/KeyFrame.cc:647-649),
// MapPoint::EraseObservation (src/MapPoint.cc:123-149) and MapPoint::SetBadFlag (:163-180) change the map.  No context and no device.
#include <vector>
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_keyframe_culling_replay(const olf_map_graph* g, const olf_cull_view* v, int n_list, const int32_t* kf_list, const int32_t* table_n_mps,
                                           const int32_t* table_n_redundant, const int32_t* row_offsets, const int32_t* slot_count, const uint8_t* slot_flags,
                                           int32_t* decision, int32_t* n_mps, int32_t* n_redundant, int32_t* mp_nobs_out, uint8_t* mp_bad_out, int32_t* went_bad,
                                           int32_t* n_went_bad)
{
    const char* who = "olf_keyframe_culling_replay";
    size_t n_obs = 0, n_kmp = 0, n_rows = 0;
    bool ok = g && v && n_list >= 0 && g->n_kf >= 0 && g->n_mp >= 0 && table_n_mps && table_n_redundant && row_offsets && decision && n_mps && n_redundant;
    ok = ok && csr_ok(g->mp_obs_offsets, g->mp_obs_kf, g->n_mp, &n_obs) && csr_ok(g->kf_mp_offsets, g->kf_mp_index, g->n_kf, &n_kmp);
    ok = ok && ((g->mp_bad && v->mp_nobs) || !g->n_mp) && (v->mp_obs_slot || !n_obs) && ((v->kf_slot_octave && v->kf_slot_stereo) || !n_kmp) && (v->kf_mode || !g->n_kf);
    ok = ok && csr_ok(row_offsets, slot_count, n_list, &n_rows) && (slot_flags || !n_rows);
    const int n_kf = ok ? g->n_kf : 0, n_mp = ok ? g->n_mp : 0;
    std::vector<int> kf_of((size_t)(ok ? n_list : 0));
    for (int j = 0; ok && j < n_list; ++j) {                         // row_offsets is the running sum of the listed rows' lengths
        const int kf = kf_list ? kf_list[j] : j;
        kf_of[j] = kf >= 0 && kf < n_kf ? kf : -1;
        ok = row_offsets[j + 1] - row_offsets[j] == (kf_of[j] < 0 ? 0 : g->kf_mp_offsets[kf_of[j] + 1] - g->kf_mp_offsets[kf_of[j]]);
    }
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }

    // the working state: the counters and flags of the points, the removed observations, and the tables
    std::vector<int32_t> nobs(v->mp_nobs, v->mp_nobs + n_mp), count(slot_count, slot_count + n_rows), mps(table_n_mps, table_n_mps + n_list),
        red(table_n_redundant, table_n_redundant + n_list);
    std::vector<uint8_t> bad(g->mp_bad, g->mp_bad + n_mp), flags(slot_flags, slot_flags + n_rows), erased(n_obs, 0), culled((size_t)n_kf, 0);
    // point -> (listed position, slot of the row) of every counted slot, as a CSR built once
    std::vector<int32_t> holder_off((size_t)n_mp + 1, 0), holder_pos, holder_slot;
    for (int pass = 0; pass < 2; ++pass) {
        for (int j = 0; j < n_list; ++j) {
            if (kf_of[j] < 0) continue;
            const int32_t* row = g->kf_mp_index + g->kf_mp_offsets[kf_of[j]];
            for (int i = 0, n = row_offsets[j + 1] - row_offsets[j]; i < n; ++i) {
                if (!(flags[row_offsets[j] + i] & 1) || row[i] < 0 || row[i] >= n_mp) continue;
                if (pass == 0) ++holder_off[row[i] + 1];
                else { const int at = holder_off[row[i]]++; holder_pos[at] = j; holder_slot[at] = i; }
            }
        }
        if (pass == 0) {
            for (int p = 0; p < n_mp; ++p) holder_off[p + 1] += holder_off[p];
            holder_pos.resize(holder_off[n_mp]); holder_slot.resize(holder_off[n_mp]);
        } else {
            for (int p = n_mp; p > 0; --p) holder_off[p] = holder_off[p - 1];      // (the fill moved every begin to its end)
            holder_off[0] = 0;
        }
    }

    int n_bad = 0;
    for (int j = 0; j < n_list; ++j) {
        const int A = kf_of[j];
        decision[j] = 0; n_mps[j] = 0; n_redundant[j] = 0;
        if (A < 0 || v->kf_mode[A] == 2 || culled[A]) continue;      // mnId == 0, :643; a key frame that is gone is not in the reference's list a second time
        n_mps[j] = mps[j]; n_redundant[j] = red[j];
        if (!((double)red[j] > 0.9 * (double)mps[j])) continue;      // :693
        if (v->kf_mode[A] == 1) { decision[j] = 2; continue; }       // mbNotErase: mbToBeErased = true, src/KeyFrame.cc:637-641
        decision[j] = 1;
        culled[A] = 1;
        const int a0 = g->kf_mp_offsets[A], a_len = g->kf_mp_offsets[A + 1] - a0;
        for (int i = 0; i < a_len; ++i) {                            // mvpMapPoints[i]->EraseObservation(this), src/KeyFrame.cc:647-649
            const int p = g->kf_mp_index[a0 + i];
            if (p < 0 || p >= n_mp || bad[p]) continue;              // (a bad point's observations are cleared: mObservations.count(pKF) == 0)
            int at = -1;
            for (int o = g->mp_obs_offsets[p]; o < g->mp_obs_offsets[p + 1] && at < 0; ++o)
                if (g->mp_obs_kf[o] == A && !erased[o] && v->mp_obs_slot[o] >= 0 && v->mp_obs_slot[o] < a_len) at = o;
            if (at < 0) continue;
            const int s = v->mp_obs_slot[at];                        // int idx = mObservations[pKF], src/MapPoint.cc:130
            erased[at] = 1;
            nobs[p] -= v->kf_slot_stereo[a0 + s] ? 2 : 1;            // :131-134
            const int oct_a = v->kf_slot_octave[a0 + s];
            const bool goes_bad = nobs[p] <= 2;                      // :142-148
            if (goes_bad) { bad[p] = 1; if (went_bad) went_bad[n_bad] = p; ++n_bad; }
            for (int h = holder_off[p]; h < holder_off[p + 1]; ++h) {
                const int pos = holder_pos[h];
                if (pos <= j) continue;                              // (decided)
                const int at_slot = row_offsets[pos] + holder_slot[h];
                const bool was_red = (flags[at_slot] & 2) != 0;
                if (goes_bad) {                                      // the slot no longer counts, :656
                    --mps[pos]; red[pos] -= was_red;
                    flags[at_slot] = 0;
                    continue;
                }
                const int own = v->kf_slot_octave[g->kf_mp_offsets[kf_of[pos]] + holder_slot[h]];
                if (kf_of[pos] != A && oct_a <= own + 1) --count[at_slot];      // the observation qualified there, :677
                const bool is_red = nobs[p] > 3 && count[at_slot] >= 3;      // :665, :684
                red[pos] += (int)is_red - (int)was_red;
                flags[at_slot] = (uint8_t)(1 | (is_red ? 2 : 0));
            }
        }
    }
    if (mp_nobs_out) std::copy(nobs.begin(), nobs.end(), mp_nobs_out);
    if (mp_bad_out) std::copy(bad.begin(), bad.end(), mp_bad_out);
    if (n_went_bad) *n_went_bad = n_bad;
    return OLF_OK;
}
