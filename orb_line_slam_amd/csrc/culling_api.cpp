// culling_api.cpp -- the host-pointer forms of culling_batch.hip: olf_keyframe_culling (upload, tables, download, replay: culling_host.cpp),
// olf_tracked_map_points and olf_map_point_culling.  Each checks what the device form leaves to its caller (the shape of the CSR pairs it reads), stages the
// arrays and the outputs in one carve and runs the same kernels.
#include <vector>
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_keyframe_culling(olf_ctx* c, const olf_map_graph* g, const olf_cull_view* v, int n_list, const int32_t* kf_list, int monocular, int32_t* decision,
                                    int32_t* n_mps, int32_t* n_redundant, int32_t* table_n_mps, int32_t* table_n_redundant, uint8_t* table_redundant,
                                    int32_t* mp_nobs_out, uint8_t* mp_bad_out, int32_t* went_bad, int32_t* n_went_bad)
{
    const char* who = "olf_keyframe_culling";
    size_t n_obs = 0, n_kmp = 0;
    bool ok = c && g && v && n_list >= 0 && g->n_kf >= 0 && g->n_mp >= 0 && decision && n_mps && n_redundant;
    ok = ok && csr_ok(g->mp_obs_offsets, g->mp_obs_kf, g->n_mp, &n_obs) && csr_ok(g->kf_mp_offsets, g->kf_mp_index, g->n_kf, &n_kmp);
    ok = ok && ((g->mp_bad && v->mp_nobs) || !g->n_mp) && (v->mp_obs_slot || !n_obs) && ((v->kf_slot_octave && v->kf_slot_depth && v->kf_slot_stereo) || !n_kmp) &&
         ((v->kf_th_depth && v->kf_mode) || !g->n_kf);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n_went_bad) *n_went_bad = 0;
    if (n_list == 0) {
        if (mp_nobs_out) std::copy(v->mp_nobs, v->mp_nobs + g->n_mp, mp_nobs_out);
        if (mp_bad_out) std::copy(g->mp_bad, g->mp_bad + g->n_mp, mp_bad_out);
        return OLF_OK;
    }

    const size_t nl = (size_t)n_list, nk = (size_t)g->n_kf, nm = (size_t)g->n_mp;
    long long total = 0;                                             // the listed rows, which size the slot arrays
    for (int j = 0; j < n_list; ++j) {
        const int kf = kf_list ? kf_list[j] : j;
        if (kf >= 0 && kf < g->n_kf) total += g->kf_mp_offsets[kf + 1] - g->kf_mp_offsets[kf];
    }
    if (total > 0x7fffffffLL) { set_error(std::string(who) + ": more than 2^31 listed slots"); return OLF_ERR_CAPACITY; }
    const size_t ns = (size_t)total;

    olf_map_graph d = {};                                            // (only these fields are read)
    olf_cull_view dv = {};
    d.n_kf = g->n_kf; d.n_mp = g->n_mp;
    int32_t *d_obs_off, *d_obs_kf, *d_obs_slot, *d_nobs, *d_kmp_off, *d_kmp, *d_list = nullptr, *d_nm, *d_nr, *d_row, *d_cnt;
    uint8_t *d_mp_bad, *d_oct, *d_red, *d_flags;
    float *d_depth, *d_th;
    HostCall h(c, who);
    h.add(&d_obs_off, nm + 1); h.add(&d_obs_kf, n_obs + 1); h.add(&d_obs_slot, n_obs + 1); h.add(&d_nobs, nm + 1); h.add(&d_mp_bad, nm + 1);
    h.add(&d_kmp_off, nk + 1); h.add(&d_kmp, n_kmp + 1); h.add(&d_oct, n_kmp + 1); h.add(&d_depth, n_kmp + 1); h.add(&d_th, nk + 1);
    if (kf_list) h.add(&d_list, nl);
    h.add(&d_nm, nl); h.add(&d_nr, nl); h.add(&d_red, nl); h.add(&d_row, nl + 1); h.add(&d_cnt, ns + 1); h.add(&d_flags, ns + 1);
    OLF_TRY(h.bind(SCRATCH_STAGE));

    OLF_TRY(h.up(d_obs_off, g->mp_obs_offsets, (nm + 1) * 4)); OLF_TRY(h.up(d_obs_kf, g->mp_obs_kf, n_obs * 4)); OLF_TRY(h.up(d_obs_slot, v->mp_obs_slot, n_obs * 4));
    OLF_TRY(h.up(d_nobs, v->mp_nobs, nm * 4)); OLF_TRY(h.up(d_mp_bad, g->mp_bad, nm));
    OLF_TRY(h.up(d_kmp_off, g->kf_mp_offsets, (nk + 1) * 4)); OLF_TRY(h.up(d_kmp, g->kf_mp_index, n_kmp * 4)); OLF_TRY(h.up(d_oct, v->kf_slot_octave, n_kmp));
    OLF_TRY(h.up(d_depth, v->kf_slot_depth, n_kmp * 4)); OLF_TRY(h.up(d_th, v->kf_th_depth, nk * 4));
    if (kf_list) OLF_TRY(h.up(d_list, kf_list, nl * 4));
    d.mp_obs_offsets = d_obs_off; d.mp_obs_kf = d_obs_kf; d.mp_bad = d_mp_bad; d.kf_mp_offsets = d_kmp_off; d.kf_mp_index = d_kmp;
    dv.mp_obs_slot = d_obs_slot; dv.mp_nobs = d_nobs; dv.kf_slot_octave = d_oct; dv.kf_slot_depth = d_depth; dv.kf_th_depth = d_th;

    OLF_TRY(olf_keyframe_culling_tables_dev(c, &d, &dv, n_list, d_list, monocular, d_nm, d_nr, d_red, d_row, d_cnt, d_flags, (int)ns, h.stream()));

    std::vector<int32_t> t_mps(nl), t_red(nl), row(nl + 1), cnt(ns + 1);
    std::vector<uint8_t> t_flag(nl), flags(ns + 1);
    OLF_TRY(h.down(t_mps.data(), d_nm, nl * 4)); OLF_TRY(h.down(t_red.data(), d_nr, nl * 4)); OLF_TRY(h.down(t_flag.data(), d_red, nl));
    OLF_TRY(h.down(row.data(), d_row, (nl + 1) * 4)); OLF_TRY(h.down(cnt.data(), d_cnt, ns * 4)); OLF_TRY(h.down(flags.data(), d_flags, ns));
    const int status_rc = h.finish_status();
    if (status_rc != OLF_OK && status_rc != OLF_ERR_CAPACITY) return status_rc;
    if (table_n_mps) std::copy(t_mps.begin(), t_mps.end(), table_n_mps);
    if (table_n_redundant) std::copy(t_red.begin(), t_red.end(), table_n_redundant);
    if (table_redundant) std::copy(t_flag.begin(), t_flag.end(), table_redundant);
    OLF_TRY(olf_keyframe_culling_replay(g, v, n_list, kf_list, t_mps.data(), t_red.data(), row.data(), cnt.data(), flags.data(), decision, n_mps, n_redundant, mp_nobs_out,
                                        mp_bad_out, went_bad, n_went_bad));
    return status_rc;                                                // (a malformed index: the outputs are complete, the code and the message are the bit's)
}

extern "C" int olf_tracked_map_points(olf_ctx* c, const olf_map_graph* g, const int32_t* mp_nobs, const int32_t* ml_nobs, int n_list, const int32_t* kf_list,
                                      int min_obs_points, int min_obs_lines, int32_t* n_points, int32_t* n_lines)
{
    const char* who = "olf_tracked_map_points";
    size_t n_kmp = 0, n_kml = 0;
    bool ok = c && g && n_list >= 0 && n_points && n_lines && g->n_kf >= 0 && g->n_mp >= 0 && g->n_ml >= 0;
    ok = ok && csr_ok(g->kf_mp_offsets, g->kf_mp_index, g->n_kf, &n_kmp) && (g->mp_bad || !g->n_mp) && (mp_nobs || min_obs_points <= 0 || !g->n_mp);
    const bool lines = ok && g->kf_ml_offsets;
    ok = ok && (!lines || (csr_ok(g->kf_ml_offsets, g->kf_ml_index, g->n_kf, &n_kml) && (g->ml_bad || !g->n_ml) && (ml_nobs || min_obs_lines <= 0 || !g->n_ml)));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n_list == 0) return OLF_OK;

    const size_t nl = (size_t)n_list, nk = (size_t)g->n_kf, nm = (size_t)g->n_mp, nml = (size_t)g->n_ml;
    olf_map_graph d = {};
    d.n_kf = g->n_kf; d.n_mp = g->n_mp; d.n_ml = g->n_ml;
    int32_t *d_kmp_off, *d_kmp, *d_kml_off = nullptr, *d_kml = nullptr, *d_nobs = nullptr, *d_lnobs = nullptr, *d_list = nullptr, *d_np, *d_nlines;
    uint8_t *d_mp_bad, *d_ml_bad = nullptr;
    HostCall h(c, who);
    h.add(&d_kmp_off, nk + 1); h.add(&d_kmp, n_kmp + 1); h.add(&d_mp_bad, nm + 1);
    if (mp_nobs) h.add(&d_nobs, nm + 1);
    if (lines) { h.add(&d_kml_off, nk + 1); h.add(&d_kml, n_kml + 1); h.add(&d_ml_bad, nml + 1); if (ml_nobs) h.add(&d_lnobs, nml + 1); }
    if (kf_list) h.add(&d_list, nl);
    h.add(&d_np, nl); h.add(&d_nlines, nl);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(d_kmp_off, g->kf_mp_offsets, (nk + 1) * 4)); OLF_TRY(h.up(d_kmp, g->kf_mp_index, n_kmp * 4)); OLF_TRY(h.up(d_mp_bad, g->mp_bad, nm));
    if (mp_nobs) OLF_TRY(h.up(d_nobs, mp_nobs, nm * 4));
    if (lines) {
        OLF_TRY(h.up(d_kml_off, g->kf_ml_offsets, (nk + 1) * 4)); OLF_TRY(h.up(d_kml, g->kf_ml_index, n_kml * 4)); OLF_TRY(h.up(d_ml_bad, g->ml_bad, nml));
        if (ml_nobs) OLF_TRY(h.up(d_lnobs, ml_nobs, nml * 4));
    }
    if (kf_list) OLF_TRY(h.up(d_list, kf_list, nl * 4));
    d.kf_mp_offsets = d_kmp_off; d.kf_mp_index = d_kmp; d.mp_bad = d_mp_bad; d.kf_ml_offsets = d_kml_off; d.kf_ml_index = d_kml; d.ml_bad = d_ml_bad;
    OLF_TRY(olf_tracked_map_points_batch_dev(c, &d, d_nobs, d_lnobs, n_list, d_list, min_obs_points, min_obs_lines, d_np, d_nlines, h.stream()));
    OLF_TRY(h.down(n_points, d_np, nl * 4)); OLF_TRY(h.down(n_lines, d_nlines, nl * 4));
    return h.finish_status();
}

extern "C" int olf_map_point_culling(olf_ctx* c, int n, const uint8_t* bad, const int32_t* found, const int32_t* visible, const int32_t* nobs,
                                     const int64_t* first_kf_id, int64_t current_kf_id, int monocular, uint8_t* action)
{
    const char* who = "olf_map_point_culling";
    if (!c || n < 0 || (n && (!bad || !found || !visible || !nobs || !first_kf_id || !action))) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (n == 0) return OLF_OK;
    const size_t nn = (size_t)n;
    uint8_t *d_bad, *d_action;
    int32_t *d_found, *d_visible, *d_nobs;
    int64_t* d_first;
    HostCall h(c, who);
    h.add(&d_first, nn); h.add(&d_found, nn); h.add(&d_visible, nn); h.add(&d_nobs, nn); h.add(&d_bad, nn); h.add(&d_action, nn);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(d_first, first_kf_id, nn * 8)); OLF_TRY(h.up(d_found, found, nn * 4)); OLF_TRY(h.up(d_visible, visible, nn * 4)); OLF_TRY(h.up(d_nobs, nobs, nn * 4));
    OLF_TRY(h.up(d_bad, bad, nn));
    OLF_TRY(olf_map_point_culling_dev(c, n, d_bad, d_found, d_visible, d_nobs, d_first, current_kf_id, monocular, d_action, h.stream()));
    OLF_TRY(h.down(action, d_action, nn));
    return h.finish();
}
