// localmap_api.cpp -- olf_update_local_map: the host-pointer form of olf_update_local_map_batch_dev (localmap_batch.hip).  It checks what the device form
// leaves to its caller (the shape of the graph's CSR arrays, the ascending children of convention C.16), stages the graph, the frames and the outputs in one
// carve and runs the same kernels.
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_update_local_map(olf_ctx* c, const olf_map_graph* g, int n_frames, int img_stride, const int32_t* counts, const int32_t* lcounts,
                                    const int32_t* frame_mp, const int32_t* frame_ml, int32_t* frame_mp_out, int32_t* frame_ml_out, int32_t* ref_kf,
                                    int32_t* n_voted, int32_t* kf_offsets, int32_t* kf_index, int kf_capacity, int32_t* mp_offsets, int32_t* mp_index,
                                    int mp_capacity, int32_t* ml_offsets, int32_t* ml_index, int ml_capacity)
{
    const char* who = "olf_update_local_map";
    size_t n_obs = 0, n_kmp = 0, n_kml = 0, n_cov = 0, n_child = 0;
    bool ok = c && g && n_frames >= 0 && img_stride >= 1 && kf_capacity >= 0 && mp_capacity >= 0 && ml_capacity >= 0 && g->n_kf >= 0 && g->n_mp >= 0 && g->n_ml >= 0;
    ok = ok && frame_mp && ref_kf && n_voted && kf_offsets && mp_offsets && ml_offsets && (kf_index || !kf_capacity) && (mp_index || !mp_capacity) &&
         (ml_index || !ml_capacity);
    ok = ok && g->kf_bad && g->kf_parent && (g->mp_bad || !g->n_mp) && (g->ml_bad || !g->n_ml) && csr_ok(g->mp_obs_offsets, g->mp_obs_kf, g->n_mp, &n_obs) &&
         csr_ok(g->kf_mp_offsets, g->kf_mp_index, g->n_kf, &n_kmp) && (g->n_ml == 0 || csr_ok(g->kf_ml_offsets, g->kf_ml_index, g->n_kf, &n_kml)) &&
         csr_ok(g->kf_covis_offsets, g->kf_covis_index, g->n_kf, &n_cov) && csr_ok(g->kf_child_offsets, g->kf_child_index, g->n_kf, &n_child);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    for (int k = 0; k < g->n_kf; ++k)                                // std::set<KeyFrame*> order (C.16)
        for (int o = g->kf_child_offsets[k] + 1; o < g->kf_child_offsets[k + 1]; ++o)
            if (g->kf_child_index[o] <= g->kf_child_index[o - 1]) { set_error(std::string(who) + ": the children of a key frame do not ascend strictly"); return OLF_ERR_INVALID; }
    if (g->n_kf > OLF_LOCALMAP_MAX_KF) { set_error(std::string(who) + ": more than OLF_LOCALMAP_MAX_KF key frames (a frame's vote table lives in LDS)"); return OLF_ERR_CAPACITY; }
    if (n_frames == 0) return OLF_OK;

    const size_t nf = (size_t)n_frames, nk = (size_t)g->n_kf, cap = (size_t)olf_orb_capacity(c), lcap = (size_t)olf_line_capacity(c);
    const size_t n_counts = (nf - 1) * (size_t)img_stride + 1;
    const bool lines = g->n_ml > 0;
    olf_map_graph d = *g;
    int32_t *d_obs_off, *d_obs_kf, *d_kmp_off, *d_kmp, *d_kml_off = nullptr, *d_kml = nullptr, *d_cov_off, *d_cov, *d_child_off, *d_child, *d_parent;
    uint8_t *d_mp_bad, *d_ml_bad = nullptr, *d_kf_bad;
    int32_t *d_counts = nullptr, *d_lcounts = nullptr, *d_fmp, *d_fml = nullptr, *d_ref, *d_nv, *d_kf_offs, *d_kf_idx, *d_mp_offs, *d_mp_idx, *d_ml_offs, *d_ml_idx;
    HostCall h(c, who);
    h.add(&d_obs_off, (size_t)g->n_mp + 1); h.add(&d_obs_kf, n_obs); h.add(&d_mp_bad, (size_t)g->n_mp); h.add(&d_kf_bad, nk);
    h.add(&d_kmp_off, nk + 1); h.add(&d_kmp, n_kmp); h.add(&d_cov_off, nk + 1); h.add(&d_cov, n_cov); h.add(&d_child_off, nk + 1); h.add(&d_child, n_child);
    h.add(&d_parent, nk);
    if (lines) { h.add(&d_ml_bad, (size_t)g->n_ml); h.add(&d_kml_off, nk + 1); h.add(&d_kml, n_kml); }
    if (counts) h.add(&d_counts, n_counts);
    if (lcounts) h.add(&d_lcounts, n_counts);
    h.add(&d_fmp, nf * cap);                                         // (cleaned in place; downloaded when the caller wants the rows)
    if (frame_ml) h.add(&d_fml, nf * lcap);
    h.add(&d_ref, nf); h.add(&d_nv, nf);
    h.add(&d_kf_offs, nf + 1); h.add(&d_kf_idx, (size_t)kf_capacity); h.add(&d_mp_offs, nf + 1); h.add(&d_mp_idx, (size_t)mp_capacity);
    h.add(&d_ml_offs, nf + 1); h.add(&d_ml_idx, (size_t)ml_capacity);
    OLF_TRY(h.bind(SCRATCH_STAGE));

    OLF_TRY(h.up(d_obs_off, g->mp_obs_offsets, ((size_t)g->n_mp + 1) * 4)); OLF_TRY(h.up(d_obs_kf, g->mp_obs_kf, n_obs * 4));
    OLF_TRY(h.up(d_mp_bad, g->mp_bad, (size_t)g->n_mp)); OLF_TRY(h.up(d_kf_bad, g->kf_bad, nk));
    OLF_TRY(h.up(d_kmp_off, g->kf_mp_offsets, (nk + 1) * 4)); OLF_TRY(h.up(d_kmp, g->kf_mp_index, n_kmp * 4));
    OLF_TRY(h.up(d_cov_off, g->kf_covis_offsets, (nk + 1) * 4)); OLF_TRY(h.up(d_cov, g->kf_covis_index, n_cov * 4));
    OLF_TRY(h.up(d_child_off, g->kf_child_offsets, (nk + 1) * 4)); OLF_TRY(h.up(d_child, g->kf_child_index, n_child * 4));
    OLF_TRY(h.up(d_parent, g->kf_parent, nk * 4));
    if (lines) { OLF_TRY(h.up(d_ml_bad, g->ml_bad, (size_t)g->n_ml)); OLF_TRY(h.up(d_kml_off, g->kf_ml_offsets, (nk + 1) * 4)); OLF_TRY(h.up(d_kml, g->kf_ml_index, n_kml * 4)); }
    if (counts) OLF_TRY(h.up(d_counts, counts, n_counts * 4));
    if (lcounts) OLF_TRY(h.up(d_lcounts, lcounts, n_counts * 4));
    OLF_TRY(h.up(d_fmp, frame_mp, nf * cap * 4));
    if (frame_ml) OLF_TRY(h.up(d_fml, frame_ml, nf * lcap * 4));
    d.mp_obs_offsets = d_obs_off; d.mp_obs_kf = d_obs_kf; d.mp_bad = d_mp_bad; d.ml_bad = d_ml_bad; d.kf_bad = d_kf_bad;
    d.kf_mp_offsets = d_kmp_off; d.kf_mp_index = d_kmp; d.kf_ml_offsets = d_kml_off; d.kf_ml_index = d_kml;
    d.kf_covis_offsets = d_cov_off; d.kf_covis_index = d_cov; d.kf_child_offsets = d_child_off; d.kf_child_index = d_child; d.kf_parent = d_parent;

    OLF_TRY(olf_update_local_map_batch_dev(c, &d, n_frames, img_stride, d_counts, d_lcounts, d_fmp, d_fml, d_fmp, d_fml, d_ref, d_nv, d_kf_offs, d_kf_idx, kf_capacity,
                                           d_mp_offs, d_mp_idx, mp_capacity, d_ml_offs, d_ml_idx, ml_capacity, h.stream()));

    if (frame_mp_out) OLF_TRY(h.down(frame_mp_out, d_fmp, nf * cap * 4));
    if (frame_ml && frame_ml_out) OLF_TRY(h.down(frame_ml_out, d_fml, nf * lcap * 4));
    OLF_TRY(h.down(ref_kf, d_ref, nf * 4)); OLF_TRY(h.down(n_voted, d_nv, nf * 4));
    int len = 0;
    OLF_TRY(h.down_counted(kf_offsets, d_kf_offs, nf + 1, kf_index, d_kf_idx, kf_capacity, &len));
    OLF_TRY(h.down_counted(mp_offsets, d_mp_offs, nf + 1, mp_index, d_mp_idx, mp_capacity, &len));
    OLF_TRY(h.down_counted(ml_offsets, d_ml_offs, nf + 1, ml_index, d_ml_idx, ml_capacity, &len));
    return h.finish_status();
}
