// connections_api.cpp -- olf_update_connections: the host-pointer form of olf_update_connections_batch_dev (connections_batch.hip).  It checks what the
// device form leaves to its caller (the shape of the three CSR pairs it reads), stages them, the list and the outputs in one carve and runs the same kernels.
#include "staging.hpp"
#include "../../include/orbline.h"

using namespace olf;

extern "C" int olf_update_connections(olf_ctx* c, const olf_map_graph* g, int n_list, const int32_t* kf_list, int th, int32_t* n_counted, int32_t* kf_max,
                                      int32_t* w_max, int32_t* conn_offsets, int32_t* conn_index, int32_t* conn_weight, int conn_capacity,
                                      int32_t* covis_offsets, int32_t* covis_index, int32_t* covis_weight, int covis_capacity)
{
    const char* who = "olf_update_connections";
    size_t n_obs = 0, n_kmp = 0;
    bool ok = c && g && n_list >= 0 && th >= 1 && conn_capacity >= 0 && covis_capacity >= 0 && g->n_kf >= 0 && g->n_mp >= 0;
    ok = ok && n_counted && kf_max && w_max && conn_offsets && covis_offsets && ((conn_index && conn_weight) || !conn_capacity) &&
         ((covis_index && covis_weight) || !covis_capacity);
    ok = ok && (g->mp_bad || !g->n_mp) && csr_ok(g->mp_obs_offsets, g->mp_obs_kf, g->n_mp, &n_obs) && csr_ok(g->kf_mp_offsets, g->kf_mp_index, g->n_kf, &n_kmp);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    if (g->n_kf > OLF_LOCALMAP_MAX_KF) { set_error(std::string(who) + ": more than OLF_LOCALMAP_MAX_KF key frames (a key frame's vote table lives in LDS)"); return OLF_ERR_CAPACITY; }
    if (n_list == 0) return OLF_OK;

    const size_t nl = (size_t)n_list, nk = (size_t)g->n_kf;
    olf_map_graph d = {};                                            // (only these fields are read)
    d.n_kf = g->n_kf; d.n_mp = g->n_mp;
    int32_t *d_obs_off, *d_obs_kf, *d_kmp_off, *d_kmp, *d_list = nullptr, *d_nc, *d_kmax, *d_wmax, *d_conn_off, *d_conn_idx, *d_conn_w, *d_cov_off, *d_cov_idx, *d_cov_w;
    uint8_t* d_mp_bad;
    HostCall h(c, who);
    h.add(&d_obs_off, (size_t)g->n_mp + 1); h.add(&d_obs_kf, n_obs); h.add(&d_mp_bad, (size_t)g->n_mp); h.add(&d_kmp_off, nk + 1); h.add(&d_kmp, n_kmp);
    if (kf_list) h.add(&d_list, nl);
    h.add(&d_nc, nl); h.add(&d_kmax, nl); h.add(&d_wmax, nl);
    h.add(&d_conn_off, nl + 1); h.add(&d_conn_idx, (size_t)conn_capacity); h.add(&d_conn_w, (size_t)conn_capacity);
    h.add(&d_cov_off, nl + 1); h.add(&d_cov_idx, (size_t)covis_capacity); h.add(&d_cov_w, (size_t)covis_capacity);
    OLF_TRY(h.bind(SCRATCH_STAGE));

    OLF_TRY(h.up(d_obs_off, g->mp_obs_offsets, ((size_t)g->n_mp + 1) * 4)); OLF_TRY(h.up(d_obs_kf, g->mp_obs_kf, n_obs * 4)); OLF_TRY(h.up(d_mp_bad, g->mp_bad, (size_t)g->n_mp));
    OLF_TRY(h.up(d_kmp_off, g->kf_mp_offsets, (nk + 1) * 4)); OLF_TRY(h.up(d_kmp, g->kf_mp_index, n_kmp * 4));
    if (kf_list) OLF_TRY(h.up(d_list, kf_list, nl * 4));
    d.mp_obs_offsets = d_obs_off; d.mp_obs_kf = d_obs_kf; d.mp_bad = d_mp_bad; d.kf_mp_offsets = d_kmp_off; d.kf_mp_index = d_kmp;

    OLF_TRY(olf_update_connections_batch_dev(c, &d, n_list, d_list, th, d_nc, d_kmax, d_wmax, d_conn_off, d_conn_idx, d_conn_w, conn_capacity, d_cov_off, d_cov_idx, d_cov_w,
                                             covis_capacity, h.stream()));

    OLF_TRY(h.down(n_counted, d_nc, nl * 4)); OLF_TRY(h.down(kf_max, d_kmax, nl * 4)); OLF_TRY(h.down(w_max, d_wmax, nl * 4));
    int len = 0;
    OLF_TRY(h.down_counted(conn_offsets, d_conn_off, nl + 1, conn_index, d_conn_idx, conn_capacity, &len));
    OLF_TRY(h.down(conn_weight, d_conn_w, (size_t)std::max(std::min(len, conn_capacity), 0) * 4));
    OLF_TRY(h.down_counted(covis_offsets, d_cov_off, nl + 1, covis_index, d_cov_idx, covis_capacity, &len));
    OLF_TRY(h.down(covis_weight, d_cov_w, (size_t)std::max(std::min(len, covis_capacity), 0) * 4));
    return h.finish_status();
}
