// api_host.cpp -- the host-pointer entries of the C ABI: each stages its arrays on the device, calls the _dev entry or the launcher of the same name and
// brings the results back.  The entries on caller-sized arrays go through HostCall (staging.hpp); those on the context's own frame arrays (fb_copy, the
// one-pair slab of olf_stereo_frames) keep the copies they were measured with.  Every entry checks its arguments, then the device, then touches HIP.
#include <cmath>
#include <string>
#include "ctx.hpp"
#include "staging.hpp"

using namespace olf;

extern "C" {

// ---- on the context's frame arrays ---------------------------------------------------------------------------------------------------------
int olf_orb_extract(olf_ctx* c, const uint8_t* images, int n_images, olf_keypoint* kps, uint8_t* desc, int32_t* counts)
{
    if (!c || !images || !kps || !desc || !counts) { set_error("olf_orb_extract: null argument"); return OLF_ERR_INVALID; }
    if (n_images < 0 || n_images > c->max_images) return OLF_ERR_CAPACITY;
    if (n_images == 0) return OLF_OK;
    OLF_TRY(check_device(c, "olf_orb_extract"));
    olf_frame_buffers h = {}; h.kps = kps; h.desc = desc; h.counts = counts;
    OLF_HIP_CHECK(hipMemcpyAsync(c->d_images, images, (size_t)c->W * c->H * n_images, hipMemcpyHostToDevice, c->stream));
    OLF_TRY(olf_orb_extract_dev(c, c->d_images, n_images, c->d_out.kps, c->d_out.desc, c->d_out.counts, c->stream));
    OLF_TRY(fb_copy(c, h, FB_KPS, FB_COUNTS, n_images, hipMemcpyDeviceToHost));
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return check_status(c);
}

int olf_orb_extract_strided(olf_ctx* c, const uint8_t* image, size_t row_stride, olf_keypoint* kps, uint8_t* desc, int32_t* count)
{
    if (!c || !image || !kps || !desc || !count || row_stride < (size_t)c->W) { set_error("olf_orb_extract_strided: bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_orb_extract_strided"));
    olf_frame_buffers h = {}; h.kps = kps; h.desc = desc; h.counts = count;
    OLF_HIP_CHECK(hipMemcpy2DAsync(c->d_images, c->W, image, row_stride, c->W, c->H, hipMemcpyHostToDevice, c->stream));
    OLF_TRY(olf_orb_extract_dev(c, c->d_images, 1, c->d_out.kps, c->d_out.desc, c->d_out.counts, c->stream));
    OLF_TRY(fb_copy(c, h, FB_KPS, FB_COUNTS, 1, hipMemcpyDeviceToHost));
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return check_status(c);
}

int olf_stereo_points(olf_ctx* c, const uint8_t* images, int n_pairs, olf_keypoint* kps, uint8_t* desc, int32_t* counts, float* uright,
                      float* depth)
{
    if (!c || !images || !kps || !desc || !counts || !uright || !depth) { set_error("olf_stereo_points: null argument"); return OLF_ERR_INVALID; }
    const int n_images = 2 * n_pairs;
    if (n_pairs < 0 || n_images > c->max_images) return OLF_ERR_CAPACITY;
    if (n_pairs == 0) return OLF_OK;
    OLF_TRY(check_device(c, "olf_stereo_points"));
    olf_frame_buffers h = {}; h.kps = kps; h.desc = desc; h.counts = counts; h.uright = uright; h.depth = depth;
    OLF_HIP_CHECK(hipMemcpyAsync(c->d_images, images, (size_t)c->W * c->H * n_images, hipMemcpyHostToDevice, c->stream));
    OLF_TRY(olf_orb_extract_dev(c, c->d_images, n_images, c->d_out.kps, c->d_out.desc, c->d_out.counts, c->stream));
    OLF_TRY(olf_stereo_points_dev(c, n_pairs, c->d_out.kps, c->d_out.desc, c->d_out.counts, c->d_out.uright, c->d_out.depth, c->stream));
    OLF_TRY(fb_copy(c, h, FB_KPS, FB_DEPTH, n_images, hipMemcpyDeviceToHost));
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return check_status(c);
}

int olf_line_extract(olf_ctx* c, const uint8_t* images, int n_images, olf_keyline* kls, uint8_t* ldesc, int32_t* lcounts)
{
    if (!c || !images || !kls || !ldesc || !lcounts) { set_error("olf_line_extract: null argument"); return OLF_ERR_INVALID; }
    if (n_images < 0 || n_images > c->max_images) return OLF_ERR_CAPACITY;
    if (n_images == 0) return OLF_OK;
    OLF_TRY(check_device(c, "olf_line_extract"));
    olf_frame_buffers h = {}; h.kls = kls; h.ldesc = ldesc; h.lcounts = lcounts;
    OLF_HIP_CHECK(hipMemcpyAsync(c->d_images, images, (size_t)c->W * c->H * n_images, hipMemcpyHostToDevice, c->stream));
    OLF_TRY(olf_line_extract_dev(c, c->d_images, n_images, c->d_out.kls, c->d_out.ldesc, c->d_out.lcounts, c->stream));
    OLF_TRY(fb_copy(c, h, FB_KLS, FB_LCOUNTS, n_images, hipMemcpyDeviceToHost));
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return check_status(c);
}

int olf_line_extract_strided(olf_ctx* c, const uint8_t* image, size_t row_stride, olf_keyline* kls, uint8_t* ldesc, int32_t* lcount)
{
    if (!c || !image || !kls || !ldesc || !lcount || row_stride < (size_t)c->W) { set_error("olf_line_extract_strided: bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_line_extract_strided"));
    olf_frame_buffers h = {}; h.kls = kls; h.ldesc = ldesc; h.lcounts = lcount;
    OLF_HIP_CHECK(hipMemcpy2DAsync(c->d_images, c->W, image, row_stride, c->W, c->H, hipMemcpyHostToDevice, c->stream));
    OLF_TRY(olf_line_extract_dev(c, c->d_images, 1, c->d_out.kls, c->d_out.ldesc, c->d_out.lcounts, c->stream));
    OLF_TRY(fb_copy(c, h, FB_KLS, FB_LCOUNTS, 1, hipMemcpyDeviceToHost));
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return check_status(c);
}

int olf_lbd_compute(olf_ctx* c, const uint8_t* images, int n_images, const olf_keyline* kls, const int32_t* lcounts, uint8_t* ldesc)
{
    if (!c || !images || !kls || !lcounts || !ldesc) { set_error("olf_lbd_compute: null argument"); return OLF_ERR_INVALID; }
    if (n_images < 0 || n_images > c->max_images) return OLF_ERR_CAPACITY;
    if (n_images == 0) return OLF_OK;
    for (int i = 0; i < n_images; ++i)
        if (lcounts[i] < 0 || lcounts[i] > c->line.geom.outCap) { set_error("olf_lbd_compute: count exceeds capacity"); return OLF_ERR_CAPACITY; }
    // the accepted domain (include/orbline.h): beyond it the reference's float -> short conversion and its libm calls have no defined answer to reproduce
    for (int i = 0; i < n_images; ++i)
        for (int j = 0; j < lcounts[i]; ++j) {
            const olf_keyline& kl = kls[(size_t)i * c->line.geom.outCap + j];
            const float xy[4] = {kl.sPointInOctaveX, kl.sPointInOctaveY, kl.ePointInOctaveX, kl.ePointInOctaveY};
            for (float v : xy)
                if (!std::isfinite(v) || std::fabs(v) > 1e6f) {
                    set_error("olf_lbd_compute: key line " + std::to_string(j) + " of image " + std::to_string(i) + " has a non-finite coordinate or one beyond +-1e6");
                    return OLF_ERR_INVALID;
                }
            if (!std::isfinite(kl.angle)) {
                set_error("olf_lbd_compute: key line " + std::to_string(j) + " of image " + std::to_string(i) + " has a non-finite angle");
                return OLF_ERR_INVALID;
            }
            if (c->line.geom.libmFloat && !(std::fabs(kl.angle) < 120.0f)) {      // (glibc_sincosf_core, device_math.hpp: glibc's fast range reduction only)
                set_error("olf_lbd_compute: key line " + std::to_string(j) + " of image " + std::to_string(i) + " has |angle| >= 120 under conv_libm_float");
                return OLF_ERR_INVALID;
            }
        }
    OLF_TRY(check_device(c, "olf_lbd_compute"));
    olf_frame_buffers h = {}; h.kls = const_cast<olf_keyline*>(kls); h.ldesc = ldesc; h.lcounts = const_cast<int32_t*>(lcounts);
    OLF_HIP_CHECK(hipMemcpyAsync(c->d_images, images, (size_t)c->W * c->H * n_images, hipMemcpyHostToDevice, c->stream));
    // BinaryDescriptor::compute on the caller's key lines: no LSD, no selection
    OLF_TRY(fb_copy(c, h, FB_KLS, FB_KLS, n_images, hipMemcpyHostToDevice));
    OLF_TRY(fb_copy(c, h, FB_LCOUNTS, FB_LCOUNTS, n_images, hipMemcpyHostToDevice));
    OLF_TRY(launch_lbd_dense(c->line.geom, c->lb, c->d_images, c->W, n_images, c->stream));
    OLF_TRY(launch_lbd_desc(c->line.geom, c->lb, n_images, c->d_out.kls, c->d_out.ldesc, c->d_out.lcounts, false, c->stream));
    OLF_TRY(fb_copy(c, h, FB_LDESC, FB_LDESC, n_images, hipMemcpyDeviceToHost));
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return OLF_OK;
}

int olf_stereo_lines(olf_ctx* c, int n_pairs, const olf_keyline* kls, const uint8_t* ldesc, const int32_t* lcounts, int32_t* m12, float* disp,
                     double* le)
{
    if (!c || !kls || !ldesc || !lcounts || !m12 || !disp || !le) { set_error("olf_stereo_lines: null argument"); return OLF_ERR_INVALID; }
    if (n_pairs < 0 || 2 * n_pairs > c->max_images) { set_error("olf_stereo_lines: n_pairs exceeds the context's max_images"); return OLF_ERR_CAPACITY; }
    if (n_pairs == 0) return OLF_OK;
    const size_t cap = c->line.geom.outCap, ni = 2 * (size_t)n_pairs;
    for (size_t i = 0; i < ni; ++i)
        if (lcounts[i] < 0 || lcounts[i] > (int)cap) { set_error("olf_stereo_lines: count exceeds capacity"); return OLF_ERR_CAPACITY; }
    OLF_TRY(check_device(c, "olf_stereo_lines"));
    olf_frame_buffers h = {}; h.kls = const_cast<olf_keyline*>(kls); h.ldesc = const_cast<uint8_t*>(ldesc); h.lcounts = const_cast<int32_t*>(lcounts);
    h.lmatches12 = m12; h.ldisp = disp; h.lle = le;
    OLF_TRY(fb_copy(c, h, FB_KLS, FB_LCOUNTS, ni, hipMemcpyHostToDevice));
    OLF_TRY(olf_stereo_lines_dev(c, n_pairs, c->d_out.kls, c->d_out.ldesc, c->d_out.lcounts, c->d_out.lmatches12, c->d_out.ldisp, c->d_out.lle, c->stream));
    OLF_TRY(fb_copy(c, h, FB_LMATCHES12, FB_LLE, ni, hipMemcpyDeviceToHost));
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return OLF_OK;
}

int olf_stereo_frames(olf_ctx* c, const uint8_t* images, int n_pairs, const olf_frame_buffers* o)
{
    if (!c || !images || !o) { set_error("olf_stereo_frames: null argument"); return OLF_ERR_INVALID; }
    if (n_pairs < 0 || 2 * n_pairs > c->max_images) return OLF_ERR_CAPACITY;
    if (n_pairs == 0) return OLF_OK;
    OLF_TRY(check_device(c, "olf_stereo_frames"));
    const size_t ni = 2 * (size_t)n_pairs;
    c->input_event = nullptr;           // (the upload below is on the context's stream: the line stream must fork from it, whatever event an earlier caller left)
    OLF_HIP_CHECK(hipMemcpyAsync(c->d_images, images, (size_t)c->W * c->H * ni, hipMemcpyHostToDevice, c->stream));
    OLF_TRY(olf_stereo_frames_dev(c, c->d_images, n_pairs, &c->d_out, c->stream));
    OLF_TRY(olf_stereo_frames_join_dev(c, c->stream));      // (a context with the deferred join on: the copies below read the line outputs)
    if (c->d_outslab && (int)ni == c->max_images) {
        // one copy for all eleven arrays, then host copies out of the pinned slab (the arrays are laid out for exactly this many images)
        OLF_HIP_CHECK(hipMemcpyAsync(c->h_outslab, c->d_outslab, c->outslab_bytes, hipMemcpyDeviceToHost, c->stream));
        OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < FB_FIELDS; ++k) memcpy(fb_field(*o, k), c->h_outslab + c->outslab_off[k], fb_bytes(c, k, ni));
        return check_status(c);
    }
    OLF_TRY(fb_copy(c, *o, 0, FB_FIELDS - 1, ni, hipMemcpyDeviceToHost));
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return check_status(c);
}

// ---- on caller-sized arrays: HostCall ----------------------------------------------------------------------------------------------------------
// (stages in SCRATCH_STAGE: olf_match_bf_dev takes SCRATCH_KNN under it)
int olf_match_bf(olf_ctx* c, const uint8_t* descA, int nA, const uint8_t* descB, int nB, float nnr, int best_lr, int32_t* m12)
{
    if (!c || !m12 || nA < 0 || nB < 0 || (nA && !descA) || (nB && !descB)) { set_error("olf_match_bf: bad argument"); return OLF_ERR_INVALID; }
    if (nA == 0) return OLF_OK;
    HostCall h(c, "olf_match_bf");
    uint8_t *dA, *dB; int *dn, *dm;
    h.add(&dA, (size_t)nA * 32); h.add(&dB, (size_t)nB * 32); h.add(&dn, 2); h.add(&dm, nA);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    const int n[2] = {nA, nB};
    OLF_TRY(h.up(dA, descA, (size_t)nA * 32)); OLF_TRY(h.up(dB, descB, (size_t)nB * 32)); OLF_TRY(h.up(dn, n, sizeof(n)));
    OLF_TRY(olf_match_bf_dev(c, dA, dn, nA, 1, dB, dn + 1, std::max(nB, 1), 1, 1, nnr, best_lr, dm, h.stream()));
    OLF_TRY(h.down(m12, dm, (size_t)nA * 4));
    return h.finish();
}

int olf_knn2(olf_ctx* c, const uint8_t* descQ, int nQ, const uint8_t* descT, int nT, int32_t* idx0, int32_t* dist0, int32_t* dist1)
{
    if (!c || !idx0 || !dist0 || !dist1 || nQ < 0 || nT < 0 || (nQ && !descQ) || (nT && !descT)) { set_error("olf_knn2: bad argument"); return OLF_ERR_INVALID; }
    if (nQ == 0) return OLF_OK;
    HostCall h(c, "olf_knn2");
    uint8_t *dQ, *dT; int *dn, *o;
    h.add(&dQ, (size_t)nQ * 32); h.add(&dT, (size_t)nT * 32); h.add(&dn, 2); h.add(&o, (size_t)3 * nQ);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    const int n[2] = {nQ, nT};
    OLF_TRY(h.up(dQ, descQ, (size_t)nQ * 32)); OLF_TRY(h.up(dT, descT, (size_t)nT * 32)); OLF_TRY(h.up(dn, n, sizeof(n)));
    OLF_TRY(launch_knn2(dQ, dn, nQ, dT, dn + 1, std::max(nT, 1), 1, o, o + nQ, o + 2 * nQ, h.stream()));
    OLF_TRY(h.down(idx0, o, (size_t)nQ * 4)); OLF_TRY(h.down(dist0, o + nQ, (size_t)nQ * 4)); OLF_TRY(h.down(dist1, o + 2 * nQ, (size_t)nQ * 4));
    return h.finish();
}

int olf_match_candidates(olf_ctx* c, const uint8_t* descQ, int nQ, const uint8_t* descT, int nT, const int32_t* offs, const int32_t* cand,
                         uint16_t* dist)
{
    if (!c || nQ < 0 || nT < 0 || (nQ && (!descQ || !offs)) || (nT && !descT)) { set_error("olf_match_candidates: bad argument"); return OLF_ERR_INVALID; }
    if (nQ == 0) return OLF_OK;
    const int nnz = offs[nQ];
    if (nnz < 0 || offs[0] != 0 || (nnz && (!cand || !dist))) { set_error("olf_match_candidates: bad CSR"); return OLF_ERR_INVALID; }
    if (nnz == 0) return OLF_OK;
    HostCall h(c, "olf_match_candidates");
    uint8_t *dQ, *dT; int *dO, *dC; uint16_t* dD;
    h.add(&dQ, (size_t)nQ * 32); h.add(&dT, (size_t)nT * 32); h.add(&dO, (size_t)nQ + 1); h.add(&dC, nnz); h.add(&dD, nnz);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(dQ, descQ, (size_t)nQ * 32)); OLF_TRY(h.up(dT, descT, (size_t)nT * 32));
    OLF_TRY(h.up(dO, offs, ((size_t)nQ + 1) * 4)); OLF_TRY(h.up(dC, cand, (size_t)nnz * 4));
    OLF_TRY(olf_match_candidates_dev(c, dQ, nQ, dT, nT, dO, dC, dD, h.stream()));
    OLF_TRY(h.down(dist, dD, (size_t)nnz * 2));
    return h.finish();
}

// ---- Frame::mGrid (grid.hip) -----------------------------------------------------------------------------------------------------------
int olf_frame_grid(olf_ctx* c, const olf_keypoint* keys, int n, float minX, float maxX, float minY, float maxY, int32_t* cell_offsets, int32_t* cell_index)
{
    float wInv, hInv;
    if (!c || n < 0 || (n && (!keys || !cell_index)) || !cell_offsets || !grid_scales(minX, maxX, minY, maxY, &wInv, &hInv)) {
        set_error("olf_frame_grid: bad argument"); return OLF_ERR_INVALID;
    }
    if (n > OLF_GRID_MAX_KEYS) { set_error("olf_frame_grid: more than OLF_GRID_MAX_KEYS key points"); return OLF_ERR_CAPACITY; }
    HostCall h(c, "olf_frame_grid");
    olf_keypoint* dK; int *dO, *dI;
    h.add(&dK, n); h.add(&dO, OLF_GRID_CELLS + 1); h.add(&dI, n);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(dK, keys, (size_t)n * sizeof(olf_keypoint)));
    OLF_TRY(launch_assign_grid(dK, 0, nullptr, 0, n, n, minX, minY, wInv, hInv, 1, dO, dI, (size_t)std::max(n, 1), h.stream()));
    int used;
    OLF_TRY(h.down_counted(cell_offsets, dO, OLF_GRID_CELLS + 1, cell_index, dI, n, &used));
    return h.finish();
}

int olf_features_in_area(olf_ctx* c, const olf_keypoint* keys, int n_keys, const int32_t* cell_offsets, const int32_t* cell_index, float minX, float maxX,
                         float minY, float maxY, int n_queries, const olf_area_query* queries, int32_t* cand_offsets, int32_t* cand_idx, int cand_capacity)
{
    if (!c || n_keys < 0 || (n_keys && !keys) || n_queries < 0 || cand_capacity < 0 || !cand_offsets || (n_queries && !queries) || (cand_capacity && !cand_idx) ||
        !(maxX > minX) || !(maxY > minY)) {
        set_error("olf_features_in_area: bad argument"); return OLF_ERR_INVALID;
    }
    if (!grid_is_valid(cell_offsets, cell_index, n_keys)) { set_error("olf_features_in_area: the grid does not describe n_keys features"); return OLF_ERR_INVALID; }
    HostCall h(c, "olf_features_in_area");
    const int used = cell_offsets[OLF_GRID_CELLS];
    olf_keypoint* dK; olf_area_query* dQ; int *dO, *dI, *dCO, *dC;
    h.add(&dK, n_keys); h.add(&dO, OLF_GRID_CELLS + 1); h.add(&dI, used); h.add(&dQ, n_queries); h.add(&dCO, (size_t)n_queries + 1); h.add(&dC, cand_capacity);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(dK, keys, (size_t)n_keys * sizeof(olf_keypoint))); OLF_TRY(h.up(dO, cell_offsets, (size_t)(OLF_GRID_CELLS + 1) * 4));
    OLF_TRY(h.up(dI, cell_index, (size_t)used * 4)); OLF_TRY(h.up(dQ, queries, (size_t)n_queries * sizeof(olf_area_query)));
    OLF_TRY(olf_features_in_area_dev(c, dK, dO, dI, minX, maxX, minY, maxY, n_queries, dQ, dCO, dC, cand_capacity, h.stream()));
    int total;
    OLF_TRY(h.down_counted(cand_offsets, dCO, (size_t)n_queries + 1, cand_idx, dC, cand_capacity, &total));
    return h.finish_status();
}

// ---- input conditioning (precond.hip): image-sized, SCRATCH_BATCH --------------------------------------------------------------------------------
int olf_init_undistort_rectify_map(olf_ctx* c, const double* K, const double* D, int n_dist, const double* R, const double* P, int w, int h, float* map1, float* map2)
{
    if (!c || !map1 || !map2 || w < 1 || h < 1) { set_error("olf_init_undistort_rectify_map: bad argument"); return OLF_ERR_INVALID; }
    HostCall hc(c, "olf_init_undistort_rectify_map");
    const size_t npx = (size_t)w * h;
    float *d1, *d2;
    hc.add(&d1, npx); hc.add(&d2, npx);
    OLF_TRY(hc.bind(SCRATCH_BATCH));
    OLF_TRY(olf_init_undistort_rectify_map_dev(c, K, D, n_dist, R, P, w, h, d1, d2, hc.stream()));
    OLF_TRY(hc.down(map1, d1, npx * sizeof(float))); OLF_TRY(hc.down(map2, d2, npx * sizeof(float)));
    return hc.finish();
}

int olf_cvt_gray(olf_ctx* c, const uint8_t* src, int code, int n_images, uint8_t* gray)
{
    if (!c || !src || !gray || code < 0 || code > 3 || n_images < 0) { set_error("olf_cvt_gray: bad argument"); return OLF_ERR_INVALID; }
    if (n_images == 0) return OLF_OK;
    HostCall h(c, "olf_cvt_gray");
    const size_t npx = (size_t)c->W * c->H * n_images, cn = code >= 2 ? 4 : 3;
    uint8_t *ds, *dd;
    h.add(&ds, npx * cn); h.add(&dd, npx);
    OLF_TRY(h.bind(SCRATCH_BATCH));
    OLF_TRY(h.up(ds, src, npx * cn));
    OLF_TRY(olf_cvt_gray_dev(c, ds, code, n_images, dd, h.stream()));
    OLF_TRY(h.down(gray, dd, npx));
    return h.finish();
}

int olf_remap_linear(olf_ctx* c, const uint8_t* src, int sw, int sh, const float* mapx, const float* mapy, int dw, int dh, int n_images, uint8_t* dst)
{
    if (!c || !src || !mapx || !mapy || !dst || sw < 1 || sh < 1 || dw < 1 || dh < 1 || n_images < 0) { set_error("olf_remap_linear: bad argument"); return OLF_ERR_INVALID; }
    if (n_images == 0) return OLF_OK;
    HostCall h(c, "olf_remap_linear");
    const size_t bs = (size_t)sw * sh * n_images, npx = (size_t)dw * dh, bd = npx * n_images;
    uint8_t *ds, *dd; float *mx, *my;
    h.add(&ds, bs); h.add(&mx, npx); h.add(&my, npx); h.add(&dd, bd);
    OLF_TRY(h.bind(SCRATCH_BATCH));
    OLF_TRY(h.up(ds, src, bs)); OLF_TRY(h.up(mx, mapx, npx * 4)); OLF_TRY(h.up(my, mapy, npx * 4));
    OLF_TRY(olf_remap_linear_dev(c, ds, sw, sh, mx, my, dw, dh, n_images, dd, h.stream()));
    OLF_TRY(h.down(dst, dd, bd));
    return h.finish();
}

// ---- descriptor sets (match.hip) ---------------------------------------------------------------------------------------------------------------
int olf_hamming_matrix(olf_ctx* c, const uint8_t* descA, int nA, const uint8_t* descB, int nB, uint16_t* out)
{
    if (!c || !out || nA < 0 || nB < 0 || (nA && !descA) || (nB && !descB)) { set_error("olf_hamming_matrix: bad argument"); return OLF_ERR_INVALID; }
    if (nA == 0 || nB == 0) return OLF_OK;
    HostCall h(c, "olf_hamming_matrix");
    uint8_t *dA, *dB; uint16_t* dO;
    h.add(&dA, (size_t)nA * 32); h.add(&dB, (size_t)nB * 32); h.add(&dO, (size_t)nA * nB);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(dA, descA, (size_t)nA * 32)); OLF_TRY(h.up(dB, descB, (size_t)nB * 32));
    OLF_TRY(launch_hamming_matrix(dA, nA, dB, nB, dO, h.stream()));
    OLF_TRY(h.down(out, dO, (size_t)nA * nB * 2));
    return h.finish();
}

int olf_distinctive_descriptors(olf_ctx* c, const uint8_t* desc, const int32_t* offs, int n_points, int32_t* best)
{
    if (!c || !offs || !best || n_points < 0) { set_error("olf_distinctive_descriptors: bad argument"); return OLF_ERR_INVALID; }
    if (n_points == 0) return OLF_OK;
    const int total = offs[n_points];
    if (offs[0] != 0 || total < 0 || (total > 0 && !desc)) { set_error("olf_distinctive_descriptors: bad offsets"); return OLF_ERR_INVALID; }
    for (int i = 0; i < n_points; ++i) {
        if (offs[i + 1] < offs[i]) { set_error("olf_distinctive_descriptors: offsets must not decrease"); return OLF_ERR_INVALID; }
        if (offs[i + 1] - offs[i] > 1024) { set_error("olf_distinctive_descriptors: more than 1024 observations of one landmark"); return OLF_ERR_CAPACITY; }
    }
    HostCall h(c, "olf_distinctive_descriptors");
    uint8_t* dD; int *dO, *dB;
    h.add(&dD, (size_t)total * 32); h.add(&dO, (size_t)n_points + 1); h.add(&dB, n_points);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_TRY(h.up(dD, desc, (size_t)total * 32)); OLF_TRY(h.up(dO, offs, ((size_t)n_points + 1) * 4));
    OLF_TRY(launch_distinctive(dD, dO, n_points, dB, h.stream()));
    OLF_TRY(h.down(best, dB, (size_t)n_points * 4));
    return h.finish();
}

}  // extern "C"
