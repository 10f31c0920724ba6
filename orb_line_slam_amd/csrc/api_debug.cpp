// api_debug.cpp -- the entries of the C ABI that exist for the tests and the tools: olf_debug_*, and the readers of a context's intermediate buffers
// (olf_orb_pyramid_level, olf_orb_debug_candidates, olf_lsd_debug_scaled).
#include "ctx.hpp"
#include "staging.hpp"
#include "wg_state.hpp"

namespace olf {
int launch_copy16(const void* src, void* dst, size_t bytes, hipStream_t s);
}

using namespace olf;

// the counters a sweep kernel adds its mismatches to: n words of SCRATCH_STAGE, zeroed
static int sweep_counters(HostCall& h, unsigned long long** st, int n)
{
    h.add(st, n);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    OLF_HIP_CHECK(hipMemsetAsync(*st, 0, (size_t)n * 8, h.stream()));
    return OLF_OK;
}

extern "C" {

int olf_orb_pyramid_level(olf_ctx* c, int image, int level, int blurred, uint8_t* dst)
{
    if (!c || !dst || image < 0 || image >= c->max_images || level < 0 || level >= c->orb.geom.nlevels) return OLF_ERR_INVALID;
    const LevelGeom& L = c->orb.geom.lv[level];
    const uint8_t* src = (blurred ? c->ob.blur : c->ob.pyr) + (size_t)image * c->orb.geom.pyrBytes + L.offset;
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    OLF_HIP_CHECK(hipMemcpy2D(dst, L.w, src, L.pitch, L.w, L.h, hipMemcpyDeviceToHost));
    return OLF_OK;
}

int olf_debug_octree_launches(const olf_orb_params* p, int width, int height, int32_t* level_launch, int32_t* launch_lds)
{
    if (!p || !level_launch || !launch_lds) return OLF_ERR_INVALID;
    OrbHostTables t;
    OLF_TRY(t.build(*p, width, height));
    OctLaunch la[3];
    const int n = octree_launches(t.geom, la);
    for (int i = 0; i < 3; ++i) launch_lds[i] = i < n ? (int32_t)la[i].lds : -1;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < la[i].lv.n; ++k) level_launch[la[i].lv.id[k]] = i;
    return n;
}

int olf_debug_sim3_solver_lds_limit(int bytes)
{
    g_sim3_solver_lds.set(bytes);
    return OLF_OK;
}

int olf_debug_pnp_solver_lds_limit(int bytes)
{
    g_pnp_solver_lds.set(bytes);
    return OLF_OK;
}

int olf_debug_initializer_lds_limit(int bytes)
{
    g_initializer_lds.set(bytes);
    return OLF_OK;
}

int olf_debug_pose_points_lds_limit(int bytes)
{
    g_pose_points_lds.set(bytes);
    return OLF_OK;
}

int olf_debug_optimize_sim3_lds_limit(int bytes)
{
    g_optimize_sim3_lds.set(bytes);
    return OLF_OK;
}

int olf_debug_status(olf_ctx* c, int32_t* out64)
{
    if (!c || !out64) return OLF_ERR_INVALID;
    OLF_HIP_CHECK(hipDeviceSynchronize());
    OLF_HIP_CHECK(hipMemcpy(out64, c->ob.status, 256, hipMemcpyDeviceToHost));
    return OLF_OK;
}

int olf_debug_copy_bandwidth(olf_ctx* c, size_t bytes, int reps, double* gbytes_per_s)
{
    if (!c || !gbytes_per_s || bytes < 16 || reps < 1) { set_error("olf_debug_copy_bandwidth: bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_debug_copy_bandwidth"));
    void *a = nullptr, *b = nullptr;
    OLF_HIP_CHECK(hipMalloc(&a, bytes));
    if (hipMalloc(&b, bytes) != hipSuccess) { (void)hipFree(a); set_error("olf_debug_copy_bandwidth: hipMalloc failed"); return OLF_ERR_HIP; }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipMemsetAsync(a, 1, bytes, c->stream);
    int rc = olf::launch_copy16(a, b, bytes, c->stream);                    // warm-up
    (void)hipEventRecord(e0, c->stream);
    for (int i = 0; i < reps && rc == OLF_OK; ++i) rc = olf::launch_copy16(i & 1 ? b : a, i & 1 ? a : b, bytes, c->stream);
    (void)hipEventRecord(e1, c->stream);
    const hipError_t se = hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(a); (void)hipFree(b);
    if (rc != OLF_OK || se != hipSuccess || !(ms > 0)) { set_error("olf_debug_copy_bandwidth: copy failed"); return OLF_ERR_HIP; }
    *gbytes_per_s = 2.0 * (double)(bytes / 16 * 16) * reps / (ms * 1e-3) / 1e9;      // bytes read + bytes written
    return OLF_OK;
}

int olf_debug_lsd_waves(olf_ctx* c, int waves_per_image, int rob_entries)
{
    const bool pow2 = rob_entries > 0 && (rob_entries & (rob_entries - 1)) == 0;
    if (!c || waves_per_image > 16 || waves_per_image < -1 || (rob_entries != 0 && (!pow2 || rob_entries < 128 || rob_entries > 1024))) {
        set_error("olf_debug_lsd_waves: bad argument"); return OLF_ERR_INVALID;
    }
    c->lsd_force.waves = waves_per_image;
    c->lsd_force.robEntries = rob_entries;
    return OLF_OK;
}

// debug / tests: workgroups per image of the multi-wave growth (1, 2 or 4; 0: chosen from the batch size)
int olf_debug_lsd_groups(olf_ctx* c, int groups)
{
    if (!c || !(groups == 0 || groups == 1 || groups == 2 || groups == 4)) { set_error("olf_debug_lsd_groups: bad argument"); return OLF_ERR_INVALID; }
    c->lsd_force.groups = groups > 0 ? groups : -1;
    return OLF_OK;
}

// debug / tests: cap the one-wave agent's primary pixel log at `entries` (0: the context's own size): images whose logged regions need more move to the spill arena
int olf_debug_lsd_log_cap(olf_ctx* c, int entries)
{
    if (!c || entries < 0) { set_error("olf_debug_lsd_log_cap: bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_debug_lsd_log_cap"));
    LineGeom& g = c->line.geom;
    if (entries > 0 && !g.spillArena) {      // a context whose log holds every pixel has no arena of its own
        const size_t blocks = std::max<size_t>(2, (size_t)c->max_images - (size_t)c->max_images / 4);      // (tests: three quarters of the images may spill)
        void* q = nullptr;
        OLF_HIP_CHECK(hipMalloc(&q, blocks * 8 * (size_t)g.Ps));
        c->allocs.push_back(q);
        g.spillArena = static_cast<uint32_t*>(q); g.spillBlocks = (int)blocks;
    }
    g.logCap = entries > 0 ? std::min(entries, g.regionStride / 2) : g.regionStride / 2;
    OLF_HIP_CHECK(hipDeviceSynchronize());
    OLF_HIP_CHECK(hipMemcpy(c->lb.geom, &g, sizeof(LineGeom), hipMemcpyHostToDevice));
    return OLF_OK;
}

// debug / tests: deal the growth groups of an image to consecutive workgroups (different XCDs under round-robin placement) instead of to one XCD
int olf_debug_lsd_scatter(olf_ctx* c, int on)
{
    if (!c) { set_error("olf_debug_lsd_scatter: bad argument"); return OLF_ERR_INVALID; }
    c->lsd_force.scatter = on ? 1 : 0;
    return OLF_OK;
}

// debug / tests: the std::sort seed-order kernel (lsd_seedsort.hip) on a caller-supplied key array ((field << 22) | payload, sorted by the
// 10-bit field ascending exactly as libstdc++'s std::sort would leave it); kthr: only keys whose field is <= kthr are listed (-1: from the
// image statistics -- not meaningful here, pass n_bins - 1 to list everything); depth_limit: introsort's depth limit (-1: 2 * floor(log2 n))
int olf_debug_seed_sort(olf_ctx* c, const uint32_t* keys, int n, int kthr, int depth_limit, uint32_t* out, int32_t* out_n)
{
    if (!c || !keys || !out || !out_n || n < 0 || n > c->line.geom.Ps || kthr < 0 || kthr > 1023) { set_error("olf_debug_seed_sort: bad argument"); return OLF_ERR_INVALID; }
    HostCall h(c, "olf_debug_seed_sort");
    OLF_TRY(h.begin());
    OLF_TRY(h.up(c->lb.keysA, keys, (size_t)n * 4));
    OLF_TRY(launch_lsd_seedsort(c->line.geom, c->lb, lsd_plan(c->line.geom, c->lb, c->lsd_force, c->limits, 1), 1, h.stream(), n, kthr, depth_limit));
    OLF_TRY(h.down_counted(out_n, c->lb.keyCount, 1, out, c->lb.keysB, n, out_n));
    OLF_TRY(h.finish());
    if (*out_n < 0 || *out_n > n) { set_error("olf_debug_seed_sort: count out of range"); return OLF_ERR_HIP; }
    return OLF_OK;
}

// debug / tests: the 64-bit seed-order kernel (lsd_wide.hip) on a caller-supplied key array (field << 32 | payload); full = 0: compared by the field alone, the
// order libstdc++'s std::sort leaves (convention C.9 variant 1); full = 1: compared as whole words (variant 0); kthr: the keys whose field is <= kthr are listed;
// depth_limit: introsort's depth limit (-1: 2 * floor(log2 n)).  out receives the listed keys' payloads (the pixel addresses) in order.
int olf_debug_seed_sort_wide(olf_ctx* c, const uint64_t* keys, int n, int64_t kthr, int depth_limit, int full, uint32_t* out, int32_t* out_n)
{
    if (!c || !keys || !out || !out_n || n < 0 || n > c->line.geom.Ps || kthr < 0 || kthr > 0xffffffffll || !c->line.geom.wide) {
        set_error("olf_debug_seed_sort_wide: bad argument (the context must be a wide one: lsd_n_bins > 1024 or 2^22 pixels and more)"); return OLF_ERR_INVALID; }
    HostCall h(c, "olf_debug_seed_sort_wide");
    OLF_TRY(h.begin());
    OLF_TRY(h.up(c->lb.keysA, keys, (size_t)n * 8));
    OLF_TRY(launch_lsd_sort_wide(c->line.geom, c->lb, 1, h.stream(), n, (long long)kthr, depth_limit, full ? 1 : 0));
    OLF_TRY(h.down_counted(out_n, c->lb.keyCount, 1, out, c->lb.keysB, n, out_n));
    OLF_TRY(h.finish());
    if (*out_n < 0 || *out_n > n) { set_error("olf_debug_seed_sort_wide: count out of range"); return OLF_ERR_HIP; }
    return check_status(c);
}

// debug / tests: which seed-sort kernel runs (-1: chosen from the batch size; 0: one wave per image; 1 / 2 / 5: 4 / 8 / 2 waves per image)
int olf_debug_seed_sort_mode(olf_ctx* c, int mode)
{
    if (!c || mode < -1 || mode == 3 || mode == 4 || mode > 5) { set_error("olf_debug_seed_sort_mode: bad argument"); return OLF_ERR_INVALID; }
    c->lsd_force.sortMode = mode;
    return OLF_OK;
}

// debug / tests: cap the chunk pool of the multi-wave growth (0: the whole pool) so that the fall-back to the one-wave agent can be exercised
int olf_debug_lsd_pool(olf_ctx* c, int pool_chunks)
{
    if (!c || pool_chunks < 0) { set_error("olf_debug_lsd_pool: bad argument"); return OLF_ERR_INVALID; }
    c->lsd_force.poolChunks = pool_chunks;
    return OLF_OK;
}

// debug: the regions logged by the last growth for `image`, in detection order: (first chunk or list start, pixels, final region angle) triples
int olf_debug_lsd_regions(olf_ctx* c, int image, int32_t* start_n /* [cap][2] */, double* angle, int cap, int32_t* count)
{
    if (!c || !start_n || !angle || !count || image < 0 || image >= c->max_images) return OLF_ERR_INVALID;
    OLF_HIP_CHECK(hipDeviceSynchronize());
    int nr = 0;
    OLF_HIP_CHECK(hipMemcpy(&nr, c->lb.regCount + image, sizeof(int), hipMemcpyDeviceToHost));
    *count = nr;
    struct Rec { int start, n; double angle; };
    std::vector<Rec> r((size_t)std::min(nr, cap));
    if (!r.empty())
        OLF_HIP_CHECK(hipMemcpy(r.data(), reinterpret_cast<const Rec*>(c->lb.keysA) + (size_t)image * c->line.geom.maxRegions, r.size() * sizeof(Rec), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < r.size(); ++i) { start_n[2 * i] = r[i].start; start_n[2 * i + 1] = r[i].n; angle[i] = r[i].angle; }
    return OLF_OK;
}

// debug: the owner words (seed rank << 10 | ROB slot, 0xffffffff = never claimed) the last multi-region growth left for `image` (Ws*Hs words)
int olf_debug_lsd_owner(olf_ctx* c, int image, uint32_t* out)
{
    if (!c || !out || image < 0 || image >= c->lb.ownerImages) return OLF_ERR_INVALID;
    OLF_HIP_CHECK(hipDeviceSynchronize());
    OLF_HIP_CHECK(hipMemcpy(out, c->lb.owner + (size_t)image * c->line.geom.Ps, (size_t)c->line.geom.Ps * 4, hipMemcpyDeviceToHost));
    return OLF_OK;
}

int olf_debug_status_n(olf_ctx* c, int32_t* out, int n)
{
    if (!c || !out || n < 1 || n > 256) return OLF_ERR_INVALID;
    OLF_HIP_CHECK(hipDeviceSynchronize());
    OLF_HIP_CHECK(hipMemcpy(out, c->ob.status, (size_t)n * 4, hipMemcpyDeviceToHost));
    return OLF_OK;
}

int olf_debug_fdiv_sweep(olf_ctx* c, uint64_t seed, int blocks, int per_thread, uint64_t* mismatches)
{
    if (!c || !mismatches || blocks < 1 || per_thread < 1) { set_error("olf_debug_fdiv_sweep: bad argument"); return OLF_ERR_INVALID; }
    HostCall h(c, "olf_debug_fdiv_sweep");
    unsigned long long* st;
    OLF_TRY(sweep_counters(h, &st, 1));
    OLF_TRY(launch_fdiv_sweep((unsigned long long)seed, blocks, per_thread, st, h.stream()));
    OLF_TRY(h.down(mismatches, st, 8));
    return h.finish();
}

int olf_debug_sqrtq_sweep(olf_ctx* c, int count, uint64_t* mismatches)
{
    if (!c || !mismatches || count < 1) { set_error("olf_debug_sqrtq_sweep: bad argument"); return OLF_ERR_INVALID; }
    HostCall h(c, "olf_debug_sqrtq_sweep");
    unsigned long long* st;
    OLF_TRY(sweep_counters(h, &st, 1));
    OLF_TRY(launch_sqrtq_sweep(count, st, h.stream()));
    OLF_TRY(h.down(mismatches, st, 8));
    return h.finish();
}

int olf_debug_align_sweep(olf_ctx* c, uint64_t seed, int blocks, int per_thread, uint64_t* out3)
{
    if (!c || !out3 || blocks < 1 || per_thread < 1) { set_error("olf_debug_align_sweep: bad argument"); return OLF_ERR_INVALID; }
    if (c->line.geom.alignTanLo < 0.f) { set_error("olf_debug_align_sweep: the cheap alignment test is off for lsd_ang_th > 80 degrees"); return OLF_ERR_INVALID; }
    HostCall h(c, "olf_debug_align_sweep");
    unsigned long long* st;
    OLF_TRY(sweep_counters(h, &st, 3));
    OLF_TRY(launch_align_sweep(c->lb, (unsigned long long)seed, blocks, per_thread, st, h.stream()));
    OLF_TRY(h.down(out3, st, 24));
    return h.finish();
}

int olf_orb_debug_candidates(olf_ctx* c, int image, int level, int32_t* xys, int cap, int32_t* count)
{
    if (!c || !xys || !count || image < 0 || image >= c->max_images || level < 0 || level >= c->orb.geom.nlevels) return OLF_ERR_INVALID;
    const OrbGeom& g = c->orb.geom;
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    int n = 0;
    OLF_HIP_CHECK(hipMemcpy(&n, c->ob.candCount + image * g.nlevels + level, sizeof(int), hipMemcpyDeviceToHost));
    *count = n;
    std::vector<uint32_t> tmp(std::max(n, 1));
    OLF_HIP_CHECK(hipMemcpy(tmp.data(), c->ob.cand + (size_t)image * g.candTotal + g.lv[level].candBase, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < std::min(n, cap); ++i) {
        xys[3 * i] = tmp[i] >> 20; xys[3 * i + 1] = (tmp[i] >> 8) & 0xfff; xys[3 * i + 2] = tmp[i] & 0xff;
    }
    return OLF_OK;
}

int olf_lsd_debug_scaled(olf_ctx* c, int image, uint8_t* dst, int32_t* ws, int32_t* hs)
{
    if (!c || !dst || image < 0 || image >= c->max_images) return OLF_ERR_INVALID;
    if (c->scaled_aliased) { set_error("olf_lsd_debug_scaled: a batch context does not keep the enlarged image (use a context of at most 2048 images)"); return OLF_ERR_INVALID; }
    const LineGeom& g = c->line.geom;
    OLF_HIP_CHECK(hipDeviceSynchronize());
    OLF_HIP_CHECK(hipMemcpy2D(dst, g.Ws, c->lb.scaled + (size_t)image * g.pitchS * g.Hs, g.pitchS, g.Ws, g.Hs, hipMemcpyDeviceToHost));
    if (ws) *ws = g.Ws;
    if (hs) *hs = g.Hs;
    return OLF_OK;
}

}  // extern "C"
