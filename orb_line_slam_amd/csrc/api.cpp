// api.cpp -- the extern "C" boundary of liborbline_hip.so (include/orbline.h): the context, its status and profiling, the stages, the _dev entries
// and the fused frame call.  (api_host.cpp: the host-pointer entries; api_debug.cpp: the entries that read intermediate buffers for the tests.)
// Owns the device context; every compute entry point launches HIP kernels -- there is no CPU
// fallback: without a gfx950 device olf_ctx_create fails with OLF_ERR_NODEVICE.
#include "ctx.hpp"
#include "staging.hpp"
#include <map>
#include <mutex>

namespace olf {
static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }

int check_device(const olf_ctx* c, const char* who)
{
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess || d != c->device) { set_error(std::string(who) + ": the context belongs to another device than the current one"); return OLF_ERR_INVALID; }
    return OLF_OK;
}

// the detectors (ORB, LSD) run in landscape contexts only; a portrait context (include/orbline.h, olf_ctx_create) describes and matches what the caller supplies
static int check_landscape(const olf_ctx* c, const char* who)
{
    if (c->orb.portrait) {
        set_error(std::string(who) + ": the context's image is portrait (a pyramid level's octree would have round(width / height) == 0 root cells, where the "
                                     "reference divides by zero): no detector runs in it");
        return OLF_ERR_INVALID;
    }
    return OLF_OK;
}

int scratch_get(olf_ctx* c, ScratchSlot slot, size_t bytes, void** out)
{
    if (c->scratch_bytes[slot] < bytes) {
        if (c->scratch[slot]) { OLF_HIP_CHECK(hipDeviceSynchronize()); (void)hipFree(c->scratch[slot]); c->scratch[slot] = nullptr; c->scratch_bytes[slot] = 0; }
        size_t want = std::max<size_t>(bytes * 3 / 2, 4096);
        OLF_HIP_CHECK(hipMalloc(&c->scratch[slot], want));
        c->scratch_bytes[slot] = want;
    }
    *out = c->scratch[slot];
    return OLF_OK;
}

int check_status(olf_ctx* c)
{
    int st[4] = {0, 0, 0, 0};
    OLF_HIP_CHECK(hipMemcpy(st, c->ob.status, sizeof(st), hipMemcpyDeviceToHost));
    if (st[0]) {
        (void)hipMemset(c->ob.status, 0, 16);
        std::string what;                                           // the set bits, each with its row of kStatusText
        for (const StatusText& t : kStatusText)
            if (st[0] & t.bit) what += (what.empty() ? "" : ", ") + std::to_string(t.bit) + ": " + t.text;
        set_error("device capacity overflow, flags=" + std::to_string(st[0]) + " (" + what + ")");
        return OLF_ERR_CAPACITY;
    }
    return OLF_OK;
}

int join_if_pending(olf_ctx* c, hipStream_t s)
{
    if (!c->join_pending) return OLF_OK;
    OLF_HIP_CHECK(hipStreamWaitEvent(s, c->ev_join, 0));
    if (s == c->pend_stream) c->join_pending = false;      // (a side stream's wait orders the side stream only)
    return OLF_OK;
}
bool in_pending_line_outputs(const olf_ctx* c, const void* p)
{
    if (!c->join_pending || !p) return false;
    const uint8_t* q = static_cast<const uint8_t*>(p);
    for (const auto& r : c->pend) if (r.p && q >= r.p && q < r.p + r.bytes) return true;
    return false;
}

hipEvent_t prof_event(olf_ctx* c)
{
    if (!c->prof_pool.empty()) { hipEvent_t e = c->prof_pool.back(); c->prof_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
}  // namespace olf

using namespace olf;

// The LSD angle / cos-sin tables depend on nothing but the packed gradient pair: one copy per device, shared by every context of the process
// (a reference Frame is served by four extractor objects, each with a context of its own; include/orbline_adaptor.hpp).
namespace {
struct AngleTables { float* angDeg = nullptr; void* angEnt = nullptr; int refs = 0; };
std::mutex g_tab_mu;
std::map<int, AngleTables> g_tabs;

// (one table per device AND per convention C.6 variant: the entries' cos / sin differ between them)
int angle_tables_acquire(int device, int libmFloat, LineDeviceBufs& l, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_tab_mu);
    AngleTables& t = g_tabs[device * 2 + (libmFloat ? 1 : 0)];
    if (t.refs == 0) {
        if (hipMalloc(&t.angDeg, sizeof(float) << 22) != hipSuccess || hipMalloc(&t.angEnt, (size_t)32 << 22) != hipSuccess) {
            (void)hipFree(t.angDeg); (void)hipFree(t.angEnt);
            t = AngleTables();
            set_error("hipMalloc failed (LSD angle tables)");
            return OLF_ERR_HIP;
        }
        l.angDeg = t.angDeg; l.angEnt = t.angEnt;
        if (launch_lsd_angle_table(l, libmFloat, s) != OLF_OK || hipStreamSynchronize(s) != hipSuccess) {
            (void)hipFree(t.angDeg); (void)hipFree(t.angEnt);
            t = AngleTables();
            set_error("LSD angle table build failed");
            return OLF_ERR_HIP;
        }
    }
    ++t.refs;
    l.angDeg = t.angDeg; l.angEnt = t.angEnt;
    return OLF_OK;
}

void angle_tables_release(int device, int libmFloat)
{
    std::lock_guard<std::mutex> lk(g_tab_mu);
    auto it = g_tabs.find(device * 2 + (libmFloat ? 1 : 0));
    if (it == g_tabs.end() || it->second.refs <= 0) return;
    if (--it->second.refs == 0) {
        (void)hipFree(it->second.angDeg); (void)hipFree(it->second.angEnt);
        g_tabs.erase(it);
    }
}
}  // namespace

namespace olf {
int launch_pack_records(const olf_frame_buffers& fb, int n_pairs, int cap, int lcap, uint8_t* d_dst, size_t dst_capacity, int* d_rowOfs,
                        unsigned long long* d_bytes, int* d_status, hipStream_t s);
size_t pack_records_bound(int n_pairs, int cap, int lcap);
int launch_depth_mask(const float* depth, uint8_t* mask, size_t n, hipStream_t s);
}

namespace olf {
int ctx_join_line_outputs(olf_ctx* c, hipStream_t s, const void* p0, const void* p1, const void* p2, const void* p3)
{
    if (in_pending_line_outputs(c, p0) || in_pending_line_outputs(c, p1) || in_pending_line_outputs(c, p2) || in_pending_line_outputs(c, p3)) return join_if_pending(c, s);
    return OLF_OK;
}
hipStream_t ctx_stream(olf_ctx* c, void* stream) { return stream ? static_cast<hipStream_t>(stream) : c->stream; }
int ctx_scratch(olf_ctx* c, ScratchSlot slot, size_t bytes, void** out) { return scratch_get(c, slot, bytes, out); }
int* ctx_status(olf_ctx* c) { return c->ob.status; }
int ctx_check_device(const olf_ctx* c, const char* who) { return check_device(c, who); }
int ctx_check_status(olf_ctx* c) { return check_status(c); }
int ctx_level_scales(const olf_ctx* c, float* sf)
{
    const int n = std::min(c->params.orb.nlevels, (int)OLF_MAX_LEVELS);
    for (int l = 0; l < OLF_MAX_LEVELS; ++l) sf[l] = l < n ? c->orb.sf[l] : 1.f;
    return n;
}
int ctx_level_inv_sigma2(const olf_ctx* c, float* inv_sigma2)
{
    float sf[OLF_MAX_LEVELS];
    const int n = ctx_level_scales(c, sf);
    for (int l = 0; l < OLF_MAX_LEVELS; ++l) { const float sigma2 = sf[l] * sf[l]; inv_sigma2[l] = 1.0f / sigma2; }      // src/ORBextractor.cc:434-436
    return n;
}
int ctx_level_thresholds(olf_ctx* c, float* thr)
{
    const int n = c->params.orb.nlevels;
    if (c->level_thr_rc > 0) c->level_thr_rc = n <= OLF_MAX_LEVELS ? olf_predict_scale_thresholds(c->orb.sf.data(), n, c->level_thr) : OLF_ERR_INVALID;
    for (int k = 0; k + 1 < n && c->level_thr_rc == OLF_OK; ++k) thr[k] = c->level_thr[k];
    return c->level_thr_rc;
}
}

static const char* kStageNames[ST_COUNT] = {"orb_pyramid", "orb_fast_cells", "orb_octree", "orb_blur", "orb_describe", "stereo_points",
                                            "lsd_front", "lsd_grow", "lsd_rect", "line_select_lbd", "stereo_lines", "match_bf"};

template <typename T>
static int dev_alloc(olf_ctx* c, T** p, size_t n)
{
    void* q = nullptr;
    OLF_HIP_CHECK(hipMalloc(&q, std::max<size_t>(n * sizeof(T), 256)));
    c->allocs.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return OLF_OK;
}

extern "C" {

const char* olf_last_error(void) { return g_err.c_str(); }

int olf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int olf_default_params(olf_params* p)
{
    if (!p) return OLF_ERR_INVALID;
    std::memset(p, 0, sizeof(*p));
    p->abi_version = OLF_ABI_VERSION; p->struct_size = (uint32_t)sizeof(olf_params);
    p->orb.nfeatures = 2000; p->orb.scale_factor = 1.2f; p->orb.nlevels = 8; p->orb.ini_th_fast = 20; p->orb.min_th_fast = 7;
    p->line.lsd_nfeatures = 500; p->line.min_line_length = 0.025; p->line.lsd_refine = 0; p->line.lsd_scale = 1.2;
    p->line.lsd_sigma_scale = 0.6; p->line.lsd_quant = 2.0; p->line.lsd_ang_th = 22.5; p->line.lsd_log_eps = 1.0;
    p->line.lsd_density_th = 0.6; p->line.lsd_n_bins = 1024;
    p->line.conv_seed_order = 1;      // OpenCV >= 3.3 (the reference asks for 3.4 first, CMakeLists.txt:37-43): std::sort seed order
    p->stereo.fx = 718.856f; p->stereo.bf = 386.1448f; p->stereo.matching_s_ws = 10; p->stereo.line_sim_th = 0.75;
    p->stereo.min_ratio_12_l = 0.9; p->stereo.min_disp = 1.0; p->stereo.line_horiz_th = 0.1; p->stereo.stereo_overlap_th = 0.75;
    p->stereo.ls_min_disp_ratio = 0.7; p->stereo.best_lr_matches = 1;
    return OLF_OK;
}

void olf_ctx_destroy(olf_ctx* c)
{
    if (!c) return;
    if (c->has_tables) angle_tables_release(c->device, c->params.line.conv_libm_float);
    if (c->h_outslab) (void)hipHostFree(c->h_outslab);
    for (void* p : c->allocs) (void)hipFree(p);
    for (void* p : c->scratch) if (p) (void)hipFree(p);
    for (auto& r : c->prof_recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (hipEvent_t e : c->prof_pool) (void)hipEventDestroy(e);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_front) (void)hipEventDestroy(c->ev_front);
    if (c->ev_sort) (void)hipEventDestroy(c->ev_sort);
    if (c->ev_lbd) (void)hipEventDestroy(c->ev_lbd);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int olf_ctx_create(const olf_params* p, int width, int height, int max_images, olf_ctx** out)
{
    if (!p || !out || width < 64 || height < 64 || max_images < 1) { set_error("olf_ctx_create: bad argument"); return OLF_ERR_INVALID; }
    *out = nullptr;
    if (p->abi_version != OLF_ABI_VERSION || p->struct_size != (uint32_t)sizeof(olf_params)) {
        set_error("olf_ctx_create: the parameter block was not initialised by this library's olf_default_params() (abi_version / struct_size differ: "
                  "caller built against another include/orbline_types.h)");
        return OLF_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        set_error("olf_ctx_create: no HIP device visible (this library has no CPU path)");
        return OLF_ERR_NODEVICE;
    }
    olf_ctx* c = new olf_ctx();
    c->params = *p; c->W = width; c->H = height; c->max_images = max_images;
    int rc = c->orb.build(p->orb, width, height);
    if (rc != OLF_OK) {
        set_error(rc == OLF_ERR_CAPACITY ? "olf_ctx_create: more than 32760 key points on one pyramid level (nfeatures too large for this scale factor / level count)"
                  : (width > kMaxOrbSide || height > kMaxOrbSide) ? "olf_ctx_create: image wider or higher than 4131 pixels (FAST candidates are packed with 12 bits per coordinate)"
                                         : "olf_ctx_create: image size / ORB parameters not supported (every pyramid level needs at least 62 x 62 pixels)");
        delete c; return rc;
    }
    auto fail = [&](int code) { olf_ctx_destroy(c); return code; };
    if (hipGetDevice(&c->device) != hipSuccess) return fail(OLF_ERR_HIP);
    if (hipDeviceGetAttribute(&c->limits.nCU, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || c->limits.nCU <= 0) c->limits.nCU = 64;
    if (hipDeviceGetAttribute(&c->limits.maxLds, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device) != hipSuccess) c->limits.maxLds = 64 * 1024;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); return fail(OLF_ERR_HIP); }
    const OrbGeom& g = c->orb.geom;
    const size_t n = (size_t)max_images;
    OrbDeviceBufs& b = c->ob;
    const bool allocTrace = getenv("OLF_ALLOC_TRACE") != nullptr;      // (tools/mem_per_pair.py: every buffer of the context, per image)
#define A(ptr, count) do { if ((rc = dev_alloc(c, &(ptr), (count))) != OLF_OK) return fail(rc); \
                           if (allocTrace) fprintf(stderr, "alloc %-18s %8.3f MB per image\n", #ptr, (double)(count) * sizeof(*(ptr)) / 1e6 / (double)n); } while (0)
    A(b.pyr, n * g.pyrBytes); A(b.blur, n * g.pyrBytes);
    A(b.cells, n * g.totalCells * g.cellCap); A(b.cellCount, n * g.totalCells);
    A(b.cand, n * g.candTotal); A(b.candNode, n * g.candTotal); A(b.candCount, n * g.nlevels);
    if (g.maxNodes > 2048) A(b.octSpill, n * g.nlevels * octree_spill_bytes(g));
    A(b.lvlKp, n * g.kpTotal); A(b.lvlCount, n * g.nlevels); A(b.lvlAngle, n * g.kpTotal);
    A(b.rx, c->orb.rx.size() + 1); A(b.ry, c->orb.ry.size() + 1); A(b.geom, 1); A(b.status, 256);
    A(c->d_sad, ((n + 1) / 2) * g.outCap); A(c->d_bestkey, ((n + 1) / 2) * g.outCap); A(c->d_rowperm, n * g.outCap);
    A(c->d_images, n * width * height);
#undef A
    if (hipMemcpy(b.rx, c->orb.rx.data(), c->orb.rx.size() * sizeof(ResizeCoef), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b.ry, c->orb.ry.data(), c->orb.ry.size() * sizeof(ResizeCoef), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b.geom, &g, sizeof(OrbGeom), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(b.status, 0, 1024) != hipSuccess) {
        set_error("olf_ctx_create: table upload failed");
        return fail(OLF_ERR_HIP);
    }
    // ---- line side ----
    rc = c->line.build(p->line, width, height, max_images);
    if (rc != OLF_OK) { set_error("olf_ctx_create: LSD parameters not supported"); return fail(rc); }
    LineGeom& lg = c->line.geom;
    // The line stream gets a priority of its own.  The runtime multiplexes streams onto a few hardware queues, and two streams of the SAME priority can land on
    // one queue: the line path and the caller's stream then run back to back (measured: the host-to-host pipeline at 330 ms per 3072-pair batch instead of 220
    // whenever the caller's compute stream and this one aliased, profiles/r4aq_stream_queue_aliasing.txt).  Streams of different priorities never share a queue.
    // The least priority leaves the high level to a caller's copy streams (pipeline.py); the step time was the same with the high one and with the caller's
    // level (226-231 ms on one box).
    int prLeast = 0, prGreatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prLeast, &prGreatest);
    if (hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prLeast) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_front, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_sort, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_lbd, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) { set_error("stream/event creation failed"); return fail(OLF_ERR_HIP); }
    LineDeviceBufs& l = c->lb;
#define A(ptr, count) do { if ((rc = dev_alloc(c, &(ptr), (count))) != OLF_OK) return fail(rc); \
                           if (allocTrace) fprintf(stderr, "alloc %-18s %8.3f MB per image\n", #ptr, (double)(count) * sizeof(*(ptr)) / 1e6 / (double)n); } while (0)
    // batch contexts (> kBatchCtxImages images): the LSD blur and the enlarged working image are dead before the key kernel / the seed sort write the key
    // buffers (one stream, kernels in order): they live there
    const bool batchCtx = n > (size_t)kBatchCtxImages;
    const size_t keyWords = lg.wide ? 2 : 1;      // (64-bit sort keys: lsd_wide.hip)
    A(l.grad, n * lg.Ps); A(l.keysA, n * lg.Ps * keyWords); A(l.keysB, n * lg.Ps * keyWords);
    if (batchCtx && lg.Ps * 4 >= lg.pitchW * lg.H && lg.Ps * 4 >= lg.pitchS * lg.Hs) { l.lsdBlur = reinterpret_cast<uint8_t*>(l.keysA); l.scaled = reinterpret_cast<uint8_t*>(l.keysB); c->scaled_aliased = true; }
    else { A(l.lsdBlur, n * lg.pitchW * lg.H); A(l.scaled, n * lg.pitchS * lg.Hs); }
    A(l.topBuf, n * (size_t)lsd_seedsort_top_words()); A(l.keyCount, n * 32); A(l.maxN, n * 32); A(l.chunkCnt, n * ((lg.Ps + 4095) / 4096)); A(l.sortHist, n * (size_t)lsd_sort_max_chunks(lg.Ps) * 32); A(l.sortBase, n * 32);
    // chunk pool of the multi-wave growth: every pixel in a list once (Ps / 32) plus one partly filled chunk per logged region and ROB slot;
    // at least the 2 * Ps words the one-wave agent's log needs (LineGeom::regionStride, one stride for both formats).  An image that still runs out is
    // grown again by the one-wave agent (launch_lsd_grow)
    l.nChunks = lg.regionStride / 32;
    // region: chunk pool of the multi-wave growth / 8-byte (pixel, gradient word) log of the one-wave agent
    // (batch contexts: the one-wave agent only -- no owner words, a log sized by a bound (host_tables.cpp) and a spill arena of full-size logs for the images that outgrow it)
    A(l.region, n * (size_t)lg.regionStride); l.ownerImages = (batchCtx || lg.wide) ? 0 : (int)std::min<size_t>(n, kMwMaxImages); A(l.owner, (size_t)l.ownerImages * lg.Ps); A(l.links, n * (size_t)l.nChunks);
    // (a full-size log never spills: other contexts get an arena only when olf_debug_lsd_log_cap asks for one)
    lg.logCap = lg.regionStride / 2;
    lg.spillBlocks = lg.regionStride / 2 >= lg.Ps ? 0 : (int)std::max<size_t>(4, n / 16);      // (one image in 16 may have more than half of its pixels in logged regions)
    if (lg.spillBlocks) A(lg.spillArena, (size_t)lg.spillBlocks * 2 * lg.Ps);
    A(lg.spillCtl, 64); A(lg.spillOf, n);
    l.mgImages = (int)std::min<size_t>(n, kMgMaxImages); l.mgStride = lsd_grow_mg_stride(lg.maxRegions);
    A(l.mg, (size_t)l.mgImages * l.mgStride);
    A(l.rawLines, n * lg.maxDetect); A(l.rawCount, n); A(l.regCount, n); A(l.growFmt, n); A(l.lbdBlur, n * lg.pitchW * lg.H); A(l.dxdy, n * lg.pitchD * lg.H);
    A(l.rowSums, n * lg.outCap * 63 * 4); A(l.lbdStarts, n * lg.outCap * 64 * 2); A(l.rx, c->line.rx.size()); A(l.ry, c->line.ry.size()); A(l.geom, 1);
    A(c->d_ldist, ((n + 1) / 2) * lg.outCap * lg.outCap); A(c->d_lm21, ((n + 1) / 2) * lg.outCap);
    if (hipMalloc(&c->d_lprep, stereo_lines_prep_bytes((int)n, lg.outCap)) != hipSuccess) { set_error("hipMalloc failed"); return fail(OLF_ERR_HIP); }
    c->allocs.push_back(c->d_lprep);
    // the output arrays: one slab for small contexts (256-byte aligned offsets), an allocation each otherwise
    const bool slab = n <= 16;
    if (slab) {
        size_t off = 0;
        for (int k = 0; k < FB_FIELDS; ++k) { c->outslab_off[k] = off; off += (fb_bytes(c, k, n) + 255) & ~(size_t)255; }
        c->outslab_bytes = off;
        A(c->d_outslab, off);
        if (hipHostMalloc(reinterpret_cast<void**>(&c->h_outslab), off, hipHostMallocDefault) != hipSuccess) { set_error("hipHostMalloc failed"); return fail(OLF_ERR_HIP); }
    }
    for (int k = 0; k < FB_FIELDS; ++k) {
        uint8_t* q = nullptr;
        if (slab) q = c->d_outslab + c->outslab_off[k];
        else if ((rc = dev_alloc(c, &q, fb_bytes(c, k, n))) != OLF_OK) return fail(rc);
        fb_set_field(c->d_out, k, q);
        if (allocTrace) fprintf(stderr, "alloc %-18s %8.3f MB per image\n", kFrameFields[k].name, (double)fb_bytes(c, k, n) / 1e6 / (double)n);
    }
#undef A
    l.status = b.status;
    if (hipMemcpy(l.rx, c->line.rx.data(), c->line.rx.size() * sizeof(ResizeCoef), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(l.ry, c->line.ry.data(), c->line.ry.size() * sizeof(ResizeCoef), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(l.geom, &lg, sizeof(LineGeom), hipMemcpyHostToDevice) != hipSuccess) { set_error("line table upload failed"); return fail(OLF_ERR_HIP); }
    if ((rc = angle_tables_acquire(c->device, p->line.conv_libm_float, l, c->stream)) != OLF_OK) return fail(rc);
    c->has_tables = true;
    *out = c;
    return OLF_OK;
}

int olf_ctx_synchronize(olf_ctx* c)
{
    if (!c) return OLF_ERR_INVALID;
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream));
    OLF_HIP_CHECK(hipStreamSynchronize(c->stream2));
    c->join_pending = false;            // (both streams are idle: nothing is left to wait for)
    return check_status(c);
}

int olf_ctx_set_input_event(olf_ctx* c, void* hip_event)
{
    if (!c) return OLF_ERR_INVALID;
    c->input_event = static_cast<hipEvent_t>(hip_event);
    return OLF_OK;
}

int olf_ctx_poll_status(olf_ctx* c)
{
    if (!c) return OLF_ERR_INVALID;
    return check_status(c);
}

// ---- stage profiling: HIP events on the launching streams -------------------------------------
int olf_profile_enable(olf_ctx* c, int on)
{
    if (!c) return OLF_ERR_INVALID;
    c->prof_on = on != 0;
    return OLF_OK;
}

static int prof_collect(olf_ctx* c)
{
    OLF_HIP_CHECK(hipDeviceSynchronize());
    for (auto& r : c->prof_recs) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { c->prof_ms[r.stage] += ms; c->prof_calls[r.stage] += 1; }
        c->prof_pool.push_back(r.a); c->prof_pool.push_back(r.b);
    }
    c->prof_recs.clear();
    return OLF_OK;
}

int olf_profile_reset(olf_ctx* c)
{
    if (!c) return OLF_ERR_INVALID;
    OLF_TRY(prof_collect(c));
    for (int i = 0; i < 16; ++i) { c->prof_ms[i] = 0; c->prof_calls[i] = 0; }
    return OLF_OK;
}

int olf_profile_stage_count(void) { return ST_COUNT; }
const char* olf_profile_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }

int olf_profile_read(olf_ctx* c, double* total_ms, int32_t* calls)
{
    if (!c || !total_ms || !calls) return OLF_ERR_INVALID;
    OLF_TRY(prof_collect(c));
    for (int i = 0; i < ST_COUNT; ++i) { total_ms[i] = c->prof_ms[i]; calls[i] = c->prof_calls[i]; }
    return OLF_OK;
}

int olf_orb_scale_tables(const olf_ctx* c, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2, int32_t* fpl)
{
    if (!c) return OLF_ERR_INVALID;
    for (int i = 0; i < c->params.orb.nlevels; ++i) {
        if (scale) scale[i] = c->orb.sf[i];
        if (inv_scale) inv_scale[i] = c->orb.inv_sf[i];
        if (sigma2) sigma2[i] = c->orb.sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = c->orb.inv_sigma2[i];
        if (fpl) fpl[i] = c->orb.nPerLevel[i];
    }
    return OLF_OK;
}

int olf_orb_level_sizes(const olf_ctx* c, int32_t* widths, int32_t* heights)
{
    if (!c) return OLF_ERR_INVALID;
    for (int i = 0; i < c->orb.geom.nlevels; ++i) { widths[i] = c->orb.geom.lv[i].w; heights[i] = c->orb.geom.lv[i].h; }
    return OLF_OK;
}

int olf_orb_capacity(const olf_ctx* c) { return c ? c->orb.geom.outCap : OLF_ERR_INVALID; }

// ---- the stages: each opens its StageScope on the stream it is launched on and calls its launcher.  The entries below list them in the order they enqueue them
static int stage_orb_pyramid(olf_ctx* c, const uint8_t* d_images, int n, hipStream_t s) { StageScope t(c, s, ST_ORB_PYRAMID); return launch_orb_pyramid(c->orb.geom, c->ob, d_images, n, s); }
static int stage_orb_fast(olf_ctx* c, int n, hipStream_t s) { StageScope t(c, s, ST_ORB_FAST); return launch_orb_fast(c->orb.geom, c->ob, n, s); }
static int stage_orb_octree(olf_ctx* c, int n, hipStream_t s) { StageScope t(c, s, ST_ORB_OCTREE); return launch_orb_octree(c->orb.geom, c->ob, n, s); }
static int stage_orb_blur(olf_ctx* c, int n, hipStream_t s) { StageScope t(c, s, ST_ORB_BLUR); return launch_orb_blur(c->orb.geom, c->ob, n, s); }
static int stage_orb_describe(olf_ctx* c, int n, olf_keypoint* kps, uint8_t* desc, int32_t* counts, hipStream_t s) { StageScope t(c, s, ST_ORB_DESCRIBE); return launch_orb_describe(c->orb.geom, c->ob, n, kps, desc, counts, c->orb.geom.outCap, s); }
static int stage_stereo_points(olf_ctx* c, int n_pairs, const olf_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_counts, float* d_uright, float* d_depth, hipStream_t s)
{
    StageScope t(c, s, ST_STEREO_POINTS);
    return launch_stereo_points(c->orb.geom, c->ob, n_pairs, d_kps, d_desc, d_counts, c->orb.geom.outCap, c->params.stereo.bf, c->params.stereo.fx, d_uright, d_depth,
                                c->d_sad, c->d_bestkey, c->d_rowperm, s);
}
// (dense half, seed order; olf_stereo_frames_dev records an event between the two and spells them out)
static int stage_lsd_front(olf_ctx* c, const LsdPlan& plan, const uint8_t* d_images, int n, hipStream_t s, bool writeScaled)
{
    StageScope t(c, s, ST_LSD_FRONT);
    OLF_TRY(launch_lsd_dense(c->line.geom, c->lb, plan, d_images, c->W, n, s, writeScaled));
    return launch_lsd_seed_order(c->line.geom, c->lb, plan, n, s);
}
static int stage_lsd_grow(olf_ctx* c, const LsdPlan& plan, int n, hipStream_t s) { StageScope t(c, s, ST_LSD_GROW); return launch_lsd_grow(c->line.geom, c->lb, plan, n, s); }
static int stage_lsd_rect(olf_ctx* c, const LsdPlan& plan, int n, hipStream_t s) { StageScope t(c, s, ST_LSD_RECT); return launch_lsd_rect(c->line.geom, c->lb, plan, n, s); }
// (selection, LBD gradient images, descriptors; olf_stereo_frames_dev has the gradient images from its ORB stream and spells the rest out)
static int stage_line_lbd(olf_ctx* c, const uint8_t* d_images, int n, olf_keyline* d_kls, uint8_t* d_ldesc, int32_t* d_lcounts, hipStream_t s)
{
    StageScope t(c, s, ST_LINE_LBD);
    OLF_TRY(launch_line_select(c->line.geom, c->lb, n, d_kls, d_lcounts, s));
    OLF_TRY(launch_lbd_dense(c->line.geom, c->lb, d_images, c->W, n, s));
    return launch_lbd_desc(c->line.geom, c->lb, n, d_kls, d_ldesc, d_lcounts, true, s);
}
static int stage_stereo_lines(olf_ctx* c, int n_pairs, const olf_keyline* d_kls, const uint8_t* d_ldesc, const int32_t* d_lcounts, int32_t* d_m12, float* d_disp, double* d_le, hipStream_t s)
{
    StageScope t(c, s, ST_STEREO_LINES);
    return launch_stereo_lines(c->W, c->H, c->params.stereo, n_pairs, d_kls, d_ldesc, d_lcounts, c->line.geom.outCap, c->d_lprep, c->d_ldist, c->d_lm21, d_m12, d_disp, d_le, s);
}

int olf_orb_extract_dev(olf_ctx* c, const uint8_t* d_images, int n_images, olf_keypoint* d_kps, uint8_t* d_desc, int32_t* d_counts,
                        void* stream)
{
    if (!c || !d_images || !d_kps || !d_desc || !d_counts) { set_error("olf_orb_extract_dev: null argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_orb_extract_dev"));
    if (n_images < 0 || n_images > c->max_images) { set_error("olf_orb_extract_dev: n_images exceeds the context capacity"); return OLF_ERR_CAPACITY; }
    if (n_images == 0) return OLF_OK;   // ORBextractor::operator() returns silently on an empty image
    OLF_TRY(check_landscape(c, "olf_orb_extract_dev"));
    hipStream_t s = ctx_stream(c, stream);
    OLF_TRY(stage_orb_pyramid(c, d_images, n_images, s));
    OLF_TRY(stage_orb_fast(c, n_images, s));
    OLF_TRY(stage_orb_octree(c, n_images, s));
    OLF_TRY(stage_orb_blur(c, n_images, s));
    return stage_orb_describe(c, n_images, d_kps, d_desc, d_counts, s);
}

size_t olf_frames_pack_bound(const olf_ctx* c, int n_pairs)
{
    return c && n_pairs >= 0 ? olf::pack_records_bound(n_pairs, c->orb.geom.outCap, c->line.geom.outCap) : 0;
}

int olf_stereo_points_mask_dev(olf_ctx* c, const float* d_depth, size_t n, uint8_t* d_mask, void* stream)
{
    if (!c || !d_depth || !d_mask) { set_error("olf_stereo_points_mask_dev: null argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_stereo_points_mask_dev"));
    return olf::launch_depth_mask(d_depth, d_mask, n, ctx_stream(c, stream));
}

int olf_frames_pack_dev(olf_ctx* c, const olf_frame_buffers* fb, int n_pairs, uint8_t* d_dst, size_t dst_capacity, uint64_t* d_bytes, void* stream)
{
    if (!c || !fb || !d_dst || !d_bytes || n_pairs < 0 || 2 * n_pairs > c->max_images || dst_capacity < 64 + (size_t)16 * n_pairs + 16) {
        set_error("olf_frames_pack_dev: bad argument"); return OLF_ERR_INVALID;
    }
    OLF_TRY(check_device(c, "olf_frames_pack_dev"));
    OLF_TRY(join_if_pending(c, ctx_stream(c, stream)));      // (the packer reads every output of the frame call, the line path's too)
    void* ofs = nullptr;
    OLF_TRY(scratch_get(c, SCRATCH_PACK, (size_t)8 * n_pairs * sizeof(int) + 64, &ofs));
    return olf::launch_pack_records(*fb, n_pairs, c->orb.geom.outCap, c->line.geom.outCap, d_dst, dst_capacity, static_cast<int*>(ofs),
                                    reinterpret_cast<unsigned long long*>(d_bytes), c->ob.status, ctx_stream(c, stream));
}

// ---------------------------------------------------------------------------------------------
int olf_stereo_points_dev(olf_ctx* c, int n_pairs, const olf_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                          float* d_uright, float* d_depth, void* stream)
{
    if (!c || !d_kps || !d_desc || !d_counts || !d_uright || !d_depth) { set_error("olf_stereo_points_dev: null argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_stereo_points_dev"));
    if (n_pairs < 0 || 2 * n_pairs > c->max_images) return OLF_ERR_CAPACITY;
    if (n_pairs == 0) return OLF_OK;
    OLF_TRY(check_landscape(c, "olf_stereo_points_dev"));      // (it reads the pyramids of the ORB extraction before it)
    return stage_stereo_points(c, n_pairs, d_kps, d_desc, d_counts, d_uright, d_depth, ctx_stream(c, stream));
}

int olf_match_bf_dev(olf_ctx* c, const uint8_t* dA, const int32_t* nA, int strideA, int a_step, const uint8_t* dB, const int32_t* nB,
                     int strideB, int b_step, int n_sets, float nnr, int best_lr, int32_t* d_m12, void* stream)
{
    if (!c || !dA || !dB || !nA || !nB || !d_m12 || strideA < 0 || strideB < 0 || n_sets < 0) { set_error("olf_match_bf_dev: bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_match_bf_dev"));
    if (n_sets == 0 || strideA == 0) return OLF_OK;
    hipStream_t s = ctx_stream(c, stream);
    // line descriptors / counts of a frame call whose line path is still running (deferred join): wait for it; ORB descriptors go ahead
    if (in_pending_line_outputs(c, dA) || in_pending_line_outputs(c, dB) || in_pending_line_outputs(c, nA) || in_pending_line_outputs(c, nB)) OLF_TRY(join_if_pending(c, s));
    int* ws = nullptr;
    Carve k;
    k.add(&ws, (size_t)3 * (strideA + strideB) * n_sets);
    OLF_TRY(k.bind(c, SCRATCH_KNN));
    StageScope t(c, s, ST_MATCH_BF);
    return launch_match_bf(dA, nA, strideA, a_step, dB, nB, strideB, b_step, n_sets, nnr, best_lr, ws, d_m12, s);
}

int olf_match_candidates_dev(olf_ctx* c, const uint8_t* dQ, int nQ, const uint8_t* dT, int nT, const int32_t* d_offs, const int32_t* d_cand,
                             uint16_t* d_dist, void* stream)
{
    if (!c || nQ < 0 || nT < 0 || (nQ && (!dQ || !d_offs || !d_dist))) { set_error("olf_match_candidates_dev: bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_match_candidates_dev"));
    hipStream_t s = ctx_stream(c, stream);
    StageScope t(c, s, ST_MATCH_BF);
    return launch_match_candidates(dQ, nQ, dT, nT, d_offs, d_cand, d_dist, s);
}

int olf_frame_grid_dev(olf_ctx* c, int n_frames, int img_stride, const olf_keypoint* d_kps, const int32_t* d_counts, float minX, float maxX, float minY,
                       float maxY, int32_t* d_cell_offsets, int32_t* d_cell_index, void* stream)
{
    float wInv, hInv;
    if (!c || n_frames < 0 || img_stride < 1 || !d_kps || !d_counts || !d_cell_offsets || !d_cell_index || !grid_scales(minX, maxX, minY, maxY, &wInv, &hInv)) {
        set_error("olf_frame_grid_dev: bad argument"); return OLF_ERR_INVALID;
    }
    OLF_TRY(check_device(c, "olf_frame_grid_dev"));
    const int cap = c->orb.geom.outCap;
    if (cap > OLF_GRID_MAX_KEYS) { set_error("olf_frame_grid_dev: more than OLF_GRID_MAX_KEYS key points per frame (their cells sit in LDS)"); return OLF_ERR_CAPACITY; }
    return launch_assign_grid(d_kps, (size_t)img_stride * cap, d_counts, img_stride, 0, cap, minX, minY, wInv, hInv, n_frames, d_cell_offsets, d_cell_index,
                              (size_t)cap, ctx_stream(c, stream));
}

int olf_features_in_area_dev(olf_ctx* c, const olf_keypoint* d_keys, const int32_t* d_cell_offsets, const int32_t* d_cell_index, float minX, float maxX,
                             float minY, float maxY, int n_queries, const olf_area_query* d_queries, int32_t* d_cand_offsets, int32_t* d_cand_idx,
                             int cand_capacity, void* stream)
{
    float wInv, hInv;
    if (!c || n_queries < 0 || cand_capacity < 0 || !d_cell_offsets || !d_cand_offsets || (n_queries && !d_queries) || (cand_capacity && !d_cand_idx) ||
        !grid_scales(minX, maxX, minY, maxY, &wInv, &hInv)) {
        set_error("olf_features_in_area_dev: bad argument"); return OLF_ERR_INVALID;
    }
    OLF_TRY(check_device(c, "olf_features_in_area_dev"));
    return launch_features_in_area(d_keys, d_cell_offsets, d_cell_index, minX, minY, wInv, hInv, n_queries, d_queries, d_cand_offsets, d_cand_idx,
                                   cand_capacity, c->ob.status, ctx_stream(c, stream));
}

int olf_ctx_device_buffers(const olf_ctx* c, olf_frame_buffers* out)
{
    if (!c || !out) { set_error("olf_ctx_device_buffers: null argument"); return OLF_ERR_INVALID; }
    *out = c->d_out;
    return OLF_OK;
}

int olf_cvt_gray_dev(olf_ctx* c, const uint8_t* d_src, int code, int n_images, uint8_t* d_gray, void* stream)
{
    if (!c || !d_src || !d_gray || code < 0 || code > 3 || n_images < 0) { set_error("olf_cvt_gray_dev: bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_cvt_gray_dev"));
    if (n_images == 0) return OLF_OK;
    return launch_cvt_gray(d_src, d_gray, c->W, c->H, code, n_images, ctx_stream(c, stream));
}

int olf_init_undistort_rectify_map_dev(olf_ctx* c, const double* K, const double* D, int n_dist, const double* R, const double* P, int w, int h,
                                       float* d_map1, float* d_map2, void* stream)
{
    if (!c || !K || !R || !P || !d_map1 || !d_map2 || w < 1 || h < 1 || n_dist < 0 || n_dist > 8 || (n_dist && !D)) {
        set_error("olf_init_undistort_rectify_map_dev: bad argument (up to 8 distortion coefficients k1 k2 p1 p2 k3 k4 k5 k6)"); return OLF_ERR_INVALID;
    }
    OLF_TRY(check_device(c, "olf_init_undistort_rectify_map_dev"));
    // iR = (P * R)^-1 in double: cv::invert's closed form for 3 x 3 (convention C.13)
    double m[9];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) m[3 * r + q] = P[3 * r] * R[q] + P[3 * r + 1] * R[3 + q] + P[3 * r + 2] * R[6 + q];
    double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (d == 0.) { set_error("olf_init_undistort_rectify_map_dev: P * R is singular"); return OLF_ERR_INVALID; }
    d = 1. / d;
    double ir[9];
    ir[0] = (m[4] * m[8] - m[5] * m[7]) * d; ir[1] = (m[2] * m[7] - m[1] * m[8]) * d; ir[2] = (m[1] * m[5] - m[2] * m[4]) * d;
    ir[3] = (m[5] * m[6] - m[3] * m[8]) * d; ir[4] = (m[0] * m[8] - m[2] * m[6]) * d; ir[5] = (m[2] * m[3] - m[0] * m[5]) * d;
    ir[6] = (m[3] * m[7] - m[4] * m[6]) * d; ir[7] = (m[1] * m[6] - m[0] * m[7]) * d; ir[8] = (m[0] * m[4] - m[1] * m[3]) * d;
    double k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n_dist; ++i) k[i] = D[i];
    return launch_init_rectify_map(ir, k, K[0], K[4], K[2], K[5], w, h, d_map1, d_map2, ctx_stream(c, stream));
}

int olf_remap_linear_dev(olf_ctx* c, const uint8_t* d_src, int sw, int sh, const float* d_mapx, const float* d_mapy, int dw, int dh, int n_images,
                         uint8_t* d_dst, void* stream)
{
    if (!c || !d_src || !d_mapx || !d_mapy || !d_dst || sw < 1 || sh < 1 || dw < 1 || dh < 1 || n_images < 0) { set_error("olf_remap_linear_dev: bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_remap_linear_dev"));
    if (n_images == 0) return OLF_OK;
    return launch_remap_linear(d_src, sw, sh, d_mapx, d_mapy, dw, dh, d_dst, n_images, ctx_stream(c, stream));
}

// ---------------------------------------------------------------------------------------------
int olf_line_capacity(const olf_ctx* c) { return c ? c->line.geom.outCap : OLF_ERR_INVALID; }

int olf_line_extract_dev(olf_ctx* c, const uint8_t* d_images, int n_images, olf_keyline* d_kls, uint8_t* d_ldesc, int32_t* d_lcounts, void* stream)
{
    if (!c || !d_images || !d_kls || !d_ldesc || !d_lcounts) { set_error("olf_line_extract_dev: null argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_line_extract_dev"));
    if (n_images < 0 || n_images > c->max_images) return OLF_ERR_CAPACITY;
    if (n_images == 0) return OLF_OK;
    OLF_TRY(check_landscape(c, "olf_line_extract_dev"));
    hipStream_t s = ctx_stream(c, stream);
    const LsdPlan plan = lsd_plan(c->line.geom, c->lb, c->lsd_force, c->limits, n_images);
    OLF_TRY(stage_lsd_front(c, plan, d_images, n_images, s, true));
    OLF_TRY(stage_lsd_grow(c, plan, n_images, s));
    OLF_TRY(stage_lsd_rect(c, plan, n_images, s));
    return stage_line_lbd(c, d_images, n_images, d_kls, d_ldesc, d_lcounts, s);
}

int olf_stereo_lines_dev(olf_ctx* c, int n_pairs, const olf_keyline* d_kls, const uint8_t* d_ldesc, const int32_t* d_lcounts, int32_t* d_m12,
                         float* d_disp, double* d_le, void* stream)
{
    if (!c || !d_kls || !d_ldesc || !d_lcounts || !d_m12 || !d_disp || !d_le) { set_error("olf_stereo_lines_dev: null argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_stereo_lines_dev"));
    if (n_pairs < 0 || 2 * n_pairs > c->max_images) { set_error("olf_stereo_lines_dev: n_pairs exceeds the context's max_images"); return OLF_ERR_CAPACITY; }
    if (n_pairs == 0) return OLF_OK;
    hipStream_t s = ctx_stream(c, stream);
    // key lines / descriptors of a frame call whose line path is still running (deferred join): this stream waits for it first
    if (s != c->stream2 && (in_pending_line_outputs(c, d_kls) || in_pending_line_outputs(c, d_ldesc) || in_pending_line_outputs(c, d_lcounts))) OLF_TRY(join_if_pending(c, s));
    return stage_stereo_lines(c, n_pairs, d_kls, d_ldesc, d_lcounts, d_m12, d_disp, d_le, s);
}

int olf_stereo_frames_dev(olf_ctx* c, const uint8_t* d_images, int n_pairs, const olf_frame_buffers* o, void* stream)
{
    bool args = c && d_images && o;
    for (int k = 0; args && k < FB_FIELDS; ++k) args = fb_field(*o, k) != nullptr;
    if (!args) { set_error("olf_stereo_frames_dev: null argument"); return OLF_ERR_INVALID; }
    OLF_TRY(check_device(c, "olf_stereo_frames_dev"));
    if (n_pairs < 0 || 2 * n_pairs > c->max_images) return OLF_ERR_CAPACITY;
    if (n_pairs == 0) return OLF_OK;
    OLF_TRY(check_landscape(c, "olf_stereo_frames_dev"));
    hipStream_t s = ctx_stream(c, stream), ls = c->stream2;
    const int n_images = 2 * n_pairs;
    const LineGeom& lg = c->line.geom;
    const LsdPlan plan = lsd_plan(lg, c->lb, c->lsd_force, c->limits, n_images);
    if (c->join_pending) { OLF_HIP_CHECK(hipStreamWaitEvent(s, c->ev_join, 0)); c->join_pending = false; }      // (a deferred join the caller never asked for)
    // OLF_ONE_STREAM serialises the two paths: every stage on the caller's stream, the line path first
    static const bool one_stream = getenv("OLF_ONE_STREAM") != nullptr;
    if (one_stream) {
        OLF_TRY(stage_lsd_front(c, plan, d_images, n_images, s, true));
        OLF_TRY(stage_lsd_grow(c, plan, n_images, s));
        OLF_TRY(stage_lsd_rect(c, plan, n_images, s));
        OLF_TRY(stage_line_lbd(c, d_images, n_images, o->kls, o->ldesc, o->lcounts, s));
        OLF_TRY(stage_stereo_lines(c, n_pairs, o->kls, o->ldesc, o->lcounts, o->lmatches12, o->ldisp, o->lle, s));
        OLF_TRY(stage_orb_pyramid(c, d_images, n_images, s));
        OLF_TRY(stage_orb_fast(c, n_images, s));
        OLF_TRY(stage_orb_octree(c, n_images, s));
        OLF_TRY(stage_orb_blur(c, n_images, s));
        OLF_TRY(stage_orb_describe(c, n_images, o->kps, o->desc, o->counts, s));
        return stage_stereo_points(c, n_pairs, o->kps, o->desc, o->counts, o->uright, o->depth, s);
    }
    // The schedule.  What follows is every stage of both streams and every record / wait of the five events, in the order the host enqueues them (which
    // matters: a wait enqueued before its event's record is a no-op):
    //
    //      caller's stream `s`: the ORB path                    line stream `ls`: the line path
    //      ---------------------------------                    -------------------------------
    //      ev_fork (or the caller's input event) ------------>
    //      pyramid                                              LSD front, dense half
    //                      <------------------------ ev_sort
    //      blur                                                 LSD front, seed order
    //      LBD gradient images
    //      ev_lbd ---------------------------------+
    //                      <---------------------- | ev_front
    //      FAST                                    |            growth
    //      octree                                  |            rectangles
    //      describe                                +--------->
    //      stereo points                                        selection, LBD descriptors
    //                                                           line stereo
    //                      <------------------------ ev_join
    //
    // The line path runs beside the ORB path on the second stream (the reference's 4 extraction threads, src/Frame.cc:164-171).  The ORB
    // stream builds its pyramid beside the dense half of the LSD front, runs its blur and the LBD gradient images (6 ms of dense work) in the shadow of
    // the seed ordering, and waits for the front's end before FAST: two dense pipelines at once only slow each other down (290 ms per 3072-pair step
    // with no wait at all), whereas FAST beside the latency-bound growth agents is hidden almost completely (105 ms beside them, 24 alone, and the
    // agents keep their stand-alone speed).  (The other schedules measured: profiles/HISTORY_design_rounds1-4.md, profiles/r4o_*.)
    //
    // Fork.  With the caller's input event (olf_ctx_set_input_event) the line stream does not wait for what is still queued on `s` -- the ORB / stereo /
    // matching tail of the previous batch -- and the LSD front of this batch runs beside it.  Safe: the LSD front, growth and rectangles write line-path
    // scratch that nothing on `s` reads, and selection / LBD / line stereo (which write the output buffers the previous batch's matchers and packer on `s`
    // may still read) sit behind ev_lbd, recorded on `s` behind all of the previous batch's work there.
    // (the event is consumed by the call: one-shot -- a stale handle must never order a later call)
    hipEvent_t in_ev = c->input_event;
    c->input_event = nullptr;
    if (in_ev) OLF_HIP_CHECK(hipStreamWaitEvent(ls, in_ev, 0));
    else {
        OLF_HIP_CHECK(hipEventRecord(c->ev_fork, s));
        OLF_HIP_CHECK(hipStreamWaitEvent(ls, c->ev_fork, 0));
    }
    // line stream, up to the rectangles.  ev_sort is recorded in front of the seed ordering (the dense, bandwidth-bound half of the front is through) and
    // ev_front behind it.  One quirk, kept: without the std::sort seed order ev_sort is recorded in front of the WHOLE front, not behind its dense half
    if (lg.seedOrder != 1) OLF_HIP_CHECK(hipEventRecord(c->ev_sort, ls));      // (no sort kernel to hide behind: the event is already true)
    {
        StageScope t(c, ls, ST_LSD_FRONT);
        OLF_TRY(launch_lsd_dense(lg, c->lb, plan, d_images, c->W, n_images, ls, false));      // (nothing behind reads the working image)
        if (lg.seedOrder == 1) OLF_HIP_CHECK(hipEventRecord(c->ev_sort, ls));
        OLF_TRY(launch_lsd_seed_order(lg, c->lb, plan, n_images, ls));
    }
    OLF_HIP_CHECK(hipEventRecord(c->ev_front, ls));
    OLF_TRY(stage_lsd_grow(c, plan, n_images, ls));
    OLF_TRY(stage_lsd_rect(c, plan, n_images, ls));
    // ORB stream.  The blur only needs the pyramid, so it runs ahead of FAST in the shadow of the seed sort -- behind the dense half of
    // the LSD front (ev_sort) -- and so do the LBD gradient images (GaussianBlur + Sobel of the LBD octave need the input images only; ev_lbd tells the line
    // stream they are done); FAST waits for the whole front (ev_front)
    OLF_TRY(stage_orb_pyramid(c, d_images, n_images, s));
    OLF_HIP_CHECK(hipStreamWaitEvent(s, c->ev_sort, 0));
    OLF_TRY(stage_orb_blur(c, n_images, s));
    OLF_TRY(launch_lbd_dense(lg, c->lb, d_images, c->W, n_images, s));
    OLF_HIP_CHECK(hipEventRecord(c->ev_lbd, s));
    OLF_HIP_CHECK(hipStreamWaitEvent(s, c->ev_front, 0));
    OLF_TRY(stage_orb_fast(c, n_images, s));
    OLF_TRY(stage_orb_octree(c, n_images, s));
    OLF_TRY(stage_orb_describe(c, n_images, o->kps, o->desc, o->counts, s));
    // the line stream's selection + LBD wait for ev_lbd, so they are enqueued behind the ORB extraction (an event has to be recorded before the wait for it
    // is enqueued)
    OLF_HIP_CHECK(hipStreamWaitEvent(ls, c->ev_lbd, 0));
    {
        StageScope t(c, ls, ST_LINE_LBD);
        OLF_TRY(launch_line_select(lg, c->lb, n_images, o->kls, o->lcounts, ls));
        OLF_TRY(launch_lbd_desc(lg, c->lb, n_images, o->kls, o->ldesc, o->lcounts, true, ls));
    }
    OLF_TRY(stage_stereo_lines(c, n_pairs, o->kls, o->ldesc, o->lcounts, o->lmatches12, o->ldisp, o->lle, ls));
    OLF_HIP_CHECK(hipEventRecord(c->ev_join, ls));
    OLF_TRY(stage_stereo_points(c, n_pairs, o->kps, o->desc, o->counts, o->uright, o->depth, s));
    // the join.  Deferred (olf_ctx_set_deferred_join): the caller's stream goes on with the ORB outputs -- key points, descriptors, stereo points are complete on
    // it here -- while the line path's tail (selection, LBD, line stereo: 20 ms of a 3072-pair batch) still runs on the line stream; olf_stereo_frames_join_dev
    // (or the next call) makes the stream wait for it
    if (c->deferred_join) {
        c->join_pending = true;
        c->pend_stream = s;
        for (int k = FB_KLS; k < FB_FIELDS; ++k) c->pend[k - FB_KLS] = {static_cast<const uint8_t*>(fb_field(*o, k)), fb_bytes(c, k, n_images)};
    } else OLF_HIP_CHECK(hipStreamWaitEvent(s, c->ev_join, 0));
    return OLF_OK;
}

int olf_ctx_set_deferred_join(olf_ctx* c, int on)
{
    if (!c) return OLF_ERR_INVALID;
    c->deferred_join = on != 0;
    return OLF_OK;
}

int olf_stereo_frames_join_dev(olf_ctx* c, void* stream)
{
    if (!c) return OLF_ERR_INVALID;
    return join_if_pending(c, ctx_stream(c, stream));
}

}  // extern "C"
