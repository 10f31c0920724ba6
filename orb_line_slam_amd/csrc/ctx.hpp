// ctx.hpp -- the device context behind the C ABI and what the three api*.cpp translation units share of it.  Host translation units only: a .hip file
// sees a context through the ctx_* accessors of olf_internal.hpp.
//   api.cpp        context lifecycle, status, profiling, the stages, the _dev entries, the fused frame call
//   api_host.cpp   the host-pointer entries: stage, call the _dev entry or the launcher, bring the results back
//   api_debug.cpp  olf_debug_* and the other entries that read a context's intermediate buffers for the tests
#pragma once
#include "olf_internal.hpp"
#include "line_internal.hpp"
#include "../../include/orbline.h"
#include <cstddef>
#include <cstring>

// ---- the layout of olf_frame_buffers (include/orbline.h), in the order of its fields: whose rows an array has (every image's or every pair's), how many
// per image or pair (the ORB capacity, the line capacity, or one for the two count arrays) and the bytes of a row
enum { FB_KPS, FB_DESC, FB_COUNTS, FB_URIGHT, FB_DEPTH, FB_KLS, FB_LDESC, FB_LCOUNTS, FB_LMATCHES12, FB_LDISP, FB_LLE, FB_FIELDS };
enum FieldCap { CAP_ONE, CAP_ORB, CAP_LINE };
struct FrameField { const char* name; size_t offset; bool perPair; FieldCap cap; size_t rowBytes; };
#define FIELD(f, perPair, cap, rowBytes) {#f, offsetof(olf_frame_buffers, f), perPair, cap, rowBytes}
constexpr FrameField kFrameFields[] = {
    FIELD(kps, false, CAP_ORB, sizeof(olf_keypoint)),   FIELD(desc, false, CAP_ORB, OLF_DESC_BYTES),    FIELD(counts, false, CAP_ONE, sizeof(int32_t)),
    FIELD(uright, true, CAP_ORB, sizeof(float)),        FIELD(depth, true, CAP_ORB, sizeof(float)),
    FIELD(kls, false, CAP_LINE, sizeof(olf_keyline)),   FIELD(ldesc, false, CAP_LINE, OLF_DESC_BYTES),  FIELD(lcounts, false, CAP_ONE, sizeof(int32_t)),
    FIELD(lmatches12, true, CAP_LINE, sizeof(int32_t)), FIELD(ldisp, true, CAP_LINE, 2 * sizeof(float)), FIELD(lle, true, CAP_LINE, 3 * sizeof(double))};
#undef FIELD
// (the struct is eleven object pointers and nothing else: a field is read and written through its offset as a void*)
constexpr bool frame_fields_in_order()
{
    for (size_t k = 0; k < sizeof(kFrameFields) / sizeof(kFrameFields[0]); ++k) if (kFrameFields[k].offset != k * sizeof(void*)) return false;
    return true;
}
static_assert(sizeof(kFrameFields) / sizeof(kFrameFields[0]) == FB_FIELDS && sizeof(olf_frame_buffers) == FB_FIELDS * sizeof(void*) && frame_fields_in_order(),
              "kFrameFields has one entry per field of olf_frame_buffers, in the struct's order");

inline void* fb_field(const olf_frame_buffers& f, int k) { void* p; std::memcpy(&p, reinterpret_cast<const char*>(&f) + kFrameFields[k].offset, sizeof(p)); return p; }
inline void fb_set_field(olf_frame_buffers& f, int k, void* p) { std::memcpy(reinterpret_cast<char*>(&f) + kFrameFields[k].offset, &p, sizeof(p)); }

struct olf_ctx {
    olf_params params;
    int W = 0, H = 0, max_images = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    olf::OrbHostTables orb;
    olf::OrbDeviceBufs ob;
    // staging for the host-pointer entry points
    uint8_t* d_images = nullptr;
    olf_frame_buffers d_out = {};  // the eleven output arrays, sized for max_images (kFrameFields)
    int* d_sad = nullptr;          // [max_pairs][outCap]
    int* d_bestkey = nullptr;
    unsigned* d_rowperm = nullptr; // [max_images][outCap] key point lists ordered by row (stereo candidate search)
    // line side
    olf::LineHostTables line;
    olf::LineDeviceBufs lb;
    olf::LsdOverrides lsd_force;       // olf_debug_lsd_* / olf_debug_seed_sort_mode (tests)
    olf::DeviceLimits limits;          // of `device`
    void* d_lprep = nullptr;
    uint16_t* d_ldist = nullptr;
    int* d_lm21 = nullptr;
    hipStream_t stream2 = nullptr;
    bool has_tables = false;       // holds a reference on the device's shared LSD angle tables
    hipEvent_t ev_front = nullptr;     // fused entry: recorded behind the LSD front including the seed ordering (the ORB stream's FAST waits for it)
    hipEvent_t input_event = nullptr;  // olf_ctx_set_input_event: not owned; the fused entry's line stream waits for it instead of forking from the caller's stream
    hipEvent_t ev_lbd = nullptr;       // fused entry: the LBD gradient images are ready (computed on the ORB stream in the seed ordering's shadow)
    bool deferred_join = false;        // olf_ctx_set_deferred_join: olf_stereo_frames_dev returns with the line path still running on the line stream
    bool scaled_aliased = false;       // batch context: the LSD working images live in the key buffers (dead before those are written)
    bool join_pending = false;         // ... and this call's line path has not been joined yet (olf_stereo_frames_join_dev, or the next call)
    // small contexts (the drop-in's one-pair-per-call shape): the eleven arrays of d_out sit in ONE device slab, so that the host entry brings them
    // back with one copy into pinned memory instead of eleven (each a launch and a gap of its own: 0.44 ms of a 9 ms call, profiles/r5b_pair_timeline.txt)
    uint8_t* d_outslab = nullptr; uint8_t* h_outslab = nullptr; size_t outslab_bytes = 0; size_t outslab_off[11] = {0};
    // every line-side output that call is still writing (key lines, LBD descriptors, counts, line matches, disparities, line equations): an entry that is handed
    // one of them (matcher, line stereo, packer) joins first.  The obligation is discharged for the whole context only when the frame call's OWN stream has
    // waited (pend_stream); a join on another stream orders that stream and leaves the obligation standing
    struct { const uint8_t* p; size_t bytes; } pend[FB_FIELDS - FB_KLS] = {};
    hipStream_t pend_stream = nullptr;
    hipEvent_t ev_sort = nullptr;      // fused entry: recorded in front of the seed ordering (the dense, bandwidth-bound half of the LSD front is through)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // stage profiling (olf_profile_*): HIP events recorded on the stream each stage is launched on
    bool prof_on = false;
    struct ProfRec { int stage; hipEvent_t a, b; };
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[16] = {0};
    int prof_calls[16] = {0};
    // grow-on-demand scratch, one slab per ScratchSlot (olf_internal.hpp says who holds which)
    void* scratch[olf::SCRATCH_SLOTS] = {};
    size_t scratch_bytes[olf::SCRATCH_SLOTS] = {};
    std::vector<void*> allocs;
    // olf_predict_scale_thresholds of the context's own scale factors, built by the first call that needs it (level_thr_rc > 0: not built yet)
    float level_thr[OLF_MAX_LEVELS] = {0};
    int level_thr_rc = 1;
};

namespace olf {

// A context (and everything it owns) lives on the device that was current when it was created; calling into it with another device
// current would send its launches and allocations to the wrong GPU.
int check_device(const olf_ctx* c, const char* who);
int check_status(olf_ctx* c);
int scratch_get(olf_ctx* c, ScratchSlot slot, size_t bytes, void** out);
// a deferred join that the caller has not asked for yet, in front of an entry that reads what the line stream is still writing
int join_if_pending(olf_ctx* c, hipStream_t s);
bool in_pending_line_outputs(const olf_ctx* c, const void* p);

// bytes of field k for n_images images (the pairs they make: an odd last image counts as a pair)
inline size_t fb_bytes(const olf_ctx* c, int k, size_t n_images)
{
    const FrameField& f = kFrameFields[k];
    const size_t cap = f.cap == CAP_ORB ? c->orb.geom.outCap : f.cap == CAP_LINE ? c->line.geom.outCap : 1;
    return (f.perPair ? (n_images + 1) / 2 : n_images) * cap * f.rowBytes;
}

// the copies of the host-pointer entries: fields first..last of n_images images between the context's arrays and the caller's (`h`, host pointers)
inline int fb_copy(olf_ctx* c, const olf_frame_buffers& h, int first, int last, size_t n_images, hipMemcpyKind kind)
{
    const olf_frame_buffers &src = kind == hipMemcpyDeviceToHost ? c->d_out : h, &dst = kind == hipMemcpyDeviceToHost ? h : c->d_out;
    for (int k = first; k <= last; ++k) OLF_HIP_CHECK(hipMemcpyAsync(fb_field(dst, k), fb_field(src, k), fb_bytes(c, k, n_images), kind, c->stream));
    return OLF_OK;
}

enum { ST_ORB_PYRAMID, ST_ORB_FAST, ST_ORB_OCTREE, ST_ORB_BLUR, ST_ORB_DESCRIBE, ST_STEREO_POINTS, ST_LSD_FRONT, ST_LSD_GROW, ST_LSD_RECT, ST_LINE_LBD,
       ST_STEREO_LINES, ST_MATCH_BF, ST_COUNT };

hipEvent_t prof_event(olf_ctx* c);
struct StageScope {
    olf_ctx* c; hipStream_t s; int stage; hipEvent_t a = nullptr;
    StageScope(olf_ctx* c_, hipStream_t s_, int st) : c(c_), s(s_), stage(st) { if (c->prof_on) { a = prof_event(c); (void)hipEventRecord(a, s); } }
    ~StageScope() { if (a) { hipEvent_t b = prof_event(c); (void)hipEventRecord(b, s); c->prof_recs.push_back({stage, a, b}); } }
};

}  // namespace olf
