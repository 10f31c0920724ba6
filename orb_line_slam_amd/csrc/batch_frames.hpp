// batch_frames.hpp -- what the batched point matchers (track_batch.hip, local_batch.hip, fuse_batch.hip, sim3_batch.hip, projection_batch.hip and the kernel
// of triangulation_batch.hip) share beside the grid walk: the view of one frame of an olf_track_batch, with what every entry derives from the context
// (FrameView, filled and validated by batch_frames); the ordered walks' traversal of their kept lists (walk_lists, first_open) and their rotation-histogram
// rejection (histo_reject); and the per-frame pose block of the gates that project map points (pose_store).
#pragma once
#include <string>
#include "grid_walk.hpp"
#include "search_math.hpp"
#include "../../include/orbline.h"

namespace olf {

#ifdef __HIPCC__
// key points of frame f, inside [0, cap] whatever the count holds
__device__ __forceinline__ int frame_count(int f, const int* __restrict__ counts, int img_stride, int cap) { return min(max(counts[(size_t)f * img_stride], 0), cap); }
#endif

// The frames of an olf_track_batch (include/orbline.h) as the kernels index them, and what an entry derives from its context.  A matcher's argument block
// starts with it.
struct FrameView {
    olf_track_batch in;
    int cap, capW, nlevels;        // key points per frame (olf_orb_capacity); 32-bit words of one bit per key point; the context's levels
    float wInv, hInv;              // mfGridElementWidthInv / HeightInv (grid_scales)
    float sf[OLF_MAX_LEVELS];      // mvScaleFactors
    float thr[OLF_MAX_LEVELS];     // olf_predict_scale_thresholds (zero until the entry asks for them)

#ifdef __HIPCC__
    __device__ __forceinline__ size_t row(int f) const { return (size_t)f * in.img_stride * cap; }      // frame f in the per-image arrays
    __device__ __forceinline__ int count(int f) const { return frame_count(f, in.counts, in.img_stride, cap); }      // (in.counts is not NULL)
    __device__ __forceinline__ const olf_keypoint* keys(int f) const { return in.kps + row(f); }
    __device__ __forceinline__ const uint4* desc(int f) const { return reinterpret_cast<const uint4*>(in.desc) + 2 * row(f); }
    __device__ __forceinline__ const float* uright(int f) const { return in.uright + (size_t)f * cap; }
    // pMP->GetDescriptor() of the map point feature i of frame f holds: in.mp_desc, or the feature's own descriptor where the batch carries none
    __device__ __forceinline__ const uint4* point_desc(int f, int i) const
    {
        return in.mp_desc ? reinterpret_cast<const uint4*>(in.mp_desc) + 2 * ((size_t)f * cap + i) : desc(f) + 2 * (size_t)i;
    }
    // frame f's grid as grid_walk reads it.  Where a kernel does much before its walk, call it at the walk, so that the four floats hold scalar registers
    // only there (held from the start of k_track_lists they cost it four more, and 0.5 ms per call on an MI355X: DESIGN 4.5).  Where a wave does little else
    // (k_sim3_search), call it beside the entry's other loads: the count is a scalar load, and at the walk it is a wait of its own (5.90 against 5.81 ms).
    __device__ __forceinline__ GridView grid(int f) const
    {
        return {keys(f), in.cell_offsets + (size_t)f * (OLF_GRID_CELLS + 1), in.cell_index + (size_t)f * cap, count(f), cap, in.minX, in.minY, wInv, hInv};
    }
    // the same for a caller that holds n = count(f) already
    __device__ __forceinline__ GridView grid(int f, int n) const
    {
        return {keys(f), in.cell_offsets + (size_t)f * (OLF_GRID_CELLS + 1), in.cell_index + (size_t)f * cap, n, cap, in.minX, in.minY, wInv, hInv};
    }
#endif
};

// ---- the ordered walks (k_track_walk, k_local_walk; k_proj_walk keeps the traversal in its own text, it is slower through walk_lists) --------------------
// The kept lists [qb, qe) by one wave, 64 per chunk: body(q, l, x, e) for every non-empty list in index order, all of it wave-uniform -- list q = chunk + lane
// l, x its first word with the two flags, e its four entries.  A lane that needs more about its list than the list itself loads that beside it in
// chunk(q, q < qe), and the body fetches it from lane l.  The LDS state the body reads and writes is the caller's.
template <class Ch, class B>
__device__ __forceinline__ void walk_lists(const uint4* __restrict__ lists, int qb, int qe, int lane, Ch&& chunk, B&& body)
{
    for (int c0 = qb; c0 < qe; c0 += 64) {
        const int q = c0 + lane;
        uint4 L = make_uint4(Best4::NONE, Best4::NONE, Best4::NONE, Best4::NONE);
        if (q < qe) L = lists[q];
        chunk(q, q < qe);
        unsigned long long todo = wave_vote((L.x & Best4::NONE) != Best4::NONE);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const unsigned x = (unsigned)__shfl((int)L.x, l, 64);
            const unsigned e[Best4::K] = {x & Best4::NONE, (unsigned)__shfl((int)L.y, l, 64), (unsigned)__shfl((int)L.z, l, 64), (unsigned)__shfl((int)L.w, l, 64)};
            body(c0 + l, l, x, e);
        }
    }
}

// the first kept entry whose key point (its low 13 bits) open(f) lets through, or Best4::NONE; exhausted: all Best4::K kept entries are closed, so only a
// list that held more can still yield one
template <class O>
__device__ __forceinline__ unsigned first_open(const unsigned (&e)[Best4::K], bool& exhausted, O&& open)
{
    unsigned hit = Best4::NONE;
    exhausted = true;
    for (int k = 0; k < Best4::K; ++k) {
        if (e[k] == Best4::NONE) { exhausted = false; break; }
        if (open(e[k] & 0x1fffu)) { hit = e[k]; exhausted = false; break; }
    }
    return hit;
}

// ComputeThreeMaxima and the rejection behind it (src/ORBmatcher.cc:1449-1465, :1736-1745), by one thread: the bins outside the three maxima as a mask, their
// events taken off n
__device__ __forceinline__ unsigned histo_reject(const int* hist, int& n)
{
    int ind1, ind2, ind3;
    three_maxima(hist, ind1, ind2, ind3);
    unsigned rej = 0;
    for (int i = 0; i < HISTO_LENGTH; i++) if (i != ind1 && i != ind2 && i != ind3) { rej |= 1u << i; n -= hist[i]; }
    return rej;
}

// ---- the pose of a key frame as fuse_point_gate reads it --------------------------------------------------------------------------------------------------
constexpr int POSE_FLOATS = 16;                     // floats per key frame in scratch: Rcw (9), tcw (3), Ow (3), one of padding
__device__ __forceinline__ void pose_store(float* __restrict__ o, const float* R, const float* t, const float* ow)
{
    for (int k = 0; k < 9; ++k) o[k] = R[k];
    for (int k = 0; k < 3; ++k) { o[9 + k] = t[k]; o[12 + k] = ow[k]; }
    o[15] = 0.f;
}

// ---- the host side of an entry -----------------------------------------------------------------------------------------------------------------------------
// the planes of an olf_track_batch an entry reads, beside the bounds every entry needs; and those of an olf_local_map beside world, normal, maxd, mind, bad
enum : unsigned { NEED_GRID = 1, NEED_URIGHT = 2, NEED_TCW = 4, NEED_WORLD = 8 };      // NEED_GRID: kps, desc, counts, img_stride, cell_offsets, cell_index
enum : unsigned { MAP_DESC = 1, MAP_OBS = 2 };

// What every entry does before its own work.  `ok` is the entry's check of its own arguments; with the planes `need` names, the map (where the entry takes
// one: map_need says which of its optional planes) and the bounds it decides OLF_ERR_INVALID.  Then the device, the capacity (a list entry holds 13 index
// bits), and the entry's number of work items against 2^31: the map's entries, or rows * cap where the entry has no map.  Fills V and *n_items.
inline int batch_frames(olf_ctx* c, const char* who, bool ok, const olf_track_batch* in, unsigned need, int n_frames, const olf_local_map* map, unsigned map_need,
                        long long rows, const char* items, FrameView& V, int* n_items)
{
    const std::string w(who);
    ok = ok && c && in && n_frames >= 0 && grid_scales(in->minX, in->maxX, in->minY, in->maxY, &V.wInv, &V.hInv);
    if (ok && (need & NEED_GRID)) ok = in->kps && in->desc && in->counts && in->img_stride >= 1 && in->cell_offsets && in->cell_index;
    if (ok && (need & NEED_URIGHT)) ok = in->uright != nullptr;
    if (ok && (need & NEED_TCW)) ok = in->Tcw != nullptr;
    if (ok && (need & NEED_WORLD)) ok = in->mp_world != nullptr;
    if (ok && map) {
        ok = map->n_mp >= 0 && !(map->list_offsets && (map->n_entries < 0 || (map->n_entries && !map->list_index)));
        if (ok && map->n_mp) ok = map->world && map->normal && map->maxd && map->mind && map->bad && (!(map_need & MAP_DESC) || map->desc) && (!(map_need & MAP_OBS) || map->obs);
    }
    if (!ok) { set_error(w + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    V.in = *in;
    V.cap = olf_orb_capacity(c);
    V.capW = (V.cap + 31) / 32;
    if (V.cap > OLF_GRID_MAX_KEYS) { set_error(w + ": more than OLF_GRID_MAX_KEYS key points per frame (a list entry holds 13 index bits)"); return OLF_ERR_CAPACITY; }
    const long long n = !map ? rows * V.cap : map->list_offsets ? (long long)map->n_entries : (long long)n_frames * map->n_mp;
    if (n > 0x7fffffffLL - 256) { set_error(w + ": more than 2^31 " + items); return OLF_ERR_CAPACITY; }
    if (n_items) *n_items = (int)n;
    V.nlevels = ctx_level_scales(c, V.sf);
    for (int l = 0; l < OLF_MAX_LEVELS; ++l) V.thr[l] = 0.f;      // (an entry that predicts levels fills them once it has work: ctx_level_thresholds)
    return OLF_OK;
}

}  // namespace olf
