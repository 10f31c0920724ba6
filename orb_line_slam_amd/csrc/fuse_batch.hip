// fuse_batch.hip -- the search part of int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th) (src/ORBmatcher.cc:827-948;
// LocalMapping::SearchInNeighbors, src/LocalMapping.cc:489, :514) and of int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints,
// float th, vector<MapPoint*> &vpReplacePoint) (:977-1102; LoopClosing::SearchAndFuse, src/LoopClosing.cc:605) for a whole batch of key frames on the device.
// The arithmetic is fuse_core's (search_host.cpp): the Sim3 decomposition, the gates on a point and the gates on a key point are the text both sides run
// (search_math.hpp); no contraction (-ffp-contract=off), correctly rounded divisions and square root.
//
// Nothing in the search part depends on the order of the map points: there is no vbMatched, no ratio test and no rotation histogram, and the map is only
// changed after the search (:950-972, :1086-1099).  A point's outcome is, among the key points of its window that pass the level gate (and, in the plain
// form, the chi-square gate), the one with the smallest distance -- the FIRST in scan order on a tie (`dist < bestDist`, :937, :1079).  That is one
// minimum over (distance << 20 | scan position), so there is no ordered walk, no kept list and nothing to recompute:
//   k_fuse_pose    one thread per key frame: Rcw | tcw | Ow (15 floats), from mTcw and GetCameraCenter() or from Scw (sim3_decompose)
//   k_fuse_held    one thread per (frame, feature): the bitmap of map points a key frame holds (IsInKeyFrame, :851; spAlreadyFound, :992, :1007) -- the
//                  scatter local_batch.hip uses (held_mark, entry_lists.hpp)
//   k_fuse_gate    one thread per entry: bad / held, then fuse_point_gate and the level from the table of olf_predict_scale_thresholds; writes
//                  (u, v, ur, level or -1), 16 bytes, and the "nothing" pair of the entry
//   k_fuse_search  one wave per entry that passed: walks the window (grid_walk, grid_walk.hpp) with the level gate; every lane keeps its smallest key and
//                  that key's feature; the wave's minimum with its owner lane's feature (wave_min_fetch, grid_walk.hpp), lane 0 writes the pair and counts
//                  the entry for its frame when it lies within TH_LOW (an integer atomic: the count does not depend on scheduling)
#include "batch_frames.hpp"
#include "entry_lists.hpp"
#include "device_math.hpp"
#include "staging.hpp"

namespace olf {

constexpr int FB_TH_LOW = 50;                       // src/ORBmatcher.cc:40
constexpr int FB_NOKEY = 0x7fffffff;                // above every key: distance <= 256, so a key is below 257 << 20
constexpr int FB_POS_BITS = 20;                     // scan positions: at most OLF_GRID_COLS ranges of at most OLF_GRID_MAX_KEYS indices, malformed grids included
static_assert(OLF_GRID_COLS * OLF_GRID_MAX_KEYS <= (1 << FB_POS_BITS), "key layout");

struct FuseArgs : FrameView {
    olf_local_map map;
    EntryLists L;
    const int* frame_mp;
    const float* Scw;              // NULL: the plain form
    const float* Ow;
    int n_frames, n_entries, mpW;  // mpW: 32-bit words of the held bitmap per frame
    float th;
};

__global__ __launch_bounds__(256) void k_fuse_pose(FuseArgs A, float* __restrict__ pose)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= A.n_frames) return;
    float R[9], t[3], ow[3];
    if (A.Scw) sim3_decompose(A.Scw + 16 * (size_t)j, R, t, ow);
    else {
        const float* T = A.in.Tcw + 16 * (size_t)j;
        for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) R[3 * r + k] = T[4 * r + k]; t[r] = T[4 * r + 3]; }
        if (A.Ow) for (int k = 0; k < 3; ++k) ow[k] = A.Ow[3 * (size_t)j + k];
        else camera_centre(T, ow);
    }
    pose_store(pose + (size_t)POSE_FLOATS * j, R, t, ow);
}

__global__ __launch_bounds__(256) void k_fuse_held(FuseArgs A, unsigned* __restrict__ held, int* __restrict__ status)
{
    const int j = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < A.count(j)) held_mark(A.frame_mp[(size_t)j * A.cap + idx], A.map.n_mp, A.map.bad, held + (size_t)j * A.mpW, status, STATUS_POINT_INDEX);
}

__global__ __launch_bounds__(256) void k_fuse_gate(FuseArgs A, const float* __restrict__ pose, const unsigned* __restrict__ held, float4* __restrict__ gate,
                                                  int* __restrict__ best_idx, int* __restrict__ best_dist, int* __restrict__ status)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.n_entries) return;
    best_idx[e] = -1;
    best_dist[e] = A.Scw ? FB_NOKEY : 256;                            // bestDist as the two forms start it (:897, :1053)
    float4 g = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    int i = -1;
    const int j = A.L.frame_of(e, i);
    if (j >= 0) {
        if ((unsigned)i >= (unsigned)A.map.n_mp) atomicOr(status, STATUS_POINT_INDEX);
        // if(!pMP) continue; if(pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue (:848-852); if(pMP->isBad() || spAlreadyFound.count(pMP)) continue (:1007)
        else if (!A.map.bad[i] && !(held && ((held[(size_t)j * A.mpW + (i >> 5)] >> (i & 31)) & 1u))) {
            const olf_track_batch& in = A.in;
            const float cam[5] = {in.fx, in.fy, in.cx, in.cy, in.mbf}, bounds[4] = {in.minX, in.maxX, in.minY, in.maxY};
            const float* P = pose + (size_t)POSE_FLOATS * j;
            float uvr[3], dist3D;
            if (fuse_point_gate(P, P + 9, P + 12, A.map.world + 3 * (size_t)i, A.map.normal + 3 * (size_t)i, A.map.maxd[i], A.map.mind[i], cam, bounds, uvr, dist3D))
                g = make_float4(uvr[0], uvr[1], uvr[2], __int_as_float(fuse_level(A.map.maxd[i], dist3D, A.thr, A.nlevels)));
        }
    }
    gate[e] = g;
}

__global__ __launch_bounds__(256) void k_fuse_search(FuseArgs A, const float4* __restrict__ gate, int* __restrict__ best_idx, int* __restrict__ best_dist,
                                                    int* __restrict__ nfused, int* __restrict__ status)
{
    const int e = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;      // (the wave's entry: scalar from here on)
    if (e >= A.n_entries) return;
    const float4 g = gate[e];
    const int level = __builtin_amdgcn_readfirstlane(__float_as_int(g.w));
    if (level < 0) return;                                            // (the entry keeps the "nothing" pair)
    int i = -1;
    const int j = A.L.frame_of(e, i);                                 // (passed the gate: j is a frame and i a map point)
    const olf_keypoint* keys = A.keys(j);
    const uint4* kd = A.desc(j);
    const float* kur = A.uright(j);
    const uint4* md = reinterpret_cast<const uint4*>(A.map.desc) + 2 * (size_t)i;
    const uint4 a0 = md[0], a1 = md[1];
    const float uvr[3] = {g.x, g.y, g.z};
    const bool plain = A.Scw == nullptr;
    // mvScaleFactors of the two octaves the level gate lets through, wave-uniform
    const float sfHi = A.sf[level], sfLo = A.sf[max(level - 1, 0)];
    // Search in a radius (:896, :1052)
    const float radius = A.th * sfHi;
    int bestKey = FB_NOKEY, bestJ = -1;
    bool badOct = false;
    // GetFeaturesInArea(u, v, radius) and the level gate (:905-908) in one: the walk leaves out what the gate would, and keeps the order of the rest
    grid_walk(A.grid(j), uvr[0], uvr[1], radius, level - 1, level, lane, [&](bool take, int j2, int pos) {
        if (!take) return;
        if (plain) {
            const olf_keypoint& kp = keys[j2];
            // (level - 1 <= octave <= level < nlevels: only octave -1 under level 0 lies outside mvScaleFactors)
            if (kp.octave < 0) { badOct = true; return; }
            if (!fuse_chi2_ok(uvr, kp.x, kp.y, kur[j2], kp.octave == level ? sfHi : sfLo)) return;
        }
        const int dist = ham256(a0, a1, kd[2 * (size_t)j2], kd[2 * (size_t)j2 + 1]);
        if (plain && dist >= 256) return;                             // (bestDist starts at 256, :897: such a candidate never registers)
        const int key = (dist << FB_POS_BITS) | pos;
        if (key < bestKey) { bestKey = key; bestJ = j2; }
    });
    int m, idx = -1;
    wave_min_fetch(bestKey, bestJ, FB_NOKEY, m, idx);
    const bool anyBad = wave_vote(badOct) != 0;
    if (lane == 0) {
        if (anyBad) atomicOr(status, STATUS_OCTAVE);
        if (idx >= 0) {
            const int dist = m >> FB_POS_BITS;
            best_idx[e] = idx; best_dist[e] = dist;
            if (nfused && dist <= FB_TH_LOW) atomicAdd(&nfused[j], 1);
        }
    }
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_fuse_search_batch_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const olf_local_map* map, const int32_t* d_frame_mp, const float* d_Scw,
                              const float* d_Ow, float th, int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_nfused, void* stream)
{
    FuseArgs A;
    OLF_TRY(batch_frames(c, "olf_fuse_search_batch_dev", map && d_best_idx && d_best_dist, in, NEED_GRID | NEED_URIGHT | (d_Scw ? 0 : NEED_TCW), n_frames, map,
                         MAP_DESC, 0, "entries", A, &A.n_entries));
    if (n_frames == 0) return OLF_OK;
    const int cap = A.cap;
    A.map = *map;
    A.L = {map->list_offsets, map->list_index, map->n_mp, n_frames, A.n_entries};
    A.frame_mp = d_frame_mp; A.Scw = d_Scw; A.Ow = d_Ow;
    A.n_frames = n_frames;
    A.mpW = (map->n_mp + 31) / 32;
    A.th = th;
    OLF_TRY(ctx_level_thresholds(c, A.thr));
    hipStream_t s = ctx_stream(c, stream);
    if (d_nfused) OLF_HIP_CHECK(hipMemsetAsync(d_nfused, 0, (size_t)n_frames * 4, s));
    if (A.n_entries == 0) return OLF_OK;
    // scratch: 16 bytes per entry (u, v, ur, level); 64 bytes per frame (the pose) and, with d_frame_mp, one bit per (frame, map point)
    float4* gate; float* pose; unsigned* held;
    const size_t bh = d_frame_mp ? (size_t)n_frames * A.mpW : 0;
    Carve k;
    k.add(&gate, (size_t)A.n_entries); k.add(&pose, (size_t)POSE_FLOATS * n_frames); k.add(&held, bh);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    hipLaunchKernelGGL(k_fuse_pose, dim3((n_frames + 255) / 256), dim3(256), 0, s, A, pose);
    if (bh) OLF_HIP_CHECK(hipMemsetAsync(held, 0, bh * 4, s));
    if (d_frame_mp) hipLaunchKernelGGL(k_fuse_held, dim3((cap + 255) / 256, n_frames), dim3(256), 0, s, A, held, ctx_status(c));      // (an empty map: every held index lies outside it)
    hipLaunchKernelGGL(k_fuse_gate, dim3((A.n_entries + 255) / 256), dim3(256), 0, s, A, pose, bh ? held : nullptr, gate, d_best_idx, d_best_dist, ctx_status(c));
    hipLaunchKernelGGL(k_fuse_search, dim3((A.n_entries + 3) / 4), dim3(256), 0, s, A, gate, d_best_idx, d_best_dist, d_nfused, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
