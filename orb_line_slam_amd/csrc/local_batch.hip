// local_batch.hip -- the point half of Tracking::SearchLocalPointsAndLines (src/Tracking.cc:1877-1942) for a whole batch of frames on the device:
// Frame::isInFrustum (src/Frame.cc:388-444) for every (frame, local map point), then ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*>&, th)
// (src/ORBmatcher.cc:47-131).  The arithmetic is that of search_host.cpp (olf_is_in_frustum, olf_search_local_map): its own cv::Mat products of
// convention C.12 (search_math.hpp), no contraction (-ffp-contract=off), correctly rounded divisions and square root.
//
// Only one thing in the matcher's loop depends on the order of the map points: a feature is passed over while the point it holds has observations
// (:89-91), and a point that is assigned changes that (:125).  Everything else -- radius, grid walk, level gates, the mvuRight gate, the distance -- is a
// function of (frame, point) alone.  The reference's running best / second best (:104-116) ends as the first two elements of the candidates sorted stably
// by distance (a candidate at distance 256 never registers, :112), so a point's outcome is decided by the first two UNBLOCKED entries of that sorted list:
//   k_local_held     one thread per (frame, feature): the bitmap of map points a frame holds (the mnLastFrameSeen test, src/Tracking.cc:1921), and the
//                    features blocked from the start (they hold a point with observations; a blocked feature stays blocked)
//   k_local_frustum  one thread per (frame, entry): Frame::isInFrustum; the level from the table of olf_predict_scale_thresholds, no logarithm
//   k_local_lists    one wave per (frame, entry in view): walks the window (grid_walk, grid_walk.hpp) and keeps the LB_K best candidates (Best4) that are not
//                    blocked from the start, in (distance, scan position) order, each with "octave == predicted level", plus "there were more" (16 bytes
//                    per entry).  No cut at TH_HIGH: the second best decides the ratio test at any distance
//   k_local_walk     one workgroup per frame: one wave walks the entries in list order against the blocked bits in LDS; an entry whose kept candidates
//                    do not yield two unblocked ones although the window held more is recomputed on the spot by the wave, with the blocked test inside
//                    the scan -- there is no capacity and no approximate case
#include <algorithm>
#include "batch_frames.hpp"
#include "entry_lists.hpp"
#include "device_math.hpp"
#include "staging.hpp"

namespace olf {

constexpr int LB_TH_HIGH = 100;                     // src/ORBmatcher.cc:39
constexpr int LB_K = 4;                             // candidates kept per entry (one uint4)
// a kept candidate: distance << 18 | (octave == predicted level) << 13 | feature (< OLF_GRID_MAX_KEYS = 2^13); the first word of a list also carries two flags
constexpr unsigned LB_NONE = Best4::NONE, LB_OBS = 1u << 30, LB_MORE = 1u << 31;
constexpr int LB_NOKEY = Best4::NOKEY;
static_assert(OLF_GRID_MAX_KEYS <= (1 << 13) && LB_K == Best4::K, "candidate layout");

struct LocalArgs : FrameView {
    olf_local_map map;
    EntryLists L;
    const int* frame_mp;
    int n_frames, n_entries;
    int mpW, blkW;                 // per frame: 32-bit words of the held bitmap, 64-bit words of the blocked bitmap
    float cosLimit, th, nnratio;
    const float* d_th;
};

struct LbFrame {
    const olf_keypoint* k;
    const uint4* d;
    const float* ur;
    int n;
};

struct LbQuery {
    float u, v, xr, radius;
    int level;
};

__device__ __forceinline__ LbFrame lb_frame(const LocalArgs& A, int j) { return {A.keys(j), A.desc(j), A.uright(j), A.count(j)}; }

__global__ __launch_bounds__(256) void k_local_held(LocalArgs A, unsigned* __restrict__ held, unsigned long long* __restrict__ blk0, int* __restrict__ status)
{
    const int j = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    bool blocked = false;
    if (idx < (A.in.counts ? A.count(j) : A.cap)) {                  // (olf_is_in_frustum_batch_dev without counts: every frame holds cap key points)
        // (a bad point is dropped from its feature, src/Tracking.cc:1885-1888)
        const int v = held_mark(A.frame_mp[(size_t)j * A.cap + idx], A.map.n_mp, A.map.bad, held + (size_t)j * A.mpW, status, STATUS_POINT_INDEX);
        blocked = v >= 0 && blk0 && A.map.obs[v] != 0;
    }
    const unsigned long long m = wave_vote(blocked);
    if (blk0 && (threadIdx.x & 63) == 0 && (idx >> 6) < A.blkW) blk0[(size_t)j * A.blkW + (idx >> 6)] = m;
}

// Frame::isInFrustum as olf_is_in_frustum evaluates it (search_host.cpp)
__global__ __launch_bounds__(256) void k_local_frustum(LocalArgs A, const unsigned* __restrict__ held, uint8_t* __restrict__ in_view, int* __restrict__ level,
                                                      float* __restrict__ view_cos, float* __restrict__ proj3, int* __restrict__ status)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.n_entries) return;
    int i = -1;
    const int j = A.L.frame_of(e, i);
    in_view[e] = 0;
    if (j < 0) return;
    if ((unsigned)i >= (unsigned)A.map.n_mp) { atomicOr(status, STATUS_POINT_INDEX); return; }
    if (A.map.bad[i]) return;
    if (held && ((held[(size_t)j * A.mpW + (i >> 5)] >> (i & 31)) & 1u)) return;
    const olf_track_batch& in = A.in;
    const float* T = in.Tcw + 16 * (size_t)j;
    const float* P = A.map.world + 3 * (size_t)i;
    const float* N = A.map.normal + 3 * (size_t)i;
    float Ow[3], Pc[3];
    camera_centre(T, Ow);                                            // mOw = -mRcw.t() * mtcw
    rot_apply(T, P, 1.0f, Pc);
    const float PcX = Pc[0], PcY = Pc[1], PcZ = Pc[2];
    if (PcZ < 0.0f) return;
    const float invz = __fdiv_rn(1.0f, PcZ);
    const float u = in.fx * PcX * invz + in.cx, v = in.fy * PcY * invz + in.cy;
    if (u < in.minX || u > in.maxX) return;
    if (v < in.minY || v > in.maxY) return;
    const float maxd = A.map.maxd[i];
    const float maxDistance = 1.2f * maxd, minDistance = 0.8f * A.map.mind[i];
    double nrm = 0, dot = 0;
    for (int k = 0; k < 3; ++k) { const float po = P[k] - Ow[k]; nrm += (double)po * (double)po; dot += (double)po * (double)N[k]; }
    const float dist = (float)__dsqrt_rn(nrm);
    if (dist < minDistance || dist > maxDistance) return;
    const float viewCos = (float)__ddiv_rn(dot, (double)dist);
    if (viewCos < A.cosLimit) return;
    const float ratio = __fdiv_rn(maxd, dist);                     // MapPoint::PredictScale: the number of thresholds <= ratio
    int lv = 0;
    for (int k = 0; k + 1 < A.nlevels; ++k) lv += A.thr[k] <= ratio ? 1 : 0;
    level[e] = lv;
    in_view[e] = 1;
    proj3[3 * (size_t)e] = u; proj3[3 * (size_t)e + 1] = v; proj3[3 * (size_t)e + 2] = u - in.mbf * invz;
    view_cos[e] = viewCos;
}

// the window of an entry in view (src/ORBmatcher.cc:62-71); it is searched as GetFeaturesInArea(u, v, radius, level - 1, level)
__device__ __forceinline__ LbQuery lb_query(const LocalArgs& A, float th, int level, float viewCos, const float* p3)
{
    LbQuery q;
    float r = viewCos > 0.998 ? 2.5f : 4.0f;                          // RadiusByViewingCos, :133-139
    if (th != 1.0) r *= th;                                          // bFactor
    q.level = min(max(level, 0), A.nlevels - 1);
    q.radius = r * A.sf[q.level];
    q.u = p3[0]; q.v = p3[1]; q.xr = p3[2];
    return q;
}

// the tests on one candidate that do not depend on the blocked state (:93-102).  true: the candidate registers as best or second best (distance < 256);
// key orders such candidates as the reference's scan does, ent is the kept form
__device__ __forceinline__ bool lb_candidate(const LbFrame& P, const LbQuery& q, const uint4& a0, const uint4& a1, int j, int pos, int& key, unsigned& ent)
{
    const float uR = P.ur[j];
    if (uR > 0) {
        const float er = fabsf(q.xr - uR);
        if (er > q.radius) return false;
    }
    const int dist = ham256(a0, a1, P.d[2 * (size_t)j], P.d[2 * (size_t)j + 1]);
    if (dist >= 256) return false;
    key = (dist << 16) | pos;
    ent = ((unsigned)dist << 18) | (P.k[j].octave == q.level ? 1u << 13 : 0u) | (unsigned)j;
    return true;
}

__global__ __launch_bounds__(256) void k_local_lists(LocalArgs A, const uint8_t* __restrict__ in_view, const int* __restrict__ level,
                                                    const float* __restrict__ view_cos, const float* __restrict__ proj3,
                                                    const unsigned long long* __restrict__ blk0, uint4* __restrict__ lists)
{
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= A.n_entries) return;                                    // (wave-uniform, as every branch on e below)
    int i = -1;
    const int j = A.L.frame_of(e, i);
    unsigned out[LB_K] = {LB_NONE, LB_NONE, LB_NONE, LB_NONE};
    int cnt = 0;
    bool obs = false;
    float th;
    if (j >= 0 && in_view[e] && item_radius(A.th, A.d_th, j, th)) {               // (in view: i is inside the map; a skipped frame's entries get empty lists)
        const LbFrame P = lb_frame(A, j);
        const LbQuery q = lb_query(A, th, level[e], view_cos[e], proj3 + 3 * (size_t)e);
        const uint4* md = reinterpret_cast<const uint4*>(A.map.desc) + 2 * (size_t)i;
        const uint4 a0 = md[0], a1 = md[1];
        const unsigned long long* b0 = blk0 + (size_t)j * A.blkW;
        obs = A.map.obs[i] != 0;
        Best4 best;
        grid_walk(A.grid(j), q.u, q.v, q.radius, q.level - 1, q.level, lane, [&](bool take, int j2, int pos) {
            int key = LB_NOKEY;
            unsigned ent = LB_NONE;
            const bool ok = take && !((b0[j2 >> 6] >> (j2 & 63)) & 1ull) && lb_candidate(P, q, a0, a1, j2, pos, key, ent);
            cnt += __popcll(wave_vote(ok));
            best.push(ok, key, ent);
        });
        best.drain(out);
    }
    if (lane == 0) {
        unsigned x = out[0];
        if (cnt > LB_K) x |= LB_MORE;
        if (obs) x |= LB_OBS;
        lists[e] = make_uint4(x, out[1], out[2], out[3]);
    }
}

// the window of entry e again, with the blocked test inside the scan: the first two candidates of the sorted list that are not blocked now (LB_NONE: none)
__device__ __forceinline__ void lb_rescan(const LbFrame& P, const LocalArgs& A, int j, const LbQuery& q, int i, int lane, const unsigned* s_blk, unsigned& c1, unsigned& c2)
{
    const uint4* md = reinterpret_cast<const uint4*>(A.map.desc) + 2 * (size_t)i;
    const uint4 a0 = md[0], a1 = md[1];
    int k1 = LB_NOKEY, k2 = LB_NOKEY;
    c1 = c2 = LB_NONE;
    grid_walk(A.grid(j), q.u, q.v, q.radius, q.level - 1, q.level, lane, [&](bool take, int j2, int pos) {
        int key = LB_NOKEY;
        unsigned ent = LB_NONE;
        const bool ok = take && !((s_blk[j2 >> 5] >> (j2 & 31)) & 1u) && lb_candidate(P, q, a0, a1, j2, pos, key, ent);
        if (!ok) key = LB_NOKEY;
        for (int t = 0; t < 2; ++t) {                                // the chunk's two smallest keys, merged into the running two (keys are distinct)
            int m;
            unsigned em;
            if (!wave_min_fetch(key, ent, k2, m, em)) break;
            if (m < k1) { k2 = k1; c2 = c1; k1 = m; c1 = em; }
            else { k2 = m; c2 = em; }
            if (key == m) key = LB_NOKEY;
        }
    });
}

// One workgroup per frame; dynamic LDS: cap ints (the map index a feature received), then 2 * capW words (blocked bits).
__global__ __launch_bounds__(256) void k_local_walk(LocalArgs A, const uint4* __restrict__ lists, const int* __restrict__ level, const float* __restrict__ view_cos,
                                                   const float* __restrict__ proj3, const unsigned long long* __restrict__ blk0, int* __restrict__ matches,
                                                   int* __restrict__ nmatches)
{
    extern __shared__ int s_match[];
    __shared__ int s_n;
    unsigned* s_blk = reinterpret_cast<unsigned*>(s_match + A.cap);
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, cap = A.cap;
    float th;
    if (!item_radius(A.th, A.d_th, j, th)) return;
    const LbFrame P = lb_frame(A, j);
    const unsigned* b0 = reinterpret_cast<const unsigned*>(blk0 + (size_t)j * A.blkW);
    for (int i = tid; i < cap; i += 256) s_match[i] = -1;
    for (int w = tid; w < 2 * A.blkW; w += 256) s_blk[w] = b0[w];
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (tid < 64) {
        int n = 0, eb, ee, mi = -1;                                  // mi: this lane's list's map index
        A.L.range(j, eb, ee);
        walk_lists(lists, eb, ee, lane, [&](int e, bool in) { mi = !in ? -1 : A.L.offsets ? A.L.index[e] : e - eb; },
                   [&](int e1, int l, unsigned x, const unsigned (&k)[LB_K]) {
            const int i = __shfl(mi, l, 64);
            // the first two kept candidates that are not blocked now
            unsigned c1 = LB_NONE, c2 = LB_NONE;
            bool complete = false;                                   // the kept candidates decide the entry
            for (int t = 0; t < LB_K; ++t) {
                if (k[t] == LB_NONE) { complete = true; break; }
                const unsigned f = k[t] & 0x1fffu;
                if (f >= (unsigned)P.n || ((s_blk[f >> 5] >> (f & 31)) & 1u)) continue;
                if (c1 == LB_NONE) {
                    c1 = k[t];
                    if ((int)(c1 >> 18) > LB_TH_HIGH) { complete = true; break; }      // (bestDist > TH_HIGH: the second best is not looked at, :120)
                } else { c2 = k[t]; complete = true; break; }
            }
            if (!complete && !(x & LB_MORE)) complete = true;
            if (!complete && c1 == LB_NONE && (int)(k[LB_K - 1] >> 18) > LB_TH_HIGH) complete = true;      // (whatever follows is no nearer)
            if (!complete) lb_rescan(P, A, j, lb_query(A, th, level[e1], view_cos[e1], proj3 + 3 * (size_t)e1), i, lane, s_blk, c1, c2);
            if (c1 == LB_NONE) return;
            const int bestDist = (int)(c1 >> 18);
            if (bestDist > LB_TH_HIGH) return;
            // Apply ratio to second match (only if best and second are in the same scale level), :119-123 -- without a second: bestLevel2 = -1
            if (c2 != LB_NONE && ((c1 ^ c2) & (1u << 13)) == 0 && (float)bestDist > A.nnratio * (float)(int)(c2 >> 18)) return;
            const unsigned f = c1 & 0x1fffu;
            s_match[f] = i;                                           // (every lane stores the same values: the next entry's reads are ordered behind them)
            if (x & LB_OBS) s_blk[f >> 5] |= 1u << (f & 31);
            ++n;
        });
        if (lane == 0) s_n = n;
    }
    __syncthreads();
    for (int i = tid; i < cap; i += 256) matches[(size_t)j * cap + i] = s_match[i];
    if (tid == 0) nmatches[j] = s_n;
}

}  // namespace olf

using namespace olf;

namespace {

// the checks and the argument block the two entries share (batch_frames forms n_entries when the map carries no lists)
int local_args(olf_ctx* c, const char* who, const olf_track_batch* in, int n_frames, const olf_local_map* map, bool search, LocalArgs& A)
{
    OLF_TRY(batch_frames(c, who, map != nullptr, in, search ? NEED_GRID | NEED_URIGHT | NEED_TCW : NEED_TCW, n_frames, map, search ? MAP_DESC | MAP_OBS : 0, 0,
                         "entries", A, &A.n_entries));
    A.map = *map;
    A.L = {map->list_offsets, map->list_index, map->n_mp, n_frames, A.n_entries};
    A.frame_mp = nullptr;
    A.n_frames = n_frames;
    A.mpW = (map->n_mp + 31) / 32; A.blkW = (A.cap + 63) / 64;
    A.cosLimit = 0.f; A.th = 1.f; A.nnratio = 0.f; A.d_th = nullptr;
    return ctx_level_thresholds(c, A.thr);
}

// the held / blocked bitmaps, then the frustum pass
int launch_frustum(olf_ctx* c, const LocalArgs& A, unsigned* held, unsigned long long* blk0, uint8_t* in_view, int* level, float* view_cos, float* proj3, hipStream_t s)
{
    const size_t bh = (size_t)A.n_frames * A.mpW * 4;
    const bool scatter = A.frame_mp != nullptr;
    if (bh) OLF_HIP_CHECK(hipMemsetAsync(held, 0, bh, s));
    if (blk0 && !scatter) OLF_HIP_CHECK(hipMemsetAsync(blk0, 0, (size_t)A.n_frames * A.blkW * 8, s));
    if (scatter) hipLaunchKernelGGL(k_local_held, dim3((A.cap + 255) / 256, A.n_frames), dim3(256), 0, s, A, held, blk0, ctx_status(c));
    if (A.n_entries) hipLaunchKernelGGL(k_local_frustum, dim3((A.n_entries + 255) / 256), dim3(256), 0, s, A, scatter ? held : nullptr, in_view, level, view_cos, proj3, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // namespace

extern "C" {

int olf_is_in_frustum_batch_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const olf_local_map* map, const int32_t* d_frame_mp,
                                float viewing_cos_limit, uint8_t* d_in_view, int32_t* d_level, float* d_view_cos, float* d_proj3, void* stream)
{
    LocalArgs A;
    OLF_TRY(local_args(c, "olf_is_in_frustum_batch_dev", in, n_frames, map, false, A));
    if (d_frame_mp && in->counts && in->img_stride < 1) { set_error("olf_is_in_frustum_batch_dev: bad argument"); return OLF_ERR_INVALID; }
    if (n_frames == 0 || A.n_entries == 0) return OLF_OK;
    if (!d_in_view || !d_level || !d_view_cos || !d_proj3) { set_error("olf_is_in_frustum_batch_dev: bad argument"); return OLF_ERR_INVALID; }
    A.frame_mp = d_frame_mp; A.cosLimit = viewing_cos_limit;
    unsigned* held;
    Carve k;
    k.add(&held, (size_t)n_frames * A.mpW);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    return launch_frustum(c, A, held, nullptr, d_in_view, d_level, d_view_cos, d_proj3, ctx_stream(c, stream));
}

int olf_search_local_map_batch_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const olf_local_map* map, const int32_t* d_frame_mp,
                                   float viewing_cos_limit, float th, const float* d_th, float nnratio, int32_t* d_matches, int32_t* d_nmatches,
                                   void* stream)
{
    LocalArgs A;
    OLF_TRY(local_args(c, "olf_search_local_map_batch_dev", in, n_frames, map, true, A));
    if (!d_matches || !d_nmatches) { set_error("olf_search_local_map_batch_dev: bad argument"); return OLF_ERR_INVALID; }
    if (n_frames == 0) return OLF_OK;
    A.frame_mp = d_frame_mp; A.cosLimit = viewing_cos_limit; A.th = th; A.d_th = d_th; A.nnratio = nnratio;
    // scratch, 37 bytes per entry: the kept candidates (16), mTrackProjX / Y / XR (12), mnTrackScaleLevel (4), mTrackViewCos (4), mbTrackInView (1); then the bitmaps
    const size_t ne = (size_t)A.n_entries;
    uint4* lists; float *proj3, *view_cos; int* level; uint8_t* in_view; unsigned* held; unsigned long long* blk0;
    Carve k;
    k.add(&lists, ne); k.add(&proj3, 3 * ne); k.add(&level, ne); k.add(&view_cos, ne); k.add(&in_view, ne);
    k.add(&held, (size_t)n_frames * A.mpW); k.add(&blk0, (size_t)n_frames * A.blkW);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    hipStream_t s = ctx_stream(c, stream);
    OLF_TRY(launch_frustum(c, A, held, blk0, in_view, level, view_cos, proj3, s));
    if (A.n_entries) hipLaunchKernelGGL(k_local_lists, dim3((A.n_entries + 3) / 4), dim3(256), 0, s, A, in_view, level, view_cos, proj3, blk0, lists);
    const size_t lds = (size_t)A.cap * 4 + (size_t)A.blkW * 8;
    hipLaunchKernelGGL(k_local_walk, dim3(n_frames), dim3(256), lds, s, A, lists, level, view_cos, proj3, blk0, d_matches, d_nmatches);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
