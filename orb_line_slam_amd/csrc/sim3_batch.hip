// sim3_batch.hip -- int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12,
// const cv::Mat &t12, const float th) (src/ORBmatcher.cc:1104-1328; LoopClosing::ComputeSim3, src/LoopClosing.cc:329) for a list of key-frame pairs of a
// device-resident batch, each pair with its own similarity.  The arithmetic is olf_search_by_sim3's (search_host.cpp): the transforms between the cameras
// and the gates on a point are the text both sides run (search_math.hpp); no contraction (-ffp-contract=off), correctly rounded divisions and square root.
//
// Nothing in the search depends on the order of the points: vbAlreadyMatched1 / 2 are fixed before the loops (:1134-1144), a point's outcome is, among the
// key points of its window that pass the level gate, the one with the smallest distance -- the FIRST in scan order on a tie (`dist < bestDist`, :1216, :1296)
// -- and vpMatches12 is only written by the agreement pass (:1312-1325).  That is one minimum over (distance << 20 | scan position), the key of
// fuse_batch.hip, and the division of work is that file's, per (pair, direction, feature) instead of per (key frame, map point):
//   k_sim3_transform  one thread per pair: validates the pair and writes sR12 | sR21 | t12 | t21 | valid (32 floats; sim3_pair_transforms); nfound = 0, or
//                     -1 and status bit 2048 for a pair outside the batch
//   k_sim3_mark       one thread per (pair, feature of kf1): vbAlreadyMatched2 as one bit per (pair, feature of kf2), scattered with atomicOr from the
//                     pre-matches in [0, N2); both vnMatch rows of the pair to -1
//   k_sim3_gate       one thread per (pair, direction, source feature): holds a point / already matched / bad, then sim3_point_gate and the level from the
//                     table of olf_predict_scale_thresholds; writes (u, v, level or -1), 12 bytes
//   k_sim3_search     one wave per entry, four per workgroup; an entry that failed the gate leaves at once.  The entry index, hence pair, direction, both
//                     frames, the level and the radius, is wave-uniform (readfirstlane).  The wave walks the window in the other key frame's grid
//                     (grid_walk, grid_walk.hpp) with the level gate; every lane keeps its smallest key and that key's feature; the wave's minimum
//                     with its owner lane's feature (wave_min_fetch, grid_walk.hpp); lane 0 writes vnMatch when the distance lies within TH_HIGH
//   k_sim3_agree      one thread per (pair, feature of kf1): vnMatch2[vnMatch1[i1]] == i1 writes vpMatches12[i1]; the count goes wave by wave into the
//                     pair's zeroed counter with an integer atomic, so it does not depend on scheduling
#include "batch_frames.hpp"
#include "device_math.hpp"
#include "staging.hpp"

namespace olf {

constexpr int SB_TH_HIGH = 100;                     // src/ORBmatcher.cc:39
constexpr int SB_NOKEY = 0x7fffffff;                // above every key: distance <= 256, so a key is below 257 << 20
constexpr int SB_POS_BITS = 20;                     // scan positions: at most OLF_GRID_COLS ranges of at most OLF_GRID_MAX_KEYS indices, malformed grids included
constexpr int SB_XF = 32;                           // floats per pair in scratch: sR12 (9), sR21 (9), t12 (3), t21 (3), valid (1, an int), seven of padding
constexpr int SB_XF_VALID = 24;
static_assert(OLF_GRID_COLS * OLF_GRID_MAX_KEYS <= (1 << SB_POS_BITS), "key layout");

struct Sim3Gate { float u, v; int level; };         // level -1: nothing to search

struct Sim3Args : FrameView {      // (capW: the 32-bit words of vbAlreadyMatched2 per pair)
    const uint8_t* mp_bad;         // [n_frames][cap] or NULL
    const float *mp_maxd, *mp_mind;
    const int* pairs;
    const float *s12, *R12, *t12;
    int n_frames, n_pairs;
    float th;
};

__device__ __forceinline__ bool sb_valid(const float* __restrict__ xf, int p) { return __float_as_int(xf[(size_t)SB_XF * p + SB_XF_VALID]) != 0; }

__global__ __launch_bounds__(256) void k_sim3_transform(Sim3Args A, float* __restrict__ xf, int* __restrict__ nfound, int* __restrict__ status)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= A.n_pairs) return;
    float* o = xf + (size_t)SB_XF * p;
    for (int k = 0; k < SB_XF; ++k) o[k] = 0.f;
    const int f1 = A.pairs[2 * (size_t)p], f2 = A.pairs[2 * (size_t)p + 1];
    if (!pair_in_batch(f1, f2, A.n_frames)) {
        nfound[p] = -1;
        atomicOr(status, STATUS_PAIR);
        return;
    }
    float R[9], t[3], sR12[9], sR21[9], t21[3];
    for (int k = 0; k < 9; ++k) R[k] = A.R12[9 * (size_t)p + k];
    for (int k = 0; k < 3; ++k) t[k] = A.t12[3 * (size_t)p + k];
    sim3_pair_transforms(A.s12[p], R, t, sR12, sR21, t21);
    for (int k = 0; k < 9; ++k) { o[k] = sR12[k]; o[9 + k] = sR21[k]; }
    for (int k = 0; k < 3; ++k) { o[18 + k] = t[k]; o[21 + k] = t21[k]; }
    o[SB_XF_VALID] = __int_as_float(1);
    nfound[p] = 0;
}

__global__ __launch_bounds__(256) void k_sim3_mark(Sim3Args A, const float* __restrict__ xf, const int* __restrict__ matches12, unsigned* __restrict__ already2,
                                                  int* __restrict__ vn1, int* __restrict__ vn2)
{
    const int p = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
    if (i >= A.cap || !sb_valid(xf, p)) return;
    const size_t row = (size_t)p * A.cap;
    vn1[row + i] = -1; vn2[row + i] = -1;
    const int f1 = A.pairs[2 * (size_t)p], f2 = A.pairs[2 * (size_t)p + 1];
    if (i >= A.count(f1)) return;
    // vbAlreadyMatched2[idx2] = true for idx2 = pMP->GetIndexInKeyFrame(pKF2) in [0, N2) (:1137-1143)
    const int idx2 = matches12[row + i];
    if (idx2 >= 0 && idx2 < A.count(f2)) atomicOr(&already2[(size_t)p * A.capW + (idx2 >> 5)], 1u << (idx2 & 31));
}

__global__ __launch_bounds__(256) void k_sim3_gate(Sim3Args A, const float* __restrict__ xf, const int* __restrict__ matches12,
                                                  const unsigned* __restrict__ already2, Sim3Gate* __restrict__ gate)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int per = 2 * A.cap;
    if (e >= A.n_pairs * per) return;
    const int p = e / per, r = e - p * per, dir = r >= A.cap ? 1 : 0, i = r - dir * A.cap;
    Sim3Gate g = {0.f, 0.f, -1};
    if (sb_valid(xf, p)) {
        // dir 0: the map points of KF1 into KF2 with sR21, t21 (:1150-1227); dir 1: those of KF2 into KF1 with sR12, t12 (:1230-1307)
        const int f1 = A.pairs[2 * (size_t)p], f2 = A.pairs[2 * (size_t)p + 1];
        const int src = dir ? f2 : f1;
        const size_t s = (size_t)src * A.cap + i;
        if (i < A.count(src)) {
            const olf_track_batch& in = A.in;
            // if(!pMP || vbAlreadyMatched[i]) continue; if(pMP->isBad()) continue (:1154-1158, :1234-1238)
            const bool holds = !in.mp_valid || in.mp_valid[s];
            const bool already = dir ? ((already2[(size_t)p * A.capW + (i >> 5)] >> (i & 31)) & 1u) != 0 : matches12[(size_t)p * A.cap + i] != -1;
            if (holds && !already && !(A.mp_bad && A.mp_bad[s])) {
                const float* X = xf + (size_t)SB_XF * p;
                const float cam[4] = {in.fx, in.fy, in.cx, in.cy}, bounds[4] = {in.minX, in.maxX, in.minY, in.maxY};
                float uv[2], dist3D;
                if (sim3_point_gate(in.Tcw + 16 * (size_t)src, in.mp_world + 3 * s, dir ? X : X + 9, dir ? X + 18 : X + 21, A.mp_maxd[s], A.mp_mind[s], cam,
                                    bounds, uv, dist3D)) {
                    g.u = uv[0]; g.v = uv[1];
                    g.level = fuse_level(A.mp_maxd[s], dist3D, A.thr, A.nlevels);
                }
            }
        }
    }
    gate[e] = g;
}

__global__ __launch_bounds__(256) void k_sim3_search(Sim3Args A, const Sim3Gate* __restrict__ gate, int* __restrict__ vn1, int* __restrict__ vn2,
                                                    int* __restrict__ status)
{
    const int e = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;      // (the wave's entry: scalar from here on)
    const int per = 2 * A.cap;
    if (e >= A.n_pairs * per) return;
    const Sim3Gate g = gate[e];
    const int level = __builtin_amdgcn_readfirstlane(g.level);
    if (level < 0) return;                                            // (the feature keeps vnMatch = -1)
    const int p = e / per, r = e - p * per, dir = r >= A.cap ? 1 : 0, i = r - dir * A.cap;
    const int f1 = A.pairs[2 * (size_t)p], f2 = A.pairs[2 * (size_t)p + 1];      // (passed the gate: both are frames of the batch)
    const int src = dir ? f2 : f1, dst = dir ? f1 : f2;
    const olf_keypoint* keys = A.keys(dst);
    const uint4* kd = A.desc(dst);
    const GridView G = A.grid(dst);                                   // (here, beside the entry's other loads: FrameView::grid)
    // const cv::Mat dMP = pMP->GetDescriptor() (:1199, :1279)
    const uint4* md = A.point_desc(src, i);
    const uint4 a0 = md[0], a1 = md[1];
    // Search in a radius (:1191, :1271)
    const float radius = A.th * A.sf[level];
    int bestKey = SB_NOKEY, bestJ = -1;
    bool badOct = false;
    // GetFeaturesInArea(u, v, radius) and the level gate (:1209-1210, :1289-1290) in one: the walk leaves out what the gate would, and keeps the order of the rest
    grid_walk(G, g.u, g.v, radius, level - 1, level, lane, [&](bool take, int j2, int pos) {
        if (!take) return;
        // (level - 1 <= octave <= level < nlevels: only octave -1 under level 0 lies outside the context's levels)
        if (keys[j2].octave < 0) { badOct = true; return; }
        const int dist = ham256(a0, a1, kd[2 * (size_t)j2], kd[2 * (size_t)j2 + 1]);
        const int key = (dist << SB_POS_BITS) | pos;
        if (key < bestKey) { bestKey = key; bestJ = j2; }
    });
    int m, idx = -1;
    wave_min_fetch(bestKey, bestJ, SB_NOKEY, m, idx);
    const bool anyBad = wave_vote(badOct) != 0;
    if (lane == 0) {
        if (anyBad) atomicOr(status, STATUS_OCTAVE);
        // if(bestDist<=TH_HIGH) vnMatch[i] = bestIdx (:1223-1226, :1303-1306)
        if (idx >= 0 && (m >> SB_POS_BITS) <= SB_TH_HIGH) (dir ? vn2 : vn1)[(size_t)p * A.cap + i] = idx;
    }
}

__global__ __launch_bounds__(256) void k_sim3_agree(Sim3Args A, const float* __restrict__ xf, const int* __restrict__ vn1, const int* __restrict__ vn2,
                                                   int* __restrict__ matches12, int* __restrict__ nfound)
{
    const int p = blockIdx.x, i1 = blockIdx.y * 256 + threadIdx.x;
    if (!sb_valid(xf, p)) return;                                     // (block-uniform)
    const size_t row = (size_t)p * A.cap;
    bool ok = false;
    if (i1 < A.count(A.pairs[2 * (size_t)p])) {
        // Check agreement (:1312-1325)
        const int idx2 = vn1[row + i1];
        if (idx2 >= 0 && idx2 < A.cap && vn2[row + idx2] == i1) { matches12[row + i1] = idx2; ok = true; }
    }
    const int n = wave_sum_i32(ok ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&nfound[p], n);
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_search_by_sim3_pairs_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, const float* d_mp_maxd, const float* d_mp_mind,
                                 int n_pairs, const int32_t* d_pairs, const float* d_s12, const float* d_R12, const float* d_t12, float th,
                                 int32_t* d_matches12, int32_t* d_vn_match1, int32_t* d_vn_match2, int32_t* d_nfound, void* stream)
{
    Sim3Args A;
    int ne;
    // (the per-pair arrays of a call without pairs may be NULL: nothing is required of them)
    const bool ok = n_pairs >= 0 && d_mp_maxd && d_mp_mind && (!n_pairs || (d_pairs && d_s12 && d_R12 && d_t12 && d_matches12 && d_nfound));
    OLF_TRY(batch_frames(c, "olf_search_by_sim3_pairs_dev", ok, in, NEED_GRID | NEED_TCW | NEED_WORLD, n_frames, nullptr, 0, 2LL * n_pairs, "entries", A, &ne));
    if (n_pairs == 0 || n_frames == 0) return OLF_OK;
    const int cap = A.cap;
    A.mp_bad = d_mp_bad; A.mp_maxd = d_mp_maxd; A.mp_mind = d_mp_mind;
    A.pairs = d_pairs; A.s12 = d_s12; A.R12 = d_R12; A.t12 = d_t12;
    A.n_frames = n_frames; A.n_pairs = n_pairs;
    A.th = th;
    OLF_TRY(ctx_level_thresholds(c, A.thr));
    hipStream_t s = ctx_stream(c, stream);
    // scratch: 128 bytes and one bit per feature of the capacity per pair; 12 bytes per (pair, direction, feature); 4 bytes per (pair, feature) for each
    // vnMatch row the caller does not take
    float* xf; unsigned* already2; Sim3Gate* gate; int *vn1 = d_vn_match1, *vn2 = d_vn_match2, *own1, *own2;
    const size_t rows = (size_t)n_pairs * cap, bw = (size_t)n_pairs * A.capW;
    Carve k;
    k.add(&xf, (size_t)SB_XF * n_pairs); k.add(&already2, bw); k.add(&gate, (size_t)ne); k.add(&own1, vn1 ? 0 : rows); k.add(&own2, vn2 ? 0 : rows);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    if (!vn1) vn1 = own1;
    if (!vn2) vn2 = own2;
    const dim3 perPair(n_pairs, (cap + 255) / 256);
    OLF_HIP_CHECK(hipMemsetAsync(already2, 0, bw * 4, s));
    hipLaunchKernelGGL(k_sim3_transform, dim3((n_pairs + 255) / 256), dim3(256), 0, s, A, xf, d_nfound, ctx_status(c));
    hipLaunchKernelGGL(k_sim3_mark, perPair, dim3(256), 0, s, A, xf, d_matches12, already2, vn1, vn2);
    hipLaunchKernelGGL(k_sim3_gate, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, A, xf, d_matches12, already2, gate);
    hipLaunchKernelGGL(k_sim3_search, dim3((unsigned)((ne + 3) / 4)), dim3(256), 0, s, A, gate, vn1, vn2, ctx_status(c));
    hipLaunchKernelGGL(k_sim3_agree, perPair, dim3(256), 0, s, A, xf, vn1, vn2, d_matches12, d_nfound);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
