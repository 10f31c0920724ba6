// projection_batch.hip -- the two key-frame forms of ORBmatcher::SearchByProjection for batches on the device:
//   relocalisation  int SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th, const int ORBdist)
//                   (src/ORBmatcher.cc:1620-1747; Tracking::Relocalization, src/Tracking.cc:2322, :2336) for a list of (current frame, key frame) pairs, each
//                   with its own pose, mvpMapPoints mask and sAlreadyFound
//   loop            int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)
//                   (src/ORBmatcher.cc:292-405; LoopClosing::ComputeSim3, src/LoopClosing.cc:381) for every key frame of a batch against its list of points
// The arithmetic is that of search_host.cpp (olf_search_by_projection_kf; fuse_core with `matched`), and the gates on a point are the text both sides run
// (search_math.hpp: reloc_point_gate, sim3_decompose, fuse_point_gate, fuse_level_ok, rot_bin, three_maxima), the frames, list traversal, recompute and
// histogram rejection those of every ordered walk (batch_frames.hpp, grid_walk.hpp).  No contraction (-ffp-contract=off),
// correctly rounded divisions and square root.
//
// Both are ordered greedy searches: a key point that takes a point is closed to every later point (:1693-1694 with :1714; :378 with :400), and nothing else
// depends on the order.  A query's outcome is "the first entry, in (distance, scan position) order, with distance <= the acceptance threshold, whose key
// point is open": the reference accepts the best open candidate only if its distance is within the threshold (:1712, :397), so a cut at the threshold
// loses nothing.  That is the structure of track_batch.hip and local_batch.hip:
//   k_loop_pose    loop form, one thread per key frame: Rcw | tcw | Ow from Scw (sim3_decompose)
//   k_loop_held    loop form, one thread per (key frame, key point): spAlreadyFound (:307-308) as one bit per (key frame, map point), from vpMatched
//   k_reloc_gate   one thread per (pair, key-frame feature): holds a point / bad / already found, reloc_point_gate, the level from the table of
//   k_loop_gate    olf_predict_scale_thresholds -- one thread per entry: bad / already found, fuse_point_gate without the chi-square gate, the level.
//                  Both write (u, v, radius, level or -1), 16 bytes, and the query's empty list
//   k_proj_lists   one wave per passing query: walks the window (grid_walk, grid_walk.hpp) and keeps the PB_K best entries (Best4, key = distance << 16 |
//                  scan position) whose distance is within the threshold and whose key point was open on entry, plus "there were more" (16 bytes per query)
//   k_proj_walk    one workgroup per pair / key frame, the closed bits in LDS: one wave walks the queries in the reference's order and takes the first
//                  open kept entry; a query whose kept entries are all closed although the window held more is recomputed on the spot by the whole wave,
//                  with the closed test inside the scan -- there is no capacity to exceed.  Every take closes its key point, so a key point receives at most
//                  one event.  The relocalisation form then runs the rotation histogram (ComputeThreeMaxima, :1749-1790) and the rejection
// k_proj_lists and k_proj_walk are one text for both forms, instantiated on RelocForm / LoopForm: what a work item is, which key points are closed on entry,
// where a query's descriptor lives, the levels of its window and what a take stores.
#include <string>
#include "batch_frames.hpp"
#include "entry_lists.hpp"
#include "device_math.hpp"
#include "staging.hpp"

namespace olf {

constexpr int PB_TH_LOW = 50;                       // src/ORBmatcher.cc:40
constexpr int PB_K = 4;                             // entries kept per query (one uint4)
// a list entry: distance << 18 | rotation bin << 13 | key point (< OLF_GRID_MAX_KEYS = 2^13); the first word of a list also carries a flag
constexpr unsigned PB_NONE = Best4::NONE, PB_MORE = 1u << 31;
constexpr int PB_NOKEY = Best4::NOKEY;
static_assert(OLF_GRID_MAX_KEYS <= (1 << 13) && HISTO_LENGTH <= 32 && PB_K == Best4::K, "entry layout");

struct ProjArgs : FrameView {      // (capW: the 32-bit words of the closed bitmap)
    // the relocalisation form
    const uint8_t* mp_bad;         // [n_frames][cap] or NULL
    const float *mp_maxd, *mp_mind;
    const int* pairs;
    const float* pairTcw;          // [n_pairs][16] or NULL
    const uint8_t *cur_valid, *already;      // [n_pairs][cap] or NULL
    const int* d_orb_dist;
    int orb_dist, checkOri;
    // the loop form
    olf_local_map map;
    EntryLists L;
    const float* Scw;
    int* frame_matched;
    int mpW;                       // 32-bit words of the spAlreadyFound bitmap per key frame
    // both
    int n_frames, n_items, n_queries;      // n_items: pairs / key frames
    float th;
    const float* d_th;
};

// a pair (relocalisation) or a key frame (loop)
struct ProjItem {
    int state;                     // 0: skipped (d_th <= 0), 1: searched, 2: a malformed pair
    int tgt, src;                  // the frame whose grid is searched; relocalisation: the key frame whose points are projected
    int nT;                        // key points of tgt
    int qb, qe;                    // its queries, in the reference's order
    int accept;                    // ORBdist / TH_LOW
    float th;
};

struct ProjQuery {
    uint4 a0, a1;                  // the point's descriptor
    float u, v, radius, angle;
    int level;
};

// ---- what differs between the two forms ---------------------------------------------------------------------------------------------------------------
struct RelocForm {
    static constexpr bool kRot = true;              // the rotation histogram (:1716-1734)
    static __device__ __forceinline__ ProjItem item(const ProjArgs& A, int p)
    {
        ProjItem I = {0, 0, 0, 0, 0, 0, 0, 0.f};
        if (!item_radius(A.th, A.d_th, p, I.th)) return I;
        const int fc = A.pairs[2 * (size_t)p], fk = A.pairs[2 * (size_t)p + 1];
        if (!pair_in_batch(fc, fk, A.n_frames)) { I.state = 2; return I; }
        I.state = 1; I.tgt = fc; I.src = fk;
        I.nT = A.count(fc);
        I.qb = p * A.cap; I.qe = I.qb + A.count(fk);
        I.accept = A.d_orb_dist ? A.d_orb_dist[p] : A.orb_dist;
        return I;
    }
    // the item query q belongs to (-1: none) and what the query is inside it: the key-frame feature
    static __device__ __forceinline__ int item_of(const ProjArgs& A, int q, int& local) { const int p = q / A.cap; local = q - p * A.cap; return p; }
    static __device__ __forceinline__ int local_of(const ProjArgs& A, const ProjItem& I, int q) { return q - I.qb; }
    // if(CurrentFrame.mvpMapPoints[i2]) continue (:1693-1694), as the frame stands on entry
    static __device__ __forceinline__ bool closed0(const ProjArgs& A, int p, int j2) { return A.cur_valid && A.cur_valid[(size_t)p * A.cap + j2] != 0; }
    // const cv::Mat dMP = pMP->GetDescriptor() (:1684) and pKF->mvKeysUn[i].angle (:1718)
    static __device__ __forceinline__ void source(const ProjArgs& A, const ProjItem& I, int i, ProjQuery& Q)
    {
        const uint4* md = A.point_desc(I.src, i);
        Q.a0 = md[0]; Q.a1 = md[1];
        Q.angle = A.keys(I.src)[i].angle;
    }
    // GetFeaturesInArea(u, v, radius, nPredictedLevel - 1, nPredictedLevel + 1) (:1679)
    static __device__ __forceinline__ void window(int level, int& lo, int& hi) { lo = level - 1; hi = level + 1; }
    static __device__ __forceinline__ bool level_ok(int, int) { return true; }
    // what a take stores for its key point until the histogram is known: rotation bin << 16 | key-frame feature
    static __device__ __forceinline__ int value(int i, int bin) { return (bin << 16) | i; }
};

struct LoopForm {
    static constexpr bool kRot = false;
    static __device__ __forceinline__ ProjItem item(const ProjArgs& A, int j)
    {
        ProjItem I = {0, 0, 0, 0, 0, 0, 0, 0.f};
        if (!item_radius(A.th, A.d_th, j, I.th)) return I;
        I.state = 1; I.tgt = j; I.src = j;
        I.nT = A.count(j);
        A.L.range(j, I.qb, I.qe);
        I.accept = PB_TH_LOW;
        return I;
    }
    // the key frame entry q belongs to (-1: none) and its map index (unchecked)
    static __device__ __forceinline__ int item_of(const ProjArgs& A, int q, int& local) { return A.L.frame_of(q, local); }
    static __device__ __forceinline__ int local_of(const ProjArgs& A, const ProjItem& I, int q) { return A.L.offsets ? A.L.index[q] : q - I.qb; }
    // if(vpMatched[idx]) continue (:378), as vpMatched stands on entry: any value but -1 is a point
    static __device__ __forceinline__ bool closed0(const ProjArgs& A, int j, int j2) { return A.frame_matched[(size_t)j * A.cap + j2] != -1; }
    // const cv::Mat dMP = pMP->GetDescriptor() (:370)
    static __device__ __forceinline__ void source(const ProjArgs& A, const ProjItem&, int mi, ProjQuery& Q)
    {
        const uint4* md = reinterpret_cast<const uint4*>(A.map.desc) + 2 * (size_t)mi;
        Q.a0 = md[0]; Q.a1 = md[1];
        Q.angle = 0.f;
    }
    // GetFeaturesInArea(u, v, radius) (:364), then the level gate on every candidate (:383-384)
    static __device__ __forceinline__ void window(int, int& lo, int& hi) { lo = -1; hi = -1; }
    static __device__ __forceinline__ bool level_ok(int kpLevel, int level) { return fuse_level_ok(kpLevel, level); }
    // vpMatched[bestIdx] = pMP (:400)
    static __device__ __forceinline__ int value(int mi, int) { return mi; }
};

// ---- the point gates -------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 pb_empty() { return make_uint4(PB_NONE, PB_NONE, PB_NONE, PB_NONE); }

__global__ __launch_bounds__(256) void k_reloc_gate(ProjArgs A, float4* __restrict__ gate, uint4* __restrict__ lists, int* __restrict__ nmatches,
                                                   int* __restrict__ status)
{
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.cap) return;
    const ProjItem I = RelocForm::item(A, p);
    if (I.state == 2 && i == 0) { nmatches[p] = -1; atomicOr(status, STATUS_PAIR); }
    const int q = p * A.cap + i;
    float4 g = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    if (I.state == 1 && q < I.qe) {
        const olf_track_batch& in = A.in;
        const size_t s = (size_t)I.src * A.cap + i;
        // if(pMP) if(!pMP->isBad() && !sAlreadyFound.count(pMP)) (:1644-1648)
        const bool holds = !in.mp_valid || in.mp_valid[s];
        if (holds && !(A.mp_bad && A.mp_bad[s]) && !(A.already && A.already[q])) {
            const float* T = A.pairTcw ? A.pairTcw + 16 * (size_t)p : in.Tcw + 16 * (size_t)I.tgt;
            const float cam[4] = {in.fx, in.fy, in.cx, in.cy}, bounds[4] = {in.minX, in.maxX, in.minY, in.maxY};
            float Ow[3], uv[2], dist3D;
            camera_centre(T, Ow);                                     // const cv::Mat Ow = -Rcw.t() * tcw (:1628)
            const float maxd = A.mp_maxd[s];
            if (reloc_point_gate(T, Ow, in.mp_world + 3 * s, maxd, A.mp_mind[s], cam, bounds, uv, dist3D)) {
                const int level = fuse_level(maxd, dist3D, A.thr, A.nlevels);
                // Search in a window (:1677)
                g = make_float4(uv[0], uv[1], I.th * A.sf[level], __int_as_float(level));
            }
        }
    }
    gate[q] = g;
    lists[q] = pb_empty();
}

__global__ __launch_bounds__(256) void k_loop_pose(ProjArgs A, float* __restrict__ pose)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= A.n_frames) return;
    float R[9], t[3], ow[3];
    sim3_decompose(A.Scw + 16 * (size_t)j, R, t, ow);
    pose_store(pose + (size_t)POSE_FLOATS * j, R, t, ow);
}

// set<MapPoint*> spAlreadyFound(vpMatched.begin(), vpMatched.end()) (:307-308)
__global__ __launch_bounds__(256) void k_loop_held(ProjArgs A, unsigned* __restrict__ held, int* __restrict__ status)
{
    const int j = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < A.count(j)) held_mark(A.frame_matched[(size_t)j * A.cap + idx], A.map.n_mp, A.map.bad, held + (size_t)j * A.mpW, status, STATUS_POINT_INDEX);
}

__global__ __launch_bounds__(256) void k_loop_gate(ProjArgs A, const float* __restrict__ pose, const unsigned* __restrict__ held, float4* __restrict__ gate,
                                                  uint4* __restrict__ lists, int* __restrict__ status)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.n_queries) return;
    float4 g = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    int i = -1;
    const int j = A.L.frame_of(e, i);
    float th;
    if (j >= 0 && item_radius(A.th, A.d_th, j, th)) {
        if ((unsigned)i >= (unsigned)A.map.n_mp) atomicOr(status, STATUS_POINT_INDEX);
        // Discard Bad MapPoints and already found (:321)
        else if (!A.map.bad[i] && !((held[(size_t)j * A.mpW + (i >> 5)] >> (i & 31)) & 1u)) {
            const olf_track_batch& in = A.in;
            const float cam[5] = {in.fx, in.fy, in.cx, in.cy, in.mbf}, bounds[4] = {in.minX, in.maxX, in.minY, in.maxY};
            const float* P = pose + (size_t)POSE_FLOATS * j;
            float uvr[3], dist3D;
            const float maxd = A.map.maxd[i];
            if (fuse_point_gate(P, P + 9, P + 12, A.map.world + 3 * (size_t)i, A.map.normal + 3 * (size_t)i, maxd, A.map.mind[i], cam, bounds, uvr, dist3D)) {
                const int level = fuse_level(maxd, dist3D, A.thr, A.nlevels);
                // Search in a radius (:362)
                g = make_float4(uvr[0], uvr[1], th * A.sf[level], __int_as_float(level));
            }
        }
    }
    gate[e] = g;
    lists[e] = pb_empty();
}

// ---- the ordered part, one text for both forms -------------------------------------------------------------------------------------------------------------
template <class F>
__device__ __forceinline__ ProjQuery pb_query(const ProjArgs& A, const ProjItem& I, int local, const float4& g)
{
    ProjQuery Q;
    Q.u = g.x; Q.v = g.y; Q.radius = g.z; Q.level = __float_as_int(g.w);
    F::source(A, I, local, Q);
    return Q;
}

// the state-free tests on one candidate: the level gate of the loop form and the distance.  true: the candidate could be chosen (distance within the
// threshold; bestDist starts at 256, so 256 itself never registers); key orders such candidates as the reference's `dist < bestDist` scan does
template <class F>
__device__ __forceinline__ bool pb_candidate(const ProjItem& I, const ProjQuery& Q, const olf_keypoint* __restrict__ keys, const uint4* __restrict__ kd, int j,
                                             int pos, int& key, unsigned& ent)
{
    const olf_keypoint& kp = keys[j];
    if (!F::level_ok(kp.octave, Q.level)) return false;
    const int dist = ham256(Q.a0, Q.a1, kd[2 * (size_t)j], kd[2 * (size_t)j + 1]);
    if (dist > I.accept || dist >= 256) return false;
    int bin = 0;
    if (F::kRot) {
        bin = rot_bin(Q.angle, kp.angle);                              // (:1718-1725)
        bin = min(max(bin, 0), HISTO_LENGTH - 1);      // (angles outside [0, 360) index past rotHist in the reference; here they land in an end bin)
    }
    key = (dist << 16) | pos;
    ent = ((unsigned)dist << 18) | ((unsigned)bin << 13) | (unsigned)j;
    return true;
}

template <class F>
__global__ __launch_bounds__(256) void k_proj_lists(ProjArgs A, const float4* __restrict__ gate, uint4* __restrict__ lists)
{
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;      // (the wave's query: scalar from here on)
    if (q >= A.n_queries) return;
    const float4 g = gate[q];
    if (__builtin_amdgcn_readfirstlane(__float_as_int(g.w)) < 0) return;      // (the query keeps its empty list)
    int local = -1;
    const int it = F::item_of(A, q, local);                           // (passed the gate: an item that is searched)
    const ProjItem I = F::item(A, it);
    const ProjQuery Q = pb_query<F>(A, I, local, g);
    const GridView G = A.grid(I.tgt, I.nT);
    const uint4* kd = A.desc(I.tgt);
    int lo, hi;
    F::window(Q.level, lo, hi);
    unsigned out[PB_K] = {PB_NONE, PB_NONE, PB_NONE, PB_NONE};
    int cnt = 0;
    Best4 best;
    grid_walk(G, Q.u, Q.v, Q.radius, lo, hi, lane, [&](bool take, int j2, int pos) {
        int key = PB_NOKEY;
        unsigned ent = PB_NONE;
        const bool ok = take && !F::closed0(A, it, j2) && pb_candidate<F>(I, Q, G.keys, kd, j2, pos, key, ent);
        cnt += __popcll(wave_vote(ok));
        best.push(ok, key, ent);
    });
    best.drain(out);
    if (lane == 0) lists[q] = make_uint4(out[0] | (cnt > PB_K ? PB_MORE : 0u), out[1], out[2], out[3]);
}

// query q again, with the closed test inside the scan: the entry the reference would choose now, or PB_NONE
template <class F>
__device__ __forceinline__ unsigned pb_rescan(const ProjArgs& A, const ProjItem& I, int local, const float4& g, int lane, const unsigned* s_closed)
{
    const ProjQuery Q = pb_query<F>(A, I, local, g);
    const GridView G = A.grid(I.tgt, I.nT);
    const uint4* kd = A.desc(I.tgt);
    int lo, hi;
    F::window(Q.level, lo, hi);
    return window_best(G, Q.u, Q.v, Q.radius, lo, hi, lane, [&](int j2, int pos, int& key, unsigned& ent) {
        return !((s_closed[j2 >> 5] >> (j2 & 31)) & 1u) && pb_candidate<F>(I, Q, G.keys, kd, j2, pos, key, ent);
    });
}

// One workgroup per pair / key frame; dynamic LDS: cap ints (what a key point received in this call, -1: nothing), then capW words (closed bits).
// matches: the relocalisation form's rows [n_pairs][cap]; the loop form's d_frame_matched, of which only the key points that took a point are written.
template <class F>
__global__ __launch_bounds__(256) void k_proj_walk(ProjArgs A, const float4* __restrict__ gate, const uint4* __restrict__ lists, int* __restrict__ matches,
                                                   int* __restrict__ nmatches)
{
    extern __shared__ int s_match[];
    __shared__ int s_hist[HISTO_LENGTH], s_n;
    __shared__ unsigned s_reject;
    unsigned* s_closed = reinterpret_cast<unsigned*>(s_match + A.cap);
    const int it = blockIdx.x, tid = threadIdx.x, lane = tid & 63, cap = A.cap;
    const ProjItem I = F::item(A, it);
    if (I.state != 1) return;                                        // (skipped: rows untouched; malformed: k_reloc_gate wrote nmatches = -1)
    for (int i = tid; i < cap; i += 256) s_match[i] = -1;
    for (int w = tid; w < A.capW; w += 256) s_closed[w] = 0u;
    if (tid == 0) { s_n = 0; s_reject = 0; }
    __syncthreads();
    for (int i = tid; i < I.nT; i += 256) if (F::closed0(A, it, i)) atomicOr(&s_closed[i >> 5], 1u << (i & 31));
    __syncthreads();
    if (tid < 64) {
        int n = 0, myHist = 0;                                       // lane b counts the events of rotation bin b
        // (the traversal walk_lists states, in this kernel's own text: through walk_lists the relocalisation form's walk took 56.0 us where this takes 53.4,
        // kernel trace on an MI355X)
        for (int c0 = I.qb; c0 < I.qe; c0 += 64) {
            const int q = c0 + lane;
            uint4 L = pb_empty();
            int local = -1;
            if (q < I.qe) { L = lists[q]; local = F::local_of(A, I, q); }
            unsigned long long todo = wave_vote((L.x & PB_NONE) != PB_NONE);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const unsigned x = (unsigned)__shfl((int)L.x, l, 64);
                const unsigned e[PB_K] = {x & PB_NONE, (unsigned)__shfl((int)L.y, l, 64), (unsigned)__shfl((int)L.z, l, 64), (unsigned)__shfl((int)L.w, l, 64)};
                const int who = __shfl(local, l, 64);
                bool exhausted;
                unsigned hit = first_open(e, exhausted, [&](unsigned f) { return !((s_closed[f >> 5] >> (f & 31)) & 1u); });
                if (exhausted && (x & PB_MORE)) hit = pb_rescan<F>(A, I, who, gate[c0 + l], lane, s_closed);
                if (hit != PB_NONE) {
                    // CurrentFrame.mvpMapPoints[bestIdx2] = pMP; nmatches++; rotHist[bin].push_back(bestIdx2) (:1712-1733) / vpMatched[bestIdx] = pMP;
                    // nmatches++ (:397-401)
                    const unsigned i2 = hit & 0x1fffu;
                    const int bin = (int)((hit >> 13) & 31u);
                    s_match[i2] = F::value(who, bin);                // (every lane stores the same values: the next query's reads are ordered behind them)
                    s_closed[i2 >> 5] |= 1u << (i2 & 31);
                    if (F::kRot && A.checkOri && lane == bin) ++myHist;
                    ++n;
                }
            }
        }
        if (lane < HISTO_LENGTH) s_hist[lane] = myHist;
        if (lane == 0) s_n = n;
    }
    __syncthreads();
    if (F::kRot) {
        if (A.checkOri) {
            if (tid == 0) { int n = s_n; s_reject = histo_reject(s_hist, n); s_n = n; }
            __syncthreads();
        }
        const unsigned rej = s_reject;
        for (int i2 = tid; i2 < cap; i2 += 256) {
            const int m = s_match[i2];
            const bool keep = m >= 0 && !((rej >> (m >> 16)) & 1u);
            matches[(size_t)it * cap + i2] = keep ? (m & 0xffff) : -1;
        }
    } else {
        for (int i2 = tid; i2 < cap; i2 += 256) {
            const int m = s_match[i2];
            if (m >= 0) matches[(size_t)it * cap + i2] = m;
        }
    }
    if (tid == 0) nmatches[it] = s_n;
}

}  // namespace olf

using namespace olf;

namespace {

template <class F>
void pb_ordered(const ProjArgs& A, const float4* gate, uint4* lists, int* matches, int* nmatches, hipStream_t s)
{
    if (A.n_queries) hipLaunchKernelGGL(k_proj_lists<F>, dim3((unsigned)(((long long)A.n_queries + 3) / 4)), dim3(256), 0, s, A, gate, lists);
    const size_t lds = ((size_t)A.cap + A.capW) * 4;
    hipLaunchKernelGGL(k_proj_walk<F>, dim3(A.n_items), dim3(256), lds, s, A, gate, lists, matches, nmatches);
}

}  // namespace

extern "C" {

int olf_search_by_projection_kf_pairs_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, const float* d_mp_maxd,
                                          const float* d_mp_mind, int n_pairs, const int32_t* d_pairs, const float* d_Tcw, const uint8_t* d_cur_valid,
                                          const uint8_t* d_already_found, float th, const float* d_th, int orb_dist, const int32_t* d_orb_dist,
                                          int check_orientation, int32_t* d_matches, int32_t* d_nmatches, void* stream)
{
    ProjArgs A = {};
    // (the per-pair arrays of a call without pairs may be NULL: nothing is required of them)
    const bool ok = n_pairs >= 0 && d_mp_maxd && d_mp_mind && (!n_pairs || (d_pairs && d_matches && d_nmatches));
    OLF_TRY(batch_frames(c, "olf_search_by_projection_kf_pairs_dev", ok, in, NEED_GRID | NEED_WORLD | (d_Tcw ? 0 : NEED_TCW), n_frames, nullptr, 0, n_pairs, "queries",
                         A, &A.n_queries));
    if (n_pairs == 0 || n_frames == 0) return OLF_OK;
    const int cap = A.cap, nq = A.n_queries;
    A.n_frames = n_frames; A.th = th; A.d_th = d_th;
    A.mp_bad = d_mp_bad; A.mp_maxd = d_mp_maxd; A.mp_mind = d_mp_mind;
    A.pairs = d_pairs; A.pairTcw = d_Tcw; A.cur_valid = d_cur_valid; A.already = d_already_found;
    A.d_orb_dist = d_orb_dist; A.orb_dist = orb_dist; A.checkOri = check_orientation ? 1 : 0;
    A.n_items = n_pairs;
    OLF_TRY(ctx_level_thresholds(c, A.thr));
    hipStream_t s = ctx_stream(c, stream);
    // scratch: 32 bytes per (pair, feature): (u, v, radius, level) and the kept entries
    float4* gate; uint4* lists;
    Carve k;
    k.add(&gate, (size_t)nq); k.add(&lists, (size_t)nq);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    hipLaunchKernelGGL(k_reloc_gate, dim3((cap + 255) / 256, n_pairs), dim3(256), 0, s, A, gate, lists, d_nmatches, ctx_status(c));
    pb_ordered<RelocForm>(A, gate, lists, d_matches, d_nmatches, s);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_search_by_projection_sim3_batch_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const olf_local_map* map, const float* d_Scw,
                                            int32_t* d_frame_matched, float th, const float* d_th, int32_t* d_nmatches, void* stream)
{
    ProjArgs A = {};
    OLF_TRY(batch_frames(c, "olf_search_by_projection_sim3_batch_dev", map && d_Scw && d_frame_matched && d_nmatches, in, NEED_GRID, n_frames, map, MAP_DESC, 0,
                         "entries", A, &A.n_queries));
    if (n_frames == 0) return OLF_OK;
    const int cap = A.cap, ne = A.n_queries;
    A.n_frames = n_frames; A.th = th; A.d_th = d_th;
    A.map = *map;
    A.L = {map->list_offsets, map->list_index, map->n_mp, n_frames, ne};
    A.Scw = d_Scw; A.frame_matched = d_frame_matched;
    A.mpW = (map->n_mp + 31) / 32;
    A.n_items = n_frames;
    OLF_TRY(ctx_level_thresholds(c, A.thr));
    hipStream_t s = ctx_stream(c, stream);
    // scratch: 32 bytes per entry: (u, v, radius, level) and the kept entries; 64 bytes per key frame (the pose) and one bit per (key frame, map point)
    float4* gate; uint4* lists; float* pose; unsigned* held;
    const size_t bh = (size_t)n_frames * A.mpW;
    Carve k;
    k.add(&gate, (size_t)ne); k.add(&lists, (size_t)ne); k.add(&pose, (size_t)POSE_FLOATS * n_frames); k.add(&held, bh);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    hipLaunchKernelGGL(k_loop_pose, dim3((n_frames + 255) / 256), dim3(256), 0, s, A, pose);
    if (bh) OLF_HIP_CHECK(hipMemsetAsync(held, 0, bh * 4, s));
    hipLaunchKernelGGL(k_loop_held, dim3((cap + 255) / 256, n_frames), dim3(256), 0, s, A, held, ctx_status(c));      // (an empty map: every held index lies outside it)
    if (ne) hipLaunchKernelGGL(k_loop_gate, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, A, pose, held, gate, lists, ctx_status(c));
    pb_ordered<LoopForm>(A, gate, lists, d_frame_matched, d_nmatches, s);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
