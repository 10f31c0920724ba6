// track_batch.hip -- ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono[, map<int,int>& match12])
// (src/ORBmatcher.cc:1330-1472, :1474-1618; Tracking::TrackWithMotionModel[WithLine], src/Tracking.cc:1296,1302) for a whole batch of consecutive frames on
// the device, and Frame::UnprojectStereo (src/Frame.cc:1073-1087) for every feature of a batch.  The arithmetic is that of search_host.cpp
// (search_by_projection_frames): convention C.12 for the cv::Mat products, no contraction (-ffp-contract=off).
//
// Only one thing in the reference's loop depends on the order of the last frame's features: a CurrentFrame feature is skipped while the map point it received
// last has observations (:1405-1407).  Everything else -- projection, image gates, the grid walk, level gates, the window tests, the mvuRight gate, the
// distance -- is a function of (pair, last feature) alone, and a query's outcome is "the first entry, in (distance, scan position) order, with distance <=
// TH_HIGH, whose feature is not blocked".  So:
//   k_track_lists   one wave per (pair, last feature): walks the window as k_features_in_area does and keeps the TB_K best entries with distance <= TH_HIGH
//                   (16 bytes per query, whatever the window holds), plus "there were more" and the point's Observations() bit
//   k_track_walk    one workgroup per pair: one wave walks the lists in index order against the pair's blocked bits in LDS; a query whose kept entries
//                   are all blocked although the window held more is recomputed on the spot by the whole wave, with the blocked test inside the scan -- so
//                   there is no capacity to exceed; then the rotation histogram (ComputeThreeMaxima, :1749-1790) and the output rows
//   k_unproject_stereo  Frame::UnprojectStereo, one thread per feature
#include <algorithm>
#include "olf_internal.hpp"
#include "../../include/orbline.h"

namespace olf {

hipStream_t ctx_stream(olf_ctx* c);
int ctx_scratch(olf_ctx* c, int slot, size_t bytes, void** out);
int* ctx_status(olf_ctx* c);
int ctx_check_device(const olf_ctx* c, const char* who);
int ctx_orb_levels(const olf_ctx* c);

constexpr int TB_TH_HIGH = 100, TB_HISTO = 30;      // src/ORBmatcher.cc:39-41
constexpr int TB_K = 4;                             // entries kept per query (one uint4)
constexpr int TB_ROWS = OLF_GRID_ROWS, TB_COLS = OLF_GRID_COLS;
// a list entry: distance << 18 | rotation bin << 13 | CurrentFrame feature (< OLF_GRID_MAX_KEYS = 2^13); the first word of a list also carries two flags
constexpr unsigned TB_NONE = 0x3fffffffu, TB_OBS = 1u << 30, TB_MORE = 1u << 31;
// per CurrentFrame feature in the walk: bit b = an event of rotation bin b landed here, then
constexpr unsigned TB_SEEN = 1u << 30, TB_BLOCKED = 1u << 31;
constexpr int TB_NOKEY = 0x7fffffff;
constexpr int TB_STATUS_OCTAVE = 256;               // status bit: a pair was skipped, its last frame holds an octave outside the context's levels
static_assert(OLF_GRID_MAX_KEYS <= (1 << 13) && TB_HISTO <= 30, "entry and word layouts");

struct TrackArgs {
    olf_track_batch in;
    int cap, nlevels, bMono;
    float th;
    const float* d_th;
    float wInv, hInv;
    float sf[OLF_MAX_LEVELS];      // mvScaleFactors
};

struct TbPair {
    const olf_keypoint *kL, *kC;
    const uint4 *dL, *dC;
    const float *urC, *TcwC, *world;
    const int *offs, *idx;
    const uint8_t *valid, *obs, *outl;
    int nL, nC;
    bool fwd, bwd;
    float th;
};

struct TbQuery {
    float u, v, invzc, radius;
    int minLevel, maxLevel;
    int state;                     // 0: no window, 1: search it, 2: octave outside the levels
};

// the radius of pair j; false: the pair is skipped (d_th[j] <= 0)
__device__ __forceinline__ bool tb_radius(const TrackArgs& A, int j, float& th)
{
    th = A.th;
    if (!A.d_th) return true;
    th = A.d_th[j];
    return th > 0.f;
}

__device__ __forceinline__ TbPair tb_pair(const TrackArgs& A, int j, float th)
{
    const olf_track_batch& in = A.in;
    const size_t cap = (size_t)A.cap, fL = (size_t)j, fC = (size_t)j + 1, st = (size_t)in.img_stride;
    TbPair P;
    P.kL = in.kps + fL * st * cap; P.kC = in.kps + fC * st * cap;
    P.dL = reinterpret_cast<const uint4*>(in.mp_desc ? in.mp_desc + 32 * fL * cap : in.desc + 32 * fL * st * cap);
    P.dC = reinterpret_cast<const uint4*>(in.desc + 32 * fC * st * cap);
    P.urC = in.uright + fC * cap;
    P.TcwC = in.Tcw + 16 * fC;
    P.world = in.mp_world + 3 * fL * cap;
    P.offs = in.cell_offsets + fC * (OLF_GRID_CELLS + 1);
    P.idx = in.cell_index + fC * cap;
    P.valid = in.mp_valid ? in.mp_valid + fL * cap : nullptr;
    P.obs = in.mp_obs ? in.mp_obs + fL * cap : nullptr;
    P.outl = in.outlier ? in.outlier + fL * cap : nullptr;
    P.nL = min(max(in.counts[fL * st], 0), A.cap);
    P.nC = min(max(in.counts[fC * st], 0), A.cap);
    P.th = th;
    // twc = -Rcw.t() * tcw;  tlc = Rlw * twc + tlw                                   (:1341-1349)
    const float* Tc = P.TcwC;
    const float* Tl = in.Tcw + 16 * fL;
    float twc[3];
    for (int r = 0; r < 3; ++r) {
        double acc = 0;
        for (int k = 0; k < 3; ++k) acc += (double)Tc[4 * k + r] * (double)Tc[4 * k + 3];
        twc[r] = (float)(-acc);
    }
    const float t = Tl[8] * twc[0] + Tl[9] * twc[1] + Tl[10] * twc[2];
    const float tlc2 = (float)((double)t + (double)1.0f * (double)Tl[11]);
    const float mb = in.mbf / in.fx;
    P.fwd = tlc2 > mb && !A.bMono;
    P.bwd = -tlc2 > mb && !A.bMono;
    return P;
}

// the gates of one last-frame feature up to its window (:1369-1400)
__device__ __forceinline__ TbQuery tb_query(const TbPair& P, const TrackArgs& A, int i)
{
    TbQuery q;
    q.state = 0; q.u = q.v = q.invzc = q.radius = 0.f; q.minLevel = q.maxLevel = -1;
    if (P.valid && !P.valid[i]) return q;
    if (P.outl && P.outl[i]) return q;
    const float* T = P.TcwC;
    const float* w = P.world + 3 * (size_t)i;
    float x3Dc[3];
    for (int r = 0; r < 3; ++r) {
        const float t = T[4 * r] * w[0] + T[4 * r + 1] * w[1] + T[4 * r + 2] * w[2];
        x3Dc[r] = (float)((double)t + (double)1.0f * (double)T[4 * r + 3]);
    }
    const float xc = x3Dc[0], yc = x3Dc[1];
    const float invzc = (float)(1.0 / x3Dc[2]);
    if (invzc < 0) return q;
    const olf_track_batch& in = A.in;
    const float u = in.fx * xc * invzc + in.cx, v = in.fy * yc * invzc + in.cy;
    if (u < in.minX || u > in.maxX) return q;
    if (v < in.minY || v > in.maxY) return q;
    const int nLastOctave = P.kL[i].octave;
    if (nLastOctave < 0 || nLastOctave >= A.nlevels) { q.state = 2; return q; }
    q.u = u; q.v = v; q.invzc = invzc;
    q.radius = P.th * A.sf[nLastOctave];
    if (P.fwd) { q.minLevel = nLastOctave; q.maxLevel = -1; }
    else if (P.bwd) { q.minLevel = 0; q.maxLevel = nLastOctave; }
    else { q.minLevel = nLastOctave - 1; q.maxLevel = nLastOctave + 1; }
    q.state = 1;
    return q;
}

// Frame::GetFeaturesInArea(u, v, radius, minLevel, maxLevel) on the CurrentFrame's grid, by one wave: f(take, j, pos) is called by every lane for every chunk
// of 64 grid entries; `take` lanes hold feature j, the pos-th index the reference's vIndices2 would hold (ix outer, iy inner, stored order inside a cell --
// the walk of k_features_in_area, grid.hip).  Entries that a malformed grid points outside the frame are left out.
template <class F>
__device__ __forceinline__ void tb_scan(const TbPair& P, const TrackArgs& A, const TbQuery& q, int lane, F&& f)
{
    const float x = q.u, y = q.v, r = q.radius, minX = A.in.minX, minY = A.in.minY;
    const float fx0 = floorf((x - minX - r) * A.wInv), fx1 = ceilf((x - minX + r) * A.wInv);
    const float fy0 = floorf((y - minY - r) * A.hInv), fy1 = ceilf((y - minY + r) * A.hInv);
    if (!(fx0 < (float)TB_COLS) || !(fx1 >= 0.f) || !(fy0 < (float)TB_ROWS) || !(fy1 >= 0.f)) return;
    const int nMinCellX = fx0 < 0.f ? 0 : (int)fx0, nMaxCellX = fx1 > (float)(TB_COLS - 1) ? TB_COLS - 1 : (int)fx1;
    const int nMinCellY = fy0 < 0.f ? 0 : (int)fy0, nMaxCellY = fy1 > (float)(TB_ROWS - 1) ? TB_ROWS - 1 : (int)fy1;
    if (nMinCellY > nMaxCellY) return;
    const bool bCheckLevels = (q.minLevel > 0) || (q.maxLevel >= 0);
    int total = 0;
    for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
        const int p0 = max(P.offs[ix * TB_ROWS + nMinCellY], 0), p1 = min(P.offs[ix * TB_ROWS + nMaxCellY + 1], A.cap);
        for (int pb = p0; pb < p1; pb += 64) {
            const int p = pb + lane;
            bool take = false;
            int j = 0;
            if (p < p1) {
                j = P.idx[p];
                if ((unsigned)j < (unsigned)P.nC) {
                    const olf_keypoint& kp = P.kC[j];
                    take = true;
                    if (bCheckLevels) {
                        if (kp.octave < q.minLevel) take = false;
                        if (q.maxLevel >= 0 && kp.octave > q.maxLevel) take = false;
                    }
                    const float distx = kp.x - x, disty = kp.y - y;
                    if (!(fabsf(distx) < r && fabsf(disty) < r)) take = false;
                }
            }
            const unsigned long long m = wave_vote(take);
            f(take, j, total + wave_rank_below(m));
            total += __popcll(m);
        }
    }
}

// the state-free tests on one candidate (:1409-1423): the mvuRight gate and the distance.  true: the candidate could be chosen (distance <= TH_HIGH);
// key orders such candidates as the reference's `dist < bestDist` scan does, ent is the list entry
__device__ __forceinline__ bool tb_candidate(const TbPair& P, const TrackArgs& A, const TbQuery& q, const uint4& a0, const uint4& a1, float angL, int j, int pos,
                                             int& key, unsigned& ent)
{
    const float uR = P.urC[j];
    if (uR > 0) {
        const float ur = q.u - A.in.mbf * q.invzc;
        const float er = fabsf(ur - uR);
        if (er > q.radius) return false;
    }
    const uint4 x0 = P.dC[2 * (size_t)j], x1 = P.dC[2 * (size_t)j + 1];
    const int dist = __popc(a0.x ^ x0.x) + __popc(a0.y ^ x0.y) + __popc(a0.z ^ x0.z) + __popc(a0.w ^ x0.w) + __popc(a1.x ^ x1.x) + __popc(a1.y ^ x1.y) +
                     __popc(a1.z ^ x1.z) + __popc(a1.w ^ x1.w);
    if (dist > TB_TH_HIGH) return false;
    float rot = angL - P.kC[j].angle;                                           // (:1434-1441)
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / TB_HISTO));
    if (bin == TB_HISTO) bin = 0;
    bin = min(max(bin, 0), TB_HISTO - 1);      // (angles outside [0, 360) index past rotHist in the reference; here they land in an end bin)
    key = (dist << 16) | pos;
    ent = ((unsigned)dist << 18) | ((unsigned)bin << 13) | (unsigned)j;
    return true;
}

__global__ __launch_bounds__(256) void k_track_lists(TrackArgs A, uint4* __restrict__ lists, int* __restrict__ pairBad, int* __restrict__ status)
{
    const int j = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    float th;
    if (!tb_radius(A, j, th)) return;
    const TbPair P = tb_pair(A, j, th);
    if (i >= P.nL) return;                                       // (wave-uniform)
    const TbQuery q = tb_query(P, A, i);
    unsigned out[TB_K] = {TB_NONE, TB_NONE, TB_NONE, TB_NONE};
    int cnt = 0;
    if (q.state == 2) {
        if (lane == 0) { atomicOr(status, TB_STATUS_OCTAVE); pairBad[j] = 1; }
    } else if (q.state == 1) {
        const uint4 a0 = P.dL[2 * (size_t)i], a1 = P.dL[2 * (size_t)i + 1];
        const float angL = P.kL[i].angle;
        // every lane keeps the TB_K smallest keys it meets, ascending; the TB_K smallest of the window are among them
        int h0 = TB_NOKEY, h1 = TB_NOKEY, h2 = TB_NOKEY, h3 = TB_NOKEY;
        unsigned e0 = TB_NONE, e1 = TB_NONE, e2 = TB_NONE, e3 = TB_NONE;
        tb_scan(P, A, q, lane, [&](bool take, int j2, int pos) {
            int key = TB_NOKEY;
            unsigned ent = TB_NONE;
            const bool ok = take && tb_candidate(P, A, q, a0, a1, angL, j2, pos, key, ent);
            cnt += __popcll(wave_vote(ok));
            if (ok && key < h3) {
                h3 = key; e3 = ent;
                if (h3 < h2) { const int t = h2; h2 = h3; h3 = t; const unsigned u = e2; e2 = e3; e3 = u; }
                if (h2 < h1) { const int t = h1; h1 = h2; h2 = t; const unsigned u = e1; e1 = e2; e2 = u; }
                if (h1 < h0) { const int t = h0; h0 = h1; h1 = t; const unsigned u = e0; e0 = e1; e1 = u; }
            }
        });
        for (int k = 0; k < TB_K; ++k) {
            const int m = wave_min_i32(h0);
            if (m == TB_NOKEY) break;
            const bool mine = h0 == m;                               // keys are distinct: one lane
            const int owner = __ffsll((long long)wave_vote(mine)) - 1;
            out[k] = (unsigned)__shfl((int)e0, owner, 64);
            if (mine) { h0 = h1; e0 = e1; h1 = h2; e1 = e2; h2 = h3; e2 = e3; h3 = TB_NOKEY; e3 = TB_NONE; }
        }
    }
    if (lane == 0) {
        unsigned x = out[0];
        if (cnt > TB_K) x |= TB_MORE;
        if (!P.obs || P.obs[i]) x |= TB_OBS;
        lists[(size_t)j * A.cap + i] = make_uint4(x, out[1], out[2], out[3]);
    }
}

// the query of last-frame feature i again, with the blocked test inside the scan: the entry the reference would choose now, or TB_NONE
__device__ __forceinline__ unsigned tb_rescan(const TbPair& P, const TrackArgs& A, int i, int lane, const unsigned* s_word)
{
    const TbQuery q = tb_query(P, A, i);
    if (q.state != 1) return TB_NONE;
    const uint4 a0 = P.dL[2 * (size_t)i], a1 = P.dL[2 * (size_t)i + 1];
    const float angL = P.kL[i].angle;
    int best = TB_NOKEY;
    unsigned bestEnt = TB_NONE;
    tb_scan(P, A, q, lane, [&](bool take, int j2, int pos) {
        int key = TB_NOKEY;
        unsigned ent = TB_NONE;
        const bool ok = take && !(s_word[j2] & TB_BLOCKED) && tb_candidate(P, A, q, a0, a1, angL, j2, pos, key, ent);
        const int m = wave_min_i32(ok ? key : TB_NOKEY);
        if (m < best) {                                              // (later chunks hold later scan positions: a tie is impossible, `<` as in the reference)
            const int owner = __ffsll((long long)wave_vote(ok && key == m)) - 1;
            best = m;
            bestEnt = (unsigned)__shfl((int)ent, owner, 64);
        }
    });
    return bestEnt;
}

// One workgroup per pair; dynamic LDS: cap words, then cap uint16 (the last frame's index a feature holds).
__global__ __launch_bounds__(256) void k_track_walk(TrackArgs A, const uint4* __restrict__ lists, const int* __restrict__ pairBad, int checkOri,
                                                    int* __restrict__ matches, int* __restrict__ match12, int* __restrict__ nmatches)
{
    extern __shared__ unsigned s_word[];
    __shared__ int s_hist[TB_HISTO], s_n;
    __shared__ unsigned s_reject;
    unsigned short* s_last = reinterpret_cast<unsigned short*>(s_word + A.cap);
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, cap = A.cap;
    float th;
    if (!tb_radius(A, j, th)) return;
    if (pairBad[j]) { if (tid == 0) nmatches[j] = -1; return; }
    const TbPair P = tb_pair(A, j, th);
    for (int i = tid; i < cap; i += 256) { s_word[i] = 0; s_last[i] = 0xffff; }
    if (tid == 0) { s_n = 0; s_reject = 0; }
    __syncthreads();
    if (tid < 64) {
        int n = 0, myHist = 0;                                       // lane b counts the events of rotation bin b
        int* m12 = match12 ? match12 + (size_t)j * cap : nullptr;
        for (int c0 = 0; c0 < P.nL; c0 += 64) {
            const int i = c0 + lane;
            uint4 L = make_uint4(TB_NONE, TB_NONE, TB_NONE, TB_NONE);
            if (i < P.nL) L = lists[(size_t)j * cap + i];
            unsigned long long todo = wave_vote((L.x & TB_NONE) != TB_NONE);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const unsigned x = (unsigned)__shfl((int)L.x, l, 64);
                const unsigned e[TB_K] = {x & TB_NONE, (unsigned)__shfl((int)L.y, l, 64), (unsigned)__shfl((int)L.z, l, 64), (unsigned)__shfl((int)L.w, l, 64)};
                unsigned hit = TB_NONE;
                bool exhausted = true;
                for (int k = 0; k < TB_K; ++k) {
                    if (e[k] == TB_NONE) { exhausted = false; break; }
                    if (!(s_word[e[k] & 0x1fffu] & TB_BLOCKED)) { hit = e[k]; exhausted = false; break; }
                }
                if (exhausted && (x & TB_MORE)) hit = tb_rescan(P, A, c0 + l, lane, s_word);
                if (hit != TB_NONE) {
                    // mvpMapPoints[bestIdx2] = pMP; match12.insert(...); nmatches++; rotHist[bin].push_back(bestIdx2)           (:1427-1445, :1574-1590)
                    const int i2 = (int)(hit & 0x1fffu), bin = (int)((hit >> 13) & 31u);
                    unsigned w = s_word[i2];
                    const bool first = !(w & TB_SEEN);
                    w |= TB_SEEN;
                    if (x & TB_OBS) w |= TB_BLOCKED;
                    if (checkOri) { w |= 1u << bin; if (lane == bin) ++myHist; }
                    s_word[i2] = w;                                  // (every lane stores the same word: the next query's read is ordered behind it)
                    s_last[i2] = (unsigned short)(c0 + l);
                    if (first && m12 && lane == 0) m12[i2] = c0 + l;
                    ++n;
                }
            }
        }
        if (lane < TB_HISTO) s_hist[lane] = myHist;
        if (lane == 0) s_n = n;
    }
    __syncthreads();
    if (checkOri) {
        if (tid == 0) {
            int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;      // ComputeThreeMaxima, src/ORBmatcher.cc:1749-1790
            for (int i = 0; i < TB_HISTO; i++) {
                const int s = s_hist[i];
                if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
                else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
                else if (s > max3) { max3 = s; ind3 = i; }
            }
            if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
            else if (max3 < 0.1f * (float)max1) ind3 = -1;
            unsigned rej = 0;
            int n = s_n;
            for (int i = 0; i < TB_HISTO; i++) if (i != ind1 && i != ind2 && i != ind3) { rej |= 1u << i; n -= s_hist[i]; }
            s_reject = rej; s_n = n;
        }
        __syncthreads();
    }
    const unsigned rej = s_reject;
    for (int i2 = tid; i2 < cap; i2 += 256) {
        const unsigned w = s_word[i2];
        const bool keep = (w & TB_SEEN) && !(w & rej);
        matches[(size_t)j * cap + i2] = keep ? (int)s_last[i2] : -1;
        if (match12 && !keep) match12[(size_t)j * cap + i2] = -1;      // (a kept feature holds the index its first event stored)
    }
    if (tid == 0) nmatches[j] = s_n;
}

// cv::Mat Frame::UnprojectStereo(const int &i), src/Frame.cc:1073-1087: mRwc * x3Dc + mOw under C.12, (0, 0, 0) where the reference returns cv::Mat()
__global__ __launch_bounds__(256) void k_unproject_stereo(const olf_keypoint* __restrict__ kps, const int* __restrict__ counts, const float* __restrict__ depth,
                                                         int cap, int img_stride, float cx, float cy, float invfx, float invfy,
                                                         const float* __restrict__ Twc, float* __restrict__ world)
{
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const size_t at = (size_t)f * cap + i;
    float o[3] = {0.f, 0.f, 0.f};
    const int n = min(max(counts[(size_t)f * img_stride], 0), cap);
    const float z = i < n ? depth[at] : 0.f;
    if (z > 0) {
        const olf_keypoint& kp = kps[(size_t)f * img_stride * cap + i];
        const float u = kp.x, v = kp.y;
        const float x3Dc[3] = {(u - cx) * z * invfx, (v - cy) * z * invfy, z};
        const float* T = Twc + 16 * (size_t)f;
        for (int r = 0; r < 3; ++r) {
            const float t = T[4 * r] * x3Dc[0] + T[4 * r + 1] * x3Dc[1] + T[4 * r + 2] * x3Dc[2];
            o[r] = (float)((double)t + (double)1.0f * (double)T[4 * r + 3]);
        }
    }
    world[3 * at] = o[0]; world[3 * at + 1] = o[1]; world[3 * at + 2] = o[2];
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_search_by_projection_batch_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, float th, const float* d_th, int bMono, int check_orientation,
                                       int32_t* d_matches, int32_t* d_match12, int32_t* d_nmatches, void* stream)
{
    if (!c || !in || n_frames < 0 || !d_matches || !d_nmatches || !in->kps || !in->desc || !in->counts || in->img_stride < 1 || !in->uright ||
        !in->cell_offsets || !in->cell_index || !in->Tcw || !in->mp_world || !(in->maxX > in->minX) || !(in->maxY > in->minY)) {
        set_error("olf_search_by_projection_batch_dev: bad argument"); return OLF_ERR_INVALID;
    }
    const int rcd = ctx_check_device(c, "olf_search_by_projection_batch_dev");
    if (rcd != OLF_OK) return rcd;
    const int cap = olf_orb_capacity(c);
    if (cap > OLF_GRID_MAX_KEYS) {
        set_error("olf_search_by_projection_batch_dev: more than OLF_GRID_MAX_KEYS key points per frame (a list entry holds 13 index bits)"); return OLF_ERR_CAPACITY;
    }
    if (n_frames < 2) return OLF_OK;
    const int n_pairs = n_frames - 1;
    TrackArgs A;
    A.in = *in;
    A.cap = cap; A.bMono = bMono ? 1 : 0; A.th = th; A.d_th = d_th;
    // mfGridElementWidthInv / mfGridElementHeightInv, src/Frame.cc:186-187
    A.wInv = static_cast<float>(OLF_GRID_COLS) / (in->maxX - in->minX);
    A.hInv = static_cast<float>(OLF_GRID_ROWS) / (in->maxY - in->minY);
    for (int l = 0; l < OLF_MAX_LEVELS; ++l) A.sf[l] = 1.f;
    A.nlevels = std::min(ctx_orb_levels(c), (int)OLF_MAX_LEVELS);
    olf_orb_scale_tables(c, A.sf, nullptr, nullptr, nullptr, nullptr);
    void* st = nullptr;
    const size_t bl = (size_t)n_pairs * cap * sizeof(uint4);
    const int rc = ctx_scratch(c, 2, bl + (size_t)n_pairs * 4 + 64, &st);
    if (rc != OLF_OK) return rc;
    uint4* lists = (uint4*)st;
    int* pairBad = (int*)((uint8_t*)st + bl);
    hipStream_t s = stream ? (hipStream_t)stream : ctx_stream(c);
    OLF_HIP_CHECK(hipMemsetAsync(pairBad, 0, (size_t)n_pairs * 4, s));
    hipLaunchKernelGGL(k_track_lists, dim3((cap + 3) / 4, n_pairs), dim3(256), 0, s, A, lists, pairBad, ctx_status(c));
    const size_t lds = (size_t)cap * 4 + (((size_t)cap * 2 + 3) & ~(size_t)3);
    hipLaunchKernelGGL(k_track_walk, dim3(n_pairs), dim3(256), lds, s, A, lists, pairBad, check_orientation ? 1 : 0, d_matches, d_match12, d_nmatches);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_unproject_stereo_dev(olf_ctx* c, int n_frames, int img_stride, const olf_keypoint* d_kps, const int32_t* d_counts, const float* d_depth, float fx,
                             float fy, float cx, float cy, const float* d_Twc, float* d_world, void* stream)
{
    if (!c || n_frames < 0 || img_stride < 1 || !d_kps || !d_counts || !d_depth || !d_Twc || !d_world) {
        set_error("olf_unproject_stereo_dev: bad argument"); return OLF_ERR_INVALID;
    }
    const int rcd = ctx_check_device(c, "olf_unproject_stereo_dev");
    if (rcd != OLF_OK) return rcd;
    if (n_frames == 0) return OLF_OK;
    const int cap = olf_orb_capacity(c);
    const float invfx = 1.0f / fx, invfy = 1.0f / fy;             // src/Frame.cc:188-189
    hipLaunchKernelGGL(k_unproject_stereo, dim3((cap + 255) / 256, n_frames), dim3(256), 0, stream ? (hipStream_t)stream : ctx_stream(c), d_kps, d_counts,
                       d_depth, cap, img_stride, cx, cy, invfx, invfy, d_Twc, d_world);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
