// grid_walk.hpp -- what the device callers of Frame::mGrid share: Frame::GetFeaturesInArea (src/Frame.cc:517-570) by one wave (grid.hip's k_features_in_area and
// the batched matchers), the wave's smallest key with its owner's payload, the four best entries of a window (Best4), a window's best entry under a
// caller's test (window_best), and the matchers' per-item radius.  The matchers' sort keys carry the scan position this walk hands out, so their results rest
// on every caller running this one text.
#pragma once
#include "olf_internal.hpp"

namespace olf {

// one frame's grid (layout: include/orbline_types.h, "Frame::mGrid as two arrays")
struct GridView {
    const olf_keypoint* keys;
    const int *cell_offsets, *cell_index;
    int n;                       // key points of the frame: an index outside [0, n) is left out
    int limit;                   // entries of cell_index: the offsets are clamped into [0, limit]
    float minX, minY, wInv, hInv;
};

// GetFeaturesInArea(x, y, r, minLevel, maxLevel) by one wave.  The cells (ix, nMinCellY .. nMaxCellY) of a column are one range of cell_index: it is read 64
// entries at a time, and f(take, j, pos) is called by every lane for every such chunk; `take` lanes hold feature j, the pos-th index the reference's vIndices
// would hold (ix outer, iy inner, stored order inside a cell: vote + rank keep the order).  Returns how many indices that is.
// n and limit keep a malformed grid from being read outside its arrays; a caller that knows neither passes INT_MAX for both, which never binds on a well-formed
// grid -- a negative offset or index is then still clamped or left out.
template <class F>
__device__ __forceinline__ int grid_walk(const GridView& G, float x, float y, float r, int minLevel, int maxLevel, int lane, F&& f)
{
    constexpr int kCols = OLF_GRID_COLS, kRows = OLF_GRID_ROWS;
    // max(0,(int)floor(v)) then ">= COLS -> return", min(COLS-1,(int)ceil(v)) then "< 0 -> return": decided on the float so that no value outside int's
    // range is ever converted (a NaN takes the early return)
    const float fx0 = floorf((x - G.minX - r) * G.wInv), fx1 = ceilf((x - G.minX + r) * G.wInv);
    const float fy0 = floorf((y - G.minY - r) * G.hInv), fy1 = ceilf((y - G.minY + r) * G.hInv);
    if (!(fx0 < (float)kCols) || !(fx1 >= 0.f) || !(fy0 < (float)kRows) || !(fy1 >= 0.f)) return 0;
    const int nMinCellX = fx0 < 0.f ? 0 : (int)fx0, nMaxCellX = fx1 > (float)(kCols - 1) ? kCols - 1 : (int)fx1;
    const int nMinCellY = fy0 < 0.f ? 0 : (int)fy0, nMaxCellY = fy1 > (float)(kRows - 1) ? kRows - 1 : (int)fy1;
    if (nMinCellY > nMaxCellY) return 0;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    int total = 0;
    for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
        const int p0 = max(G.cell_offsets[ix * kRows + nMinCellY], 0), p1 = min(G.cell_offsets[ix * kRows + nMaxCellY + 1], G.limit);
        for (int pb = p0; pb < p1; pb += 64) {
            const int p = pb + lane;
            bool take = false;
            int j = 0;
            if (p < p1) {
                j = G.cell_index[p];
                if ((unsigned)j < (unsigned)G.n) {
                    const olf_keypoint& kp = G.keys[j];
                    const int octave = kp.octave;                   // (read beside x and y whether or not the levels are checked: one trip to memory, not two)
                    const float distx = kp.x - x, disty = kp.y - y;
                    take = true;
                    if (bCheckLevels) {
                        if (octave < minLevel) take = false;
                        if (maxLevel >= 0 && octave > maxLevel) take = false;
                    }
                    if (!(fabsf(distx) < r && fabsf(disty) < r)) take = false;
                }
            }
            const unsigned long long m = wave_vote(take);
            f(take, j, total + wave_rank_below(m));
            total += __popcll(m);
        }
    }
    return total;
}

// The wave's smallest key m and, where m < below, the payload of the lane that holds it (both wave-uniform); false: no key lies below `below`.  The keys below
// Best4::NOKEY are distinct (a matcher's key ends in the scan position), so such a minimum has one owner lane.  Every lane of the wave calls it.
template <class T>
__device__ __forceinline__ bool wave_min_fetch(int key, T payload, int below, int& m, T& out)
{
    m = wave_min_i32(key);
    if (m >= below) return false;
    const int owner = __ffsll((long long)wave_vote(key == m)) - 1;
    out = (T)__shfl((int)payload, owner, 64);
    return true;
}

// The four smallest (key, entry) pairs a wave meets.  Every lane keeps the four smallest keys pushed to it, ascending: one of the window's four smallest is
// one of its lane's four smallest, so the lanes' registers hold them all, and drain() takes them out by four wave minima.  The keys are distinct (a matcher's
// key ends in the scan position), so each minimum has one owner lane.
struct Best4 {
    static constexpr int K = 4;
    static constexpr int NOKEY = 0x7fffffff;            // above every key
    static constexpr unsigned NONE = 0x3fffffffu;       // the entry of an empty place: the 30 bits below a list word's two flags
    int h0 = NOKEY, h1 = NOKEY, h2 = NOKEY, h3 = NOKEY;
    unsigned e0 = NONE, e1 = NONE, e2 = NONE, e3 = NONE;

    __device__ __forceinline__ void push(bool ok, int key, unsigned ent)
    {
        if (ok && key < h3) {
            h3 = key; e3 = ent;
            if (h3 < h2) { const int t = h2; h2 = h3; h3 = t; const unsigned u = e2; e2 = e3; e3 = u; }
            if (h2 < h1) { const int t = h1; h1 = h2; h2 = t; const unsigned u = e1; e1 = e2; e2 = u; }
            if (h1 < h0) { const int t = h0; h0 = h1; h1 = t; const unsigned u = e0; e0 = e1; e1 = u; }
        }
    }
    // the wave's entries in key order into out[0 ..), wave-uniform; places beyond the number pushed are left as they are.  Every lane of the wave calls it.
    __device__ __forceinline__ void drain(unsigned (&out)[K])
    {
        for (int k = 0; k < K; ++k) {
            int m;
            if (!wave_min_fetch(h0, e0, NOKEY, m, out[k])) break;
            if (h0 == m) { h0 = h1; e0 = e1; h1 = h2; e1 = e2; h2 = h3; e2 = e3; h3 = NOKEY; e3 = NONE; }
        }
    }
};

// A window again by the whole wave, for the ordered walks' recompute path: the entry of the smallest key among the features that cand(j, pos, key, ent)
// accepts -- the caller's closed test is part of cand --, or Best4::NONE.  Wave-uniform.
template <class C>
__device__ __forceinline__ unsigned window_best(const GridView& G, float x, float y, float r, int minLevel, int maxLevel, int lane, C&& cand)
{
    int best = Best4::NOKEY;
    unsigned bestEnt = Best4::NONE;
    grid_walk(G, x, y, r, minLevel, maxLevel, lane, [&](bool take, int j, int pos) {
        int key = Best4::NOKEY, m;
        unsigned ent = Best4::NONE, e;
        if (!(take && cand(j, pos, key, ent))) key = Best4::NOKEY;
        // (later chunks hold later scan positions: a tie is impossible, `<` as in the reference)
        if (wave_min_fetch(key, ent, best, m, e)) { best = m; bestEnt = e; }
    });
    return bestEnt;
}

// the radius factor of item j of a batch (a pair, a frame): th, or d_th[j] where the caller gives one per item; false: the item is skipped (d_th[j] <= 0)
__device__ __forceinline__ bool item_radius(float th, const float* d_th, int j, float& out)
{
    out = th;
    if (!d_th) return true;
    out = d_th[j];
    return out > 0.f;
}

}  // namespace olf
