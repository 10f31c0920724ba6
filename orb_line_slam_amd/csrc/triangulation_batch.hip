// triangulation_batch.hip -- ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs,
// const bool bOnlyStereo, const cv::Mat Cw) (src/ORBmatcher.cc:659-825; LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:268) for a list of key-frame
// pairs of a device-resident batch.  The FeatureVectors come from the stage bow_match.hip shares (launch_bow_feature_vectors), once per frame and call;
// the candidate gate is the text olf_search_for_triangulation runs (search_math.hpp).  No contraction (-ffp-contract=off).
//
// The reference declares vbMatched2 and never sets it, so nothing a query does is seen by another: a key-frame-1 feature's match is, among the key-frame-2
// features of its vocabulary node that hold no map point, pass bOnlyStereo, lie within TH_LOW and pass the epipole and epipolar-line gates, the one with the
// smallest distance -- the LAST in list order on a tie (`dist > bestDist -> continue`, :740).  That is one minimum over (distance << 16 | 0xffff - position).
//   k_search_for_triangulation   one workgroup per pair.  Its waves claim the nodes of key frame 1's list one at a time (the compare-and-swap head of
//                                k_search_by_bow).  The lanes of a wave hold 64 of the node's key-frame-2 features -- descriptor, position, scale factor, the
//                                two per-feature flags -- and the node's key-frame-1 features stream past them as wave-uniform values: one wave_min_i32 per
//                                query and chunk.  A node's segment longer than a wave is walked in chunks, chunk outside, query inside, so the lanes are loaded
//                                once; the minima of the chunks meet in the query's LDS word, and a later chunk's positions are larger, so the tie rule holds
//                                across chunks.  Then the rotation histogram in integer counters, ComputeThreeMaxima, and the row.
#include "batch_frames.hpp"
#include "device_math.hpp"

namespace olf {

constexpr int TRI_TH_LOW = 50;                      // src/ORBmatcher.cc:40
constexpr int TRI_WAVES = 4;
constexpr int TRI_NOKEY = 0x7fffffff;

struct TriArgs : FrameView {       // (no grid is read: capW, wInv, hInv and thr stay zero)
    int n_frames, onlyStereo, checkOri;
    const int* pairs;
    const float* F12;
    const float* Cw;
};

// dynamic LDS: cap words (a query's best key, then its match), then one rotation bin byte per key-frame-1 feature
__global__ __launch_bounds__(64 * TRI_WAVES) void k_search_for_triangulation(TriArgs A, const unsigned long long* __restrict__ sortedAll, const int* __restrict__ mAll,
                                                                             int* __restrict__ status, int* __restrict__ matches12, int* __restrict__ nmatches)
{
    extern __shared__ int s_key[];
    __shared__ int s_hist[HISTO_LENGTH], s_seg, s_n, s_bad, s_keep[3];
    __shared__ float s_epi[2];
    const int cap = A.cap, p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    uint8_t* binOf = reinterpret_cast<uint8_t*>(s_key + cap);
    const int f1 = A.pairs[2 * (size_t)p], f2 = A.pairs[2 * (size_t)p + 1];
    if (!pair_in_batch(f1, f2, A.n_frames)) {                        // (block-uniform)
        if (tid == 0) { nmatches[p] = -1; atomicOr(status, STATUS_PAIR); }
        return;
    }
    const olf_track_batch& in = A.in;
    const unsigned long long* SK = sortedAll + (size_t)f1 * cap;
    const unsigned long long* SF = sortedAll + (size_t)f2 * cap;
    // mp_valid == NULL: every feature holds a map point, nothing is searched
    const int mK = in.mp_valid ? mAll[f1] : 0, mF = mAll[f2];
    const int N1 = A.count(f1);
    const olf_keypoint *k1 = A.keys(f1), *k2 = A.keys(f2);
    const uint4 *d1 = A.desc(f1), *d2 = A.desc(f2);
    const float *u1 = A.uright(f1), *u2 = A.uright(f2);
    const uint8_t* v1 = in.mp_valid + (size_t)f1 * cap;      // (read only when mK > 0)
    const uint8_t* v2 = in.mp_valid + (size_t)f2 * cap;
    const float* F12 = A.F12 + 9 * (size_t)p;
    for (int i = tid; i < cap; i += 64 * TRI_WAVES) { s_key[i] = TRI_NOKEY; binOf[i] = 0; }
    if (tid < HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) {
        s_seg = 0; s_n = 0; s_bad = 0;
        // Compute epipole in second image (:666-676), once per pair
        float cw[3], ex, ey;
        if (A.Cw) { cw[0] = A.Cw[3 * (size_t)p]; cw[1] = A.Cw[3 * (size_t)p + 1]; cw[2] = A.Cw[3 * (size_t)p + 2]; }
        else camera_centre(in.Tcw + 16 * (size_t)f1, cw);
        tri_epipole(in.Tcw + 16 * (size_t)f2, cw, in.fx, in.fy, in.cx, in.cy, ex, ey);
        s_epi[0] = ex; s_epi[1] = ey;
    }
    __syncthreads();
    const float ex = s_epi[0], ey = s_epi[1];
    for (;;) {
        int kb = 0, ke = 0;
        if (lane == 0) {
            // claim [kb, ke), one node of key frame 1's list: compare-and-swap so that exactly one wave advances the head from kb to ke
            for (;;) {
                kb = atomicAdd(&s_seg, 0);
                if (kb >= mK) { ke = kb; break; }
                const unsigned long long node = SK[kb] >> 16;
                ke = bm_lower_bound(SK, mK, (node + 1) << 16);
                if (atomicCAS(&s_seg, kb, ke) == kb) break;
            }
        }
        kb = __builtin_amdgcn_readfirstlane(kb); ke = __builtin_amdgcn_readfirstlane(ke);
        if (kb >= mK) break;
        const unsigned long long node = SK[kb] >> 16;
        const int fb = bm_lower_bound(SF, mF, node << 16), fe = bm_lower_bound(SF, mF, (node + 1) << 16);
        for (int c0 = fb; c0 < fe; c0 += 64) {
            // this lane's key-frame-2 feature and everything about it that no query changes
            const int pos = c0 + lane;
            const bool on = pos < fe;
            const int idx2 = on ? (int)(SF[pos] & 0xffffu) : 0;
            const bool stereo2 = u2[idx2] >= 0;
            // If we have already matched or there is a MapPoint skip; if(bOnlyStereo) if(!bStereo2) continue (:723-735)
            const bool cand = on && !v2[idx2] && !(A.onlyStereo && !stereo2);
            const olf_keypoint kp2 = k2[idx2];
            const bool badOct = cand && (kp2.octave < 0 || kp2.octave >= A.nlevels);
            const float sf2 = A.sf[min(max(kp2.octave, 0), OLF_MAX_LEVELS - 1)];
            const uint4 x0 = d2[2 * (size_t)idx2], x1 = d2[2 * (size_t)idx2 + 1];
            const bool anyBadOct = wave_vote(badOct) != 0;
            for (int q = kb; q < ke; ++q) {
                const int idx1 = (int)(SK[q] & 0xffffu);                     // (wave-uniform from here to the reduction)
                // If there is already a MapPoint skip (:700-704); if(bOnlyStereo) if(!bStereo1) continue (:706-710)
                if (v1[idx1]) continue;
                const bool stereo1 = u1[idx1] >= 0;
                if (A.onlyStereo && !stereo1) continue;
                if (anyBadOct) { if (lane == 0) s_bad = 1; break; }
                const uint4 a0 = d1[2 * (size_t)idx1], a1 = d1[2 * (size_t)idx1 + 1];
                float l[3];
                tri_epiline(F12, k1[idx1].x, k1[idx1].y, l);
                const int dist = ham256(a0, a1, x0, x1);
                bool ok = cand && dist <= TRI_TH_LOW;
                if (ok && !stereo1 && !stereo2 && tri_near_epipole(ex, ey, kp2.x, kp2.y, sf2)) ok = false;
                if (ok && !tri_epiline_ok(l, kp2.x, kp2.y, sf2)) ok = false;
                const int m = wave_min_i32(ok ? (dist << 16) | (0xffff - pos) : TRI_NOKEY);
                if (lane == 0 && m < s_key[idx1]) s_key[idx1] = m;           // (a feature sits in one node: this wave alone touches its word)
            }
        }
    }
    __syncthreads();
    if (s_bad) {
        if (tid == 0) { nmatches[p] = -1; atomicOr(status, STATUS_OCTAVE); }
        return;
    }
    // a key becomes its match: matches12[idx1] = bestIdx2, and the rotation bin (:767-786)
    int found = 0;
    for (int i = tid; i < cap; i += 64 * TRI_WAVES) {
        const int key = s_key[i];
        int m = -1;
        if (i < N1 && key != TRI_NOKEY) {
            m = (int)(SF[0xffff - (key & 0xffff)] & 0xffffu);
            if (A.checkOri) {
                int bin = rot_bin(k1[i].angle, k2[m].angle);
                bin = min(max(bin, 0), HISTO_LENGTH - 1);      // (angles outside [0, 360) index past rotHist in the reference; here they land in an end bin)
                binOf[i] = (uint8_t)bin;
                atomicAdd(&s_hist[bin], 1);
            }
            ++found;
        }
        s_key[i] = m;
    }
    if (found) atomicAdd(&s_n, found);
    __syncthreads();
    if (A.checkOri) {
        if (tid == 0) {
            int ind1, ind2, ind3;
            three_maxima(s_hist, ind1, ind2, ind3);
            s_keep[0] = ind1; s_keep[1] = ind2; s_keep[2] = ind3;
        }
        __syncthreads();
        int dropped = 0;
        for (int i = tid; i < N1; i += 64 * TRI_WAVES)
            if (s_key[i] >= 0) { const int b = binOf[i]; if (b != s_keep[0] && b != s_keep[1] && b != s_keep[2]) { s_key[i] = -1; ++dropped; } }
        if (dropped) atomicSub(&s_n, dropped);
        __syncthreads();
    }
    for (int i = tid; i < cap; i += 64 * TRI_WAVES) matches12[(size_t)p * cap + i] = s_key[i];
    if (tid == 0) nmatches[p] = s_n;
}

int launch_search_for_triangulation_batch(const olf_track_batch& in, int n_frames, int cap, const float* sf, int nlevels, int n_pairs, const int* d_pairs,
                                          const float* d_F12, const float* d_Cw, int only_stereo, int check_ori, const unsigned long long* d_sorted,
                                          const int* d_m, int* d_status, int* d_matches12, int* d_nmatches, hipStream_t s)
{
    TriArgs A = {};
    A.in = in;
    A.cap = cap; A.nlevels = nlevels; A.n_frames = n_frames; A.onlyStereo = only_stereo; A.checkOri = check_ori;
    A.pairs = d_pairs; A.F12 = d_F12; A.Cw = d_Cw;
    for (int l = 0; l < OLF_MAX_LEVELS; ++l) A.sf[l] = sf[l];
    hipLaunchKernelGGL(k_search_for_triangulation, dim3(n_pairs), dim3(64 * TRI_WAVES), (size_t)cap * 4 + ((cap + 3) & ~3), s, A, d_sorted, d_m, d_status,
                       d_matches12, d_nmatches);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // namespace olf
