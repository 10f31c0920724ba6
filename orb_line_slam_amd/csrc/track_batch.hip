// track_batch.hip -- ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono[, map<int,int>& match12])
// (src/ORBmatcher.cc:1330-1472, :1474-1618; Tracking::TrackWithMotionModel[WithLine], src/Tracking.cc:1296,1302) for a whole batch of consecutive frames on
// the device, and Frame::UnprojectStereo (src/Frame.cc:1073-1087) for every feature of a batch.  The arithmetic is that of search_host.cpp
// (search_by_projection_frames), and where it is a cv::Mat product (convention C.12) or the rotation histogram it is the same text: search_math.hpp.
// No contraction (-ffp-contract=off).
//
// Only one thing in the reference's loop depends on the order of the last frame's features: a CurrentFrame feature is skipped while the map point it received
// last has observations (:1405-1407).  Everything else -- projection, image gates, the grid walk, level gates, the window tests, the mvuRight gate, the
// distance -- is a function of (pair, last feature) alone, and a query's outcome is "the first entry, in (distance, scan position) order, with distance <=
// TH_HIGH, whose feature is not blocked".  So:
//   k_track_lists   one wave per (pair, last feature): walks the window (grid_walk, grid_walk.hpp) and keeps the TB_K best entries (Best4) with distance <= TH_HIGH
//                   (16 bytes per query, whatever the window holds), plus "there were more" and the point's Observations() bit
//   k_track_walk    one workgroup per pair: one wave walks the lists in index order against the pair's blocked bits in LDS; a query whose kept entries
//                   are all blocked although the window held more is recomputed on the spot by the whole wave, with the blocked test inside the scan -- so
//                   there is no capacity to exceed; then the rotation histogram (ComputeThreeMaxima, :1749-1790) and the output rows
//   k_unproject_stereo  Frame::UnprojectStereo, one thread per feature
#include <algorithm>
#include "batch_frames.hpp"
#include "device_math.hpp"
#include "staging.hpp"

namespace olf {

constexpr int TB_TH_HIGH = 100;                     // src/ORBmatcher.cc:39
constexpr int TB_K = 4;                             // entries kept per query (one uint4)
// a list entry: distance << 18 | rotation bin << 13 | CurrentFrame feature (< OLF_GRID_MAX_KEYS = 2^13); the first word of a list also carries two flags
constexpr unsigned TB_NONE = Best4::NONE, TB_OBS = 1u << 30, TB_MORE = 1u << 31;
// per CurrentFrame feature in the walk: bit b = an event of rotation bin b landed here, then
constexpr unsigned TB_SEEN = 1u << 30, TB_BLOCKED = 1u << 31;
constexpr int TB_NOKEY = Best4::NOKEY;
static_assert(OLF_GRID_MAX_KEYS <= (1 << 13) && HISTO_LENGTH <= 30 && TB_K == Best4::K, "entry and word layouts");

struct TrackArgs : FrameView {
    int bMono;
    float th;
    const float* d_th;
};

struct TbPair {
    const olf_keypoint *kL, *kC;
    const uint4 *dL, *dC;
    const float *urC, *TcwC, *world;
    const uint8_t *valid, *obs, *outl;
    int nL;
    bool fwd, bwd;
    float th;
};

struct TbQuery {
    float u, v, invzc, radius;
    int minLevel, maxLevel;
    int state;                     // 0: no window, 1: search it, 2: octave outside the levels
};

__device__ __forceinline__ TbPair tb_pair(const TrackArgs& A, int j, float th)
{
    const olf_track_batch& in = A.in;
    const size_t cap = (size_t)A.cap, fL = (size_t)j, fC = (size_t)j + 1;
    TbPair P;
    P.kL = A.keys(j); P.kC = A.keys(j + 1);
    P.dL = A.point_desc(j, 0);
    P.dC = A.desc(j + 1);
    P.urC = A.uright(j + 1);
    P.TcwC = in.Tcw + 16 * fC;
    P.world = in.mp_world + 3 * fL * cap;
    P.valid = in.mp_valid ? in.mp_valid + fL * cap : nullptr;
    P.obs = in.mp_obs ? in.mp_obs + fL * cap : nullptr;
    P.outl = in.outlier ? in.outlier + fL * cap : nullptr;
    P.nL = A.count(j);
    P.th = th;
    // twc = -Rcw.t() * tcw;  tlc = Rlw * twc + tlw                                   (:1341-1349)
    float twc[3], tlc[3];
    camera_centre(P.TcwC, twc);
    rot_apply(in.Tcw + 16 * fL, twc, 1.0f, tlc);
    const float mb = in.mbf / in.fx;
    P.fwd = tlc[2] > mb && !A.bMono;
    P.bwd = -tlc[2] > mb && !A.bMono;
    return P;
}

// the gates of one last-frame feature up to its window (:1369-1400)
__device__ __forceinline__ TbQuery tb_query(const TbPair& P, const TrackArgs& A, int i)
{
    TbQuery q;
    q.state = 0; q.u = q.v = q.invzc = q.radius = 0.f; q.minLevel = q.maxLevel = -1;
    if (P.valid && !P.valid[i]) return q;
    if (P.outl && P.outl[i]) return q;
    float x3Dc[3];
    rot_apply(P.TcwC, P.world + 3 * (size_t)i, 1.0f, x3Dc);
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
    const int dist = ham256(a0, a1, P.dC[2 * (size_t)j], P.dC[2 * (size_t)j + 1]);
    if (dist > TB_TH_HIGH) return false;
    int bin = rot_bin(angL, P.kC[j].angle);                                     // (:1434-1441)
    bin = min(max(bin, 0), HISTO_LENGTH - 1);      // (angles outside [0, 360) index past rotHist in the reference; here they land in an end bin)
    key = (dist << 16) | pos;
    ent = ((unsigned)dist << 18) | ((unsigned)bin << 13) | (unsigned)j;
    return true;
}

__global__ __launch_bounds__(256) void k_track_lists(TrackArgs A, uint4* __restrict__ lists, int* __restrict__ pairBad, int* __restrict__ status)
{
    const int j = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    float th;
    if (!item_radius(A.th, A.d_th, j, th)) return;
    const TbPair P = tb_pair(A, j, th);
    if (i >= P.nL) return;                                       // (wave-uniform)
    const TbQuery q = tb_query(P, A, i);
    unsigned out[TB_K] = {TB_NONE, TB_NONE, TB_NONE, TB_NONE};
    int cnt = 0;
    if (q.state == 2) {
        if (lane == 0) { atomicOr(status, STATUS_OCTAVE); pairBad[j] = 1; }
    } else if (q.state == 1) {
        const uint4 a0 = P.dL[2 * (size_t)i], a1 = P.dL[2 * (size_t)i + 1];
        const float angL = P.kL[i].angle;
        Best4 best;
        grid_walk(A.grid(j + 1), q.u, q.v, q.radius, q.minLevel, q.maxLevel, lane, [&](bool take, int j2, int pos) {
            int key = TB_NOKEY;
            unsigned ent = TB_NONE;
            const bool ok = take && tb_candidate(P, A, q, a0, a1, angL, j2, pos, key, ent);
            cnt += __popcll(wave_vote(ok));
            best.push(ok, key, ent);
        });
        best.drain(out);
    }
    if (lane == 0) {
        unsigned x = out[0];
        if (cnt > TB_K) x |= TB_MORE;
        if (!P.obs || P.obs[i]) x |= TB_OBS;
        lists[(size_t)j * A.cap + i] = make_uint4(x, out[1], out[2], out[3]);
    }
}

// the query of last-frame feature i of pair j again, with the blocked test inside the scan: the entry the reference would choose now, or TB_NONE
__device__ __forceinline__ unsigned tb_rescan(const TbPair& P, const TrackArgs& A, int j, int i, int lane, const unsigned* s_word)
{
    const TbQuery q = tb_query(P, A, i);
    if (q.state != 1) return TB_NONE;
    const uint4 a0 = P.dL[2 * (size_t)i], a1 = P.dL[2 * (size_t)i + 1];
    const float angL = P.kL[i].angle;
    return window_best(A.grid(j + 1), q.u, q.v, q.radius, q.minLevel, q.maxLevel, lane, [&](int j2, int pos, int& key, unsigned& ent) {
        return !(s_word[j2] & TB_BLOCKED) && tb_candidate(P, A, q, a0, a1, angL, j2, pos, key, ent);
    });
}

// One workgroup per pair; dynamic LDS: cap words, then cap uint16 (the last frame's index a feature holds).
__global__ __launch_bounds__(256) void k_track_walk(TrackArgs A, const uint4* __restrict__ lists, const int* __restrict__ pairBad, int checkOri,
                                                    int* __restrict__ matches, int* __restrict__ match12, int* __restrict__ nmatches)
{
    extern __shared__ unsigned s_word[];
    __shared__ int s_hist[HISTO_LENGTH], s_n;
    __shared__ unsigned s_reject;
    unsigned short* s_last = reinterpret_cast<unsigned short*>(s_word + A.cap);
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, cap = A.cap;
    float th;
    if (!item_radius(A.th, A.d_th, j, th)) return;
    if (pairBad[j]) { if (tid == 0) nmatches[j] = -1; return; }
    const TbPair P = tb_pair(A, j, th);
    for (int i = tid; i < cap; i += 256) { s_word[i] = 0; s_last[i] = 0xffff; }
    if (tid == 0) { s_n = 0; s_reject = 0; }
    __syncthreads();
    if (tid < 64) {
        int n = 0, myHist = 0;                                       // lane b counts the events of rotation bin b
        int* m12 = match12 ? match12 + (size_t)j * cap : nullptr;
        walk_lists(lists + (size_t)j * cap, 0, P.nL, lane, [](int, bool) {}, [&](int i, int, unsigned x, const unsigned (&e)[TB_K]) {
            bool exhausted;
            unsigned hit = first_open(e, exhausted, [&](unsigned f) { return !(s_word[f] & TB_BLOCKED); });
            if (exhausted && (x & TB_MORE)) hit = tb_rescan(P, A, j, i, lane, s_word);
            if (hit == TB_NONE) return;
            // mvpMapPoints[bestIdx2] = pMP; match12.insert(...); nmatches++; rotHist[bin].push_back(bestIdx2)           (:1427-1445, :1574-1590)
            const int i2 = (int)(hit & 0x1fffu), bin = (int)((hit >> 13) & 31u);
            unsigned w = s_word[i2];
            const bool first = !(w & TB_SEEN);
            w |= TB_SEEN;
            if (x & TB_OBS) w |= TB_BLOCKED;
            if (checkOri) { w |= 1u << bin; if (lane == bin) ++myHist; }
            s_word[i2] = w;                                          // (every lane stores the same word: the next query's read is ordered behind it)
            s_last[i2] = (unsigned short)i;
            if (first && m12 && lane == 0) m12[i2] = i;
            ++n;
        });
        if (lane < HISTO_LENGTH) s_hist[lane] = myHist;
        if (lane == 0) s_n = n;
    }
    __syncthreads();
    if (checkOri) {
        if (tid == 0) { int n = s_n; s_reject = histo_reject(s_hist, n); s_n = n; }
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
    const int n = frame_count(f, counts, img_stride, cap);
    const float z = i < n ? depth[at] : 0.f;
    if (z > 0) {
        const olf_keypoint& kp = kps[(size_t)f * img_stride * cap + i];
        unproject_stereo_point(kp.x, kp.y, z, cx, cy, invfx, invfy, Twc + 16 * (size_t)f, o);
    }
    world[3 * at] = o[0]; world[3 * at + 1] = o[1]; world[3 * at + 2] = o[2];
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_search_by_projection_batch_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, float th, const float* d_th, int bMono, int check_orientation,
                                       int32_t* d_matches, int32_t* d_match12, int32_t* d_nmatches, void* stream)
{
    TrackArgs A;
    OLF_TRY(batch_frames(c, "olf_search_by_projection_batch_dev", d_matches && d_nmatches, in, NEED_GRID | NEED_URIGHT | NEED_TCW | NEED_WORLD, n_frames, nullptr, 0,
                         0, "", A, nullptr));
    if (n_frames < 2) return OLF_OK;
    const int n_pairs = n_frames - 1, cap = A.cap;
    A.bMono = bMono ? 1 : 0; A.th = th; A.d_th = d_th;
    uint4* lists; int* pairBad;
    Carve k;
    k.add(&lists, (size_t)n_pairs * cap); k.add(&pairBad, n_pairs);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    hipStream_t s = ctx_stream(c, stream);
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
    OLF_TRY(ctx_check_device(c, "olf_unproject_stereo_dev"));
    if (n_frames == 0) return OLF_OK;
    const int cap = olf_orb_capacity(c);
    const float invfx = 1.0f / fx, invfy = 1.0f / fy;             // src/Frame.cc:188-189
    hipLaunchKernelGGL(k_unproject_stereo, dim3((cap + 255) / 256, n_frames), dim3(256), 0, ctx_stream(c, stream), d_kps, d_counts,
                       d_depth, cap, img_stride, cx, cy, invfx, invfy, d_Twc, d_world);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
