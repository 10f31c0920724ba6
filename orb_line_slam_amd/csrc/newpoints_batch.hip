// newpoints_batch.hip -- the entries that PRODUCE map arrays on the device: LocalMapping::ComputeF12 (src/LocalMapping.cc:536-553) and the body of
// LocalMapping::CreateNewMapPoints behind the search (:245-253, :286-431) for a list of key-frame pairs, and MapPoint::UpdateNormalAndDepth
// (src/MapPoint.cc:342-383) for a list of map points of one snapshot (olf_map_graph with an olf_cull_view beside it).  The arithmetic is
// newpoints_terms.hpp, the text the host forms (newpoints_host.cpp) run too.
//   k_create_new_map_points  one workgroup per pair, the row's matches compacted into LDS and one match per dense lane (see the kernel): bound by
//                   instruction issue, some thousand operations per match against 100 bytes read and 13 written
//   k_f12_pairs     one lane per pair: about 150 float and 60 double operations on 32 floats read and 9 written; a call is one launch of a few waves and
//                   costs its launch
//   k_normal_depth  ONE LANE PER POINT.  The normal is a float sum in row order (the reference's std::map iteration), so the observations of a point are
//                   taken sequentially by one lane: no atomics, no tree, the same bits wherever the point stands in the list.  Per observation a chain of
//                   dependent gathers (the observation, its key frame's row offsets, its camera centre) and one double square root and division: bound
//                   by the gathers' latency, hidden across the 64 independent points of a wave and the waves of a CU, not by bytes.
#include "newpoints_terms.hpp"
#include "batch_frames.hpp"
#include "map_kernels.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int NP_THREADS = 256;

struct F12Args {
    const float* Tcw;
    const int* pairs;
    float* F12;
    int n_frames, n_pairs;
    float cam[4];
};

constexpr int NP_SEG = 2048;                                         // idx1 slots compacted at a time: 8 KB of LDS

struct NewPointsArgs {
    const olf_keypoint* kps;
    const int *counts, *pairs, *matches12;
    const float *uright, *depth, *Tcw;
    float* x3D;
    uint8_t* code;
    int* nnew;
    int img_stride, cap, n_frames, nlevels, monocular;
    NewPointCam K;
    float sf[OLF_MAX_LEVELS];
};

__global__ __launch_bounds__(NP_THREADS) void k_f12_pairs(F12Args A, int* __restrict__ status)
{
    const int p = blockIdx.x * NP_THREADS + threadIdx.x;
    if (p >= A.n_pairs) return;
    const int f1 = A.pairs[2 * (size_t)p], f2 = A.pairs[2 * (size_t)p + 1];
    if (!pair_in_batch(f1, f2, A.n_frames)) { atomicOr(status, STATUS_PAIR); return; }
    float T1[12], T2[12], F[9];
    for (int k = 0; k < 12; ++k) { T1[k] = A.Tcw[16 * (size_t)f1 + k]; T2[k] = A.Tcw[16 * (size_t)f2 + k]; }
    f12_compute(T1, T2, A.cam, F);
    for (int k = 0; k < 9; ++k) A.F12[9 * (size_t)p + k] = F[k];
}

// One workgroup per pair.  A row of d_matches12 is sparse (a few hundred matches among a capacity of about 2000) and a match costs some thousand
// operations, most of them the Jacobi sweeps: a lane per idx1 slot would leave most lanes of every wave idle through them.  So the row is taken in segments
// of NP_SEG slots: the slots that hold a usable match are compacted into LDS in idx1 order (block_rank, map_kernels.hpp; DESIGN 4.5, "What the map-side
// kernels share"), then dense lanes take one match each and write code and x3D back to its idx1 slot.  A match's result depends on nothing but its own
// inputs and nnew is an integer sum, so nothing depends on scheduling or on where the pair stands.
__global__ __launch_bounds__(NP_THREADS) void k_create_new_map_points(NewPointsArgs A, int* __restrict__ status)
{
    __shared__ int s_list[NP_SEG];
    __shared__ int s_cnt[1][NP_THREADS / 64];
    __shared__ int s_new;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, cap = A.cap;
    const int f1 = A.pairs[2 * (size_t)p], f2 = A.pairs[2 * (size_t)p + 1];
    if (!pair_in_batch(f1, f2, A.n_frames)) {                        // (the whole workgroup: the pair is uniform)
        if (tid == 0) { atomicOr(status, STATUS_PAIR); A.nnew[p] = -1; }
        return;
    }
    KfPose P1, P2;
    kf_pose(A.Tcw + 16 * (size_t)f1, P1);
    kf_pose(A.Tcw + 16 * (size_t)f2, P2);
    const bool skip = !A.monocular && np_short_baseline(P1, P2, A.K.mb);      // :249-253
    const int N1 = skip ? 0 : frame_count(f1, A.counts, A.img_stride, cap), N2 = frame_count(f2, A.counts, A.img_stride, cap);
    const olf_keypoint* kp1 = A.kps + (size_t)f1 * A.img_stride * cap;
    const olf_keypoint* kp2 = A.kps + (size_t)f2 * A.img_stride * cap;
    const size_t row = (size_t)p * cap, r1 = (size_t)f1 * cap, r2 = (size_t)f2 * cap;
    if (tid == 0) s_new = 0;
    int created = 0;
    for (int seg0 = 0; seg0 < cap; seg0 += NP_SEG) {
        const int seg1 = min(seg0 + NP_SEG, cap);
        int n = 0;
        for (int base = seg0; base < seg1; base += NP_THREADS) {     // (uniform trip count)
            const int i = base + tid;
            bool live = false;
            if (i < seg1 && i < N1) {
                const int idx2 = A.matches12[row + i];
                if ((unsigned)idx2 < (unsigned)N2) {                 // an idx2 outside [0, N2) is no match
                    const bool levels = (unsigned)kp1[i].octave < (unsigned)A.nlevels && (unsigned)kp2[idx2].octave < (unsigned)A.nlevels;
                    if (!levels) atomicOr(status, STATUS_OCTAVE);
                    live = levels;
                }
            }
            if (i < seg1 && !live) { A.code[row + i] = 0; A.x3D[3 * (row + i)] = 0.f; A.x3D[3 * (row + i) + 1] = 0.f; A.x3D[3 * (row + i) + 2] = 0.f; }
            int step;
            const int at = n + block_rank<NP_THREADS / 64>(live, s_cnt, step);
            if (live) s_list[at] = i;                                // (at <= i - seg0 < NP_SEG)
            n += step;
            __syncthreads();
        }
        for (int q = tid; q < n; q += NP_THREADS) {
            const int i = s_list[q], idx2 = A.matches12[row + i];
            const olf_keypoint a = kp1[i], b = kp2[idx2];
            float x[3] = {0.f, 0.f, 0.f};
            const int code = np_create_point(P1, P2, A.K, a.x, a.y, A.uright[r1 + i], A.depth[r1 + i], A.sf[a.octave], b.x, b.y, A.uright[r2 + idx2],
                                             A.depth[r2 + idx2], A.sf[b.octave], x);
            const bool made = code >= NP_TRIANGULATED && code <= NP_UNPROJECT_2;
            A.code[row + i] = (uint8_t)code;
            A.x3D[3 * (row + i)] = made ? x[0] : 0.f; A.x3D[3 * (row + i) + 1] = made ? x[1] : 0.f; A.x3D[3 * (row + i) + 2] = made ? x[2] : 0.f;
            created += made;
        }
        __syncthreads();
    }
    created = wave_sum_i32(created);
    if (lane == 0) atomicAdd(&s_new, created);
    __syncthreads();
    if (tid == 0) A.nnew[p] = s_new;
}

__global__ __launch_bounds__(NP_THREADS) void k_normal_depth(NormalDepthView A, int n_points, const int* __restrict__ points, int* __restrict__ status)
{
    const int i = blockIdx.x * NP_THREADS + threadIdx.x;
    if (i >= n_points) return;
    normal_depth_point(A, points ? points[i] : i, status);
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_compute_f12_pairs_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* d_pairs, float* d_F12, void* stream)
{
    const char* who = "olf_compute_f12_pairs_dev";
    if (!c || !in || n_frames < 0 || n_pairs < 0 || (n_pairs && (!d_pairs || !d_F12)) || (n_pairs && n_frames && !in->Tcw)) {
        set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID;
    }
    OLF_TRY(ctx_check_device(c, who));
    if (n_pairs == 0) return OLF_OK;
    F12Args A;
    A.Tcw = in->Tcw; A.pairs = d_pairs; A.F12 = d_F12; A.n_frames = n_frames; A.n_pairs = n_pairs;
    A.cam[0] = in->fx; A.cam[1] = in->fy; A.cam[2] = in->cx; A.cam[3] = in->cy;
    hipLaunchKernelGGL(k_f12_pairs, dim3((n_pairs + NP_THREADS - 1) / NP_THREADS), dim3(NP_THREADS), 0, ctx_stream(c, stream), A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_create_new_map_points_batch_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const float* d_depth, float mb, int n_pairs, const int32_t* d_pairs,
                                        const int32_t* d_matches12, int monocular, float* d_x3D, uint8_t* d_code, int32_t* d_nnew, void* stream)
{
    const char* who = "olf_create_new_map_points_batch_dev";
    bool ok = c && in && n_frames >= 0 && n_pairs >= 0;
    ok = ok && (!n_pairs || (d_pairs && d_matches12 && d_x3D && d_code && d_nnew));
    ok = ok && (!n_pairs || !n_frames || (in->kps && in->counts && in->img_stride >= 1 && in->uright && in->Tcw && d_depth));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_pairs == 0) return OLF_OK;
    NewPointsArgs A;
    A.kps = in->kps; A.counts = in->counts; A.pairs = d_pairs; A.matches12 = d_matches12; A.uright = in->uright; A.depth = d_depth; A.Tcw = in->Tcw;
    A.x3D = d_x3D; A.code = d_code; A.nnew = d_nnew;
    A.img_stride = in->img_stride; A.cap = olf_orb_capacity(c); A.n_frames = n_frames; A.monocular = monocular ? 1 : 0;
    A.nlevels = ctx_level_scales(c, A.sf);
    A.K = new_point_cam(in->fx, in->fy, in->cx, in->cy, in->mbf, mb, A.sf[1]);
    hipLaunchKernelGGL(k_create_new_map_points, dim3(n_pairs), dim3(NP_THREADS), 0, ctx_stream(c, stream), A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_update_normal_and_depth_dev(olf_ctx* c,const olf_map_graph* g, const olf_cull_view* v, int n_points, const int32_t* d_points, const float* d_mp_world,
                                    const int32_t* d_mp_ref_kf, const float* d_kf_Ow, float* d_normal, float* d_maxd, float* d_mind, void* stream)
{
    const char* who = "olf_update_normal_and_depth_dev";
    bool ok = c && g && v && n_points >= 0 && g->n_kf >= 0 && g->n_mp >= 0 && g->mp_obs_offsets && g->kf_mp_offsets;
    ok = ok && ((g->mp_obs_kf && v->mp_obs_slot && g->mp_bad && d_mp_world && d_mp_ref_kf && d_normal && d_maxd && d_mind) || !g->n_mp);
    ok = ok && ((v->kf_slot_octave && d_kf_Ow) || !g->n_kf);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_points == 0) return OLF_OK;
    NormalDepthView A;
    A.n_kf = g->n_kf; A.n_mp = g->n_mp;
    A.n_levels = ctx_level_scales(c, A.sf);
    A.obs_off = g->mp_obs_offsets; A.obs_kf = g->mp_obs_kf; A.obs_slot = v->mp_obs_slot; A.kmp_off = g->kf_mp_offsets; A.ref_kf = d_mp_ref_kf;
    A.mp_bad = g->mp_bad; A.slot_octave = v->kf_slot_octave;
    A.world = d_mp_world; A.Ow = d_kf_Ow; A.normal = d_normal; A.maxd = d_maxd; A.mind = d_mind;
    hipLaunchKernelGGL(k_normal_depth, dim3((n_points + NP_THREADS - 1) / NP_THREADS), dim3(NP_THREADS), 0, ctx_stream(c, stream), A, n_points, d_points,
                       ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
