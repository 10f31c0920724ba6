// culling_batch.hip -- the data-parallel part of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:632-696) for a list of key frames against one snapshot of
// the map (olf_map_graph with an olf_cull_view beside it, include/orbline.h): every listed key frame as the map stands.  The sequential rest -- a culled key
// frame changes what the later ones of the list see -- is host code (culling_host.cpp).  With it: KeyFrame::TrackedMapPoints / TrackedMapLines
// (src/KeyFrame.cc:328-353, 407-432) for a list of key frames and LocalMapping::MapPointCulling (:170-205) as a per-point predicate.  Integers only, apart from
// nRed > 0.9 * nMPs in fp64 and found / visible in fp32 (f_div): exact.  Integer sums need no fixed order, so nothing here depends on convention C.16.
//   k_cull_rows    one workgroup: the listed rows' lengths into d_row_offsets, then their running sum; a total beyond slot_capacity raises STATUS_CONNECTIONS_LIST
//   k_cull_tables  one workgroup per listed key frame: nMPs, nRedundantObservations and, per slot, the uncapped count of qualifying observations and two flags
//   k_tracked      one workgroup per listed key frame: the two counts over its point and line rows
//   k_mp_culling   one thread per point
// The slot-to-lane mapping of k_cull_tables: ONE SLOT PER LANE, SLOT_PER slots of a thread and SLOT_OBS observations of a slot in flight together: the
// walk k_conn_count makes over the same rows (SlotChunk, map_kernels.hpp; DESIGN 4.5, "What the map-side kernels share").  The walk is a chain of dependent gathers per observation (the observation, its key frame's row
// offsets, the octave at the observer's slot) and is bound by their latency, not by bytes.  A point has about 10 observers: a wave per slot with a lane per
// observation would keep 10 of 64 lanes busy and need a reduction per slot; a lane per slot keeps all 64 busy on independent chains, needs no cross-lane step
// before the two sums at the end, and a row of about 2000 slots fills the workgroup's 256 lanes twice with SLOT_PER = 4.  Every stage of the chain is issued
// for all SLOT_OBS observations before the first is used (addresses of left-out observations are replaced by safe ones, not branched round), so a lane has up
// to SLOT_OBS loads per stage outstanding; the slot row itself (index, depth, octave) is read coalesced.  There is no per-key-frame LDS table, so
// OLF_LOCALMAP_MAX_KF does not apply, and a workgroup uses 8 bytes of LDS: occupancy is bounded by registers alone.
#include "map_kernels.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int CL_THREADS = 256;
constexpr int CL_CHUNK = CL_THREADS * SLOT_PER;                // slots per chunk of the walk
constexpr int CL_TH_OBS = 3;                                   // thObs, :647-648

struct CullArgs {
    olf_map_graph g;
    olf_cull_view v;
    int n_list, monocular;
    const int* kf_list;
    int *n_mps, *n_red;
    uint8_t* redundant;
    int* row_offsets;
    int* slot_count;
    uint8_t* slot_flags;
    int slot_capacity;
};

// the listed rows' lengths (0 for a key frame outside the graph), then their running sum
__global__ __launch_bounds__(OFFSET_SCAN_THREADS) void k_cull_rows(CullArgs A, int* __restrict__ status)
{
    const int n_kf = A.g.n_kf;
    for (int j = threadIdx.x; j < A.n_list; j += OFFSET_SCAN_THREADS) {      // (thread t writes and, in offset_scan, reads the entries j = t mod 1024)
        int kf, b = 0, e = 0;
        if (listed_kf(A.kf_list, j, n_kf, kf)) csr_row(A.g.kf_mp_offsets, n_kf, kf, b, e);
        A.row_offsets[j + 1] = e - b;
    }
    offset_scan(A.row_offsets, A.n_list, A.slot_capacity, status, STATUS_CONNECTIONS_LIST);
}

__global__ __launch_bounds__(CL_THREADS) void k_cull_tables(CullArgs A, int* __restrict__ status)
{
    __shared__ int s_mps, s_red;
    const olf_map_graph& g = A.g;
    const olf_cull_view& v = A.v;
    const int j = blockIdx.x, tid = threadIdx.x, n_kf = g.n_kf;
    int kf;
    if (!listed_kf(A.kf_list, j, n_kf, kf)) {                        // (the whole workgroup: kf is uniform)
        if (tid == 0) { atomicOr(status, STATUS_KF_INDEX); A.n_mps[j] = 0; A.n_red[j] = 0; A.redundant[j] = 0; }
        return;
    }
    if (tid == 0) { s_mps = 0; s_red = 0; }
    __syncthreads();

    int b, e;
    csr_row(g.kf_mp_offsets, n_kf, kf, b, e);
    const int slots_total = max(g.kf_mp_offsets[n_kf], 0);
    const int obs_total = max(g.mp_obs_offsets[g.n_mp], 0);
    const float th_depth = v.kf_th_depth[kf];
    const long long out0 = (long long)A.row_offsets[j] - b;          // slot s of the graph is entry out0 + s of the slot outputs
    int n_mps = 0, n_red = 0;
    for (int c0 = b; c0 < e; c0 += CL_CHUNK) {
        SlotChunk<SLOT_PER, CL_THREADS> C;
        int own[SLOT_PER];
        float depth[SLOT_PER];
#pragma unroll
        for (int k = 0; k < SLOT_PER; ++k) {
            const int s = C.slot(c0, k);
            depth[k] = s < e ? v.kf_slot_depth[s] : 0.0f;
            own[k] = s < e ? (int)v.kf_slot_octave[s] : 0;
        }
        // a point counts when it is live (:654-656) and, unless monocular, not beyond th_depth or behind (:658-662, as written: a NaN depth counts)
        C.take(g.kf_mp_index, c0, e, g.n_mp, g.mp_bad, g.mp_obs_offsets, obs_total, status, STATUS_POINT_INDEX,
               [&](int k) { return A.monocular || !(depth[k] > th_depth || depth[k] < 0); });
#pragma unroll
        for (int k = 0; k < SLOT_PER; ++k) {
            const int s = C.slot(c0, k), nobs = C.item[k] >= 0 ? v.mp_nobs[C.item[k]] : 0;
            int count = 0;                                           // the observations that qualify, :670-683 without the break
            for (int o = C.ob[k]; o < C.oe[k]; o += SLOT_OBS) {
                int q[SLOT_OBS], qs[SLOT_OBS], rb[SLOT_OBS], re[SLOT_OBS], oct[SLOT_OBS];
                bool ok[SLOT_OBS];
#pragma unroll
                for (int t = 0; t < SLOT_OBS; ++t) {                 // (past the row: the key frame itself, which is skipped)
                    q[t] = o + t < C.oe[k] ? g.mp_obs_kf[o + t] : kf;
                    qs[t] = o + t < C.oe[k] ? v.mp_obs_slot[o + t] : 0;
                }
#pragma unroll
                for (int t = 0; t < SLOT_OBS; ++t) {
                    ok[t] = q[t] != kf;                              // pKFi == pKF, :673: before anything of the observation is read
                    if (ok[t] && (unsigned)q[t] >= (unsigned)n_kf) { atomicOr(status, STATUS_KF_INDEX); ok[t] = false; }
                    csr_clamp(g.kf_mp_offsets, ok[t] ? q[t] : kf, slots_total, rb[t], re[t]);      // (else: a row that exists)
                }
#pragma unroll
                for (int t = 0; t < SLOT_OBS; ++t) {
                    if (ok[t] && (unsigned)qs[t] >= (unsigned)(re[t] - rb[t])) { atomicOr(status, STATUS_KF_INDEX); ok[t] = false; }
                    oct[t] = v.kf_slot_octave[ok[t] ? rb[t] + qs[t] : s];      // (the own slot: an address that exists)
                }
#pragma unroll
                for (int t = 0; t < SLOT_OBS; ++t) count += ok[t] && oct[t] <= own[k] + 1;      // :677
            }
            const bool counted = C.item[k] >= 0;
            const bool red = counted && nobs > CL_TH_OBS && count >= CL_TH_OBS;      // :665, :684
            n_mps += counted;
            n_red += red;
            if (s < e && out0 + s < (long long)A.slot_capacity) {
                A.slot_count[out0 + s] = count;
                A.slot_flags[out0 + s] = (uint8_t)((counted ? 1 : 0) | (red ? 2 : 0));
            }
        }
    }
    n_mps = wave_sum_i32(n_mps);
    n_red = wave_sum_i32(n_red);
    if ((tid & 63) == 0) { atomicAdd(&s_mps, n_mps); atomicAdd(&s_red, n_red); }
    __syncthreads();
    if (tid == 0) {
        A.n_mps[j] = s_mps;
        A.n_red[j] = s_red;
        A.redundant[j] = (double)s_red > 0.9 * (double)s_mps ? 1 : 0;      // :693
    }
}

struct TrackedArgs {
    olf_map_graph g;
    const int *mp_nobs, *ml_nobs;
    int n_list, min_obs_points, min_obs_lines;
    const int* kf_list;
    int *n_points, *n_lines;
};

// the slots of row kf that are not NULL, not bad and observed at least min_obs times (min_obs <= 0: no test), summed over the workgroup into *s_sum
__device__ __forceinline__ void tracked_row(const int* __restrict__ offs, const int* __restrict__ index, int n_kf, int kf, int n_items, const uint8_t* __restrict__ bad,
                                            const int* __restrict__ nobs, int min_obs, int bit, int* __restrict__ status, int* s_sum)
{
    int b, e, n = 0;
    csr_row(offs, n_kf, kf, b, e);
    for (int s = b + (int)threadIdx.x; s < e; s += CL_THREADS) {
        const int i = live_item(index[s], n_items, bad, status, bit);
        if (i >= 0) n += min_obs <= 0 || nobs[i] >= min_obs;
    }
    n = wave_sum_i32(n);
    if ((threadIdx.x & 63) == 0) atomicAdd(s_sum, n);
}

__global__ __launch_bounds__(CL_THREADS) void k_tracked(TrackedArgs A, int* __restrict__ status)
{
    __shared__ int s_points, s_lines;
    const olf_map_graph& g = A.g;
    const int j = blockIdx.x, tid = threadIdx.x;
    int kf;
    if (!listed_kf(A.kf_list, j, g.n_kf, kf)) {                      // (-1: no reference key frame, which is no error)
        if (tid == 0) { if (kf != -1) atomicOr(status, STATUS_KF_INDEX); A.n_points[j] = 0; A.n_lines[j] = 0; }
        return;
    }
    if (tid == 0) { s_points = 0; s_lines = 0; }
    __syncthreads();
    tracked_row(g.kf_mp_offsets, g.kf_mp_index, g.n_kf, kf, g.n_mp, g.mp_bad, A.mp_nobs, A.min_obs_points, STATUS_POINT_INDEX, status, &s_points);
    if (g.kf_ml_offsets) tracked_row(g.kf_ml_offsets, g.kf_ml_index, g.n_kf, kf, g.n_ml, g.ml_bad, A.ml_nobs, A.min_obs_lines, STATUS_LINE_INDEX, status, &s_lines);
    __syncthreads();
    if (tid == 0) { A.n_points[j] = s_points; A.n_lines[j] = s_lines; }
}

// the branches of :186-203 in their order
__global__ __launch_bounds__(CL_THREADS) void k_mp_culling(int n, const uint8_t* __restrict__ bad, const int* __restrict__ found, const int* __restrict__ visible,
                                                           const int* __restrict__ nobs, const long long* __restrict__ first_kf_id, long long current_kf_id, int th_obs,
                                                           uint8_t* __restrict__ action)
{
    const int i = blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int age = (int)current_kf_id - (int)first_kf_id[i];        // (int)nCurrentKFid - (int)pMP->mnFirstKFid, :195, :200
    int a = 0;
    if (bad[i]) a = 1;
    else if (f_div((float)found[i], (float)visible[i]) < 0.25f) a = 2;      // GetFoundRatio(), src/MapPoint.cc: static_cast<float>(mnFound) / mnVisible
    else if (age >= 2 && nobs[i] <= th_obs) a = 3;
    else if (age >= 3) a = 4;
    action[i] = (uint8_t)a;
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_keyframe_culling_tables_dev(olf_ctx* c, const olf_map_graph* g, const olf_cull_view* v, int n_list, const int32_t* d_kf_list, int monocular,
                                    int32_t* d_n_mps, int32_t* d_n_redundant, uint8_t* d_redundant, int32_t* d_row_offsets, int32_t* d_slot_count,
                                    uint8_t* d_slot_flags, int slot_capacity, void* stream)
{
    const char* who = "olf_keyframe_culling_tables_dev";
    bool ok = c && g && v && n_list >= 0 && slot_capacity >= 0 && g->n_kf >= 0 && g->n_mp >= 0;
    ok = ok && d_n_mps && d_n_redundant && d_redundant && d_row_offsets && ((d_slot_count && d_slot_flags) || !slot_capacity);
    ok = ok && g->kf_mp_offsets && g->mp_obs_offsets && ((g->mp_bad && v->mp_nobs && v->mp_obs_slot && g->mp_obs_kf) || !g->n_mp) &&
         ((v->kf_th_depth && v->kf_slot_octave && v->kf_slot_depth && g->kf_mp_index) || !g->n_kf);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_list == 0) return OLF_OK;
    CullArgs A;
    A.g = *g; A.v = *v;
    A.n_list = n_list; A.monocular = monocular ? 1 : 0; A.kf_list = d_kf_list;
    A.n_mps = d_n_mps; A.n_red = d_n_redundant; A.redundant = d_redundant;
    A.row_offsets = d_row_offsets; A.slot_count = d_slot_count; A.slot_flags = d_slot_flags; A.slot_capacity = slot_capacity;
    hipStream_t s = ctx_stream(c, stream);
    hipLaunchKernelGGL(k_cull_rows, dim3(1), dim3(OFFSET_SCAN_THREADS), 0, s, A, ctx_status(c));
    hipLaunchKernelGGL(k_cull_tables, dim3(n_list), dim3(CL_THREADS), 0, s, A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_tracked_map_points_batch_dev(olf_ctx* c, const olf_map_graph* g, const int32_t* d_mp_nobs, const int32_t* d_ml_nobs, int n_list,
                                     const int32_t* d_kf_list, int min_obs_points, int min_obs_lines, int32_t* d_n_points, int32_t* d_n_lines, void* stream)
{
    const char* who = "olf_tracked_map_points_batch_dev";
    bool ok = c && g && n_list >= 0 && d_n_points && d_n_lines && g->n_kf >= 0 && g->n_mp >= 0 && g->n_ml >= 0;
    ok = ok && g->kf_mp_offsets && (g->mp_bad || !g->n_mp) && (d_mp_nobs || min_obs_points <= 0 || !g->n_mp);
    ok = ok && (!g->kf_ml_offsets || ((g->ml_bad || !g->n_ml) && (d_ml_nobs || min_obs_lines <= 0 || !g->n_ml)));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_list == 0) return OLF_OK;
    TrackedArgs A;
    A.g = *g; A.mp_nobs = d_mp_nobs; A.ml_nobs = d_ml_nobs;
    A.n_list = n_list; A.min_obs_points = min_obs_points; A.min_obs_lines = min_obs_lines; A.kf_list = d_kf_list;
    A.n_points = d_n_points; A.n_lines = d_n_lines;
    hipLaunchKernelGGL(k_tracked, dim3(n_list), dim3(CL_THREADS), 0, ctx_stream(c, stream), A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_map_point_culling_dev(olf_ctx* c, int n, const uint8_t* d_bad, const int32_t* d_found, const int32_t* d_visible, const int32_t* d_nobs,
                              const int64_t* d_first_kf_id, int64_t current_kf_id, int monocular, uint8_t* d_action, void* stream)
{
    const char* who = "olf_map_point_culling_dev";
    if (!c || n < 0 || (n && (!d_bad || !d_found || !d_visible || !d_nobs || !d_first_kf_id || !d_action))) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n == 0) return OLF_OK;
    hipLaunchKernelGGL(k_mp_culling, dim3((n + CL_THREADS - 1) / CL_THREADS), dim3(CL_THREADS), 0, ctx_stream(c, stream), n, d_bad, d_found, d_visible, d_nobs,
                       (const long long*)d_first_kf_id, (long long)current_kf_id, monocular ? 2 : 3, d_action);      // nThObs, :176-180
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
