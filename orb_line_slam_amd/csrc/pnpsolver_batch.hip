// pnpsolver_batch.hip -- PnPsolver's RANSAC (src/PnPsolver.cc) for a list of (key frame, frame) pairs, as Tracking::Relocalization drives it
// (src/Tracking.cc:2255-2308), and what the tracker does with an accepted solver's inliers (:2297-2308).  The arithmetic is pnpsolver_terms.hpp, the text
// the host form (pnpsolver_host.cpp) runs too.
//   k_pnp_solver   one workgroup of four waves per pair (a grid of at most 1024 workgroups strides the list).
//     1. The row's correspondences are compacted in ascending frame feature (the order decides what a draw picks): block_rank (map_kernels.hpp).  Each
//        keeps 8 words -- the 3-D point, the 2-D point, mvMaxError, its feature, and the best set's list -- as planes of `cap` words, in LDS where
//        32 * cap bytes fit the limit and in the workgroup's part of the batch scratch slot above it (one flat pointer, one text).
//     2. The window [iterations_done, max(cap(N), iterations_done + n_iterations)) -- the reference's loop condition is an OR -- is taken in rounds of 32
//        iterations.  A fit is EPnP on four points: a 12 x 12 Jacobi SVD and a dozen small ones, thousands of dependent double operations, so ONE LANE
//        PER FIT, eight lanes in each wave; but its matrices do not fit a lane's registers (At alone is 288 of 512), so every array the fit indexes at
//        run time is a workspace of PNP_WS doubles in LDS, lane-interleaved ([word * 33 + fit]: the lanes of a wave read neighbouring doubles).  Then
//        every wave takes eight hypotheses, R and t broadcast from the fit's workspace, the lanes striding over the correspondences, a wave sum per count.
//     3. The acceptance rule is walked over the round's 32 counts by the whole workgroup (uniformly): an iteration with n >= min_inliers and n > the best
//        so far is a record.  A record's flags become the best set, in ascending order its list, and Refine fits the whole list: compute_pose again,
//        by the workgroup, its six kinds of sums over the correspondences in the terms header's blocked order, what lies between two sums by thread 0 in
//        workspace 32.  Refine's outcome is carried with the best (it is a function of the best set), so an iteration that is no record costs nothing
//        more.  The first iteration with n >= min_inliers whose best set's Refine has more than min_inliers inliers ends the call; counts behind it
//        are dropped, so nothing depends on the round size.
//     Bound by instruction issue and LDS latency of the dependent Jacobi chain: 32 fits per round on 32 of 256 lanes.
//   k_pnp_apply    one workgroup per pair, a lane per feature.
#include "pnpsolver_terms.hpp"
#include "batch_frames.hpp"
#include "host_table_cache.hpp"
#include "map_kernels.hpp"
#include "solver_args.hpp"
#include "wg_state.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int PNP_FITS = 32, PNP_SLOTS = PNP_FITS + 1, PNP_PER_WAVE = PNP_FITS / PNP_WAVES, PNP_MAX_GRID = 1024;
constexpr int PNP_WS_BYTES = PNP_WS * PNP_SLOTS * (int)sizeof(double);      // 111408
constexpr int PNP_LDS_DEFAULT = 46 * 1024;          // what the planes may take beside the workspaces and 3 KB of static LDS, of 160 KiB
static_assert(PNP_WS_BYTES + PNP_LDS_DEFAULT + 4096 <= 160 * 1024, "a workgroup's LDS");
LdsLimit g_pnp_solver_lds(PNP_LDS_DEFAULT);

struct PnpSolverArgs {
    const olf_keypoint* kps;
    const int *counts, *pairs, *matches, *table;    // table[2 N], table[2 N + 1]: the effective min_inliers and the cap of N correspondences
    const float* world;
    const uint8_t *valid, *bad;
    const uint32_t* draws;
    olf_pnp_solver_io io;
    float* state;                                   // [gridDim.x][PNP_WORDS][cap] in scratch, or NULL: LDS
    int img_stride, cap, n_frames, n_pairs, nlevels, max_iterations, n_iterations;
    float th2;
    double cam[4];
    float sf[OLF_MAX_LEVELS];
};

extern __shared__ double pnp_dyn[];

// Refine's environment: the workgroup, the blocked order of pnpsolver_terms.hpp
struct PnpDevBlockEnv {
    double* base;                                   // workspace PNP_FITS
    PnpPlanes P;
    const int* list;
    int count;
    double (*red)[78];
    template <int K>
    struct Acc {
        double part[K];
        __device__ __forceinline__ void add(int k, double v) { part[k] = d_add(part[k], v); }
    };
    __device__ __forceinline__ double& at(int k) { return base[k * PNP_SLOTS]; }
    __device__ __forceinline__ int n() const { return count; }
    __device__ __forceinline__ void point(int i, double* X, double* u) const { P.load(list[i], X, u); }
    template <int K, class F>
    __device__ __forceinline__ void sum(int off, F f)
    {
        const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
        Acc<K> acc;
#pragma unroll
        for (int k = 0; k < K; ++k) acc.part[k] = 0.0;
        for (int i = tid; i < count; i += PNP_THREADS) f(i, acc);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double v = acc.part[k];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) v = d_add(v, __shfl_xor(v, d, 64));
            if (lane == 0) red[w][k] = v;
        }
        __syncthreads();
        if (tid < K) at(off + tid) = d_add(d_add(d_add(red[0][tid], red[1][tid]), red[2][tid]), red[3][tid]);
        __syncthreads();
    }
    template <class F>
    __device__ __forceinline__ void single(F f)
    {
        if (threadIdx.x == 0) f();
        __syncthreads();
    }
};

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_solver(PnpSolverArgs A, int* __restrict__ status)
{
    __shared__ int s_cnt[1][PNP_WAVES];
    __shared__ int s_counts[PNP_FITS], s_deg[PNP_FITS], s_total;
    __shared__ double s_red[PNP_WAVES][78];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, cap = A.cap;
    double* ws = pnp_dyn;
    float* st = wg_state_ptr(!A.state, reinterpret_cast<float*>(pnp_dyn + PNP_WS * PNP_SLOTS), A.state, (size_t)PNP_WORDS * cap);
    int* st_feat = reinterpret_cast<int*>(st + (size_t)6 * cap);
    int* st_list = reinterpret_cast<int*>(st + (size_t)7 * cap);
    const PnpPlanes P = {st, cap};

    for (int p = blockIdx.x; p < A.n_pairs; p += gridDim.x) {
        __syncthreads();                                             // (the previous pair's LDS is done with)
        const int kf = A.pairs[2 * (size_t)p], fr = A.pairs[2 * (size_t)p + 1];
        if (!pair_in_batch(kf, fr, A.n_frames)) {                    // (the whole workgroup: the pair is uniform)
            if (tid == 0) { atomicOr(status, STATUS_PAIR); A.io.n_inliers[p] = -1; }
            continue;
        }
        const int Nf = frame_count(fr, A.counts, A.img_stride, cap), Nk = frame_count(kf, A.counts, A.img_stride, cap);
        const olf_keypoint* kpf = A.kps + (size_t)fr * A.img_stride * cap;
        const size_t row = (size_t)p * cap, rk = (size_t)kf * cap;
        // ---- 1. the correspondences, in ascending frame feature (:67-110, :154-156)
        int N = 0;
        for (int base = 0; base < Nf; base += PNP_THREADS) {         // (uniform trip count)
            const int i = base + tid;
            bool live = false;
            int v = -1, o = 0;
            if (i < Nf) {
                A.io.inliers[row + i] = 0;
                v = A.matches[row + i];
                if (s3_is_match(v, Nk) && (!A.valid || A.valid[rk + v]) && !(A.bad && A.bad[rk + v])) {
                    o = kpf[i].octave;
                    if ((unsigned)o < (unsigned)A.nlevels) live = true;
                    else atomicOr(status, STATUS_OCTAVE);
                }
            }
            int step;
            const int q = N + block_rank<PNP_WAVES>(live, s_cnt, step);     // q <= i < cap
            N += step;
            if (live) {
                for (int k = 0; k < 3; ++k) st[(size_t)k * cap + q] = A.world[3 * (rk + v) + k];
                st[(size_t)3 * cap + q] = kpf[i].x; st[(size_t)4 * cap + q] = kpf[i].y;
                st[(size_t)5 * cap + q] = pnp_max_error(A.sf[o], A.th2);
                st_feat[q] = i;
            }
            __syncthreads();
        }
        const int min_eff = A.table[2 * N], cap_its = A.table[2 * N + 1];
        if (N < min_eff) {                                           // :173-177: bNoMore, nothing else changes
            if (tid == 0) { A.io.n_correspondences[p] = N; A.io.accepted[p] = 0; A.io.no_more[p] = 1; A.io.n_inliers[p] = 0; }
            continue;
        }
        // ---- 2. and 3. the window
        const int it0 = min(max(A.io.iterations_done[p], 0), 1 << 30);
        const int it_end = max(cap_its, it0 + min(A.n_iterations, A.max_iterations));
        int best = A.io.best_inliers[p], refined = A.io.refined_inliers[p], accept = -1;
        for (int base = it0; base < it_end && accept < 0; base += PNP_FITS) {
            __syncthreads();                                         // (the last round's workspaces and counts are done with)
            if (lane < PNP_PER_WAVE) {
                const int slot = w * PNP_PER_WAVE + lane, j = base + slot;
                if (j < it_end) {
                    const uint32_t* r = A.draws + 4 * ((size_t)p * A.max_iterations + j % A.max_iterations);      // C.26
                    const uint32_t rr[4] = {r[0], r[1], r[2], r[3]};
                    int idx[4];
                    ransac_sample<4>(N, rr, idx);
                    PnpSeqEnv e = {ws + slot, PNP_SLOTS, P, idx[0], idx[1], idx[2], idx[3]};
                    pnp_compute_pose(e, A.cam);
                }
            }
            __syncthreads();
            for (int k = 0; k < PNP_PER_WAVE; ++k) {                 // (wave-uniform)
                const int h = w * PNP_PER_WAVE + k;
                if (base + h >= it_end) break;
                const double* wh = ws + h;
                const int var = (int)wh[W_CHOICE * PNP_SLOTS];
                const bool full = wh[W_FLAG * PNP_SLOTS] == 0.0;
                double R[9], t[3];
                for (int x = 0; x < 9; ++x) R[x] = wh[(W_R + 9 * var + x) * PNP_SLOTS];
                for (int x = 0; x < 3; ++x) t[x] = wh[(W_T + 3 * var + x) * PNP_SLOTS];
                int cnt = 0;
                if (full) for (int q = lane; q < N; q += 64) cnt += P.inlier(q, R, t, A.cam) ? 1 : 0;
                cnt = wave_sum_i32(cnt);
                if (lane == 0) { s_counts[h] = cnt; s_deg[h] = !full; }
            }
            __syncthreads();
            for (int h = 0; h < PNP_FITS && base + h < it_end; ++h) {        // (uniform: the sequential rule of :209-238)
                const int j = base + h, n = s_counts[h];
                if (tid == 0) {
                    if (s_deg[h]) atomicOr(status, STATUS_PNP_DEGENERATE);
                    if (A.io.counts) A.io.counts[(size_t)p * A.max_iterations + j % A.max_iterations] = n;
                }
                if (n < min_eff) continue;
                if (n > best) {
                    best = n;
                    const double* wh = ws + h;
                    const int var = (int)wh[W_CHOICE * PNP_SLOTS];
                    double R[9], t[3];
                    for (int x = 0; x < 9; ++x) R[x] = wh[(W_R + 9 * var + x) * PNP_SLOTS];
                    for (int x = 0; x < 3; ++x) t[x] = wh[(W_T + 3 * var + x) * PNP_SLOTS];
                    if (tid == 0) {
                        float T[16];
                        pnp_tcw(R, t, T);
                        for (int x = 0; x < 16; ++x) A.io.best_Tcw[16 * (size_t)p + x] = T[x];
                        A.io.best_inliers[p] = n;
                    }
                    // the best set: its flags by frame feature and its list in ascending order
                    int m = 0;
                    for (int b0 = 0; b0 < N; b0 += PNP_THREADS) {    // (uniform trip count)
                        const int q = b0 + tid;
                        const bool f = q < N && P.inlier(q, R, t, A.cam);
                        if (q < N) A.io.best_flags[row + st_feat[q]] = f;
                        __syncthreads();                             // (s_cnt's last readers)
                        int step;
                        const int at = m + block_rank<PNP_WAVES>(f, s_cnt, step);
                        m += step;
                        if (f) st_list[at] = q;
                    }
                    __syncthreads();
                    // Refine (:260-305)
                    PnpDevBlockEnv e = {ws + PNP_FITS, P, st_list, m, s_red};
                    pnp_compute_pose(e, A.cam);
                    double Rr[9], tr[3];
                    const bool full = pnp_result(e, Rr, tr);
                    if (tid == 0) {
                        s_total = 0;
                        if (!full) atomicOr(status, STATUS_PNP_DEGENERATE);
                        float T[16];
                        pnp_tcw(Rr, tr, T);
                        for (int x = 0; x < 16; ++x) A.io.refined_Tcw[16 * (size_t)p + x] = T[x];
                    }
                    __syncthreads();
                    int cnt = 0;
                    for (int q = tid; q < N; q += PNP_THREADS) {
                        const bool f = full && P.inlier(q, Rr, tr, A.cam);
                        A.io.refined_flags[row + st_feat[q]] = f;
                        cnt += f;
                    }
                    cnt = wave_sum_i32(cnt);
                    if (lane == 0) atomicAdd(&s_total, cnt);
                    __syncthreads();
                    refined = s_total;
                    if (tid == 0) A.io.refined_inliers[p] = refined;
                    __syncthreads();                                 // (s_total's readers, before a later record's reset)
                }
                if (refined > min_eff) { accept = j; break; }        // :226, :292
            }
        }
        // ---- 4. what the call returns (:226-236, :241-255)
        const bool at_cap = accept < 0 && best >= min_eff;
        if (accept >= 0 || at_cap) {
            const uint8_t* from = accept >= 0 ? A.io.refined_flags : A.io.best_flags;
            for (int q = tid; q < N; q += PNP_THREADS) A.io.inliers[row + st_feat[q]] = from[row + st_feat[q]];      // (a thread reads what it wrote itself, or an earlier call did)
        }
        if (tid == 0) {
            A.io.n_correspondences[p] = N;
            A.io.iterations_done[p] = accept >= 0 ? accept + 1 : max(it0, it_end);
            A.io.accepted[p] = accept >= 0 || at_cap;
            A.io.no_more[p] = accept < 0;
            A.io.n_inliers[p] = accept >= 0 ? refined : at_cap ? best : 0;
            if (accept >= 0 || at_cap) {
                const float* T = (accept >= 0 ? A.io.refined_Tcw : A.io.best_Tcw) + 16 * (size_t)p;
                for (int x = 0; x < 16; ++x) A.io.Tcw[16 * (size_t)p + x] = T[x];
            }
        }
    }
}

// Tracking.cc:2297-2308 for one pair per workgroup
__global__ __launch_bounds__(PNP_THREADS) void k_pnp_apply(int cap, int n_frames, const int* __restrict__ counts, int img_stride, const int* __restrict__ pairs,
                                                            const int* matches, const uint8_t* __restrict__ inl, const int* __restrict__ accepted,
                                                            const int* __restrict__ n_inl, int* out, uint8_t* __restrict__ cur_valid, uint8_t* __restrict__ found)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    if (accepted[p] <= 0 || n_inl[p] < 0) return;                    // (uniform) nothing accepted, or a refused pair: the rows stay
    const int fr = pairs[2 * (size_t)p + 1];
    if (fr < 0 || fr >= n_frames) return;
    const int Nf = frame_count(fr, counts, img_stride, cap);
    const size_t row = (size_t)p * cap;
    if (found) for (int i = tid; i < cap; i += PNP_THREADS) found[row + i] = 0;
    __syncthreads();
    for (int i = tid; i < cap; i += PNP_THREADS) {
        const bool on = i < Nf && inl[row + i];
        const int v = matches[row + i];
        if (out) out[row + i] = on ? v : -1;
        if (cur_valid) cur_valid[row + i] = on;
        if (found && on && (unsigned)v < (unsigned)cap) found[row + v] = 1;
    }
}

// the effective min_inliers and the cap of every N in [0, cap] for one parameter set (host_table_cache.hpp)
static HostTableCache g_pnp_tables(2);

}  // namespace olf

using namespace olf;

extern "C" {

int olf_pnp_solver_pairs_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, int n_pairs, const int32_t* d_pairs,
                             const int32_t* d_matches, const olf_pnp_ransac* ransac, const uint32_t* d_draws, const olf_pnp_solver_io* io, void* stream)
{
    const char* who = "olf_pnp_solver_pairs_dev";
    bool ok = c && in && io && n_frames >= 0 && n_pairs >= 0 && pnp_ransac_ok(ransac);
    ok = ok && (!n_pairs || (d_pairs && d_matches && d_draws && pnp_io_ok(io)));
    ok = ok && (!n_pairs || !n_frames || (in->kps && in->counts && in->img_stride >= 1 && in->mp_world));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_pairs == 0) return OLF_OK;
    PnpSolverArgs A;
    A.cap = olf_orb_capacity(c);
    const size_t state_bytes = (size_t)PNP_WORDS * A.cap * sizeof(float);
    const int grid = std::min(n_pairs, PNP_MAX_GRID);
    int* d_tab;
    Carve k;
    k.add(&d_tab, 2 * ((size_t)A.cap + 1));
    const bool lds = wg_state_in_lds(k, g_pnp_solver_lds, state_bytes, grid, &A.state);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    hipStream_t s = ctx_stream(c, stream);
    OLF_TRY(g_pnp_tables.upload({ransac->probability, ransac->min_inliers, ransac->max_iterations, A.cap, ransac->epsilon}, [&](int N, int* row) {
        pnp_parameters(N, ransac->probability, ransac->min_inliers, ransac->max_iterations, ransac->min_set, ransac->epsilon, row, row + 1); }, d_tab, s));
    OLF_TRY(allow_large_lds(reinterpret_cast<const void*>(&k_pnp_solver), PNP_WS_BYTES + PNP_LDS_DEFAULT));
    A.kps = in->kps; A.counts = in->counts; A.pairs = d_pairs; A.matches = d_matches; A.table = d_tab; A.world = in->mp_world;
    A.valid = in->mp_valid; A.bad = d_mp_bad; A.draws = d_draws; A.io = *io;
    A.img_stride = in->img_stride; A.n_frames = n_frames; A.n_pairs = n_pairs;
    A.max_iterations = ransac->max_iterations; A.n_iterations = ransac->n_iterations; A.th2 = ransac->th2;
    A.cam[0] = (double)in->fx; A.cam[1] = (double)in->fy; A.cam[2] = (double)in->cx; A.cam[3] = (double)in->cy;
    A.nlevels = ctx_level_scales(c, A.sf);
    hipLaunchKernelGGL(k_pnp_solver, dim3(grid), dim3(PNP_THREADS), PNP_WS_BYTES + (lds ? state_bytes : 0), s, A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_pnp_apply_inliers_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* d_pairs, const int32_t* d_matches,
                              const uint8_t* d_inliers, const int32_t* d_accepted, const int32_t* d_n_inliers, int32_t* d_out, uint8_t* d_cur_valid,
                              uint8_t* d_already_found, void* stream)
{
    const char* who = "olf_pnp_apply_inliers_dev";
    bool ok = c && in && n_frames >= 0 && n_pairs >= 0;
    ok = ok && (!n_pairs || (d_pairs && d_matches && d_inliers && d_accepted && d_n_inliers && in->counts && in->img_stride >= 1));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_pairs == 0 || olf_orb_capacity(c) == 0) return OLF_OK;
    hipLaunchKernelGGL(k_pnp_apply, dim3(n_pairs), dim3(PNP_THREADS), 0, ctx_stream(c, stream), olf_orb_capacity(c), n_frames, in->counts, in->img_stride,
                       d_pairs, d_matches, d_inliers, d_accepted, d_n_inliers, d_out, d_cur_valid, d_already_found);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
