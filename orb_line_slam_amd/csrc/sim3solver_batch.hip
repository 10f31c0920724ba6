// sim3solver_batch.hip -- Sim3Solver's RANSAC (src/Sim3Solver.cc) for a list of key-frame pairs, as LoopClosing::ComputeSim3 drives it
// (src/LoopClosing.cc:280-307), and the filter of the matches by the accepted inliers (:319-324).  The arithmetic is sim3solver_terms.hpp, the text the
// host form (sim3solver_host.cpp) runs too.
//   k_sim3_solver   one workgroup of four waves per pair (a grid of at most 1024 workgroups strides the list).
//     1. The row's correspondences are compacted in ascending i1 (the order decides what a draw picks): block_rank (map_kernels.hpp; DESIGN 4.5, "What the
//        map-side kernels share").  Each keeps 13 words -- both camera-frame points, both images, both gates, i1 -- as planes of `cap` words, in LDS where
//        52 * cap bytes fit the limit and in the workgroup's part of the batch scratch slot above it (one flat pointer, one text).
//     2. The window [iterations_done, min(cap(N), iterations_done + n_iterations)) is taken in rounds of 64 iterations.  The hypotheses do not depend on one
//        another once the draws are fixed: in a round every wave takes 16 iterations (dealt round-robin, so a window of 5 works all four), ONE LANE PER FIT (the Jacobi sweeps are the long dependent chain
//        of a fit; a wave that computed one fit uniformly would spend 64 lanes on it), then walks its 16 hypotheses, the two 3 x 4 transforms broadcast
//        from the fitting lane, the lanes striding over the correspondences and a wave sum giving n_it.
//     3. Wave 0 takes the round's 64 counts: an exclusive prefix maximum seeded with the carried best, the record iterations (n >= every earlier count
//        and the carried best) and the first record with n > min_inliers -- the sequential acceptance rule as a scan.  An accepting round is
//        the last; counts behind the accepting iteration are dropped, so nothing depends on the round size.
//     4. The last record of the call is fitted again -- by the same text, in one more turn of the round loop: the fit is inlined once -- and written as
//        the new best; an accepted one scatters its flags to i1.
//     Bound by instruction issue: a fit is some thousand dependent float operations, a hypothesis 2 * N projections; the bytes are the row and 100 per
//     correspondence, read once.
//   k_sim3_filter   one lane per (pair, i1).
#include "sim3solver_terms.hpp"
#include "batch_frames.hpp"
#include "host_table_cache.hpp"
#include "map_kernels.hpp"
#include "solver_args.hpp"
#include "wg_state.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int S3_THREADS = 256, S3_WAVES = 4, S3_PER_WAVE = 16, S3_ROUND = 64, S3_MAX_GRID = 1024;
constexpr int S3_LDS_DEFAULT = 60 * 1024;           // of the 64 KiB a workgroup takes without asking for more; the kernel's own LDS is below 1 KiB
LdsLimit g_sim3_solver_lds(S3_LDS_DEFAULT);

struct Sim3SolverArgs {
    const olf_keypoint* kps;
    const int *counts, *pairs, *matches12, *its_of_N;
    const float *Tcw, *world;
    const uint8_t *valid, *bad;
    const uint32_t* draws;
    olf_sim3_solver_io io;
    float* state;                                   // [gridDim.x][S3_WORDS][cap] in scratch, or NULL: LDS
    int img_stride, cap, n_frames, n_pairs, nlevels, fix_scale, min_inliers, max_iterations, n_iterations;
    float cam[4];
    float sf[OLF_MAX_LEVELS];
};

extern __shared__ float s3_dyn[];

__device__ __forceinline__ void s3_load_corr(const float* st, int cap, int q, float* X1, float* X2, float* p1, float* p2, float& g1, float& g2)
{
    for (int k = 0; k < 3; ++k) { X1[k] = st[(size_t)k * cap + q]; X2[k] = st[(size_t)(3 + k) * cap + q]; }
    p1[0] = st[(size_t)6 * cap + q]; p1[1] = st[(size_t)7 * cap + q]; p2[0] = st[(size_t)8 * cap + q]; p2[1] = st[(size_t)9 * cap + q];
    g1 = st[(size_t)10 * cap + q]; g2 = st[(size_t)11 * cap + q];
}

// the fit of absolute iteration j of pair p from its draws and the compacted points
__device__ __forceinline__ void s3_fit_iteration(const Sim3SolverArgs& A, const float* st, int p, int j, int N, S3Hyp& H)
{
    const uint32_t* r = A.draws + 3 * ((size_t)p * A.max_iterations + j);
    const uint32_t rr[3] = {r[0], r[1], r[2]};
    int idx[3];
    ransac_sample<3>(N, rr, idx);
    float P1[3][3], P2[3][3];
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) { P1[k][c] = st[(size_t)c * A.cap + idx[k]]; P2[k][c] = st[(size_t)(3 + c) * A.cap + idx[k]]; }
    s3_fit(P1, P2, A.fix_scale != 0, H);
}

__global__ __launch_bounds__(S3_THREADS) void k_sim3_solver(Sim3SolverArgs A, int* __restrict__ status)
{
    __shared__ int s_cnt[1][S3_WAVES];
    __shared__ int s_accept, s_best_it, s_carry;
    __shared__ int s_counts[S3_ROUND];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, cap = A.cap;
    // (its own text, not wg_state_ptr: the product in another order moved this kernel, which is at its scalar register limit, outside the timing rule)
    float* st = A.state ? A.state + (size_t)blockIdx.x * S3_WORDS * cap : s3_dyn;
    int* st_i1 = reinterpret_cast<int*>(st + (size_t)12 * cap);

    for (int p = blockIdx.x; p < A.n_pairs; p += gridDim.x) {
        __syncthreads();                                             // (the previous pair's LDS is done with)
        const int f1 = A.pairs[2 * (size_t)p], f2 = A.pairs[2 * (size_t)p + 1];
        if (!pair_in_batch(f1, f2, A.n_frames)) {                    // (the whole workgroup: the pair is uniform)
            if (tid == 0) { atomicOr(status, STATUS_PAIR); A.io.n_inliers[p] = -1; }
            continue;
        }
        const int N1 = frame_count(f1, A.counts, A.img_stride, cap), N2 = frame_count(f2, A.counts, A.img_stride, cap);
        const olf_keypoint* kp1 = A.kps + (size_t)f1 * A.img_stride * cap;
        const olf_keypoint* kp2 = A.kps + (size_t)f2 * A.img_stride * cap;
        const size_t row = (size_t)p * cap, r1 = (size_t)f1 * cap, r2 = (size_t)f2 * cap;
        // ---- 1. the correspondences, in ascending i1 (:62-109)
        int N = 0;
        for (int base = 0; base < N1; base += S3_THREADS) {          // (uniform trip count)
            const int i = base + tid;
            bool live = false;
            float X1[3], X2[3], p1[2], p2[2], g1 = 0.f, g2 = 0.f;
            if (i < N1) {
                A.io.inliers[row + i] = 0;
                const int v = A.matches12[row + i];
                if (s3_is_match(v, N2) && (!A.valid || (A.valid[r1 + i] && A.valid[r2 + v])) && !(A.bad && (A.bad[r1 + i] || A.bad[r2 + v]))) {
                    const int o1 = kp1[i].octave, o2 = kp2[v].octave;
                    if ((unsigned)o1 < (unsigned)A.nlevels && (unsigned)o2 < (unsigned)A.nlevels) {
                        live = true;
                        rot_apply(A.Tcw + 16 * (size_t)f1, A.world + 3 * (r1 + i), 1.0f, X1);
                        rot_apply(A.Tcw + 16 * (size_t)f2, A.world + 3 * (r2 + v), 1.0f, X2);
                        s3_image(X1, A.cam, p1);
                        s3_image(X2, A.cam, p2);
                        g1 = s3_gate(A.sf[o1]); g2 = s3_gate(A.sf[o2]);
                    } else atomicOr(status, STATUS_OCTAVE);
                }
            }
            int step;
            const int q = N + block_rank<S3_WAVES>(live, s_cnt, step);      // q <= i < cap
            N += step;
            if (live) {
                for (int k = 0; k < 3; ++k) { st[(size_t)k * cap + q] = X1[k]; st[(size_t)(3 + k) * cap + q] = X2[k]; }
                st[(size_t)6 * cap + q] = p1[0]; st[(size_t)7 * cap + q] = p1[1]; st[(size_t)8 * cap + q] = p2[0]; st[(size_t)9 * cap + q] = p2[1];
                st[(size_t)10 * cap + q] = g1; st[(size_t)11 * cap + q] = g2;
                st_i1[q] = i;
            }
            __syncthreads();
        }
        if (N < A.min_inliers) {                                     // :146-150: bNoMore, nothing else changes
            if (tid == 0) { A.io.n_correspondences[p] = N; A.io.accepted[p] = 0; A.io.no_more[p] = 1; A.io.n_inliers[p] = 0; }
            continue;
        }
        // ---- 2. and 3. the window
        const int cap_its = A.its_of_N[N];                           // 1 <= cap_its <= max_iterations
        const int it0 = min(max(A.io.iterations_done[p], 0), A.max_iterations);
        const int it_end = min(cap_its, it0 + min(A.n_iterations, A.max_iterations));
        if (tid == 0) { s_accept = -1; s_best_it = -1; s_carry = A.io.best_inliers[p]; }
        __syncthreads();
        int accept = -1, best_it = -1, best = 0;
        for (int base = it0;; base += S3_ROUND) {
            // a round of the window, or -- after the last -- the record of the call once more: one text of the fit for both
            accept = s_accept; best_it = s_best_it; best = s_carry;  // (uniform: behind a barrier)
            const bool final = accept >= 0 || base >= it_end;
            if (final && best_it < 0) break;
            const int j = final ? best_it : base + lane * S3_WAVES + w;        // iterations dealt round-robin: a window of 5 works four waves
            S3Hyp H = {};
            if (final ? lane == 0 : (lane < S3_PER_WAVE && j < it_end)) s3_fit_iteration(A, st, p, j, N, H);
            if (final) {
                // ---- 4. the new best; an accepted one scatters its flags to i1
                if (tid == 0) {
                    A.io.best_inliers[p] = best;
                    A.io.best_s[p] = H.s;
                    for (int k = 0; k < 9; ++k) A.io.best_R[9 * (size_t)p + k] = H.R[k];
                    for (int k = 0; k < 3; ++k) A.io.best_t[3 * (size_t)p + k] = H.t[k];
                    for (int k = 0; k < 16; ++k) A.io.best_T12[16 * (size_t)p + k] = H.T12[k];
                }
                if (accept >= 0) {
                    float T12[12], T21[12];
                    for (int k = 0; k < 12; ++k) { T12[k] = __shfl(H.T12[k], 0, 64); T21[k] = __shfl(H.T21[k], 0, 64); }
                    for (int q = tid; q < N; q += S3_THREADS) {
                        float X1[3], X2[3], p1[2], p2[2], g1, g2;
                        s3_load_corr(st, cap, q, X1, X2, p1, p2, g1, g2);
                        if (s3_inlier(T12, T21, A.cam, X1, X2, p1, p2, g1, g2)) A.io.inliers[row + st_i1[q]] = 1;
                    }
                }
                break;
            }
            for (int h = 0; h < S3_PER_WAVE && base + h * S3_WAVES + w < it_end; ++h) {      // (wave-uniform)
                float T12[12], T21[12];
                for (int k = 0; k < 12; ++k) { T12[k] = __shfl(H.T12[k], h, 64); T21[k] = __shfl(H.T21[k], h, 64); }
                int cnt = 0;
                for (int q = lane; q < N; q += 64) {
                    float X1[3], X2[3], p1[2], p2[2], g1, g2;
                    s3_load_corr(st, cap, q, X1, X2, p1, p2, g1, g2);
                    cnt += s3_inlier(T12, T21, A.cam, X1, X2, p1, p2, g1, g2) ? 1 : 0;
                }
                cnt = wave_sum_i32(cnt);
                if (lane == 0) s_counts[h * S3_WAVES + w] = cnt;
            }
            __syncthreads();
            if (w == 0) {
                const int jj = base + lane;
                const bool in = jj < it_end;
                const int v = in ? s_counts[lane] : -1;
                int incl = v;
                for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(incl, d, 64); if (lane >= d) incl = max(incl, y); }
                int excl = __shfl_up(incl, 1, 64);
                const int carry = s_carry;
                excl = lane == 0 ? carry : max(carry, excl);
                const bool rec = in && v >= excl;                    // mnInliersi >= mnBestInliers at its turn (:183)
                const unsigned long long mr = wave_vote(rec), ma = wave_vote(rec && v > A.min_inliers);      // (:192)
                const int a = ma ? __ffsll((long long)ma) - 1 : 64;
                if (in && lane <= a && A.io.counts) A.io.counts[(size_t)p * A.max_iterations + jj] = v;
                if (ma) { if (lane == a) { s_accept = jj; s_best_it = jj; s_carry = v; } }
                else if (mr) { if (lane == 63 - __clzll((long long)mr)) { s_best_it = jj; s_carry = v; } }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int done = accept >= 0 ? accept + 1 : max(it0, it_end);
            A.io.n_correspondences[p] = N;
            A.io.iterations_done[p] = done;
            A.io.accepted[p] = accept >= 0;
            A.io.no_more[p] = accept < 0 && done >= cap_its;         // :203-204
            A.io.n_inliers[p] = accept >= 0 ? best : 0;
        }
    }
}

__global__ __launch_bounds__(S3_THREADS) void k_sim3_filter(int n_pairs, int cap, const int* m12, const uint8_t* __restrict__ inl,
                                                             const int* __restrict__ n_inl, int* out)
{
    const size_t e = (size_t)blockIdx.x * S3_THREADS + threadIdx.x;
    if (e >= (size_t)n_pairs * cap) return;
    if (n_inl && n_inl[e / cap] < 0) return;
    out[e] = inl[e] ? m12[e] : -1;
}

// the iteration caps of every N in [0, cap] for one parameter set (host_table_cache.hpp)
static HostTableCache g_s3_tables(1);

}  // namespace olf

using namespace olf;

extern "C" {

int olf_sim3_solver_pairs_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, int n_pairs, const int32_t* d_pairs,
                              const int32_t* d_matches12, const olf_sim3_ransac* ransac, const uint32_t* d_draws, const olf_sim3_solver_io* io, void* stream)
{
    const char* who = "olf_sim3_solver_pairs_dev";
    bool ok = c && in && io && n_frames >= 0 && n_pairs >= 0 && sim3_ransac_ok(ransac);
    ok = ok && (!n_pairs || (d_pairs && d_matches12 && d_draws && sim3_io_ok(io)));
    ok = ok && (!n_pairs || !n_frames || (in->kps && in->counts && in->img_stride >= 1 && in->Tcw && in->mp_world));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_pairs == 0) return OLF_OK;
    Sim3SolverArgs A;
    A.cap = olf_orb_capacity(c);
    const size_t state_bytes = (size_t)S3_WORDS * A.cap * sizeof(float);
    const int grid = std::min(n_pairs, S3_MAX_GRID);
    int* d_its;
    Carve k;
    k.add(&d_its, (size_t)A.cap + 1);
    const bool lds = wg_state_in_lds(k, g_sim3_solver_lds, state_bytes, grid, &A.state);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    hipStream_t s = ctx_stream(c, stream);
    OLF_TRY(g_s3_tables.upload({ransac->probability, ransac->min_inliers, ransac->max_iterations, A.cap, 0.f},
                               [&](int N, int* row) { *row = s3_iteration_cap(N, ransac->probability, ransac->min_inliers, ransac->max_iterations); }, d_its, s));
    A.kps = in->kps; A.counts = in->counts; A.pairs = d_pairs; A.matches12 = d_matches12; A.its_of_N = d_its; A.Tcw = in->Tcw; A.world = in->mp_world;
    A.valid = in->mp_valid; A.bad = d_mp_bad; A.draws = d_draws; A.io = *io;
    A.img_stride = in->img_stride; A.n_frames = n_frames; A.n_pairs = n_pairs; A.fix_scale = ransac->fix_scale ? 1 : 0;
    A.min_inliers = ransac->min_inliers; A.max_iterations = ransac->max_iterations; A.n_iterations = ransac->n_iterations;
    A.cam[0] = in->fx; A.cam[1] = in->fy; A.cam[2] = in->cx; A.cam[3] = in->cy;
    A.nlevels = ctx_level_scales(c, A.sf);
    hipLaunchKernelGGL(k_sim3_solver, dim3(grid), dim3(S3_THREADS), lds ? state_bytes : 0, s, A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_sim3_filter_matches_dev(olf_ctx* c, int n_pairs, const int32_t* d_matches12, const uint8_t* d_inliers, const int32_t* d_n_inliers, int32_t* d_out,
                                void* stream)
{
    const char* who = "olf_sim3_filter_matches_dev";
    if (!c || n_pairs < 0 || (n_pairs && (!d_matches12 || !d_inliers || !d_out))) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    const size_t n = (size_t)n_pairs * olf_orb_capacity(c);
    if (n == 0) return OLF_OK;
    if (n > 0x7fffffffULL) { set_error(std::string(who) + ": more than 2^31 row entries"); return OLF_ERR_CAPACITY; }
    hipLaunchKernelGGL(k_sim3_filter, dim3((unsigned)((n + S3_THREADS - 1) / S3_THREADS)), dim3(S3_THREADS), 0, ctx_stream(c, stream), n_pairs,
                       olf_orb_capacity(c), d_matches12, d_inliers, d_n_inliers, d_out);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
