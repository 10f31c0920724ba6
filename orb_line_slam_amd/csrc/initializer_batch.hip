// initializer_batch.hip -- Initializer::Initialize (src/Initializer.cc:44-121) for a list of (reference frame, current frame) pairs, as
// Tracking::MonocularInitialization drives it (src/Tracking.cc:722, :756), and what the tracker does with a successful initialisation (:758-772).  The
// arithmetic is initializer_terms.hpp, the text the host form (initializer_host.cpp) runs too.
//   k_initializer   one workgroup of four waves per pair (a grid of at most 1024 workgroups strides the list).
//     1. The row's correspondences are compacted in ascending reference feature (the order decides what a draw picks and how a score is summed):
//        block_rank (map_kernels.hpp).  Each keeps 8 words -- u1 v1 u2 v2, its feature, CheckRT's cosine and code, its flags -- as planes of `cap` words,
//        in LDS where 32 * cap bytes fit the limit and in the workgroup's part of the batch scratch slot above it (one flat pointer, one text).
//     2. Threads 0..3 walk the four Normalize sums (two frames, two axes) over ALL key points of their frame, sequentially in float (C.32).
//     3. The 2 * max_iterations fits -- iteration `it` as a homography, then as a fundamental matrix, from the same eight draws -- are taken in rounds
//        of 128: ONE LANE PER FIT, 32 lanes in each wave.  A fit is a one-sided Jacobi on 9 rows of 16 (or 8 of 9 and a 3 x 3 behind it): tens of
//        thousands of dependent float operations on a matrix no lane's registers hold, so every array the fit indexes at run time is a workspace of
//        INI_WS_F floats and INI_WS_D doubles in LDS, lane-interleaved ([word * 129 + fit]).  128 of them are what the CU's 160 KiB hold beside 24 KiB
//        of correspondences.  The lane then scores its hypothesis over all correspondences in order (broadcast LDS reads) and keeps its own best under
//        strict >; its fits come in ascending iteration, so that is its first maximum.
//     4. The workgroup takes the first of the maxima over the lanes' bests (the larger score, then the lower iteration), the winners' matrices go
//        through LDS, and the flags of both are recomputed by all threads.
//     5. Thread 0 chooses the model and forms the 4 or 8 motion hypotheses; CheckRT runs per hypothesis with the threads over the correspondences, a
//        count per hypothesis and C.35's selection as at most 51 rounds of a workgroup minimum; the decision is taken by every thread alike; the chosen
//        hypothesis' vP3D / vbTriangulated rows are recomputed and written last.
//     A thread that writes a row by reference feature also writes the zeros of the features between its correspondence and the one before, so every
//     element of a row has one writer.  Every loop is bounded.  Bound by instruction issue and LDS latency of the dependent Jacobi chain.
//   k_initializer_apply   one workgroup per pair, a lane per feature.
#include "initializer_terms.hpp"
#include "batch_frames.hpp"
#include "map_kernels.hpp"
#include "solver_args.hpp"
#include "wg_state.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int INI_FITS = 128, INI_SLOTS = INI_FITS + 1, INI_PER_WAVE = INI_FITS / INI_WAVES, INI_MAX_GRID = 1024;
constexpr int INI_WD_BYTES = INI_WS_D * INI_SLOTS * (int)sizeof(double);                                             // 9288
constexpr int INI_WS_BYTES = (INI_WD_BYTES + INI_WS_F * INI_SLOTS * (int)sizeof(float) + 15) & ~15;                  // 125392
constexpr int INI_LDS_DEFAULT = 24 * 1024;          // what the planes may take beside the workspaces and 4 KB of static LDS, of 160 KiB
static_assert(INI_WS_BYTES + INI_LDS_DEFAULT + 8192 <= 160 * 1024, "a workgroup's LDS");
static_assert(INI_WD_BYTES % 8 == 0 && INI_WS_BYTES % 16 == 0, "the float workspaces and the planes start aligned");
LdsLimit g_initializer_lds(INI_LDS_DEFAULT);

struct IniArgs {
    const olf_keypoint* kps;
    const int *counts, *pairs, *matches;
    const uint32_t* draws;
    olf_initializer_io io;
    float* state;                                   // [gridDim.x][INI_WORDS][cap] in scratch, or NULL: LDS
    int img_stride, cap, n_frames, n_pairs, max_iterations, min_triangulated;
    float sigma, min_parallax, cos_gt, cos_ge;
    IniCam K;
};

extern __shared__ double ini_dyn[];

// the sum of one int per thread over the workgroup (uniform result); part: INI_WAVES words of LDS, free again after the call
__device__ __forceinline__ int ini_block_sum(int v, int* part)
{
    v = wave_sum_i32(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// the minimum of one key per thread over the workgroup (uniform result)
__device__ __forceinline__ unsigned long long ini_block_min(unsigned long long v, unsigned long long* part)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = part[0];
#pragma unroll
    for (int k = 1; k < INI_WAVES; ++k) m = part[k] < m ? part[k] : m;
    return m;
}

__global__ __launch_bounds__(INI_THREADS) void k_initializer(IniArgs A, int* __restrict__ status)
{
    __shared__ int s_cnt[1][INI_WAVES];
    __shared__ int s_part[INI_WAVES];
    __shared__ unsigned long long s_min[INI_WAVES];
    __shared__ float s_norm[8];
    __shared__ float s_bs[2][INI_FITS];
    __shared__ int s_bi[2][INI_FITS];
    __shared__ float s_M[2][9], s_Rs[72], s_ts[24], s_cos[8];
    __shared__ int s_ng[8], s_hflags;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, cap = A.cap;
    double* ws_d = ini_dyn;
    float* ws_f = reinterpret_cast<float*>(reinterpret_cast<char*>(ini_dyn) + INI_WD_BYTES);
    float* st = wg_state_ptr(!A.state, reinterpret_cast<float*>(reinterpret_cast<char*>(ini_dyn) + INI_WS_BYTES), A.state, (size_t)INI_WORDS * cap);
    const IniPlanes P = {st, cap};
    const IniCam K = A.K;
    const int mi = A.max_iterations;

    for (int p = blockIdx.x; p < A.n_pairs; p += gridDim.x) {
        __syncthreads();                                             // (the previous pair's LDS is done with)
        const int ref = A.pairs[2 * (size_t)p], cur = A.pairs[2 * (size_t)p + 1];
        if (!pair_in_batch(ref, cur, A.n_frames)) {                  // (the whole workgroup: the pair is uniform)
            if (tid == 0) { atomicOr(status, STATUS_PAIR); A.io.ok[p] = -1; }
            continue;
        }
        const int N1 = frame_count(ref, A.counts, A.img_stride, cap), N2 = frame_count(cur, A.counts, A.img_stride, cap);
        const olf_keypoint* kp1 = A.kps + (size_t)ref * A.img_stride * cap;
        const olf_keypoint* kp2 = A.kps + (size_t)cur * A.img_stride * cap;
        const size_t row = (size_t)p * cap;
        // ---- 1. mvMatches12 (:51-63), in ascending reference feature
        int N = 0;
        for (int base = 0; base < N1; base += INI_THREADS) {         // (uniform trip count)
            const int i = base + tid;
            int v = -1;
            if (i < N1) v = A.matches[row + i];
            const bool live = i < N1 && s3_is_match(v, N2);
            int step;
            const int q = N + block_rank<INI_WAVES>(live, s_cnt, step);      // q <= i < cap
            N += step;
            if (live) {
                st[q] = kp1[i].x; st[(size_t)cap + q] = kp1[i].y; st[(size_t)2 * cap + q] = kp2[v].x; st[(size_t)3 * cap + q] = kp2[v].y;
                P.feat(q) = i;
                P.flags(q) = 0;
            }
            __syncthreads();
        }
        if (N < 8) {                                                 // C.33
            if (tid == 0) { A.io.n_correspondences[p] = N; A.io.ok[p] = 0; A.io.model[p] = 0; }
            continue;
        }
        // ---- 2. Normalize (:749-795): four sequential walks
        if (tid < 4) ini_normalize_axis(tid < 2 ? kp1 : kp2, tid < 2 ? N1 : N2, tid & 1, &s_norm[2 * tid], &s_norm[2 * tid + 1]);
        __syncthreads();
        const IniNorm n1 = {s_norm[0], s_norm[2], s_norm[1], s_norm[3]}, n2 = {s_norm[4], s_norm[6], s_norm[5], s_norm[7]};
        const float invSigmaSquare = ini_inv_sigma_square(A.sigma);
        // ---- 3. the fits and their scores (:148-171, :199-222)
        if (lane < INI_PER_WAVE) {
            const int slot = w * INI_PER_WAVE + lane;
            IniWs e = {ws_f + slot, ws_d + slot, INI_SLOTS};
            float bestH = 0, bestF = 0, mH[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, mF[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            int itH = -1, itF = -1;
            for (int base = 0; base < 2 * mi; base += INI_FITS) {
                const int f = base + slot;
                if (f >= 2 * mi) break;
                const bool fund = f >= mi;
                const int it = fund ? f - mi : f;
                const uint32_t* r = A.draws + 8 * ((size_t)p * mi + it);
                const uint32_t rr[8] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
                int idx[8];
                ransac_sample<8>(N, rr, idx);
                if (!fund) {
                    float Hi[9], Hinv[9];
                    ini_fit_h(e, P, idx, n1, n2, Hi, Hinv);
                    const float sc = ini_score_h(P, N, Hi, Hinv, invSigmaSquare);
                    if (sc > bestH) {
                        bestH = sc; itH = it;
#pragma unroll
                        for (int k = 0; k < 9; ++k) mH[k] = Hi[k];
                    }
                } else {
                    float Fi[9], sc = 0;
                    if (ini_fit_f(e, P, idx, n1, n2, Fi)) sc = ini_score_f(P, N, Fi, invSigmaSquare);
                    else atomicOr(status, STATUS_INI_DEGENERATE);
                    if (sc > bestF) {
                        bestF = sc; itF = it;
#pragma unroll
                        for (int k = 0; k < 9; ++k) mF[k] = Fi[k];
                    }
                }
            }
            // the lane's bests, and their matrices in words 0 .. 17 of its own workspace (the fits are done with it)
            s_bs[0][slot] = bestH; s_bi[0][slot] = itH; s_bs[1][slot] = bestF; s_bi[1][slot] = itF;
#pragma unroll
            for (int k = 0; k < 9; ++k) { e.at(k) = mH[k]; e.at(9 + k) = mF[k]; }
        }
        __syncthreads();
        // ---- 4. the first of the maxima (C.32)
        int win[2];
        float SS[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            int ws_ = -1, wi = 0x7fffffff;
            float sc = 0;
            for (int s = 0; s < INI_FITS; ++s) {
                const float v = s_bs[m][s];
                const int it = s_bi[m][s];
                if (it >= 0 && (v > sc || (v == sc && it < wi))) { sc = v; wi = it; ws_ = s; }
            }
            win[m] = ws_; SS[m] = sc;
        }
        if (tid < 18) {
            const int m = tid >= 9, k = tid - 9 * m;
            s_M[m][k] = win[m] >= 0 ? ws_f[(size_t)(9 * m + k) * INI_SLOTS + win[m]] : 0.0f;
        }
        __syncthreads();
        const bool anyH = win[0] >= 0, anyF = win[1] >= 0;
        const float SH = SS[0], SF = SS[1];
        float H21[9], H12[9], F21[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { H21[k] = s_M[0][k]; F21[k] = s_M[1][k]; }
        inv3_f32(H21, H12);
        const bool useH = ini_choose_h(SH, SF);
        const int bit = useH ? 1 : 2;
        int cnt = 0;
        for (int q = tid; q < N; q += INI_THREADS) {
            float c[4], s = 0;
            P.load(q, c);
            const int f = (anyH && ini_check_h(H21, H12, c, invSigmaSquare, s) ? 1 : 0) | (anyF && ini_check_f(F21, c, invSigmaSquare, s) ? 2 : 0);
            P.flags(q) = f;
            cnt += (f & bit) ? 1 : 0;
            const int i = P.feat(q), from = q > 0 ? P.feat(q - 1) + 1 : 0, to = q == N - 1 ? N1 : i + 1;
            for (int j = from; j < to; ++j) { A.io.inliers_H[row + j] = j == i ? (f & 1) : 0; A.io.inliers_F[row + j] = j == i ? (f >> 1) & 1 : 0; }
        }
        const int Nin = ini_block_sum(cnt, s_part);
        // ---- 5. the motion hypotheses (thread 0, in workspace 0), CheckRT, the decision
        if (tid == 0) {
            IniWs e = {ws_f, ws_d, INI_SLOTS};
            s_hflags = useH ? ini_hypotheses_h(e, H21, K, s_Rs, s_ts) : ini_hypotheses_f(e, F21, K, s_Rs, s_ts);
        }
        if (tid < 8) { s_ng[tid] = 0; s_cos[tid] = 0.0f; }
        __syncthreads();
        const int hflags = s_hflags;
        int chosen = -1;
        const float th2 = ini_th2(A.sigma);
        if (hflags >= 0) {                                           // (uniform)
            if (tid == 0 && (hflags & 2)) atomicOr(status, STATUS_INI_DEGENERATE);
            const int nh = useH ? 8 : 4;
            for (int h = 0; h < nh; ++h) {                           // CheckRT (:798-907)
                IniPose Hp;
                ini_pose_prepare(K, s_Rs + 9 * h, s_ts + 3 * h, Hp);
                int good = 0;
                for (int q = tid; q < N; q += INI_THREADS) {
                    int code = 0;
                    if (P.flags(q) & bit) {
                        float c[4], p3d[3], cp = 0;
                        P.load(q, c);
                        code = ini_check_point(K, Hp, c, th2, p3d, cp);
                        if (code) {
                            P.cosv(q) = cp;
                            if (cp != cp) atomicOr(status, STATUS_INI_NAN);
                        }
                    }
                    P.code(q) = code;
                    good += code ? 1 : 0;
                }
                const int nGood = ini_block_sum(good, s_part);
                if (nGood > 0) {                                     // C.35: the (min(50, n - 1))-th key in ascending order, a minimum per round
                    const int last = min(50, nGood - 1);
                    unsigned long long lb = 0, m = 0;
                    for (int r = 0; r <= last; ++r) {
                        unsigned long long mine = ~0ull;
                        for (int q = tid; q < N; q += INI_THREADS)
                            if (P.code(q)) {
                                const unsigned long long key = ((unsigned long long)ini_cos_key(P.cosv(q)) << 32) | (unsigned)q;
                                if (key >= lb && key < mine) mine = key;
                            }
                        m = ini_block_min(mine, s_min);
                        lb = m + 1;
                    }
                    if (tid == 0) { s_ng[h] = nGood; s_cos[h] = P.cosv((int)(unsigned)(m & 0xffffffffu)); }
                }
                __syncthreads();                                     // (the codes and cosines of this hypothesis are done with)
            }
            int nGood[8];
            float cosv[8];
#pragma unroll
            for (int h = 0; h < 8; ++h) { nGood[h] = s_ng[h]; cosv[h] = s_cos[h]; }
            chosen = useH ? ini_decide_h(nGood, cosv, Nin, A.min_triangulated, A.cos_ge, 0.0f >= A.min_parallax)
                          : ini_decide_f(nGood, cosv, Nin, A.min_triangulated, A.cos_gt, 0.0f > A.min_parallax);
        }
        if (chosen >= 0) {                                           // (uniform) vP3D and vbTriangulated of the chosen hypothesis
            IniPose Hp;
            ini_pose_prepare(K, s_Rs + 9 * chosen, s_ts + 3 * chosen, Hp);
            for (int q = tid; q < N; q += INI_THREADS) {
                int code = 0;
                float c[4], p3d[3] = {0.0f, 0.0f, 0.0f}, cp = 0;
                if (P.flags(q) & bit) {
                    P.load(q, c);
                    code = ini_check_point(K, Hp, c, th2, p3d, cp);
                }
                const int i = P.feat(q), from = q > 0 ? P.feat(q - 1) + 1 : 0, to = q == N - 1 ? N1 : i + 1;
                for (int j = from; j < to; ++j) {
                    const bool here = j == i && code;
                    A.io.triangulated[row + j] = here && code == 3;
                    for (int k = 0; k < 3; ++k) A.io.P3D[3 * (row + j) + k] = here ? p3d[k] : 0.0f;
                }
            }
        }
        if (tid == 0) {
            A.io.n_correspondences[p] = N;
            A.io.ok[p] = chosen >= 0;
            A.io.model[p] = useH ? 1 : 2;
            A.io.score_H[p] = SH; A.io.score_F[p] = SF;
            if (anyH) for (int k = 0; k < 9; ++k) A.io.H21[9 * (size_t)p + k] = H21[k];
            if (anyF) for (int k = 0; k < 9; ++k) A.io.F21[9 * (size_t)p + k] = F21[k];
            for (int h = 0; h < 8; ++h) { A.io.n_good[8 * (size_t)p + h] = s_ng[h]; A.io.cos_parallax[8 * (size_t)p + h] = s_cos[h]; }
            A.io.hypothesis[p] = chosen;
            if (chosen >= 0) {
                for (int k = 0; k < 9; ++k) A.io.R21[9 * (size_t)p + k] = s_Rs[9 * chosen + k];
                for (int k = 0; k < 3; ++k) A.io.t21[3 * (size_t)p + k] = s_ts[3 * chosen + k];
            }
        }
    }
}

// Tracking.cc:758-772 for one pair per workgroup
__global__ __launch_bounds__(INI_THREADS) void k_initializer_apply(int cap, int n_frames, const int* __restrict__ counts, int img_stride, const int* __restrict__ pairs,
                                                                    const int* matches, const uint8_t* __restrict__ tri, const int* __restrict__ ok,
                                                                    const float* __restrict__ R21, const float* __restrict__ t21, int* out,
                                                                    int* __restrict__ n_matches, float* __restrict__ Tcw)
{
    __shared__ int s_part[INI_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (ok[p] <= 0) return;                                          // (uniform) no initialisation, or a refused pair: the rows stay
    const int ref = pairs[2 * (size_t)p], cur = pairs[2 * (size_t)p + 1];
    if (!pair_in_batch(ref, cur, n_frames)) return;
    const int N1 = frame_count(ref, counts, img_stride, cap), N2 = frame_count(cur, counts, img_stride, cap);
    const size_t row = (size_t)p * cap;
    int cnt = 0;
    for (int i = tid; i < cap; i += INI_THREADS) {
        const int v = matches[row + i];
        const bool on = i < N1 && s3_is_match(v, N2) && tri[row + i];
        if (out) out[row + i] = on ? v : -1;
        cnt += on;
    }
    const int total = ini_block_sum(cnt, s_part);
    if (tid == 0) {
        if (n_matches) n_matches[p] = total;
        if (Tcw) {
            float* T = Tcw + 16 * (size_t)p;
            for (int r = 0; r < 3; ++r) {
                for (int k = 0; k < 3; ++k) T[4 * r + k] = R21[9 * (size_t)p + 3 * r + k];
                T[4 * r + 3] = t21[3 * (size_t)p + r];
                T[12 + r] = 0.0f;
            }
            T[15] = 1.0f;
        }
    }
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_initializer_pairs_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* d_pairs, const int32_t* d_matches,
                              const olf_initializer_params* prm, const uint32_t* d_draws, const olf_initializer_io* io, void* stream)
{
    const char* who = "olf_initializer_pairs_dev";
    bool ok = c && in && io && n_frames >= 0 && n_pairs >= 0 && ini_params_ok(prm);
    ok = ok && (!n_pairs || (d_pairs && d_matches && d_draws && ini_io_ok(io)));
    ok = ok && (!n_pairs || !n_frames || (in->kps && in->counts && in->img_stride >= 1));
    IniArgs A;
    ok = ok && ini_cos_threshold(prm->min_parallax, true, &A.cos_gt) && ini_cos_threshold(prm->min_parallax, false, &A.cos_ge);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_pairs == 0) return OLF_OK;
    A.cap = olf_orb_capacity(c);
    const size_t state_bytes = (size_t)INI_WORDS * A.cap * sizeof(float);
    const int grid = std::min(n_pairs, INI_MAX_GRID);
    int use_lds;
    OLF_TRY(wg_state_place(c, g_initializer_lds, state_bytes, grid, &A.state, &use_lds));
    OLF_TRY(allow_large_lds(reinterpret_cast<const void*>(&k_initializer), INI_WS_BYTES + INI_LDS_DEFAULT));
    A.kps = in->kps; A.counts = in->counts; A.pairs = d_pairs; A.matches = d_matches; A.draws = d_draws; A.io = *io;
    A.img_stride = in->img_stride; A.n_frames = n_frames; A.n_pairs = n_pairs;
    A.max_iterations = prm->max_iterations; A.min_triangulated = prm->min_triangulated; A.sigma = prm->sigma; A.min_parallax = prm->min_parallax;
    A.K = {in->fx, in->fy, in->cx, in->cy};
    hipLaunchKernelGGL(k_initializer, dim3(grid), dim3(INI_THREADS), INI_WS_BYTES + (use_lds ? state_bytes : 0), ctx_stream(c, stream), A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_initializer_apply_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* d_pairs, const int32_t* d_matches,
                              const uint8_t* d_triangulated, const int32_t* d_ok, const float* d_R21, const float* d_t21, int32_t* d_out,
                              int32_t* d_n_matches, float* d_Tcw, void* stream)
{
    const char* who = "olf_initializer_apply_dev";
    bool ok = c && in && n_frames >= 0 && n_pairs >= 0;
    ok = ok && (!n_pairs || (d_pairs && d_matches && d_triangulated && d_ok && in->counts && in->img_stride >= 1 && (!d_Tcw || (d_R21 && d_t21))));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_pairs == 0) return OLF_OK;
    hipLaunchKernelGGL(k_initializer_apply, dim3(n_pairs), dim3(INI_THREADS), 0, ctx_stream(c, stream), olf_orb_capacity(c), n_frames, in->counts,
                       in->img_stride, d_pairs, d_matches, d_triangulated, d_ok, d_R21, d_t21, d_out, d_n_matches, d_Tcw);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
