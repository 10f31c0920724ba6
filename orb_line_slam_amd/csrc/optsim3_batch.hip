// optsim3_batch.hip -- olf_optimize_sim3_pairs_dev: int Optimizer::OptimizeSim3 (src/Optimizer.cc:2013-2208) for a list of key-frame pairs.
//
// One launch; one workgroup of 256 lanes carries a pair through both optimisations and both checks (grid-strided over the pairs, at most OS_MAX_GRID
// workgroups), no grid-wide synchronisation.  The driver, the Sim3 algebra and every edge term are optsim3_terms.hpp, the Levenberg loop and the 7 x 7 LDLT
// g2o_levenberg.hpp, the text optsim3_host.cpp runs too.  Every lane runs the driver on the same values, so all lanes take the same branches and the
// dense pieces need no broadcast.  The workgroup cooperates in two places.  The sums (wg_sums.hpp): feature i belongs to lane i % 256, which adds e12_i
// then e21_i in ascending i -- activeRobustChi2's one sum, buildSystem's 28 + 7 -- then the butterfly over the wave and the four waves in wave order; no
// floating-point atomics, a pair's outputs depend on nothing but its own inputs.  And the numeric Jacobian's 14 perturbed estimates with their 14
// inverses, which depend on the vertex alone: lanes 0 .. 13 form one each per linearisation into LDS (28 x 8 doubles), a barrier, and every edge reads
// them; the barrier inside the sum that ends the linearisation stands between these reads and the next linearisation's writes.
// State: per feature of the capacity both edges' current _error (4 doubles: what the stale-error quirk lives in), P1c and P2c (6 floats: they are floats
// widened), both invSigma2 (2 floats), the kf2 feature (the row itself is written) and one byte: 69 bytes, one slab per workgroup, in LDS when it fits and
// otherwise in the batch scratch slot; the code is the same (wg_state.hpp).  Every slab element is read and written by its owning lane only.
#include <algorithm>
#include <math.h>
#include "optsim3_terms.hpp"
#include "wg_state.hpp"
#include "wg_sums.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int OS_THREADS = 256, OS_MAX_GRID = 1024;
constexpr int OS_LDS_DEFAULT = 60 * 1024;                            // the slab beside the kernel's static LDS, within the 64 KB a launch gets unasked
LdsLimit g_optimize_sim3_lds(OS_LDS_DEFAULT);

struct OptSim3Args {
    olf_track_batch in;
    olf_optimize_sim3_io io;
    const uint8_t* mp_bad;
    const int32_t *pairs, *row_active;
    const float *s12, *R12, *t12;
    int n_pairs, n_frames, cap, nlevels, use_lds, fix_scale;
    double th2, delta;
    float inv_sigma2[OLF_MAX_LEVELS];
    unsigned char* slabs;                           // [gridDim.x][slab_bytes] in scratch, or NULL: LDS
    size_t slab_bytes;
};

struct OsSlab {
    size_t err, P, w, i2, f, total;
    __host__ __device__ constexpr explicit OsSlab(int cap) : err(0), P(0), w(0), i2(0), f(0), total(0)
    {
        Regions r;
        err = r.cut(32 * (size_t)cap); P = r.cut(24 * (size_t)cap); w = r.cut(8 * (size_t)cap); i2 = r.cut(4 * (size_t)cap); f = r.cut((size_t)cap);
        total = r.total;
    }
};
static_assert(OsSlab(2000).P == 64000 && OsSlab(2000).w == 112000 && OsSlab(2000).i2 == 128000 && OsSlab(2000).f == 136000 && OsSlab(2000).total == 138000 &&
              OsSlab(1001).P == 32032 && OsSlab(1001).total == 69104, "the slab's offsets");

using namespace optsim3;

// The two long pieces of a linearisation are calls, not inlined copies: the driver around them (the Levenberg loop with its 7 x 7 arrays) and these bodies
// then get their registers separately, which is what keeps the kernel's loops out of private memory.
__device__ __noinline__ void os_perturbed(const VertexSim3& v, int k, Sim3* fwd, Sim3* inv) { perturbed(v, k, fwd, inv); }
__device__ __noinline__ bool os_corr_quadratic_form(const Cam& c, const Sim3* pert, const double* P1, const double* P2, const double* obs1, const double* obs2,
                                                    const double* e, double w1, double w2, double delta, double* S)
{
    return corr_quadratic_form(c, pert, P1, P2, obs1, obs2, e, w1, w2, delta, S);
}

struct OsDevOps {
    Cam c;
    double delta;
    int tid, n, ncorr, active;
    const olf_keypoint *kp1, *kp2;
    double* err;
    float *P, *w;
    int32_t* i2;
    uint8_t* f;
    int32_t* matches;
    float* chi2;
    Sim3* pert;
    WgSums<OS_THREADS, N_SUMS> wg;

    __device__ void load(int i, double* P1, double* P2, double* obs1, double* obs2) const
    {
        for (int k = 0; k < 3; ++k) { P1[k] = (double)P[6 * i + k]; P2[k] = (double)P[6 * i + 3 + k]; }
        const int v = i2[i];
        obs1[0] = (double)kp1[i].x; obs1[1] = (double)kp1[i].y;
        obs2[0] = (double)kp2[v].x; obs2[1] = (double)kp2[v].y;
    }
    __device__ int n_edges() const { return ncorr; }
    __device__ int n_active() const { return active; }
    __device__ bool errors(const VertexSim3& v, bool, double* chi)
    {
        Sim3 inv;
        sim3_inverse(v.est, &inv);
        double S[1] = {0.0}, P1[3], P2[3], obs1[2], obs2[2];
        int bad = 0;
        for (int i = tid; i < n; i += OS_THREADS) if (f[i] == C_HELD) {
            double e[4];
            load(i, P1, P2, obs1, obs2);
            if (!corr_errors(c, v.est, inv, P1, P2, obs1, obs2, e)) { ++bad; continue; }
            for (int k = 0; k < 4; ++k) err[4 * i + k] = e[k];
            S[0] = S[0] + edge_robust_chi2(e, (double)w[2 * i], delta);
            S[0] = S[0] + edge_robust_chi2(e + 2, (double)w[2 * i + 1], delta);
        }
        wg.reduce(S, 1, &bad);
        *chi = S[0];
        return bad == 0;
    }
    __device__ bool system(const VertexSim3& v, bool, double* S)
    {
        if (tid < 14) os_perturbed(v, tid, &pert[tid], &pert[14 + tid]);
        __syncthreads();
        double P1[3], P2[3], obs1[2], obs2[2];
        int bad = 0;
        for (int k = 0; k < N_SUMS; ++k) S[k] = 0.0;
        for (int i = tid; i < n; i += OS_THREADS) if (f[i] == C_HELD) {
            const double e[4] = {err[4 * i], err[4 * i + 1], err[4 * i + 2], err[4 * i + 3]};
            load(i, P1, P2, obs1, obs2);
            bad += !os_corr_quadratic_form(c, pert, P1, P2, obs1, obs2, e, (double)w[2 * i], (double)w[2 * i + 1], delta, S);
        }
        wg.reduce(S, N_SUMS, &bad);
        return bad == 0;
    }
    __device__ int check(double th2)
    {
        int bad = 0;
        for (int i = tid; i < n; i += OS_THREADS) if (f[i] == C_HELD) {
            const double a = edge_chi2(err + 4 * i, (double)w[2 * i]), b = edge_chi2(err + 4 * i + 2, (double)w[2 * i + 1]);
            chi2[2 * i] = (float)a; chi2[2 * i + 1] = (float)b;
            if (a > th2 || b > th2) { f[i] = C_HELD | C_OUT; matches[i] = -1; ++bad; }
        }
        bad = wg.count(bad);
        active -= bad;
        return bad;
    }
};

__global__ __launch_bounds__(OS_THREADS) void k_optimize_sim3_pairs(OptSim3Args A, int* __restrict__ status)
{
    extern __shared__ __align__(16) unsigned char os_dyn[];
    __shared__ WgSums<OS_THREADS, N_SUMS>::Lds s_sums;
    __shared__ Sim3 s_pert[N_PERT];

    const int tid = threadIdx.x;
    const olf_track_batch& in = A.in;
    const OsSlab lay(A.cap);
    unsigned char* slab = wg_state_ptr(A.use_lds != 0, os_dyn, A.slabs, A.slab_bytes);
    const size_t cap = (size_t)A.cap;

    OsDevOps ops;
    ops.c.fx = (double)in.fx; ops.c.fy = (double)in.fy; ops.c.cx = (double)in.cx; ops.c.cy = (double)in.cy;
    ops.delta = A.delta;
    ops.tid = tid;
    ops.err = reinterpret_cast<double*>(slab + lay.err); ops.P = reinterpret_cast<float*>(slab + lay.P); ops.w = reinterpret_cast<float*>(slab + lay.w);
    ops.i2 = reinterpret_cast<int32_t*>(slab + lay.i2); ops.f = slab + lay.f;
    ops.pert = s_pert;
    ops.wg.lds = &s_sums; ops.wg.tid = tid; ops.wg.parity = 0;

    for (int p = blockIdx.x; p < A.n_pairs; p += gridDim.x) {        // (every condition below is uniform over the workgroup)
        if (A.row_active && A.row_active[p] <= 0) { if (tid == 0) A.io.n_inliers[p] = -1; continue; }
        const int kf1 = A.pairs[2 * (size_t)p], kf2 = A.pairs[2 * (size_t)p + 1];
        if (!pair_in_batch(kf1, kf2, A.n_frames)) { if (tid == 0) { A.io.n_inliers[p] = -1; atomicOr(status, STATUS_PAIR); } continue; }
        const size_t r1 = (size_t)kf1 * cap, r2 = (size_t)kf2 * cap, row = (size_t)p * cap;
        const int N1 = max(0, min(in.counts[(size_t)kf1 * in.img_stride], A.cap)), N2 = max(0, min(in.counts[(size_t)kf2 * in.img_stride], A.cap));
        ops.n = N1;
        ops.kp1 = in.kps + (size_t)kf1 * in.img_stride * cap;
        ops.kp2 = in.kps + (size_t)kf2 * in.img_stride * cap;
        ops.matches = A.io.matches12 + row;
        ops.chi2 = A.io.chi2 + 2 * row;
        const float* T1 = in.Tcw + 16 * (size_t)kf1;
        const float* T2 = in.Tcw + 16 * (size_t)kf2;

        // the graph (:2066-2145)
        int bad_octave = 0, ncorr = 0;
        for (int i = tid; i < A.cap; i += OS_THREADS) {
            uint8_t f = 0;
            ops.chi2[2 * i] = 0.f; ops.chi2[2 * i + 1] = 0.f;
            if (i < N1) {
                const int v = ops.matches[i];
                bool ok = (unsigned)v < (unsigned)N2;
                if (ok && in.mp_valid) ok = in.mp_valid[r1 + i] && in.mp_valid[r2 + v];
                if (ok && A.mp_bad) ok = !(A.mp_bad[r1 + i] || A.mp_bad[r2 + v]);
                if (ok) {
                    const int o1 = ops.kp1[i].octave, o2 = ops.kp2[v].octave;
                    if (!((unsigned)o1 < (unsigned)A.nlevels && (unsigned)o2 < (unsigned)A.nlevels)) bad_octave = 1;
                    else {
                        double P1[3], P2[3];
                        cam_point(T1, in.mp_world + 3 * (r1 + i), P1);
                        cam_point(T2, in.mp_world + 3 * (r2 + v), P2);
                        for (int k = 0; k < 3; ++k) { ops.P[6 * i + k] = (float)P1[k]; ops.P[6 * i + 3 + k] = (float)P2[k]; }
                        ops.w[2 * i] = A.inv_sigma2[o1]; ops.w[2 * i + 1] = A.inv_sigma2[o2];
                        ops.i2[i] = v;
                        for (int k = 0; k < 4; ++k) ops.err[4 * i + k] = 0.0;
                        f = C_HELD;
                        ++ncorr;
                    }
                }
            }
            ops.f[i] = f;
        }
        bad_octave = ops.wg.count(bad_octave);
        ncorr = ops.wg.count(ncorr);
        ops.ncorr = ncorr; ops.active = ncorr;

        Sim3 S12;
        sim3_from_floats(A.s12[p], A.R12 + 9 * (size_t)p, A.t12 + 3 * (size_t)p, &S12);
        Result res;
        run_pair(ops, S12, A.fix_scale, A.th2, &res);

        if (tid == 0) {
            double R[9];
            float Scw[16];
            quat_to_mat3(res.S12.q, R);
            sim3_scw(res.S12, T2, Scw);
            double* So = A.io.S12_out + 8 * (size_t)p;
            for (int k = 0; k < 4; ++k) So[k] = res.S12.q[k];
            for (int k = 0; k < 3; ++k) { So[4 + k] = res.S12.t[k]; A.io.t12_out[3 * (size_t)p + k] = (float)res.S12.t[k]; }
            So[7] = res.S12.s;
            A.io.s12_out[p] = (float)res.S12.s;
            for (int k = 0; k < 9; ++k) A.io.R12_out[9 * (size_t)p + k] = (float)R[k];
            for (int k = 0; k < 16; ++k) A.io.Scw_out[16 * (size_t)p + k] = Scw[k];
            A.io.n_inliers[p] = res.n_inliers; A.io.n_correspondences[p] = res.n_correspondences; A.io.n_bad_first[p] = res.n_bad_first;
            A.io.iters[2 * (size_t)p] = res.iters[0]; A.io.iters[2 * (size_t)p + 1] = res.iters[1];
            A.io.status[p] = res.status | (bad_octave ? ST_OCTAVE : 0);
        }
    }
}

}  // namespace olf

using namespace olf;

extern "C" int olf_optimize_sim3_pairs_dev(olf_ctx* c, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, int n_pairs, const int32_t* d_pairs,
                                           const float* d_s12, const float* d_R12, const float* d_t12, float th2, int fix_scale, const int32_t* d_row_active,
                                           const olf_optimize_sim3_io* io, void* stream)
{
    const char* who = "olf_optimize_sim3_pairs_dev";
    bool ok = c && in && io && n_pairs >= 0 && n_frames >= 0 && th2 > 0.f;
    ok = ok && (!n_pairs || (d_pairs && d_s12 && d_R12 && d_t12 && in->kps && in->counts && in->img_stride >= 1 && in->Tcw && in->mp_world));
    ok = ok && (!n_pairs || (io->matches12 && io->S12_out && io->s12_out && io->R12_out && io->t12_out && io->Scw_out && io->n_inliers && io->n_correspondences &&
                             io->n_bad_first && io->iters && io->status && io->chi2));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_pairs == 0) return OLF_OK;
    OptSim3Args A;
    A.in = *in; A.io = *io; A.mp_bad = d_mp_bad; A.pairs = d_pairs; A.row_active = d_row_active; A.s12 = d_s12; A.R12 = d_R12; A.t12 = d_t12;
    A.n_pairs = n_pairs; A.n_frames = n_frames; A.fix_scale = fix_scale != 0;
    A.th2 = (double)th2;
    A.delta = (double)sqrtf(th2);                                    // const float deltaHuber = sqrt(th2), :2062
    A.cap = olf_orb_capacity(c);
    A.nlevels = ctx_level_inv_sigma2(c, A.inv_sigma2);
    const OsSlab lay(A.cap);
    const int grid = std::min(n_pairs, OS_MAX_GRID);
    A.slab_bytes = lay.total;
    OLF_TRY(wg_state_place(c, g_optimize_sim3_lds, lay.total, grid, &A.slabs, &A.use_lds));
    hipLaunchKernelGGL(k_optimize_sim3_pairs, dim3(grid), dim3(OS_THREADS), A.use_lds ? lay.total : 0, ctx_stream(c, stream), A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}
