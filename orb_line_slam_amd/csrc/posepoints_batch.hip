// posepoints_batch.hip -- olf_pose_optimization_batch_dev: int Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:239-451) for a list of rows.
//
// One launch; one workgroup of 256 lanes carries a row through the four passes and the epilogue (grid-strided over the rows, at most PP_MAX_GRID
// workgroups), no grid-wide synchronisation.  The driver and every edge term are posepoints_terms.hpp, the Levenberg loop and the 6 x 6 LDLT
// g2o_levenberg.hpp, the text posepoints_host.cpp runs too.  Every lane runs the driver on the same values, so all lanes take the same branches and the dense pieces need no broadcast;
// the workgroup cooperates inside DevOps only through the sums of wg_sums.hpp (shared with pose_batch.hip): feature i belongs to lane i % 256, which adds
// its edges in ascending i -- activeRobustChi2's one sum, buildSystem's 21 + 6 -- then the butterfly over the wave and the four waves in wave order.  No
// floating-point atomics; a row's outputs depend on nothing but its own inputs.
// State: per feature of the capacity the edge's current _error (3 doubles: what the stale-error quirk of the reference lives in), invSigma2 (float, widened
// at use as the reference widens it) and one byte (held, outlier, stereo): 29 bytes, one slab per workgroup, in LDS when it fits (58 KB at the default
// capacity of 2000, so two rows share a CU) and otherwise in the batch scratch slot; the code is the same (wg_state.hpp).  Xw and the observation are
// re-read from global memory as floats and widened.  Every slab element is read and written by its owning lane only, so the slab needs no barrier of its own.
#include <algorithm>
#include "posepoints_terms.hpp"
#include "wg_state.hpp"
#include "wg_sums.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int PP_THREADS = 256, PP_MAX_GRID = 1024, PP_SUMS = 27;
constexpr int PP_LDS_DEFAULT = 60 * 1024;                            // the slab beside the kernel's static LDS, within the 64 KB a launch gets unasked
LdsLimit g_pose_points_lds(PP_LDS_DEFAULT);

struct PosePointsArgs {
    olf_pose_points_batch in;
    olf_pose_points_outputs out;
    int n_rows, n_frames, cap, nlevels, use_lds;
    float inv_sigma2[OLF_MAX_LEVELS];
    unsigned char* slabs;                           // [gridDim.x][slab_bytes] in scratch, or NULL: LDS
    size_t slab_bytes;
};

struct PpSlab {
    size_t err, w, f, total;
    __host__ __device__ constexpr explicit PpSlab(int cap) : err(0), w(0), f(0), total(0)
    {
        Regions r;
        err = r.cut(24 * (size_t)cap); w = r.cut(4 * (size_t)cap); f = r.cut((size_t)cap);
        total = r.total;
    }
};
static_assert(PpSlab(2000).w == 48000 && PpSlab(2000).f == 56000 && PpSlab(2000).total == 58000 && PpSlab(1001).w == 24032 && PpSlab(1001).f == 28048 &&
              PpSlab(1001).total == 29056, "the slab's offsets");

using namespace posepoints;

struct PpDevOps {
    Cam c;
    int tid, n, held, active;
    const olf_keypoint* kps;
    const float *ur, *mpw;
    const int32_t* fmp;
    long long base;
    double* err;
    float* w;
    uint8_t* f;
    float* chi2;
    WgSums<PP_THREADS, PP_SUMS> wg;

    __device__ void load(int i, double* X, double* obs) const
    {
        const float* p = mpw + 3 * (size_t)(fmp[i] + base);
        X[0] = (double)p[0]; X[1] = (double)p[1]; X[2] = (double)p[2];
        obs[0] = (double)kps[i].x; obs[1] = (double)kps[i].y; obs[2] = (double)ur[i];
    }
    __device__ int n_edges() const { return held; }
    __device__ int n_active() const { return active; }
    __device__ bool errors(const VertexSE3& v, bool robust, double* chi)
    {
        double S[1] = {0.0}, X[3], obs[3];
        int bad = 0;
        for (int i = tid; i < n; i += PP_THREADS) if ((f[i] & (E_HELD | E_OUT)) == E_HELD) {
            double e[3];
            load(i, X, obs);
            if (!edge_error(c, v.est, X, obs, f[i] & E_STEREO, e)) { ++bad; continue; }
            err[3 * i] = e[0]; err[3 * i + 1] = e[1]; err[3 * i + 2] = e[2];
            S[0] = S[0] + edge_robust_chi2(e, (double)w[i], f[i] & E_STEREO, robust);
        }
        wg.reduce(S, 1, &bad);
        *chi = S[0];
        return bad == 0;
    }
    __device__ bool system(const VertexSE3& v, bool robust, double* S)
    {
        double X[3], obs[3];
        int bad = 0;
        for (int k = 0; k < PP_SUMS; ++k) S[k] = 0.0;
        for (int i = tid; i < n; i += PP_THREADS) if ((f[i] & (E_HELD | E_OUT)) == E_HELD) {
            const double e[3] = {err[3 * i], err[3 * i + 1], err[3 * i + 2]};
            load(i, X, obs);
            bad += !edge_quadratic_form(c, v.est, X, e, (double)w[i], f[i] & E_STEREO, robust, S);
        }
        wg.reduce(S, PP_SUMS, &bad);
        return bad == 0;
    }
    __device__ bool classify(const Se3& est, int* n_bad)
    {
        double X[3], obs[3];
        int bad = 0;
        for (int i = tid; i < n; i += PP_THREADS) if ((f[i] & (E_HELD | E_OUT)) == (E_HELD | E_OUT)) {
            double e[3];
            load(i, X, obs);
            if (!edge_error(c, est, X, obs, f[i] & E_STEREO, e)) { ++bad; continue; }
            err[3 * i] = e[0]; err[3 * i + 1] = e[1]; err[3 * i + 2] = e[2];
        }
        bad = wg.count(bad);
        if (bad) return false;                                      // (uniform) the flags stay as they stood
        for (int i = tid; i < n; i += PP_THREADS) if (f[i] & E_HELD) {
            const double e[3] = {err[3 * i], err[3 * i + 1], err[3 * i + 2]};
            const float v = (float)edge_chi2(e, (double)w[i], f[i] & E_STEREO);
            chi2[i] = v;
            if (v > chi2_threshold(f[i] & E_STEREO)) { f[i] |= E_OUT; ++bad; } else f[i] &= ~E_OUT;
        }
        bad = wg.count(bad);
        *n_bad = bad;
        active = held - bad;
        return true;
    }
};

__global__ __launch_bounds__(PP_THREADS) void k_pose_points_rows(PosePointsArgs A, int* __restrict__ status)
{
    extern __shared__ __align__(16) unsigned char pp_dyn[];
    __shared__ WgSums<PP_THREADS, PP_SUMS>::Lds s_sums;

    const int tid = threadIdx.x;
    const olf_pose_points_batch& in = A.in;
    const PpSlab lay(A.cap);
    unsigned char* slab = wg_state_ptr(A.use_lds != 0, pp_dyn, A.slabs, A.slab_bytes);

    PpDevOps ops;
    ops.c.fx = (double)in.fx; ops.c.fy = (double)in.fy; ops.c.cx = (double)in.cx; ops.c.cy = (double)in.cy; ops.c.bf = (double)in.bf;
    ops.tid = tid;
    ops.mpw = in.mp_world;
    ops.err = reinterpret_cast<double*>(slab + lay.err); ops.w = reinterpret_cast<float*>(slab + lay.w); ops.f = slab + lay.f;
    ops.wg.lds = &s_sums; ops.wg.tid = tid; ops.wg.parity = 0;

    for (int r = blockIdx.x; r < A.n_rows; r += gridDim.x) {        // (every condition below is uniform over the workgroup)
        if (in.row_active && in.row_active[r] <= 0) { if (tid == 0) A.out.n_good[r] = -1; continue; }
        int frame = r;
        long long base = in.mp_index_offset ? in.mp_index_offset[r] : 0;
        if (in.pairs) {
            const int kf = in.pairs[2 * (size_t)r];
            frame = in.pairs[2 * (size_t)r + 1];
            if (!pair_in_batch(kf, frame, A.n_frames)) { if (tid == 0) { A.out.n_good[r] = -1; atomicOr(status, STATUS_PAIR); } continue; }
            base += (long long)kf * A.cap;
        }
        const size_t img = (size_t)frame * in.img_stride, row = (size_t)r * A.cap;
        ops.n = max(0, min(in.counts[img], A.cap));
        ops.kps = in.kps + img * A.cap;
        ops.ur = in.uright + (size_t)frame * A.cap;
        ops.fmp = in.frame_mp + row;
        ops.base = base;
        ops.chi2 = A.out.chi2 + row;

        // who holds what (:280-360): mvpMapPoints as flags, every mvbOutlier cleared
        int bad_octave = 0, held = 0;
        for (int i = tid; i < A.cap; i += PP_THREADS) {
            uint8_t f = 0;
            float w = 0.f;
            if (i < ops.n && ops.fmp[i] >= 0) {
                const long long m = ops.fmp[i] + base;
                const int oct = ops.kps[i].octave;
                if (m < 0 || m >= in.n_mp) atomicOr(status, STATUS_POINT_INDEX);
                else if (oct < 0 || oct >= A.nlevels) bad_octave = 1;
                else { f = E_HELD | (ops.ur[i] < 0.f ? 0 : E_STEREO); w = A.inv_sigma2[oct]; ++held; }
            }
            ops.f[i] = f; ops.w[i] = w;
            ops.chi2[i] = 0.f;
        }
        bad_octave = ops.wg.count(bad_octave);
        held = ops.wg.count(held);
        ops.held = held; ops.active = held;

        Result res;
        run_row(ops, in.Tcw + (size_t)r * 16, &res);

        uint8_t* oo = A.out.outlier_out + row;
        for (int i = tid; i < A.cap; i += PP_THREADS) oo[i] = (ops.f[i] & E_OUT) ? 1 : 0;
        if (tid == 0) {
            for (int i = 0; i < 16; ++i) A.out.Tcw_out[(size_t)r * 16 + i] = res.Tcw[i];
            A.out.n_good[r] = res.n_good; A.out.n_initial[r] = res.n_initial; A.out.passes[r] = res.passes;
            for (int p = 0; p < 4; ++p) A.out.iters[4 * (size_t)r + p] = res.iters[p];
            A.out.status[r] = res.status | (bad_octave ? ST_OCTAVE : 0);
        }
    }
}

}  // namespace olf

using namespace olf;

extern "C" int olf_pose_optimization_batch_dev(olf_ctx* c, const olf_pose_points_batch* in, int n_rows, int n_frames, const olf_pose_points_outputs* o, void* stream)
{
    const char* who = "olf_pose_optimization_batch_dev";
    bool ok = c && in && o && n_rows >= 0 && n_frames >= 0 && in->n_mp >= 0 && in->img_stride >= 1 && (in->pairs || n_rows <= n_frames);
    ok = ok && in->kps && in->counts && in->uright && in->Tcw && in->frame_mp && (in->mp_world || !in->n_mp);
    ok = ok && o->Tcw_out && o->outlier_out && o->n_good && o->n_initial && o->chi2 && o->passes && o->iters && o->status;
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_rows == 0) return OLF_OK;
    PosePointsArgs A;
    A.in = *in; A.out = *o; A.n_rows = n_rows; A.n_frames = n_frames;
    A.cap = olf_orb_capacity(c);
    A.nlevels = ctx_level_inv_sigma2(c, A.inv_sigma2);
    const PpSlab lay(A.cap);
    const int grid = std::min(n_rows, PP_MAX_GRID);
    A.slab_bytes = lay.total;
    OLF_TRY(wg_state_place(c, g_pose_points_lds, lay.total, grid, &A.slabs, &A.use_lds));
    hipLaunchKernelGGL(k_pose_points_rows, dim3(grid), dim3(PP_THREADS), A.use_lds ? lay.total : 0, ctx_stream(c, stream), A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}
