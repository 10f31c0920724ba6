// pose_batch.hip -- olf_pose_optimization_with_line_batch_dev and olf_discard_outliers_batch_dev: Optimizer::PoseOptimizationWithLine
// (src/Optimizer.cc:604-697) and the "discard outliers" loops after its three calls (src/Tracking.cc:1034-1074, :1547-1590) for a batch of frames.
//
// One launch, one workgroup of 256 lanes per frame, which carries the frame through the four passes and the epilogue; no grid-wide synchronisation.  The
// driver and every term are pose_terms.hpp, the text pose_host.cpp runs too.  Every lane runs the driver on the same values, so all lanes take the same
// branches and the 6 x 6 pieces need no broadcast; the workgroup cooperates inside DevOps:
//   sums            (wg_sums.hpp) feature i belongs to lane i % 256, which adds its features in ascending i, points then lines, into 28 doubles; the lanes' sums are
//                   combined by an xor butterfly over the wave (both partners form the same sum, so every lane ends with the same bits) and the four
//                   waves' sums are added in wave order.  No floating-point atomics; the shape depends on nothing but the frame's own rows.
//   select          element n / 2 of the ascending residuals, exactly: a radix select over the ordered 64-bit patterns, eight bits a round (integer
//                   LDS atomics into 256 bins, whose counts do not depend on the order of arrival).
// State: a frame's previous-frame points (3 doubles) and lines (6), the held / outlier flags, the octaves and two 64-bit keys per feature for the
// selections are one slab, in LDS when it fits (it does at the default capacities) and otherwise in the batch scratch slot; the code is the same
// (wg_state.hpp).
#include <algorithm>
#include "pose_terms.hpp"
#include "wg_state.hpp"
#include "wg_sums.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int PO_THREADS = 256, PO_WAVES = PO_THREADS / 64;
constexpr int PO_LDS_BUDGET = 160 * 1024 - 4096;                     // the slab beside the kernel's static LDS
constexpr uint8_t F_HELD = 1, F_OUT = 2;

struct PoseArgs {
    olf_pose_batch in;
    olf_pose_outputs out;
    olf_pose_params p;
    int n_frames, cap, lcap, nlevels, use_lds;
    float inv_sigma2[OLF_MAX_LEVELS];
    unsigned char* slabs;                           // [n_frames][slab_bytes] in scratch, or NULL: LDS
    size_t slab_bytes;
};

// offsets of the slab's regions.  Its own text, not Regions of wg_state.hpp, and the integer sums below are reduce(none, 0, &n), not WgSums::count: with
// either shared form k_pose_frames, which is at its register limit, compiles to other code and falls outside the timing rule.
__host__ __device__ inline size_t po_align(size_t v) { return Regions::round16(v); }
struct SlabLayout {
    size_t P, L, key, key2, pf, poct, lf, loct, total;
    __host__ __device__ SlabLayout(int cap, int lcap)
    {
        const size_t m = (size_t)std::max(cap, lcap);
        size_t o = 0;
        P = o; o = po_align(o + 24 * (size_t)cap);
        L = o; o = po_align(o + 48 * (size_t)lcap);
        key = o; o = po_align(o + 8 * m);
        key2 = o; o = po_align(o + 8 * m);
        pf = o; o = po_align(o + (size_t)cap);
        poct = o; o = po_align(o + (size_t)cap);
        lf = o; o = po_align(o + (size_t)lcap);
        loct = o; o = po_align(o + (size_t)lcap);
        total = o;
    }
};

struct DevOps {
    pose::Cfg c;
    int tid, np, nl;
    const olf_keypoint* kps;
    const olf_keyline* kls;
    const double* lle;
    const float *mpw, *mlw;
    const int32_t *fmp, *fml;
    long long off, offl;
    double *P, *L;
    unsigned long long *key, *key2;
    uint8_t *pf, *poct, *lf, *loct;
    const float* inv_sigma2;
    // static LDS of the kernel
    WgSums<PO_THREADS, pose::N_SUMS> wg;
    unsigned* hist;
    unsigned* gsum;

    __device__ double sq_of(int oct) const { return sqrt((double)inv_sigma2[oct]); }
    __device__ void line_obs(int i, double* o) const { o[0] = kls[i].startPointX; o[1] = kls[i].startPointY; o[2] = kls[i].endPointX; o[3] = kls[i].endPointY; }

    __device__ void reduce(double* S, int m, int* n) { wg.reduce(S, m, n); }      // wg_sums.hpp

    // the key of rank `rank` (0-based, ascending) among keys[0 .. n_items); rank < n_items
    __device__ unsigned long long select(const unsigned long long* keys, int n_items, int rank)
    {
        unsigned long long prefix = 0, mask = 0;
        unsigned r = (unsigned)rank;
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < n_items; i += PO_THREADS) {
                const unsigned long long k = keys[i];
                if ((k & mask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 16) { unsigned s = 0; for (int b = 0; b < 16; ++b) s += hist[tid * 16 + b]; gsum[tid] = s; }
            __syncthreads();
            unsigned acc = 0;
            int g = 0;
            for (; g < 15; ++g) { const unsigned v = gsum[g]; if (r < acc + v) break; acc += v; }
            int b = g * 16;
            for (; b < g * 16 + 15; ++b) { const unsigned v = hist[b]; if (r < acc + v) break; acc += v; }
            r -= acc;
            prefix |= (unsigned long long)b << shift;
            mask |= 0xffull << shift;
            __syncthreads();
        }
        return prefix;
    }
    // 1.4826 * MAD of the n valid keys of key[0 .. n_items) (the others hold ~0), the deviations left in key2; *median with it
    __device__ double stdv_mad(int n_items, int n, double* median)
    {
        *median = 0.0;
        if (n == 0) return 0.0;
        const double med = pose::value_of(select(key, n_items, n / 2));
        for (int i = tid; i < n_items; i += PO_THREADS) key2[i] = key[i] == ~0ull ? ~0ull : pose::key_of(pose::mad_dev(pose::value_of(key[i]), med));
        __syncthreads();
        *median = med;
        return 1.4826 * pose::value_of(select(key2, n_items, n / 2));
    }

    __device__ void prepare(const double* Tlw)
    {
        for (int i = tid; i < np; i += PO_THREADS) if (pf[i] & F_HELD) {
            const float* X = mpw + 3 * (size_t)(fmp[i] + off);
            const double Xd[3] = {(double)X[0], (double)X[1], (double)X[2]};
            pose::transform3(Tlw, Xd, &P[3 * i]);
        }
        for (int i = tid; i < nl; i += PO_THREADS) if (lf[i] & F_HELD) {
            const float* X = mlw + 6 * (size_t)(fml[i] + offl);
            const double s[3] = {(double)X[0], (double)X[1], (double)X[2]}, e[3] = {(double)X[3], (double)X[4], (double)X[5]};
            pose::transform3(Tlw, s, &L[6 * i]);
            pose::transform3(Tlw, e, &L[6 * i + 3]);
        }
        __syncthreads();
    }
    __device__ void sums(const double* DT, int robust, double sp, double sl, double* S, int* cnt)
    {
        for (int k = 0; k < pose::N_SUMS; ++k) S[k] = 0.0;
        int n = 0;
        for (int i = tid; i < np; i += PO_THREADS) if (pf[i] == F_HELD) {
            pose::accumulate_point(c, DT, &P[3 * i], (double)kps[i].x, (double)kps[i].y, robust, sq_of(poct[i]), sp, S);
            ++n;
        }
        for (int i = tid; i < nl; i += PO_THREADS) if (lf[i] == F_HELD) {
            double o[4];
            line_obs(i, o);
            pose::accumulate_line(c, DT, &L[6 * i], &lle[3 * i], o, robust, sq_of(loct[i]), sl, S);
            ++n;
        }
        reduce(S, pose::N_SUMS, &n);
        *cnt = n;
    }
    // key[i] of the points (lines) that take part: the error norm under DT times the level's factor when `scaled`; returns their number
    __device__ int point_keys(const double* DT, bool active_only, bool scaled)
    {
        int n = 0;
        for (int i = tid; i < np; i += PO_THREADS) {
            const bool take = active_only ? pf[i] == F_HELD : (pf[i] & F_HELD) != 0;
            unsigned long long k = ~0ull;
            if (take) {
                double r = pose::point_term(c, DT, &P[3 * i], (double)kps[i].x, (double)kps[i].y, nullptr);
                if (scaled) r = r * sq_of(poct[i]);
                k = pose::key_of(r);
                ++n;
            }
            key[i] = k;
        }
        double none[1];
        reduce(none, 0, &n);
        return n;
    }
    __device__ int line_keys(const double* DT, bool active_only, bool scaled)
    {
        int n = 0;
        for (int i = tid; i < nl; i += PO_THREADS) {
            const bool take = active_only ? lf[i] == F_HELD : (lf[i] & F_HELD) != 0;
            unsigned long long k = ~0ull;
            if (take) {
                double r = pose::line_term(c, DT, &L[6 * i], &lle[3 * i], nullptr, nullptr, nullptr);
                if (scaled) r = r * sq_of(loct[i]);
                k = pose::key_of(r);
                ++n;
            }
            key[i] = k;
        }
        double none[1];
        reduce(none, 0, &n);
        return n;
    }
    __device__ void robust_scales(const double* DT, double* sp, double* sl)
    {
        double med;
        int n = point_keys(DT, true, false);
        *sp = stdv_mad(np, n, &med);
        __syncthreads();
        n = line_keys(DT, true, false);
        *sl = stdv_mad(nl, n, &med);
        __syncthreads();
    }
    // vector_mean_stdv_mad and the flag loop of removeOutliers over key[0 .. n_items), n of them valid
    __device__ void decide(int n_items, int n, uint8_t* flag)
    {
        if (n == 0) return;
        double med;
        const double stdv = stdv_mad(n_items, n, &med);
        double S[2] = {0.0, 0.0};
        int k = 0;
        for (int i = tid; i < n_items; i += PO_THREADS) if (key[i] != ~0ull) {
            const double r = pose::value_of(key[i]);
            if (r < 2.0 * stdv) { S[0] = S[0] + r; ++k; }
            S[1] = S[1] + r;
        }
        reduce(S, 2, &k);
        const double mean = pose::mad_mean(S[0], k, S[1], n), th = c.inlier_k * stdv;
        for (int i = tid; i < n_items; i += PO_THREADS) if (key[i] != ~0ull) flag[i] = pose::is_outlier(pose::value_of(key[i]), mean, th) ? (F_HELD | F_OUT) : F_HELD;
        __syncthreads();
    }
    __device__ void remove_outliers(const double* DT)
    {
        if (c.has_points) { const int n = point_keys(DT, false, true); decide(np, n, pf); }
        if (c.has_lines) { const int n = line_keys(DT, false, true); decide(nl, n, lf); }
    }
};

__global__ __launch_bounds__(PO_THREADS) void k_pose_frames(PoseArgs A, int* __restrict__ status)
{
    extern __shared__ __align__(16) unsigned char po_dyn[];
    __shared__ WgSums<PO_THREADS, pose::N_SUMS>::Lds s_sums;
    __shared__ unsigned s_hist[256], s_gsum[16];

    const int j = blockIdx.x, tid = threadIdx.x;
    const olf_pose_batch& in = A.in;
    const SlabLayout lay(A.cap, A.lcap);
    unsigned char* slab = wg_state_ptr(A.use_lds != 0, po_dyn, A.slabs, A.slab_bytes);

    DevOps ops;
    pose::Cfg& c = ops.c;
    c.max_iters = A.p.max_iters_ref; c.homog_th = A.p.homog_th; c.min_error = A.p.min_error; c.min_error_change = A.p.min_error_change; c.inlier_k = A.p.inlier_k;
    c.use_motion_model = A.p.use_motion_model != 0; c.has_points = A.p.has_points != 0; c.has_lines = A.p.has_lines != 0;
    c.fx = in.fx; c.fy = in.fy; c.cx = in.cx; c.cy = in.cy;
    const size_t img = (size_t)j * in.img_stride;
    ops.tid = tid;
    ops.np = A.cap ? max(0, min(in.counts[img], A.cap)) : 0;
    ops.nl = A.lcap ? max(0, min(in.lcounts[img], A.lcap)) : 0;
    ops.kps = in.kps + img * A.cap; ops.kls = in.kls + img * A.lcap; ops.lle = in.lle + (size_t)j * A.lcap * 3;
    ops.mpw = in.mp_world; ops.mlw = in.ml_world;
    ops.fmp = in.frame_mp + (size_t)j * A.cap; ops.fml = in.frame_ml + (size_t)j * A.lcap;
    ops.off = in.mp_index_offset ? in.mp_index_offset[j] : 0; ops.offl = in.ml_index_offset ? in.ml_index_offset[j] : 0;
    ops.P = reinterpret_cast<double*>(slab + lay.P); ops.L = reinterpret_cast<double*>(slab + lay.L);
    ops.key = reinterpret_cast<unsigned long long*>(slab + lay.key); ops.key2 = reinterpret_cast<unsigned long long*>(slab + lay.key2);
    ops.pf = slab + lay.pf; ops.poct = slab + lay.poct; ops.lf = slab + lay.lf; ops.loct = slab + lay.loct;
    ops.inv_sigma2 = A.inv_sigma2;
    ops.wg.lds = &s_sums; ops.wg.tid = tid; ops.wg.parity = 0; ops.hist = s_hist; ops.gsum = s_gsum;

    // who holds what: mvpMapPoints / mvpMapLines as flags, with the entry's outlier flags
    int bad_octave = 0;
    const uint8_t* oin = in.outlier ? in.outlier + (size_t)j * A.cap : nullptr;
    const uint8_t* olin = in.outlier_l ? in.outlier_l + (size_t)j * A.lcap : nullptr;
    for (int i = tid; i < ops.np; i += PO_THREADS) {
        uint8_t f = 0, o = 0;
        if (ops.fmp[i] >= 0) {
            const long long m = ops.fmp[i] + ops.off;
            const int oct = ops.kps[i].octave;
            if (m < 0 || m >= in.n_mp) atomicOr(status, STATUS_POINT_INDEX);
            else if (oct < 0 || oct >= A.nlevels) bad_octave = 1;
            else { f = F_HELD | ((oin && oin[i]) ? F_OUT : 0); o = (uint8_t)oct; }
        }
        ops.pf[i] = f; ops.poct[i] = o;
    }
    for (int i = tid; i < ops.nl; i += PO_THREADS) {
        uint8_t f = 0, o = 0;
        if (ops.fml[i] >= 0) {
            const long long m = ops.fml[i] + ops.offl;
            const int oct = ops.kls[i].octave;
            if (m < 0 || m >= in.n_ml) atomicOr(status, STATUS_LINE_INDEX);
            else if (oct < 0 || oct >= A.nlevels) bad_octave = 1;
            else { f = F_HELD | ((olin && olin[i]) ? F_OUT : 0); o = (uint8_t)oct; }
        }
        ops.lf[i] = f; ops.loct[i] = o;
    }
    bad_octave = __syncthreads_or(bad_octave);

    pose::Result r;
    const float* Tcw = in.Tcw + (size_t)j * 16;
    pose::run_frame(ops, c, Tcw, in.Tcw_prev ? in.Tcw_prev + (size_t)j * 16 : Tcw, in.DT_cov_in ? in.DT_cov_in + (size_t)j * 36 : nullptr, &r);
    __syncthreads();

    int cnt[2] = {0, 0};
    uint8_t* oo = A.out.outlier_out + (size_t)j * A.cap;
    uint8_t* ol = A.out.outlier_l_out + (size_t)j * A.lcap;
    for (int i = tid; i < A.cap; i += PO_THREADS) {
        const uint8_t f = i < ops.np ? ops.pf[i] : 0;
        oo[i] = (f & F_OUT) ? 1 : 0;
        cnt[0] += f == F_HELD;
    }
    for (int i = tid; i < A.lcap; i += PO_THREADS) {
        const uint8_t f = i < ops.nl ? ops.lf[i] : 0;
        ol[i] = (f & F_OUT) ? 1 : 0;
        cnt[1] += f == F_HELD;
    }
    double none[1];
    ops.reduce(none, 0, &cnt[0]);
    ops.reduce(none, 0, &cnt[1]);
    if (tid == 0) {
        for (int i = 0; i < 16; ++i) { A.out.Tcw_out[(size_t)j * 16 + i] = r.Tcw[i]; A.out.DT[(size_t)j * 16 + i] = r.DT[i]; }
        for (int i = 0; i < 36; ++i) A.out.DT_cov[(size_t)j * 36 + i] = r.cov[i];
        for (int i = 0; i < 6; ++i) A.out.DT_cov_eig[(size_t)j * 6 + i] = r.eig[i];
        A.out.err_norm[j] = r.err;
        A.out.good[j] = (uint8_t)r.good;
        A.out.n_inliers[2 * j] = cnt[0]; A.out.n_inliers[2 * j + 1] = cnt[1];
        for (int p = 0; p < 4; ++p) A.out.iters[4 * j + p] = r.iters[p];
        A.out.status[j] = r.status | (bad_octave ? pose::ST_OCTAVE : 0);
    }
}

struct DiscardArgs {
    olf_discard_batch io;
    int cap, lcap, mode, only_tracking, stereo;
    int32_t* n_matches;
};

// one kind of one frame: the loops of src/Tracking.cc:1036-1054 (mode 0) and :1549-1568 (mode 1); returns this lane's count
__device__ __forceinline__ int discard_row(int n, int32_t* held, uint8_t* outlier, long long off, const uint8_t* obs, int n_map, const DiscardArgs& A, int bit, int* status)
{
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += PO_THREADS) {
        if (held[i] < 0) continue;
        const long long m = held[i] + off;
        if (m < 0 || m >= n_map) { atomicOr(status, bit); continue; }
        const bool seen = !obs || obs[m];
        if (A.mode == 0) {
            if (outlier[i]) { held[i] = -1; outlier[i] = 0; }
            else if (seen) ++cnt;
        } else {
            if (!outlier[i]) cnt += A.only_tracking || seen;
            else if (A.stereo) held[i] = -1;
        }
    }
    return cnt;
}

__global__ __launch_bounds__(PO_THREADS) void k_discard_outliers(DiscardArgs A, int* __restrict__ status)
{
    __shared__ int s_cnt[2];
    const int j = blockIdx.x, tid = threadIdx.x;
    const olf_discard_batch& io = A.io;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    const size_t img = (size_t)j * io.img_stride;
    const int n = A.cap ? max(0, min(io.counts[img], A.cap)) : 0, nl = A.lcap ? max(0, min(io.lcounts[img], A.lcap)) : 0;
    int cp = discard_row(n, io.frame_mp + (size_t)j * A.cap, io.outlier + (size_t)j * A.cap, io.mp_index_offset ? io.mp_index_offset[j] : 0, io.mp_obs, io.n_mp, A,
                         STATUS_POINT_INDEX, status);
    int cl = discard_row(nl, io.frame_ml + (size_t)j * A.lcap, io.outlier_l + (size_t)j * A.lcap, io.ml_index_offset ? io.ml_index_offset[j] : 0, io.ml_obs, io.n_ml, A,
                         STATUS_LINE_INDEX, status);
    cp = wave_sum_i32(cp);
    cl = wave_sum_i32(cl);
    if ((tid & 63) == 0) { atomicAdd(&s_cnt[0], cp); atomicAdd(&s_cnt[1], cl); }
    __syncthreads();
    if (tid < 2) A.n_matches[2 * j + tid] = s_cnt[tid];
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_pose_optimization_with_line_batch_dev(olf_ctx* c, const olf_pose_batch* in, int n_frames, const olf_pose_params* p, const olf_pose_outputs* o, void* stream)
{
    const char* who = "olf_pose_optimization_with_line_batch_dev";
    bool ok = c && in && p && o && n_frames >= 0 && p->max_iters_ref >= 1 && p->homog_th > 0.0 && p->inlier_k >= 0.0 && in->n_mp >= 0 && in->n_ml >= 0 && in->img_stride >= 1;
    ok = ok && in->kps && in->counts && in->kls && in->lcounts && in->lle && in->Tcw && in->frame_mp && in->frame_ml && (in->mp_world || !in->n_mp) && (in->ml_world || !in->n_ml);
    ok = ok && o->Tcw_out && o->DT && o->DT_cov && o->DT_cov_eig && o->err_norm && o->good && o->outlier_out && o->outlier_l_out && o->n_inliers && o->iters && o->status;
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_frames == 0) return OLF_OK;
    PoseArgs A;
    A.in = *in; A.out = *o; A.p = *p; A.n_frames = n_frames;
    A.cap = olf_orb_capacity(c); A.lcap = olf_line_capacity(c);
    A.nlevels = ctx_level_inv_sigma2(c, A.inv_sigma2);
    const SlabLayout lay(A.cap, A.lcap);
    A.slab_bytes = lay.total;
    OLF_TRY(wg_state_place(c, LdsLimit(PO_LDS_BUDGET), lay.total, n_frames, &A.slabs, &A.use_lds));
    // (the launch asks for lay.total bytes: a small slab leaves room for more workgroups on a CU)
    if (A.use_lds && lay.total > 64 * 1024) OLF_TRY(allow_large_lds(reinterpret_cast<const void*>(&k_pose_frames), PO_LDS_BUDGET));
    hipLaunchKernelGGL(k_pose_frames, dim3(n_frames), dim3(PO_THREADS), A.use_lds ? lay.total : 0, ctx_stream(c, stream), A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_discard_outliers_batch_dev(olf_ctx* c, const olf_discard_batch* io, int n_frames, int mode, int only_tracking, int stereo, int32_t* d_n_matches, void* stream)
{
    const char* who = "olf_discard_outliers_batch_dev";
    bool ok = c && io && n_frames >= 0 && (mode == 0 || mode == 1) && d_n_matches && io->counts && io->lcounts && io->frame_mp && io->frame_ml && io->outlier && io->outlier_l &&
              io->n_mp >= 0 && io->n_ml >= 0 && io->img_stride >= 1;
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_frames == 0) return OLF_OK;
    DiscardArgs A;
    A.io = *io; A.cap = olf_orb_capacity(c); A.lcap = olf_line_capacity(c); A.mode = mode; A.only_tracking = only_tracking != 0; A.stereo = stereo != 0; A.n_matches = d_n_matches;
    hipLaunchKernelGGL(k_discard_outliers, dim3(n_frames), dim3(PO_THREADS), 0, ctx_stream(c, stream), A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
