// keyframe_batch.hip -- the key-frame step for a batch of device-resident frames: which stereo features get a new map point or line, in which order and
// with what geometry (Tracking::StereoInitialization, CreateNewKeyFrame, UpdateLastFrame: src/Tracking.cc:639-677, :1744-1865, :1092-1204), and
// Tracking::NeedNewKeyFrame (:1606-1725).  The rules and the arithmetic are keyframe_terms.hpp, the text the host forms (keyframe_host.cpp) run too.
//   k_stereo_landmarks    one workgroup per (frame, half): blockIdx.x = 0 the points, 1 the lines.  The entries of vDepthIdx are compacted in index order
//                   into LDS as 64-bit keys (block_rank, map_kernels.hpp), the number of close ones is counted beside it, the keys are sorted in place,
//                   the visited prefix is a formula of the two counts (lm_prefix), and a second ordered compaction over the prefix hands out the creation
//                   ranks; the geometry runs for created entries only.  Every output slot is written exactly once: where a feature does not enter, where
//                   its key lies behind the prefix, or where it is visited.
//                   The sort is a bitonic network over the next power of two above the number of keys (not the capacity), padded with ~0.  Keys are
//                   unique, so any correct sort gives std::sort's order; the network needs no second buffer -- 8192 keys are 64 KB, a radix sort's two
//                   buffers would not fit beside anything else -- and no data-dependent control, and at 2048 slots it is 66 steps of
//                   4 compare-exchanges per thread (two 8-byte LDS reads, a 64-bit compare, two selects, two writes: about 16 instructions), some 4000
//                   instructions per thread, against a four-pass 8-bit radix whose stable scatter alone costs 8 ballots per key and pass.
//                   Bound by instruction issue and barriers, not by bytes: a frame reads 8 KB of depth, the 56 KB of key points only where a point is
//                   created, and writes 45 bytes per point slot and 85 per line slot (DESIGN 4.5 has the sum and the measured times).
//   k_need_new_keyframe   one workgroup per frame: the four counts by a strided loop and a wave sum, then thread 0 runs the decision.
#include "keyframe_terms.hpp"
#include "batch_frames.hpp"
#include "map_kernels.hpp"
#include "wg_state.hpp"

namespace olf {

constexpr int KF_THREADS = 256;

struct LandmarkArgs {
    olf_landmarks_batch in;
    olf_landmarks_outputs out;
    int cap, lcap, mode, nlevels;
    LandmarkCam K;
    float sf[OLF_MAX_LEVELS];
};

// the keys of a workgroup's half in LDS, ascending: a bitonic network over p2 (a power of two, >= 2) slots
__device__ __forceinline__ void bitonic_sort(unsigned long long* __restrict__ keys, int p2)
{
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (p2 >> 1); t += KF_THREADS) {
                const int a = 2 * t - (t & (j - 1)), b = a + j;
                const unsigned long long x = keys[a], y = keys[b];
                const bool up = (a & k) == 0;
                if ((x > y) == up) { keys[a] = y; keys[b] = x; }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(KF_THREADS) void k_stereo_landmarks(LandmarkArgs A)
{
    extern __shared__ unsigned long long s_keys[];
    __shared__ int s_cnt[1][KF_THREADS / 64];
    __shared__ int s_close, s_flags;
    const int half = blockIdx.x, j = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const bool lines = half == 1;
    const int cap = lines ? A.lcap : A.cap, mode = A.mode;
    const size_t img = (size_t)j * A.in.img_stride, row = (size_t)j * cap;
    const int N = min(max((lines ? A.in.lcounts : A.in.counts)[img], 0), cap);
    const float* depth = A.in.depth + (size_t)j * A.cap;
    const float* ldisp = A.in.ldisp + 2 * (size_t)j * A.lcap;
    const int* held_row = lines ? (A.in.frame_ml ? A.in.frame_ml + row : nullptr) : (A.in.frame_mp ? A.in.frame_mp + row : nullptr);
    int* visit_order = (lines ? A.out.visit_order_l : A.out.visit_order) + row;
    int* created_order = (lines ? A.out.created_order_l : A.out.created_order) + row;
    int* frame_out = (lines ? A.out.frame_ml_out : A.out.frame_mp_out) + row;
    uint8_t* created = (lines ? A.out.created_l : A.out.created) + row;
    const float* Twc = A.in.Twc + 16 * (size_t)j;

    // what a slot holds when nothing is created for it
    auto blank = [&](int i) {
        created[i] = 0;
        frame_out[i] = held_row ? held_row[i] : -1;
        if (lines) {
            for (int k = 0; k < 6; ++k) { A.out.ml_world[6 * (row + i) + k] = 0.f; if (A.out.ml_world_d) A.out.ml_world_d[6 * (row + i) + k] = 0.0; }
        } else {
            for (int k = 0; k < 3; ++k) { A.out.mp_world[3 * (row + i) + k] = 0.f; A.out.mp_normal[3 * (row + i) + k] = 0.f; }
            A.out.mp_maxd[row + i] = 0.f; A.out.mp_mind[row + i] = 0.f;
        }
    };

    if (tid == 0) { s_close = 0; s_flags = 0; }
    __syncthreads();
    // ---- vDepthIdx, in index order, and nClose
    int m = 0, close = 0, flags = 0;                                 // flags: 1 a NaN line depth, 2 (lines, LASTFRAME) the frame has a stereo point
    for (int base = 0; base < cap; base += KF_THREADS) {             // (uniform trip count)
        const int i = base + tid;
        bool enters = false;
        float z = 0.f;
        if (i < N) {
            if (lines) { bool nan; enters = lm_line_enters(mode, A.in.mbf, ldisp[2 * (size_t)i], ldisp[2 * (size_t)i + 1], z, nan); if (enters && nan) flags |= 1; }
            else { z = depth[i]; enters = lm_point_enters(z); }
        }
        if (i < cap && !enters) blank(i);
        int step;
        const int at = m + block_rank<KF_THREADS / 64>(enters, s_cnt, step);
        if (enters) { s_keys[at] = lm_key(z, i); close += !(z > A.in.thDepth); }
        m += step;
        __syncthreads();
    }
    if (lines && mode == LM_LASTFRAME) {                             // :1105-1106: the point list of this frame
        const int Np = min(max(A.in.counts[img], 0), A.cap);
        bool any = false;
        for (int i = tid; i < Np; i += KF_THREADS) any = any || lm_point_enters(depth[i]);
        if (any) flags |= 2;
    }
    close = wave_sum_i32(close);
    if (lane == 0 && close) atomicAdd(&s_close, close);
    if (flags) atomicOr(&s_flags, flags);
    int p2 = 2;
    while (p2 < m) p2 <<= 1;
    if (mode != LM_INIT && m > 1) for (int q = m + tid; q < p2; q += KF_THREADS) s_keys[q] = LM_KEY_PAD;
    __syncthreads();
    flags = s_flags;
    if (lines && mode == LM_LASTFRAME && !(flags & 2)) flags = 4;    // no stereo point: the lines are not looked at, NaN or not
    int n_visit = m;
    if (mode != LM_INIT) {
        n_visit = lm_prefix(m, s_close, lines ? LM_MIN_LINES : LM_MIN_POINTS);
        if (flags & 5) n_visit = 0;
        if (m > 1 && n_visit > 0) bitonic_sort(s_keys, p2);
    }
    // ---- the walk: ranks of the created among the visited, in visit order
    const int n_map = lines ? A.in.n_ml : A.in.n_mp;
    const int* nobs = lines ? A.in.ml_nobs : A.in.mp_nobs;
    const int new_base = lines ? (A.in.new_base_ml ? A.in.new_base_ml[j] : A.in.n_ml) : (A.in.new_base_mp ? A.in.new_base_mp[j] : A.in.n_mp);
    int n_created = 0, bits = (flags & 1) && tid == 0 ? LM_ST_NAN_DEPTH : 0;
    for (int base = 0; base < cap; base += KF_THREADS) {
        const int q = base + tid;
        int i = -1;
        bool create = false;
        if (q < m) {
            i = lm_key_index(s_keys[q]);
            if (q < n_visit) create = lm_creates(mode, held_row ? held_row[i] : -1, n_map, nobs, bits);
            if (!create) blank(i);
        }
        if (q < cap) visit_order[q] = q < n_visit ? i : -1;
        int step;
        const int k = n_created + block_rank<KF_THREADS / 64>(create, s_cnt, step);
        if (create) {
            created_order[k] = i;
            created[i] = 1;
            frame_out[i] = new_base + k;
            if (lines) {
                double wd[6]; float wf[6];
                lm_line(A.in.kls[img * cap + i], ldisp[2 * (size_t)i], ldisp[2 * (size_t)i + 1], A.K, Twc, wd, wf);
                for (int c = 0; c < 6; ++c) { A.out.ml_world[6 * (row + i) + c] = wf[c]; if (A.out.ml_world_d) A.out.ml_world_d[6 * (row + i) + c] = wd[c]; }
            } else {
                float w[3], nv[3], maxd, mind;
                lm_point(mode, A.in.kps[img * cap + i], depth[i], A.K, Twc, A.sf, A.nlevels, w, nv, maxd, mind, bits);
                for (int c = 0; c < 3; ++c) { A.out.mp_world[3 * (row + i) + c] = w[c]; A.out.mp_normal[3 * (row + i) + c] = nv[c]; }
                A.out.mp_maxd[row + i] = maxd; A.out.mp_mind[row + i] = mind;
            }
        }
        n_created += step;
        __syncthreads();
    }
    for (int q = n_created + tid; q < cap; q += KF_THREADS) created_order[q] = -1;
    if (bits) atomicOr(A.out.status + j, bits);
    if (tid == 0) { A.out.n_visited[2 * (size_t)j + half] = n_visit; A.out.n_created[2 * (size_t)j + half] = n_created; }
}

struct KeyFrameTestArgs {
    olf_keyframe_test_batch in;
    olf_keyframe_test_outputs out;
    int cap, lcap, n_frames;
};

__global__ __launch_bounds__(KF_THREADS) void k_need_new_keyframe(KeyFrameTestArgs A)
{
    __shared__ int s_cnt[4], s_bits;
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const size_t img = (size_t)j * A.in.img_stride, row = (size_t)j * A.cap, lrow = (size_t)j * A.lcap;
    const int* r = A.in.rows + (size_t)KF_ROW * j;
    if (tid < 4) s_cnt[tid] = 0;
    if (tid == 0) s_bits = 0;
    __syncthreads();
    int c[4] = {0, 0, 0, 0}, bits = 0;
    if (!r[KF_MONOCULAR]) {                                          // (uniform)
        const int N = min(max(A.in.counts[img], 0), A.cap), Nl = min(max(A.in.lcounts[img], 0), A.lcap);
        for (int i = tid; i < N; i += KF_THREADS) {
            const int k = kf_point_class(A.in.depth[row + i], A.in.thDepth, A.in.frame_mp && A.in.frame_mp[row + i] >= 0, A.in.outlier && A.in.outlier[row + i]);
            c[0] += k == 1; c[1] += k == 2;
        }
        const int lf = A.in.ldisp_frame ? A.in.ldisp_frame[j] : j;
        const int Nd = lf >= 0 && lf < A.n_frames ? min(max(A.in.lcounts[(size_t)lf * A.in.img_stride], 0), A.lcap) : 0;
        for (int i = tid; i < Nl; i += KF_THREADS) {
            if (i >= Nd) { bits |= KF_ST_LDISP_RANGE; continue; }
            const float* d = A.in.ldisp + 2 * ((size_t)lf * A.lcap + i);
            const int k = kf_line_class(A.in.mbf, d[0], d[1], A.in.thDepth, A.in.frame_ml && A.in.frame_ml[lrow + i] >= 0, A.in.outlier_l && A.in.outlier_l[lrow + i]);
            c[2] += k == 1; c[3] += k == 2;
        }
    }
    for (int k = 0; k < 4; ++k) { const int s = wave_sum_i32(c[k]); if (lane == 0 && s) atomicAdd(&s_cnt[k], s); }
    if (bits) atomicOr(&s_bits, bits);
    __syncthreads();
    if (tid == 0) {
        const int cnt[4] = {s_cnt[0], s_cnt[1], s_cnt[2], s_cnt[3]};
        int interrupt, cond;
        const bool need = kf_need_new_keyframe(r, A.in.n_ref_matches[j], A.in.n_ref_matches_l[j], A.in.n_inliers[2 * (size_t)j], A.in.n_inliers[2 * (size_t)j + 1], cnt,
                                               interrupt, cond);
        A.out.need[j] = need ? 1 : 0;
        A.out.interrupt_ba[j] = (uint8_t)interrupt;
        for (int k = 0; k < 4; ++k) A.out.counts[4 * (size_t)j + k] = cnt[k];
        A.out.conditions[j] = cond;
        A.out.status[j] = s_bits;
    }
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_stereo_landmarks_batch_dev(olf_ctx* c, const olf_landmarks_batch* in, int n_frames, int mode, const olf_landmarks_outputs* out, void* stream)
{
    const char* who = "olf_stereo_landmarks_batch_dev";
    if (!c || !lm_args_ok(in, n_frames, mode, out)) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    LandmarkArgs A;
    A.in = *in; A.out = *out; A.mode = mode;
    A.cap = olf_orb_capacity(c); A.lcap = olf_line_capacity(c);
    if (A.cap > OLF_GRID_MAX_KEYS || A.lcap > OLF_GRID_MAX_KEYS) { set_error(std::string(who) + ": more than OLF_GRID_MAX_KEYS key points or key lines per frame"); return OLF_ERR_CAPACITY; }
    if (n_frames == 0) return OLF_OK;
    A.nlevels = ctx_level_scales(c, A.sf);
    A.K = landmark_cam(in->fx, in->fy, in->cx, in->cy, in->mbf);
    int p2 = 2;
    while (p2 < std::max(A.cap, A.lcap)) p2 <<= 1;
    // 8192 slots are 64 KB of dynamic LDS beside the kernel's few static words: above the 64 KB a launch gets unasked, so that size (the only one above
    // 32 KB: p2 is a power of two) is allowed once per device.  The attribute bounds the dynamic part alone.
    const int lds = p2 * (int)sizeof(unsigned long long);
    if (lds >= 64 * 1024) OLF_TRY(allow_large_lds(reinterpret_cast<const void*>(k_stereo_landmarks), lds));
    hipStream_t s = ctx_stream(c, stream);
    OLF_HIP_CHECK(hipMemsetAsync(out->status, 0, (size_t)n_frames * 4, s));
    hipLaunchKernelGGL(k_stereo_landmarks, dim3(2, n_frames), dim3(KF_THREADS), lds, s, A);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_need_new_keyframe_batch_dev(olf_ctx* c, const olf_keyframe_test_batch* in, int n_frames, const olf_keyframe_test_outputs* out, void* stream)
{
    const char* who = "olf_need_new_keyframe_batch_dev";
    if (!c || !kf_args_ok(in, n_frames, out)) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    KeyFrameTestArgs A;
    A.in = *in; A.out = *out; A.n_frames = n_frames;
    A.cap = olf_orb_capacity(c); A.lcap = olf_line_capacity(c);
    if (A.cap > OLF_GRID_MAX_KEYS || A.lcap > OLF_GRID_MAX_KEYS) { set_error(std::string(who) + ": more than OLF_GRID_MAX_KEYS key points or key lines per frame"); return OLF_ERR_CAPACITY; }
    if (n_frames == 0) return OLF_OK;
    hipLaunchKernelGGL(k_need_new_keyframe, dim3(n_frames), dim3(KF_THREADS), 0, ctx_stream(c, stream), A);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
