// line_batch.hip -- the line half of tracking for a whole batch of frames on the device:
//   Frame::isInFrustum_l                                     src/Frame.cc:446-515
//   the line half of Tracking::SearchLocalPointsAndLines     src/Tracking.cc:1897-1913, :1945-2023
//   the f2f line tracking of TrackWithMotionModelWithLine    src/Tracking.cc:1305-1349 (and of the reference key frame variant, :976-1020)
// The arithmetic is that of the host forms in search_host.cpp (olf_is_in_frustum_l, olf_local_lines_assign, olf_track_lines_assign), from the same text
// (search_math.hpp: project_closed, line_turned, line_moved, line_is_mono), no contraction.
//
// The local search, per call:
//   k_ll_held      one thread per (frame, line): mvpMapLines without its bad lines (:1902-1905) and the bitmap of map lines a frame holds (:1953)
//   k_ll_frustum   one thread per entry: the skips of :1953-1956, then both end points
//   k_ll_compact   one workgroup per frame: the in-view entries in list order get ranks -- the reference's i1 into mvpLocalMapLines_InFrustum
//   k_ll_tiles     the running sum of ceil(in-view count / 256) over the frames
//   k_knn2_indexed (match.hip) kNN(2) of every frame's in-view map lines against the frame's own lines, the queries fetched through rank -> entry -> list_index
//   k_ll_gate, k_ll_finish   the loop :1976-2016 as two passes of integer reductions per (frame, i2):
// The loop depends on the order of the ranks only through "the line i2 holds now has observations" (:1981-1983).  If the holder on entry has, nothing that
// targets i2 changes.  Otherwise, among the ranks that target i2 (the disparity gate is a property of i2), let P be those that pass the position gate and f
// the smallest rank of P whose map line has observations: from f on every rank meets an observed holder and is passed over, before f every rank is
// gated -- a failure gets -1 (:2010), a pass takes i2 until the next pass.  So with f the holder is f's line and exactly the failures below f are -1;
// without f every failure is -1 and the holder is the largest rank of P (or stays).  k_ll_gate forms min(f) and max(P) with atomicMin / atomicMax,
// k_ll_finish reads them: integer reductions, the result does not depend on scheduling.
#include <algorithm>
#include "entry_lists.hpp"
#include "device_math.hpp"
#include "search_math.hpp"
#include "staging.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int LL_MAX_LINES = 4096;                  // lines per frame: the fused (distance << 12 | index) key of the kNN
constexpr int LL_NO_RANK = 0x7f7f7f7f;              // (memset 0x7f) no rank with observations passed the position gate
// what k_ll_gate found for a rank
enum : uint8_t { LL_KEEP = 0, LL_FAIL = 1, LL_PASS = 2 };

struct LineArgs {
    olf_line_batch in;
    olf_local_line_map map;
    EntryLists L;
    const int* frame_ml;
    int n_frames, n_entries, cap, mlW;               // mlW: 32-bit words of the held bitmap per frame
    float nnr;
    double dW, dH;                                   // deltaWidth, deltaHeight
};

__device__ __forceinline__ int ll_count(const olf_line_batch& in, int j, int cap)
{
    return in.lcounts ? min(max(in.lcounts[(size_t)j * in.img_stride], 0), cap) : cap;
}
__device__ __forceinline__ const olf_keyline* ll_lines(const olf_line_batch& in, int j, int cap) { return in.kls + (size_t)j * in.img_stride * cap; }

__global__ __launch_bounds__(256) void k_ll_held(LineArgs A, unsigned* __restrict__ held, int* __restrict__ frame_ml_out, int* __restrict__ status)
{
    const int j = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= A.cap) return;
    int v = -1;
    if (A.frame_ml && idx < ll_count(A.in, j, A.cap)) v = A.frame_ml[(size_t)j * A.cap + idx];
    if (v >= A.map.n_ml) { atomicOr(status, STATUS_LINE_INDEX); v = -1; }
    else if (v < 0 || A.map.bad[v]) v = -1;                            // (a bad line is dropped from its frame line, src/Tracking.cc:1902-1905)
    if (v >= 0) atomicOr(&held[(size_t)j * A.mlW + (v >> 5)], 1u << (v & 31));
    if (frame_ml_out) frame_ml_out[(size_t)j * A.cap + idx] = v;
}

__global__ __launch_bounds__(256) void k_ll_frustum(LineArgs A, const unsigned* __restrict__ held, uint8_t* __restrict__ in_view, float* __restrict__ proj4,
                                                   int* __restrict__ status)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= A.n_entries) return;
    int i = -1;
    const int j = A.L.frame_of(e, i);
    in_view[e] = 0;
    if (j < 0) return;
    if ((unsigned)i >= (unsigned)A.map.n_ml) { atomicOr(status, STATUS_LINE_INDEX); return; }
    if (held && ((held[(size_t)j * A.mlW + (i >> 5)] >> (i & 31)) & 1u)) return;   // mnLastFrameSeen == mCurrentFrame.mnId, :1953 (NULL: the frames hold nothing)
    if (A.map.bad[i]) return;                                                      // :1955
    const olf_line_batch& in = A.in;
    const float cam[4] = {in.fx, in.fy, in.cx, in.cy}, bounds[4] = {in.minX, in.maxX, in.minY, in.maxY};
    const float* T = in.Tcw + 16 * (size_t)j;
    const float* P = A.map.world + 6 * (size_t)i;
    float s[2], t[2];
    if (!project_closed(T, P, cam, bounds, s)) return;
    if (!project_closed(T, P + 3, cam, bounds, t)) return;
    in_view[e] = 1;
    *reinterpret_cast<float4*>(proj4 + 4 * (size_t)e) = make_float4(s[0], s[1], t[0], t[1]);
}

// exclusive sum over the 256 threads of a workgroup (s_w: 4 ints; two barriers); total = the sum
__device__ __forceinline__ int block_scan_256(int v, int* s_w, int& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();                                                   // (s_w of the previous round has been read)
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < 4; ++w) before += w < wv ? s_w[w] : 0;
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return before + x - v;
}

// rank_entry[b + r] = the entry of rank r of frame j, b = the start of the frame's entries; nq[j] = mvpLocalMapLines_InFrustum.size(), qbase[j] = b
__global__ __launch_bounds__(256) void k_ll_compact(LineArgs A, const uint8_t* __restrict__ in_view, int* __restrict__ rank_entry, int* __restrict__ nq,
                                                   int* __restrict__ qbase)
{
    __shared__ int s_w[4];
    const int j = blockIdx.x;
    int b, ee, n = 0;
    A.L.range(j, b, ee);
    for (int c0 = b; c0 < ee; c0 += 256) {
        const int e = c0 + (int)threadIdx.x;
        const int f = (e < ee && in_view[e]) ? 1 : 0;
        int total;
        const int r = block_scan_256(f, s_w, total);
        if (f) rank_entry[b + n + r] = e;
        n += total;
    }
    if (threadIdx.x == 0) { nq[j] = n; qbase[j] = b; }
}

__global__ __launch_bounds__(256) void k_ll_tiles(const int* __restrict__ nq, int n_frames, int* __restrict__ tile_prefix)
{
    __shared__ int s_w[4];
    int base = 0;
    for (int c0 = 0; c0 < n_frames; c0 += 256) {
        const int j = c0 + (int)threadIdx.x;
        const int t = j < n_frames ? (nq[j] + 255) >> 8 : 0;
        int total;
        const int x = block_scan_256(t, s_w, total);
        if (j < n_frames) tile_prefix[j] = base + x;
        base += total;
    }
    if (threadIdx.x == 0) tile_prefix[n_frames] = base;
}

// One thread per rank (place p = qbase[j] + rank): the ratio test of matchNNR (src/LineMatcher.cpp:54-59, as k_ratio_mutual of match.hip writes it), then
// what the loop's body does with the rank as far as the rank alone decides it.  idx0[p] becomes matches_12[rank] before the loop.
__global__ __launch_bounds__(256) void k_ll_gate(LineArgs A, const int* __restrict__ rank_entry, const int* __restrict__ nq, const int* __restrict__ frame_ml0,
                                                const float* __restrict__ proj4, int* __restrict__ idx0, const int* __restrict__ dist0,
                                                const int* __restrict__ dist1, uint8_t* __restrict__ cls, int* __restrict__ first_obs, int* __restrict__ last_pass)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= A.n_entries) return;
    int unused, b, ee;
    const int j = A.L.frame_of(p, unused);
    if (j < 0) return;
    A.L.range(j, b, ee);
    const int r = p - b;
    if (r < 0 || r >= nq[j]) return;
    const int nb = ll_count(A.in, j, A.cap);
    int i2 = -1;
    if (nb >= 2 && (float)dist0[p] < f_mul((float)dist1[p], A.nnr)) i2 = idx0[p];
    idx0[p] = i2;
    uint8_t c = LL_KEEP;
    if (i2 >= 0 && !line_is_mono(A.in.ldisp + 2 * (size_t)j * A.cap, i2)) {
        const int h = frame_ml0[(size_t)j * A.cap + i2];
        if (!(h >= 0 && A.map.obs[h])) {                                           // (an observed holder on entry: nothing that targets i2 changes)
            const int e = rank_entry[p];
            const int mi = A.L.index ? A.L.index[e] : e - b;
            const float4 q = *reinterpret_cast<const float4*>(proj4 + 4 * (size_t)e);
            if (line_moved(ll_lines(A.in, j, A.cap)[i2], q.x, q.y, q.z, q.w, A.dW, A.dH)) c = LL_FAIL;
            else {
                c = LL_PASS;
                atomicMax(&last_pass[(size_t)j * A.cap + i2], r);
                if (A.map.obs[mi]) atomicMin(&first_obs[(size_t)j * A.cap + i2], r);
            }
        }
    }
    cls[p] = c;
}

// per rank: matches_12 at the end, written at the rank's entry; per (frame, i2): mvpMapLines at the end, and n_inliers_ls
__global__ __launch_bounds__(256) void k_ll_finish(LineArgs A, const int* __restrict__ rank_entry, const int* __restrict__ nq, const int* __restrict__ idx0,
                                                  const uint8_t* __restrict__ cls, const int* __restrict__ first_obs, const int* __restrict__ last_pass,
                                                  int* __restrict__ m12, int* __restrict__ frame_ml_out, int* __restrict__ ninliers)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < A.n_entries) {
        int unused, b, ee;
        const int j = A.L.frame_of(p, unused);
        if (j >= 0) {
            A.L.range(j, b, ee);
            const int r = p - b;
            if (r >= 0 && r < nq[j]) {
                int i2 = idx0[p];
                if (cls[p] == LL_FAIL && r < first_obs[(size_t)j * A.cap + i2]) i2 = -1;
                m12[rank_entry[p]] = i2;
            }
        }
    }
    bool holds = false;
    int j = 0;
    if (p < A.n_frames * A.cap) {
        j = p / A.cap;
        const int i2 = p - j * A.cap;
        int r = first_obs[p];
        if (r == LL_NO_RANK) r = last_pass[p];
        int h = frame_ml_out[p];
        if (r >= 0) {
            int b, ee;
            A.L.range(j, b, ee);
            const int e = rank_entry[b + r];
            h = A.L.index ? A.L.index[e] : e - b;
            frame_ml_out[p] = h;
        }
        holds = h >= 0 && i2 < ll_count(A.in, j, A.cap);
    }
    // one atomic per frame a wave touches (a wave straddles frames wherever the capacity is no multiple of 64)
    unsigned long long todo = wave_vote(holds);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        const int jl = __shfl(j, l, 64);
        const unsigned long long m = wave_vote(holds && j == jl);
        if ((int)(threadIdx.x & 63) == l) atomicAdd(&ninliers[jl], __popcll(m));
        todo &= ~m;
    }
}

// The gates and the assignment of the f2f line tracking behind match() (launch_match_bf), one workgroup per pair; dynamic LDS: cap ints (the largest i1 that
// takes i2 -- the loop runs i1 upwards and the last assignment stays).
struct TrackLineArgs {
    olf_line_batch in;
    const int *last_ml, *enable, *m12_knn;
    int cap, knn_stride, skip_null, gates;
    double dA, dW, dH;
};

__global__ __launch_bounds__(256) void k_lt_assign(TrackLineArgs A, int* __restrict__ m12, int* __restrict__ cur_ml, int* __restrict__ ninliers)
{
    extern __shared__ int s_win[];
    __shared__ int s_n;
    const int j = blockIdx.x, tid = threadIdx.x, cap = A.cap;
    if (A.enable && A.enable[j] == 0) return;
    const int nl = ll_count(A.in, j, cap), nc = ll_count(A.in, j + 1, cap);
    const olf_keyline* kl = ll_lines(A.in, j, cap);
    const olf_keyline* kc = ll_lines(A.in, j + 1, cap);
    const float* disp = A.in.ldisp + 2 * (size_t)(j + 1) * cap;
    const int* lml = A.last_ml + (size_t)j * cap;
    for (int i = tid; i < cap; i += 256) s_win[i] = -1;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int i1 = tid; i1 < cap; i1 += 256) {
        int i2 = -1;
        if (i1 < nl) {
            i2 = A.m12_knn[(size_t)j * A.knn_stride + i1];
            if (i2 >= nc) i2 = -1;
            const bool skip = (A.skip_null && lml[i1] < 0) || i2 < 0 || line_is_mono(disp, i2);
            if (!skip) {
                const olf_keyline& l = kl[i1];
                if (A.gates && (line_turned(kc[i2].angle, l.angle, A.dA) ||
                                line_moved(kc[i2], l.startPointX, l.startPointY, l.endPointX, l.endPointY, A.dW, A.dH))) i2 = -1;
                else { atomicMax(&s_win[i2], i1); atomicAdd(&s_n, 1); }
            }
        }
        m12[(size_t)j * cap + i1] = i2;
    }
    __syncthreads();
    for (int i2 = tid; i2 < cap; i2 += 256) {
        const int w = s_win[i2];
        cur_ml[(size_t)j * cap + i2] = w >= 0 ? max(lml[w], -1) : -1;
    }
    if (tid == 0) ninliers[j] = s_n;
}

}  // namespace olf

using namespace olf;

namespace {

int line_capacity_checked(olf_ctx* c, const std::string& w, int& cap)
{
    cap = olf_line_capacity(c);
    if (cap > LL_MAX_LINES) { set_error(w + ": more than 4096 key lines per frame (the matcher's key holds 12 index bits)"); return OLF_ERR_CAPACITY; }
    return OLF_OK;
}

// the checks and the argument block the two local entries share; n_entries is formed here when the map carries no lists
int line_args(olf_ctx* c, const char* who, const olf_line_batch* in, int n_frames, const olf_local_line_map* map, const int32_t* d_frame_ml, bool search, LineArgs& A)
{
    const std::string w(who);
    if (!c || !in || !map || n_frames < 0 || map->n_ml < 0 || !in->Tcw || !(in->maxX > in->minX) || !(in->maxY > in->minY) ||
        (map->n_ml && (!map->world || !map->bad)) || (map->list_offsets && (map->n_entries < 0 || (map->n_entries && !map->list_index))) ||
        ((d_frame_ml || search) && in->lcounts && in->img_stride < 1) ||
        (search && (!in->kls || !in->ldesc || !in->lcounts || !in->ldisp || (map->n_ml && (!map->desc || !map->obs))))) {
        set_error(w + ": bad argument"); return OLF_ERR_INVALID;
    }
    OLF_TRY(ctx_check_device(c, who));
    int cap;
    OLF_TRY(line_capacity_checked(c, w, cap));
    const long long ne = map->list_offsets ? (long long)map->n_entries : (long long)n_frames * map->n_ml;
    if (ne > 0x7fffffffLL - 256 || (long long)n_frames * cap > 0x7fffffffLL - 256) { set_error(w + ": more than 2^31 entries"); return OLF_ERR_CAPACITY; }
    A.in = *in; A.map = *map;
    A.L = {map->list_offsets, map->list_index, map->n_ml, n_frames, (int)ne};
    A.frame_ml = d_frame_ml;
    A.n_frames = n_frames; A.n_entries = (int)ne; A.cap = cap;
    A.mlW = (map->n_ml + 31) / 32;
    A.nnr = 0.f;
    A.dW = (double)(in->maxX - in->minX) * 0.1; A.dH = (double)(in->maxY - in->minY) * 0.1;      // src/Tracking.cc:1974-1975
    return OLF_OK;
}

// the held bitmap (and mvpMapLines without its bad lines), then the frustum pass.  Frames that hold nothing (no d_frame_ml) need no bitmap: it is neither
// cleared nor read, and mvpMapLines, where asked for, is all -1
int launch_line_frustum(olf_ctx* c, const LineArgs& A, unsigned* held, int* frame_ml_out, uint8_t* in_view, float* proj4, hipStream_t s)
{
    const size_t bh = (size_t)A.n_frames * A.mlW * 4;
    if (A.frame_ml) {
        if (bh) OLF_HIP_CHECK(hipMemsetAsync(held, 0, bh, s));
        hipLaunchKernelGGL(k_ll_held, dim3((A.cap + 255) / 256, A.n_frames), dim3(256), 0, s, A, held, frame_ml_out, ctx_status(c));
    } else if (frame_ml_out) OLF_HIP_CHECK(hipMemsetAsync(frame_ml_out, 0xff, (size_t)A.n_frames * A.cap * 4, s));
    if (A.n_entries) hipLaunchKernelGGL(k_ll_frustum, dim3((A.n_entries + 255) / 256), dim3(256), 0, s, A, A.frame_ml ? held : nullptr, in_view, proj4, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // namespace

extern "C" {

int olf_is_in_frustum_l_batch_dev(olf_ctx* c, const olf_line_batch* in, int n_frames, const olf_local_line_map* map, const int32_t* d_frame_ml,
                                  uint8_t* d_in_view, float* d_proj4, void* stream)
{
    LineArgs A;
    OLF_TRY(line_args(c, "olf_is_in_frustum_l_batch_dev", in, n_frames, map, d_frame_ml, false, A));
    if (n_frames == 0 || A.n_entries == 0) return OLF_OK;
    if (!d_in_view || !d_proj4) { set_error("olf_is_in_frustum_l_batch_dev: bad argument"); return OLF_ERR_INVALID; }
    hipStream_t s = ctx_stream(c, stream);
    if (d_frame_ml) OLF_TRY(ctx_join_line_outputs(c, s, in->lcounts, nullptr, nullptr, nullptr));
    unsigned* held;
    Carve k;
    k.add(&held, d_frame_ml ? (size_t)n_frames * A.mlW : 0);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    return launch_line_frustum(c, A, held, nullptr, d_in_view, d_proj4, s);
}

int olf_search_local_lines_batch_dev(olf_ctx* c, const olf_line_batch* in, int n_frames, const olf_local_line_map* map, const int32_t* d_frame_ml, float nnr,
                                     uint8_t* d_in_view, float* d_proj4, int32_t* d_m12, int32_t* d_frame_ml_out, int32_t* d_ninliers, void* stream)
{
    LineArgs A;
    OLF_TRY(line_args(c, "olf_search_local_lines_batch_dev", in, n_frames, map, d_frame_ml, true, A));
    if (!d_frame_ml_out || !d_ninliers || (A.n_entries && (!d_in_view || !d_proj4 || !d_m12))) { set_error("olf_search_local_lines_batch_dev: bad argument"); return OLF_ERR_INVALID; }
    if (n_frames == 0) return OLF_OK;
    A.nnr = nnr;
    hipStream_t s = ctx_stream(c, stream);
    OLF_TRY(ctx_join_line_outputs(c, s, in->kls, in->ldesc, in->lcounts, in->ldisp));
    // scratch, 17 bytes per entry: rank -> entry (4), the kNN's index and two distances (12), what the gate found (1); 8 bytes per (frame, line): the two
    // reductions; one bit per (frame, map line) when the frames hold lines; three ints per frame
    const size_t ne = (size_t)A.n_entries, nl = (size_t)n_frames * A.cap;
    int *rank_entry, *knn, *reduced, *per_frame;
    uint8_t* cls;
    unsigned* held;
    Carve k;
    k.add(&rank_entry, ne); k.add(&knn, 3 * ne); k.add(&reduced, 2 * nl); k.add(&per_frame, 3 * (size_t)n_frames + 1);
    k.add(&held, d_frame_ml ? (size_t)n_frames * A.mlW : 0); k.add(&cls, ne);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    int *idx0 = knn, *dist0 = knn + ne, *dist1 = knn + 2 * ne, *first_obs = reduced, *last_pass = reduced + nl;
    int *nq = per_frame, *qbase = per_frame + n_frames, *tile_prefix = per_frame + 2 * (size_t)n_frames;
    OLF_TRY(launch_line_frustum(c, A, held, d_frame_ml_out, d_in_view, d_proj4, s));
    OLF_HIP_CHECK(hipMemsetAsync(first_obs, 0x7f, nl * 4, s));
    OLF_HIP_CHECK(hipMemsetAsync(last_pass, 0xff, nl * 4, s));
    OLF_HIP_CHECK(hipMemsetAsync(d_ninliers, 0, (size_t)n_frames * 4, s));
    if (ne) {
        OLF_HIP_CHECK(hipMemsetAsync(d_m12, 0xff, ne * 4, s));
        hipLaunchKernelGGL(k_ll_compact, dim3(n_frames), dim3(256), 0, s, A, d_in_view, rank_entry, nq, qbase);
        hipLaunchKernelGGL(k_ll_tiles, dim3(1), dim3(256), 0, s, nq, n_frames, tile_prefix);
        // the in-view count of a frame exists on the device only: sum of ceil(count / 256) <= n_entries / 256 + n_frames
        OLF_TRY(launch_knn2_indexed(map->desc, rank_entry, map->list_offsets ? map->list_index : nullptr, qbase, nq, tile_prefix, n_frames,
                                    A.n_entries / 256 + n_frames, in->ldesc, in->lcounts, in->img_stride * A.cap, in->img_stride, A.cap, idx0, dist0, dist1, s));
        hipLaunchKernelGGL(k_ll_gate, dim3((A.n_entries + 255) / 256), dim3(256), 0, s, A, rank_entry, nq, d_frame_ml_out, d_proj4, idx0, dist0, dist1, cls,
                           first_obs, last_pass);
    }
    const size_t nt = std::max(ne, nl);
    hipLaunchKernelGGL(k_ll_finish, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, A, rank_entry, nq, idx0, cls, first_obs, last_pass, d_m12, d_frame_ml_out,
                       d_ninliers);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_track_lines_batch_dev(olf_ctx* c, const olf_line_batch* in, int n_frames, const int32_t* d_last_ml, float nnr, int best_lr, int skip_null, int gates,
                              double delta_angle, double pos_frac, const int32_t* d_enable, int32_t* d_m12, int32_t* d_cur_ml, int32_t* d_ninliers, void* stream)
{
    const std::string w("olf_track_lines_batch_dev");
    if (!c || !in || n_frames < 0 || !in->kls || !in->ldesc || !in->lcounts || in->img_stride < 1 || !in->ldisp || !(in->maxX > in->minX) || !(in->maxY > in->minY) ||
        !d_last_ml || !d_m12 || !d_cur_ml || !d_ninliers) {
        set_error(w + ": bad argument"); return OLF_ERR_INVALID;
    }
    OLF_TRY(ctx_check_device(c, w.c_str()));
    TrackLineArgs A;
    OLF_TRY(line_capacity_checked(c, w, A.cap));
    if (n_frames < 2) return OLF_OK;
    const int n_pairs = n_frames - 1, stride = in->img_stride * A.cap;
    hipStream_t s = ctx_stream(c, stream);
    OLF_TRY(ctx_join_line_outputs(c, s, in->kls, in->ldesc, in->lcounts, in->ldisp));
    int *ws, *m12_knn;
    Carve k;
    k.add(&ws, (size_t)6 * stride * n_pairs); k.add(&m12_knn, (size_t)stride * n_pairs);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    // match(desc_last, desc_cur, nnr, m12): set j = images j * img_stride and (j + 1) * img_stride of the same arrays
    const size_t next = (size_t)stride * OLF_DESC_BYTES;
    OLF_TRY(launch_match_bf(in->ldesc, in->lcounts, stride, in->img_stride, in->ldesc + next, in->lcounts + in->img_stride, stride, in->img_stride, n_pairs, nnr,
                            best_lr, ws, m12_knn, s));
    A.in = *in; A.last_ml = d_last_ml; A.enable = d_enable; A.m12_knn = m12_knn;
    A.knn_stride = stride; A.skip_null = skip_null; A.gates = gates;
    A.dA = delta_angle;
    A.dW = (double)(in->maxX - in->minX) * pos_frac; A.dH = (double)(in->maxY - in->minY) * pos_frac;
    hipLaunchKernelGGL(k_lt_assign, dim3(n_pairs), dim3(256), (size_t)A.cap * 4, s, A, d_m12, d_cur_ml, d_ninliers);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
