// grid.hip -- Frame::mGrid on the device (layout: include/orbline_types.h, "Frame::mGrid as two arrays").
//   k_assign_grid       Frame::AssignFeaturesToGrid + PosInGrid (src/Frame.cc:334-349, :572-582): one wave per frame, a stable counting sort of the
//                       frame's key points by cell with the OLF_GRID_CELLS counters in LDS
//   k_features_in_area  Frame::GetFeaturesInArea (src/Frame.cc:517-570) for many queries: one wave per query (the walk: grid_walk.hpp), once to count and once to fill
//   k_area_scan         the prefix sum between the two passes (one workgroup)
// Float expressions are written as the reference writes them; the library is built with -ffp-contract=off.
#include <climits>
#include "grid_walk.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int kCols = OLF_GRID_COLS, kRows = OLF_GRID_ROWS, kCells = OLF_GRID_CELLS;
constexpr unsigned short kNoCell = 0xffff;
static_assert(kCells % 64 == 0 && kCells < 4096, "the scan walks the cells 64 at a time; match_cell compares 12 bits");

bool grid_is_valid(const int32_t* offs, const int32_t* idx, int n)
{
    if (!offs || n < 0 || offs[0] != 0) return false;
    for (int c = 0; c < kCells; ++c) if (offs[c + 1] < offs[c]) return false;
    const int used = offs[kCells];
    if (used > n || (used && !idx)) return false;
    for (int k = 0; k < used; ++k) if (idx[k] < 0 || idx[k] >= n) return false;
    return true;
}

// the lanes of the wave that hold the same cell as this lane (among the lanes with `in` set); every lane of the wave calls it
__device__ __forceinline__ unsigned long long match_cell(int cell, bool in)
{
    unsigned long long m = wave_vote(in);
#pragma unroll
    for (int b = 0; b < 12; ++b) {
        const bool bit = (cell >> b) & 1;
        const unsigned long long v = wave_vote(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

__device__ __forceinline__ int wave_scan_inclusive(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
    return v;
}

// grid: one block of ONE wave per frame.  Frame j: key points kps + j * frame_stride, count counts[j * count_stride] (counts == NULL: n_fixed), clamped to
// [0, n_limit] (n_limit <= OLF_GRID_MAX_KEYS and <= index_stride).  Three phases:
//   1. every key's cell (PosInGrid) into LDS, cell sizes by LDS atomics -- integer sums, the same whatever order they land in;
//   2. exclusive scan of the sizes = the frame's cell_offsets;
//   3. the keys again in index order, 64 at a time: a key's slot is its cell's cursor plus its rank among the chunk's keys of the same cell (lane masks, 12
//      votes per chunk -- the same cost whether the 64 keys share one cell or none), then the cursors advance.  Inside a cell the indices ascend.
__global__ __launch_bounds__(64) void k_assign_grid(const olf_keypoint* __restrict__ kps, size_t frame_stride, const int* __restrict__ counts, int count_stride,
                                                    int n_fixed, int n_limit, float minX, float minY, float wInv, float hInv, int* __restrict__ cell_offsets,
                                                    int* __restrict__ cell_index, size_t index_stride)
{
    __shared__ int s_cur[kCells];
    __shared__ unsigned short s_of[OLF_GRID_MAX_KEYS];
    const int frame = blockIdx.x, lane = threadIdx.x;
    int n = counts ? counts[(size_t)frame * count_stride] : n_fixed;
    n = min(max(n, 0), n_limit);
    const olf_keypoint* k = kps + (size_t)frame * frame_stride;
    int* offs = cell_offsets + (size_t)frame * (kCells + 1);
    int* idx = cell_index + (size_t)frame * index_stride;

    for (int c = lane; c < kCells; c += 64) s_cur[c] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        // posX = round((kp.pt.x-mnMinX)*mfGridElementWidthInv): C round() on the float product, half away from zero
        const float px = roundf((k[i].x - minX) * wInv), py = roundf((k[i].y - minY) * hInv);
        const bool in = px >= 0.f && px < (float)kCols && py >= 0.f && py < (float)kRows;      // (NaN: in no cell)
        const int cell = in ? (int)px * kRows + (int)py : kNoCell;
        s_of[i] = (unsigned short)cell;
        if (in) atomicAdd(&s_cur[cell], 1);
    }
    __syncthreads();
    int carry = 0;
    for (int c0 = 0; c0 < kCells; c0 += 64) {
        const int v = s_cur[c0 + lane], inc = wave_scan_inclusive(v, lane);
        const int start = carry + inc - v;
        s_cur[c0 + lane] = start;
        offs[c0 + lane] = start;
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) offs[kCells] = carry;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const int cell = i < n ? s_of[i] : kNoCell;
        const bool in = cell != kNoCell;
        const unsigned long long m = match_cell(cell, in);
        const int rank = wave_rank_below(m), cnt = __popcll(m);
        int base = 0;
        if (in) { base = s_cur[cell]; idx[base + rank] = i; }
        __syncthreads();
        if (in && rank == cnt - 1) s_cur[cell] = base + cnt;
        __syncthreads();
    }
}

int launch_assign_grid(const olf_keypoint* d_kps, size_t frame_stride, const int* d_counts, int count_stride, int n_fixed, int n_limit, float minX,
                       float minY, float wInv, float hInv, int n_frames, int* d_cell_offsets, int* d_cell_index, size_t index_stride, hipStream_t s)
{
    if (n_frames <= 0) return OLF_OK;
    if (n_limit > OLF_GRID_MAX_KEYS || (size_t)n_limit > index_stride) { set_error("launch_assign_grid: more key points per frame than the kernel sorts"); return OLF_ERR_CAPACITY; }
    hipLaunchKernelGGL(k_assign_grid, dim3(n_frames), dim3(64), 0, s, d_kps, frame_stride, d_counts, count_stride, n_fixed, n_limit, minX, minY, wInv, hInv,
                       d_cell_offsets, d_cell_index, index_stride);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

// One wave per query, four queries per block.  fill == 0: cand_offsets[q + 1] = the number of indices GetFeaturesInArea returns for query q;
// fill != 0 (cand_offsets scanned): the indices themselves at cand_idx[cand_offsets[q] ..), in the reference's order -- ix outer, iy inner, stored order
// inside a cell (grid_walk's scan positions).  Nothing is written at or past cand_capacity.
__global__ __launch_bounds__(256) void k_features_in_area(const olf_keypoint* __restrict__ keys, const int* __restrict__ cell_offsets,
                                                          const int* __restrict__ cell_index, float minX, float minY, float wInv, float hInv,
                                                          int n_queries, const olf_area_query* __restrict__ queries, int* __restrict__ cand_offsets,
                                                          int* __restrict__ cand_idx, int cand_capacity, int fill)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= n_queries) return;                                   // (wave-uniform)
    const GridView G = {keys, cell_offsets, cell_index, INT_MAX, INT_MAX, minX, minY, wInv, hInv};      // (the entry knows neither the key count nor the index length)
    const long long out0 = fill ? cand_offsets[q] : 0;
    const int total = grid_walk(G, queries[q].x, queries[q].y, queries[q].r, queries[q].min_level, queries[q].max_level, lane, [&](bool take, int j, int pos) {
        if (fill && take) {
            const long long at = out0 + pos;
            if (at < (long long)cand_capacity) cand_idx[at] = j;
        }
    });
    if (!fill && lane == 0) cand_offsets[q + 1] = total;
}

// cand_offsets[1 .. n] holds the per-query counts: make it the running sums (cand_offsets[0] = 0); a total beyond cand_capacity raises the context's capacity
// flag (bit 128 of the status word).  One block of 1024; sums saturate at INT_MAX.
__global__ __launch_bounds__(1024) void k_area_scan(int* __restrict__ cand_offsets, int n, int cand_capacity, int* __restrict__ status)
{
    __shared__ long long s_wave[16];
    __shared__ long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) { s_carry = 0; cand_offsets[0] = 0; }
    __syncthreads();
    for (int b = 0; b < n; b += 1024) {
        const int i = b + tid;
        long long v = i < n ? cand_offsets[i + 1] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const long long t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
        if (lane == 63) s_wave[w] = v;
        __syncthreads();
        long long pre = s_carry;
        for (int k = 0; k < w; ++k) pre += s_wave[k];
        v += pre;
        if (i < n) cand_offsets[i + 1] = (int)(v < 0x7fffffffLL ? v : 0x7fffffffLL);
        __syncthreads();
        if (tid == 1023) s_carry = v;
        __syncthreads();
    }
    if (tid == 0 && s_carry > (long long)cand_capacity) atomicOr(status, 128);
}

int launch_features_in_area(const olf_keypoint* d_keys, const int* d_cell_offsets, const int* d_cell_index, float minX, float minY, float wInv, float hInv,
                            int n_queries, const olf_area_query* d_queries, int* d_cand_offsets, int* d_cand_idx, int cand_capacity, int* d_status,
                            hipStream_t s)
{
    if (n_queries == 0) { OLF_HIP_CHECK(hipMemsetAsync(d_cand_offsets, 0, sizeof(int), s)); return OLF_OK; }
    const dim3 grid((unsigned)((n_queries + 3) / 4)), block(256);
    hipLaunchKernelGGL(k_features_in_area, grid, block, 0, s, d_keys, d_cell_offsets, d_cell_index, minX, minY, wInv, hInv, n_queries, d_queries, d_cand_offsets,
                       d_cand_idx, cand_capacity, 0);
    hipLaunchKernelGGL(k_area_scan, dim3(1), dim3(1024), 0, s, d_cand_offsets, n_queries, cand_capacity, d_status);
    hipLaunchKernelGGL(k_features_in_area, grid, block, 0, s, d_keys, d_cell_offsets, d_cell_index, minX, minY, wInv, hInv, n_queries, d_queries, d_cand_offsets,
                       d_cand_idx, cand_capacity, 1);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // namespace olf
