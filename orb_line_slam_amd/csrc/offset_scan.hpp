// offset_scan.hpp -- what the map-graph kernels (localmap_batch.hip, connections_batch.hip) share about CSR offsets: a row read with clamped ends, and
// per-row counts made into offsets by one workgroup of 1024.
#pragma once
#include "olf_internal.hpp"

#ifdef __HIPCC__
namespace olf {

constexpr int OFFSET_SCAN_THREADS = 1024;

// row k of a CSR of n rows, inside [0, offs[n]] whatever the offsets hold
__device__ __forceinline__ void lm_row(const int* __restrict__ offs, int n, int k, int& b, int& e)
{
    const int total = max(offs[n], 0);
    b = min(max(offs[k], 0), total);
    e = min(max(offs[k + 1], b), total);
}

// offs[1 .. n] holds per-row counts: make them running sums (offs[0] = 0, saturating at INT_MAX).  A total beyond `capacity` raises `bit` of *status.
// Called by every thread of a workgroup of OFFSET_SCAN_THREADS.
__device__ __forceinline__ void offset_scan(int* __restrict__ offs, int n, int capacity, int* __restrict__ status, int bit)
{
    __shared__ long long s_wave[OFFSET_SCAN_THREADS / 64];
    __shared__ long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) { s_carry = 0; offs[0] = 0; }
    __syncthreads();
    for (int b = 0; b < n; b += OFFSET_SCAN_THREADS) {
        const int i = b + tid;
        long long v = i < n ? offs[i + 1] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const long long t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
        if (lane == 63) s_wave[w] = v;
        __syncthreads();
        long long pre = s_carry;
        for (int k = 0; k < w; ++k) pre += s_wave[k];
        v += pre;
        if (i < n) offs[i + 1] = (int)(v < 0x7fffffffLL ? v : 0x7fffffffLL);
        __syncthreads();
        if (tid == OFFSET_SCAN_THREADS - 1) s_carry = v;
        __syncthreads();
    }
    if (tid == 0 && s_carry > (long long)capacity) atomicOr(status, bit);
}

}  // namespace olf
#endif
