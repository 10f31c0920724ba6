// wg_sums.hpp -- the workgroup sum of the one-workgroup-per-row optimisers (pose_batch.hip, posepoints_batch.hip, optsim3_batch.hip), stated once.  Each lane brings the sums
// of its own items (item i belongs to lane i % THREADS, added in ascending i); the lanes' sums are combined by an xor butterfly over the wave (both partners
// form the same sum, so every lane ends with the same bits) and the waves' sums are added in wave order.  No floating-point atomics; the shape depends on
// nothing but THREADS.
#pragma once
#include <hip/hip_runtime.h>

namespace olf {

template <int THREADS, int MAX_SUMS>
struct WgSums {
    static_assert(THREADS == 256, "four waves, added in wave order");
    struct Lds { double red[2][THREADS / 64][MAX_SUMS]; int redn[2][THREADS / 64]; };      // a kernel's __shared__ instance
    Lds* lds;
    int tid, parity;

    // the workgroup's sums of S[0 .. m) and of *n, the same bits in every lane
    __device__ void reduce(double* S, int m, int* n)
    {
        int cnt = *n;
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        for (int k = 0; k < m; ++k) {
            double v = S[k];
            for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
            S[k] = v;
        }
        const int w = tid >> 6;
        if ((tid & 63) == 0) { for (int k = 0; k < m; ++k) lds->red[parity][w][k] = S[k]; lds->redn[parity][w] = cnt; }
        __syncthreads();
        for (int k = 0; k < m; ++k) S[k] = ((lds->red[parity][0][k] + lds->red[parity][1][k]) + lds->red[parity][2][k]) + lds->red[parity][3][k];
        *n = ((lds->redn[parity][0] + lds->redn[parity][1]) + lds->redn[parity][2]) + lds->redn[parity][3];
        parity ^= 1;             // the next call writes the other buffer: whoever reaches it has passed a barrier behind every lane's reads of this one
    }
    // the workgroup's sum of one integer alone: reduce() with no doubles, so the same barrier and the same parity flip
    __device__ int count(int n)
    {
        double none[1];
        reduce(none, 0, &n);
        return n;
    }
};

}  // namespace olf
