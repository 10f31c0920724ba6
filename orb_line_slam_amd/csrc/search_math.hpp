// search_math.hpp -- the arithmetic the host searches (search_host.cpp) and the batched device matchers (track_batch.hip, local_batch.hip, bow_match.hip)
// both run: the cv::Mat products of convention C.12 and the rotation histogram of ORBmatcher.  One text for both sides; every file that includes it is
// built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

namespace olf {

constexpr int HISTO_LENGTH = 30;                                       // src/ORBmatcher.cc:41

// cv::Mat products of CV_32F operands (convention C.12): a plain product A*b (+ c) of inner length 3 takes cv::gemm's
// small-matrix path (flags == 0, 2 <= len <= 4): the three products are summed in float, alpha and the C term are applied in double and the
// result is rounded once.  Products with a transposed operand (A.t()*b) take the generic path: double accumulation, one rounding.
__host__ __device__ __forceinline__ float dot3_small(const float* a, const float* b)
{
    float t = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];        // ((a0*b0 + a1*b1) + a2*b2) in float, no contraction (-ffp-contract=off)
    return t;
}
__host__ __device__ __forceinline__ void rot_apply(const float* T, const float* v, float alpha_t, float* out)     // R * v + alpha_t * t, T = 4x4 row-major
{
    for (int r = 0; r < 3; ++r) out[r] = (float)((double)dot3_small(T + 4 * r, v) + (double)alpha_t * (double)T[4 * r + 3]);
}
__host__ __device__ __forceinline__ void camera_centre(const float* Tcw, float* Ow)                 // -Rcw.t() * tcw
{
    for (int r = 0; r < 3; ++r) {
        double acc = 0;
        for (int k = 0; k < 3; ++k) acc += (double)Tcw[4 * k + r] * (double)Tcw[4 * k + 3];
        Ow[r] = (float)(-acc);
    }
}

// the rotation bin of a match (src/ORBmatcher.cc:1434-1441 and its siblings); angles outside [0, 360) give a bin outside [0, HISTO_LENGTH)
__host__ __device__ __forceinline__ int rot_bin(float angle1, float angle2)
{
    float rot = angle1 - angle2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / HISTO_LENGTH));
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// ORBmatcher::ComputeThreeMaxima, src/ORBmatcher.cc:1749-1790, on the sizes of the HISTO_LENGTH bins
__host__ __device__ __forceinline__ void three_maxima(const int* counts, int& ind1, int& ind2, int& ind3)
{
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = counts[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if (max3 < 0.1f * (float)max1) i3 = -1;
    ind1 = i1; ind2 = i2; ind3 = i3;
}

}  // namespace olf
