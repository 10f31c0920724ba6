// ransac_terms.hpp -- what the two RANSAC solvers (sim3solver_terms.hpp, pnpsolver_terms.hpp) share: which row values are correspondences and how an
// iteration's draws become its sample (convention C.20).  One text for the host forms and the kernels; the results are integers.
#pragma once
#include "device_math.hpp"

namespace olf {

// is row value v of a match row a correspondence: 0 <= v < N2 (-1, -2 and >= N2 of the matchers are all "none")
OLF_HD bool s3_is_match(int v, int N2) { return (unsigned)v < (unsigned)N2; }

// C.20: a draw is a raw rand() value below 2^31; it picks position (int)(((double)r / 2147483648.0) * n) of the n indices still available
// (DUtils::Random::RandomInt with glibc's RAND_MAX).  Bit 31 of a draw is dropped: rand() never sets it, and with it the position would leave [0, n).
OLF_HD int s3_pos(uint32_t r, int n) { return (int)d_mul(d_div((double)(r & 0x7fffffffu), 2147483648.0), (double)n); }

// The K sample indices of one iteration (src/Sim3Solver.cc:163-177 with K = 3, src/PnPsolver.cc:188-201 with K = 4): vAvailableIndices starts as
// 0 .. N - 1; a drawn position takes the back's value and the back is dropped.  The array is never formed: after j draws it differs from the identity in
// at most j places -- position p[j'] holds what the back, N - 1 - j', held when draw j' was made -- so draw k's value is found by walking its position
// back through the k substitutions before it.  N >= K.
template <int K>
OLF_HD void ransac_sample(int N, const uint32_t* r, int* idx)
{
    int p[K];
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] = s3_pos(r[k], N - k);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int x = p[k];
#pragma unroll
        for (int j = k - 1; j >= 0; --j) if (x == p[j]) x = N - 1 - j;
        idx[k] = x;
    }
}

}  // namespace olf
