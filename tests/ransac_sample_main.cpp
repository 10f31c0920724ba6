// ransac_sample_main.cpp -- ransac_sample<3> and ransac_sample<4> (csrc/ransac_terms.hpp: the sample of a Sim3Solver / PnPsolver iteration as K - 1
// remembered substitutions) against the literal procedure of src/Sim3Solver.cc:163-177 and src/PnPsolver.cc:188-201: an array 0 .. N - 1 where a drawn
// position takes the back's value and the back is dropped.  Every N from K to 9 and every tuple of positions (p0 < N, p1 < N - 1, ...), so each position
// of each stage is reached, each tuple once with plain draws and once with bit 31 set in one of them (the bit is dropped: convention C.20).  The results
// are integers and must be equal throughout.  A stand-alone program (tests/test_sim3solver_cpu.py builds it with -fsanitize=address,undefined); prints
// "ransac_sample_main ok".
#include <cstdint>
#include <cstdio>
#include <vector>
#include "ransac_terms.hpp"

// a draw below 2^31 that picks position p of n: the middle of the draws that do
static uint32_t draw_for(int p, int n) { return (uint32_t)(((double)p + 0.5) * 2147483648.0 / (double)n); }
static int literal_pos(uint32_t r, int n) { return (int)(((double)(r & 0x7fffffffu) / 2147483648.0) * (double)n); }

template <int K>
static bool literal_equals(int N, const uint32_t* r, long* checked)
{
    std::vector<int> avail((size_t)N);
    for (int i = 0; i < N; ++i) avail[(size_t)i] = i;
    int want[K], got[K];
    for (int k = 0; k < K; ++k) {
        const int pos = literal_pos(r[k], (int)avail.size());
        want[k] = avail.at((size_t)pos);
        avail[(size_t)pos] = avail.back();
        avail.pop_back();
    }
    olf::ransac_sample<K>(N, r, got);
    for (int k = 0; k < K; ++k)
        if (got[k] != want[k]) {
            std::printf("K %d N %d draws %08x %08x %08x %08x: index %d is %d, the literal procedure gives %d\n", K, N, r[0], r[1], r[2], K > 3 ? r[3] : 0u, k, got[k], want[k]);
            return false;
        }
    ++*checked;
    return true;
}

template <int K>
static bool sweep(long* checked)
{
    for (int N = K; N <= 9; ++N) {
        int p[K] = {0};
        long tuple = 0;
        for (;;) {
            uint32_t r[4] = {0, 0, 0, 0};
            for (int k = 0; k < K; ++k) {
                r[k] = draw_for(p[k], N - k);
                if (olf::s3_pos(r[k], N - k) != p[k] || literal_pos(r[k], N - k) != p[k]) { std::printf("draw_for(%d, %d) misses its position\n", p[k], N - k); return false; }
            }
            if (!literal_equals<K>(N, r, checked)) return false;
            r[tuple % K] |= 0x80000000u;
            if (!literal_equals<K>(N, r, checked)) return false;
            ++tuple;
            int k = K - 1;                                          // the next tuple: p[k] < N - k
            while (k >= 0 && ++p[k] == N - k) p[k--] = 0;
            if (k < 0) break;
        }
    }
    return true;
}

int main()
{
    long checked = 0;
    if (!sweep<3>(&checked) || !sweep<4>(&checked)) return 1;
    // 2 * sum over N of N (N - 1) (N - 2) [(N - 3)]
    long want = 0;
    for (int N = 3; N <= 9; ++N) want += 2L * N * (N - 1) * (N - 2);
    for (int N = 4; N <= 9; ++N) want += 2L * N * (N - 1) * (N - 2) * (N - 3);
    if (checked != want) { std::printf("%ld samples checked, %ld expected\n", checked, want); return 1; }
    std::printf("ransac_sample_main ok (%ld samples)\n", checked);
    return 0;
}
