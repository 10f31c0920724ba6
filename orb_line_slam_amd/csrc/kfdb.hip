// kfdb.hip -- place recognition on gfx950: the data-parallel half of KeyFrameDatabase's four Detect members and DBoW2's L1 score.
//   the walk of the inverted file    src/KeyFrameDatabase.cc:117-135, :246-284, :410-425, :528-560   (common-word counts, first encounter)
//   L1Scoring::score                 Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68                  (called at :164, :334-335, :452, :605-606)
// for a batch of queries against every key frame (slot) of the database, and the score alone for a list of pairs (src/LoopClosing.cc:126-144).
//
// One wave per (query, slot).  A block stages its query's word ids in LDS once (at most OLF_KFDB_MAX_WORDS ids = 16 KB) and its four waves take
// kKfdbSlotsPerBlock slots between them.  The 64 lanes take 64 consecutive words of the key frame's vector and each looks its word up in the query by
// binary search (LDS; at most 13 steps).  The hits of those 64 words are then added to the score by the whole wave in lane order -- ascending word id -- one
// after the other: the ballot of the hits is walked bit by bit and each term is read from its lane.  The sum is therefore the reference's sequential
// double sum, term for term; nothing is reduced by tree or butterfly.  The term is the reference's expression (the build keeps -ffp-contract=off).
// Every loop is bounded by a vector length or by 64.  With ~1500-word vectors over 10^6 word ids a pair has two or three common words, so the serial part
// is a few iterations and the time is the look-ups'.
// (The alternative shape, a device-side inverted file with atomic counts, gives the counts cheaply but not the scores: they need the pair's common words
// in ascending order anyway, which is this kernel's search.  It was not built.)
#include "olf_internal.hpp"
#include "../../include/orbline.h"

namespace olf {

constexpr int kKfdbSlotsPerBlock = 16;

__device__ __forceinline__ double wave_read_f64(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// score(v1 = the na words at aid / aval, v2 = the nb words at bid / bval) by one wave; every lane returns the same three values.
// AIds: a pointer to v1's ids in LDS or in global memory.
template <typename AIds>
__device__ __forceinline__ void l1_wave(AIds aid, const double* __restrict__ aval, int na, const int* __restrict__ bid, const double* __restrict__ bval, int nb,
                                        int lane, int& common, int& first, double& score)
{
    common = 0;
    first = -1;
    double sum = 0.0;
    for (int base = 0; base < nb; base += 64) {
        const int i = base + lane;
        const bool valid = i < nb;
        const int w = valid ? bid[i] : 0;
        int lo = 0, hi = na;                                  // lower bound of w in v1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (aid[mid] < w) lo = mid + 1; else hi = mid;
        }
        const bool found = valid && lo < na && aid[lo] == w;
        double term = 0.0;
        if (found) {
            const double vi = aval[lo], wi = bval[i];
            term = fabs(vi - wi) - fabs(vi) - fabs(wi);       // ScoringObject.cpp:41
        }
        unsigned long long m = wave_vote(found);
        while (m) {                                           // the hits of these 64 words in ascending word id
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            sum += wave_read_f64(term, b);
            if (first < 0) first = __builtin_amdgcn_readlane(w, b);
            ++common;
        }
    }
    score = -sum / 2.0;                                       // :65; no common word: -0.0
}

__global__ __launch_bounds__(256) void k_kfdb_tables(const int* __restrict__ qoff, const int* __restrict__ qids, const double* __restrict__ qvals,
                                                     const int* __restrict__ beg, const int* __restrict__ len, const int* __restrict__ kids,
                                                     const double* __restrict__ kvals, int n_slots, int blocks_per_query, int* __restrict__ common,
                                                     int* __restrict__ first, double* __restrict__ score)
{
    __shared__ int s_q[OLF_KFDB_MAX_WORDS];
    const int q = blockIdx.x / blocks_per_query, sb = blockIdx.x % blocks_per_query;
    const int q0 = qoff[q];
    const int nq = max(0, min(qoff[q + 1] - q0, OLF_KFDB_MAX_WORDS));     // (the entry has refused a longer query; this keeps the staging in bounds regardless)
    for (int i = threadIdx.x; i < nq; i += 256) s_q[i] = qids[q0 + i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = wave; j < kKfdbSlotsPerBlock; j += 4) {
        const int k = sb * kKfdbSlotsPerBlock + j;
        if (k >= n_slots) break;
        const int k0 = beg[k], nk = len[k];
        int c, f; double s;
        l1_wave(s_q, qvals + q0, nq, kids + k0, kvals + k0, nk, lane, c, f, s);
        if (lane == 0) {
            const size_t o = (size_t)q * n_slots + k;
            common[o] = c; first[o] = f; score[o] = s;
        }
    }
}

// a_len == nullptr: vector a of the first operand is [a_beg[a], a_beg[a + 1]) (a CSR of queries); else [a_beg[a], a_beg[a] + a_len[a]) (the database's slots)
__global__ __launch_bounds__(256) void k_bow_score_pairs(const int* __restrict__ pairs, int n_pairs, const int* __restrict__ a_beg, const int* __restrict__ a_len,
                                                         int n_a, const int* __restrict__ a_ids, const double* __restrict__ a_vals, const int* __restrict__ b_beg,
                                                         const int* __restrict__ b_len, int n_b, const int* __restrict__ b_ids, const double* __restrict__ b_vals,
                                                         double* __restrict__ score)
{
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n_pairs) return;
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a < 0 || a >= n_a || b < 0 || b >= n_b) {
        if (lane == 0) score[p] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const int a0 = a_beg[a], na = max(0, a_len ? a_len[a] : a_beg[a + 1] - a0), b0 = b_beg[b], nb = b_len[b];
    int c, f; double s;
    l1_wave(a_ids + a0, a_vals + a0, na, b_ids + b0, b_vals + b0, nb, lane, c, f, s);
    if (lane == 0) score[p] = s;
}

int launch_kfdb_tables(const int* d_qoff, const int* d_qids, const double* d_qvals, int n_queries, const int* d_beg, const int* d_len, const int* d_ids,
                       const double* d_vals, int n_slots, int* d_common, int* d_first, double* d_score, hipStream_t s)
{
    if (n_queries <= 0 || n_slots <= 0) return OLF_OK;
    const int bpq = (n_slots + kKfdbSlotsPerBlock - 1) / kKfdbSlotsPerBlock;
    hipLaunchKernelGGL(k_kfdb_tables, dim3((unsigned)n_queries * (unsigned)bpq), dim3(256), 0, s, d_qoff, d_qids, d_qvals, d_beg, d_len, d_ids, d_vals, n_slots,
                       bpq, d_common, d_first, d_score);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int launch_bow_score_pairs(const int* d_pairs, int n_pairs, const int* a_beg, const int* a_len, int n_a, const int* a_ids, const double* a_vals,
                           const int* b_beg, const int* b_len, int n_b, const int* b_ids, const double* b_vals, double* d_score, hipStream_t s)
{
    if (n_pairs <= 0) return OLF_OK;
    hipLaunchKernelGGL(k_bow_score_pairs, dim3((n_pairs + 3) / 4), dim3(256), 0, s, d_pairs, n_pairs, a_beg, a_len, n_a, a_ids, a_vals, b_beg, b_len, n_b,
                       b_ids, b_vals, d_score);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // namespace olf
