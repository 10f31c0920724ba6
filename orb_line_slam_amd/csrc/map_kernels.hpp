// map_kernels.hpp -- what the kernels of the map side share, each stated once ("What the map-side kernels share"): the ordered compaction
// step, counts made into CSR offsets, the listed key frame, the pKFmax key, the chunked slot walk.  csr_row, live_item, status_raise: olf_internal.hpp.
#pragma once
#include "olf_internal.hpp"

#ifdef __HIPCC__
namespace olf {

// One step of an ordered compaction by a workgroup of W waves: every thread passes N predicates; rank[k] is the number of threads below this one (in
// thread order) whose predicate k is set, count[k] the workgroup's number of set predicates k.  A ballot per wave, the waves' counts through
// cnt[N][W] of the caller's LDS, no atomics.  One barrier inside; the caller keeps its running totals and puts a barrier before cnt's next use.
// (The wave's index is a scalar.  With one predicate it bounds a loop over the waves below: selecting by q < w keeps masks in scalar registers, which
// the two callers at the scalar register limit spill.  With several, all W counts are read at once and selected: the loop's latency, once per
// predicate, cost update_local_map 6 %.  DESIGN 4.5.)
template <int W, int N>
__device__ __forceinline__ void block_rank(const bool (&p)[N], int (*cnt)[W], int (&rank)[N], int (&count)[N])
{
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const unsigned long long m = wave_vote(p[k]);
        rank[k] = wave_rank_below(m);
        if (lane == 0) cnt[k][w] = __popcll(m);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        count[k] = 0;
        if (N == 1) for (int q = 0; q < w; ++q) rank[k] += cnt[k][q];
#pragma unroll
        for (int q = 0; q < W; ++q) { if (N > 1 && q < w) rank[k] += cnt[k][q]; count[k] += cnt[k][q]; }
    }
}
template <int W>
__device__ __forceinline__ int block_rank(bool p, int (*cnt)[W], int& count)
{
    const bool pp[1] = {p};
    int rank[1], n[1];
    block_rank<W, 1>(pp, cnt, rank, n);
    count = n[0];
    return rank[0];
}

constexpr int OFFSET_SCAN_THREADS = 1024;

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

// The key frame entry j of a listed call works on: kf_list[j], or j itself without a list.  false: it is outside the graph of n_kf key frames (uniform
// for a workgroup whose j is its block; what the entry writes and raises then is its own).
__device__ __forceinline__ bool listed_kf(const int* __restrict__ kf_list, int j, int n_kf, int& kf)
{
    kf = kf_list ? kf_list[j] : j;
    return (unsigned)kf < (unsigned)n_kf;
}

// pKFmax as the maximum of one unsigned word per key frame: more votes first, then -- the tie rule of C.16, ascending index standing for the address
// order of std::map<KeyFrame*,int> -- the lower index.  0: nobody (votes > 0 for every key that enters).
__device__ __forceinline__ unsigned long long vote_key(int votes, int k) { return ((unsigned long long)(unsigned)votes << 32) | (unsigned)(0x7fffffff - k); }
__device__ __forceinline__ int vote_key_kf(unsigned long long key) { return key ? 0x7fffffff - (int)(unsigned)(key & 0xffffffffu) : -1; }
__device__ __forceinline__ int vote_key_votes(unsigned long long key) { return (int)(key >> 32); }

// The chunked walk over a key frame's slot row [.., e) by a workgroup of THREADS: a chunk is PER * THREADS slots, thread t's slot k of the chunk at c0
// is c0 + k * THREADS + t (every load coalesced, the PER of a thread in flight together).  take() reads the items, decides what each slot holds
// (live_item; `keep(k)` false drops a live one) and reads the clamped observation row [ob, oe) of what is left -- item -1 and an empty row otherwise.
// The per-observation loop that follows is the kernel's own.
constexpr int SLOT_PER = 4, SLOT_OBS = 4;      // slots per thread and per chunk of a walk; observations of a point in flight per thread
template <int PER, int THREADS>
struct SlotChunk {
    int item[PER], ob[PER], oe[PER];
    static __device__ __forceinline__ int slot(int c0, int k) { return c0 + k * THREADS + (int)threadIdx.x; }
    template <class Keep>
    __device__ __forceinline__ void take(const int* __restrict__ index, int c0, int e, int n_items, const uint8_t* __restrict__ bad, const int* __restrict__ obs_offsets,
                                         int obs_total, int* __restrict__ status, int bit, Keep keep)
    {
#pragma unroll
        for (int k = 0; k < PER; ++k) { const int s = slot(c0, k); item[k] = s < e ? index[s] : -1; }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            item[k] = live_item(item[k], n_items, bad, status, bit);
            if (item[k] >= 0 && !keep(k)) item[k] = -1;
            ob[k] = 0; oe[k] = 0;
            if (item[k] >= 0) csr_clamp(obs_offsets, item[k], obs_total, ob[k], oe[k]);
        }
    }
};

}  // namespace olf
#endif
