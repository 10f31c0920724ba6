// connections_batch.hip -- KeyFrame::UpdateConnections (src/KeyFrame.cc:446-557) for a list of key frames against one snapshot of the map (olf_map_graph,
// include/orbline.h), each computed as its own call would compute it from the map as it stands, and KeyFrame::UpdateBestCovisibles (:216-235) for a batch
// of rows.  Integers only: the results are the reference's, element for element, under convention C.16 (ascending key-frame index stands for the address
// order of std::map<KeyFrame*,int>).  One workgroup per listed key frame:
//   k_conn_count  the votes of the key frame's slots (:461-479) into an LDS table (integer LDS atomics: the sums do not depend on arrival order); the table
//                 goes to scratch as it is; KFcounter.size(), the number of key frames at or above th, and pKFmax = the most votes, lowest index on ties
//   k_conn_scan   the two per-key-frame counts into the two offset arrays; a total beyond its capacity raises STATUS_CONNECTIONS_LIST
//   k_conn_fill   the table again: KFcounter by an ordered compaction over ascending index, the key frames at or above th (or the one fallback pair) into
//                 LDS as 64-bit keys (weight, index), sorted descending (conn_sort), to their place
// The slot walk, the compaction step, the pKFmax key and the listed key frame are map_kernels.hpp's ("What the map-side kernels share").
// A weight is bounded by the length of a slot row only, so a sort key is 64 bits.  Scratch between the passes: 4 bytes per (listed key frame, key frame).
#include <algorithm>
#include "batch_frames.hpp"
#include "map_kernels.hpp"
#include "staging.hpp"      // Carve

namespace olf {

constexpr int CN_THREADS = 256, CN_WAVES = CN_THREADS / 64;
constexpr int CN_CHUNK = CN_THREADS * SLOT_PER;                // slots per chunk of the vote walk
constexpr int CN_SORT_MAX = OLF_LOCALMAP_MAX_KF;               // keys a workgroup sorts: 64 KB of the CU's 160 KB of LDS, two workgroups per CU

struct ConnArgs {
    olf_map_graph g;
    int n_list, th;
    const int* kf_list;
    int *n_counted, *kf_max, *w_max;
    int *conn_offsets, *conn_index, *conn_weight, *covis_offsets, *covis_index, *covis_weight;
    int conn_capacity, covis_capacity;
    int* votes;                                                // [n_list][n_kf] in scratch: KFcounter between the passes, 0 = not counted
};

// (weight, index) as pair<int, KeyFrame*> compares (C.16), in one unsigned word
__device__ __forceinline__ unsigned long long conn_key(int weight, int index)
{
    return ((unsigned long long)((unsigned)weight ^ 0x80000000u) << 32) | ((unsigned)index ^ 0x80000000u);
}
__device__ __forceinline__ int conn_key_weight(unsigned long long k) { return (int)((unsigned)(k >> 32) ^ 0x80000000u); }
__device__ __forceinline__ int conn_key_index(unsigned long long k) { return (int)((unsigned)k ^ 0x80000000u); }

// s[0 .. n) descending, by the whole workgroup: sort(vPairs) followed by the push_front loop (:532-539, :224-231).  A bitonic network whose merges begin
// with a flip, so that every comparator puts the larger key at the lower place: the places from n up to the next power of two stand for keys below every
// real one, never move and so are never stored.  The keys of a row are unique (a key frame appears once), so the order is the one answer.
__device__ __forceinline__ void conn_sort(unsigned long long* s, int n)
{
    int logp = 0;
    while ((1 << logp) < n) ++logp;
    const int half_p = (1 << logp) >> 1;
    __syncthreads();
    for (int lk = 1; lk <= logp; ++lk) {
        for (int lj = lk - 1; lj >= 0; --lj) {                       // pairs at distance 2^lj inside blocks of 2^lk; the first step of a merge flips
            for (int p = threadIdx.x; p < half_p; p += CN_THREADS) {
                const int r = p & ((1 << lj) - 1);
                const int lo = ((p >> lj) << (lj + 1)) + r;
                const int hi = lj == lk - 1 ? lo + ((1 << lk) - 1 - 2 * r) : lo + (1 << lj);
                if (hi < n) {
                    const unsigned long long a = s[lo], b = s[hi];
                    if (a < b) { s[lo] = b; s[hi] = a; }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(CN_THREADS) void k_conn_count(ConnArgs A, int* __restrict__ status)
{
    __shared__ int s_votes[OLF_LOCALMAP_MAX_KF];
    __shared__ unsigned long long s_best;
    __shared__ int s_counted, s_strong;
    const olf_map_graph& g = A.g;
    const int j = blockIdx.x, tid = threadIdx.x, n_kf = g.n_kf;
    int kf;
    if (!listed_kf(A.kf_list, j, n_kf, kf)) {                        // (the whole workgroup: kf is uniform)
        if (tid == 0) {
            atomicOr(status, STATUS_KF_INDEX);
            A.n_counted[j] = 0; A.kf_max[j] = -1; A.w_max[j] = 0; A.conn_offsets[j + 1] = 0; A.covis_offsets[j + 1] = 0;
        }
        return;
    }
    for (int k = tid; k < n_kf; k += CN_THREADS) s_votes[k] = 0;
    if (tid == 0) { s_best = 0; s_counted = 0; s_strong = 0; }
    __syncthreads();

    // ---- the votes, :461-479: the slots by chunks (SlotChunk), then each point's observations ----
    int b, e;
    csr_row(g.kf_mp_offsets, n_kf, kf, b, e);
    const int obs_total = max(g.mp_obs_offsets[g.n_mp], 0);
    for (int c0 = b; c0 < e; c0 += CN_CHUNK) {
        SlotChunk<SLOT_PER, CN_THREADS> C;
        C.take(g.kf_mp_index, c0, e, g.n_mp, g.mp_bad, g.mp_obs_offsets, obs_total, status, STATUS_POINT_INDEX, [](int) { return true; });
#pragma unroll
        for (int k = 0; k < SLOT_PER; ++k) {
            for (int o = C.ob[k]; o < C.oe[k]; o += SLOT_OBS) {
                int q[SLOT_OBS];
#pragma unroll
                for (int t = 0; t < SLOT_OBS; ++t) q[t] = o + t < C.oe[k] ? g.mp_obs_kf[o + t] : kf;      // (past the row: the key frame itself, which gets nothing)
#pragma unroll
                for (int t = 0; t < SLOT_OBS; ++t) {
                    if ((unsigned)q[t] >= (unsigned)n_kf) atomicOr(status, STATUS_KF_INDEX);
                    else if (q[t] != kf) atomicAdd(&s_votes[q[t]], 1);                                // mnId == mnId, :475
                }
            }
        }
    }
    __syncthreads();

    // ---- KFcounter.size(), the key frames at or above th, pKFmax (:512-518); the table to scratch ----
    int* row = A.votes + (size_t)j * n_kf;
    int counted = 0, strong = 0;
    unsigned long long best = 0;
    for (int k = tid; k < n_kf; k += CN_THREADS) {
        const int votes = s_votes[k];
        row[k] = votes;
        counted += votes > 0;
        strong += votes >= A.th;
        if (votes > 0) best = max(best, vote_key(votes, k));
    }
    counted = wave_sum_i32(counted);
    strong = wave_sum_i32(strong);
    if ((tid & 63) == 0) { atomicAdd(&s_counted, counted); atomicAdd(&s_strong, strong); }
    if (best) atomicMax(&s_best, best);
    __syncthreads();
    if (tid == 0) {
        A.n_counted[j] = s_counted;
        A.kf_max[j] = vote_key_kf(s_best);
        A.w_max[j] = vote_key_votes(s_best);
        A.conn_offsets[j + 1] = s_counted;
        A.covis_offsets[j + 1] = s_strong ? s_strong : s_counted ? 1 : 0;      // (:526-530: nobody at or above th leaves the one pair (nmax, pKFmax))
    }
}

// block 0: conn_offsets, block 1: covis_offsets
__global__ __launch_bounds__(OFFSET_SCAN_THREADS) void k_conn_scan(int* __restrict__ conn_offsets, int* __restrict__ covis_offsets, int n, int conn_capacity,
                                                                    int covis_capacity, int* __restrict__ status)
{
    offset_scan(blockIdx.x == 0 ? conn_offsets : covis_offsets, n, blockIdx.x == 0 ? conn_capacity : covis_capacity, status, STATUS_CONNECTIONS_LIST);
}

__global__ __launch_bounds__(CN_THREADS) void k_conn_fill(ConnArgs A)
{
    __shared__ unsigned long long s_keys[CN_SORT_MAX];
    __shared__ int s_cnt[2][CN_WAVES];
    const int j = blockIdx.x, tid = threadIdx.x, n_kf = A.g.n_kf;
    if (A.n_counted[j] == 0) return;                                 // (:501; also a listed index outside the graph)
    const int* row = A.votes + (size_t)j * n_kf;
    const long long c0 = A.conn_offsets[j], v0 = A.covis_offsets[j];
    int counted = 0, strong = 0;
    for (int k0 = 0; k0 < n_kf; k0 += CN_THREADS) {
        const int k = k0 + tid;
        const int votes = k < n_kf ? row[k] : 0;
        const bool p[2] = {votes > 0, votes >= A.th};
        int rank[2], n[2];
        block_rank<CN_WAVES, 2>(p, s_cnt, rank, n);
        const int at = counted + rank[0], sat = strong + rank[1];
        counted += n[0]; strong += n[1];
        if (votes > 0 && c0 + at < (long long)A.conn_capacity) { A.conn_index[c0 + at] = k; A.conn_weight[c0 + at] = votes; }
        if (votes >= A.th) s_keys[sat] = conn_key(votes, k);        // (sat < n_kf <= CN_SORT_MAX)
        __syncthreads();
    }
    if (strong == 0) {                                               // :526-530
        if (tid == 0) s_keys[0] = conn_key(A.w_max[j], A.kf_max[j]);
        strong = 1;
    }
    conn_sort(s_keys, strong);
    for (int i = tid; i < strong; i += CN_THREADS)
        if (v0 + i < (long long)A.covis_capacity) { A.covis_index[v0 + i] = conn_key_index(s_keys[i]); A.covis_weight[v0 + i] = conn_key_weight(s_keys[i]); }
}

// UpdateBestCovisibles (:216-235) of row blockIdx.x: every entry kept, in the order of conn_sort, at the same offsets
__global__ __launch_bounds__(CN_THREADS) void k_best_covisibles(int n_rows, const int* __restrict__ offsets, const int* __restrict__ index, const int* __restrict__ weight,
                                                                int* __restrict__ out_index, int* __restrict__ out_weight, int* __restrict__ status)
{
    __shared__ unsigned long long s_keys[CN_SORT_MAX];
    int b, e;
    csr_row(offsets, n_rows, blockIdx.x, b, e);
    const int n = e - b, tid = threadIdx.x;
    if (n > CN_SORT_MAX) { if (tid == 0) atomicOr(status, STATUS_CONNECTIONS_LIST); return; }
    for (int i = tid; i < n; i += CN_THREADS) s_keys[i] = conn_key(weight[b + i], index[b + i]);
    conn_sort(s_keys, n);
    for (int i = tid; i < n; i += CN_THREADS) { out_index[b + i] = conn_key_index(s_keys[i]); out_weight[b + i] = conn_key_weight(s_keys[i]); }
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_update_connections_batch_dev(olf_ctx* c, const olf_map_graph* g, int n_list, const int32_t* d_kf_list, int th, int32_t* d_n_counted, int32_t* d_kf_max,
                                     int32_t* d_w_max, int32_t* d_conn_offsets, int32_t* d_conn_index, int32_t* d_conn_weight, int conn_capacity,
                                     int32_t* d_covis_offsets, int32_t* d_covis_index, int32_t* d_covis_weight, int covis_capacity, void* stream)
{
    const char* who = "olf_update_connections_batch_dev";
    bool ok = c && g && n_list >= 0 && th >= 1 && conn_capacity >= 0 && covis_capacity >= 0 && g->n_kf >= 0 && g->n_mp >= 0;
    ok = ok && d_n_counted && d_kf_max && d_w_max && d_conn_offsets && d_covis_offsets && ((d_conn_index && d_conn_weight) || !conn_capacity) &&
         ((d_covis_index && d_covis_weight) || !covis_capacity);
    ok = ok && g->kf_mp_offsets && g->mp_obs_offsets && (g->mp_bad || !g->n_mp);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (g->n_kf > OLF_LOCALMAP_MAX_KF) { set_error(std::string(who) + ": more than OLF_LOCALMAP_MAX_KF key frames (a key frame's vote table lives in LDS)"); return OLF_ERR_CAPACITY; }
    if (n_list == 0) return OLF_OK;
    if ((long long)n_list * std::max(g->n_kf, 1) > 0x7fffffffLL) { set_error(std::string(who) + ": more than 2^31 (listed key frame, key frame) pairs"); return OLF_ERR_CAPACITY; }
    ConnArgs A;
    A.g = *g;
    A.n_list = n_list; A.th = th; A.kf_list = d_kf_list;
    A.n_counted = d_n_counted; A.kf_max = d_kf_max; A.w_max = d_w_max;
    A.conn_offsets = d_conn_offsets; A.conn_index = d_conn_index; A.conn_weight = d_conn_weight; A.conn_capacity = conn_capacity;
    A.covis_offsets = d_covis_offsets; A.covis_index = d_covis_index; A.covis_weight = d_covis_weight; A.covis_capacity = covis_capacity;
    // scratch: 4 bytes per (listed key frame, key frame of the graph), the vote tables between the passes
    Carve k;
    k.add(&A.votes, (size_t)n_list * g->n_kf);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    hipStream_t s = ctx_stream(c, stream);
    hipLaunchKernelGGL(k_conn_count, dim3(n_list), dim3(CN_THREADS), 0, s, A, ctx_status(c));
    hipLaunchKernelGGL(k_conn_scan, dim3(2), dim3(OFFSET_SCAN_THREADS), 0, s, d_conn_offsets, d_covis_offsets, n_list, conn_capacity, covis_capacity, ctx_status(c));
    hipLaunchKernelGGL(k_conn_fill, dim3(n_list), dim3(CN_THREADS), 0, s, A);
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

int olf_best_covisibles_batch_dev(olf_ctx* c, int n_rows, const int32_t* d_conn_offsets, const int32_t* d_conn_index, const int32_t* d_conn_weight,
                                  int32_t* d_covis_index, int32_t* d_covis_weight, void* stream)
{
    const char* who = "olf_best_covisibles_batch_dev";
    if (!c || n_rows < 0 || !d_conn_offsets || !d_conn_index || !d_conn_weight || !d_covis_index || !d_covis_weight) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (n_rows == 0) return OLF_OK;
    hipLaunchKernelGGL(k_best_covisibles, dim3(n_rows), dim3(CN_THREADS), 0, ctx_stream(c, stream), n_rows, d_conn_offsets, d_conn_index, d_conn_weight, d_covis_index,
                       d_covis_weight, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
