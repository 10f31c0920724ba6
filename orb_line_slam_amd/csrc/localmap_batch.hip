// localmap_batch.hip -- Tracking::UpdateLocalMap (src/Tracking.cc:2028-2205) for a whole batch of frames against one snapshot of the map (olf_map_graph,
// include/orbline.h): UpdateLocalKeyFrames (:2080-2205), then UpdateLocalPointsAndLines (:2039-2078), emitting mvpLocalKeyFrames, mvpLocalMapPoints and
// mvpLocalMapLines of every frame as three CSR lists and mpReferenceKF.  Integers only: the results are the reference's, element for element, under
// convention C.16 (ascending key-frame index stands for the address order of std::map<KeyFrame*,int> and std::set<KeyFrame*>).  One workgroup per frame:
//   k_localmap_count  votes of the frame's held points into an LDS table (integer LDS atomics: the sums do not depend on arrival order); the first list by
//                     an ordered compaction over ascending key-frame index, pKFmax = the most votes, lowest index on ties; the extension loop (:2149-2198)
//                     by wave 0 -- over the first list only, the `> 80` test, 10 neighbours, children, the parent and its break; then the number of
//                     distinct live points and lines of the local key frames (first_seen, counting)
//   k_localmap_scan   the three per-frame counts into the three offset arrays; a total beyond its capacity raises STATUS_LOCALMAP_LIST
//   k_localmap_fill   the key-frame list to its place, then the same walk again (first_seen, filling): survivors in (key frame, slot) order
// "The first occurrence wins" is positional (first_seen): the winner among equal points of a chunk is the lowest position, decided through LDS, never by
// which atomic arrives first.  Both passes run the same walk over the same list against a bitmap in the same state, so their counts agree.  A frame's two
// bitmaps (one bit per map point, one per map line) live in LDS -- in the words of the vote table, which is done with by then -- while they fit
// LM_BITS_WORDS words; beyond that they live in scratch, where the counting pass sets the bits and the filling pass clears them again.
// The compaction step, the pKFmax key, the CSR row and the item test: map_kernels.hpp, olf_internal.hpp ("What the map-side kernels share").
#include <algorithm>
#include "batch_frames.hpp"
#include "map_kernels.hpp"
#include "staging.hpp"

namespace olf {

constexpr int LM_THREADS = 256, LM_WAVES = LM_THREADS / 64;
constexpr int LM_PER = 4, LM_CHUNK = LM_THREADS * LM_PER;      // slots per thread and per chunk of first_seen
constexpr int LM_HASH_BITS = 12, LM_HASH = 1 << LM_HASH_BITS;  // buckets of first_seen's table: four per position of a chunk
constexpr int LM_BITS_WORDS = OLF_LOCALMAP_MAX_KF;             // words of LDS for a frame's two bitmaps: the vote table's, which is done with by then
constexpr int LM_HEAD = 128;                        // leading members of the key-frame list kept in LDS: the extension loop reads at most 81 and appends below 84
constexpr int LM_ROUNDS = 8;                        // hashed rounds of first_seen before the plain scan decides what is left
static_assert(OLF_LOCALMAP_MAX_KF % 64 == 0 && OLF_LOCALMAP_MAX_KF * 4 <= 32 * 1024 && LM_CHUNK == 1024, "the vote table and the other LDS arrays of k_localmap_count stay below 64 KB; a position is 10 bits");

struct LocalMapArgs {
    olf_map_graph g;
    int n_frames, img_stride, cap, lcap;           // key points / lines per frame (olf_orb_capacity, olf_line_capacity)
    const int *counts, *lcounts, *frame_mp, *frame_ml;
    int *frame_mp_out, *frame_ml_out, *ref_kf, *n_voted;
    int *kf_offsets, *kf_index, *mp_offsets, *mp_index, *ml_offsets, *ml_index;
    int kf_capacity, mp_capacity, ml_capacity;
    int mpW, mlW;                                  // per frame: 32-bit words of the point and of the line bitmap
    int lds_bits;                                  // the two bitmaps of a frame fit LM_BITS_WORDS words of LDS: no scratch bitmap
    unsigned *seen_mp, *seen_ml;                   // otherwise [n_frames][mpW], [n_frames][mlW] in scratch, zero on entry
    int* kf_list;                                  // [n_frames][n_kf]: mvpLocalKeyFrames between the passes
};

// this wave's global writes have reached L2 (the explicit wait: the compiler may leave the fence without one)
__device__ __forceinline__ void lm_publish()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

struct SeenLds {
    unsigned table[LM_HASH];      // (round << 10 | 1023 - position), kept by atomicMax: a later round beats every earlier entry, the lowest position wins a round
    int val[LM_CHUNK];            // the chunk's candidates by position (-1: none)
    int wcnt[LM_PER][LM_WAVES];
    unsigned round;
};

// The slots index[b .. e) of one key frame (GetMapPointMatches / GetMapLineMatches as map indices) against the frame's bitmap, by the whole workgroup,
// LM_CHUNK slots per chunk in slot order: position p = k * LM_THREADS + thread of a chunk is slot c0 + p (LM_PER loads per thread, each coalesced and all in
// flight together).  A slot survives when it is not NULL, inside the map (else `bit` of *status), not bad and new.  The bitmap is `bits`:
//   LDS = true   the frame's own words in LDS, zero when the pass began: a clear bit means new, and the pass sets it;
//   LDS = false  the frame's words in scratch: the counting pass (FILL = false) finds them zero, a clear bit means new and it sets it; the filling pass finds
//                what the counting pass left, a set bit means new and it clears it.  The words are written by atomics, which act in L2, and read there.
// Among equal items of one chunk the lowest slot survives.  Survivors are numbered from `total` on in slot order; the filling pass writes survivor number r to
// out[out0 + r] when that lies below capacity.  Every thread returns the new total.
template <bool LDS, bool FILL>
__device__ __forceinline__ long long first_seen(SeenLds& S, unsigned* bits, const int* __restrict__ index, int b, int e, int n_items, const uint8_t* __restrict__ bad,
                                                int* __restrict__ status, int bit, long long total, int* __restrict__ out, long long out0, int capacity)
{
    const int tid = threadIdx.x;
    for (int c0 = b; c0 < e; c0 += LM_CHUNK) {
        if (!LDS) lm_publish();                                      // the bitmap writes of the chunk before have reached L2 ...
        __syncthreads();                                             // ... before anyone reads the bitmap again; and its LDS reads are done
        int v[LM_PER];
#pragma unroll
        for (int k = 0; k < LM_PER; ++k) { const int s = c0 + k * LM_THREADS + tid; v[k] = s < e ? index[s] : -1; }
#pragma unroll
        for (int k = 0; k < LM_PER; ++k) v[k] = live_item(v[k], n_items, bad, status, bit);
        unsigned open = 0, win = 0;                                  // per position of this thread.  open: not decided yet
#pragma unroll
        for (int k = 0; k < LM_PER; ++k) {
            if (v[k] >= 0) {
                const bool seen = LDS ? (bits[v[k] >> 5] >> (v[k] & 31)) & 1u
                                      : ((__hip_atomic_load(bits + (v[k] >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (v[k] & 31)) & 1u) != (FILL ? 1u : 0u);
                if (seen) v[k] = -1;
            }
            S.val[k * LM_THREADS + tid] = v[k];
            if (v[k] >= 0) open |= 1u << k;
        }
        for (int r = 0; ; ++r) {
            unsigned round = S.round;
            __syncthreads();                                         // (also: everyone holds `round` before thread 0 moves it)
            if (round >= (1u << 22) - 1) {                           // the tag is running out: start the table again
                for (int k = tid; k < LM_HASH; k += LM_THREADS) S.table[k] = 0;
                round = 0;
                __syncthreads();
            }
            ++round;
            if (tid == 0) S.round = round;
            if (r == LM_ROUNDS) {                                    // hashes kept colliding: the lower positions decide
#pragma unroll
                for (int k = 0; k < LM_PER; ++k) {
                    if (!((open >> k) & 1u)) continue;
                    bool first = true;
                    for (int q = 0; q < k * LM_THREADS + tid; ++q) if (S.val[q] == v[k]) { first = false; break; }
                    if (first) win |= 1u << k;
                }
                open = 0;
                break;
            }
            unsigned h[LM_PER];
#pragma unroll
            for (int k = 0; k < LM_PER; ++k) {
                h[k] = (((unsigned)v[k] ^ ((unsigned)r * 0x9e3779b9u)) * 2654435761u) >> (32 - LM_HASH_BITS);
                if ((open >> k) & 1u) atomicMax(&S.table[h[k]], (round << 10) | (unsigned)(LM_CHUNK - 1 - (k * LM_THREADS + tid)));
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < LM_PER; ++k) {
                if (!((open >> k) & 1u)) continue;
                const int m = LM_CHUNK - 1 - (int)(S.table[h[k]] & 0x3ffu);      // the lowest open position of this bucket
                if (m == k * LM_THREADS + tid) { win |= 1u << k; open &= ~(1u << k); }      // every position of an item shares its bucket, so this is the item's first
                else if (S.val[m] == v[k]) open &= ~(1u << k);       // a lower position holds the same item
            }                                                        // else another item's: all positions of this one stay open together
            if (!__syncthreads_or(open != 0)) break;
        }
        bool won[LM_PER];
        int rank[LM_PER], cnt[LM_PER];
#pragma unroll
        for (int k = 0; k < LM_PER; ++k) won[k] = (win >> k) & 1u;
        block_rank<LM_WAVES, LM_PER>(won, S.wcnt, rank, cnt);       // (the barrier at the chunk's start separates this from the next call)
        long long at[LM_PER];                                        // positions ascend with k first, then with the wave, then with the lane
#pragma unroll
        for (int k = 0; k < LM_PER; ++k) { at[k] = total + rank[k]; total += cnt[k]; }
#pragma unroll
        for (int k = 0; k < LM_PER; ++k) {
            if (!((win >> k) & 1u)) continue;
            const unsigned m = 1u << (v[k] & 31);
            if (LDS || !FILL) atomicOr(&bits[v[k] >> 5], m); else atomicAnd(&bits[v[k] >> 5], ~m);
            if (FILL && out0 + at[k] < (long long)capacity) out[out0 + at[k]] = v[k];
        }
    }
    return total;
}

// the walk of UpdateLocalPointsAndLines (:2039-2078) over the key-frame list, counting or filling; the frame's point words come first in `bits`, then its line words
template <bool LDS, bool FILL>
__device__ __forceinline__ void lm_walk(const LocalMapArgs& A, SeenLds& S, unsigned* bits_mp, unsigned* bits_ml, const int* list, const int* s_head, int size,
                                        int* __restrict__ status, long long mp0, long long ml0, long long& np, long long& nl)
{
    const olf_map_graph& g = A.g;
    for (int m = 0; m < size; ++m) {
        const int kf = s_head && m < LM_HEAD ? s_head[m] : __hip_atomic_load(list + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int b, e;
        csr_row(g.kf_mp_offsets, g.n_kf, kf, b, e);
        np = first_seen<LDS, FILL>(S, bits_mp, g.kf_mp_index, b, e, g.n_mp, g.mp_bad, status, STATUS_POINT_INDEX, np, A.mp_index, mp0, A.mp_capacity);
        if (g.n_ml > 0) {
            csr_row(g.kf_ml_offsets, g.n_kf, kf, b, e);
            nl = first_seen<LDS, FILL>(S, bits_ml, g.kf_ml_index, b, e, g.n_ml, g.ml_bad, status, STATUS_LINE_INDEX, nl, A.ml_index, ml0, A.ml_capacity);
        }
    }
}

// frame j's features i < n: a held item that is bad is cleared (:2097, :2114), everything from n on is -1; returns what feature i holds and votes with
// (-1: nothing, a temporal item, a bad one or one outside the map, which sets `bit`)
__device__ __forceinline__ int lm_clean(const int* __restrict__ in, int* __restrict__ out, size_t at, bool inside, int n_items, const uint8_t* __restrict__ bad,
                                        int* __restrict__ status, int bit)
{
    const int v = inside ? in[at] : -1, held = live_item(v, n_items, bad, status, bit);
    if (out) out[at] = (unsigned)v < (unsigned)n_items ? held : v;      // (an index outside the map stays as it came, a bad item becomes -1)
    return held;
}

__global__ __launch_bounds__(LM_THREADS) void k_localmap_count(LocalMapArgs A, int* __restrict__ status)
{
    __shared__ int s_votes[OLF_LOCALMAP_MAX_KF];
    __shared__ unsigned long long s_stamp[OLF_LOCALMAP_MAX_KF / 64];      // mnTrackReferenceForFrame == mCurrentFrame.mnId
    __shared__ int s_head[LM_HEAD];
    __shared__ SeenLds S;
    __shared__ unsigned long long s_best;
    __shared__ int s_cnt[2][LM_WAVES], s_size;
    const olf_map_graph& g = A.g;
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n_kf = g.n_kf;
    int* list = A.kf_list + (size_t)j * n_kf;

    for (int k = tid; k < n_kf; k += LM_THREADS) s_votes[k] = 0;
    for (int k = tid; k < LM_HASH; k += LM_THREADS) S.table[k] = 0;
    if (tid == 0) { S.round = 0; s_best = 0; s_size = 0; }
    __syncthreads();

    // ---- the votes, :2084-2117 ----
    const int n = A.counts ? frame_count(j, A.counts, A.img_stride, A.cap) : A.cap;
    for (int i = tid; i < A.cap; i += LM_THREADS) {
        const int v = lm_clean(A.frame_mp, A.frame_mp_out, (size_t)j * A.cap + i, i < n, g.n_mp, g.mp_bad, status, STATUS_POINT_INDEX);
        if (v < 0) continue;
        int b, e;
        csr_row(g.mp_obs_offsets, g.n_mp, v, b, e);
        for (int o = b; o < e; ++o) {
            const int kf = g.mp_obs_kf[o];
            if ((unsigned)kf >= (unsigned)n_kf) atomicOr(status, STATUS_KF_INDEX); else atomicAdd(&s_votes[kf], 1);
        }
    }
    if (A.frame_ml) {
        const int nl = A.lcounts ? frame_count(j, A.lcounts, A.img_stride, A.lcap) : A.lcap;
        for (int i = tid; i < A.lcap; i += LM_THREADS)
            lm_clean(A.frame_ml, A.frame_ml_out, (size_t)j * A.lcap + i, i < nl, g.n_ml, g.ml_bad, status, STATUS_LINE_INDEX);      // (lines do not vote, :2110)
    }
    __syncthreads();

    // ---- the first list, :2130-2145: the voted key frames in ascending index, the bad ones neither listed nor stamped ----
    int size = 0, voted = 0;
    unsigned long long best = 0;
    for (int k0 = 0; k0 < n_kf; k0 += LM_THREADS) {
        const int k = k0 + tid;
        const int votes = k < n_kf ? s_votes[k] : 0;
        const bool member = votes > 0 && !g.kf_bad[k];
        const unsigned long long mm = wave_vote(member);
        if (lane == 0 && k < n_kf) s_stamp[k >> 6] = mm;
        const bool p[2] = {member, votes > 0};
        int rank[2], n[2];
        block_rank<LM_WAVES, 2>(p, s_cnt, rank, n);
        const int at = size + rank[0];
        size += n[0]; voted += n[1];
        if (member) {
            list[at] = k;
            if (at < LM_HEAD) s_head[at] = k;
            best = max(best, vote_key(votes, k));
        }
        __syncthreads();
    }
    if (best) atomicMax(&s_best, best);
    __syncthreads();
    if (tid == 0) {
        A.n_voted[j] = voted;
        A.ref_kf[j] = vote_key_kf(s_best);
    }

    // ---- the extension, :2149-2198, by wave 0.  The end iterator is the first list's: `first` members are visited, what is appended is not ----
    if (w == 0) {
        volatile unsigned long long* stamp = s_stamp;
        const int first = size;
        for (int m = 0; m < first; ++m) {
            if (size > 80) break;
            const int kf = s_head[m];                                // (m <= 80 < LM_HEAD)
            int b, e;
            // GetBestCovisibilityKeyFrames(10): the first min(10, size) of the ordered list -- the first that is not bad and not stamped
            csr_row(g.kf_covis_offsets, n_kf, kf, b, e);
            e = min(e, b + 10);
            {
                const int c = b + lane < e ? g.kf_covis_index[b + lane] : -1;
                const bool oob = b + lane < e && (unsigned)c >= (unsigned)n_kf;
                if (oob) atomicOr(status, STATUS_KF_INDEX);
                const bool ok = b + lane < e && !oob && !g.kf_bad[c] && !((stamp[c >> 6] >> (c & 63)) & 1ull);
                const unsigned long long okm = wave_vote(ok);
                if (okm) {
                    const int add = __shfl(c, __ffsll((long long)okm) - 1, 64);
                    if (lane == 0) { list[size] = add; s_head[size] = add; stamp[add >> 6] = stamp[add >> 6] | (1ull << (add & 63)); }
                    ++size;
                }
            }
            // GetChilds(): std::set order = ascending index (C.16) -- the first that is not bad and not stamped
            csr_row(g.kf_child_offsets, n_kf, kf, b, e);
            for (int c0 = b; c0 < e; c0 += 64) {
                const int c = c0 + lane < e ? g.kf_child_index[c0 + lane] : -1;
                const bool oob = c0 + lane < e && (unsigned)c >= (unsigned)n_kf;
                if (oob) atomicOr(status, STATUS_KF_INDEX);
                const bool ok = c0 + lane < e && !oob && !g.kf_bad[c] && !((stamp[c >> 6] >> (c & 63)) & 1ull);
                const unsigned long long okm = wave_vote(ok);
                if (okm) {
                    const int add = __shfl(c, __ffsll((long long)okm) - 1, 64);
                    if (lane == 0) { list[size] = add; s_head[size] = add; stamp[add >> 6] = stamp[add >> 6] | (1ull << (add & 63)); }
                    ++size;
                    break;
                }
            }
            // GetParent(): not tested for bad; appending it ends the loop (:2194)
            const int p = g.kf_parent[kf];
            if (p != -1 && (unsigned)p >= (unsigned)n_kf) { if (lane == 0) atomicOr(status, STATUS_KF_INDEX); }
            else if (p != -1 && !((stamp[p >> 6] >> (p & 63)) & 1ull)) {
                if (lane == 0) { list[size] = p; s_head[size] = p; stamp[p >> 6] = stamp[p >> 6] | (1ull << (p & 63)); }
                ++size;
                break;
            }
        }
        if (lane == 0) s_size = size;
    }
    lm_publish();                                                    // (the list is read back below)
    __syncthreads();
    size = s_size;
    if (tid == 0) A.kf_offsets[j + 1] = size;

    // ---- UpdateLocalPointsAndLines, :2039-2078, counting ----
    long long np = 0, nl = 0;
    if (A.lds_bits) {
        unsigned* s_bits = reinterpret_cast<unsigned*>(s_votes);     // (the votes are done with; the barrier above is behind their last read)
        for (int k = tid; k < A.mpW + A.mlW; k += LM_THREADS) s_bits[k] = 0;
        lm_walk<true, false>(A, S, s_bits, s_bits + A.mpW, list, s_head, size, status, 0, 0, np, nl);
    } else {
        lm_walk<false, false>(A, S, A.seen_mp + (size_t)j * A.mpW, A.seen_ml + (size_t)j * A.mlW, list, s_head, size, status, 0, 0, np, nl);
    }
    if (tid == 0) {
        A.mp_offsets[j + 1] = (int)min(np, 0x7fffffffLL);
        A.ml_offsets[j + 1] = (int)min(nl, 0x7fffffffLL);
    }
}

// offsets[1 .. n] holds per-frame counts: make them running sums (offset_scan); block x is list x.  A total beyond the list's capacity raises
// STATUS_LOCALMAP_LIST.
__global__ __launch_bounds__(OFFSET_SCAN_THREADS) void k_localmap_scan(int* __restrict__ kf_offsets, int* __restrict__ mp_offsets, int* __restrict__ ml_offsets, int n,
                                                        int kf_capacity, int mp_capacity, int ml_capacity, int* __restrict__ status)
{
    int* offs = blockIdx.x == 0 ? kf_offsets : blockIdx.x == 1 ? mp_offsets : ml_offsets;
    const int capacity = blockIdx.x == 0 ? kf_capacity : blockIdx.x == 1 ? mp_capacity : ml_capacity;
    offset_scan(offs, n, capacity, status, STATUS_LOCALMAP_LIST);
}

__global__ __launch_bounds__(LM_THREADS) void k_localmap_fill(LocalMapArgs A, int* __restrict__ status)
{
    __shared__ SeenLds S;
    __shared__ unsigned s_bits[LM_BITS_WORDS];
    const int j = blockIdx.x, tid = threadIdx.x, n_kf = A.g.n_kf;
    const int* list = A.kf_list + (size_t)j * n_kf;
    const int kf0 = A.kf_offsets[j], size = min(max(A.kf_offsets[j + 1] - kf0, 0), n_kf);
    const long long mp0 = A.mp_offsets[j], ml0 = A.ml_offsets[j];
    for (int k = tid; k < LM_HASH; k += LM_THREADS) S.table[k] = 0;
    if (tid == 0) S.round = 0;
    for (int m = tid; m < size; m += LM_THREADS) if ((long long)kf0 + m < (long long)A.kf_capacity) A.kf_index[kf0 + m] = list[m];
    long long np = 0, nl = 0;
    if (A.lds_bits) {
        for (int k = tid; k < A.mpW + A.mlW; k += LM_THREADS) s_bits[k] = 0;
        lm_walk<true, true>(A, S, s_bits, s_bits + A.mpW, list, nullptr, size, status, mp0, ml0, np, nl);
    } else {
        lm_walk<false, true>(A, S, A.seen_mp + (size_t)j * A.mpW, A.seen_ml + (size_t)j * A.mlW, list, nullptr, size, status, mp0, ml0, np, nl);
    }
}

}  // namespace olf

using namespace olf;

extern "C" {

int olf_update_local_map_batch_dev(olf_ctx* c, const olf_map_graph* g, int n_frames, int img_stride, const int32_t* d_counts, const int32_t* d_lcounts,
                                   const int32_t* d_frame_mp, const int32_t* d_frame_ml, int32_t* d_frame_mp_out, int32_t* d_frame_ml_out, int32_t* d_ref_kf,
                                   int32_t* d_n_voted, int32_t* d_kf_offsets, int32_t* d_kf_index, int kf_capacity, int32_t* d_mp_offsets, int32_t* d_mp_index,
                                   int mp_capacity, int32_t* d_ml_offsets, int32_t* d_ml_index, int ml_capacity, void* stream)
{
    const char* who = "olf_update_local_map_batch_dev";
    bool ok = c && g && n_frames >= 0 && img_stride >= 1 && kf_capacity >= 0 && mp_capacity >= 0 && ml_capacity >= 0 && g->n_kf >= 0 && g->n_mp >= 0 && g->n_ml >= 0;
    ok = ok && d_frame_mp && d_ref_kf && d_n_voted && d_kf_offsets && d_mp_offsets && d_ml_offsets && (d_kf_index || !kf_capacity) && (d_mp_index || !mp_capacity) &&
         (d_ml_index || !ml_capacity);
    ok = ok && g->kf_bad && g->kf_mp_offsets && g->kf_covis_offsets && g->kf_child_offsets && g->kf_parent && g->mp_obs_offsets && (g->mp_bad || !g->n_mp) &&
         (g->n_ml == 0 || (g->ml_bad && g->kf_ml_offsets));
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(c, who));
    if (g->n_kf > OLF_LOCALMAP_MAX_KF) { set_error(std::string(who) + ": more than OLF_LOCALMAP_MAX_KF key frames (a frame's vote table lives in LDS)"); return OLF_ERR_CAPACITY; }
    if (n_frames == 0) return OLF_OK;
    LocalMapArgs A;
    A.g = *g;
    A.n_frames = n_frames; A.img_stride = img_stride; A.cap = olf_orb_capacity(c); A.lcap = olf_line_capacity(c);
    A.counts = d_counts; A.lcounts = d_lcounts; A.frame_mp = d_frame_mp; A.frame_ml = d_frame_ml;
    A.frame_mp_out = d_frame_mp_out; A.frame_ml_out = d_frame_ml ? d_frame_ml_out : nullptr;
    A.ref_kf = d_ref_kf; A.n_voted = d_n_voted;
    A.kf_offsets = d_kf_offsets; A.kf_index = d_kf_index; A.mp_offsets = d_mp_offsets; A.mp_index = d_mp_index; A.ml_offsets = d_ml_offsets; A.ml_index = d_ml_index;
    A.kf_capacity = kf_capacity; A.mp_capacity = mp_capacity; A.ml_capacity = ml_capacity;
    A.mpW = (g->n_mp + 31) / 32; A.mlW = (g->n_ml + 31) / 32;
    A.lds_bits = (long long)A.mpW + A.mlW <= LM_BITS_WORDS;
    if ((long long)n_frames * std::max(g->n_kf, 1) > 0x7fffffffLL) { set_error(std::string(who) + ": more than 2^31 (frame, key frame) pairs"); return OLF_ERR_CAPACITY; }
    // scratch: 4 bytes per (frame, key frame) for the key-frame lists between the passes; one bit per (frame, map point) and per (frame, map line) when a
    // frame's two bitmaps do not fit LM_BITS_WORDS words of LDS
    const size_t nb = A.lds_bits ? 0 : (size_t)n_frames;
    Carve k;
    k.add(&A.seen_mp, nb * A.mpW); k.add(&A.seen_ml, nb * A.mlW); k.add(&A.kf_list, (size_t)n_frames * g->n_kf);
    OLF_TRY(k.bind(c, SCRATCH_BATCH));
    hipStream_t s = ctx_stream(c, stream);
    // (the two bitmaps are the slab's first two regions: one memset, the padding between them included)
    if (nb) OLF_HIP_CHECK(hipMemsetAsync(A.seen_mp, 0, (size_t)(reinterpret_cast<char*>(A.kf_list) - reinterpret_cast<char*>(A.seen_mp)), s));
    hipLaunchKernelGGL(k_localmap_count, dim3(n_frames), dim3(LM_THREADS), 0, s, A, ctx_status(c));
    hipLaunchKernelGGL(k_localmap_scan, dim3(3), dim3(OFFSET_SCAN_THREADS), 0, s, d_kf_offsets, d_mp_offsets, d_ml_offsets, n_frames, kf_capacity, mp_capacity, ml_capacity, ctx_status(c));
    hipLaunchKernelGGL(k_localmap_fill, dim3(n_frames), dim3(LM_THREADS), 0, s, A, ctx_status(c));
    OLF_HIP_CHECK(hipGetLastError());
    return OLF_OK;
}

}  // extern "C"
