// entry_lists.hpp -- how the per-entry arrays of a local map are indexed (olf_local_map / olf_local_line_map, include/orbline.h): with list_offsets, entry e
// in [list_offsets[j], list_offsets[j + 1]) is item list_index[e] for frame j; without, entry e = j * n_items + i is item i for frame j.  The offsets are
// device data: whatever they hold, a range stays inside [0, n_entries).  Also the scatter of what a frame already holds into one bit per (frame, item).
#pragma once
#include "olf_internal.hpp"

namespace olf {

struct EntryLists {
    const int *offsets, *index;      // list_offsets [n_frames + 1] (or NULL), list_index [n_entries]
    int n_items, n_frames, n_entries;

    // the frame entry e belongs to (-1: none) and its map index (unchecked)
    __device__ __forceinline__ int frame_of(int e, int& mi) const
    {
        if (!offsets) {
            const int j = e / n_items;
            mi = e - j * n_items;
            return j;
        }
        int lo = 0, hi = n_frames;                      // the last frame whose list starts at or before e
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= e) lo = mid; else hi = mid;
        }
        mi = index[e];
        return (e >= offsets[lo] && e < offsets[lo + 1]) ? lo : -1;
    }

    // the entries of frame j, inside [0, n_entries) whatever the offsets hold
    __device__ __forceinline__ void range(int j, int& b, int& e) const
    {
        if (!offsets) { b = j * n_items; e = b + n_items; return; }
        csr_clamp(offsets, j, n_entries, b, e);
    }
};

// One feature's item into its frame's held bitmap (one bit per item; held_row: the frame's (n_items + 31) / 32 words, zeroed before).  v is the feature's
// entry of mvpMapPoints as an index into the map, taken as live_item takes it: a bad item is dropped from its feature.  Returns v where the frame holds
// a live item now, -1 otherwise.
__device__ __forceinline__ int held_mark(int v, int n_items, const uint8_t* __restrict__ bad, unsigned* __restrict__ held_row, int* __restrict__ status, int bit)
{
    v = live_item(v, n_items, bad, status, bit);
    if (v >= 0) atomicOr(&held_row[v >> 5], 1u << (v & 31));
    return v;
}

}  // namespace olf
