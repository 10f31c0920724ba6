// carve.hpp -- cut one slab into typed regions: the offset arithmetic of staging.hpp.  Plain host C++ (no HIP header): tests/staging_layout.cpp
// compiles it with g++ alone.
//
//     CarveLayout k;  k.add(&dQ, nQ * 32);  k.add(&dT, nT * 32);  k.add(&dn, 2);      // (pointer to fill, ELEMENT count)
//     ... get k.total() bytes from somewhere ...  k.fill(base);
//
// Regions lie in request order, each at a multiple of kCarveAlign from the base and disjoint from the others.  A region of no elements still takes one
// unit, so its pointer is valid, non-null and different from every other region's: a launcher may be handed it with a count of zero.
//
// One alignment, 16 bytes: the widest type carved is uint4 and no kernel reads a carved region with a wider access.  (olf_search_by_bow_batch_dev used to
// round its node array to 64; bow_match.hip reads it as int and the sorted list behind it as unsigned long long, so that was a cache-line habit and 16 is
// enough.)  The slab itself comes from hipMalloc, aligned to 256.
#pragma once
#include <cassert>
#include <cstddef>
#include <cstring>

namespace olf {

constexpr size_t kCarveAlign = 16;
constexpr int kCarveMaxRegions = 32;     // (olf_update_local_map stages a map graph and its outputs: twenty-six)

class CarveLayout {
public:
    template <typename T>
    void add(T** p, size_t count)
    {
        assert(n_ < kCarveMaxRegions);
        const size_t bytes = count * sizeof(T);
        req_[n_++] = {p, total_};
        total_ += ((bytes ? bytes : 1) + kCarveAlign - 1) & ~(kCarveAlign - 1);
    }
    size_t total() const { return total_; }
    // (a request holds the address of a T* of any T: the pointer is stored through memcpy, as fb_set_field does)
    void fill(void* base) const
    {
        for (int i = 0; i < n_; ++i) { char* q = static_cast<char*>(base) + req_[i].offset; std::memcpy(req_[i].ptr, &q, sizeof(q)); }
    }

private:
    struct Request { void* ptr; size_t offset; };
    Request req_[kCarveMaxRegions];
    int n_ = 0;
    size_t total_ = 0;
};

}  // namespace olf
