// staging.hpp -- how an entry point gets device scratch and how a host-pointer entry moves its arrays: a carve and a host call, nothing else.
//
// Carve: a CarveLayout (carve.hpp) bound to one of the context's scratch slots.  A _dev entry that needs working arrays says
//     Carve k;  k.add(&lists, n);  k.add(&bad, m);  OLF_TRY(k.bind(c, SCRATCH_BATCH));
//
// HostCall: a carve plus the copy recipe of a host-pointer entry on the context's stream.  After its argument checks the entry says
//     HostCall h(c, "olf_x");                                       -- checks the device
//     h.add(&dA, nA * 32);  h.add(&dOut, nA);  OLF_TRY(h.bind(SCRATCH_STAGE));      -- fails with the device check's code before any HIP call
//     OLF_TRY(h.up(dA, descA, nA * 32));  OLF_TRY(launch or _dev entry on h.stream());  OLF_TRY(h.down(out, dOut, nA * 4));
//     return h.finish();                                            -- or finish_status()
#pragma once
#include <algorithm>
#include "carve.hpp"
#include "olf_internal.hpp"

namespace olf {

struct Carve : CarveLayout {
    int bind(olf_ctx* c, ScratchSlot slot)
    {
        void* base = nullptr;
        OLF_TRY(ctx_scratch(c, slot, total(), &base));
        fill(base);
        return OLF_OK;
    }
};

// what a host-pointer entry checks of a CSR pair of its caller's: offsets [n + 1] non-decreasing from 0 (and an index array where there are entries);
// *total = offsets[n]
inline bool csr_ok(const int32_t* offs, const int32_t* index, int n, size_t* total)
{
    if (!offs || offs[0] != 0) return false;
    for (int k = 0; k < n; ++k) if (offs[k + 1] < offs[k]) return false;
    *total = (size_t)offs[n];
    return index || !*total;
}

class HostCall : public Carve {
public:
    HostCall(olf_ctx* c, const char* who) : c_(c), s_(ctx_stream(c)), device_rc_(ctx_check_device(c, who)) {}
    hipStream_t stream() const { return s_; }
    // an entry that carves nothing (its arrays are the context's own) calls begin() instead of bind()
    int begin() const { return device_rc_; }
    int bind(ScratchSlot slot) { OLF_TRY(begin()); return Carve::bind(c_, slot); }
    int up(void* dev, const void* host, size_t bytes) { return copy(dev, host, bytes, hipMemcpyHostToDevice); }
    int down(void* host, const void* dev, size_t bytes) { return copy(host, dev, bytes, hipMemcpyDeviceToHost); }
    // The two-step download of a list whose length the device decides: n_head words (a CSR offsets array, or one count word) whose LAST word is the
    // length; synchronise; then that many 4-byte items, at most max_items.  *length is the word as the device wrote it: the caller judges one out of range.
    int down_counted(int32_t* head, const int32_t* d_head, size_t n_head, void* items, const void* d_items, int max_items, int* length)
    {
        OLF_TRY(down(head, d_head, n_head * 4));
        OLF_HIP_CHECK(hipStreamSynchronize(s_));
        *length = head[n_head - 1];
        return down(items, d_items, (size_t)std::max(std::min(*length, max_items), 0) * 4);
    }
    int finish() { OLF_HIP_CHECK(hipStreamSynchronize(s_)); return OLF_OK; }
    int finish_status() { OLF_TRY(finish()); return ctx_check_status(c_); }

private:
    int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
    {
        if (bytes) OLF_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, kind, s_));
        return OLF_OK;
    }
    olf_ctx* c_;
    hipStream_t s_;
    int device_rc_;
};

}  // namespace olf
