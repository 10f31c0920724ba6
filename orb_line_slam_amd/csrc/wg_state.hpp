// wg_state.hpp -- where the per-row state of a one-workgroup-per-row kernel lives, stated once for pose_batch.hip, posepoints_batch.hip, optsim3_batch.hip,
// sim3solver_batch.hip and pnpsolver_batch.hip.  A row's state is one slab of regions; it is dynamic LDS when it fits the kernel's limit and otherwise
// the workgroup's part of the batch scratch slot, and the kernel's text is the same either way (one flat pointer).
//   Regions          cuts a slab into regions, each at a multiple of 16 bytes (host and device: a kernel forms the same offsets its launcher sized);
//                    pose_batch.hip takes the rounding alone and keeps its own layout text (it says why)
//   LdsLimit         a kernel's limit: its default and what a test lowered it to (olf_debug_*_lds_limit), so that the scratch path runs at small sizes
//   wg_state_in_lds  the launcher's half: LDS or a slab per workgroup in the launcher's Carve; wg_state_place for a launcher that carves nothing else
//   wg_state_ptr     the kernel's half (k_sim3_solver keeps its own text: sim3solver_batch.hip says why)
//   allow_large_lds  dynamic LDS above 64 KB, allowed once per kernel and device
#pragma once
#include <mutex>
#include <utility>
#include <vector>
#include "staging.hpp"

namespace olf {

struct Regions {
    size_t total = 0;
    __host__ __device__ static constexpr size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }
    // the offset of a new region of `bytes`
    __host__ __device__ constexpr size_t cut(size_t bytes) { const size_t at = total; total = round16(total + bytes); return at; }
};

struct LdsLimit {
    int def, cur;
    constexpr explicit LdsLimit(int d) : def(d), cur(d) {}
    void set(int bytes) { cur = bytes > 0 ? std::min(bytes, def) : def; }      // 0 or less: back to the default; never above it
    bool fits(size_t bytes) const { return bytes <= (size_t)cur; }
};
// the five limits a test can lower, each defined beside its kernel (api_debug.cpp sets them)
extern LdsLimit g_pose_points_lds, g_optimize_sim3_lds, g_sim3_solver_lds, g_pnp_solver_lds, g_initializer_lds;

// True: `bytes` of state per workgroup fit the limit, the launch asks for that much dynamic LDS and *slabs stays NULL.  False: `grid` slabs of `bytes` are
// added to k, which the launcher binds to SCRATCH_BATCH with whatever else it carves there.
template <class T>
inline bool wg_state_in_lds(Carve& k, const LdsLimit& lim, size_t bytes, int grid, T** slabs)
{
    *slabs = nullptr;
    if (lim.fits(bytes)) return true;
    k.add(slabs, (size_t)grid * bytes / sizeof(T));
    return false;
}
// the same for a launcher that carves nothing else: the batch scratch slot is asked for only when the state does not fit
template <class T>
inline int wg_state_place(olf_ctx* c, const LdsLimit& lim, size_t bytes, int grid, T** slabs, int* use_lds)
{
    Carve k;
    *use_lds = wg_state_in_lds(k, lim, bytes, grid, slabs);
    return *use_lds ? OLF_OK : k.bind(c, SCRATCH_BATCH);
}

// the workgroup's state: the dynamic LDS at dyn, or slab blockIdx.x of `stride` elements.  The launcher's answer comes as a flag of the kernel's arguments:
// tested as `slabs != NULL` the three optimisers' kernels compiled to other code and two of them fell outside the timing rule.
template <class T>
__device__ __forceinline__ T* wg_state_ptr(bool in_lds, T* dyn, T* slabs, size_t stride)
{
    return in_lds ? dyn : slabs + (size_t)blockIdx.x * stride;
}

// dynamic LDS above 64 KB has to be allowed once per kernel and device: remembered here, so an entry makes no attribute call after its first on a device
inline int allow_large_lds(const void* kernel, int bytes)
{
    static std::mutex mu;
    static std::vector<std::pair<const void*, int>> done;
    int dev = 0;
    OLF_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& e : done) if (e.first == kernel && e.second == dev) return OLF_OK;
    OLF_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.emplace_back(kernel, dev);
    return OLF_OK;
}

}  // namespace olf
