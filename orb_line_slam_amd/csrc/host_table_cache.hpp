// host_table_cache.hpp -- the parameter tables of the RANSAC solvers (sim3solver_batch.hip, pnpsolver_batch.hip): a row of `words` ints for every N in
// [0, cap], a function of N and one parameter set, built on the host (libm) and uploaded on the call's stream from pinned memory.  The upload of a call may
// read its table after the call has returned, so a table is never changed while its last upload can be pending: at most kTables parameter sets are kept;
// one more takes the place of the least recently used, after that one's last upload has completed (an event per table; the wait is the only one an entry
// ever makes, and only a caller that sweeps more than kTables parameter sets meets it).  One mutex per cache.
#pragma once
#include <mutex>
#include <vector>
#include "olf_internal.hpp"

namespace olf {

class HostTableCache {
public:
    struct Key {
        double probability;
        int min_inliers, max_iterations, cap;
        float epsilon;                              // (0 where a solver has none)
        bool operator==(const Key& o) const
        {
            return probability == o.probability && min_inliers == o.min_inliers && max_iterations == o.max_iterations && cap == o.cap && epsilon == o.epsilon;
        }
    };
    explicit HostTableCache(int words) : words_((size_t)words) {}

    // d_tab [words * (key.cap + 1)] receives the table of `key`; fill(N, row) writes the row of N where the table is not kept yet
    template <class Fill>
    int upload(const Key& key, Fill fill, int* d_tab, hipStream_t s)
    {
        std::lock_guard<std::mutex> lock(mutex_);
        const size_t n = words_ * ((size_t)key.cap + 1);
        Table* t = nullptr;
        for (Table& e : tables_) if (e.key == key) t = &e;
        if (!t) {
            if (tables_.size() < kTables) {
                Table e = {};
                OLF_HIP_CHECK(hipEventCreateWithFlags(&e.last, hipEventDisableTiming));
                tables_.push_back(e);
                t = &tables_.back();
            } else {
                t = &tables_[0];
                for (Table& e : tables_) if (e.used < t->used) t = &e;
                OLF_HIP_CHECK(hipEventSynchronize(t->last));
            }
            if (t->room < n) {
                if (t->host) OLF_HIP_CHECK(hipHostFree(t->host));
                t->host = nullptr; t->room = 0;
                OLF_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&t->host), n * sizeof(int), hipHostMallocDefault));
                t->room = n;
            }
            t->key = key;
            for (int N = 0; N <= key.cap; ++N) fill(N, t->host + words_ * (size_t)N);
        }
        t->used = ++clock_;
        OLF_HIP_CHECK(hipMemcpyAsync(d_tab, t->host, n * sizeof(int), hipMemcpyHostToDevice, s));
        OLF_HIP_CHECK(hipEventRecord(t->last, s));
        return OLF_OK;
    }

private:
    static constexpr size_t kTables = 8;
    struct Table { Key key; size_t room; int* host; hipEvent_t last; unsigned long long used; };
    const size_t words_;
    std::mutex mutex_;
    std::vector<Table> tables_;
    unsigned long long clock_ = 0;
};

}  // namespace olf
