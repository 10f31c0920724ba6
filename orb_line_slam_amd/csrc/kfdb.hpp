// kfdb.hpp -- the key-frame database behind olf_kfdb_* (include/orbline.h): what kfdb_host.cpp (selection, plain host C++, no HIP header: it links into
// a stand-alone program) and kfdb_api.cpp (the device copy and the entries that launch) share.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/orbline.h"

namespace olf {

void set_error(const std::string& s);

// one vocabulary's key-frame BoW vectors: slot k is ids / vals [beg[k], beg[k] + len[k]); an erased slot has len 0 (its words stay where they are)
struct KfdbVectors {
    int n_words = 0;                      // the vocabulary's size: 0 = this vocabulary is absent
    std::vector<int32_t> beg, len;        // host copies of d_beg / d_len
    size_t used = 0;                      // words appended so far
    int32_t *d_beg = nullptr, *d_len = nullptr, *d_ids = nullptr;
    double* d_vals = nullptr;
    size_t cap_slots = 0, cap_words = 0;  // what the four device arrays hold
};

// the per-key-frame members that cross queries, and the bounds of the two id counters
struct KfdbState {
    std::vector<float> reloc_score, reloc_score_l, reloc_score_pl;     // mRelocScore, mRelocScore_l, mRelocScore_pl: 0 at construction, src/KeyFrame.cc:35-37
    int64_t last_loop_id = 0, last_reloc_id = 0;
};

struct SelectArgs {
    int form, n_queries;
    const int64_t* query_ids;
    const int32_t *np, *nl;
    const float* min_score;
    const int32_t *conn_off, *conn_slots, *nb_off, *nb_slots;
    int n_slots;
    const olf_kfdb_tables *tp, *tl;
};
// the four Detect members from the tables on: candidates per query as CSR (cand_off resized to n_queries + 1).  `st` is updated in place; has_lines: the
// database has a line vocabulary (:232, :516).  Returns OLF_OK, or OLF_ERR_INVALID (message set) before st is touched.
int kfdb_select(const SelectArgs& a, bool has_lines, KfdbState& st, std::vector<int32_t>& cand_off, std::vector<int32_t>& cand);

}  // namespace olf

struct olf_kfdb {
    olf_ctx* ctx = nullptr;
    int n_slots = 0, n_live = 0;
    std::vector<uint8_t> live;
    olf::KfdbVectors v[2];                // points, lines
    olf::KfdbState st;
    // olf_kfdb_tables_dev's query offsets on their way to the device: pinned, and an event (a hipEvent_t) behind the copy so that the next call does not
    // overwrite them while it is still pending
    int32_t* h_qoff = nullptr; size_t h_qoff_cap = 0; void* ev_qoff = nullptr; bool ev_pending = false;
};
