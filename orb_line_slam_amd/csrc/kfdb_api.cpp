// kfdb_api.cpp -- the entries of the key-frame database that own or launch on the device (include/orbline.h, "place recognition"): the database's device
// copy (CSR per vocabulary, grown on add), the tables, detect = tables + download + select, and the L1 score of pairs.  The selection itself and the
// entries that need no device are kfdb_host.cpp.
#include <climits>
#include "kfdb.hpp"
#include "staging.hpp"

using namespace olf;

namespace {

bool vector_ok(const int32_t* ids, const double* vals, int n, int n_words)
{
    if (n < 0 || (n > 0 && (!ids || !vals))) return false;
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= n_words || (i > 0 && ids[i] <= ids[i - 1])) return false;
    return true;
}

template <typename T>
int regrow(T** d, size_t keep, size_t cap)
{
    T* p = nullptr;
    OLF_HIP_CHECK(hipMalloc((void**)&p, cap * sizeof(T)));
    if (keep) OLF_HIP_CHECK(hipMemcpy(p, *d, keep * sizeof(T), hipMemcpyDeviceToDevice));
    (void)hipFree(*d);
    *d = p;
    return OLF_OK;
}

// room for one more slot of n words in the device copy (the arrays move: nothing of this database may be running)
int reserve(KfdbVectors& v, size_t n)
{
    const size_t slots = v.beg.size();
    if (slots + 1 > v.cap_slots || v.used + n > v.cap_words) OLF_HIP_CHECK(hipDeviceSynchronize());
    if (slots + 1 > v.cap_slots) {
        const size_t cap = std::max<size_t>(1024, 2 * v.cap_slots);
        OLF_TRY(regrow(&v.d_beg, slots, cap)); OLF_TRY(regrow(&v.d_len, slots, cap));
        v.cap_slots = cap;
    }
    if (v.used + n > v.cap_words) {
        const size_t cap = std::max<size_t>({(size_t)1 << 16, 2 * v.cap_words, v.used + n});
        OLF_TRY(regrow(&v.d_ids, v.used, cap)); OLF_TRY(regrow(&v.d_vals, v.used, cap));
        v.cap_words = cap;
    }
    return OLF_OK;
}

int csr_check(const char* who, const olf_bow_csr* q, int n_queries)
{
    if (q->off[0] < 0) { set_error(std::string(who) + ": query offsets must start at >= 0"); return OLF_ERR_INVALID; }
    for (int i = 0; i < n_queries; ++i) {
        if (q->off[i + 1] < q->off[i]) { set_error(std::string(who) + ": query offsets must not decrease"); return OLF_ERR_INVALID; }
        if (q->off[i + 1] - q->off[i] > OLF_KFDB_MAX_WORDS) {
            set_error(std::string(who) + ": a query has more than OLF_KFDB_MAX_WORDS = 4096 words (a query's word ids are staged in 16 KB of LDS)");
            return OLF_ERR_CAPACITY;
        }
    }
    return OLF_OK;
}

bool csr_whole(const olf_bow_csr* q) { return q && q->off && q->ids && q->vals; }
bool tables_whole(const olf_kfdb_tables* t) { return t && t->common && t->first && t->score; }

}  // namespace

extern "C" {

int olf_kfdb_create(olf_ctx* ctx, int n_words_p, int n_words_l, int scoring_p, int scoring_l, olf_kfdb** out)
{
    if (!out || n_words_p < 1 || n_words_l < 0) { set_error("olf_kfdb_create: bad argument"); return OLF_ERR_INVALID; }
    if (scoring_p != OLF_SCORING_L1_NORM || (n_words_l > 0 && scoring_l != OLF_SCORING_L1_NORM)) {
        set_error("olf_kfdb_create: only L1_NORM scoring is supported (the scoring of both of the reference's vocabularies)"); return OLF_ERR_INVALID;
    }
    if (ctx) OLF_TRY(ctx_check_device(ctx, "olf_kfdb_create"));
    olf_kfdb* db = new olf_kfdb;
    db->ctx = ctx;
    db->v[0].n_words = n_words_p; db->v[1].n_words = n_words_l;
    *out = db;
    return OLF_OK;
}

void olf_kfdb_destroy(olf_kfdb* db)
{
    if (!db) return;
    if (db->ctx) {
        (void)hipDeviceSynchronize();
        for (KfdbVectors& v : db->v) { (void)hipFree(v.d_beg); (void)hipFree(v.d_len); (void)hipFree(v.d_ids); (void)hipFree(v.d_vals); }
        if (db->h_qoff) (void)hipHostFree(db->h_qoff);
        if (db->ev_qoff) (void)hipEventDestroy((hipEvent_t)db->ev_qoff);
    }
    delete db;
}

int olf_kfdb_add(olf_kfdb* db, const int32_t* ids_p, const double* vals_p, int n_p, const int32_t* ids_l, const double* vals_l, int n_l, int32_t* slot)
{
    if (!db || !slot || n_p < 0 || n_l < 0 || (n_p > 0 && (!ids_p || !vals_p)) || (n_l > 0 && (!ids_l || !vals_l))) {
        set_error("olf_kfdb_add: bad argument"); return OLF_ERR_INVALID;
    }
    if (db->v[1].n_words == 0) n_l = 0;                  // no line vocabulary: there is no line inverted file to enter
    if (!vector_ok(ids_p, vals_p, n_p, db->v[0].n_words) || !vector_ok(ids_l, vals_l, n_l, db->v[1].n_words)) {
        set_error("olf_kfdb_add: word ids must be ascending, distinct and inside the vocabulary"); return OLF_ERR_INVALID;
    }
    if (n_p > OLF_KFDB_MAX_WORDS || n_l > OLF_KFDB_MAX_WORDS) { set_error("olf_kfdb_add: more than OLF_KFDB_MAX_WORDS = 4096 words in a vector"); return OLF_ERR_CAPACITY; }
    if (db->n_slots >= OLF_KFDB_MAX_SLOTS) { set_error("olf_kfdb_add: more than OLF_KFDB_MAX_SLOTS = 2^20 slots (olf_kfdb_clear starts again)"); return OLF_ERR_CAPACITY; }
    if (db->v[0].used + (size_t)n_p > (size_t)INT_MAX || db->v[1].used + (size_t)n_l > (size_t)INT_MAX) {
        set_error("olf_kfdb_add: more than 2^31 - 1 words in the database"); return OLF_ERR_CAPACITY;
    }
    const int n[2] = {n_p, n_l};
    const int32_t* ids[2] = {ids_p, ids_l};
    const double* vals[2] = {vals_p, vals_l};
    if (db->ctx) {
        OLF_TRY(ctx_check_device(db->ctx, "olf_kfdb_add"));
        for (int t = 0; t < 2; ++t) {
            KfdbVectors& v = db->v[t];
            if (v.n_words == 0) continue;
            OLF_TRY(reserve(v, n[t]));
            const int32_t b = (int32_t)v.used, l = n[t];
            if (n[t]) {
                OLF_HIP_CHECK(hipMemcpy(v.d_ids + v.used, ids[t], (size_t)n[t] * 4, hipMemcpyHostToDevice));
                OLF_HIP_CHECK(hipMemcpy(v.d_vals + v.used, vals[t], (size_t)n[t] * 8, hipMemcpyHostToDevice));
            }
            OLF_HIP_CHECK(hipMemcpy(v.d_beg + db->n_slots, &b, 4, hipMemcpyHostToDevice));
            OLF_HIP_CHECK(hipMemcpy(v.d_len + db->n_slots, &l, 4, hipMemcpyHostToDevice));
        }
    }
    for (int t = 0; t < 2; ++t) {
        KfdbVectors& v = db->v[t];
        if (v.n_words == 0) continue;
        v.beg.push_back((int32_t)v.used); v.len.push_back(n[t]);
        v.used += n[t];
    }
    db->live.push_back(1);
    db->st.reloc_score.push_back(0.f); db->st.reloc_score_l.push_back(0.f); db->st.reloc_score_pl.push_back(0.f);
    *slot = db->n_slots++;
    ++db->n_live;
    return OLF_OK;
}

int olf_kfdb_erase(olf_kfdb* db, int32_t slot)
{
    if (!db) { set_error("olf_kfdb_erase: null database"); return OLF_ERR_INVALID; }
    if (slot < 0 || slot >= db->n_slots) { set_error("olf_kfdb_erase: no such slot"); return OLF_ERR_INVALID; }
    if (!db->live[slot]) return OLF_OK;
    if (db->ctx) {
        OLF_TRY(ctx_check_device(db->ctx, "olf_kfdb_erase"));
        const int32_t zero = 0;
        for (KfdbVectors& v : db->v) if (v.n_words) OLF_HIP_CHECK(hipMemcpy(v.d_len + slot, &zero, 4, hipMemcpyHostToDevice));
    }
    for (KfdbVectors& v : db->v) if (v.n_words) v.len[slot] = 0;
    db->live[slot] = 0;
    --db->n_live;
    return OLF_OK;
}

int olf_kfdb_clear(olf_kfdb* db)
{
    if (!db) { set_error("olf_kfdb_clear: null database"); return OLF_ERR_INVALID; }
    for (KfdbVectors& v : db->v) { v.beg.clear(); v.len.clear(); v.used = 0; }
    db->live.clear();
    db->st = KfdbState();
    db->n_slots = db->n_live = 0;
    return OLF_OK;
}

int olf_kfdb_tables_dev(olf_kfdb* db, int n_queries, const olf_bow_csr* qp, const olf_bow_csr* ql, const olf_kfdb_tables* d_tp, const olf_kfdb_tables* d_tl,
                        void* stream)
{
    if (!db || n_queries < 0 || !csr_whole(qp) || !tables_whole(d_tp) || (ql != nullptr) != (d_tl != nullptr) || (ql && (!csr_whole(ql) || !tables_whole(d_tl)))) {
        set_error("olf_kfdb_tables_dev: bad argument"); return OLF_ERR_INVALID;
    }
    if (!db->ctx) { set_error("olf_kfdb_tables_dev: the database was created without a context"); return OLF_ERR_INVALID; }
    if (ql && db->v[1].n_words == 0) { set_error("olf_kfdb_tables_dev: line queries for a database without a line vocabulary"); return OLF_ERR_INVALID; }
    OLF_TRY(csr_check("olf_kfdb_tables_dev", qp, n_queries));
    if (ql) OLF_TRY(csr_check("olf_kfdb_tables_dev", ql, n_queries));
    if ((long long)n_queries * db->n_slots > OLF_KFDB_MAX_CELLS) {
        set_error("olf_kfdb_tables_dev: n_queries x slots exceeds OLF_KFDB_MAX_CELLS = 2^26 table entries: split the batch"); return OLF_ERR_CAPACITY;
    }
    OLF_TRY(ctx_check_device(db->ctx, "olf_kfdb_tables_dev"));
    if (n_queries == 0 || db->n_slots == 0) return OLF_OK;
    hipStream_t s = ctx_stream(db->ctx, stream);
    const size_t n_off = (size_t)n_queries + 1, n_vocs = ql ? 2 : 1;
    if (!db->ev_qoff) { hipEvent_t e; OLF_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); db->ev_qoff = e; }
    if (db->ev_pending) { OLF_HIP_CHECK(hipEventSynchronize((hipEvent_t)db->ev_qoff)); db->ev_pending = false; }
    if (db->h_qoff_cap < 2 * n_off) {
        if (db->h_qoff) (void)hipHostFree(db->h_qoff);
        db->h_qoff = nullptr; db->h_qoff_cap = 0;
        OLF_HIP_CHECK(hipHostMalloc((void**)&db->h_qoff, 2 * n_off * 4, hipHostMallocDefault));
        db->h_qoff_cap = 2 * n_off;
    }
    std::copy(qp->off, qp->off + n_off, db->h_qoff);
    if (ql) std::copy(ql->off, ql->off + n_off, db->h_qoff + n_off);
    int32_t* d_qoff;
    Carve k;
    k.add(&d_qoff, 2 * n_off);
    OLF_TRY(k.bind(db->ctx, SCRATCH_BATCH));
    OLF_HIP_CHECK(hipMemcpyAsync(d_qoff, db->h_qoff, n_vocs * n_off * 4, hipMemcpyHostToDevice, s));
    OLF_HIP_CHECK(hipEventRecord((hipEvent_t)db->ev_qoff, s));
    db->ev_pending = true;
    const KfdbVectors& vp = db->v[0];
    OLF_TRY(launch_kfdb_tables(d_qoff, qp->ids, qp->vals, n_queries, vp.d_beg, vp.d_len, vp.d_ids, vp.d_vals, db->n_slots, d_tp->common, d_tp->first,
                               d_tp->score, s));
    if (ql) {
        const KfdbVectors& vl = db->v[1];
        OLF_TRY(launch_kfdb_tables(d_qoff + n_off, ql->ids, ql->vals, n_queries, vl.d_beg, vl.d_len, vl.d_ids, vl.d_vals, db->n_slots, d_tl->common,
                                   d_tl->first, d_tl->score, s));
    }
    return OLF_OK;
}

int olf_kfdb_detect(olf_kfdb* db, int form, int n_queries, const int64_t* query_ids, const olf_bow_csr* qp, const olf_bow_csr* ql, const int32_t* np,
                    const int32_t* nl, const float* min_score, const int32_t* conn_off, const int32_t* conn_slots, const int32_t* nb_off,
                    const int32_t* nb_slots, int32_t* cand_off, int32_t* cand_slots, int cand_capacity)
{
    const bool loop = form == OLF_KFDB_LOOP || form == OLF_KFDB_LOOP_LINE, line = form == OLF_KFDB_LOOP_LINE || form == OLF_KFDB_RELOC_LINE;
    if (!db || form < OLF_KFDB_LOOP || form > OLF_KFDB_RELOC_LINE || n_queries < 0 || cand_capacity < 0 || !cand_off || !nb_off ||
        (cand_capacity > 0 && !cand_slots) || (conn_off && !conn_slots) || !qp || !qp->off || (line && (!ql || !ql->off)) ||
        (n_queries > 0 && (!query_ids || (loop && !min_score) || (line && (!np || !nl))))) {
        set_error("olf_kfdb_detect: bad argument"); return OLF_ERR_INVALID;
    }
    const int n = db->n_slots;
    if (nb_off[0] != 0) { set_error("olf_kfdb_detect: nb_off must start at 0"); return OLF_ERR_INVALID; }
    for (int k = 0; k < n; ++k) if (nb_off[k + 1] < nb_off[k]) { set_error("olf_kfdb_detect: nb_off must not decrease"); return OLF_ERR_INVALID; }
    if (nb_off[n] > 0 && !nb_slots) { set_error("olf_kfdb_detect: bad argument"); return OLF_ERR_INVALID; }
    if (conn_off) for (int q = 0; q < n_queries; ++q) if (conn_off[q] < 0 || conn_off[q + 1] < conn_off[q]) { set_error("olf_kfdb_detect: conn_off must not decrease"); return OLF_ERR_INVALID; }
    const bool has_lines = db->v[1].n_words > 0, both = line && has_lines;
    std::vector<int32_t> common[2], first[2];
    std::vector<double> score[2];
    olf_kfdb_tables ht[2] = {};
    if (!(line && !has_lines) && n_queries > 0 && n > 0) {
        if (!db->ctx) { set_error("olf_kfdb_detect: the database was created without a context"); return OLF_ERR_INVALID; }
        const olf_bow_csr* hq[2] = {qp, ql};
        const int n_vocs = both ? 2 : 1;
        const size_t cells = (size_t)n_queries * n;
        for (int t = 0; t < n_vocs; ++t) {
            OLF_TRY(csr_check("olf_kfdb_detect", hq[t], n_queries));
            if (hq[t]->off[n_queries] > hq[t]->off[0] && (!hq[t]->ids || !hq[t]->vals)) { set_error("olf_kfdb_detect: bad argument"); return OLF_ERR_INVALID; }
        }
        if (cells > (size_t)OLF_KFDB_MAX_CELLS) {
            set_error("olf_kfdb_detect: n_queries x slots exceeds OLF_KFDB_MAX_CELLS = 2^26 table entries: split the batch"); return OLF_ERR_CAPACITY;
        }
        HostCall h(db->ctx, "olf_kfdb_detect");
        int32_t *d_ids[2], *d_cf[2]; double *d_vals[2], *d_score[2];       // d_cf: the common table, then the first table
        size_t nw[2] = {0, 0};
        for (int t = 0; t < n_vocs; ++t) { nw[t] = (size_t)hq[t]->off[n_queries]; h.add(&d_score[t], cells); h.add(&d_vals[t], nw[t]); }
        for (int t = 0; t < n_vocs; ++t) { h.add(&d_ids[t], nw[t]); h.add(&d_cf[t], 2 * cells); }
        OLF_TRY(h.bind(SCRATCH_STAGE));
        olf_bow_csr dq[2]; olf_kfdb_tables dt[2];
        for (int t = 0; t < n_vocs; ++t) {
            OLF_TRY(h.up(d_ids[t], hq[t]->ids, nw[t] * 4)); OLF_TRY(h.up(d_vals[t], hq[t]->vals, nw[t] * 8));
            dq[t] = {hq[t]->off, d_ids[t], d_vals[t]};
            dt[t] = {d_cf[t], d_cf[t] + cells, d_score[t]};
        }
        OLF_TRY(olf_kfdb_tables_dev(db, n_queries, &dq[0], both ? &dq[1] : nullptr, &dt[0], both ? &dt[1] : nullptr, h.stream()));
        for (int t = 0; t < n_vocs; ++t) {
            common[t].resize(cells); first[t].resize(cells); score[t].resize(cells);
            OLF_TRY(h.down(common[t].data(), d_cf[t], cells * 4)); OLF_TRY(h.down(first[t].data(), d_cf[t] + cells, cells * 4));
            OLF_TRY(h.down(score[t].data(), d_score[t], cells * 8));
            ht[t] = {common[t].data(), first[t].data(), score[t].data()};
        }
        OLF_TRY(h.finish());
    }
    const SelectArgs a = {form, n_queries, query_ids, np, nl, min_score, conn_off, conn_slots, nb_off, nb_slots, n, &ht[0], &ht[1]};
    KfdbState st = db->st;
    std::vector<int32_t> off, cand;
    OLF_TRY(kfdb_select(a, has_lines, st, off, cand));
    if (cand.size() > (size_t)cand_capacity) { set_error("olf_kfdb_detect: more candidates than cand_capacity"); return OLF_ERR_CAPACITY; }
    db->st = st;
    std::copy(off.begin(), off.end(), cand_off);
    std::copy(cand.begin(), cand.end(), cand_slots);
    return OLF_OK;
}

int olf_bow_score_pairs_dev(olf_kfdb* db, int line, int n_pairs, const int32_t* d_pairs, const olf_bow_csr* d_queries, int n_queries, double* d_score,
                            void* stream)
{
    if (!db || (line != 0 && line != 1) || n_pairs < 0 || n_queries < 0 || (n_pairs > 0 && (!d_pairs || !d_score)) || (d_queries && !csr_whole(d_queries))) {
        set_error("olf_bow_score_pairs_dev: bad argument"); return OLF_ERR_INVALID;
    }
    if (!db->ctx) { set_error("olf_bow_score_pairs_dev: the database was created without a context"); return OLF_ERR_INVALID; }
    const KfdbVectors& v = db->v[line];
    if (v.n_words == 0) { set_error("olf_bow_score_pairs_dev: the database has no line vocabulary"); return OLF_ERR_INVALID; }
    OLF_TRY(ctx_check_device(db->ctx, "olf_bow_score_pairs_dev"));
    // an empty database has no device arrays yet: every pair is out of range, and the kernel reads none of them
    hipStream_t s = ctx_stream(db->ctx, stream);
    if (d_queries) return launch_bow_score_pairs(d_pairs, n_pairs, d_queries->off, nullptr, n_queries, d_queries->ids, d_queries->vals, v.d_beg, v.d_len,
                                                 db->n_slots, v.d_ids, v.d_vals, d_score, s);
    return launch_bow_score_pairs(d_pairs, n_pairs, v.d_beg, v.d_len, db->n_slots, v.d_ids, v.d_vals, v.d_beg, v.d_len, db->n_slots, v.d_ids, v.d_vals, d_score, s);
}

int olf_bow_score(olf_ctx* ctx, const int32_t* ids_a, const double* vals_a, int n_a, const int32_t* ids_b, const double* vals_b, int n_b, double* score)
{
    if (!ctx || !score || !vector_ok(ids_a, vals_a, n_a, INT_MAX) || !vector_ok(ids_b, vals_b, n_b, INT_MAX)) {
        set_error("olf_bow_score: bad argument (word ids ascending and distinct)"); return OLF_ERR_INVALID;
    }
    HostCall h(ctx, "olf_bow_score");
    int32_t *d_ia, *d_ib, *d_small; double *d_va, *d_vb, *d_s;
    h.add(&d_ia, n_a); h.add(&d_ib, n_b); h.add(&d_va, n_a); h.add(&d_vb, n_b); h.add(&d_small, 6); h.add(&d_s, 1);
    OLF_TRY(h.bind(SCRATCH_STAGE));
    const int32_t small[6] = {0, n_a, 0, n_b, 0, 0};      // a as a one-vector CSR; b's begin and length; the pair (0, 0)
    OLF_TRY(h.up(d_ia, ids_a, (size_t)n_a * 4)); OLF_TRY(h.up(d_va, vals_a, (size_t)n_a * 8));
    OLF_TRY(h.up(d_ib, ids_b, (size_t)n_b * 4)); OLF_TRY(h.up(d_vb, vals_b, (size_t)n_b * 8));
    OLF_TRY(h.up(d_small, small, sizeof(small)));
    OLF_TRY(launch_bow_score_pairs(d_small + 4, 1, d_small, nullptr, 1, d_ia, d_va, d_small + 2, d_small + 3, 1, d_ib, d_vb, d_s, h.stream()));
    OLF_TRY(h.down(score, d_s, 8));
    return h.finish();
}

}  // extern "C"
