// pose_host.cpp -- olf_pose_optimization_with_line and olf_discard_outliers: Optimizer::PoseOptimizationWithLine (src/Optimizer.cc:604-697) and the
// "discard outliers" loops that follow its three calls (src/Tracking.cc:1034-1074, :1547-1590) for one frame on the host.  Plain C++ doubles, every sum
// in the reference's index order, no context and no device: the definition the kernel of pose_batch.hip is read against.  The terms, the dense pieces and
// the driver of the four passes are pose_terms.hpp, shared with the kernel; this file owns the loops over a frame's features.
#include <algorithm>
#include <string>
#include <vector>
#include "pose_terms.hpp"
#include "../../include/orbline.h"

namespace olf { void set_error(const std::string& s); }

using namespace olf;
using namespace olf::pose;

namespace {

// element n / 2 of the ascending keys (src/Auxiliar.cc:410-415); n > 0
double middle(std::vector<uint64_t>& k)
{
    std::nth_element(k.begin(), k.begin() + k.size() / 2, k.end());
    return value_of(k[k.size() / 2]);
}
// 1.4826 * MAD (vector_stdv_mad), and the median with it; 0 for no residual
double stdv_mad(const std::vector<double>& res, double* median)
{
    *median = 0.0;
    if (res.empty()) return 0.0;
    std::vector<uint64_t> k(res.size());
    for (size_t i = 0; i < res.size(); ++i) k[i] = key_of(res[i]);
    *median = middle(k);
    for (size_t i = 0; i < res.size(); ++i) k[i] = key_of(mad_dev(res[i], *median));
    return 1.4826 * middle(k);
}

struct HostOps {
    Cfg c;
    int n = 0, nl = 0;
    const olf_keypoint* kps = nullptr;
    const olf_keyline* kls = nullptr;
    const double* lle = nullptr;
    std::vector<const float*> Xw, Lw;                                // the held feature's world position, NULL: holds nothing
    std::vector<double> P, L, sq, sql;
    uint8_t *out = nullptr, *outl = nullptr;                         // mvbOutlier, mvbOutlier_Line

    void prepare(const double* Tlw)
    {
        for (int i = 0; i < n; ++i) if (Xw[i]) { const double X[3] = {(double)Xw[i][0], (double)Xw[i][1], (double)Xw[i][2]}; transform3(Tlw, X, &P[3 * i]); }
        for (int i = 0; i < nl; ++i) if (Lw[i]) {
            const double s[3] = {(double)Lw[i][0], (double)Lw[i][1], (double)Lw[i][2]}, e[3] = {(double)Lw[i][3], (double)Lw[i][4], (double)Lw[i][5]};
            transform3(Tlw, s, &L[6 * i]);
            transform3(Tlw, e, &L[6 * i + 3]);
        }
    }
    void line_obs(int i, double* o) const { o[0] = kls[i].startPointX; o[1] = kls[i].startPointY; o[2] = kls[i].endPointX; o[3] = kls[i].endPointY; }
    void sums(const double* DT, int robust, double sp, double sl, double* S, int* cnt)
    {
        double Sp[N_SUMS] = {0}, Sl[N_SUMS] = {0};
        int np = 0, nln = 0;
        for (int i = 0; i < n; ++i) if (Xw[i] && !out[i]) { accumulate_point(c, DT, &P[3 * i], kps[i].x, kps[i].y, robust, sq[i], sp, Sp); ++np; }
        for (int i = 0; i < nl; ++i) if (Lw[i] && !outl[i]) {
            double o[4];
            line_obs(i, o);
            accumulate_line(c, DT, &L[6 * i], &lle[3 * i], o, robust, sql[i], sl, Sl);
            ++nln;
        }
        for (int k = 0; k < N_SUMS; ++k) S[k] = Sp[k] + Sl[k];
        *cnt = nln + np;
    }
    void robust_scales(const double* DT, double* sp, double* sl)
    {
        std::vector<double> rp, rl;
        double med;
        for (int i = 0; i < n; ++i) if (Xw[i] && !out[i]) rp.push_back(point_term(c, DT, &P[3 * i], kps[i].x, kps[i].y, nullptr));
        for (int i = 0; i < nl; ++i) if (Lw[i] && !outl[i]) rl.push_back(line_term(c, DT, &L[6 * i], &lle[3 * i], nullptr, nullptr, nullptr));
        *sp = stdv_mad(rp, &med);
        *sl = stdv_mad(rl, &med);
    }
    // vector_mean_stdv_mad and the flag loop of removeOutliers for one kind; res in index order of the held features idx
    void decide(const std::vector<double>& res, const std::vector<int>& idx, uint8_t* flag) const
    {
        if (res.empty()) return;
        double med, sum_below = 0.0, sum_all = 0.0;
        const double stdv = stdv_mad(res, &med);
        int k = 0;
        for (double r : res) { if (r < 2.0 * stdv) { sum_below += r; ++k; } sum_all += r; }
        const double mean = mad_mean(sum_below, k, sum_all, (int)res.size()), th = c.inlier_k * stdv;
        for (size_t j = 0; j < res.size(); ++j) flag[idx[j]] = is_outlier(res[j], mean, th) ? 1 : 0;
    }
    void remove_outliers(const double* DT)
    {
        std::vector<double> res;
        std::vector<int> idx;
        if (c.has_points) {
            for (int i = 0; i < n; ++i) if (Xw[i]) { res.push_back(point_term(c, DT, &P[3 * i], kps[i].x, kps[i].y, nullptr) * sq[i]); idx.push_back(i); }
            decide(res, idx, out);
        }
        if (c.has_lines) {
            res.clear(); idx.clear();
            for (int i = 0; i < nl; ++i) if (Lw[i]) { res.push_back(line_term(c, DT, &L[6 * i], &lle[3 * i], nullptr, nullptr, nullptr) * sql[i]); idx.push_back(i); }
            decide(res, idx, outl);
        }
    }
};

bool params_ok(const olf_pose_params* p)
{
    return p && p->max_iters_ref >= 1 && p->homog_th > 0.0 && p->inlier_k >= 0.0;
}

}  // namespace

extern "C" void olf_pose_default_params(olf_pose_params* p)
{
    if (!p) return;
    p->max_iters_ref = 10; p->homog_th = 1e-7; p->min_error = 1e-7; p->min_error_change = 1e-7; p->inlier_k = 4.0;      // src/Config.cpp:76-82
    p->use_motion_model = 1; p->has_points = 1; p->has_lines = 1;                                                        // :42-49
}

extern "C" int olf_pose_optimization_with_line(const olf_pose_batch* in, int capacity, int line_capacity, const float* inv_level_sigma2, int n_levels,
                                               const olf_pose_params* params, const olf_pose_outputs* o)
{
    const char* who = "olf_pose_optimization_with_line";
    bool ok = in && o && params_ok(params) && capacity >= 0 && line_capacity >= 0 && n_levels >= 0 && n_levels <= OLF_MAX_LEVELS && (inv_level_sigma2 || !n_levels);
    ok = ok && in->Tcw && in->counts && in->lcounts && in->n_mp >= 0 && in->n_ml >= 0;
    ok = ok && o->Tcw_out && o->DT && o->DT_cov && o->DT_cov_eig && o->err_norm && o->good && o->n_inliers && o->iters && o->status;
    ok = ok && ((in->kps && in->frame_mp && o->outlier_out) || !capacity) && ((in->kls && in->lle && in->frame_ml && o->outlier_l_out) || !line_capacity);
    ok = ok && (in->mp_world || !in->n_mp) && (in->ml_world || !in->n_ml);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }

    HostOps ops;
    Cfg& c = ops.c;
    c.max_iters = params->max_iters_ref; c.homog_th = params->homog_th; c.min_error = params->min_error; c.min_error_change = params->min_error_change;
    c.inlier_k = params->inlier_k; c.use_motion_model = params->use_motion_model != 0; c.has_points = params->has_points != 0; c.has_lines = params->has_lines != 0;
    c.fx = in->fx; c.fy = in->fy; c.cx = in->cx; c.cy = in->cy;
    const int n = std::max(0, std::min(in->counts[0], capacity)), nl = std::max(0, std::min(in->lcounts[0], line_capacity));
    ops.n = n; ops.nl = nl; ops.kps = in->kps; ops.kls = in->kls; ops.lle = in->lle;
    ops.Xw.assign(n, nullptr); ops.Lw.assign(nl, nullptr); ops.P.assign(3 * (size_t)n, 0.0); ops.L.assign(6 * (size_t)nl, 0.0); ops.sq.assign(n, 0.0); ops.sql.assign(nl, 0.0);
    int status = 0;
    const long long off = in->mp_index_offset ? in->mp_index_offset[0] : 0, offl = in->ml_index_offset ? in->ml_index_offset[0] : 0;
    for (int i = 0; i < capacity; ++i) o->outlier_out[i] = (i < n && in->outlier) ? (in->outlier[i] != 0) : 0;
    for (int i = 0; i < line_capacity; ++i) o->outlier_l_out[i] = (i < nl && in->outlier_l) ? (in->outlier_l[i] != 0) : 0;
    ops.out = o->outlier_out; ops.outl = o->outlier_l_out;
    for (int i = 0; i < n; ++i) {
        if (in->frame_mp[i] < 0) continue;
        const long long m = in->frame_mp[i] + off;
        if (m < 0 || m >= in->n_mp) { status |= 512; continue; }        // (no context here: the bits a context would raise go into the frame's word)
        const int oct = in->kps[i].octave;
        if (oct < 0 || oct >= n_levels) { status |= ST_OCTAVE; continue; }
        ops.Xw[i] = in->mp_world + 3 * m;
        ops.sq[i] = sqrt((double)inv_level_sigma2[oct]);
    }
    for (int i = 0; i < nl; ++i) {
        if (in->frame_ml[i] < 0) continue;
        const long long m = in->frame_ml[i] + offl;
        if (m < 0 || m >= in->n_ml) { status |= 1024; continue; }
        const int oct = in->kls[i].octave;
        if (oct < 0 || oct >= n_levels) { status |= ST_OCTAVE; continue; }
        ops.Lw[i] = in->ml_world + 6 * m;
        ops.sql[i] = sqrt((double)inv_level_sigma2[oct]);
    }
    for (int i = 0; i < n; ++i) if (!ops.Xw[i]) o->outlier_out[i] = 0;          // a flag stands for a held feature only
    for (int i = 0; i < nl; ++i) if (!ops.Lw[i]) o->outlier_l_out[i] = 0;

    Result r;
    run_frame(ops, c, in->Tcw, in->Tcw_prev ? in->Tcw_prev : in->Tcw, in->DT_cov_in, &r);
    for (int i = 0; i < 16; ++i) { o->Tcw_out[i] = r.Tcw[i]; o->DT[i] = r.DT[i]; }
    for (int i = 0; i < 36; ++i) o->DT_cov[i] = r.cov[i];
    for (int i = 0; i < 6; ++i) o->DT_cov_eig[i] = r.eig[i];
    *o->err_norm = r.err;
    *o->good = (uint8_t)r.good;
    int np = 0, nln = 0;
    for (int i = 0; i < n; ++i) np += ops.Xw[i] && !o->outlier_out[i];
    for (int i = 0; i < nl; ++i) nln += ops.Lw[i] && !o->outlier_l_out[i];
    o->n_inliers[0] = np; o->n_inliers[1] = nln;
    for (int p = 0; p < 4; ++p) o->iters[p] = r.iters[p];
    *o->status = status | r.status;
    return OLF_OK;
}

namespace {
// one kind of one frame: the loops of src/Tracking.cc:1036-1054 (mode 0) and :1549-1568 (mode 1)
int discard_row(int n, int32_t* held, uint8_t* outlier, long long off, const uint8_t* obs, int n_map, int mode, int only_tracking, int stereo, int bit, int* status)
{
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        if (held[i] < 0) continue;
        const long long m = held[i] + off;
        if (m < 0 || m >= n_map) { *status |= bit; continue; }
        const bool seen = !obs || obs[m];
        if (mode == 0) {
            if (outlier[i]) { held[i] = -1; outlier[i] = 0; }
            else if (seen) ++cnt;
        } else {
            if (!outlier[i]) cnt += only_tracking || seen;
            else if (stereo) held[i] = -1;
        }
    }
    return cnt;
}
}  // namespace

extern "C" int olf_discard_outliers(const olf_discard_batch* io, int capacity, int line_capacity, int mode, int only_tracking, int stereo, int32_t* n_matches,
                                    int32_t* status)
{
    const char* who = "olf_discard_outliers";
    bool ok = io && n_matches && status && capacity >= 0 && line_capacity >= 0 && (mode == 0 || mode == 1) && io->counts && io->lcounts && io->n_mp >= 0 && io->n_ml >= 0;
    ok = ok && ((io->frame_mp && io->outlier) || !capacity) && ((io->frame_ml && io->outlier_l) || !line_capacity);
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }
    const int n = std::max(0, std::min(io->counts[0], capacity)), nl = std::max(0, std::min(io->lcounts[0], line_capacity));
    int st = 0;
    n_matches[0] = discard_row(n, io->frame_mp, io->outlier, io->mp_index_offset ? io->mp_index_offset[0] : 0, io->mp_obs, io->n_mp, mode, only_tracking != 0,
                               stereo != 0, 512, &st);
    n_matches[1] = discard_row(nl, io->frame_ml, io->outlier_l, io->ml_index_offset ? io->ml_index_offset[0] : 0, io->ml_obs, io->n_ml, mode, only_tracking != 0,
                               stereo != 0, 1024, &st);
    *status = st;
    return OLF_OK;
}
