// posepoints_host.cpp -- olf_pose_optimization: int Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:239-451) for one row on the host.  Plain C++
// doubles, every sum in the order of the reference's _activeEdges (ascending feature index, the two kinds interleaved), no context and no device: the
// definition the kernel of posepoints_batch.hip is read against.  The edges' terms and the driver of the four passes are
// posepoints_terms.hpp, the LDLT and the Levenberg loop g2o_levenberg.hpp, shared with the kernel; this file owns the loops over a row's edges.
#include <algorithm>
#include <string>
#include <vector>
#include "posepoints_terms.hpp"
#include "../../include/orbline.h"

namespace olf { void set_error(const std::string& s); }

using namespace olf;
using namespace olf::posepoints;

namespace {

struct HostOps {
    Cam c;
    int n = 0;
    const olf_keypoint* kps = nullptr;
    const float* ur = nullptr;
    std::vector<const float*> Xw;                                    // the held point's world position, NULL: holds nothing
    std::vector<uint8_t> f;                                          // E_HELD | E_OUT | E_STEREO
    std::vector<double> w, err;                                      // invSigma2 widened; the edge's current _error [3]
    float* chi2 = nullptr;

    void load(int i, double* X, double* obs) const
    {
        X[0] = (double)Xw[i][0]; X[1] = (double)Xw[i][1]; X[2] = (double)Xw[i][2];
        obs[0] = (double)kps[i].x; obs[1] = (double)kps[i].y; obs[2] = (double)ur[i];
    }
    int n_edges() const { int k = 0; for (int i = 0; i < n; ++i) k += (f[i] & E_HELD) != 0; return k; }
    int n_active() const { int k = 0; for (int i = 0; i < n; ++i) k += (f[i] & (E_HELD | E_OUT)) == E_HELD; return k; }
    bool errors(const VertexSE3& v, bool robust, double* chi)
    {
        double s = 0.0, X[3], obs[3];
        bool ok = true;
        for (int i = 0; i < n; ++i) if ((f[i] & (E_HELD | E_OUT)) == E_HELD) {
            load(i, X, obs);
            if (!edge_error(c, v.est, X, obs, f[i] & E_STEREO, &err[3 * i])) { ok = false; continue; }
            s = s + edge_robust_chi2(&err[3 * i], w[i], f[i] & E_STEREO, robust);
        }
        *chi = s;
        return ok;
    }
    bool system(const VertexSE3& v, bool robust, double* S)
    {
        double X[3], obs[3];
        bool ok = true;
        for (int k = 0; k < 27; ++k) S[k] = 0.0;
        for (int i = 0; i < n; ++i) if ((f[i] & (E_HELD | E_OUT)) == E_HELD) {
            load(i, X, obs);
            ok = edge_quadratic_form(c, v.est, X, &err[3 * i], w[i], f[i] & E_STEREO, robust, S) && ok;
        }
        return ok;
    }
    bool classify(const Se3& est, int* n_bad)
    {
        double X[3], obs[3];
        for (int i = 0; i < n; ++i) if ((f[i] & (E_HELD | E_OUT)) == (E_HELD | E_OUT)) {      // first every computeError: a depth of 0 leaves the flags as they stood
            load(i, X, obs);
            if (!edge_error(c, est, X, obs, f[i] & E_STEREO, &err[3 * i])) return false;
        }
        int bad = 0;
        for (int i = 0; i < n; ++i) if (f[i] & E_HELD) {
            const float v = (float)edge_chi2(&err[3 * i], w[i], f[i] & E_STEREO);
            chi2[i] = v;
            if (v > chi2_threshold(f[i] & E_STEREO)) { f[i] |= E_OUT; ++bad; } else f[i] &= ~E_OUT;
        }
        *n_bad = bad;
        return true;
    }
};

}  // namespace

extern "C" int olf_pose_optimization(const olf_pose_points_batch* in, int capacity, int n_frames, const float* inv_level_sigma2, int n_levels,
                                     const olf_pose_points_outputs* o)
{
    const char* who = "olf_pose_optimization";
    bool ok = in && o && capacity >= 0 && n_frames >= 1 && n_levels >= 0 && n_levels <= OLF_MAX_LEVELS && (inv_level_sigma2 || !n_levels);
    ok = ok && in->counts && in->Tcw && in->n_mp >= 0 && in->img_stride >= 1 && (in->mp_world || !in->n_mp);
    ok = ok && ((in->kps && in->uright && in->frame_mp && o->outlier_out && o->chi2) || !capacity);
    ok = ok && o->Tcw_out && o->n_good && o->n_initial && o->passes && o->iters && o->status;
    if (!ok) { set_error(std::string(who) + ": bad argument"); return OLF_ERR_INVALID; }

    *o->status = 0;
    if (in->row_active && in->row_active[0] <= 0) { *o->n_good = -1; return OLF_OK; }
    int frame = 0;
    long long base = in->mp_index_offset ? in->mp_index_offset[0] : 0;
    if (in->pairs) {
        const int kf = in->pairs[0];
        frame = in->pairs[1];
        if (kf < 0 || kf >= n_frames || frame < 0 || frame >= n_frames || kf == frame) { *o->n_good = -1; *o->status = 2048; return OLF_OK; }
        base += (long long)kf * capacity;
    }
    const size_t img = (size_t)frame * in->img_stride;
    const int n = std::max(0, std::min(in->counts[img], capacity));
    HostOps ops;
    ops.c = {(double)in->fx, (double)in->fy, (double)in->cx, (double)in->cy, (double)in->bf};
    ops.n = n;
    ops.kps = in->kps + img * capacity;
    ops.ur = in->uright + (size_t)frame * capacity;
    ops.Xw.assign(n, nullptr); ops.f.assign(n, 0); ops.w.assign(n, 0.0); ops.err.assign(3 * (size_t)n, 0.0);
    ops.chi2 = o->chi2;
    int status = 0;
    for (int i = 0; i < capacity; ++i) { o->outlier_out[i] = 0; o->chi2[i] = 0.f; }
    for (int i = 0; i < n; ++i) {
        if (in->frame_mp[i] < 0) continue;
        const long long m = in->frame_mp[i] + base;
        if (m < 0 || m >= in->n_mp) { status |= 512; continue; }        // (no context here: the bits a context would raise go into the row's word)
        const int oct = ops.kps[i].octave;
        if (oct < 0 || oct >= n_levels) { status |= ST_OCTAVE; continue; }
        ops.Xw[i] = in->mp_world + 3 * m;
        ops.f[i] = E_HELD | (ops.ur[i] < 0.f ? 0 : E_STEREO);           // :286
        ops.w[i] = (double)inv_level_sigma2[oct];
    }
    Result r;
    run_row(ops, in->Tcw, &r);
    for (int i = 0; i < 16; ++i) o->Tcw_out[i] = r.Tcw[i];
    for (int i = 0; i < n; ++i) o->outlier_out[i] = (ops.f[i] & E_OUT) ? 1 : 0;
    *o->n_good = r.n_good; *o->n_initial = r.n_initial; *o->passes = r.passes;
    for (int p = 0; p < 4; ++p) o->iters[p] = r.iters[p];
    *o->status = status | r.status;
    return OLF_OK;
}
