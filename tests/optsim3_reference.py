"""A numpy restatement of int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:2013-2208) with everything it
executes through g2o (Thirdparty/g2o/g2o: types/sim3.h, types/types_seven_dof_expmap.h, types/se3_ops.hpp, core/base_edge.h,
core/base_binary_edge.hpp:55-204, core/robust_kernel_impl.cpp, core/optimization_algorithm_levenberg.cpp:61-189, core/sparse_optimizer.cpp:354-419,
solvers/linear_solver_dense.h) and the epilogue of LoopClosing::ComputeSim3 (src/LoopClosing.cc:339-341, src/Converter.cc:57-63), written from those
files.  It reads nothing from the library.  The Eigen pieces that posepoints_reference already restates from Eigen's text (Quaterniond(Matrix3d),
toRotationMatrix, Quaterniond * Vector3d, the quaternion product, LDLT) are taken from there.  Per-edge arithmetic is vectorised over the edges; the
sums over the edges run in the reference's order, e12_i then e21_i for ascending i.

The linearisation is g2o's numeric one, literally: per dimension d, oplus(+1e-9 e_d), computeError, pop, oplus(-1e-9 e_d), computeError, pop, column =
(1 / (2 * 1e-9)) * (e_plus - e_minus), _error restored.  (The perturbed vertex is the same for every edge, so forming it once per d is g2o's own values.)

Switches, as posepoints_reference (a namespace ldlt / acc / rev / flip): another LDLT, the sums' terms perturbed by a float32 rounding, the sums
reversed, and every Levenberg trial whose two chi2 differ by less than FLIP_MARGIN of their size taken the other way.
What the reference leaves undefined is defined as include/orbline.h defines it: a depth of exactly 0 at any evaluation (status 1) or a non-finite H, b,
step or estimate (status 2) stops the pair with the input S12, the matches as they stood and n_inliers = 0."""
import math
import types
import numpy as np
import posepoints_reference as PR
from posepoints_reference import BASE, SWITCHED, FLIP_MARGIN, DBL_MAX, Stop, csum, quat_of, rotation_of, rotate, quat_mul, skew, mat3, ldlt_eigen, ldlt_numpy

F = np.float32
ST_DEPTH, ST_NOT_FINITE, ST_OCTAVE, STATUS_PAIR = 1, 2, 4, 2048
I3 = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


# ---- g2o::Sim3 as (q, t, s), q = x, y, z, w, never normalised
def sim3_of_update(u):
    """Sim3(const Vector7d& update), sim3.h:70-142"""
    omega, upsilon, sigma = list(u[:3]), list(u[3:6]), u[6]
    theta = math.sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2])
    Omega = skew(omega)
    s = math.exp(sigma)
    Omega2 = mat3(Omega, Omega)
    eps = 0.00001
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B = 1. / 2., 1. / 6.
            OO = mat3(Omega, Omega)
            R = [[(I3[i][j] + Omega[i][j]) + OO[i][j] for j in range(3)] for i in range(3)]
        else:
            theta2 = theta * theta
            A = (1 - math.cos(theta)) / (theta2)
            B = (theta - math.sin(theta)) / (theta2 * theta)
            ra, rb = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
            R = [[(I3[i][j] + ra * Omega[i][j]) + rb * Omega2[i][j] for j in range(3)] for i in range(3)]
    else:
        C = (s - 1) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = [[(I3[i][j] + Omega[i][j]) + Omega2[i][j] for j in range(3)] for i in range(3)]
        else:
            ra, rb = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
            R = [[(I3[i][j] + ra * Omega[i][j]) + rb * Omega2[i][j] for j in range(3)] for i in range(3)]
            a = s * math.sin(theta)
            b = s * math.cos(theta)
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2)
    r = quat_of(R)
    W = [[(A * Omega[i][j] + B * Omega2[i][j]) + C * I3[i][j] for j in range(3)] for i in range(3)]
    t = [(W[i][0] * upsilon[0] + W[i][1] * upsilon[1]) + W[i][2] * upsilon[2] for i in range(3)]
    return r, t, s


def sim3_map(S, X):
    """s * (r * xyz) + t; X may hold arrays"""
    r = rotate(S[0], X)
    return [S[2] * r[i] + S[1][i] for i in range(3)]


def sim3_inverse(S):
    q, t, s = S
    qc = [-q[0], -q[1], -q[2], q[3]]
    f = -1. / s
    return qc, rotate(qc, [f * t[0], f * t[1], f * t[2]]), 1. / s


def sim3_mul(a, b):
    r = rotate(a[0], b[1])
    return quat_mul(a[0], b[0]), [a[2] * r[i] + a[1][i] for i in range(3)], a[2] * b[2]


def sim3_finite(S):
    return all(math.isfinite(v) for v in list(S[0]) + list(S[1]) + [S[2]])


def oplus(est, update, fix_scale):
    """VertexSim3Expmap::oplusImpl: update[6] = 0 is written into the caller's list"""
    if fix_scale:
        update[6] = 0.0
    return sim3_mul(sim3_of_update(update), est)


def cam_points(Tcw, world):
    """R * P + t of CV_32F matrices, then widened: the products summed in float, the t term added in double, one rounding (DESIGN C.12)"""
    T = np.asarray(Tcw, F).reshape(4, 4)
    P = np.asarray(world, F).reshape(-1, 3)
    out = np.zeros((P.shape[0], 3))
    for r in range(3):
        d = (T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1]) + T[r, 2] * P[:, 2]
        out[:, r] = (d.astype(np.float64) + float(T[r, 3])).astype(F).astype(np.float64)
    return out


def interleave(a, b):
    """terms of e12_i and e21_i in graph order"""
    return np.stack([a, b], axis=1).reshape((-1,) + a.shape[1:])


class Graph:
    def __init__(self, P1, P2, obs1, obs2, w1, w2, camera, delta, fix_scale, sw):
        self.sw, self.n, self.fix_scale, self.delta = sw, len(P1), fix_scale, delta
        self.fx, self.fy, self.cx, self.cy = (float(F(v)) for v in camera[:4])
        self.P1, self.P2, self.obs1, self.obs2, self.w1, self.w2 = P1, P2, obs1, obs2, w1, w2
        self.err = np.zeros((self.n, 4))
        self.removed = np.zeros(self.n, bool)
        self.log = types.SimpleNamespace(decisions=[], checks=[])

    def active(self):
        return np.nonzero(~self.removed)[0]

    def edge_error(self, S, X, obs):
        x, y, z = sim3_map(S, [X[:, 0], X[:, 1], X[:, 2]])
        if np.any(z == 0.0):
            raise Stop(ST_DEPTH)
        with np.errstate(all="ignore"):
            return np.stack([obs[:, 0] - ((x / z) * self.fx + self.cx), obs[:, 1] - ((y / z) * self.fy + self.cy)], axis=1)

    def errors_at(self, est, idx):
        """computeError of e12 and e21 of the correspondences idx: [n, 4]"""
        if len(idx) == 0:
            return np.zeros((0, 4))
        e12 = self.edge_error(est, self.P2[idx], self.obs1[idx])
        e21 = self.edge_error(sim3_inverse(est), self.P1[idx], self.obs2[idx])
        return np.concatenate([e12, e21], axis=1)

    def compute_error(self, est, idx):
        self.err[idx] = self.errors_at(est, idx)

    def chi2(self, idx):
        e, w1, w2 = self.err[idx], self.w1[idx], self.w2[idx]
        return e[:, 0] * (w1 * e[:, 0]) + e[:, 1] * (w1 * e[:, 1]), e[:, 2] * (w2 * e[:, 2]) + e[:, 3] * (w2 * e[:, 3])

    def rho(self, e):
        dsqr = self.delta * self.delta
        with np.errstate(all="ignore"):
            sq = np.sqrt(e)
            r0, r1 = (2 * sq) * self.delta - dsqr, self.delta / sq
        inl = e <= dsqr
        return np.where(inl, e, r0), np.where(inl, 1.0, r1)

    def active_robust_chi2(self):
        a, b = self.chi2(self.active())
        return float(csum(interleave(self.rho(a)[0], self.rho(b)[0]), self.sw))

    def build_system(self, est):
        idx = self.active()
        delta = 1e-9
        scalar = 1.0 / (2 * delta)
        J = np.zeros((len(idx), 4, 7))                               # rows 0-1: e12's Jacobian, 2-3: e21's
        add = [0.0] * 7
        for d in range(7):
            add[d] = delta
            bak = self.errors_at(oplus(est, add, self.fix_scale), idx)
            add[d] = -delta
            bak = bak - self.errors_at(oplus(est, add, self.fix_scale), idx)
            add[d] = 0.0
            J[:, :, d] = scalar * bak
        e, w1, w2 = self.err[idx], self.w1[idx], self.w2[idx]
        c1, c2 = self.chi2(idx)
        r1, r2 = self.rho(c1)[1], self.rho(c2)[1]
        ww1, ww2 = r1 * w1, r2 * w2
        H = [[0.0] * 7 for _ in range(7)]
        for i in range(7):
            for j in range(i + 1):
                t12 = (J[:, 0, i] * ww1) * J[:, 0, j] + (J[:, 1, i] * ww1) * J[:, 1, j]
                t21 = (J[:, 2, i] * ww2) * J[:, 2, j] + (J[:, 3, i] * ww2) * J[:, 3, j]
                H[i][j] = float(csum(interleave(t12, t21), self.sw))
                H[j][i] = H[i][j]
        o12 = [((-w1) * e[:, 0]) * r1, ((-w1) * e[:, 1]) * r1]       # omega_r = -omega * _error; omega_r *= rho[1]
        o21 = [((-w2) * e[:, 2]) * r2, ((-w2) * e[:, 3]) * r2]
        b = []
        for i in range(7):
            b.append(float(csum(interleave(J[:, 0, i] * o12[0] + J[:, 1, i] * o12[1], J[:, 2, i] * o21[0] + J[:, 3, i] * o21[1]), self.sw)))
        if not all(math.isfinite(v) for r in H for v in r) or not all(math.isfinite(v) for v in b):
            raise Stop(ST_NOT_FINITE)
        return H, b

    def optimize(self, est, iterations):
        """SparseOptimizer::optimize over OptimizationAlgorithmLevenberg::solve; returns the estimate and the iterations run"""
        log = self.log.decisions
        lam, ni, n_bad, x, done = -1.0, 2.0, 0, [0.0] * 7, 0
        for it in range(iterations):
            self.compute_error(est, self.active())
            cur = self.active_robust_chi2()
            ini = cur
            H, b = self.build_system(est)
            if it == 0:
                lam, ni, n_bad = 1e-5 * max([0.0] + [abs(H[j][j]) for j in range(7)]), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                backup = est
                Hl = [[H[i][j] + (lam if i == j else 0.0) for j in range(7)] for i in range(7)]
                ok2, sol = (ldlt_eigen if self.sw.ldlt == "eigen" else ldlt_numpy)(Hl, b)
                if ok2:
                    x = list(sol)
                if not all(math.isfinite(v) for v in x):
                    raise Stop(ST_NOT_FINITE)
                est = oplus(est, x, self.fix_scale)
                if not sim3_finite(est):
                    raise Stop(ST_NOT_FINITE)
                self.compute_error(est, self.active())
                tmp = self.active_robust_chi2()
                if not ok2:
                    tmp = DBL_MAX
                rho = cur - tmp
                scale = 0.0
                for j in range(7):
                    scale = scale + x[j] * (lam * x[j] + b[j])
                scale = scale + 1e-3
                rho = rho / scale
                if self.sw.flip and math.isfinite(tmp) and abs(cur - tmp) < FLIP_MARGIN * max(abs(cur), abs(tmp)):
                    rho = -rho
                accept = rho > 0 and math.isfinite(tmp)
                log.append(("trial", accept, cur, tmp, max(abs(v) for v in x)))
                if accept:
                    alpha = min(1.0 - math.pow(2 * rho - 1, 3), 2.0 / 3.0)
                    lam, ni, cur = lam * max(1.0 / 3.0, alpha), 2.0, tmp
                else:
                    lam, ni, est = lam * ni, ni * 2.0, backup
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            done += 1
            if qmax == 10 or rho == 0:
                break
            stop = (ini - cur) * 1e3 < ini
            log.append(("stop", stop, (ini - cur) * 1e3, ini, 0.0))
            n_bad = n_bad + 1 if stop else 0
            if n_bad >= 3:
                break
        return est, done


def to_scw(S12, T2w):
    """toCvMat(gScm * Sim3(R2w, t2w, 1.0)): s * R and t rounded to float"""
    T = np.asarray(T2w, F).reshape(4, 4).astype(np.float64)
    g = sim3_mul(S12, (quat_of(T[:3, :3].tolist()), [float(T[0, 3]), float(T[1, 3]), float(T[2, 3])], 1.0))
    R = rotation_of(g[0])
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = g[2] * R[i][j]
        out[i, 3] = g[1][i]
    return out.astype(F).reshape(16)


def outputs_of(S, T2w):
    q, t, s = S
    return dict(S12_out=np.array(list(q) + list(t) + [s], np.float64), s12_out=F(s), R12_out=np.array(rotation_of(q), np.float64).astype(F).reshape(9),
                t12_out=np.array(t, np.float64).astype(F), Scw_out=to_scw(S, T2w))


def optimize_sim3(scene, sw=BASE):
    """One call on a scene of optsim3_scenes (two key frames and a match row).  Returns a dict: matches [capacity] int32, S12_out [8], s12_out, R12_out [9],
    t12_out [3], Scw_out [16], n_inliers, n_correspondences, n_bad_first, iters [2], status, chi2 [capacity, 2] float32, log."""
    s = scene
    cap = s["matches"].shape[0]
    N1, N2 = int(s["counts"][0]), int(s["counts"][1])
    matches = s["matches"].astype(np.int32).copy()
    sig = np.asarray(s["inv_level_sigma2"], F)
    kp1, kp2 = s["keys"][0], s["keys"][1]
    status, corr = 0, []
    for i in range(N1):
        v = int(matches[i])
        if not (0 <= v < N2):
            continue
        if not (s["valid"][0][i] and s["valid"][1][v]) or s["bad"][0][i] or s["bad"][1][v]:
            continue
        o1, o2 = int(kp1["octave"][i]), int(kp2["octave"][v])
        if not (0 <= o1 < sig.shape[0] and 0 <= o2 < sig.shape[0]):
            status |= ST_OCTAVE
            continue
        corr.append((i, v))
    i1 = np.array([c[0] for c in corr], np.int64)
    i2 = np.array([c[1] for c in corr], np.int64)
    th2 = float(F(s["th2"]))
    delta = float(F(math.sqrt(th2)))                                 # const float deltaHuber = sqrt(th2)
    g = Graph(cam_points(s["Tcw"][0], s["world"][0][i1]), cam_points(s["Tcw"][1], s["world"][1][i2]),
              np.column_stack([kp1["x"][i1], kp1["y"][i1]]).astype(np.float64), np.column_stack([kp2["x"][i2], kp2["y"][i2]]).astype(np.float64),
              sig[kp1["octave"][i1]].astype(np.float64), sig[kp2["octave"][i2]].astype(np.float64), s["camera"], delta, bool(s["fix_scale"]), sw)
    R12 = np.asarray(s["R12"], F).reshape(3, 3).astype(np.float64)
    S_in = (quat_of(R12.tolist()), [float(F(v)) for v in s["t12"]], float(F(s["s12"])))
    out = dict(matches=matches, n_inliers=0, n_correspondences=len(corr), n_bad_first=0, iters=np.zeros(2, np.int32), status=status,
               chi2=np.zeros((cap, 2), F), log=g.log, i1=i1)
    out.update(outputs_of(S_in, s["Tcw"][1]))

    def check():
        idx = g.active()
        a, b = g.chi2(idx)
        g.log.checks.append((np.stack([a, b], axis=1), idx.copy()))
        out["chi2"][i1[idx], 0], out["chi2"][i1[idx], 1] = a.astype(F), b.astype(F)
        bad = (a > th2) | (b > th2)
        matches[i1[idx[bad]]] = -1
        g.removed[idx[bad]] = True
        return int(np.sum(bad))

    try:
        est = S_in
        if not sim3_finite(est):
            raise Stop(ST_NOT_FINITE)
        if g.n:
            est, out["iters"][0] = g.optimize(est, 5)
        n_bad = check()
        out["n_bad_first"] = n_bad
        more = 10 if n_bad > 0 else 5
        if len(corr) - n_bad < 10:
            return out
        est, out["iters"][1] = g.optimize(est, more)
        out["n_inliers"] = (len(corr) - n_bad) - check()
        out.update(outputs_of(est, s["Tcw"][1]))
    except Stop as stop:
        out["status"] |= stop.bit
    return out


def numeric_jacobian_column_text(S, fix_scale, camera, X, obs, inverse):
    """base_binary_edge.hpp:176-200 for ONE edge, scalar by scalar from the text: the [2, 7] Jacobian of the Sim3 vertex"""
    fx, fy, cx, cy = (float(v) for v in camera[:4])

    def compute_error(est):
        M = sim3_inverse(est) if inverse else est
        p = sim3_map(M, list(X))
        return [obs[0] - ((p[0] / p[2]) * fx + cx), obs[1] - ((p[1] / p[2]) * fy + cy)]

    delta = 1e-9
    scalar = 1.0 / (2 * delta)
    add_vj = [0.0] * 7
    J = np.zeros((2, 7))
    for d in range(7):
        add_vj[d] = delta
        errorBak = compute_error(oplus(S, add_vj, fix_scale))
        add_vj[d] = -delta
        e = compute_error(oplus(S, add_vj, fix_scale))
        errorBak = [errorBak[0] - e[0], errorBak[1] - e[1]]
        add_vj[d] = 0.0
        J[0, d], J[1, d] = scalar * errorBak[0], scalar * errorBak[1]
    return J
