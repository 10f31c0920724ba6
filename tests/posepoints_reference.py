"""A numpy restatement of int Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:239-451) with everything it executes through g2o
(Thirdparty/g2o/g2o: types/types_six_dof_expmap.{h,cpp}, types/se3quat.h, types/se3_ops.hpp, core/base_edge.h, core/base_unary_edge.hpp:43-72,
core/robust_kernel_impl.cpp, core/optimization_algorithm_levenberg.cpp:61-189, core/sparse_optimizer.cpp:354-419, core/block_solver.hpp,
solvers/linear_solver_dense.h), written from those files.  It reads nothing from the library.  Switches (a namespace ldlt / acc / rev):
  ldlt  "eigen": Eigen::LDLT as Eigen 3.3 runs it on a 6 x 6 (pivot on the largest remaining |diagonal|, in place on the lower triangle, unblocked) -- the
        base; "numpy": numpy.linalg.solve, positive when every eigenvalue of the symmetric matrix is >= 0
  acc   False: the sums over the edges sequential in double (base); True: every term perturbed by a float32 rounding of its relative part
  rev   the sums over the edges taken in reverse
  flip  every accept / reject of a Levenberg trial whose two chi2 differ by less than FLIP_MARGIN of their size goes the other way.  A pass that
        converges ends with such trials (the step no longer changes chi2 beyond rounding), so a summation of another shape may take them either way; with
        this run among the switched ones the yardstick holds both outcomes
The run keeps a log for the yardstick conditions of tests/test_posepoints_cpu.py: every Levenberg decision with the two numbers it compared, and every
classification with its chi2 in double, its thresholds, the flags before and after, and the flags a fresh computeError of every edge would give.
What the reference leaves undefined is defined as include/orbline.h defines it: a depth of exactly 0 (status 1) or a non-finite H, b, step or estimate
(status 2) stops the row with the input pose, the flags of the last completed pass and n_good = 0; an empty active set leaves the estimate alone."""
import math
import types
import numpy as np

F = np.float32
BASE = types.SimpleNamespace(ldlt="eigen", acc=False, rev=False, flip=False)
SWITCHED = (types.SimpleNamespace(ldlt="numpy", acc=False, rev=False, flip=False), types.SimpleNamespace(ldlt="eigen", acc=True, rev=False, flip=False),
            types.SimpleNamespace(ldlt="eigen", acc=False, rev=True, flip=False), types.SimpleNamespace(ldlt="eigen", acc=False, rev=False, flip=True))
FLIP_MARGIN = 1e-9                                                   # a thousand times what two summation orders differ by (measured: below 1e-12)
DBL_MAX, DBL_MIN = 1.7976931348623157e308, 2.2250738585072014e-308
ST_DEPTH, ST_NOT_FINITE, ST_OCTAVE = 1, 2, 4
DELTA = (float(F(math.sqrt(5.991))), float(F(math.sqrt(7.815))))     # deltaMono, deltaStereo: floats (:273-274)
CHI2_TH = (F(5.991), F(7.815))                                       # chi2Mono, chi2Stereo (:369-370)


class Stop(Exception):
    def __init__(self, bit):
        self.bit = bit


def csum(terms, sw):
    """a sum over the edges, terms [n, ...], from +0 in the switch's order"""
    t = np.asarray(terms, np.float64)
    if t.shape[0] == 0:
        return np.zeros(t.shape[1:])
    if sw.acc:
        t = t * (1.0 + (np.arange(t.shape[0]) % 3 - 1).reshape((-1,) + (1,) * (t.ndim - 1)) * 2.0 ** -24)
    if sw.rev:
        t = t[::-1]
    return np.cumsum(t, axis=0)[-1]


# ---- Quaterniond and SE3Quat (q = x, y, z, w)
def quat_of(R):
    """Eigen's Quaterniond(Matrix3d)"""
    q = [0.0] * 4
    t = (R[0][0] + R[1][1]) + R[2][2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k][j] - R[j][k]) * t
        q[j] = (R[j][i] + R[i][j]) * t
        q[k] = (R[k][i] + R[i][k]) * t
    return q


def normalize_rotation(q):
    """SE3Quat::normalizeRotation (se3quat.h:280-285)"""
    if q[3] < 0:
        q = [-v for v in q]
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [v / n for v in q]


def rotation_of(q):
    """Quaterniond::toRotationMatrix"""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def rotate(q, v):
    """Quaterniond * Vector3d: v + w * uv + vec x uv with uv = 2 (vec x v); v may hold arrays"""
    uv = cross(q[:3], v)
    uv = [u + u for u in uv]
    c = cross(q[:3], uv)
    return [(v[i] + q[3] * uv[i]) + c[i] for i in range(3)]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by + ay * bw) + az * bx) - ax * bz, ((aw * bz + az * bw) + ax * by) - ay * bx,
            ((aw * bw - ax * bx) - ay * by) - az * bz]


def skew(v):
    return [[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]]


def mat3(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:223-257): update = (omega, upsilon)"""
    om, up = list(u[:3]), list(u[3:])
    theta = math.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    Om = skew(om)
    OO = mat3(Om, Om)
    I = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    if theta < 0.00001:
        R = [[(I[i][j] + Om[i][j]) + OO[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        a, b, c = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta), (theta - math.sin(theta)) / math.pow(theta, 3)
        R = [[(I[i][j] + a * Om[i][j]) + b * OO[i][j] for j in range(3)] for i in range(3)]
        V = [[(I[i][j] + b * Om[i][j]) + c * OO[i][j] for j in range(3)] for i in range(3)]
    t = [(V[i][0] * up[0] + V[i][1] * up[1]) + V[i][2] * up[2] for i in range(3)]
    return normalize_rotation(quat_of(R)), t


def se3_mul(a, b):
    """SE3Quat::operator* (se3quat.h:104-110)"""
    r = rotate(a[0], b[1])
    return normalize_rotation(quat_mul(a[0], b[0])), [a[1][i] + r[i] for i in range(3)]


def to_se3quat(Tcw):
    """Converter::toSE3Quat (src/Converter.cc:37-47)"""
    T = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
    return normalize_rotation(quat_of(T[:3, :3].tolist())), [float(T[0, 3]), float(T[1, 3]), float(T[2, 3])]


def to_cvmat(est):
    """Converter::toCvMat(SE3Quat) (src/Converter.cc:51-55)"""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.array(rotation_of(est[0])), est[1]
    return T.astype(np.float32).reshape(16)


# ---- Eigen::LDLT<MatrixXd>::compute / isPositive / solve
def ldlt_eigen(A, b):
    n = len(b)
    M = [[A[i][j] if j <= i else 0.0 for j in range(n)] for i in range(n)]
    tr, sign, all_zero = list(range(n)), 0, False
    for k in range(n):
        p = max(range(k, n), key=lambda i: (abs(M[i][i]), -i))      # the first largest
        tr[k] = p
        if p != k:
            for j in range(k):
                M[k][j], M[p][j] = M[p][j], M[k][j]
            for i in range(p + 1, n):
                M[i][k], M[i][p] = M[i][p], M[i][k]
            M[k][k], M[p][p] = M[p][p], M[k][k]
            for i in range(k + 1, p):
                M[i][k], M[p][i] = M[p][i], M[i][k]
        if k > 0:
            tmp = [M[j][j] * M[k][j] for j in range(k)]
            s = M[k][0] * tmp[0]
            for j in range(1, k):
                s = s + M[k][j] * tmp[j]
            M[k][k] = M[k][k] - s
            for i in range(k + 1, n):
                r = M[i][0] * tmp[0]
                for j in range(1, k):
                    r = r + M[i][j] * tmp[j]
                M[i][k] = M[i][k] - r
        akk = M[k][k]
        valid = abs(akk) > 0.0
        if k == 0 and not valid:
            tr, all_zero = list(range(n)), True
            break
        if valid:
            for i in range(k + 1, n):
                M[i][k] = M[i][k] / akk
        if sign == 1:
            sign = 2 if akk < 0 else 1
        elif sign == -1:
            sign = 2 if akk > 0 else -1
        elif sign == 0:
            sign = 1 if akk > 0 else (-1 if akk < 0 else 0)
    if sign not in (0, 1):
        return False, None
    y = list(b)
    for k in range(n):
        if tr[k] != k:
            y[k], y[tr[k]] = y[tr[k]], y[k]
    if not all_zero:
        for j in range(n):
            for i in range(j + 1, n):
                y[i] = y[i] - M[i][j] * y[j]
    y = [y[i] / M[i][i] if abs(M[i][i]) > DBL_MIN else 0.0 for i in range(n)]
    if not all_zero:
        for i in range(n - 2, -1, -1):
            s = M[i + 1][i] * y[i + 1]
            for j in range(i + 2, n):
                s = s + M[j][i] * y[j]
            y[i] = y[i] - s
    for k in range(n - 1, -1, -1):
        if tr[k] != k:
            y[k], y[tr[k]] = y[tr[k]], y[k]
    return True, y


def ldlt_numpy(A, b):
    A = np.array(A)
    L = np.tril(A)
    S = L + L.T - np.diag(np.diag(A))
    if np.min(np.linalg.eigvalsh(S)) < 0:
        return False, None
    try:
        return True, np.linalg.solve(S, np.array(b)).tolist()
    except np.linalg.LinAlgError:
        return True, [0.0] * len(b)


class Graph:
    """the optimizer of one call: the held features as edges in ascending index"""

    def __init__(self, pts, uright, octaves, Xw, camera, inv_level_sigma2, sw):
        self.sw, self.n = sw, len(pts)
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(F(v)) for v in camera)
        self.stereo = np.asarray(uright, np.float32) >= 0
        self.obs = np.column_stack([np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64), np.asarray(uright, np.float32).astype(np.float64)])
        self.X = np.asarray(Xw, np.float32).reshape(-1, 3).astype(np.float64)
        self.w = np.asarray(inv_level_sigma2, np.float32)[np.asarray(octaves, np.int64)].astype(np.float64) if self.n else np.zeros(0)
        self.err = np.zeros((self.n, 3))
        self.outlier = np.zeros(self.n, bool)
        self.delta = np.where(self.stereo, DELTA[1], DELTA[0])
        self.log = types.SimpleNamespace(decisions=[], classified=[])

    def map(self, est, idx):
        X = self.X[idx]
        r = rotate(est[0], [X[:, 0], X[:, 1], X[:, 2]])
        return [r[i] + est[1][i] for i in range(3)]

    def compute_error(self, est, idx):
        """computeError of both kinds (types_six_dof_expmap.h:153-157, :184-188; cam_project .cpp:290-306)"""
        if len(idx) == 0:
            return
        x, y, z = self.map(est, idx)
        if np.any(z == 0.0):
            raise Stop(ST_DEPTH)
        st, o = self.stereo[idx], self.obs[idx]
        with np.errstate(all="ignore"):
            invz = (1.0 / z).astype(np.float32).astype(np.float64)          # const float invz = 1.0f / trans_xyz[2]
            us, vs = (x * invz) * self.fx + self.cx, (y * invz) * self.fy + self.cy
            um, vm = (x / z) * self.fx + self.cx, (y / z) * self.fy + self.cy
        e = np.zeros((len(idx), 3))
        e[:, 0] = np.where(st, o[:, 0] - us, o[:, 0] - um)
        e[:, 1] = np.where(st, o[:, 1] - vs, o[:, 1] - vm)
        e[:, 2] = np.where(st, o[:, 2] - (us - self.bf * invz), 0.0)
        self.err[idx] = e

    def chi2(self, idx):
        e, w = self.err[idx], self.w[idx]
        s = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
        return np.where(self.stereo[idx], s + e[:, 2] * (w * e[:, 2]), s)

    def rho(self, idx, robust):
        """robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1]"""
        e = self.chi2(idx)
        if not robust:
            return e, np.ones_like(e)
        d = self.delta[idx]
        dsqr = d * d
        with np.errstate(all="ignore"):
            sq = np.sqrt(e)
            r0, r1 = (2 * sq) * d - dsqr, d / sq
        inl = e <= dsqr
        return np.where(inl, e, r0), np.where(inl, 1.0, r1)

    def active(self):
        return np.nonzero(~self.outlier)[0]

    def active_robust_chi2(self, robust):
        idx = self.active()
        return float(csum(self.rho(idx, robust)[0], self.sw))

    def build_system(self, est, robust):
        """linearizeOplus (.cpp:266-288, :335-364) and constructQuadraticForm for every active edge: H (lower triangle) and b"""
        idx = self.active()
        x, y, z = self.map(est, idx)
        if np.any(z == 0.0):
            raise Stop(ST_DEPTH)
        fx, fy, bf = self.fx, self.fy, self.bf
        invz = 1.0 / z
        invz_2 = invz * invz
        zero = np.zeros_like(x)
        J0 = [x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx]
        J1 = [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy]
        J2 = [J0[0] - bf * y * invz_2, J0[1] + bf * x * invz_2, J0[2], J0[3], zero, J0[5] - bf * invz_2]
        st, e, w = self.stereo[idx], self.err[idx], self.w[idx]
        rho1 = self.rho(idx, robust)[1]
        ww = rho1 * w if robust else w
        H = [[0.0] * 6 for _ in range(6)]
        for i in range(6):
            for j in range(i + 1):
                t = (J0[i] * ww) * J0[j] + (J1[i] * ww) * J1[j]
                t = np.where(st, t + (J2[i] * ww) * J2[j], t)
                H[i][j] = float(csum(t, self.sw))
                H[j][i] = H[i][j]
        b = []
        for i in range(6):
            if robust:
                t = ((rho1 * J0[i]) * w) * e[:, 0] + ((rho1 * J1[i]) * w) * e[:, 1]
                t = np.where(st, t + ((rho1 * J2[i]) * w) * e[:, 2], t)
            else:
                t = (J0[i] * w) * e[:, 0] + (J1[i] * w) * e[:, 1]
                t = np.where(st, t + (J2[i] * w) * e[:, 2], t)
            b.append(-float(csum(t, self.sw)))
        if not all(math.isfinite(v) for r in H for v in r) or not all(math.isfinite(v) for v in b):
            raise Stop(ST_NOT_FINITE)
        return H, b

    def optimize(self, est, iterations, robust):
        """SparseOptimizer::optimize over OptimizationAlgorithmLevenberg::solve; returns the estimate and the iterations run"""
        log = self.log.decisions
        lam, ni, n_bad, x, done = -1.0, 2.0, 0, [0.0] * 6, 0
        for it in range(iterations):
            self.compute_error(est, self.active())
            cur = self.active_robust_chi2(robust)
            ini = cur
            H, b = self.build_system(est, robust)
            if it == 0:
                lam, ni, n_bad = 1e-5 * max([0.0] + [abs(H[j][j]) for j in range(6)]), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                backup = est
                Hl = [[H[i][j] + (lam if i == j else 0.0) for j in range(6)] for i in range(6)]
                ok2, sol = (ldlt_eigen if self.sw.ldlt == "eigen" else ldlt_numpy)(Hl, b)
                if ok2:
                    x = sol
                if not all(math.isfinite(v) for v in x):
                    raise Stop(ST_NOT_FINITE)
                est = se3_mul(se3_exp(x), est)
                if not all(math.isfinite(v) for v in est[0] + est[1]):
                    raise Stop(ST_NOT_FINITE)
                self.compute_error(est, self.active())
                tmp = self.active_robust_chi2(robust)
                if not ok2:
                    tmp = DBL_MAX
                rho = cur - tmp
                scale = 0.0
                for j in range(6):
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


def pose_optimization(pts, uright, octaves, Tcw, camera, frame_mp, mp_world, inv_level_sigma2, mp_index_offset=0, sw=BASE):
    """One call.  pts [N, 2] (kpUn.pt), uright [N], octaves [N], Tcw 4 x 4 float32, camera = (fx, fy, cx, cy, mbf), frame_mp [N] indices into mp_world
    [n_mp, 3] (negative: none).  Returns a dict: Tcw_out [16] float32, outlier [N], n_good, n_initial, chi2 [N] float32, passes, iters [4], status,
    and log (decisions, classified)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    N = pts.shape[0]
    mpw = np.asarray(mp_world, np.float32).reshape(-1, 3)
    sig = np.asarray(inv_level_sigma2, np.float32).reshape(-1)
    octaves, fmp = np.asarray(octaves, np.int64).reshape(-1), np.asarray(frame_mp, np.int64).reshape(-1)
    status, held = 0, []
    for i in range(N):
        if fmp[i] < 0:
            continue
        m = fmp[i] + mp_index_offset
        if m < 0 or m >= mpw.shape[0]:
            status |= 512
        elif octaves[i] < 0 or octaves[i] >= sig.shape[0]:
            status |= ST_OCTAVE
        else:
            held.append(i)
    held = np.array(held, np.int64)
    g = Graph(pts[held], np.asarray(uright, np.float32).reshape(-1)[held], octaves[held], mpw[fmp[held] + mp_index_offset] if len(held) else np.zeros((0, 3)),
              camera, sig, sw)
    out = dict(Tcw_out=np.asarray(Tcw, np.float32).reshape(16).copy(), outlier=np.zeros(N, np.uint8), n_good=0, n_initial=len(held), chi2=np.zeros(N, np.float32),
               passes=0, iters=np.zeros(4, np.int32), status=status, log=g.log, held=held)
    if len(held) < 3:
        return out
    robust, n_bad, est = True, 0, None
    try:
        for it in range(4):
            est = to_se3quat(Tcw)
            if not all(math.isfinite(v) for v in est[0] + est[1]):
                raise Stop(ST_NOT_FINITE)
            if len(g.active()):
                est, out["iters"][it] = g.optimize(est, 10, robust)
            stale = g.err.copy()
            g.compute_error(est, np.arange(g.n))
            fresh = g.chi2(np.arange(g.n)).astype(np.float32)           # (for the log only: what a classification without the quirk would read)
            g.err[~g.outlier] = stale[~g.outlier]                       # :388-391: only a flagged edge is recomputed
            chi = g.chi2(np.arange(g.n))
            chif = chi.astype(np.float32)
            th = np.where(g.stereo, CHI2_TH[1], CHI2_TH[0]).astype(np.float32)
            g.log.classified.append((chi.copy(), th.astype(np.float64), g.outlier.copy(), chif > th, fresh > th))
            g.outlier = chif > th
            out["chi2"][held] = chif
            n_bad = int(np.sum(g.outlier))
            out["passes"] = it + 1
            if it == 2:
                robust = False
            if g.n < 10:
                break
    except Stop as s:
        out["status"] |= s.bit
        out["outlier"][held] = g.outlier
        return out
    out["Tcw_out"], out["n_good"] = to_cvmat(est), len(held) - n_bad
    out["outlier"][held] = g.outlier
    return out
