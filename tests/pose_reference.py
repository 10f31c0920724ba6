"""Optimizer::PoseOptimizationWithLine (src/Optimizer.cc:604-697, the branch that executes) restated line by line in plain Python loops over IEEE doubles
(Python floats).  It shares nothing with the package: its own terms, its own se(3) maps, numpy.linalg for the dense pieces.

Two switches sample the rounding the restatement itself is sensitive to:
  reverse   the sums of H, g, e and of the mean run over the features in reversed index order
  lstsq     the Gauss-Newton step comes from numpy.linalg.lstsq instead of numpy.linalg.solve
Beside the outputs it returns two kinds of margins:
  outlier_margin   min | |res - mean| - th | / th over every removeOutliers decision (inf without one)
  stop_ratios      per pass, every stopping-rule ratio that was evaluated: |d err| / min_error_change, step norms / min_error_change, err / min_error
and `branches`, the set of lineSegmentOverlap cases taken (0 vertical, 1 horizontal, 2 oblique).

The two cases the reference leaves undefined are defined as include/orbline.h defines them: a feature that enters as an outlier gets its previous-frame
position like any other; a pass that starts without an active feature (status 1) or meets a non-finite H, g or DT (status 2) stops the frame, whose pose
goes through unchanged."""
import math
import struct
import numpy as np

ST_NO_FEATURE, ST_NOT_FINITE, ST_OCTAVE = 1, 2, 4
DEFAULTS = dict(max_iters_ref=10, homog_th=1e-7, min_error=1e-7, min_error_change=1e-7, inlier_k=4.0, use_motion_model=1, has_points=1, has_lines=1)


def fabsf(x):
    """fabsf(double): the argument rounded to float first"""
    if x != x or math.isinf(x):
        return abs(x)
    try:
        return abs(struct.unpack("<f", struct.pack("<f", x))[0])
    except OverflowError:
        return math.inf


def inverse_se3(T):
    R, t = T[:3, :3], T[:3, 3]
    o = np.eye(4)
    o[:3, :3] = R.T
    for i in range(3):
        o[i, 3] = ((-R[0, i]) * t[0] + (-R[1, i]) * t[1]) + (-R[2, i]) * t[2]
    return o


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def mul(A, B):
    """a matrix product summed over k in ascending order"""
    n, m, p = A.shape[0], A.shape[1], B.shape[1]
    C = np.zeros((n, p))
    for i in range(n):
        for j in range(p):
            s = float(A[i, 0]) * float(B[0, j])
            for k in range(1, m):
                s = s + float(A[i, k]) * float(B[k, j])
            C[i, j] = s
    return C


def expmap_se3(x):
    t, w = np.array(x[:3], dtype=float), np.array(x[3:], dtype=float)
    theta = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    Om, I = skew(w), np.eye(3)
    if theta < 0.00001:
        R = (I + Om) + mul(Om, Om)
        t = mul(R, t.reshape(3, 1)).reshape(3)
    else:
        s = Om / theta
        ss = mul(s, s)
        sn, c1 = math.sin(theta), 1.0 - math.cos(theta)
        R = (I + s * sn) + ss * c1
        V = (I + (s * c1) / theta) + (ss * (theta - sn)) / theta
        t = mul(V, t.reshape(3, 1)).reshape(3)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def logmap_se3(T):
    """g2o::SE3Quat(R, t).log() with the halves swapped: through a normalised quaternion with w >= 0 and its rotation matrix"""
    m = T
    tr = (m[0, 0] + m[1, 1]) + m[2, 2]
    q = [0.0] * 4                                   # x, y, z, w
    if tr > 0.0:
        t = math.sqrt(tr + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    if q[3] < 0.0:
        q = [v * -1.0 for v in q]
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    x, y, z, w = (float(v) / n for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])
    d = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0)
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    I = np.eye(3)
    if d > 0.99999:
        om = 0.5 * dR
        Om = skew(om)
        Vi = (I - 0.5 * Om) + (1. / 12.) * mul(Om, Om)
    else:
        theta = math.acos(d)
        om = theta / (2.0 * math.sqrt(1.0 - d * d)) * dR
        Om = skew(om)
        Vi = (I - 0.5 * Om) + ((1.0 - theta / (2.0 * math.tan(theta / 2.0))) / (theta * theta)) * mul(Om, Om)
    ups = mul(Vi, np.array(T[:3, 3], dtype=float).reshape(3, 1)).reshape(3)
    return np.concatenate([ups, om])


def transform(T, P):
    return [((float(T[i, 0]) * P[0] + float(T[i, 1]) * P[1]) + float(T[i, 2]) * P[2]) + float(T[i, 3]) for i in range(3)]


def div(a, b):
    """IEEE division: x / 0 is an infinity or a NaN, not an exception"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def overlap_ladder(ls, le):
    lmin, lmax = min(ls, le), max(ls, le)
    if lmin < 0.0 and lmax > 1.0:
        return 1.0
    if lmax < 0.0 or lmin > 1.0:
        return 0.0
    if lmin < 0.0:
        return lmax
    if lmax > 1.0:
        return 1.0 - lmin
    return lmax - lmin


def line_segment_overlap(so, eo, sp, ep, branches=None):
    """Frame::lineSegmentOverlap, src/Frame.cc:1108-1209"""
    if abs(so[0] - eo[0]) < 1.0:
        if branches is not None:
            branches.add(0)
        l1 = eo[1] - so[1]
        return overlap_ladder(div(sp[1] - so[1], l1), div(ep[1] - so[1], l1))
    if abs(so[1] - eo[1]) < 1.0:
        if branches is not None:
            branches.add(1)
        l0 = eo[0] - so[0]
        return overlap_ladder(div(sp[0] - so[0], l0), div(ep[0] - so[0], l0))
    if branches is not None:
        branches.add(2)
    l0 = eo[0] - so[0]
    a, b, c = so[1] - eo[1], eo[0] - so[0], so[0] * eo[1] - eo[0] * so[1]
    lxy = 1.0 / (a * a + b * b)
    sx = (b * (b * sp[0] - a * sp[1]) - a * c) * lxy
    ex = (b * (b * ep[0] - a * ep[1]) - a * c) * lxy
    return overlap_ladder(div(sx - so[0], l0), div(ex - so[0], l0))


def median_of(v):
    return sorted(v)[len(v) // 2]


def stdv_mad(res):
    """vector_stdv_mad(vector<double>), src/Auxiliar.cc:456-472"""
    if not res:
        return 0.0
    med = median_of(res)
    return 1.4826 * median_of([fabsf(r - med) for r in res])


class Frame:
    """the members the optimiser reads, as plain lists"""

    def __init__(self, keys, keylines, lle, frame_mp, mp_world, frame_ml, ml_world, inv_level_sigma2, camera, outlier=None, outlier_l=None, mp_index_offset=0,
                 ml_index_offset=0):
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(v)) for v in camera)
        self.status = 0
        n_levels = len(inv_level_sigma2)
        self.pts, self.lines = [], []               # held features: dicts
        self.N, self.NL = len(keys), len(keylines)
        self.out = [0] * self.N
        self.outl = [0] * self.NL
        for i in range(self.N):
            m = int(frame_mp[i])
            if m < 0:
                continue
            m += int(mp_index_offset)
            if m < 0 or m >= len(mp_world):
                self.status |= 512
                continue
            oct_ = int(keys[i]["octave"])
            if oct_ < 0 or oct_ >= n_levels:
                self.status |= ST_OCTAVE
                continue
            self.pts.append(dict(i=i, Xw=[float(v) for v in np.asarray(mp_world[m], dtype=np.float32)], obs=(float(keys[i]["x"]), float(keys[i]["y"])),
                                 sq=math.sqrt(float(np.float32(inv_level_sigma2[oct_])))))
            if outlier is not None and outlier[i]:
                self.out[i] = 1
        for i in range(self.NL):
            m = int(frame_ml[i])
            if m < 0:
                continue
            m += int(ml_index_offset)
            if m < 0 or m >= len(ml_world):
                self.status |= 1024
                continue
            kl = keylines[i]
            oct_ = int(kl["octave"])
            if oct_ < 0 or oct_ >= n_levels:
                self.status |= ST_OCTAVE
                continue
            W = [float(v) for v in np.asarray(ml_world[m], dtype=np.float32)]
            self.lines.append(dict(i=i, sW=W[:3], eW=W[3:], le=[float(v) for v in lle[i]],
                                   so=(float(kl["startPointX"]), float(kl["startPointY"])), eo=(float(kl["endPointX"]), float(kl["endPointY"])),
                                   sq=math.sqrt(float(np.float32(inv_level_sigma2[oct_])))))
            if outlier_l is not None and outlier_l[i]:
                self.outl[i] = 1


class Stop(Exception):
    def __init__(self, bit):
        self.bit = bit


class Solver:
    def __init__(self, frame, params, reverse, lstsq):
        self.f, self.p, self.reverse, self.lstsq = frame, dict(DEFAULTS, **(params or {})), reverse, lstsq
        self.outlier_margin = math.inf
        self.stop_ratios = [[], [], [], []]
        self.branches = set()
        self.iters = [0, 0, 0, 0]

    # ---- per-feature terms ----
    def project(self, P):
        return self.f.cx + div(self.f.fx * P[0], P[2]), self.f.cy + div(self.f.fy * P[1], P[2])

    def jac_row(self, g, a, b):
        gx, gy, gz = g
        gz2 = gz * gz
        fgz2 = self.f.fx / max(self.p["homog_th"], gz2)
        return [+fgz2 * a * gz, +fgz2 * b * gz, -fgz2 * (gx * a + gy * b), -fgz2 * (gx * gy * a + gy * gy * b + gz * gz * b),
                +fgz2 * (gx * gx * a + gz * gz * a + gx * gy * b), +fgz2 * (gx * gz * b - gy * gz * a)]

    def point_term(self, DT, pt, jac):
        P = transform(DT, pt["P"])
        u, v = self.project(P)
        dx, dy = u - pt["obs"][0], v - pt["obs"][1]
        n = math.sqrt(dx * dx + dy * dy)
        if not jac:
            return n, None
        d = max(self.p["homog_th"], n)
        return n, [div(x, d) for x in self.jac_row(P, dx, dy)]

    def line_term(self, DT, ln, jac):
        sP, eP = transform(DT, ln["sP"]), transform(DT, ln["eP"])
        sp, ep = self.project(sP), self.project(eP)
        le = ln["le"]
        ds = le[0] * sp[0] + le[1] * sp[1] + le[2]
        de = le[0] * ep[0] + le[1] * ep[1] + le[2]
        n = math.sqrt(ds * ds + de * de)
        if not jac:
            return n, None, None
        Js, Je = self.jac_row(sP, le[0], le[1]), self.jac_row(eP, le[0], le[1])
        d = max(self.p["homog_th"], n)
        J = [div(Js[i] * ds + Je[i] * de, d) for i in range(6)]
        return n, J, line_segment_overlap(ln["so"], ln["eo"], sp, ep, self.branches)

    # ---- optimizeFunctions / optimizeFunctionsRobust ----
    def evaluate(self, DT, robust, first):
        f = self.f
        act_p = [pt for pt in f.pts if not f.out[pt["i"]]]
        act_l = [ln for ln in f.lines if not f.outl[ln["i"]]]
        s_p = s_l = 1.0
        if robust:
            th_min, th_max = 0.0001, math.sqrt(7.815)
            s_p = min(max(stdv_mad([self.point_term(DT, pt, False)[0] for pt in act_p]), th_min), th_max)
            s_l = min(max(stdv_mad([self.line_term(DT, ln, False)[0] for ln in act_l]), th_min), th_max)
        n = len(act_p) + len(act_l)
        if first and n == 0:
            raise Stop(ST_NO_FEATURE)

        def sums(terms):
            H, g, e = [[0.0] * 6 for _ in range(6)], [0.0] * 6, 0.0
            for J, r, w in (reversed(terms) if self.reverse else terms):
                for i in range(6):
                    for j in range(i, 6):
                        H[i][j] = H[i][j] + J[i] * J[j] * w
                    g[i] = g[i] + J[i] * r * w
                e = e + r * r * w
            return H, g, e

        tp, tl = [], []
        for pt in act_p:
            nrm, J = self.point_term(DT, pt, True)
            r = nrm if robust else nrm * pt["sq"]
            w = div(1.0, 1.0 + (r / s_p) * (r / s_p)) if robust else div(1.0, 1.0 + r * r)
            tp.append((J, r, w))
        for ln in act_l:
            nrm, J, ov = self.line_term(DT, ln, True)
            r = nrm if robust else nrm * ln["sq"]
            w = div(1.0, 1.0 + (r / s_l) * (r / s_l)) if robust else div(1.0, 1.0 + r * r)
            tl.append((J, r, w * ov))
        (Hp, gp, ep), (Hl, gl, el) = sums(tp), sums(tl)
        H = np.zeros((6, 6))
        for i in range(6):
            for j in range(i, 6):
                H[i, j] = H[j, i] = Hp[i][j] + Hl[i][j]
        g = np.array([gp[i] + gl[i] for i in range(6)])
        e = ep + el
        if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g)) and math.isfinite(e)):
            raise Stop(ST_NOT_FINITE)
        return H, g, e / n

    def solve(self, H, g):
        with np.errstate(all="ignore"):
            if self.lstsq:
                return np.linalg.lstsq(H, g, rcond=None)[0]
            try:
                return np.linalg.solve(H, g)
            except np.linalg.LinAlgError:
                return np.full(6, math.nan)

    def step(self, DT, inc):
        if not np.all(np.isfinite(inc)):
            raise Stop(ST_NOT_FINITE)
        DT = mul(DT, inverse_se3(expmap_se3(inc)))
        if not np.all(np.isfinite(DT)):
            raise Stop(ST_NOT_FINITE)
        return DT

    @staticmethod
    def inverse(H):
        with np.errstate(all="ignore"):
            try:
                return np.linalg.inv(H)
            except np.linalg.LinAlgError:
                return np.full((6, 6), math.nan)

    def gauss_newton(self, p, DT, cov):
        """gaussNewtonOptimization, :779-816; returns DT, cov, err"""
        P, ratios = self.p, self.stop_ratios[p]
        err_prev, H, err = 999999999.9, None, 0.0
        for iters in range(P["max_iters_ref"]):
            H, g, err = self.evaluate(DT, False, iters == 0)
            self.iters[p] += 1
            if err > err_prev:
                if iters > 0:
                    break
                return DT, cov, -1.0
            ratios.append(div(err, P["min_error"]))
            ratios.append(div(abs(err - err_prev), P["min_error_change"]))
            if err < P["min_error"] or abs(err - err_prev) < P["min_error_change"]:
                break
            inc = self.solve(H, g)
            DT = self.step(DT, inc)
            nt = math.sqrt((inc[0] * inc[0] + inc[1] * inc[1]) + inc[2] * inc[2])
            nw = math.sqrt((inc[3] * inc[3] + inc[4] * inc[4]) + inc[5] * inc[5])
            ratios.append(div(max(nt, nw), P["min_error_change"]))
            if nt < P["min_error_change"] and nw < P["min_error_change"]:
                break
            err_prev = err
        return DT, self.inverse(H), err

    def gauss_newton_robust(self, p, DT, cov):
        """gaussNewtonOptimizationRobust, :818-865"""
        P, ratios = self.p, self.stop_ratios[p]
        DT0, err_prev, good, H, err = DT.copy(), 999999999.9, True, None, 0.0
        for iters in range(P["max_iters_ref"]):
            H, g, err = self.evaluate(DT, True, iters == 0)
            self.iters[p] += 1
            ratios.append(div(abs(err - err_prev), P["min_error_change"]))
            ratios.append(div(err, P["min_error"]))
            if abs(err - err_prev) < P["min_error_change"] or err < P["min_error"]:
                break
            inc = self.solve(H, g)
            with np.errstate(all="ignore"):
                sign, lad = np.linalg.slogdet(H)
            if lad < 0.0:
                good = False
                break
            DT = self.step(DT, inc)
            n = math.sqrt(sum(float(v) * float(v) for v in inc))
            ratios.append(div(n, P["min_error_change"]))
            if n < P["min_error_change"]:
                break
            err_prev = err
        if good:
            return DT, self.inverse(H), err
        return DT0, np.eye(6), -1.0

    # ---- removeOutliers, :468-602, with vector_mean_stdv_mad, src/Auxiliar.cc:399-442 ----
    def decide(self, res, idx, flags):
        if not res:
            return
        n = len(res)
        med = median_of(res)
        stdv = 1.4826 * median_of([fabsf(r - med) for r in res])
        order = list(reversed(res)) if self.reverse else res
        mean, k = 0.0, 0
        for r in order:
            if r < 2.0 * stdv:
                mean += r
                k += 1
        if k >= int(0.2 * n):
            mean = div(mean, float(k))
        else:
            mean = 0.0
            for r in order:
                mean += r
            mean = mean / float(n)
        th = self.p["inlier_k"] * stdv
        for r, i in zip(res, idx):
            dev = abs(r - mean)
            flags[i] = 1 if dev > th else 0
            if th > 0.0 and math.isfinite(dev):
                self.outlier_margin = min(self.outlier_margin, abs(dev - th) / th)
            elif th == 0.0 and dev == 0.0:
                pass                                                 # (a lone residual: |res - mean| = 0 against th = 0, nowhere near a flip)
            elif th == 0.0 and math.isfinite(dev):
                self.outlier_margin = min(self.outlier_margin, math.inf if dev > 0.0 else 0.0)

    def remove_outliers(self, DT):
        f = self.f
        if self.p["has_points"]:
            self.decide([self.point_term(DT, pt, False)[0] * pt["sq"] for pt in f.pts], [pt["i"] for pt in f.pts], f.out)
        if self.p["has_lines"]:
            self.decide([self.line_term(DT, ln, False)[0] * ln["sq"] for ln in f.lines], [ln["i"] for ln in f.lines], f.outl)


def pose_optimization_with_line(keys, keylines, lle, Tcw, camera, frame_mp, mp_world, frame_ml, ml_world, inv_level_sigma2, Tcw_prev=None, DT_cov_in=None,
                                mp_index_offset=0, ml_index_offset=0, outlier=None, outlier_l=None, params=None, reverse=False, lstsq=False):
    """Returns a dict: Tcw_out [16] float32, DT [16], DT_cov [36], DT_cov_eig [6], err_norm, good, outlier_out [N], outlier_l_out [N_l], n_inliers [2],
    iters [4], status, and outlier_margin, stop_ratios, branches."""
    f = Frame(keys, keylines, lle, frame_mp, mp_world, frame_ml, ml_world, inv_level_sigma2, camera, outlier, outlier_l, mp_index_offset, ml_index_offset)
    s = Solver(f, params, reverse, lstsq)
    T = np.array(np.asarray(Tcw, dtype=np.float32).reshape(4, 4), dtype=np.float64)
    Tp = T.copy() if Tcw_prev is None else np.array(np.asarray(Tcw_prev, dtype=np.float32).reshape(4, 4), dtype=np.float64)
    T[3], Tp[3] = [0, 0, 0, 1], [0, 0, 0, 1]
    Tpi = inverse_se3(Tp)
    DT0 = mul(T, Tpi) if s.p["use_motion_model"] else np.eye(4)
    cov = np.zeros((6, 6)) if DT_cov_in is None else np.array(DT_cov_in, dtype=np.float64).reshape(6, 6)
    for pt in f.pts:
        pt["P"] = transform(Tp, pt["Xw"])
    for ln in f.lines:
        ln["sP"], ln["eP"] = transform(Tp, ln["sW"]), transform(Tp, ln["eW"])
    status, err, DT = f.status, -1.0, DT0
    try:
        if not np.all(np.isfinite(DT0)):
            raise Stop(ST_NOT_FINITE)
        for p in range(4):
            DT, cov, err = (s.gauss_newton_robust if p == 2 else s.gauss_newton)(p, DT0.copy(), cov)
            s.remove_outliers(DT)
        with np.errstate(all="ignore"):
            try:
                eig = np.linalg.eigvalsh(cov)
            except np.linalg.LinAlgError:
                eig = np.full(6, math.nan)
        good = int(not (eig[0] < 0.0 or eig[5] > 1.0 or err < 0.0 or err > 1.0 or not np.all(np.isfinite(DT))))
        fDT = expmap_se3(logmap_se3(inverse_se3(DT)))
        Twc = expmap_se3(logmap_se3(mul(Tpi, fDT)))
        Tf = Twc.astype(np.float32)
        Tout = np.eye(4, dtype=np.float32)
        Tout[:3, :3] = Tf[:3, :3].T
        for i in range(3):
            acc = (float(Tf[0, i]) * float(Tf[0, 3]) + float(Tf[1, i]) * float(Tf[1, 3])) + float(Tf[2, i]) * float(Tf[2, 3])
            Tout[i, 3] = np.float32(-acc)
    except Stop as stop:
        status |= stop.bit
        Tout, fDT, cov, eig, err, good = np.asarray(Tcw, dtype=np.float32).reshape(4, 4).copy(), np.eye(4), np.zeros((6, 6)), np.zeros(6), -1.0, 0
    n_in = [sum(1 for pt in f.pts if not f.out[pt["i"]]), sum(1 for ln in f.lines if not f.outl[ln["i"]])]
    return dict(Tcw_out=Tout.reshape(16), DT=np.asarray(fDT).reshape(16), DT_cov=np.asarray(cov).reshape(36), DT_cov_eig=np.asarray(eig), err_norm=float(err), good=good,
                outlier_out=np.array(f.out, np.uint8), outlier_l_out=np.array(f.outl, np.uint8), n_inliers=np.array(n_in, np.int32), iters=np.array(s.iters, np.int32),
                status=status, outlier_margin=s.outlier_margin, stop_ratios=s.stop_ratios, branches=s.branches)


def discard_outliers(frame_mp, frame_ml, outlier, outlier_l, mode, only_tracking=False, stereo=True, mp_obs=None, ml_obs=None):
    """the loops of src/Tracking.cc:1034-1074 (mode 0) and :1547-1590 (mode 1) on lists; returns the changed copies and the two counts"""
    def row(held, out, obs):
        held, out, n = list(held), list(out), 0
        for i in range(len(held)):
            if held[i] < 0:
                continue
            seen = obs is None or bool(obs[held[i]])
            if mode == 0:
                if out[i]:
                    held[i], out[i] = -1, 0
                elif seen:
                    n += 1
            else:
                if not out[i]:
                    if not only_tracking:
                        if seen:
                            n += 1
                    else:
                        n += 1
                elif stereo:
                    held[i] = -1
        return held, out, n
    p, po, npts = row(frame_mp, outlier, mp_obs)
    l, lo, nls = row(frame_ml, outlier_l, ml_obs)
    return dict(frame_mp=p, frame_ml=l, outlier=po, outlier_l=lo, n_matches=[npts, nls])
