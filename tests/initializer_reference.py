"""A restatement of Initializer (src/Initializer.cc) in numpy, line by line, float32 and float64 exactly where the reference has them, under the
project's conventions (C.4 no contraction, C.12 cv::gemm, C.17 Mat / scalar, C.18 cv::invert / cv::determinant, C.20 the sample, C.30 to C.35).
Parity unpinned, like everything behind OpenCV.  Sums whose order decides bits (Normalize, the scores, the Jacobi's dot products) are numpy.cumsum, which
adds sequentially; what is independent per correspondence is vectorised, one rounding per operation as numpy does it.

Switches, to bound what an unverified memory of OpenCV costs:
  svd   "jacobi": C.30's one-sided Jacobi with C.31's fill for the fundamental matrix's null vector; "lapack": scipy.linalg.svd in single precision
        (sgesdd, what an OpenCV built with LAPACK calls), the null vector from there.  The 4 x 4 of Triangulate is numpy.linalg.svd in double under
        "jacobi" and sgesdd under "lapack", as tests/newpoints_reference.py has it.
  fill  "opencv": plus where next() & 256; "alt": minus there (the other sign pattern).
The sign and scale of F's null vector cancel in CheckFundamental and DecomposeE up to rounding, so the switches move results by rounding only -- except
the ORDER of the four hypotheses of ReconstructF, which follows the signs LAPACK happens to return."""
import math
import numpy as np

F = np.float32
D = np.float64
FLT_MIN = 1.1754943508222875e-38
EPS = F(1.1920928955078125e-7) * F(2)
FILL_ATTEMPTS = 4
PI = 3.1415926535897932384626433832795


def seqdot(x, y):
    """the double sum of double products, in order"""
    return float(np.cumsum(x.astype(D) * y.astype(D))[-1])


def sample8(N, r):
    """vAvailableIndices as written (:84-96): the literal swap-with-back, draws by C.20"""
    avail = list(range(N))
    out = []
    for j in range(8):
        randi = int((float(int(r[j]) & 0x7fffffff) / 2147483648.0) * len(avail))
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


class Rng:
    def __init__(self):
        self.s = 0x12345678

    def next(self):
        self.s = ((self.s & 0xffffffff) * 4164903690 + (self.s >> 32)) & 0xffffffffffffffff
        return self.s & 0xffffffff


def jacobi_svd(At, n, want_v=True, want_u=True, fill="opencv"):
    """C.30 / C.31.  At [n1, m] float32 whose first n rows are the operand's.  Returns (At, w float32 [n], V [n, n] or None, flags)."""
    At = np.array(At, F)
    n1, m = At.shape
    W = [seqdot(At[i], At[i]) for i in range(n)]
    V = np.eye(n, dtype=F) if want_v else None
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                a, b = W[i], W[j]
                p = seqdot(At[i], At[j])
                if abs(p) <= float(EPS) * math.sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = math.sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = F(math.sqrt(delta / gamma))
                    c = F(p / (gamma * float(s) * 2))
                else:
                    c = F(math.sqrt((gamma + beta) / (gamma * 2)))
                    s = F(p / (gamma * float(c) * 2))
                x, y = At[i].copy(), At[j].copy()
                At[i] = c * x + s * y
                At[j] = -s * x + c * y
                W[i], W[j] = seqdot(At[i], At[i]), seqdot(At[j], At[j])
                changed = True
                if want_v:
                    x, y = V[i].copy(), V[j].copy()
                    V[i] = c * x + s * y
                    V[j] = -s * x + c * y
        if not changed:
            break
    W = [math.sqrt(seqdot(At[i], At[i])) for i in range(n)]
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[[i, j]] = At[[j, i]]
            if want_v:
                V[[i, j]] = V[[j, i]]
    w = np.array([F(v) for v in W], F)
    flags = 0
    if not want_u:
        return At, w, V, flags
    rng = Rng()
    for i in range(n1):
        sd = W[i] if i < n else 0.0
        if i < n and sd <= FLT_MIN:
            flags |= 1
        ii = 0
        while ii < FILL_ATTEMPTS and sd <= FLT_MIN:
            ii += 1
            val0 = F(1. / m)
            for k in range(m):
                bit = (rng.next() & 256) != 0
                At[i, k] = val0 if bit == (fill == "opencv") else -val0
            for _ in range(2):
                for j in range(i):
                    sd = float(np.cumsum((At[i] * At[j]).astype(D))[-1])
                    t = (At[i].astype(D) - sd * At[j].astype(D)).astype(F)
                    At[i] = t
                    asum = np.cumsum(np.abs(t), dtype=F)[-1]
                    asum = F(1) / asum if asum > EPS * F(100) else F(0)
                    At[i] = At[i] * asum
            sd = math.sqrt(seqdot(At[i], At[i]))
        if not sd > FLT_MIN:
            flags |= 2
        s = F(1. / sd if sd > FLT_MIN else 0.)
        At[i] = At[i] * s
    return At, w, V, flags


def svd3(A, svd, fill):
    """cv::SVD::compute of a 3 x 3: (w, u, vt, flags)"""
    A = np.array(A, F).reshape(3, 3)
    if svd == "lapack":
        import scipy.linalg
        u, w, vt = scipy.linalg.svd(A, lapack_driver="gesdd")
        return w.astype(F), u.astype(F), vt.astype(F), 0
    At, w, V, flags = jacobi_svd(A.T.copy(), 3, fill=fill)
    return w, At.T.copy(), V, flags


def inv3(m):
    """cv::invert of a 3 x 3 CV_32F matrix (C.18)"""
    m = [float(v) for v in np.asarray(m).reshape(-1)]
    d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    if d == 0.0:
        return np.zeros((3, 3), F)
    d = 1.0 / d
    t = [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
         (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
         (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]
    return np.array(t, D).astype(F).reshape(3, 3)


def det3(m):
    m = [float(v) for v in np.asarray(m).reshape(-1)]
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])


def mul3(A, B):
    """a plain product (C.12's small-matrix path): ((a0 b0 + a1 b1) + a2 b2) in float"""
    A, B = np.asarray(A, F).reshape(3, -1), np.asarray(B, F)
    B = B.reshape(3, -1)
    return (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]


def normalize(pts):
    """Normalize (:749-795) over all key points [n, 2]: (meanX, meanY, sX, sY) and T"""
    n = len(pts)
    out = []
    for a in range(2):
        v = np.asarray(pts[:, a], F)                                 # (n > 0: a pair with fewer than eight correspondences never gets here)
        mean = np.cumsum(v, dtype=F)[-1] / F(n)
        dev = np.cumsum(np.abs(v - mean), dtype=F)[-1] / F(n)
        out.append((mean, F(1.0 / float(dev))))
    (mx, sx), (my, sy) = out
    T = np.array([[sx, 0, -mx * sx], [0, sy, -my * sy], [0, 0, 1]], F)
    return (mx, my, sx, sy), T


def _npts(c, n1, n2):
    return (c[:, 0] - n1[0]) * n1[2], (c[:, 1] - n1[1]) * n1[3], (c[:, 2] - n2[0]) * n2[2], (c[:, 3] - n2[1]) * n2[3]


def compute_h21(c8, n1, n2, svd, fill):
    u1, v1, u2, v2 = _npts(c8, n1, n2)
    A = np.zeros((16, 9), F)
    z, one = np.zeros(8, F), np.ones(8, F)
    A[0::2] = np.stack([z, z, z, -u1, -v1, -one, v2 * u1, v2 * v1, v2], 1)
    A[1::2] = np.stack([u1, v1, one, z, z, z, -u2 * u1, -u2 * v1, -u2], 1)
    if svd == "lapack":
        import scipy.linalg
        return scipy.linalg.svd(A, lapack_driver="gesdd")[2][8].astype(F).reshape(3, 3)
    return jacobi_svd(A.T.copy(), 9, want_u=False)[2][8].reshape(3, 3)


def compute_f21(c8, n1, n2, svd, fill):
    """returns (Fn, degenerate)"""
    u1, v1, u2, v2 = _npts(c8, n1, n2)
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones(8, F)], 1).astype(F)
    if svd == "lapack":
        import scipy.linalg
        Fpre, flags = scipy.linalg.svd(A, lapack_driver="gesdd")[2][8].astype(F).reshape(3, 3), 0
    else:
        At, _, _, flags = jacobi_svd(np.vstack([A, np.zeros((1, 9), F)]), 8, want_v=False, fill=fill)
        Fpre = At[8].reshape(3, 3)
    w, u, vt, _ = svd3(Fpre, svd, fill)
    Dg = np.diag(np.array([w[0], w[1], 0], F))
    return mul3(mul3(u, Dg), vt), flags != 0


def check_h(H21, H12, c, sigma):
    """CheckHomography (:305-388): (score, flags, chi [N, 2])"""
    th = F(5.991)
    inv = F(1.0 / float(F(sigma) * F(sigma)))
    u1, v1, u2, v2 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    h, g = np.asarray(H21, F).reshape(-1), np.asarray(H12, F).reshape(-1)
    with np.errstate(all="ignore"):
        w2 = (1.0 / (g[6] * u2 + g[7] * v2 + g[8]).astype(D)).astype(F)
        a, b = (g[0] * u2 + g[1] * v2 + g[2]) * w2, (g[3] * u2 + g[4] * v2 + g[5]) * w2
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv
        w1 = (1.0 / (h[6] * u1 + h[7] * v1 + h[8]).astype(D)).astype(F)
        a, b = (h[0] * u1 + h[1] * v1 + h[2]) * w1, (h[3] * u1 + h[4] * v1 + h[5]) * w1
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv
        out1, out2 = chi1 > th, chi2 > th
        add = np.stack([np.where(out1, F(0), th - chi1), np.where(out2, F(0), th - chi2)], 1).reshape(-1)
    score = np.cumsum(add, dtype=F)[-1] if len(add) else F(0)
    return score, ~(out1 | out2), np.stack([chi1 / th, chi2 / th], 1)


def check_f(F21, c, sigma):
    """CheckFundamental (:390-468)"""
    th, ths = F(3.841), F(5.991)
    inv = F(1.0 / float(F(sigma) * F(sigma)))
    u1, v1, u2, v2 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    f = np.asarray(F21, F).reshape(-1)
    with np.errstate(all="ignore"):
        a2, b2, c2 = f[0] * u1 + f[1] * v1 + f[2], f[3] * u1 + f[4] * v1 + f[5], f[6] * u1 + f[7] * v1 + f[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv
        a1, b1, c1 = f[0] * u2 + f[3] * v2 + f[6], f[1] * u2 + f[4] * v2 + f[7], f[2] * u2 + f[5] * v2 + f[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv
        out1, out2 = chi1 > th, chi2 > th
        add = np.stack([np.where(out1, F(0), ths - chi1), np.where(out2, F(0), ths - chi2)], 1).reshape(-1)
    score = np.cumsum(add, dtype=F)[-1] if len(add) else F(0)
    return score, ~(out1 | out2), np.stack([chi1 / th, chi2 / th], 1)


def null4(A, svd):
    """vt.row(3) of every 4 x 4 of A [n, 4, 4]"""
    if svd == "lapack":
        import scipy.linalg
        return np.array([scipy.linalg.svd(a, lapack_driver="gesdd")[2][3] for a in A.astype(F)], F).reshape(-1, 4)
    return np.linalg.svd(A.astype(D))[2][:, 3, :].astype(F)


def check_rt(R, t, c, inl, K, th2, svd):
    """CheckRT (:798-907) over the flagged correspondences.  Returns (nGood, cos of the 51st or 0, counted [N] bool, good [N] bool, P3D [N, 3], margin)"""
    fx, fy, cx, cy = (F(v) for v in K)
    R, t = np.asarray(R, F).reshape(3, 3), np.asarray(t, F).reshape(3)
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)
    P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], F)
    P2 = mul3(Km, np.hstack([R, t.reshape(3, 1)]))
    O2 = (mul3(R.T.copy(), t.reshape(3, 1)).reshape(3).astype(D) * -1.0).astype(F)
    N = len(c)
    counted, good, P3D, cosv = np.zeros(N, bool), np.zeros(N, bool), np.zeros((N, 3), F), np.zeros(N, F)
    q = np.flatnonzero(inl)
    margin = math.inf
    if len(q):
        cc = c[q]
        A = np.stack([cc[:, 0:1] * P1[2] - P1[0], cc[:, 1:2] * P1[2] - P1[1], cc[:, 2:3] * P2[2] - P2[0], cc[:, 3:4] * P2[2] - P2[1]], 1).astype(F)
        v = null4(A, svd)
        with np.errstate(all="ignore"):
            x = v[:, :3] * (1.0 / v[:, 3:4].astype(D)).astype(F)
            fin = np.isfinite(x).all(1)
            n2 = x - O2
            d1 = np.sqrt((x.astype(D) ** 2).sum(1)).astype(F)
            d2 = np.sqrt((n2.astype(D) ** 2).sum(1)).astype(F)
            cosp = ((x.astype(D) * n2.astype(D)).sum(1) / (d1 * d2).astype(D)).astype(F)
            low = cosp.astype(D) < 0.99998
            x2 = (mul3(R, x.T.copy()).T.astype(D) + t.astype(D)).astype(F)
            iz1 = (1.0 / x[:, 2].astype(D)).astype(F)
            e1 = (fx * x[:, 0] * iz1 + cx - cc[:, 0]) ** 2 + (fy * x[:, 1] * iz1 + cy - cc[:, 1]) ** 2
            iz2 = (1.0 / x2[:, 2].astype(D)).astype(F)
            e2 = (fx * x2[:, 0] * iz2 + cx - cc[:, 2]) ** 2 + (fy * x2[:, 1] * iz2 + cy - cc[:, 3]) ** 2
            ok = fin & ~((x[:, 2] <= 0) & low) & ~((x2[:, 2] <= 0) & low) & ~(e1 > th2) & ~(e2 > th2)
            # how far every comparison of a finite point is from flipping, relative
            rel = np.minimum.reduce([np.abs(e1 / th2 - 1), np.abs(e2 / th2 - 1), np.abs(x[:, 2]) / d1, np.abs(x2[:, 2]) / np.maximum(d2, F(1e-30)),
                                     np.abs(cosp.astype(D) - 0.99998) / 1e-5])
            rel = np.where(fin, rel, np.inf)
        counted[q], good[q] = ok, ok & low
        P3D[q[ok]] = x[ok]
        cosv[q] = cosp
        margin = rel
    n = int(counted.sum())
    cos51 = F(0)
    if n:
        cs = cosv[counted]
        key = np.where(np.isnan(cs), np.inf, cs.astype(D))
        cos51 = cs[np.argsort(key, kind="stable")[min(50, n - 1)]]
    near = np.zeros(N, bool)
    if len(q):
        near[q] = margin < 1e-3
    return n, cos51, counted, good, P3D, near


def parallax(c):
    with np.errstate(all="ignore"):
        return F(float(np.arccos(F(c)).astype(F) * F(180)) / PI)


class Result:
    pass


def initialize(kp1, kp2, matches, K, draws, sigma=1.0, max_iterations=200, min_parallax=1.0, min_triangulated=50, svd="jacobi", fill="opencv"):
    """Initialize (:44-121).  kp1 [N1, 2], kp2 [N2, 2] float32 (pt of ALL key points), matches [>= N1] (v is a correspondence iff 0 <= v < N2), draws
    [max_iterations, 8].  Returns a Result whose fields are the outputs of olf_initializer_io and what the scene builder needs to judge margins."""
    kp1, kp2 = np.asarray(kp1, F).reshape(-1, 2), np.asarray(kp2, F).reshape(-1, 2)
    N1, N2 = len(kp1), len(kp2)
    r = Result()
    feat = np.array([i for i in range(N1) if 0 <= matches[i] < N2], np.int64)
    r.feat, r.N = feat, len(feat)
    r.ok, r.model, r.hypothesis, r.degenerate = 0, 0, -1, False
    if r.N < 8:
        return r
    c = np.hstack([kp1[feat], kp2[np.asarray(matches)[feat]]]).astype(F)
    r.c = c
    n1, T1 = normalize(kp1)
    n2, T2 = normalize(kp2)
    T2inv, T2t = inv3(T2), T2.T.copy()
    SH = SF = F(0)
    r.H21 = r.F21 = None
    r.log_H, r.log_F = [], []
    flagsH = flagsF = np.zeros(r.N, bool)
    chiH = chiF = None
    r.win_H = r.win_F = -1
    for it in range(max_iterations):
        idx = sample8(r.N, draws[it])
        Hn = compute_h21(c[idx], n1, n2, svd, fill)
        H21i = mul3(mul3(T2inv, Hn), T1)
        H12i = inv3(H21i)
        s, fl, chi = check_h(H21i, H12i, c, sigma)
        r.log_H.append(float(s))
        if s > SH:
            SH, r.H21, flagsH, chiH, r.win_H = s, H21i, fl, chi, it
        Fn, deg = compute_f21(c[idx], n1, n2, svd, fill)
        r.degenerate |= deg
        F21i = mul3(mul3(T2t, Fn), T1)
        s, fl, chi = check_f(F21i, c, sigma) if not deg else (F(0), None, None)
        r.log_F.append(float(s))
        if s > SF:
            SF, r.F21, flagsF, chiF, r.win_F = s, F21i, fl, chi, it
    r.score_H, r.score_F, r.flags_H, r.flags_F, r.chi_H, r.chi_F = SH, SF, flagsH, flagsF, chiH, chiF
    with np.errstate(all="ignore"):
        RH = SH / (SH + SF)
    r.RH = float(RH)
    useH = bool(float(RH) > 0.40)
    r.model = 1 if useH else 2
    r.n_good, r.cos_parallax = [0] * 8, [F(0)] * 8
    inl = flagsH if useH else flagsF
    N = int(inl.sum())
    r.n_inliers = N
    fx, fy, cx, cy = (F(v) for v in K)
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)
    th2 = F(4.0 * float(F(sigma) * F(sigma)))
    Rs, ts = [], []
    r.gates = None
    if useH:                                                         # ReconstructH (:572-732)
        A = mul3(mul3(inv3(Km), r.H21), Km)
        w, U, Vt, _ = svd3(A, svd, fill)
        s = F(det3(U) * det3(Vt))
        d1, d2, d3 = w
        r.gates = (float(d1 / d2), float(d2 / d3))
        if float(d1 / d2) < 1.00001 or float(d2 / d3) < 1.00001:
            return r
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_stheta = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        stheta = [aux_stheta, -aux_stheta, -aux_stheta, aux_stheta]
        aux_sphi = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sphi = [aux_sphi, -aux_sphi, -aux_sphi, aux_sphi]
        for h in range(8):
            i = h & 3
            Rp = np.eye(3, dtype=F)
            if h < 4:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ctheta, -stheta[i], stheta[i], ctheta
                tp, scale = np.array([x1[i], 0, -x3[i]], F), d1 - d3
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sphi[i], -1, sphi[i], -cphi
                tp, scale = np.array([x1[i], 0, x3[i]], F), d1 + d3
            M = (mul3(U, Rp).astype(D) * float(s)).astype(F)
            Rs.append(mul3(M, Vt))
            tp = tp * scale
            t = mul3(U, tp.reshape(3, 1)).reshape(3)
            ts.append(t * F(1.0 / math.sqrt(float((t.astype(D) ** 2).sum()))))
    else:                                                            # ReconstructF (:470-570), DecomposeE (:909-929)
        M = (Km.T.astype(D) @ np.asarray(r.F21, F).astype(D)).astype(F) if r.F21 is not None else np.zeros((3, 3), F)
        if r.F21 is None:
            r.F21_missing = True
        E = mul3(M, Km)
        w, u, vt, _ = svd3(E, svd, fill)
        t = u[:, 2].copy()
        with np.errstate(all="ignore"):
            t = t * F(1.0 / math.sqrt(float((t.astype(D) ** 2).sum())))
        W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
        R1 = mul3(mul3(u, W), vt)
        if det3(R1) < 0:
            R1 = R1 * F(-1) + F(0)
        R2 = mul3((u.astype(D) @ W.T.astype(D)).astype(F), vt)
        if det3(R2) < 0:
            R2 = R2 * F(-1) + F(0)
        Rs, ts = [R1, R2, R1, R2], [t, t, t * F(-1) + F(0), t * F(-1) + F(0)]
    r.Rs, r.ts = Rs, ts
    res = [check_rt(Rs[h], ts[h], c, inl, K, th2, svd) for h in range(len(Rs))]
    r.near_rt = np.any([x[5] for x in res], axis=0)
    r.counted_h, r.near_h = [x[2] for x in res], [x[5] for x in res]
    for h, x in enumerate(res):
        r.n_good[h], r.cos_parallax[h] = x[0], x[1]
    ng = r.n_good
    chosen = -1
    r.margins = {}
    if useH:
        best = second = 0
        bi = -1
        for h in range(8):
            if ng[h] > best:
                second, best, bi = best, ng[h], h
            elif ng[h] > second:
                second = ng[h]
        par = parallax(r.cos_parallax[bi]) if bi >= 0 and ng[bi] > 0 else F(-1)
        r.margins = dict(second=0.75 * best - second if best else -math.inf, parallax=float(par) - min_parallax, tri=best - min_triangulated - 0.5, n09=best - 0.9 * N)
        if second < 0.75 * best and par >= F(min_parallax) and best > min_triangulated and best > 0.9 * N:
            chosen = bi
    else:
        mx = max(ng[:4])
        nmin = max(int(0.9 * N), min_triangulated)
        nsim = sum(1 for h in range(4) if ng[h] > 0.7 * mx)
        first = [h for h in range(4) if ng[h] == mx][0]
        par = parallax(r.cos_parallax[first]) if ng[first] > 0 else F(0)
        others = sorted(ng[:4])[-2]
        r.margins = dict(second=0.7 * mx - others if mx else math.inf, parallax=float(par) - min_parallax, tri=mx - nmin + 0.5)
        if not (mx < nmin or nsim > 1) and par > F(min_parallax):
            chosen = first
    r.parallax = float(par)
    if chosen >= 0:
        r.ok, r.hypothesis = 1, chosen
        r.R21, r.t21 = Rs[chosen], ts[chosen]
        r.counted, r.good, r.P3D = res[chosen][2], res[chosen][3], res[chosen][4]
    return r
