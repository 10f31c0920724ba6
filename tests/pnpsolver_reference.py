"""A numpy restatement of src/PnPsolver.cc in float64 / float32 as written: the constructor, SetRansacParameters, the sample of an iteration, EPnP's
compute_pose with everything it calls, CheckInliers, Refine and the literal loop of iterate (Refine at EVERY iteration with n >= min_inliers).  It reads
nothing from the library.  Switches (a namespace svd / acc / rev), as tests/sim3solver_reference.py has them:
  svd   "jacobi": the OpenCV calls as an OpenCV without LAPACK makes them (one-sided Jacobi in double, SVBkSb's threshold) -- the base; "numpy":
        numpy.linalg.svd / solve by lstsq / inv
  acc   False: the sums over the correspondences sequential in double (base); True: every term perturbed by a float32 rounding of its relative part
  rev   the sums over the correspondences taken in reverse
A hypothesis in which OpenCV would fill a singular vector from its random generator (a row norm <= DBL_MIN where the vector is read) is degenerate:
it counts no inlier (the library's definition)."""
import math
import types
import numpy as np

F = np.float32
BASE = types.SimpleNamespace(svd="jacobi", acc=False, rev=False)
SWITCHED = (types.SimpleNamespace(svd="numpy", acc=False, rev=False), types.SimpleNamespace(svd="jacobi", acc=True, rev=False),
            types.SimpleNamespace(svd="jacobi", acc=False, rev=True))
DBL_EPS, DBL_MIN = 2.220446049250313e-16, 2.2250738585072014e-308


def seq(x):
    """the sum of a vector in index order from +0"""
    return float(np.cumsum(np.asarray(x, np.float64))[-1]) if len(x) else 0.0


def csum(terms, sw):
    """a sum over correspondences, terms [n, ...]: the column sums in the switch's order"""
    t = np.asarray(terms, np.float64)
    if sw.acc:
        t = t * (1.0 + (np.arange(t.shape[0]) % 3 - 1).reshape((-1,) + (1,) * (t.ndim - 1)) * 2.0 ** -24)
    if sw.rev:
        t = t[::-1]
    return np.cumsum(t, axis=0)[-1]


# ---- the parameters (:121-157)
def parameters(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5):
    n_min = int(F(N) * F(epsilon))
    n_min = max(n_min, min_inliers, min_set)
    its = 1
    if N > n_min:
        e = F(epsilon)
        if e < F(n_min) / F(N):
            e = F(n_min) / F(N)
        x = 1 - math.pow(float(e), 3)
        den = math.log(x) if x > 0 else -math.inf                   # (libm's log(0))
        v = math.log(1 - probability) / den if den != 0 else -math.inf      # (a negative over +0)
        its = (int(math.ceil(v)) if v > 0 else 0) if v < max_iterations else max_iterations
    return n_min, max(1, min(its, max_iterations))


def max_error(sf, th2):
    return F(F(F(sf) * F(sf)) * F(th2))


# ---- the constructor (:67-110)
def correspondences(kps, counts, world, valid, bad, sf, th2, pair, row, img_stride=1):
    kf, fr = pair
    cap = world.shape[1]
    Nf, Nk = (min(max(int(counts[f * img_stride]), 0), cap) for f in (fr, kf))
    C = types.SimpleNamespace(Nf=Nf, status=0, feat=[], P2=[], P3=[], maxerr=[])
    for i in range(Nf):
        v = int(row[i])
        if not 0 <= v < Nk:
            continue
        if (valid is not None and not valid[kf, v]) or (bad is not None and bad[kf, v]):
            continue
        o = int(kps[fr * img_stride, i]["octave"])
        if not 0 <= o < len(sf):
            C.status |= 256
            continue
        C.feat.append(i)
        C.P2.append((kps[fr * img_stride, i]["x"], kps[fr * img_stride, i]["y"]))
        C.P3.append(world[kf, v])
        C.maxerr.append(max_error(sf[o], th2))
    C.N = len(C.feat)
    C.feat = np.array(C.feat, np.int64)
    C.P2, C.P3, C.maxerr = np.array(C.P2, F).reshape(-1, 2), np.array(C.P3, F).reshape(-1, 3), np.array(C.maxerr, F)
    return C


# ---- the sample (:188-201) under C.20
def sample(N, r):
    avail = list(range(N))
    idx = []
    for k in range(4):
        pos = int(((int(r[k]) & 0x7fffffff) / 2147483648.0) * len(avail))
        idx.append(avail[pos])
        avail[pos] = avail[-1]
        avail.pop()
    return idx


# ---- OpenCV without LAPACK, double
def jacobi_svd(A, want_v=True):
    """cv::SVD of A (m x n, m >= n): returns (w, Ut rows = left singular vectors [n, m], Vt [n, n], full) -- full False when a row norm is <= DBL_MIN"""
    At = np.array(A, np.float64).T.copy()
    n, m = At.shape
    V = np.eye(n)
    W = np.array([seq(At[i] * At[i]) for i in range(n)])
    eps = DBL_EPS * 10
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                a, b = W[i], W[j]
                p = seq(At[i] * At[j])
                if abs(p) <= eps * math.sqrt(a * b) if a * b >= 0 else False:
                    continue
                p *= 2
                beta = a - b
                g2 = p * p + beta * beta
                gamma = math.sqrt(g2) if g2 >= 0 else math.nan
                with np.errstate(all="ignore"):
                    if beta < 0:
                        delta = (gamma - beta) * 0.5
                        s = np.sqrt(np.float64(delta) / gamma)
                        c = np.float64(p) / (gamma * s * 2)
                    else:
                        c = np.sqrt((np.float64(gamma) + beta) / (gamma * 2))
                        s = np.float64(p) / (gamma * c * 2)
                    t0, t1 = c * At[i] + s * At[j], (-s) * At[i] + c * At[j]
                    At[i], At[j] = t0, t1
                    W[i], W[j] = seq(t0 * t0), seq(t1 * t1)
                    V[i], V[j] = c * V[i] + s * V[j], (-s) * V[i] + c * V[j]
                changed = True
        if not changed:
            break
    with np.errstate(all="ignore"):
        W = np.array([np.sqrt(np.float64(seq(At[i] * At[i]))) for i in range(n)])
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[[i, j]] = W[[j, i]]
            At[[i, j]] = At[[j, i]]
            V[[i, j]] = V[[j, i]]
    full = True
    with np.errstate(all="ignore"):
        for i in range(n):
            if W[i] <= DBL_MIN:
                full = False
            At[i] = At[i] * (1.0 / W[i] if W[i] > DBL_MIN else 0.0)
    return W, At, V, full


def svd(A, sw):
    """(w, Ut, Vt, full) of A under the switch"""
    if sw.svd == "jacobi":
        return jacobi_svd(A)
    with np.errstate(all="ignore"):
        try:
            u, w, vt = np.linalg.svd(np.asarray(A, np.float64), full_matrices=False)
        except np.linalg.LinAlgError:
            n = np.asarray(A).shape[1]
            return np.full(n, np.nan), np.full((n, np.asarray(A).shape[0]), np.nan), np.full((n, n), np.nan), True
    return w, u.T.copy(), vt.copy(), bool((w > DBL_MIN).all() or np.isnan(w).any())


def backsubst_solve(A, b, sw):
    """cvSolve(A, b, x, CV_SVD)"""
    w, Ut, Vt, _ = svd(A, sw)
    n = len(w)
    th = seq(w) * (DBL_EPS * 2)
    x = np.zeros(n)
    for i in range(n):
        if abs(w[i]) <= th:
            continue
        with np.errstate(all="ignore"):
            s = seq(Ut[i] * b) * (1.0 / w[i])
            x = x + s * Vt[i]
    return x


def backsubst_invert(A, sw):
    """cvInvert(A, Ainv, CV_SVD) of a 3 x 3"""
    w, Ut, Vt, _ = svd(A, sw)
    th = seq(w) * (DBL_EPS * 2)
    inv = np.zeros((3, 3))
    for i in range(3):
        if abs(w[i]) <= th:
            continue
        with np.errstate(all="ignore"):
            buf = Ut[i] * (1.0 / w[i])
            inv = inv + np.outer(Vt[i], buf)
    return inv


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def qr_solve(A, b, x):
    """:860-950, A [6, 4] and b changed in place; x left as it is at a singular column (C.25)"""
    nr, nc = A.shape
    A1, A2 = np.zeros(nc), np.zeros(nc)
    for k in range(nc):
        eta = abs(A[k, k])
        for i in range(k + 1, nr):
            eta = max(eta, abs(A[i - 1, k])) if not math.isnan(abs(A[i - 1, k])) and eta < abs(A[i - 1, k]) else eta
        if eta == 0:
            return
        inv_eta = 1.0 / eta
        s = 0.0
        for i in range(k, nr):
            A[i, k] *= inv_eta
            s += A[i, k] * A[i, k]
        sigma = math.sqrt(s) if s >= 0 else math.nan
        if A[k, k] < 0:
            sigma = -sigma
        A[k, k] += sigma
        A1[k] = sigma * A[k, k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s += A[i, k] * A[i, j]
            tau = s / A1[k]
            for i in range(k, nr):
                A[i, j] -= tau * A[i, k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i, j] * b[i]
        tau /= A1[j]
        for i in range(j, nr):
            b[i] -= tau * A[i, j]
    x[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s += A[i, j] * x[j]
        x[i] = (b[i] - s) / A2[i]


def gauss_newton(L, rho, betas):
    x = np.zeros(4)
    with np.errstate(all="ignore"):
        for _ in range(5):
            A, b = np.zeros((6, 4)), np.zeros(6)
            b0, b1, b2, b3 = (np.float64(v) for v in betas)
            for i in range(6):
                r = L[i]
                A[i, 0] = 2 * r[0] * b0 + r[1] * b1 + r[3] * b2 + r[6] * b3
                A[i, 1] = r[1] * b0 + 2 * r[2] * b1 + r[4] * b2 + r[7] * b3
                A[i, 2] = r[3] * b0 + r[4] * b1 + 2 * r[5] * b2 + r[8] * b3
                A[i, 3] = r[6] * b0 + r[7] * b1 + r[8] * b2 + 2 * r[9] * b3
                b[i] = rho[i] - (r[0] * b0 * b0 + r[1] * b0 * b1 + r[2] * b1 * b1 + r[3] * b0 * b2 + r[4] * b1 * b2 + r[5] * b2 * b2 + r[6] * b0 * b3 +
                                 r[7] * b1 * b3 + r[8] * b2 * b3 + r[9] * b3 * b3)
            qr_solve(A, b, x)
            betas = [np.float64(betas[i]) + x[i] for i in range(4)]
    return betas


def _sqrt(v):
    with np.errstate(all="ignore"):
        return np.sqrt(np.float64(v))


def compute_pose(pws, us, cam, sw=BASE):
    """:477-525.  pws [n, 3], us [n, 2] float64; cam = (fu, fv, uc, vc) float64.  Returns a namespace R [3, 3], t [3], variant (0..2), full, errors"""
    fu, fv, uc, vc = (np.float64(v) for v in cam)
    n = len(pws)
    full = True
    with np.errstate(all="ignore"):
        cws = np.zeros((4, 3))
        cws[0] = csum(pws, sw) / n
        d = pws - cws[0]
        S = csum(np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1), sw)
        PtP = np.array([[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]])
        dc, uct, _, ok = svd(PtP, sw)
        full &= ok
        for i in range(1, 4):
            cws[i] = cws[0] + _sqrt(dc[i - 1] / n) * uct[i - 1]
        cc = (cws[1:] - cws[0]).T.copy()
        ci = backsubst_invert(cc, sw) if sw.svd == "jacobi" else _np_inv(cc)
        al = np.zeros((n, 4))
        for j in range(3):
            al[:, 1 + j] = (ci[j, 0] * d[:, 0] + ci[j, 1] * d[:, 1]) + ci[j, 2] * d[:, 2]
        al[:, 0] = ((1.0 - al[:, 1]) - al[:, 2]) - al[:, 3]
        M1, M2 = np.zeros((n, 12)), np.zeros((n, 12))
        for k in range(4):
            M1[:, 3 * k], M1[:, 3 * k + 2] = al[:, k] * fu, al[:, k] * (uc - us[:, 0])
            M2[:, 3 * k + 1], M2[:, 3 * k + 2] = al[:, k] * fv, al[:, k] * (vc - us[:, 1])
        rows = np.empty((2 * n, 12, 12))
        rows[0::2] = M1[:, :, None] * M1[:, None, :]
        rows[1::2] = M2[:, :, None] * M2[:, None, :]
        if sw.acc or sw.rev:
            MtM = csum(rows[0::2] + rows[1::2] if sw.acc else rows, sw)
        else:
            MtM = np.cumsum(rows, axis=0)[-1]
        MtM = np.triu(MtM) + np.triu(MtM, 1).T
        _, ut, _, ok = svd(MtM, sw)
        full &= ok
        v = [ut[11], ut[10], ut[9], ut[8]]
        L = np.zeros((6, 10))
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        for r, (a, b) in enumerate(pairs):
            dv = [v[i][3 * a:3 * a + 3] - v[i][3 * b:3 * b + 3] for i in range(4)]
            L[r] = [dot3(dv[0], dv[0]), 2.0 * dot3(dv[0], dv[1]), dot3(dv[1], dv[1]), 2.0 * dot3(dv[0], dv[2]), 2.0 * dot3(dv[1], dv[2]), dot3(dv[2], dv[2]),
                    2.0 * dot3(dv[0], dv[3]), 2.0 * dot3(dv[1], dv[3]), 2.0 * dot3(dv[2], dv[3]), dot3(dv[3], dv[3])]
        rho = np.array([dot3(cws[a] - cws[b], cws[a] - cws[b]) for a, b in pairs])
        solve = (lambda A: backsubst_solve(A, rho, sw)) if sw.svd == "jacobi" else (lambda A: _np_lstsq(A, rho))
        betas = []
        b4 = solve(L[:, [0, 1, 3, 6]])
        if b4[0] < 0:
            b0 = _sqrt(-b4[0]); betas.append([b0, -b4[1] / b0, -b4[2] / b0, -b4[3] / b0])
        else:
            b0 = _sqrt(b4[0]); betas.append([b0, b4[1] / b0, b4[2] / b0, b4[3] / b0])
        b3 = solve(L[:, [0, 1, 2]])
        if b3[0] < 0:
            bb = [_sqrt(-b3[0]), _sqrt(-b3[2]) if b3[2] < 0 else 0.0]
        else:
            bb = [_sqrt(b3[0]), _sqrt(b3[2]) if b3[2] > 0 else 0.0]
        if b3[1] < 0:
            bb[0] = -bb[0]
        betas.append(bb + [0.0, 0.0])
        b5 = solve(L[:, [0, 1, 2, 3, 4]])
        if b5[0] < 0:
            bb = [_sqrt(-b5[0]), _sqrt(-b5[2]) if b5[2] < 0 else 0.0]
        else:
            bb = [_sqrt(b5[0]), _sqrt(b5[2]) if b5[2] > 0 else 0.0]
        if b5[1] < 0:
            bb[0] = -bb[0]
        betas.append(bb + [b5[3] / np.float64(bb[0]), 0.0])
        Rs, ts, errs = [], [], []
        for bt in betas:
            bt = gauss_newton(L, rho, bt)
            ccs = np.zeros(12)
            for i in range(4):
                ccs = ccs + bt[i] * v[i]
            ccs = ccs.reshape(4, 3)
            pcs = ((al[:, 0:1] * ccs[0] + al[:, 1:2] * ccs[1]) + al[:, 2:3] * ccs[2]) + al[:, 3:4] * ccs[3]
            if pcs[0, 2] < 0.0:
                ccs, pcs = -ccs, -pcs
            pc0, pw0 = csum(pcs, sw) / n, csum(pws, sw) / n
            dp, dw = pcs - pc0, pws - pw0
            abt = csum(dp[:, :, None] * dw[:, None, :], sw)
            _, Ut, Vt, ok = svd(abt, sw)
            full &= ok
            U, V = Ut.T, Vt.T
            R = np.array([[dot3(U[i], V[j]) for j in range(3)] for i in range(3)])
            det = (R[0, 0] * R[1, 1] * R[2, 2] + R[0, 1] * R[1, 2] * R[2, 0] + R[0, 2] * R[1, 0] * R[2, 1] - R[0, 2] * R[1, 1] * R[2, 0] -
                   R[0, 1] * R[1, 0] * R[2, 2] - R[0, 0] * R[1, 2] * R[2, 1])
            if det < 0:
                R[2] = -R[2]
            t = np.array([pc0[i] - dot3(R[i], pw0) for i in range(3)])
            Xc = ((R[0, 0] * pws[:, 0] + R[0, 1] * pws[:, 1]) + R[0, 2] * pws[:, 2]) + t[0]
            Yc = ((R[1, 0] * pws[:, 0] + R[1, 1] * pws[:, 1]) + R[1, 2] * pws[:, 2]) + t[1]
            iz = 1.0 / (((R[2, 0] * pws[:, 0] + R[2, 1] * pws[:, 1]) + R[2, 2] * pws[:, 2]) + t[2])
            ue, ve = uc + fu * Xc * iz, vc + fv * Yc * iz
            errs.append(csum(np.sqrt((us[:, 0] - ue) * (us[:, 0] - ue) + (us[:, 1] - ve) * (us[:, 1] - ve)), sw) / n)
            Rs.append(R); ts.append(t)
        N = 0
        if errs[1] < errs[0]:
            N = 1
        if errs[2] < errs[N]:
            N = 2
    return types.SimpleNamespace(R=Rs[N], t=ts[N], variant=N, full=bool(full), errors=errs)


def _np_inv(A):
    try:
        return np.linalg.pinv(A)
    except np.linalg.LinAlgError:
        return np.full((3, 3), np.nan)


def _np_lstsq(A, b):
    try:
        return np.linalg.lstsq(A, b, rcond=None)[0]
    except np.linalg.LinAlgError:
        return np.full(A.shape[1], np.nan)


# ---- CheckInliers (:308-339)
def check_inliers(C, R, t, cam):
    """(flags, error2) with the mixed widths as written"""
    fu, fv, uc, vc = (np.float64(v) for v in cam)
    with np.errstate(all="ignore"):
        P = C.P3.astype(np.float64)
        Xc = ((((R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1]) + R[0, 2] * P[:, 2]) + t[0])).astype(F)
        Yc = ((((R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1]) + R[1, 2] * P[:, 2]) + t[1])).astype(F)
        iz = (1.0 / (((R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1]) + R[2, 2] * P[:, 2]) + t[2])).astype(F)
        ue = uc + fu * Xc.astype(np.float64) * iz.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * iz.astype(np.float64)
        dx, dy = (C.P2[:, 0].astype(np.float64) - ue).astype(F), (C.P2[:, 1].astype(np.float64) - ve).astype(F)
        e2 = dx * dx + dy * dy
        return e2 < C.maxerr, e2


def tcw(R, t):
    T = np.eye(4, dtype=F)
    T[:3, :3], T[:3, 3] = np.asarray(R).astype(F), np.asarray(t).astype(F)
    return T


def fit(C, idx, cam, sw=BASE):
    """compute_pose of the listed correspondences and CheckInliers of all: (pose, flags, error2, n); a degenerate pose counts nothing"""
    H = compute_pose(C.P3[idx].astype(np.float64), C.P2[idx].astype(np.float64), cam, sw)
    flags, e2 = check_inliers(C, H.R, H.t, cam)
    if not H.full:
        flags = np.zeros(C.N, bool)
    return H, flags, e2, int(flags.sum())


def new_state():
    return types.SimpleNamespace(iterations_done=0, best_inliers=0, best_flags=None, best_Tcw=None)


def iterate(C, draws, st, n_iterations, cam, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, sw=BASE, log=None):
    """PnPsolver::iterate (:165-258), literally: Refine runs at every iteration with n >= min_inliers, on the best set so far.  log[j] = (n, variant,
    error2, maxerr-relative flags, refine tuple or None).  Returns a namespace accepted (a pose is returned), no_more, n_inliers, inliers (by
    correspondence), Tcw, refined (True: Refine accepted), refines (the iterations at which Refine ran with their outcomes)"""
    out = types.SimpleNamespace(accepted=0, no_more=0, n_inliers=0, inliers=np.zeros(C.N, bool), Tcw=None, refined=False, degenerate=False)
    min_eff, cap = parameters(C.N, probability, min_inliers, max_iterations, min_set, epsilon)
    out.min_eff, out.cap = min_eff, cap
    if C.N < min_eff:
        out.no_more = 1
        return out
    cur = 0
    n_iterations = min(n_iterations, max_iterations)
    while st.iterations_done < cap or cur < n_iterations:
        cur += 1
        j = st.iterations_done
        st.iterations_done += 1
        idx = sample(C.N, draws[j % max_iterations])
        H, flags, e2, n = fit(C, idx, cam, sw)
        out.degenerate |= not H.full
        rec = None
        if n >= min_eff:
            if n > st.best_inliers:
                st.best_flags, st.best_inliers, st.best_Tcw = flags.copy(), n, tcw(H.R, H.t)
            Hr, rflags, re2, rn = fit(C, np.flatnonzero(st.best_flags), cam, sw)
            out.degenerate |= not Hr.full
            rec = (rn, rflags, re2, Hr)
        if log is not None:
            log[j] = (n, H.variant, e2, flags, rec, H)
        if rec is not None and rec[0] > min_eff:
            out.accepted, out.refined, out.n_inliers, out.inliers, out.Tcw = 1, True, rec[0], rec[1].copy(), tcw(rec[3].R, rec[3].t)
            return out
    out.no_more = 1
    if st.best_inliers >= min_eff:
        out.accepted, out.n_inliers, out.inliers, out.Tcw = 1, st.best_inliers, st.best_flags.copy(), st.best_Tcw
    return out
