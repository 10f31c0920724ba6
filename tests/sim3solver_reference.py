"""A numpy restatement of Sim3Solver (src/Sim3Solver.cc) for tests/test_sim3solver_*.py.  It follows the reference's own route -- the quaternion from a
float32 Jacobi iteration (C.21), ang = atan2(norm(vec), q0) and cv::Rodrigues' sin / cos in float64, the cv::Mat products of C.12 / C.17 -- and has
switches, as tests/pose_reference.py has, whose spread is each output's own sensitivity:
  eig   "jacobi" (base) | "eigh": the eigenvector from numpy.linalg.eigh in float64
  acc   "double" (base) | "float": the sums of M, of the centroids and of the scale accumulated in float32
  rev   False (base) | True: those sums taken in reversed order
The loop of iterate() is literal.  Nothing here reads the library."""
import math
import types
import numpy as np

F = np.float32
D = np.float64
BASE = dict(eig="jacobi", acc="double", rev=False)
SWITCHED = (dict(eig="eigh", acc="double", rev=False), dict(eig="jacobi", acc="float", rev=False), dict(eig="jacobi", acc="double", rev=True))
NEAR = 1e-3


def gate(sf):
    """mvnMaxError: (size_t)(9.210 * sigmaSquare), sigmaSquare = sf * sf in float"""
    return int(9.210 * float(F(sf) * F(sf)))


def rot_apply(T, X):
    """R * x + t under C.12 for rows of X: the three products summed in float, the translation added in double, one rounding"""
    T, X = np.asarray(T, F), np.asarray(X, F).reshape(-1, 3)
    out = np.empty_like(X)
    for r in range(3):
        s = (T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]
        out[:, r] = (s.astype(D) + D(T[r, 3])).astype(F)
    return out


def image(X, cam):
    fx, fy, cx, cy = (F(v) for v in cam)
    with np.errstate(all="ignore"):
        invz = F(1) / X[:, 2]
        return np.stack([fx * (X[:, 0] * invz) + cx, fy * (X[:, 1] * invz) + cy], 1)


def correspondences(kps, counts, Tcw, world, valid, bad, cam, sf, pair, row, img_stride=1):
    """the constructor (:37-112) in the per-feature model: arrays of the kept correspondences in ascending i1, and the status bits"""
    a, b = pair
    cap = world.shape[1]
    N1, N2 = (min(max(int(counts[f * img_stride]), 0), cap) for f in (a, b))
    keep, status = [], 0
    for i1 in range(N1):
        v = int(row[i1])
        if not 0 <= v < N2:
            continue
        if valid is not None and not (valid[a, i1] and valid[b, v]):
            continue
        if bad is not None and (bad[a, i1] or bad[b, v]):
            continue
        o1, o2 = int(kps[a * img_stride, i1]["octave"]), int(kps[b * img_stride, v]["octave"])
        if not (0 <= o1 < len(sf) and 0 <= o2 < len(sf)):
            status |= 256
            continue
        keep.append((i1, v, o1, o2))
    C = types.SimpleNamespace(N=len(keep), N1=N1, status=status, cam=cam)
    k = np.array(keep, np.int64).reshape(-1, 4)
    C.i1 = k[:, 0]
    C.X1 = rot_apply(Tcw[a], world[a, k[:, 0]])
    C.X2 = rot_apply(Tcw[b], world[b, k[:, 1]])
    C.p1, C.p2 = image(C.X1, cam), image(C.X2, cam)
    C.g1 = np.array([gate(sf[o]) for o in k[:, 2]], np.int64)
    C.g2 = np.array([gate(sf[o]) for o in k[:, 3]], np.int64)
    return C


def iteration_cap(N, probability, min_inliers, max_iterations):
    its = 1
    if N > min_inliers:
        eps = float(F(min_inliers) / F(N))
        v = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(eps, 3)))
        its = v if v < max_iterations else max_iterations
    return max(1, min(its, max_iterations))


def sample(N, r):
    """three draws without replacement by swap-with-back (:163-177), literally"""
    avail, idx = list(range(N)), []
    for k in range(3):
        pos = int((float(int(r[k]) & 0x7fffffff) / 2147483648.0) * (N - k))
        idx.append(avail[pos])
        avail[pos] = avail[-1]
        avail.pop()
    return idx


def _hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(F(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(F(1) + a * a)
    return F(0)


def jacobi4(Nm):
    """C.21: cyclic Jacobi in float32; the row of the largest eigenvalue"""
    A = [[F(Nm[i][j]) for j in range(4)] for i in range(4)]
    V = [[F(i == j) for j in range(4)] for i in range(4)]
    W = [A[i][i] for i in range(4)]
    eps, half = F(1.1920928955078125e-7), F(0.5)
    for _ in range(30):
        changed = False
        for k in range(3):
            for l in range(k + 1, 4):
                p = A[k][l]
                if not abs(p) > eps:
                    continue
                y = (W[l] - W[k]) * half
                t = abs(y) + _hypot(p, y)
                s = _hypot(p, t)
                c = t / s
                s, t = p / s, (p / t) * p
                if y < 0:
                    s, t = -s, -t
                A[k][l] = F(0)
                W[k], W[l] = W[k] - t, W[l] + t

                def rot(a0, b0):
                    return a0 * c - b0 * s, a0 * s + b0 * c
                for i in range(4):
                    if i < k:
                        A[i][k], A[i][l] = rot(A[i][k], A[i][l])
                    elif k < i < l:
                        A[k][i], A[i][l] = rot(A[k][i], A[i][l])
                    elif i > l:
                        A[k][i], A[l][i] = rot(A[k][i], A[l][i])
                for i in range(4):
                    V[k][i], V[l][i] = rot(V[k][i], V[l][i])
                changed = True
        if not changed:
            break
    m = 0
    for i in range(1, 4):
        if W[m] < W[i]:
            m = i
    return np.array(V[m], F)


def _sum(terms, sw):
    terms = list(terms)[::-1] if sw["rev"] else list(terms)
    acc = F(0) if sw["acc"] == "float" else D(0)
    for t in terms:
        acc = acc + (F(t) if sw["acc"] == "float" else D(t))
    return acc


def fit(P1, P2, fix_scale, sw=BASE):
    """ComputeSim3 (:226-337).  P1, P2 [3 points][3] float32.  Returns a namespace with s, R, t, T12, T21 (float32)"""
    with np.errstate(all="ignore"):
        P1, P2 = np.asarray(P1, F), np.asarray(P2, F)
        third = F(1.0 / 3.0)
        O1 = np.array([F(_sum(P1[:, r], sw)) * third for r in range(3)], F)
        O2 = np.array([F(_sum(P2[:, r], sw)) * third for r in range(3)], F)
        Pr1, Pr2 = (P1 - O1).T.copy(), (P2 - O2).T.copy()              # [coordinate][point]
        M = np.array([[F(_sum([D(Pr2[i, k]) * D(Pr1[j, k]) if sw["acc"] == "double" else Pr2[i, k] * Pr1[j, k] for k in range(3)], sw))
                       for j in range(3)] for i in range(3)], F)
        m = M.astype(D)
        n11, n12, n13, n14 = m[0, 0] + m[1, 1] + m[2, 2], m[1, 2] - m[2, 1], m[2, 0] - m[0, 2], m[0, 1] - m[1, 0]
        n22, n23, n24 = m[0, 0] - m[1, 1] - m[2, 2], m[0, 1] + m[1, 0], m[2, 0] + m[0, 2]
        n33, n34, n44 = -m[0, 0] + m[1, 1] - m[2, 2], m[1, 2] + m[2, 1], -m[0, 0] - m[1, 1] + m[2, 2]
        Nm = np.array([[n11, n12, n13, n14], [n12, n22, n23, n24], [n13, n23, n33, n34], [n14, n24, n34, n44]], F)
        if sw["eig"] == "eigh" and np.isfinite(Nm).all():
            q = np.linalg.eigh(Nm.astype(D))[1][:, -1].astype(F)
        else:
            q = jacobi4(Nm)
        vec = q[1:4]
        nv = math.sqrt(float(np.sum(vec.astype(D) ** 2)))
        ang = math.atan2(nv, float(q[0]))
        rvec = (D(2 * ang) * vec.astype(D) / D(nv)).astype(F) if nv != 0 else np.full(3, np.nan, F)      # 0 / 0 at the identity
        r = rvec.astype(D)
        theta = math.sqrt(float(np.sum(r * r)))
        if theta < np.finfo(D).eps:
            R = np.eye(3, dtype=F)
        else:
            c, s = math.cos(theta), math.sin(theta)
            r = r / theta
            rx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
            R = (c * np.eye(3) + (1 - c) * np.outer(r, r) + s * rx).astype(F)
        H = types.SimpleNamespace(R=R)
        if not fix_scale:
            P3 = np.array([[(R[i, 0] * Pr2[0, k] + R[i, 1] * Pr2[1, k]) + R[i, 2] * Pr2[2, k] for k in range(3)] for i in range(3)], F)
            nom = _sum([D(a) * D(b) if sw["acc"] == "double" else a * b for a, b in zip(Pr1.reshape(-1), P3.reshape(-1))], sw)
            den = _sum([a * a for a in P3.reshape(-1)], sw)
            H.s = F(D(nom) / D(den))
        else:
            H.s = F(1)
        dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
        H.t = np.array([F(-D(H.s) * D(dot(R[r_], O2)) + D(O1[r_])) for r_ in range(3)], F)
        sRinv = (R.T.astype(D) * (1.0 / D(H.s))).astype(F)
        H.T12, H.T21 = np.eye(4, dtype=F), np.eye(4, dtype=F)
        H.T12[:3, :3], H.T12[:3, 3] = H.s * R, H.t
        H.T21[:3, :3] = sRinv
        H.T21[:3, 3] = [F(-1.0 * D(dot(sRinv[r_], H.t))) for r_ in range(3)]
        return H


def errors(H, C):
    """CheckInliers (:340-364): err1, err2 (float32) of every correspondence"""
    with np.errstate(all="ignore"):
        d1 = C.p1 - image(rot_apply(H.T12, C.X2), C.cam)
        d2 = image(rot_apply(H.T21, C.X1), C.cam) - C.p2
        e = lambda d: (d[:, 0].astype(D) * d[:, 0].astype(D) + d[:, 1].astype(D) * d[:, 1].astype(D)).astype(F)
        return e(d1), e(d2)


def evaluate(C, draws, j, fix_scale, sw=BASE):
    """iteration j: (hypothesis, flags, near) -- near: an error within a relative NEAR of its gate"""
    idx = sample(C.N, draws[j])
    H = fit(C.X1[idx], C.X2[idx], fix_scale, sw)
    e1, e2 = errors(H, C)
    g1, g2 = C.g1.astype(F), C.g2.astype(F)
    with np.errstate(all="ignore"):
        flags = (e1 < g1) & (e2 < g2)
        near = (np.abs(e1.astype(D) - g1) <= NEAR * g1) | (np.abs(e2.astype(D) - g2) <= NEAR * g2)
    return H, flags, near


def new_state():
    return types.SimpleNamespace(iterations_done=0, best_inliers=0, best=None)


def iterate(C, draws, st, n_iterations, fix_scale, probability=0.99, min_inliers=20, max_iterations=300, sw=BASE, log=None):
    """Sim3Solver::iterate (:140-207), literally.  st: new_state(), carried.  Returns a namespace: accepted, no_more, n_inliers, inliers (by i1, length
    N1), H (the accepted hypothesis).  log (a dict): iteration -> (count, flags, near)."""
    out = types.SimpleNamespace(accepted=0, no_more=0, n_inliers=0, inliers=np.zeros(C.N1, np.uint8), H=None)
    if C.N < min_inliers:
        out.no_more = 1
        return out
    cap = iteration_cap(C.N, probability, min_inliers, max_iterations)
    cur = 0
    while st.iterations_done < cap and cur < n_iterations:
        cur += 1
        j = st.iterations_done
        st.iterations_done += 1
        H, flags, near = evaluate(C, draws, j, fix_scale, sw)
        n = int(flags.sum())
        if log is not None:
            log[j] = (n, flags, near)
        if n >= st.best_inliers:
            st.best_inliers, st.best = n, H
            if n > min_inliers:
                out.accepted, out.n_inliers, out.H = 1, n, H
                out.inliers[C.i1[flags]] = 1
                return out
    if st.iterations_done >= cap:
        out.no_more = 1
    return out
