"""Restatements of LocalMapping::ComputeF12 (src/LocalMapping.cc:536-553), the body of LocalMapping::CreateNewMapPoints behind the search (:245-253,
:286-431) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:342-383), operation for operation in numpy.float32 / Python float (double) scalars under the
project's conventions (C.4 no contraction, C.12 cv::gemm, C.17 Mat / scalar, C.18 cv::invert).  Parity unpinned, like everything behind OpenCV.

The null vector of the triangulation comes from numpy.linalg.svd, not from a restated Jacobi iteration: `base` in float64, and two switched runs, float32
(LAPACK's sgesdd through scipy.linalg.svd, which an OpenCV built with LAPACK also calls) and float64 with A's rows reversed.  Their spread is the yardstick for triangulated points.
cosf / atan2f are the host's libm (tests/test_host_cpu.py sweeps the library's restatements against it)."""
import ctypes
import math
import numpy as np

F = np.float32
_libm = ctypes.CDLL("libm.so.6")
_libm.cosf.restype = _libm.atan2f.restype = ctypes.c_float
_libm.cosf.argtypes = [ctypes.c_float]
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
cosf = lambda x: F(_libm.cosf(float(x)))
atan2f = lambda y, x: F(_libm.atan2f(float(y), float(x)))

NONE, TRIANGULATED, UNPROJECT_1, UNPROJECT_2 = 0, 1, 2, 3
LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE_RATIO = range(16, 24)
CREATED = (TRIANGULATED, UNPROJECT_1, UNPROJECT_2)


def f32s(a):
    """the entries of an array as numpy.float32 scalars"""
    return [F(v) for v in np.asarray(a, dtype=np.float32).reshape(-1)]


def dot3_small(a, b):
    """cv::gemm's small-matrix path (C.12): ((a0 * b0 + a1 * b1) + a2 * b2) in float"""
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def inv3(m):
    """cv::invert of a 3 x 3 CV_32F matrix (C.18): determinant and cofactors in double, one rounding per element"""
    m = [float(v) for v in m]
    d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    if d == 0.0:
        return [F(0)] * 9
    d = 1.0 / d
    t = [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
         (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
         (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]
    return [F(v) for v in t]


def mul3(A, B):
    return [dot3_small(A[3 * r:3 * r + 3], [B[c], B[3 + c], B[6 + c]]) for r in range(3) for c in range(3)]


def compute_f12(T1, T2, cam):
    """:536-553.  T1, T2: 4 x 4 poses; cam = (fx, fy, cx, cy).  Returns F12 [3, 3] float32."""
    T1, T2 = np.asarray(T1, np.float32).reshape(4, 4), np.asarray(T2, np.float32).reshape(4, 4)
    R12, M = [], []
    for i in range(3):
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc += float(T1[i, k]) * float(T2[j, k])             # R1w * R2w.t(): the generic path, a double sum
            R12.append(F(acc))
            M.append(F(-1.0 * acc))                                  # (-R1w) * R2w.t(): alpha = -1 on the double sum
    t2w = f32s(T2[:3, 3])
    t12 = [F(float(dot3_small(M[3 * i:3 * i + 3], t2w)) + float(T1[i, 3])) for i in range(3)]
    z = F(0)
    t12x = [z, -t12[2], t12[1], t12[2], z, -t12[0], -t12[1], t12[0], z]
    fx, fy, cx, cy = (F(v) for v in cam)
    K1t = [fx, z, z, z, fy, z, cx, cy, F(1)]
    K2 = [fx, z, cx, z, fy, cy, z, z, F(1)]
    out = mul3(mul3(mul3(inv3(K1t), t12x), R12), inv3(K2))
    return np.array(out, np.float32).reshape(3, 3)


def update_normal_and_depth(obs_kf, obs_slot, world, ref_kf, kf_Ow, ref_octaves, sf):
    """:342-383 of one point that is not bad.  obs_kf / obs_slot: its observation row in iteration order; world [3]; kf_Ow [n_kf, 3]; ref_octaves: mvKeysUn[.].octave
    of the reference key frame; sf: mvScaleFactors.  Returns None for an empty row (:357), else (normal [3], mfMaxDistance, mfMinDistance)."""
    if len(obs_kf) == 0:
        return None
    observations = {}
    for kf, slot in zip(obs_kf, obs_slot):
        observations.setdefault(int(kf), int(slot))
    P = f32s(world)
    normal, n = [F(0)] * 3, 0
    for kf in observations:
        Owi = f32s(kf_Ow[kf])
        normali = [P[k] - Owi[k] for k in range(3)]
        nrm = math.sqrt(sum(float(v) * float(v) for v in normali))   # cv::norm: a double
        inv = F(1.0 / nrm)                                           # Mat / scalar (C.17)
        normal = [normal[k] + normali[k] * inv for k in range(3)]
        n += 1
    Owr = f32s(kf_Ow[ref_kf])
    PC = [P[k] - Owr[k] for k in range(3)]
    dist = F(math.sqrt(sum(float(v) * float(v) for v in PC)))
    if ref_kf not in observations:
        observations[ref_kf] = 0                                     # std::map::operator[] inserts a zero
    level = int(ref_octaves[observations[ref_kf]])
    sf = f32s(sf)
    maxd = dist * sf[level]
    mind = maxd / sf[len(sf) - 1]
    invn = F(1.0 / float(n))
    return np.array([v * invn for v in normal], np.float32), maxd, mind


def kf_pose(Tcw):
    """KeyFrame::SetPose (src/KeyFrame.cc:148-162): Rcw rows, tcw, Ow = -Rwc * tcw (a plain product on the materialised transpose)"""
    T = np.asarray(Tcw, np.float32).reshape(4, 4)
    R = [f32s(T[r, :3]) for r in range(3)]
    t = f32s(T[:3, 3])
    Ow = [F(float(dot3_small([R[0][r], R[1][r], R[2][r]], t)) * -1.0) for r in range(3)]
    return R, t, Ow


def short_baseline(P1, P2, mb):
    d = [P2[2][k] - P1[2][k] for k in range(3)]
    return F(math.sqrt(sum(float(v) * float(v) for v in d))) < F(mb)


def null_vector(A, svd):
    A64 = np.array([[float(v) for v in row] for row in A], np.float64)
    if svd == "f32":
        # (numpy.linalg.svd of a float32 matrix computes in double and rounds the result: scipy's calls the single-precision driver)
        import scipy.linalg
        vt = scipy.linalg.svd(A64.astype(np.float32), lapack_driver="gesdd")[2]
    elif svd == "rev":
        vt = np.linalg.svd(A64[::-1])[2]
    else:
        vt = np.linalg.svd(A64)[2]
    return f32s(vt[3])


class Margins:
    """the smallest margin of the comparisons one match evaluates: absolute for the cosine comparisons, relative for the gates that depend on x3D"""

    def __init__(self):
        self.cos, self.x3d = math.inf, math.inf

    def c(self, a, b):
        self.cos = min(self.cos, abs(float(a) - float(b)))

    def x(self, a, b, scale=None):
        a, b = float(a), float(b)
        s = max(abs(a), abs(b)) if scale is None else float(scale)
        self.x3d = min(self.x3d, abs(a - b) / s if s > 0 else 0.0)


def _row_dot(R, t, r, x):
    return F(sum(float(R[r][k]) * float(x[k]) for k in range(3)) + float(t[r]))


def _reproj_fails(P, cam, x3D, z, kx, ky, ur, sf, mg):
    fx, fy, cx, cy, mbf = cam
    sigma2 = sf * sf
    x, y = _row_dot(P[0], P[1], 0, x3D), _row_dot(P[0], P[1], 1, x3D)
    invz = F(1.0 / float(z))
    u, v = fx * x * invz + cx, fy * y * invz + cy
    ex, ey = u - kx, v - ky
    if not ur >= 0:
        e2, thr = ex * ex + ey * ey, 5.991 * float(sigma2)
    else:
        er = (u - mbf * invz) - ur
        e2, thr = ex * ex + ey * ey + er * er, 7.8 * float(sigma2)
    mg.x(e2, thr)
    return float(e2) > thr


def create_point(P1, P2, cam, mb, ratio_factor, k1, k2, svd="base"):
    """:286-431 of one match.  P1, P2: kf_pose of the current key frame and the neighbour; cam = (fx, fy, cx, cy, mbf) as float32; k1, k2 = (x, y, mvuRight,
    mvDepth, mvScaleFactors[octave]) as float32.  Returns (code, x3D or None, Margins)."""
    fx, fy, cx, cy, mbf = cam
    invfx, invfy = F(1) / fx, F(1) / fy
    mg = Margins()
    x1, y1, ur1, d1, sf1 = k1
    x2, y2, ur2, d2, sf2 = k2
    bS1, bS2 = bool(ur1 >= 0), bool(ur2 >= 0)
    xn1 = [(x1 - cx) * invfx, (y1 - cy) * invfy, F(1)]
    xn2 = [(x2 - cx) * invfx, (y2 - cy) * invfy, F(1)]
    (R1, t1, Ow1), (R2, t2, Ow2) = P1, P2
    ray1 = [dot3_small([R1[0][r], R1[1][r], R1[2][r]], xn1) for r in range(3)]
    ray2 = [dot3_small([R2[0][r], R2[1][r], R2[2][r]], xn2) for r in range(3)]
    dd = lambda a, b: sum(float(a[k]) * float(b[k]) for k in range(3))
    cosRays = F(dd(ray1, ray2) / (math.sqrt(dd(ray1, ray1)) * math.sqrt(dd(ray2, ray2))))
    cosS1 = cosS2 = cosRays + F(1)
    if bS1:
        cosS1 = cosf(F(2) * atan2f(F(mb) / F(2), d1))
    elif bS2:
        cosS2 = cosf(F(2) * atan2f(F(mb) / F(2), d2))
    cosS = min(cosS1, cosS2)

    def lt(a, b):
        mg.c(a, b)
        return a < b

    if lt(cosRays, cosS) and lt(F(0), cosRays) and (bS1 or bS2 or lt(float(cosRays), 0.9998)):
        T1 = [R1[r] + [t1[r]] for r in range(3)]
        T2 = [R2[r] + [t2[r]] for r in range(3)]
        A = [[xn1[0] * T1[2][k] - T1[0][k] for k in range(4)], [xn1[1] * T1[2][k] - T1[1][k] for k in range(4)],
             [xn2[0] * T2[2][k] - T2[0][k] for k in range(4)], [xn2[1] * T2[2][k] - T2[1][k] for k in range(4)]]
        v4 = null_vector(A, svd)
        if v4[3] == 0:
            return W_ZERO, None, mg
        inv = F(1.0 / float(v4[3]))
        x3D, code = [v4[k] * inv for k in range(3)], TRIANGULATED
    elif bS1 and lt(cosS1, cosS2):
        x3D, code = _unproject(P1, x1, y1, d1, cx, cy, invfx, invfy), UNPROJECT_1
    elif bS2 and lt(cosS2, cosS1):
        x3D, code = _unproject(P2, x2, y2, d2, cx, cy, invfx, invfy), UNPROJECT_2
    else:
        return LOW_PARALLAX, None, mg
    cam_norm = lambda P: math.sqrt(sum(float(_row_dot(P[0], P[1], r, x3D)) ** 2 for r in range(3)))
    z1 = _row_dot(R1, t1, 2, x3D)
    mg.x(z1, 0, cam_norm(P1))
    if z1 <= 0:
        return Z1, x3D, mg
    z2 = _row_dot(R2, t2, 2, x3D)
    mg.x(z2, 0, cam_norm(P2))
    if z2 <= 0:
        return Z2, x3D, mg
    if _reproj_fails(P1, cam, x3D, z1, x1, y1, ur1, sf1, mg):
        return REPROJ_1, x3D, mg
    if _reproj_fails(P2, cam, x3D, z2, x2, y2, ur2, sf2, mg):
        return REPROJ_2, x3D, mg
    n1 = [x3D[k] - Ow1[k] for k in range(3)]
    n2 = [x3D[k] - Ow2[k] for k in range(3)]
    dist1, dist2 = F(math.sqrt(dd(n1, n1))), F(math.sqrt(dd(n2, n2)))
    if dist1 == 0 or dist2 == 0:
        return ZERO_DIST, x3D, mg
    ratioDist, ratioOctave, rf = dist2 / dist1, sf1 / sf2, F(ratio_factor)
    mg.x(ratioDist * rf, ratioOctave)
    if ratioDist * rf < ratioOctave:
        return SCALE_RATIO, x3D, mg
    mg.x(ratioDist, ratioOctave * rf)
    if ratioDist > ratioOctave * rf:
        return SCALE_RATIO, x3D, mg
    return code, x3D, mg


def _unproject(P, u, v, z, cx, cy, invfx, invfy):
    """KeyFrame::UnprojectStereo (src/KeyFrame.cc:793-809): Rwc * x3Dc + Ow under C.12"""
    R, t, Ow = P
    x3Dc = [(u - cx) * z * invfx, (v - cy) * z * invfy, z]
    return [F(float(dot3_small([R[0][r], R[1][r], R[2][r]], x3Dc)) + float(Ow[r])) for r in range(3)]
