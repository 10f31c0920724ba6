"""Constructed frames for the key-frame step (tests/test_keyframe_cpu.py, tests/test_keyframe_gpu.py): small rows that hit every branch of the landmark
loops and of Tracking::NeedNewKeyFrame, their packing into the library's planes, and the expected planes from the line-by-line restatement
(tests/keyframe_reference.py).  Capacities: 512 key points and 256 key lines per frame, so a GPU test of the whole set takes well under a second."""
import functools
import numpy as np
import keyframe_reference as R
from orb_line_slam_amd._lib import KEYLINE_DTYPE, KEYPOINT_DTYPE
from orb_line_slam_amd.keyframe import ROW_FIELDS

F = np.float32
CAP, LCAP = 512, 256
FX, FY, CX, CY, MBF = 435.2047, 435.3, 367.4517, 252.2008, 47.90639384423901
TH = F(3.85)                                                         # mThDepth = mbf * ThDepth / fx with ThDepth = 35
CAM5 = (FX, FY, CX, CY, MBF)


def scale_factors(n=8):
    """mvScaleFactors of n levels at 1.2 as ORBextractor forms them: a double product of floats, rounded (src/ORBextractor.cc:419-425)"""
    sf = np.ones(n, F)
    for i in range(1, n):
        sf[i] = F(float(sf[i - 1]) * float(F(1.2)))
    return sf


SF = scale_factors()
N_MP, N_ML = 96, 48
MP_NOBS = np.array([(3 * k) % 4 for k in range(N_MP)], np.int32)     # Observations(): 0, 3, 2, 1, ...
ML_NOBS = np.array([(k + 1) % 3 for k in range(N_ML)], np.int32)


def camera(sf=SF):
    return R.Camera(FX, FY, CX, CY, MBF, TH, sf)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    """equal as bit patterns, NaN payloads aside"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _pose(rng):
    """a camera-to-world matrix: a rotation of a few degrees (rounded to float, so not exactly orthonormal) and a translation"""
    w = rng.uniform(-0.1, 0.1, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rm = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, rng.uniform(-2, 2, 3)
    return T.astype(F)


def _depths(rng, n, n_close):
    """n positive depths, n_close of them below TH, in random order, all distinct"""
    z = np.concatenate([rng.uniform(0.4, float(TH) * 0.98, n_close), rng.uniform(float(TH) * 1.02, float(TH) * 5, n - n_close)]).astype(F)
    rng.shuffle(z)
    return z


def _held(rng, n, n_map, outside_at=None):
    """mvpMapPoints: a third NULL, the rest indices into the map (whose Observations() are 0 for a quarter of them); outside_at: four features that hold
    an index outside the map"""
    h = rng.integers(0, n_map, n).astype(np.int32)
    h[rng.random(n) < 0.33] = -1
    if outside_at is not None:
        h[outside_at] = [n_map, n_map + 7, 2 ** 31 - 1, n_map + 1]
    return h


def make_frame(seed, depth, ldisp, held=None, held_l=None, octave=None):
    rng = np.random.default_rng(seed)
    depth, ldisp = np.asarray(depth, F).reshape(-1), np.asarray(ldisp, F).reshape(-1, 2)
    n, nl = len(depth), len(ldisp)
    keys = np.zeros(n, KEYPOINT_DTYPE)
    keys["x"], keys["y"] = rng.uniform(20, 1200, n).astype(F), rng.uniform(20, 360, n).astype(F)
    keys["octave"] = rng.integers(0, 8, n) if octave is None else octave
    keys["size"], keys["angle"], keys["class_id"] = 31, rng.uniform(0, 360, n).astype(F), -1
    kl = np.zeros(nl, KEYLINE_DTYPE)
    for f in ("startPointX", "endPointX"):
        kl[f] = rng.uniform(20, 1200, nl).astype(F)
    for f in ("startPointY", "endPointY"):
        kl[f] = rng.uniform(20, 360, nl).astype(F)
    kl["class_id"] = np.arange(nl)
    return R.Frame(keys, kl, depth, ldisp, _pose(rng), mp=held, ml=held_l, mp_nobs=MP_NOBS, ml_nobs=ML_NOBS)


def _ldisp(rng, nl, nl_close):
    """nl stereo lines, nl_close with both endpoint depths below TH; the farther endpoint is the start for about half of them"""
    far = np.concatenate([rng.uniform(0.5, float(TH) * 0.98, nl_close), rng.uniform(float(TH) * 1.02, float(TH) * 4, nl - nl_close)])
    near = far * rng.uniform(0.3, 0.99, nl)
    rng.shuffle(order := np.arange(nl))
    far, near = far[order], near[order]
    start_far = rng.random(nl) < 0.5
    sz, ez = np.where(start_far, far, near), np.where(start_far, near, far)
    return np.stack([MBF / sz, MBF / ez], 1).astype(F)


def _point_rows(rng):
    """(label, depth, held, octave) of the point halves"""
    rows = []
    for n in (0, 1, 100, 101, 102, 255, 256, 257, CAP):
        rows.append((f"count {n}", _depths(rng, n, n // 3), None, None))
    for nc in (99, 100, 101, 300, 0):
        rows.append((f"nClose {nc}", _depths(rng, 300, nc), _held(rng, 300, N_MP), None))
    z = _depths(rng, 300, 120)
    far = np.flatnonzero(z > TH)
    z[far[:3]] = TH                                                  # exactly mThDepth: not `> mThDepth`
    z[far[3:6]] = np.nextafter(TH, F(np.inf))                        # the next float above it
    rows.append(("depth == thDepth", z, None, None))
    z = _depths(rng, 140, 99)
    z[np.flatnonzero(z > TH)[0]] = TH                                # 99 close and one at the threshold: nClose = 100
    rows.append(("99 close and one at thDepth", z, _held(rng, 140, N_MP), None))
    # ties: 40 close, 50 distinct far ones, then 30 sharing one depth (sorted positions 90 .. 119: the break at position 100 falls inside), then larger ones
    z = np.concatenate([rng.uniform(0.5, 3.0, 40), rng.uniform(4.0, 5.0, 50), np.full(30, 6.25), rng.uniform(7.0, 9.0, 60)]).astype(F)
    rng.shuffle(z)
    rows.append(("ties across the break", z, _held(rng, len(z), N_MP), None))
    z = np.concatenate([np.full(60, 2.5), np.full(60, 2.75)]).astype(F)      # two blocks of close ties
    rows.append(("close ties", z, None, None))
    z = _depths(rng, 200, 50)
    z[[3, 50, 51, 120, 121, 199]] = [0.0, -0.0, -1.0, np.nan, np.inf, -np.inf]
    z[7] = np.inf
    rows.append(("z = 0, -0, negative, NaN, +-inf", z, None, None))
    z = _depths(rng, 300, 60)
    z[rng.random(300) < 0.2] = -1                                    # monocular points among them
    near = np.argsort(np.where(z > 0, z, np.inf))                    # two of the closest (visited) and two of the farthest (not visited)
    rows.append(("held entries, some outside the map", z, _held(rng, 300, N_MP, outside_at=[near[0], near[5], near[200], near[230]]), None))
    rows.append(("no stereo point", np.full(80, -1.0, F), None, None))
    rows.append(("count above the capacity", _depths(rng, CAP, 30), _held(rng, CAP, N_MP), None))      # (packed with a count of CAP + 88)
    octave = rng.integers(0, 8, 50)
    octave[[2, 9, 30]] = [8, -1, 1000]
    rows.append(("octave outside the levels", _depths(rng, 50, 20), None, octave))
    return rows


def _line_rows(rng):
    rows = []
    for nl in (0, 1, 50, 51, 52, 255, LCAP):
        rows.append((f"lcount {nl}", _ldisp(rng, nl, nl // 3), None))
    rows.append(("lcount above the capacity", _ldisp(rng, LCAP, 80), None))      # (packed with a count of LCAP + 44)
    for nc in (49, 50, 51, 150, 0):
        rows.append((f"line nClose {nc}", _ldisp(rng, 150, nc), _held(rng, 150, N_ML)))
    d = _ldisp(rng, 120, 30)
    d[0], d[1], d[2], d[3], d[4], d[5] = (-1, -1), (0.0, 9.0), (-0.0, 9.0), (9.0, -3.0), (9.0, 0.0), (-1, 12.0)
    d[6], d[7] = (0.0, 0.0), (np.inf, 5.0)                           # +inf depth at both ends; a depth of +0 at the start
    d[8], d[9] = (np.inf, np.inf), (-np.inf, -np.inf)                # depths of +0 and -0: -0 is not `< 0` and is kept; the two tie, the index decides
    rows.append(("line disparities -1, +0, -0, one negative", d, _held(rng, 120, N_ML)))
    d = _ldisp(rng, 90, 30)
    d[40] = (np.nan, 7.0)                                            # sz NaN, ez fine: z = ez, sorted as usual
    rows.append(("NaN start disparity", d, None))
    d = _ldisp(rng, 90, 30)
    d[41] = (7.0, np.nan)                                            # ez NaN: the sorted depth is NaN
    rows.append(("NaN line depth", d, _held(rng, 90, N_ML)))
    # ties: 20 close, 25 distinct far ones, 20 sharing one depth (sorted positions 45 .. 64 around the break at 50), then farther ones
    zs = np.concatenate([rng.uniform(0.5, 3.0, 20), rng.uniform(4.0, 5.0, 25), np.full(20, 6.5), rng.uniform(7.0, 9.0, 30)])
    rng.shuffle(zs)
    near = zs * rng.uniform(0.4, 0.9, len(zs))
    flip = rng.random(len(zs)) < 0.5
    d = np.stack([MBF / np.where(flip, zs, near), MBF / np.where(flip, near, zs)], 1).astype(F)
    tied = np.isclose(zs, 6.5)
    d[tied] = np.where(flip[tied, None], np.array([[MBF / 6.5, 20.0]]), np.array([[20.0, MBF / 6.5]])).astype(F)      # the same float at the far end
    rows.append(("line ties across the break", d, None))
    d = _ldisp(rng, 200, 40)
    near = np.argsort(MBF / d.min(1))
    rows.append(("held lines, some outside the map", d, _held(rng, 200, N_ML, outside_at=[near[1], near[7], near[150], near[190]])))
    rows.append(("stereo lines", _ldisp(rng, 80, 10), None))
    return rows


@functools.lru_cache(maxsize=None)
def scene_set():
    """the frames of the landmark tests, one per row: labels and Frames.  Row `no stereo point` carries stereo lines."""
    rng = np.random.default_rng(20241)
    prow, lrow = _point_rows(rng), _line_rows(rng)
    n = max(len(prow), len(lrow))
    labels, frames = [], []
    for k in range(n):
        pl, z, held, octave = prow[k % len(prow)]
        ll, d, held_l = lrow[k % len(lrow)]
        if pl == "no stereo point":
            ll, d, held_l = lrow[-1]
        labels.append(pl + " / " + ll)
        frames.append(make_frame(1000 + k, z, d, held, held_l, octave))
    return labels, frames


def counts_of(labels, frames):
    """N and N_l as the batch states them: beyond the capacity where the row says so"""
    c = np.array([fr.N for fr in frames], np.int32)
    lc = np.array([fr.N_l for fr in frames], np.int32)
    for k, lab in enumerate(labels):
        if lab.startswith("count above the capacity"):
            c[k] = CAP + 88
        if "lcount above the capacity" in lab:
            lc[k] = LCAP + 44
    return c, lc


def batch_arrays(frames, counts, lcounts, cap=CAP, lcap=LCAP, img_stride=1):
    """the planes of olf_landmarks_batch / olf_keyframe_test_batch for a list of frames; with img_stride 2 the odd images hold garbage"""
    n = len(frames)
    rng = np.random.default_rng(5)
    kps, kls = np.zeros((n * img_stride, cap), KEYPOINT_DTYPE), np.zeros((n * img_stride, lcap), KEYLINE_DTYPE)
    cnt, lcnt = np.full(n * img_stride, 7777, np.int32), np.full(n * img_stride, -5, np.int32)
    if img_stride > 1:
        kps["x"], kps["octave"] = 1e9, 99
        kls["startPointX"] = -1e9
    depth, ldisp = rng.uniform(0.5, 9.0, (n, cap)).astype(F), rng.uniform(1.0, 90.0, (n, lcap, 2)).astype(F)      # (garbage past the counts)
    Twc = np.zeros((n, 4, 4), F)
    fmp, fml = rng.integers(-1, N_MP, (n, cap)).astype(np.int32), rng.integers(-1, N_ML, (n, lcap)).astype(np.int32)
    for j, fr in enumerate(frames):
        q = j * img_stride
        kps[q] = 0
        kls[q] = 0
        kps[q, :fr.N], kls[q, :fr.N_l] = fr.keys, fr.klines
        cnt[q], lcnt[q] = counts[j], lcounts[j]
        depth[j, :fr.N], ldisp[j, :fr.N_l], Twc[j] = fr.depth, fr.ldisp, fr.Twc
        fmp[j, :fr.N] = -1 if fr.mp is None else fr.mp
        fml[j, :fr.N_l] = -1 if fr.ml is None else fr.ml
    return dict(kps=kps, counts=cnt, kls=kls, lcounts=lcnt, depth=depth, ldisp=ldisp, Twc=Twc, frame_mp=fmp, frame_ml=fml)


def expected(frames, mode, arrays, K, cap=CAP, lcap=LCAP, new_base_mp=None, new_base_ml=None, hold=True):
    """the planes of olf_landmarks_outputs from the restatement.  arrays: batch_arrays' planes (frame_mp / frame_ml give the entries past the count);
    hold False: the call passes no frame_mp / frame_ml."""
    n = len(frames)
    i32 = np.int32
    o = dict(n_visited=np.zeros((n, 2), i32), n_created=np.zeros((n, 2), i32), visit_order=np.full((n, cap), -1, i32), visit_order_l=np.full((n, lcap), -1, i32),
             created_order=np.full((n, cap), -1, i32), created_order_l=np.full((n, lcap), -1, i32), created=np.zeros((n, cap), np.uint8),
             created_l=np.zeros((n, lcap), np.uint8), frame_mp_out=arrays["frame_mp"].copy() if hold else np.full((n, cap), -1, i32),
             frame_ml_out=arrays["frame_ml"].copy() if hold else np.full((n, lcap), -1, i32), mp_world=np.zeros((n, cap, 3), F), mp_normal=np.zeros((n, cap, 3), F),
             mp_maxd=np.zeros((n, cap), F), mp_mind=np.zeros((n, cap), F), ml_world_d=np.zeros((n, lcap, 6), np.float64), ml_world=np.zeros((n, lcap, 6), F),
             status=np.zeros(n, i32))
    for j, fr in enumerate(frames):
        saved = fr.mp, fr.ml, fr.new_mp, fr.new_ml
        if not hold:
            fr.mp = fr.ml = None
        if new_base_mp is not None:
            fr.new_mp, fr.new_ml = int(new_base_mp[j]), int(new_base_ml[j])
        pts, lns, status = R.MODES[mode](fr, K)
        fr.mp, fr.ml, fr.new_mp, fr.new_ml = saved
        o["status"][j] = status
        for h, res, sfx, mp in ((0, pts, "", "frame_mp_out"), (1, lns, "_l", "frame_ml_out")):
            o["n_visited"][j, h], o["n_created"][j, h] = res.n_visited, len(res.created)
            o["visit_order" + sfx][j, :len(res.visit)] = res.visit
            o["created_order" + sfx][j, :len(res.created)] = res.created
            o["created" + sfx][j, res.created] = 1
            o[mp][j, :len(res.held)] = res.held
        for i, (Pos, normal, maxd, mind) in pts.geom.items():
            o["mp_world"][j, i], o["mp_normal"][j, i], o["mp_maxd"][j, i], o["mp_mind"][j, i] = Pos, normal, maxd, mind
        for i, w in lns.geom.items():
            o["ml_world_d"][j, i] = w
            o["ml_world"][j, i] = np.array(w, np.float64).astype(F)   # Converter::toCvMat: one rounding
    return o


# ---- Tracking::NeedNewKeyFrame ---------------------------------------------------------------------------------------------------------------------------
def _row(**kw):
    r = dict(mnId=100, mnLastKeyFrameId=90, mnLastRelocFrameId=0, mMinFrames=0, mMaxFrames=30, nKFs=5, bLocalMappingIdle=0, KeyframesInQueue=0, mbOnlyTracking=0,
             stopped=0, monocular=0, nRef=100, nRef_l=100, inl=80, inl_l=80)
    r.update(kw)
    assert set(r) == set(ROW_FIELDS) | {"nRef", "nRef_l", "inl", "inl_l"}
    return r


def designed_rows():
    """rows for a frame whose counts ask for nothing (bNeedToInsertClose false twice).  The base row has every condition false."""
    far = dict(mnLastKeyFrameId=60)                                  # c1a: 100 >= 60 + 30
    idle = dict(bLocalMappingIdle=1)                                 # c1b with mMinFrames 0
    rows = [_row(),
            _row(**far), _row(**idle), _row(inl=10), _row(inl_l=5), _row(inl=50), _row(inl_l=50),                       # each condition true alone
            _row(**idle, inl=20, inl_l=20), _row(**far, inl=20, inl_l=20), _row(**far, **idle, inl=50, inl_l=20),      # each false alone: c1a, c1b, c1c
            _row(**far, **idle, inl=20, inl_l=50), _row(**far, **idle, inl=10, inl_l=20), _row(**far, **idle, inl=20, inl_l=5)]      # c1c_l, c2, c2_l
    rows += [_row(**far, inl=50, nKFs=k) for k in (0, 1, 2, 3)]      # nMinObs does not enter here; thRefRatio 0.4 below two key frames: 50 < 40 fails
    rows += [_row(**far, inl=39, nKFs=1), _row(**far, inl=40, nKFs=1), _row(**far, inl=74, inl_l=39, nKFs=1)]
    # the comparisons at equality, and where float and double differ
    rows += [_row(inl=25), _row(inl=24), _row(**far, inl=75), _row(**far, inl=74)]
    rows += [_row(nRef=67108865, inl=16777216),                      # 0.25 in double: 16777216 < 16777216.25 (in float both sides are 16777216)
             _row(**far, nRef=33554433, inl=25165824),               # 0.75f in float: 25165824 < 25165824 fails (in double: < 25165824.75)
             _row(**far, nRef=33554433, inl=25165823), _row(**far, nRef_l=33554433, inl_l=25165824, inl=80)]
    # the branch that is not idle, queue lengths 2 and 3; monocular; the early returns; unsigned wrap
    rows += [_row(**far, inl=50, KeyframesInQueue=2), _row(**far, inl=50, KeyframesInQueue=3), _row(**far, inl=50, KeyframesInQueue=2, monocular=1),
             _row(**far, **idle, inl=50, monocular=1), _row(**far, inl=85, monocular=1, **idle), _row(**far, **idle, inl=50, mbOnlyTracking=1),
             _row(**far, **idle, inl=50, stopped=1), _row(**far, **idle, inl=50, mnLastRelocFrameId=80, nKFs=31), _row(**far, **idle, inl=50, mnLastRelocFrameId=80, nKFs=30),
             _row(**idle, inl=50, mnLastKeyFrameId=0xfffffff0), _row(**idle, inl=50, mnId=10, mnLastKeyFrameId=0xfffffff0, mMinFrames=20),
             _row(**idle, inl=50, mnId=3, mnLastKeyFrameId=0xfffffff0, mMinFrames=20), _row(**idle, inl=50, mnLastRelocFrameId=0xffffffff, nKFs=40)]
    return rows


@functools.lru_cache(maxsize=None)
def keyframe_scene():
    """(frames, rows, outlier, outlier_l): the designed rows on a quiet frame, then every frame of the landmark set under rows that let the counts decide"""
    rng = np.random.default_rng(77)
    quiet = make_frame(900, _depths(rng, 120, 30), _ldisp(rng, 70, 20), _held(rng, 120, N_MP), _held(rng, 70, N_ML))
    rows = designed_rows()
    frames = [quiet] * len(rows)
    _, lm = scene_set()
    for k, fr in enumerate(lm):
        frames.append(fr)
        rows.append(_row(bLocalMappingIdle=k & 1, inl=80 if k % 3 else 20, inl_l=80 if k % 4 else 20, KeyframesInQueue=k % 5, nKFs=k % 4))
    # many untracked close lines and few tracked ones: bNeedToInsertClose_l
    frames.append(make_frame(901, _depths(rng, 300, 200), _ldisp(rng, 240, 200), None, np.where(np.arange(240) < 10, 3, -1)))
    rows.append(_row(inl=20, inl_l=20))
    frames.append(make_frame(902, _depths(rng, 300, 200), _ldisp(rng, 240, 200), _held(rng, 300, N_MP), _held(rng, 240, N_ML)))
    rows.append(_row(bLocalMappingIdle=1, inl=20, inl_l=20))
    outlier = [rng.random(fr.N) < 0.25 if j % 2 else None for j, fr in enumerate(frames)]
    outlier_l = [rng.random(fr.N_l) < 0.25 if j % 3 else None for j, fr in enumerate(frames)]
    return frames, rows, outlier, outlier_l


def keyframe_arrays(frames, rows, outlier, outlier_l, cap=CAP, lcap=LCAP, img_stride=1):
    n = len(frames)
    a = batch_arrays(frames, [fr.N for fr in frames], [fr.N_l for fr in frames], cap, lcap, img_stride)
    out, out_l = np.zeros((n, cap), np.uint8), np.zeros((n, lcap), np.uint8)
    for j, fr in enumerate(frames):
        if outlier[j] is not None:
            out[j, :fr.N] = outlier[j]
        if outlier_l[j] is not None:
            out_l[j, :fr.N_l] = outlier_l[j]
    a.update(outlier=out, outlier_l=out_l, rows=[{k: r[k] for k in ROW_FIELDS} for r in rows], n_ref_matches=np.array([r["nRef"] for r in rows], np.int32),
             n_ref_matches_l=np.array([r["nRef_l"] for r in rows], np.int32), n_inliers=np.array([[r["inl"], r["inl_l"]] for r in rows], np.int32))
    return a


def keyframe_expected(frames, rows, outlier, outlier_l, K, ldisp_frame=None):
    n = len(frames)
    o = dict(need=np.zeros(n, np.uint8), interrupt_ba=np.zeros(n, np.uint8), counts=np.zeros((n, 4), np.int32), conditions=np.zeros(n, np.int32),
             status=np.zeros(n, np.int32))
    for j, (fr, r) in enumerate(zip(frames, rows)):
        lf = j if ldisp_frame is None else int(ldisp_frame[j])
        last = frames[lf] if 0 <= lf < n else None
        res = R.need_new_keyframe(r, fr, outlier[j], outlier_l[j], last.ldisp if last is not None else [], last.N_l if last is not None else 0, K, r["nRef"], r["nRef_l"],
                                  r["inl"], r["inl_l"])
        o["need"][j], o["interrupt_ba"][j], o["counts"][j], o["conditions"][j], o["status"][j] = res
    return o
