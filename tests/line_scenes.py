"""Scenes and expectations shared by test_line_track_cpu.py and test_line_batch_gpu.py: the line half of tracking -- Frame::isInFrustum_l
(src/Frame.cc:446-515), the line half of Tracking::SearchLocalPointsAndLines (src/Tracking.cc:1897-1913, :1945-2023) and the f2f line tracking of
TrackWithMotionModelWithLine (:1305-1349) / TrackReferenceKeyFrameWithLine (:976-1020).

Where the expectations come from:
  - end point projections: oracle.is_in_frustum on each end point with the point-only gates neutralised (mind = 0, maxd = 1e30, viewing_cos_limit = -2, a
    unit normal): its in_view and proj3[:, :2] are one half of isInFrustum_l;
  - matches_12 before the loops: oracle.match_bf (a frame with fewer than two lines: all -1, the project's convention for the reference's out-of-range read);
  - the loops :1976-2016, :1315-1349, :987-1020: restated below as plain sequential Python over np.float32 / np.float64 scalars, line for line.
Frames are synthetic, 320 x 240, no extractor.  Nothing here touches a device."""
import numpy as np
import orb_line_slam_amd as ola
from orb_line_slam_amd._lib import KEYLINE_DTYPE, KEYPOINT_DTYPE

W, H = 320, 240
FX = FY = 200.0
CX, CY, MBF = 160.0, 120.0, 40.0
CAM = (FX, FY, CX, CY, MBF)
BOUNDS = (0.0, 320.0, 0.0, 240.0)
NNR = 0.75
f32, f64 = np.float32, np.float64
SF8 = np.ones(8, f32)
for _i in range(1, 8):
    SF8[_i] = f32(SF8[_i - 1] * f32(1.2))


def pose(tx=0.0, ty=0.0, tz=0.0, ry_deg=0.0, rx_deg=0.0):
    T = np.eye(4)
    a, b = np.deg2rad(ry_deg), np.deg2rad(rx_deg)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T[:3, :3] = Ry @ Rx
    T[:3, 3] = [tx, ty, tz]
    return T


def flip(rng, desc, k):
    d = desc.copy()
    for r in range(len(d)):
        for b in rng.choice(256, k, replace=False):
            d[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def project(Tcw, P):
    Xc = np.asarray(P, f64) @ Tcw[:3, :3].astype(f64).T + Tcw[:3, 3].astype(f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return FX * Xc[:, 0] / Xc[:, 2] + CX, FY * Xc[:, 1] / Xc[:, 2] + CY, Xc[:, 2]


def keylines(sx, sy, ex, ey):
    k = np.zeros(len(sx), KEYLINE_DTYPE)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = sx, sy, ex, ey
    k["sPointInOctaveX"], k["sPointInOctaveY"], k["ePointInOctaveX"], k["ePointInOctaveY"] = sx, sy, ex, ey
    k["angle"] = np.arctan2(k["endPointY"].astype(f64) - k["startPointY"], k["endPointX"].astype(f64) - k["startPointX"])
    k["pt_x"], k["pt_y"] = (k["startPointX"] + k["endPointX"]) / 2, (k["startPointY"] + k["endPointY"]) / 2
    k["lineLength"] = np.hypot(k["endPointX"] - k["startPointX"], k["endPointY"] - k["startPointY"])
    k["class_id"] = np.arange(len(sx))
    k["response"], k["size"], k["numOfPixels"] = 1.0, 1.0, 10
    return k


class LineFrame:
    """kls / ldesc / ldisp of a frame's lines, its pose, mvpMapLines on entry (map indices, -1 none)"""

    def view(self, bounds=BOUNDS):
        return ola.FrameView(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), None, SF8, FX, FY, CX, CY, MBF, bounds, mTcw=self.Tcw)


class LineMap:
    pass


def segments(rng, n, margin=25.0):
    """n 3-D segments that project inside the image of the identity pose, margin pixels from its border"""
    z = rng.uniform(4, 20, (n, 2))
    z[:, 1] = z[:, 0] + rng.uniform(-0.5, 0.5, n)
    u0, v0 = rng.uniform(margin, W - margin, n), rng.uniform(margin, H - margin, n)
    ang, ln = rng.uniform(-np.pi, np.pi, n), rng.uniform(12, 40, n)
    u1 = np.clip(u0 + ln * np.cos(ang), margin, W - margin)
    v1 = np.clip(v0 + ln * np.sin(ang), margin, H - margin)
    s = np.stack([(u0 - CX) * z[:, 0] / FX, (v0 - CY) * z[:, 0] / FY, z[:, 0]], 1)
    e = np.stack([(u1 - CX) * z[:, 1] / FX, (v1 - CY) * z[:, 1] / FY, z[:, 1]], 1)
    return np.concatenate([s, e], 1)


def local_scene(seed, line_counts=(300, 70, 33, 1, 0), n_base=234, bounds=BOUNDS, behind=0):
    """5 frames and a map of 3 * n_base lines: every base line twice more, the copies 0 or 2 descriptor bits away, a quarter of the copies displaced so
    that their projection is more than 0.1 of the bounds away (several ranks target one frame line and differ at the position gate).  A frame's lines
    re-observe base lines under its pose with 4 flipped bits and up to 2 pixels of jitter, some of them moved by more than 0.1 of the bounds; the rest
    are distractors.  obs about half, some lines bad, some ldisp -1; frames hold lines on entry, with and without observations, a bad one among them."""
    rng = np.random.default_rng(seed)
    base = segments(rng, n_base)
    world = [base]
    desc0 = rng.integers(0, 256, (n_base, 32), dtype=np.uint8)
    desc = [desc0]
    for c in range(2):
        w = base.copy()
        moved = rng.random(n_base) < 0.25
        w[moved, 0] += 0.25 * w[moved, 2]                    # + 50 pixels in u for both end points
        w[moved, 3] += 0.25 * w[moved, 5]
        d = desc0.copy()
        two = (rng.random(n_base) < 0.5) | (c == 1)
        d[two] = flip(rng, desc0[two], 2)
        world.append(w); desc.append(d)
    mp = LineMap()
    mp.world = np.ascontiguousarray(np.concatenate(world), f32)
    mp.desc = np.ascontiguousarray(np.concatenate(desc))
    mp.n = len(mp.world)
    if behind:                                               # an end point behind the camera: the start of some, the end of others
        k = rng.choice(mp.n, behind, replace=False)
        mp.world[k[: behind // 2], 2] *= -1
        mp.world[k[behind // 2:], 5] *= -1
    mp.obs = rng.random(mp.n) < 0.5
    mp.bad = rng.random(mp.n) < 0.05
    mp.n_base = n_base
    poses = [pose(), pose(tx=0.05, ty=-0.03, tz=0.1, ry_deg=1.0), pose(tx=-0.08, tz=0.05, rx_deg=-1.0), pose(ty=0.04, ry_deg=-1.5), pose(tx=0.1, rx_deg=0.8)]
    frames = []
    for j, n in enumerate(line_counts):
        fr = LineFrame()
        fr.Tcw = poses[j].astype(f32)
        su, sv, sz = project(fr.Tcw, base[:, :3])
        eu, ev, ez = project(fr.Tcw, base[:, 3:])
        ok = np.flatnonzero((sz > 0.5) & (ez > 0.5) & (np.minimum(su, eu) > 4) & (np.maximum(su, eu) < W - 4) & (np.minimum(sv, ev) > 4) & (np.maximum(sv, ev) < H - 4))
        m = min(int(n * 0.9), len(ok)) if n > 1 else n
        src = rng.choice(ok, m, replace=False)
        jit = lambda a: a[src] + rng.uniform(-2, 2, m)
        sx, sy, ex, ey = jit(su), jit(sv), jit(eu), jit(ev)
        far = rng.random(m) < 0.06                           # the position gate rejects these: 40 pixels > 0.1 * 320
        sx[far] += 40.0; ex[far] += 40.0
        nd = n - m
        dsx, dsy = rng.uniform(10, W - 10, nd), rng.uniform(10, H - 10, nd)
        k = keylines(np.concatenate([sx, dsx]), np.concatenate([sy, dsy]), np.concatenate([ex, dsx + rng.uniform(-30, 30, nd)]),
                     np.concatenate([ey, dsy + rng.uniform(-30, 30, nd)]))
        d = np.concatenate([flip(rng, desc0[src], 4), rng.integers(0, 256, (nd, 32), dtype=np.uint8)])
        held = np.full(n, -1, np.int32)
        h = rng.random(m) < 0.2                              # a fifth of the re-observations hold their line or one of its copies on entry
        held[:m][h] = src[h] + n_base * rng.integers(0, 3, int(h.sum()))
        perm = rng.permutation(n)
        fr.kls, fr.ldesc, fr.frame_ml = k[perm], np.ascontiguousarray(d[perm]), held[perm]
        fr.ldisp = np.where(rng.random((n, 2)) < 0.05, -1.0, rng.uniform(0.5, 30, (n, 2))).astype(f32)
        fr.src = src
        frames.append(fr)
    hb = [i for fr in frames for i in fr.frame_ml if i >= 0]
    mp.bad[hb[::7]] = True                                   # held lines that are bad: dropped from their frame line first (:1902-1905)
    mp.obs[hb[1::2]] = True
    mp.obs[hb[0::2]] = False
    mp.bounds = bounds
    return frames, mp


def lists_for(oracle, rng, frames, mp, want):
    """per frame a list of map indices with exactly want[j] lines in view -- the lines the frame re-observes first -- plus up to 37 lines that are skipped or
    out of view, in random order.  None: every line, permuted; -1: an empty list; 0: only lines that are not in view"""
    lists = []
    for fr, w in zip(frames, want):
        if w is None:
            lists.append(rng.permutation(mp.n).astype(np.int32))
            continue
        if w < 0:
            lists.append(np.zeros(0, np.int32))
            continue
        inv = expect_frustum_frame(oracle, fr, mp, np.arange(mp.n), fr.frame_ml)[0]
        yes, no = np.flatnonzero(inv), np.flatnonzero(~inv)
        assert len(yes) >= w, (len(yes), w)
        seen = np.isin(yes % mp.n_base, fr.src)
        yes = np.concatenate([rng.permutation(yes[seen]), rng.permutation(yes[~seen])])
        pick = np.concatenate([yes[:w], rng.choice(no, min(len(no), 37), replace=False)])
        lists.append(rng.permutation(pick).astype(np.int32))
    return lists


# ---- expectations ----------------------------------------------------------------------------------------------------------------------------------
def endpoint_views(oracle, fr, world6, bounds):
    """(ok, uv) of the start points and of the end points: oracle.is_in_frustum with the point-only gates neutralised"""
    n = len(world6)
    v = fr.view(bounds)
    out = []
    for k in (0, 3):
        nrm = np.tile(np.array([0, 0, 1], f32), (n, 1))
        geom = ola.MapPointGeom(world6[:, k:k + 3], nrm, np.full(n, 1e30, f32), np.zeros(n, f32), np.zeros((n, 32), np.uint8))
        inv, _, _, proj = oracle.is_in_frustum(v, geom, -2.0)
        out.append((inv, proj[:, :2].copy()))
    return out


def expect_is_in_frustum_l(oracle, fr, world6, bounds=BOUNDS):
    """Frame::isInFrustum_l: (in_view, proj4); rows not in view are zero"""
    (so, suv), (eo, euv) = endpoint_views(oracle, fr, np.ascontiguousarray(world6, f32), bounds)
    inv = so & eo
    proj4 = np.concatenate([suv, euv], 1).astype(f32)
    proj4[~inv] = 0
    return inv, proj4


def prepass(mp, frame_ml):
    """mvpMapLines without its bad lines (src/Tracking.cc:1897-1913); a value outside the map holds nothing"""
    fm = np.asarray(frame_ml, np.int64).copy()
    fm[(fm < 0) | (fm >= mp.n)] = -1
    live = fm >= 0
    fm[live] = np.where(mp.bad[fm[live]], -1, fm[live])
    return fm


def expect_frustum_frame(oracle, fr, mp, lst, frame_ml):
    """(in_view, proj4) over a frame's list with the two skips of :1953-1956; an index outside the map is left out"""
    lst = np.asarray(lst, np.int64)
    valid = (lst >= 0) & (lst < mp.n)
    safe = np.where(valid, lst, 0)
    inv, proj4 = expect_is_in_frustum_l(oracle, fr, mp.world[safe], mp.bounds)
    held = np.zeros(mp.n, bool)
    fm = prepass(mp, frame_ml)
    held[fm[fm >= 0]] = True
    inv = inv & valid & ~held[safe] & ~mp.bad[safe]
    proj4[~inv] = 0
    return inv, proj4


def loop_local(m12, map_index, proj4, kls, ldisp, bounds, frame_ml, obs):
    """src/Tracking.cc:1974-2016 and :2021-2023, line for line.  m12 and frame_ml are updated in place; returns n_inliers_ls"""
    mnMinX, mnMaxX, mnMinY, mnMaxY = (f32(b) for b in bounds)
    deltaWidth = f64(f32(mnMaxX - mnMinX)) * f64(0.1)                                               # :1974
    deltaHeight = f64(f32(mnMaxY - mnMinY)) * f64(0.1)                                              # :1975
    for i1 in range(len(m12)):                                                                      # :1976
        i2 = int(m12[i1])                                                                           # :1977
        if i2 < 0:                                                                                  # :1978
            continue
        if ldisp[i2][0] < 0 or ldisp[i2][1] < 0:                                                    # :1979
            continue
        if frame_ml[i2] >= 0:                                                                       # :1981
            if obs[frame_ml[i2]]:                                                                   # :1982
                continue                                                                            # :1983
        pML = int(map_index[i1])                                                                    # :1986
        sX_curr, sX_last = f32(kls[i2]["startPointX"]), f32(proj4[i1][0])                           # :2000-2001
        sY_curr, sY_last = f32(kls[i2]["startPointY"]), f32(proj4[i1][1])                           # :2002-2003
        eX_curr, eX_last = f32(kls[i2]["endPointX"]), f32(proj4[i1][2])                             # :2004-2005
        eY_curr, eY_last = f32(kls[i2]["endPointY"]), f32(proj4[i1][3])                             # :2006-2007
        if (f64(abs(f32(sX_curr - sX_last))) > deltaWidth or f64(abs(f32(eX_curr - eX_last))) > deltaWidth or
                f64(abs(f32(sY_curr - sY_last))) > deltaHeight or f64(abs(f32(eY_curr - eY_last))) > deltaHeight):      # :2008
            m12[i1] = -1                                                                            # :2010
            continue                                                                                # :2011
        frame_ml[i2] = pML                                                                          # :2015
    return int(np.count_nonzero(np.asarray(frame_ml) >= 0))                                          # :2021-2023


def match_nnr(oracle, dq, dt, nnr, best_lr=False):
    if len(dq) == 0:
        return np.zeros(0, np.int32)
    if len(dt) < 2 or (best_lr and len(dq) < 2):
        return np.full(len(dq), -1, np.int32)
    return oracle.match_bf(dq, dt, nnr, best_lr=best_lr)


def expect_local_frame(oracle, fr, mp, lst, frame_ml, nnr=NNR):
    """everything olf_search_local_lines_batch_dev returns for one frame, over the frame's list: dict(in_view, proj4, m12 per entry, frame_ml, n_inliers)
    plus what the floors are counted from: m12_before, ranks (list positions in view)"""
    lst = np.asarray(lst, np.int64)
    inv, proj4 = expect_frustum_frame(oracle, fr, mp, lst, frame_ml)
    ranks = np.flatnonzero(inv)
    midx = lst[ranks]
    before = match_nnr(oracle, mp.desc[midx], fr.ldesc, nnr)
    m12 = before.copy()
    fm0 = prepass(mp, frame_ml)
    fm = fm0.copy()
    n = loop_local(m12, midx, proj4[ranks], fr.kls, fr.ldisp, mp.bounds, fm, mp.obs)
    per_entry = np.full(len(lst), -1, np.int32)
    per_entry[ranks] = m12
    return dict(in_view=inv, proj4=proj4, m12=per_entry, frame_ml=fm.astype(np.int32), n_inliers=n, m12_before=before, m12_after=m12, midx=midx, frame_ml0=fm0,
                proj4_rank=proj4[ranks])


def local_floors(fr, mp, exp):
    """the cases of the loop an expectation exercises, counted on the expectation alone"""
    out = dict(blocked=0, first_obs_wins=0, last_unobserved_wins=0, fail_before_f=0, fail_after_f_kept=0, disparity_skip=0,
               assigned=int(np.count_nonzero(exp["frame_ml"] != exp["frame_ml0"])))
    before, after, midx = exp["m12_before"], exp["m12_after"], exp["midx"]
    dW, dH = 0.1 * (mp.bounds[1] - mp.bounds[0]), 0.1 * (mp.bounds[3] - mp.bounds[2])
    for i2 in range(len(fr.kls)):
        t = np.flatnonzero(before == i2)
        if len(t) == 0:
            continue
        if fr.ldisp[i2][0] < 0 or fr.ldisp[i2][1] < 0:
            out["disparity_skip"] += len(t)
            continue
        h = exp["frame_ml0"][i2]
        if h >= 0 and mp.obs[h]:
            out["blocked"] += 1
            continue
        k, p = fr.kls[i2], exp["proj4_rank"][t].astype(f64)
        ok = ((abs(k["startPointX"] - p[:, 0]) <= dW) & (abs(k["endPointX"] - p[:, 2]) <= dW) & (abs(k["startPointY"] - p[:, 1]) <= dH) &
              (abs(k["endPointY"] - p[:, 3]) <= dH))
        fo = [r for r, o in zip(t, ok) if o and mp.obs[midx[r]]]
        if fo:
            f = fo[0]
            out["first_obs_wins"] += int(any(o and r > f for r, o in zip(t, ok)))
            out["fail_before_f"] += int(any((not o) and r < f and after[r] == -1 for r, o in zip(t, ok)))
            out["fail_after_f_kept"] += int(any((not o) and r > f and after[r] == i2 for r, o in zip(t, ok)))
        elif ok.sum() >= 2:
            out["last_unobserved_wins"] += int(exp["frame_ml"][i2] == midx[t[ok][-1]])
    return out


# ---- f2f -------------------------------------------------------------------------------------------------------------------------------------------
def f2f_scene(seed, n_frames=4, n=120):
    """frames whose lines re-observe the previous frame's under a shift of a few pixels with 4 flipped bits; a tenth of a frame's lines are listed twice
    (several i1 -> one i2 without the mutual check); some lines are moved by more than 0.1 of the bounds or turned by more than pi / 8; some pairs of
    angles straddle +-pi; ids of the last frame about half NULL; some ldisp -1"""
    rng = np.random.default_rng(seed)
    frames = []
    sx, sy = rng.uniform(30, W - 30, n), rng.uniform(30, H - 30, n)
    ang, ln = rng.uniform(-np.pi, np.pi, n), rng.uniform(15, 40, n)
    ang[:12] = np.pi - rng.uniform(0.001, 0.05, 12)          # just below +pi: a small turn takes the next frame's angle to just above -pi
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for j in range(n_frames):
        fr = LineFrame()
        a = ang + rng.uniform(-0.03, 0.03, n) + (0.08 if j else 0.0) * (np.arange(n) < 12)
        turned = rng.random(n) < 0.08
        a = a + turned * 0.6                                 # > pi / 8
        x, y = sx + rng.uniform(-3, 3, n), sy + rng.uniform(-3, 3, n)
        far = rng.random(n) < 0.08
        x = x + far * 40.0
        k = keylines(x, y, x + ln * np.cos(a), y + ln * np.sin(a))
        d = flip(rng, desc, 4) if j else desc.copy()
        dup = rng.choice(n, n // 10, replace=False)
        k, d = np.concatenate([k, k[dup]]), np.concatenate([d, d[dup]])
        nd = 15
        dx, dy = rng.uniform(10, W - 10, nd), rng.uniform(10, H - 10, nd)
        k = np.concatenate([k, keylines(dx, dy, dx + rng.uniform(-30, 30, nd), dy + rng.uniform(-30, 30, nd))])
        d = np.concatenate([d, rng.integers(0, 256, (nd, 32), dtype=np.uint8)])
        perm = rng.permutation(len(k))
        fr.kls, fr.ldesc = k[perm], np.ascontiguousarray(d[perm])
        fr.ldisp = np.where(rng.random((len(k), 2)) < 0.08, -1.0, rng.uniform(0.5, 30, (len(k), 2))).astype(f32)
        fr.ml = np.where(rng.random(len(k)) < 0.5, -1, rng.integers(0, 100000, len(k))).astype(np.int32)
        frames.append(fr)
    return frames


def loop_f2f(m12, kls_last, last_ml, kls_cur, ldisp_cur, bounds, skip_null, gates, delta_angle, pos_frac, n_cur):
    """src/Tracking.cc:1306-1349 (skip_null, gates) and :977-1020 (neither), line for line; returns (mvpMapLines of the current frame, n_inliers_ls)"""
    M_PI = f64(np.pi)
    cur_ml = np.full(n_cur, -1, np.int32)                                                           # :1306 / :977
    mnMinX, mnMaxX, mnMinY, mnMaxY = (f32(b) for b in bounds)
    deltaAngle = f64(delta_angle)                                                                   # :1310
    deltaWidth = f64(f32(mnMaxX - mnMinX)) * f64(pos_frac)                                          # :1311
    deltaHeight = f64(f32(mnMaxY - mnMinY)) * f64(pos_frac)                                         # :1312
    n_inliers_ls = 0                                                                                # :1313
    for i1 in range(len(m12)):                                                                      # :1315
        if skip_null and last_ml[i1] < 0:                                                           # :1316
            continue
        i2 = int(m12[i1])                                                                           # :1317
        if i2 < 0:                                                                                  # :1318
            continue
        if ldisp_cur[i2][0] < 0 or ldisp_cur[i2][1] < 0:                                            # :1319
            continue
        if gates:                                                                                   # :1322 `if(true)` / :993 `if(false)`
            theta = f64(f32(f32(kls_cur[i2]["angle"]) - f32(kls_last[i1]["angle"])))                # :1324
            if theta < -M_PI:                                                                       # :1325
                theta = theta + f64(2) * M_PI
            elif theta > M_PI:                                                                      # :1326
                theta = theta - f64(2) * M_PI
            if abs(theta) > deltaAngle:                                                             # :1327
                m12[i1] = -1                                                                        # :1328
                continue
            c, l = kls_cur[i2], kls_last[i1]
            if (f64(abs(f32(f32(c["startPointX"]) - f32(l["startPointX"])))) > deltaWidth or f64(abs(f32(f32(c["endPointX"]) - f32(l["endPointX"])))) > deltaWidth or
                    f64(abs(f32(f32(c["startPointY"]) - f32(l["startPointY"])))) > deltaHeight or
                    f64(abs(f32(f32(c["endPointY"]) - f32(l["endPointY"])))) > deltaHeight):          # :1340
                m12[i1] = -1                                                                        # :1342
                continue
        cur_ml[i2] = last_ml[i1] if last_ml[i1] >= 0 else -1                                        # :1347 / :1018
        n_inliers_ls += 1                                                                           # :1348
    return cur_ml, n_inliers_ls


def expect_f2f_pair(oracle, last, cur, nnr, best_lr, skip_null, gates, delta_angle=np.pi / 8.0, pos_frac=0.1, bounds=BOUNDS):
    before = match_nnr(oracle, last.ldesc, cur.ldesc, nnr, best_lr)
    m12 = before.copy()
    cur_ml, n = loop_f2f(m12, last.kls, last.ml, cur.kls, cur.ldisp, bounds, skip_null, gates, delta_angle, pos_frac, len(cur.kls))
    return dict(m12=m12, m12_before=before, cur_ml=cur_ml, n_inliers=n)


# ---- the cases both test files run --------------------------------------------------------------------------------------------------------------------
# line_counts: lines per frame (the train tile of the kNN is 32 rows: 33 and 70 leave a remainder; 0 and 1 match nothing).  want: lines in view per frame
# through the frame's list (lists_for) -- 256 and 257 sit on either side of the kNN's query tile; "no_lists": list_offsets = NULL.
LOCAL_CASES = {
    "lists_a": dict(seed=11, line_counts=(300, 70, 33, 1, 0), want=(None, 257, 256, 1, -1)),
    "lists_b": dict(seed=12, line_counts=(300, 70, 1, 0, 33), want=(0, None, 256, 257, 1)),
    "no_lists": dict(seed=13, line_counts=(300, 70, 33, 1, 0), want=None),
    "shrunk": dict(seed=14, line_counts=(300, 70, 33, 1, 0), want=None, bounds=(60.0, 260.0, 50.0, 190.0), behind=40),
}
LOOP_FLOORS = ("blocked", "first_obs_wins", "last_unobserved_wins", "fail_before_f", "fail_after_f_kept", "disparity_skip")
_cache = {}


def local_case(oracle, name):
    """(frames, map, lists or None, [expectation per frame]) of a case, built once"""
    if name not in _cache:
        c = LOCAL_CASES[name]
        frames, mp = local_scene(c["seed"], c["line_counts"], bounds=c.get("bounds", BOUNDS), behind=c.get("behind", 0))
        lists = None if c["want"] is None else lists_for(oracle, np.random.default_rng(c["seed"] + 100), frames, mp, c["want"])
        exp = [expect_local_frame(oracle, fr, mp, np.arange(mp.n) if lists is None else lists[j], fr.frame_ml) for j, fr in enumerate(frames)]
        _cache[name] = (frames, mp, lists, exp)
    return _cache[name]


def frustum_gate_counts(oracle, fr, mp):
    """which gate rejects a map line first, from the oracle's end point projections under open bounds: counts for behind_s, behind_e and the eight
    bounds gates (s_minX, s_maxX, s_minY, s_maxY, e_...)"""
    wide = (-1e30, 1e30, -1e30, 1e30)
    (so, suv), (eo, euv) = endpoint_views(oracle, fr, mp.world, wide)
    b = mp.bounds
    out = {}
    alive = np.ones(mp.n, bool)
    for tag, ok, uv in (("s", so, suv), ("e", eo, euv)):
        out["behind_" + tag] = int(np.count_nonzero(alive & ~ok))
        alive = alive & ok
        for name, rej in (("minX", uv[:, 0] < f32(b[0])), ("maxX", uv[:, 0] > f32(b[1])), ("minY", uv[:, 1] < f32(b[2])), ("maxY", uv[:, 1] > f32(b[3]))):
            out[tag + "_" + name] = int(np.count_nonzero(alive & rej))      # (in the reference's order: a line rejected at one gate never reaches the next)
            alive = alive & ~rej
    return out


F2F_MODES = {
    # Tracking::TrackWithMotionModelWithLine (:1305-1349) and TrackReferenceKeyFrameWithLine (:976-1020; 0.3 is formed, the gates never read it)
    "motion_model": dict(skip_null=True, gates=True, delta_angle=np.pi / 8.0, pos_frac=0.1),
    "reference_kf": dict(skip_null=False, gates=False, delta_angle=np.pi / 8.0, pos_frac=0.3),
    "gates_keep_null": dict(skip_null=False, gates=True, delta_angle=np.pi / 8.0, pos_frac=0.1),
    "skip_null_no_gates": dict(skip_null=True, gates=False, delta_angle=np.pi / 8.0, pos_frac=0.3),
}


def f2f_case(oracle, mode, best_lr, seed=21):
    key = ("f2f", mode, best_lr, seed)
    if key not in _cache:
        frames = _cache.setdefault(("f2f_scene", seed), f2f_scene(seed))
        _cache[key] = (frames, [expect_f2f_pair(oracle, frames[j], frames[j + 1], NNR, best_lr, **F2F_MODES[mode]) for j in range(len(frames) - 1)])
    return _cache[key]


def f2f_floors(frames, exp, mode):
    """counted on the expectation: several i1 that take one i2, assignments, gate rejections, an accepted pair of angles on either side of +-pi, NULL ids"""
    out = dict(shared_i2=0, assigned=0, gate_rejected=0, straddle_kept=0, null_assigned=0, null_skipped=0)
    m = F2F_MODES[mode]
    for j, e in enumerate(exp):
        last, cur = frames[j], frames[j + 1]
        kept = np.flatnonzero(e["m12"] >= 0)
        took = [i1 for i1 in kept if not (m["skip_null"] and last.ml[i1] < 0) and not (cur.ldisp[e["m12"][i1]] < 0).any()]
        tgt = e["m12"][took]
        out["assigned"] += len(took)
        out["shared_i2"] += int(len(tgt) - len(np.unique(tgt)))
        out["gate_rejected"] += int(np.count_nonzero((e["m12_before"] >= 0) & (e["m12"] < 0)))
        out["straddle_kept"] += int(sum(abs(float(cur.kls[e["m12"][i1]]["angle"]) - float(last.kls[i1]["angle"])) > np.pi for i1 in took))
        out["null_assigned"] += int(sum(last.ml[i1] < 0 for i1 in took))
        out["null_skipped"] += int(np.count_nonzero((e["m12"] >= 0) & (last.ml < 0))) if m["skip_null"] else 0
    return out
