"""GPU parity: olf_fuse_search_batch_dev -- the search part of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:827-948,
LocalMapping::SearchInNeighbors) and of Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:977-1102, LoopClosing::SearchAndFuse) for a batch of key frames
on the device.  Every expectation comes from the CPU oracle key frame by key frame (oracle.fuse_search / oracle.fuse_search_sim3); equality is exact
on best_idx, best_dist and nfused.  Every scenario_* builder asserts, from the oracle's output or a numpy count and without a GPU, that its case really
occurs, so that no test can pass by having nothing to compare.
Key frames are fabricated (no extractor): 320 x 240, fx = fy = 200, mbf = 40, eight levels of 1.2; a batch holds key frames of (0, 1, 63, 64, 65, 300)
key points plus one of 900, against a map of 400 points."""
import ctypes as C
import functools
import types
import numpy as np
import pytest
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, matcher
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, OLF_ERR_CAPACITY, OLF_ERR_INVALID, lib
from status_text import describes

pytestmark = pytest.mark.gpu

W, H = 320, 240
FX = FY = 200.0
CX, CY, MBF = 160.0, 120.0, 40.0
CAM = (FX, FY, CX, CY, MBF)
BOUNDS = (0.0, 320.0, 0.0, 240.0)
f32 = np.float32
TH_LOW = 50
INT_MAX = 2147483647
COUNTS = (0, 1, 63, 64, 65, 300, 900)
N_MP = 400

SF8 = np.ones(8, f32)
for _i in range(1, 8):
    SF8[_i] = f32(SF8[_i - 1] * f32(1.2))                    # the default context's mvScaleFactors (asserted against the context by the fixture)


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (the device tensors below)
    p = _lib.default_params()
    p.orb.nfeatures = 1400
    c = _lib.Context(p, W, H, 2)
    assert c.orb_capacity >= 1400
    sf = np.zeros(c.nlevels, np.float32)
    lib().olf_orb_scale_tables(c.handle, sf.ctypes.data_as(C.c_void_p), None, None, None, None)
    assert np.array_equal(sf, SF8)
    yield c
    c.close()


# ---- fabricated key frames and map ----------------------------------------------------------------------------------------------------------------
def pose(tx=0.0, ty=0.0, tz=0.0, ry_deg=0.0, rx_deg=0.0):
    T = np.eye(4)
    a, b = np.deg2rad(ry_deg), np.deg2rad(rx_deg)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T[:3, :3] = Ry @ Rx
    T[:3, 3] = [tx, ty, tz]
    return T


def camera_centre(Tcw):
    """-Rcw.t() * tcw as the library forms it when no Ow is given: double accumulation in index order, one rounding"""
    T = np.asarray(Tcw, f32).astype(np.float64)
    ow = np.zeros(3, f32)
    for r in range(3):
        acc = 0.0
        for k in range(3):
            acc += T[k, r] * T[k, 3]
        ow[r] = f32(-acc)
    return ow


def _flip(rng, desc, k):
    d = np.array(desc, np.uint8, copy=True).reshape(-1, 32)
    for r in range(len(d)):
        bits = rng.choice(256, size=int(k[r]) if np.ndim(k) else int(k), replace=False)
        for b in bits:
            d[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return d


class Map:
    """400 map points in front of the identity camera, each with the normal, the distance interval and the descriptor a creating frame at the origin
    would give it (so that PredictScale returns `octave` there) -- and fixed groups of points that one gate each rejects in every key frame of a scene"""
    GROUPS = ("bad", "negz", "outside", "below", "above", "angle")

    def __init__(self, rng, n=N_MP, per_group=8):
        u, v, z = rng.uniform(12, 308, n), rng.uniform(12, 228, n), rng.uniform(4, 20, n)
        self.octave = rng.integers(0, 8, n)
        world = np.stack([(u - CX) * z / FX, (v - CY) * z / FY, z], 1)
        self.group = {g: np.arange(k * per_group, (k + 1) * per_group) for k, g in enumerate(self.GROUPS)}
        world[self.group["negz"], 2] *= -1                                            # behind every camera of a scene
        world[self.group["outside"], 0] = (rng.uniform(380, 600, per_group) - CX) * z[self.group["outside"]] / FX      # far right of every image
        # one projection with u == maxX exactly in the identity key frame: z = 4, invz = 0.25, x = 0.8f, 200 * 0.8f rounds to 160, + 160 = 320
        self.edge = int(self.group["outside"][0]) if per_group else -1
        if per_group:
            world[self.edge] = [np.float64(f32(0.8)) * 4.0, 0.0, 4.0]
        self.world = np.ascontiguousarray(world, f32)
        dist = np.linalg.norm(self.world.astype(np.float64), axis=1)
        nrm = self.world / dist[:, None] + rng.normal(0, 0.05, world.shape)
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        nrm[self.group["angle"]] *= -1                                                # seen from behind
        self.normal = np.ascontiguousarray(nrm, f32)
        maxd = dist * SF8[self.octave] * rng.uniform(0.88, 0.99, n)
        mind = maxd / SF8[-1]
        mind[self.group["below"]] = 2.0 * dist[self.group["below"]]                   # 0.8 * mind = 1.6 * dist
        maxd[self.group["above"]] = 0.5 * dist[self.group["above"]]                   # 1.2 * maxd = 0.6 * dist
        self.maxd, self.mind = maxd.astype(f32), mind.astype(f32)
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.bad = np.zeros(n, bool)
        self.bad[self.group["bad"]] = True
        self.n = n
        self.plain = np.arange(len(self.GROUPS) * per_group, n)                       # the points no group claims


def decompose(kf):
    """(R, t, Ow) in double, for the numpy counts only"""
    if kf.Scw is not None:
        S = kf.Scw.astype(np.float64)
        s = np.linalg.norm(S[0, :3])
        R, t = S[:3, :3] / s, S[:3, 3] / s
    else:
        R, t = kf.Tcw[:3, :3].astype(np.float64), kf.Tcw[:3, 3].astype(np.float64)
    return R, t, -R.T @ t


def project(kf, mp):
    R, t, Ow = decompose(kf)
    Xc = mp.world.astype(np.float64) @ R.T + t
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = FX * Xc[:, 0] / Xc[:, 2] + CX, FY * Xc[:, 1] / Xc[:, 2] + CY
    PO = mp.world.astype(np.float64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    return Xc, u, v, dist, np.einsum("ij,ij->i", PO, mp.normal.astype(np.float64))


def classify(kf, mp):
    """the first gate that rejects each map point in key frame kf, by a numpy count in double ("pass": it reaches its window)"""
    Xc, u, v, dist, dot = project(kf, mp)
    out = np.full(mp.n, "pass", object)
    held = np.zeros(mp.n, bool)
    h = kf.held[(kf.held >= 0) & (kf.held < mp.n)]
    held[h] = True
    inimg = (u >= 0) & (u < 320) & (v >= 0) & (v < 240)
    for name, m in (("angle", dot < 0.5 * dist), ("above", dist > 1.2 * mp.maxd.astype(np.float64)), ("below", dist < 0.8 * mp.mind.astype(np.float64)),
                    ("outside", ~inimg), ("negz", Xc[:, 2] < 0), ("held", held), ("bad", mp.bad)):
        out[m] = name
    return out


class KF:
    pass


def make_kf(rng, mp, n, Tcw=None, Scw=None, jitter=2.5, held_p=1 / 3, mono_p=0.2, far_p=0.15):
    """a key frame of n key points that re-observe map points it sees: position = projection + jitter, octave around the predicted level, descriptor a
    few bits from the point's, mvuRight from the depth (or mono); a share of the features hold their point"""
    kf = KF()
    kf.Tcw = np.eye(4, dtype=f32) if Tcw is None else np.asarray(Tcw, f32)
    kf.Scw = None if Scw is None else np.asarray(Scw, f32)
    kf.held = np.zeros(0, np.int32)
    cls = classify(kf, mp)
    Xc, u, v, dist, _ = project(kf, mp)
    vis = np.flatnonzero((cls == "pass") & (u > 6) & (u < 314) & (v > 6) & (v < 234))
    assert len(vis) > 100
    src = rng.permutation(vis)[:n] if n <= len(vis) else np.concatenate([vis, rng.choice(vis, n - len(vis))])
    level = np.clip(np.ceil(np.log(mp.maxd[src] / dist[src]) / np.log(1.2) - 1e-9), 0, 7).astype(np.int64)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"] = u[src] + rng.uniform(-jitter, jitter, n)
    k["y"] = v[src] + rng.uniform(-jitter, jitter, n)
    k["octave"] = np.clip(level + rng.choice([-2, -1, -1, 0, 0, 0, 0, 1], n), 0, 7)
    k["angle"] = rng.uniform(0, 360, n)
    k["size"], k["class_id"] = 31, -1
    kf.keys = k
    kf.desc = _flip(rng, mp.desc[src], rng.integers(0, 12, n))
    far = rng.random(n) < far_p
    kf.desc[far] = rng.integers(0, 256, (int(far.sum()), 32), dtype=np.uint8)          # beyond TH_LOW
    kf.uright = np.where(rng.random(n) < mono_p, -1.0, k["x"] - MBF / Xc[src, 2] + rng.uniform(-1.5, 1.5, n)).astype(f32)
    kf.held = np.where(rng.random(n) < held_p, src, -1).astype(np.int32)
    kf.src = src
    return kf


def view(kf):
    return ola.KeyFrameView(kf.keys, kf.desc, kf.uright, SF8, FX, FY, CX, CY, MBF, BOUNDS, mTcw=kf.Tcw)


def oracle_frame(oracle, kf, mp, order, th, Ow=None, n=None):
    """(best_idx, best_dist) of key frame kf over the map points `order`, from the oracle; n: the key points in use"""
    order = np.asarray(order, np.int64)
    none = 256 if kf.Scw is None else INT_MAX
    if len(order) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    k2 = kf if n is None else types.SimpleNamespace(keys=kf.keys[:n], desc=kf.desc[:n], uright=kf.uright[:n], Tcw=kf.Tcw)
    held = np.zeros(mp.n, bool)
    hv = kf.held[:len(k2.keys)]
    held[hv[(hv >= 0) & (hv < mp.n)]] = True
    geom = ola.MapPointGeom(mp.world[order], mp.normal[order], mp.maxd[order], mp.mind[order], mp.desc[order], skip=mp.bad[order] | held[order])
    if len(k2.keys) == 0:                                    # (an empty key frame: every window is empty)
        return np.full(len(order), -1, np.int32), np.full(len(order), none, np.int32)
    if kf.Scw is None:
        bi, bd = oracle.fuse_search(view(k2), geom, th, camera_centre(kf.Tcw) if Ow is None else Ow)
    else:
        bi, bd = oracle.fuse_search_sim3(view(k2), kf.Scw, geom, th)
    return bi.astype(np.int32), bd.astype(np.int32)


def expect(oracle, kfs, mp, th, lists=None, ows=None, counts=None):
    """the batch's expected (best_idx, best_dist, nfused) over its entries"""
    bis, bds, nf = [], [], []
    for j, kf in enumerate(kfs):
        order = np.arange(mp.n) if lists is None else lists[j]
        bi, bd = oracle_frame(oracle, kf, mp, order, th, None if ows is None else ows[j], None if counts is None else counts[j])
        bis.append(bi); bds.append(bd); nf.append(int(((bi >= 0) & (bd <= TH_LOW)).sum()))
    cat = lambda a: np.concatenate(a + [np.zeros(0, np.int32)]).astype(np.int32)
    return cat(bis), cat(bds), np.asarray(nf, np.int32)


# ---- device side ----------------------------------------------------------------------------------------------------------------------------------
class DeviceBatch:
    """key frames, map and (optionally) mvpMapPoints / per-frame lists as the device arrays of the entry; counts may shorten or overstate a key frame"""

    def __init__(self, ctx, kfs, mp, held=True, lists=None, img_stride=1, counts=None, raw_lists=None):
        import torch
        self.ctx, self.n, self.st, cap = ctx, len(kfs), img_stride, ctx.orb_capacity
        nf, ni = self.n, max(self.n * img_stride, 1)
        rng = np.random.default_rng(5)
        kps = np.zeros((ni, cap), KEYPOINT_DTYPE)
        kps["octave"] = 99                                   # rows nothing may read: images between the frames, features past the count
        desc = rng.integers(0, 256, (ni, cap, 32), dtype=np.uint8)
        cnt = np.full(ni, 17, np.int32)
        ur, Tcw, Scw = np.full((max(nf, 1), cap), 5.0, f32), np.zeros((max(nf, 1), 4, 4), f32), np.zeros((max(nf, 1), 4, 4), f32)
        fmp = np.full((max(nf, 1), cap), 3, np.int32)         # (past N: a live index nothing may read)
        for j, kf in enumerate(kfs):
            m = len(kf.keys)
            assert m <= cap
            kps[j * img_stride, :m], desc[j * img_stride, :m] = kf.keys, kf.desc
            cnt[j * img_stride] = m if counts is None or counts[j] is None else counts[j]
            ur[j, :m], Tcw[j] = kf.uright, kf.Tcw
            if kf.Scw is not None:
                Scw[j] = kf.Scw
            fmp[j, :m] = kf.held
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.kps, self.desc, self.counts = up(kps.view(np.uint8).reshape(ni, cap, 28)), up(desc), up(cnt)
        self.uright, self.Tcw = up(ur), up(Tcw)
        self.Scw = up(Scw) if nf and kfs[0].Scw is not None else None
        self.frame_mp = up(fmp) if held else None
        u8 = lambda a: up(np.asarray(a, np.uint8))
        lo = li = None
        if lists is not None:
            lo = up(np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32))
            li = up(np.concatenate([np.asarray(x, np.int32) for x in lists] + [np.zeros(0, np.int32)]).astype(np.int32))
        if raw_lists is not None:
            lo, li = up(np.asarray(raw_lists[0], np.int32)), up(np.asarray(raw_lists[1], np.int32))
        self.map = matcher.LocalMapDev(up(mp.world), up(mp.normal), up(mp.maxd), up(mp.mind), up(mp.desc), None, u8(mp.bad), lo, li, n_mp=mp.n)
        self.offs = torch.full((max(nf, 1), _lib.GRID_CELLS + 1), -5, dtype=torch.int32, device="cuda")
        self.idx = torch.full((max(nf, 1), cap), -5, dtype=torch.int32, device="cuda")
        if nf:
            with matcher._torch_stream() as s:
                _lib.check(lib().olf_frame_grid_dev(ctx.handle, nf, img_stride, self.kps.data_ptr(), self.counts.data_ptr(), *BOUNDS, self.offs.data_ptr(),
                                                    self.idx.data_ptr(), s), "olf_frame_grid_dev")

    def search(self, th, Ow=None, nfused=True):
        """(best_idx, best_dist, nfused) as numpy arrays; the outputs start from a fill no result equals"""
        import torch
        ne = self.map.n_entries(self.n)
        out = (torch.full((ne,), -7, dtype=torch.int32, device="cuda"), torch.full((ne,), -7, dtype=torch.int32, device="cuda"),
               torch.full((max(self.n, 1),), -7, dtype=torch.int32, device="cuda") if nfused else None)
        ow = None if Ow is None else torch.from_numpy(np.ascontiguousarray(Ow, f32)).cuda()
        matcher.fuse_search_batch(self.n, self.kps, self.desc, self.counts, self.uright, self.offs, self.idx, self.Tcw, self.map, CAM, BOUNDS, th=th,
                                  Scw=self.Scw, Ow=ow, frame_mp=self.frame_mp, img_stride=self.st, out=out, context=self.ctx)
        torch.cuda.synchronize()
        return tuple(None if o is None else o.cpu().numpy() for o in out)


def assert_equal(res, exp, n_frames):
    bi, bd, nf = res
    assert np.array_equal(bi, exp[0]), np.flatnonzero(bi != exp[0])[:10]
    assert np.array_equal(bd, exp[1]), np.flatnonzero(bd != exp[1])[:10]
    if nf is not None:
        assert np.array_equal(nf[:n_frames], exp[2])


# ---- scenarios (each asserts, without a GPU, that its case occurs) ----------------------------------------------------------------------------------
POSES = [pose(), pose(0.05, -0.02, 0.1, 0.4), pose(-0.1, 0.03, -0.15, -0.6, 0.3), pose(0.12, 0.0, 0.2, 0.8, -0.4), pose(-0.04, 0.05, 0.05, -0.3, 0.5),
         pose(0.08, -0.06, -0.1, 0.5, 0.2), pose(-0.07, 0.02, 0.12, -0.9, -0.3)]


def sim3_of(T, s):
    S = np.array(T, np.float64)
    S[:3] *= s
    return S.astype(f32)


@functools.lru_cache(maxsize=None)
def scenario_gates(sim3):
    """1: the seven key frames of COUNTS key points at seven poses (the first is the identity); every gate rejects at least one entry, at least a tenth
    of the entries find a key point and at least one finds it within TH_LOW -- asserted on the oracle's output at th = 3 (plain) / 4 (Sim3)"""
    import oracle_lib as oracle
    rng = np.random.default_rng(101 + sim3)
    mp = Map(rng)
    scales = (1.0, 0.5, 2.0, 1.0, 0.5, 2.0, 1.0)
    kfs = [make_kf(rng, mp, n, Tcw=None if sim3 else T, Scw=sim3_of(T, s) if sim3 else None) for n, T, s in zip(COUNTS, POSES, scales)]
    th = 4.0 if sim3 else 3.0
    exp = expect(oracle, kfs, mp, th)
    none = INT_MAX if sim3 else 256
    bi, bd = exp[0].reshape(len(kfs), mp.n), exp[1].reshape(len(kfs), mp.n)
    seen = set()
    for j, kf in enumerate(kfs):
        cls = classify(kf, mp)
        rejected = cls != "pass"
        assert (bi[j][rejected] == -1).all() and (bd[j][rejected] == none).all()
        for g in Map.GROUPS:
            members = mp.group[g][mp.group[g] != mp.edge] if j else mp.group[g]      # (the edge point lies on the bound in the identity key frame only)
            assert (cls[members] == g).all(), (j, g)
        seen |= set(cls)
        if len(kf.keys):
            assert ((cls == "pass") & (bi[j] < 0)).sum() > 0                          # an empty window (or every candidate gated away)
    assert seen >= {"bad", "held", "negz", "outside", "below", "above", "angle", "pass"}
    # u == maxX exactly in the identity key frame, in the library's float arithmetic: rejected by the half-open IsInImage although the closed test of
    # Frame::isInFrustum would keep it
    p = mp.world[mp.edge]
    invz = f32(1.0) / p[2]
    assert f32(f32(f32(FX) * f32(p[0] * invz)) + f32(CX)) == f32(320.0) and classify(kfs[0], mp)[mp.edge] == "outside" and bi[0, mp.edge] == -1
    found = int((bi >= 0).sum())
    assert 10 * found >= bi.size and int(((bi >= 0) & (bd <= TH_LOW)).sum()) > 50, (found, bi.size)
    return types.SimpleNamespace(mp=mp, kfs=kfs, th=th, exp=exp)


def _one_point_scene(rng, level, z=8.0, u=150.3, v=110.7):
    """a map of one point that projects to (u, v) in the identity key frame and predicts `level` there"""
    mp = Map(rng, n=1, per_group=0)
    mp.world = np.array([[(u - CX) * z / FX, (v - CY) * z / FY, z]], f32)
    dist = np.linalg.norm(mp.world.astype(np.float64), axis=1)
    mp.normal = (mp.world / dist[:, None]).astype(f32)
    mp.maxd = (dist * SF8[level] * 0.93).astype(f32)
    mp.mind = (mp.maxd / SF8[-1]).astype(f32)
    return mp


def _kf_from(keys_xyo, desc, uright, Scw=None):
    kf = KF()
    k = np.zeros(len(keys_xyo), KEYPOINT_DTYPE)
    if len(keys_xyo):
        a = np.asarray(keys_xyo, np.float64)
        k["x"], k["y"], k["octave"] = a[:, 0], a[:, 1], a[:, 2].astype(np.int32)
    k["size"], k["class_id"] = 31, -1
    kf.keys, kf.desc, kf.uright = k, np.ascontiguousarray(desc, np.uint8).reshape(len(k), 32), np.asarray(uright, f32)
    kf.Tcw, kf.Scw = np.eye(4, dtype=f32), Scw
    kf.held = np.full(len(k), -1, np.int32)
    return kf


@functools.lru_cache(maxsize=None)
def scenario_chi2():
    """2: one point per key frame-level pair; around its projection, stereo and mono candidates on both sides of 7.8 and 5.99 (all with the point's own
    descriptor except a farther decoy), and a key point with mvuRight == 0.0 whose right-image error fails the stereo test although the mono test would
    pass.  At th = 3 the chi-square gate decides, at th = 1 the window edge does; th = 6 equals th = 3"""
    import oracle_lib as oracle
    rng = np.random.default_rng(202)
    scenes = []
    for level in (0, 2, 5):
        mp = _one_point_scene(rng, level)
        u, v, z = 150.3, 110.7, 8.0
        ur = u - MBF / z
        sf = float(SF8[level])
        kfs = []
        # each key frame: one near candidate (the one that should win or be gated) at the point's descriptor, one safe decoy 20 bits away at the centre
        for kind, r, stereo in (("stereo_in", 2.7, True), ("stereo_out", 2.9, True), ("mono_in", 2.4, False), ("mono_out", 2.5, False),
                                ("edge_th1_in", 0.95, False), ("edge_th1_out", 1.05, False)):
            # e2 = (r * sf)^2 spread evenly over the error's components: three with mvuRight, two without
            dx = r * sf if kind.startswith("edge") else r * sf / np.sqrt(3.0 if stereo else 2.0)
            dy = 0.0 if kind.startswith("edge") else dx
            keys = [(u + dx, v + dy, level), (u + 0.1, v, level)]
            kur = [ur + dx if stereo else -1.0, -1.0]
            kfs.append(_kf_from(keys, np.stack([mp.desc[0], _flip(rng, mp.desc[0], 20)[0]]), kur))
        # mvuRight == 0.0: stereo here (>= 0); e2 = 0.5 + er^2 is far beyond 7.8 * sigma2, the mono error 0.5 / sigma2 is below 5.99
        kfs.append(_kf_from([(u + 0.5, v + 0.5, level), (u + 0.1, v, level)], np.stack([mp.desc[0], _flip(rng, mp.desc[0], 20)[0]]), [0.0, -1.0]))
        res = {th: expect(oracle, kfs, mp, th) for th in (1.0, 3.0, 6.0)}
        assert np.array_equal(res[3.0][0], res[6.0][0]) and np.array_equal(res[3.0][1], res[6.0][1])
        # th = 3: in -> the near candidate (distance 0), out -> the decoy (distance 20)
        assert list(res[3.0][0]) == [0, 1, 0, 1, 0, 0, 1] and list(res[3.0][1]) == [0, 20, 0, 20, 0, 0, 20], (level, res[3.0])
        # th = 1: the window is sf wide: 2.7 / sqrt 3 ~ 1.56 sf and 2.4 / sqrt 2 ~ 1.7 sf lie outside it, 0.95 sf inside, 1.05 sf outside
        assert list(res[1.0][0]) == [1, 1, 1, 1, 0, 1, 1], (level, res[1.0])
        scenes.append(types.SimpleNamespace(mp=mp, kfs=kfs, exp=res))
    return scenes


@functools.lru_cache(maxsize=None)
def scenario_levels(sim3):
    """3: candidates at level - 2, level - 1, level, level + 1 around one projection, the nearer the descriptor the farther the level is off; predicted
    levels 0, 3 and 7 (both clamps: a ratio below 1 and one beyond 1.2^7)"""
    import oracle_lib as oracle
    rng = np.random.default_rng(303)
    scenes = []
    for level, ratio in ((0, 0.9), (3, None), (7, 6.0)):
        mp = _one_point_scene(rng, level)
        if ratio is not None:
            dist = np.linalg.norm(mp.world.astype(np.float64), axis=1)
            mp.maxd = (dist * ratio).astype(f32)
            mp.mind = (mp.maxd / f32(8.0)).astype(f32)
        u, v = 150.3, 110.7
        octs = [o for o in (level - 2, level - 1, level, level + 1) if 0 <= o <= 7]
        # descriptor distance: the off-level candidates are the nearest
        dd = {level - 2: 0, level + 1: 1, level - 1: 9, level: 12}
        keys = [(u + 0.2 * k, v - 0.2 * k, o) for k, o in enumerate(octs)]
        desc = np.stack([_flip(rng, mp.desc[0], dd[o])[0] for o in octs])
        S = np.eye(4, dtype=f32) if sim3 else None
        kf = _kf_from(keys, desc, [-1.0] * len(octs), Scw=S)
        exp = expect(oracle, [kf], mp, 4.0 if sim3 else 3.0)
        want = octs.index(level - 1) if level - 1 in octs else octs.index(level)
        assert exp[0][0] == want and exp[1][0] == dd[octs[want]], (level, exp)
        scenes.append(types.SimpleNamespace(mp=mp, kfs=[kf], exp=exp))
    return scenes


@functools.lru_cache(maxsize=None)
def scenario_crowd():
    """4: one map point, 150 key points within +-1 px of its projection, octaves from {3, 4, 5, 6} around predicted level 5, half at distance 0 and half
    at distance 1: more than 64 pass the level gate, many tie at distance 0, and the winner is the first in SCAN order, not the lowest index"""
    import oracle_lib as oracle
    rng = np.random.default_rng(404)
    mp = _one_point_scene(rng, 5, u=152.5, v=112.5)          # (a corner of four grid cells -- 5 x 5 px, rounded -- so that scan order is not index order)
    n = 150
    x, y = 152.5 + rng.uniform(-1, 1, n), 112.5 + rng.uniform(-1, 1, n)
    octs = rng.integers(3, 7, n)
    one = rng.permutation(n) < n // 2
    desc = np.repeat(mp.desc, n, 0)
    desc[one] = _flip(rng, desc[one], 1)
    kf = _kf_from(np.stack([x, y, octs], 1), desc, [-1.0] * n)
    exp = expect(oracle, [kf], mp, 3.0)
    passing = (octs >= 4) & (octs <= 5)
    tie = np.flatnonzero(passing & ~one)
    assert passing.sum() > 64 and len(tie) > 10
    assert exp[1][0] == 0 and exp[0][0] in tie and exp[0][0] != tie.min(), (exp, tie[:5])
    return types.SimpleNamespace(mp=mp, kfs=[kf], exp=exp)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim3", [0, 1])
def test_gates(ctx, sim3):
    s = scenario_gates(sim3)
    assert_equal(DeviceBatch(ctx, s.kfs, s.mp).search(s.th), s.exp, len(s.kfs))
    ctx.poll_status()


def test_window_against_chi_square(ctx, oracle):
    for s in scenario_chi2():
        dev = DeviceBatch(ctx, s.kfs, s.mp)
        for th in (1.0, 3.0):
            assert_equal(dev.search(th), s.exp[th], len(s.kfs))
    # the Sim3 form has no chi-square gate: the window alone decides, th = 4 and th = 10 on the full scene's key frames
    g = scenario_gates(1)
    dev = DeviceBatch(ctx, g.kfs, g.mp)
    e4, e10 = g.exp, expect(oracle, g.kfs, g.mp, 10.0)
    assert (e4[0] != e10[0]).sum() > 20                      # (the wider window changes results)
    assert_equal(dev.search(4.0), e4, len(g.kfs))
    assert_equal(dev.search(10.0), e10, len(g.kfs))
    ctx.poll_status()


@pytest.mark.parametrize("sim3", [0, 1])
def test_level_gate(ctx, sim3):
    for s in scenario_levels(sim3):
        assert_equal(DeviceBatch(ctx, s.kfs, s.mp).search(4.0 if sim3 else 3.0), s.exp, 1)
    ctx.poll_status()


def test_crowded_tie(ctx):
    s = scenario_crowd()
    assert_equal(DeviceBatch(ctx, s.kfs, s.mp).search(3.0), s.exp, 1)
    ctx.poll_status()


def test_distance_256(ctx, oracle):
    """5: a lone candidate with the complemented descriptor: plain never registers it (bestDist starts at 256), the Sim3 form does (INT_MAX)"""
    rng = np.random.default_rng(505)
    mp = _one_point_scene(rng, 2)
    for S, want in ((None, (-1, 256)), (np.eye(4, dtype=f32), (0, 256))):
        kf = _kf_from([(150.3, 110.7, 2)], ~mp.desc, [-1.0], Scw=S)
        exp = expect(oracle, [kf], mp, 4.0)
        assert (int(exp[0][0]), int(exp[1][0])) == want and exp[2][0] == 0
        assert_equal(DeviceBatch(ctx, [kf], mp).search(4.0), exp, 1)
    ctx.poll_status()


def test_sim3_decomposition(ctx, oracle):
    """6: scales 0.5, 1 and 2 with a small rotation (scenario_gates(1)); a scale that is no power of two as well, against oracle.sim3_decompose through
    the results: the device pose must equal the oracle's bit for bit, or projections at gate thresholds move"""
    rng = np.random.default_rng(606)
    mp = Map(rng)
    kfs = [make_kf(rng, mp, 300, Scw=sim3_of(T, s)) for T, s in zip(POSES[:4], (0.5, 1.0, 2.0, 1.37))]
    for kf in kfs:                                           # (the oracle's decomposition is what its search runs on: the scenes are not degenerate)
        R, t, Ow = oracle.sim3_decompose(kf.Scw)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-5) and np.allclose(-R.T @ t, Ow, atol=1e-5)
    exp = expect(oracle, kfs, mp, 4.0)
    assert (exp[0] >= 0).sum() > 150 and exp[2].sum() > 80
    assert_equal(DeviceBatch(ctx, kfs, mp).search(4.0), exp, len(kfs))
    ctx.poll_status()


@pytest.mark.parametrize("sim3", [0, 1])
def test_lists_strides_counts(ctx, oracle, sim3):
    """7: lists (empty ones, a point in several lists, reversed order, and offsets that leave entries before the first and after the last list outside
    every list) versus none; img_stride 1 and 2; counts beyond the capacity and below N; d_Ow given versus NULL; d_nfused NULL"""
    s = scenario_gates(sim3)
    rng = np.random.default_rng(707)
    kfs, mp = s.kfs[2:], s.mp                                 # 63, 64, 65, 300, 900 key points
    lists = [rng.permutation(mp.n)[:150], np.zeros(0, np.int64), np.arange(mp.n)[::-1], np.zeros(0, np.int64), np.concatenate([np.arange(100), np.arange(50, 120)])]
    assert len(set(lists[0]) & set(lists[2]) & set(lists[4])) > 10
    exp_l = expect(oracle, kfs, mp, s.th, lists=lists)
    assert (exp_l[0] >= 0).sum() > 30 and exp_l[2][1] == 0 and exp_l[2][3] == 0
    for st in (1, 2):
        assert_equal(DeviceBatch(ctx, kfs, mp, lists=lists, img_stride=st).search(s.th), exp_l, len(kfs))
    # the same lists after a gap of 7 entries, 9 more behind them: entries outside every list get the "nothing" pair
    none = INT_MAX if sim3 else 256
    offs = 7 + np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    li = np.concatenate([np.zeros(7, np.int64)] + lists + [np.zeros(9, np.int64)])
    pad = lambda a, fill: np.concatenate([np.full(7, fill, np.int32), a, np.full(9, fill, np.int32)])
    assert_equal(DeviceBatch(ctx, kfs, mp, raw_lists=(offs, li)).search(s.th), (pad(exp_l[0], -1), pad(exp_l[1], none), exp_l[2]), len(kfs))
    # counts: beyond the capacity reads as the capacity -- the key frame is padded to it here so that the rows past N are defined -- and below N cuts
    cap = ctx.orb_capacity
    counts = [None, 40, None, cap + 1000, 250]
    big = make_kf(rng, mp, cap, Tcw=None if sim3 else POSES[5], Scw=sim3_of(POSES[5], 2.0) if sim3 else None)
    kfs_c = [kfs[0], kfs[1], kfs[2], big, kfs[4]]
    exp_c = expect(oracle, kfs_c, mp, s.th, counts=[None, 40, None, cap, 250])
    assert_equal(DeviceBatch(ctx, kfs_c, mp, counts=counts, img_stride=2).search(s.th, nfused=False), exp_c, len(kfs_c))
    if not sim3:
        ows = np.stack([camera_centre(k.Tcw) + np.array([0.3, -0.2, 0.6], f32) * (j + 1) for j, k in enumerate(kfs)]).astype(f32)      # a centre that is not the pose's own
        exp_o = expect(oracle, kfs, mp, s.th, ows=ows)
        base = expect(oracle, kfs, mp, s.th)
        assert not (np.array_equal(exp_o[0], base[0]) and np.array_equal(exp_o[1], base[1]))
        dev = DeviceBatch(ctx, kfs, mp)
        assert_equal(dev.search(s.th, Ow=ows), exp_o, len(kfs))
        assert_equal(dev.search(s.th), base, len(kfs))
    ctx.poll_status()


def test_malformed_input(ctx, oracle):
    """8: a list index >= n_mp and a negative one, a d_frame_mp value >= n_mp: bit 512, every other entry equals the oracle.  A plain-mode candidate
    with octave -1 under predicted level 0: bit 256, the candidate left out, the others equal; olf_fuse_search refuses that key frame"""
    s = scenario_gates(0)
    kfs, mp = [s.kfs[2], s.kfs[5]], s.mp
    lists = [np.arange(mp.n), np.arange(100, 300)]
    exp = [x.copy() for x in expect(oracle, kfs, mp, 3.0, lists=lists)]
    bad_at = (7, mp.n + 20)
    li = np.concatenate(lists).astype(np.int64)
    li[bad_at[0]], li[bad_at[1]] = mp.n, -3
    for e in bad_at:                                          # the malformed entries are left out; recount their frames
        exp[0][e], exp[1][e] = -1, 256
    exp[2] = np.array([((exp[0][:mp.n] >= 0) & (exp[1][:mp.n] <= TH_LOW)).sum(), ((exp[0][mp.n:] >= 0) & (exp[1][mp.n:] <= TH_LOW)).sum()], np.int32)
    dev = DeviceBatch(ctx, kfs, mp, raw_lists=([0, mp.n, mp.n + 200], li))
    assert_equal(dev.search(3.0), exp, 2)
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert e.value.code == OLF_ERR_CAPACITY and "flags=512" in str(e.value) and describes(e.value, 512)
    ctx.poll_status()                                         # reported once, then clear
    # a held index outside the map counts as "holds nothing"
    kf = types.SimpleNamespace(**vars(kfs[1]))
    kf.held = kf.held.copy()
    kf.held[0] = mp.n + 5
    exp1 = expect(oracle, [kf], mp, 3.0)
    assert_equal(DeviceBatch(ctx, [kf], mp).search(3.0), exp1, 1)
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert "flags=512" in str(e.value) and describes(e.value, 512)
    # octave -1 under predicted level 0: the best candidate of the point is the malformed one; without it the second one wins
    rng = np.random.default_rng(808)
    mp1 = _one_point_scene(rng, 0)
    desc = np.stack([mp1.desc[0], _flip(rng, mp1.desc[0], 6)[0]])
    good = _kf_from([(150.5, 110.7, 0)], desc[1:], [-1.0])
    other = types.SimpleNamespace(**vars(s.kfs[2]))           # a second key frame of the batch, holding nothing of this one-point map
    other.held = np.full(len(other.keys), -1, np.int32)
    exp_good = expect(oracle, [good, other], mp1, 3.0)    # (the oracle never sees the octave -1 key point: it would read mvInvLevelSigma2[-1])
    assert exp_good[0][0] == 0 and exp_good[1][0] == 6
    malformed = _kf_from([(150.3, 110.7, -1), (150.5, 110.7, 0)], desc, [-1.0, -1.0])
    res = DeviceBatch(ctx, [malformed, other], mp1).search(3.0)
    assert (res[0][0], res[1][0]) == (1, 6) and res[0][1] == exp_good[0][1] and res[1][1] == exp_good[1][1]
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert "flags=256" in str(e.value) and describes(e.value, 256)
    geom = ola.MapPointGeom(mp1.world, mp1.normal, mp1.maxd, mp1.mind, mp1.desc)
    with pytest.raises(ola.OlfError) as e:
        ola.ORBmatcher(0.6, True, context=ctx).FuseSearch(view(malformed), geom, 3.0, np.zeros(3, f32))
    assert e.value.code == OLF_ERR_INVALID
    # the Sim3 form has no per-octave table to read: the same key point is a candidate like any other
    malformed.Scw = good.Scw = np.eye(4, dtype=f32)
    res = DeviceBatch(ctx, [malformed], mp1).search(3.0)
    assert (res[0][0], res[1][0]) == (0, 0)
    ctx.poll_status()


def test_error_codes(ctx):
    """9: refused before any launch; n_frames == 0 leaves the outputs untouched; no entries: nfused = 0"""
    import torch
    s = scenario_gates(0)
    dev = DeviceBatch(ctx, s.kfs[2:4], s.mp)
    ne = 2 * s.mp.n
    out = [torch.full((ne,), -7, dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.full((2,), -7, dtype=torch.int32, device="cuda")]

    def call(n_frames=2, h=None, tb_edit=None, lm_edit=None, bi=out[0], bd=out[1], bounds=BOUNDS):
        tb = matcher._track_batch_c(dev.kps, dev.desc, dev.counts, 1, dev.uright, dev.offs, dev.idx, dev.Tcw, CAM, bounds)
        lm = dev.map.c(n_frames)
        for k, v in (tb_edit or {}).items():
            setattr(tb, k, v)
        for k, v in (lm_edit or {}).items():
            setattr(lm, k, v)
        p = lambda t: None if t is None else t.data_ptr()
        torch.cuda.synchronize()
        rc = lib().olf_fuse_search_batch_dev(ctx.handle if h is None else h, C.byref(tb), n_frames, C.byref(lm), None, None, None, 3.0, p(bi), p(bd),
                                             out[2].data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    assert call(n_frames=-1) == OLF_ERR_INVALID
    assert call(bi=None) == OLF_ERR_INVALID and call(bd=None) == OLF_ERR_INVALID
    for k in ("kps", "desc", "counts", "uright", "cell_offsets", "cell_index", "Tcw"):
        assert call(tb_edit={k: None}) == OLF_ERR_INVALID, k
    assert call(tb_edit={"img_stride": 0}) == OLF_ERR_INVALID
    for k in ("world", "normal", "maxd", "mind", "desc", "bad"):
        assert call(lm_edit={k: None}) == OLF_ERR_INVALID, k
    assert call(lm_edit={"n_mp": -1}) == OLF_ERR_INVALID
    assert call(bounds=(0.0, 0.0, 0.0, 240.0)) == OLF_ERR_INVALID and call(bounds=(0.0, 320.0, 240.0, 240.0)) == OLF_ERR_INVALID
    assert all((o == -7).all() for o in out)                 # nothing was launched
    p = _lib.default_params()
    p.orb.nfeatures = _lib.GRID_MAX_KEYS + 1
    big = _lib.Context(p, W, H, 1)
    try:
        assert big.orb_capacity > _lib.GRID_MAX_KEYS
        assert call(h=big.handle) == OLF_ERR_CAPACITY                                   # (refused before anything is read)
    finally:
        big.close()
    assert call(n_frames=0) == _lib.OLF_OK and all((o == -7).all() for o in out)
    assert call(lm_edit={"n_mp": 0}) == _lib.OLF_OK                                     # no entries at all
    assert (out[0] == -7).all() and (out[1] == -7).all() and (out[2] == 0).all()
    ctx.poll_status()


# 10: extracted frames ------------------------------------------------------------------------------------------------------------------------------
def test_equals_the_loop_of_host_entries(oracle):
    """Four real stereo pairs through the fused entry, olf_frame_grid_dev and olf_unproject_stereo_dev; every frame is searched against the others'
    stereo points, in both forms, and equals olf_fuse_search / olf_fuse_search_sim3 frame by frame -- with the host form's own grid and a supplied one"""
    import torch
    from orb_line_slam_amd import synth
    w, h, B = 640, 480, 4
    cam = (435.2047, 435.2047, 320.0, 240.0, 47.9064)
    fe = ola.StereoFrontEnd(oracle.full_params(1000, 100, cam[0], cam[4]), w, h, max_pairs=B)
    try:
        imgs = synth.stereo_batch(71, B, w, h)
        for i in range(1, B):
            imgs[2 * i:2 * i + 2] = np.roll(imgs[:2], 2 * i, axis=2)
        f = fe.frames(imgs)
        ctx, cap = fe.ctx, fe.ctx.orb_capacity
        sf = np.zeros(ctx.nlevels, f32)
        lib().olf_orb_scale_tables(ctx.handle, sf.ctypes.data_as(C.c_void_p), None, None, None, None)
        bounds = (0.0, float(w), 0.0, float(h))
        # frame i's camera sits 2 i px worth of baseline to the side at depth ~ 10: identity rotations, so the shifted copies see the same points
        Tcw = np.stack([np.eye(4, dtype=f32)] * B)
        Twc = Tcw.copy()
        world = fe.unproject_stereo(cam[:4], Twc)
        mask = fe.stereo_points_mask()
        fb, n = fe._last_frames("test")
        offs, idx = torch.zeros((B, _lib.GRID_CELLS + 1), dtype=torch.int32, device="cuda"), torch.zeros((B, cap), dtype=torch.int32, device="cuda")
        with matcher._torch_stream() as s:
            _lib.check(lib().olf_frame_grid_dev(ctx.handle, B, 2, fb.kps, fb.counts, *bounds, offs.data_ptr(), idx.data_ptr(), s), "olf_frame_grid_dev")
        pairs = [f.pair(i) for i in range(B)]
        N = [len(p["mvKeys"]) for p in pairs]
        wh, mh = world.cpu().numpy(), mask.cpu().numpy().astype(bool)
        # the map: every frame's stereo points, as the frame that made them would describe them
        sel = [np.flatnonzero(mh[i, :N[i]]) for i in range(B)]
        base = np.concatenate([[0], np.cumsum([len(x) for x in sel])])
        mw = np.concatenate([wh[i, sel[i]] for i in range(B)]).astype(f32)
        dist = np.linalg.norm(mw.astype(np.float64), axis=1)
        octv = np.concatenate([pairs[i]["mvKeys"]["octave"][sel[i]] for i in range(B)])
        maxd = (dist * sf[octv] * 0.95).astype(f32)
        mind = (maxd / sf[-1]).astype(f32)
        normal = (mw / dist[:, None]).astype(f32)
        mdesc = np.concatenate([pairs[i]["mDescriptors"][sel[i]] for i in range(B)])
        n_mp = len(mw)
        lists = [np.concatenate([np.arange(base[k], base[k + 1]) for k in range(B) if k != i]) for i in range(B)]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        lo = up(np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32))
        li = up(np.concatenate(lists).astype(np.int32))
        lmap = matcher.LocalMapDev(up(mw), up(normal), up(maxd), up(mind), up(mdesc), None, up(np.zeros(n_mp, np.uint8)), lo, li, n_mp=n_mp)
        Scw = np.stack([np.eye(4, dtype=f32)] * B)
        Scw[:, :3] *= f32(1.25)
        m = ola.ORBmatcher(0.6, True, context=ctx)
        for sim3 in (False, True):
            bi, bd, nf = matcher.fuse_search_batch(B, fb.kps, fb.desc, fb.counts, fb.uright, offs, idx, up(Tcw), lmap, cam, bounds, th=4.0 if sim3 else 3.0,
                                                   Scw=up(Scw) if sim3 else None, img_stride=2, context=ctx)
            torch.cuda.synchronize()
            bi, bd, nf = bi.cpu().numpy(), bd.cpu().numpy(), nf.cpu().numpy()
            found = 0
            for i in range(B):
                p = pairs[i]
                kf = ola.KeyFrameView(p["mvKeys"], p["mDescriptors"], p["mvuRight"], sf, *cam, bounds, mTcw=Tcw[i])
                o = lists[i]
                geom = ola.MapPointGeom(mw[o], normal[o], maxd[o], mind[o], mdesc[o])
                for supplied in (False, True):
                    if supplied:
                        go, gi = ola.assign_features_to_grid(p["mvKeys"], bounds, context=ctx)
                        kf.attach_grid(go, gi)
                    hi, hd = m.FuseSearchSim3(kf, Scw[i], geom, 4.0) if sim3 else m.FuseSearch(kf, geom, 3.0)
                    a, b = int(lo[i]), int(lo[i + 1])
                    assert np.array_equal(bi[a:b], hi) and np.array_equal(bd[a:b].astype(np.int64), np.asarray(hd, np.int64))
                    assert nf[i] == ((hi >= 0) & (np.asarray(hd) <= TH_LOW)).sum()
                found += int((hi >= 0).sum())
            assert found > 200, found
        ctx.poll_status()
    finally:
        fe.ctx.close()
