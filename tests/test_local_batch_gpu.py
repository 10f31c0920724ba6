"""GPU parity: olf_is_in_frustum_batch_dev and olf_search_local_map_batch_dev -- the point half of Tracking::SearchLocalPointsAndLines
(src/Tracking.cc:1877-1942): Frame::isInFrustum (src/Frame.cc:388-444) for every (frame, local map point) and
ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:47-131) for every frame of a device-resident batch.
Every expectation comes from the CPU oracle frame by frame (oracle.is_in_frustum, then oracle.search_local_map); the skip rule of
SearchLocalPointsAndLines (bad points, points the frame already holds) is applied here by clearing mbTrackInView, and list positions are mapped to
map indices.  The floors are asserted on the ORACLE's outputs, so that no test can pass by having nothing to compare.
Frames are synthetic (no extractor), 320 x 240; the generators are those of test_track_batch_gpu.py."""
import ctypes as C
import functools
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


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (the device tensors below)
    p = _lib.default_params()
    p.orb.nfeatures = 1400
    c = _lib.Context(p, W, H, 2)
    assert c.orb_capacity >= 1400
    yield c
    c.close()


def scale_factors(ctx):
    sf = np.zeros(ctx.nlevels, np.float32)
    lib().olf_orb_scale_tables(ctx.handle, sf.ctypes.data_as(C.c_void_p), None, None, None, None)
    return sf


SF8 = np.ones(8, f32)
for _i in range(1, 8):
    SF8[_i] = f32(SF8[_i - 1] * f32(1.2))                    # the default context's mvScaleFactors (asserted against the context in every case)


# ---- synthetic frames (no extractor) ------------------------------------------------------------------------------------------------------
def pose(tx=0.0, ty=0.0, tz=0.0, ry_deg=0.0, rx_deg=0.0):
    T = np.eye(4)
    a, b = np.deg2rad(ry_deg), np.deg2rad(rx_deg)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    T[:3, :3] = Ry @ Rx
    T[:3, 3] = [tx, ty, tz]
    return T


class SynthFrame:
    """one frame: keys / desc / uright / depth of its features, its pose, and the world points of its features"""

    def unproject(self):
        Twc = np.linalg.inv(self.Tcw.astype(np.float64))
        z = self.depth.astype(np.float64)
        Xc = np.stack([(self.keys["x"] - CX) * z / FX, (self.keys["y"] - CY) * z / FY, z], 1)
        self.mp_world = (Xc @ Twc[:3, :3].T + Twc[:3, 3]).astype(np.float32)
        self.Ow = Twc[:3, 3]
        return self

    def view(self, sf, n=None):
        n = len(self.keys) if n is None else n
        return ola.FrameView(self.keys[:n], self.desc[:n], self.uright[:n], sf, FX, FY, CX, CY, MBF, BOUNDS, mTcw=self.Tcw)


def _flip(rng, desc, k):
    d = desc.copy()
    for r in range(len(d)):
        for _ in range(k):
            d[r, rng.integers(32)] ^= np.uint8(1 << rng.integers(8))
    return d


def _dup(fr, rng, max_octave=7):
    """every feature listed twice; the second copy is 0 or 2 descriptor bits away, on the same or on a neighbouring octave"""
    n = len(fr.keys)
    k2 = fr.keys.copy()
    k2["octave"] = np.clip(k2["octave"] + rng.integers(-1, 2, n), 0, max_octave)
    d2 = fr.desc.copy()
    two = rng.random(n) < 0.5
    d2[two] = _flip(rng, fr.desc[two], 2)
    fr.keys, fr.desc = np.concatenate([fr.keys, k2]), np.concatenate([fr.desc, d2])
    fr.uright, fr.depth = np.concatenate([fr.uright, fr.uright]), np.concatenate([fr.depth, fr.depth])


def first_frame(rng, n, squeeze=1.0, max_octave=7, similar=False):
    fr = SynthFrame()
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"] = (CX + (rng.uniform(8, 312, n) - CX) * squeeze).astype(f32)
    k["y"] = (CY + (rng.uniform(8, 232, n) - CY) * squeeze).astype(f32)
    k["octave"] = rng.integers(0, max_octave + 1, n)
    k["angle"] = rng.uniform(0, 360, n).astype(f32)
    k["size"], k["class_id"] = 31, -1
    fr.keys, fr.depth = k, rng.uniform(2, 20, n).astype(f32)
    fr.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if similar:                                              # every descriptor within a few bits of one base: every candidate is below TH_HIGH
        fr.desc = _flip(rng, np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), n, 0), 12)
    fr.uright = np.where(rng.random(n) < 0.2, -1.0, k["x"] - MBF / fr.depth + rng.uniform(-1, 1, n)).astype(f32)
    fr.Tcw = np.eye(4, dtype=f32)
    return fr.unproject()


def next_frame(rng, prev, D, n_dis, jitter=2.0, flips=4, max_octave=7, squeeze=1.0):
    """re-observes prev's points under the pose D * prev.Tcw, adds distractors, permutes"""
    fr = SynthFrame()
    Tcw = D @ prev.Tcw.astype(np.float64)
    nu = len(prev.keys)
    Xc = prev.mp_world.astype(np.float64) @ Tcw[:3, :3].T + Tcw[:3, 3]
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = FX * Xc[:, 0] / z + CX, FY * Xc[:, 1] / z + CY
    u, v = u + rng.uniform(-jitter, jitter, nu), v + rng.uniform(-jitter, jitter, nu)
    ok = np.flatnonzero((z > 0.5) & (u >= 8) & (u <= 312) & (v >= 8) & (v <= 232))
    m = len(ok)
    k = np.zeros(m + n_dis, KEYPOINT_DTYPE)
    k["x"][:m], k["y"][:m] = u[ok], v[ok]
    k["octave"][:m] = np.clip(prev.keys["octave"][ok] + rng.integers(-1, 2, m), 0, max_octave)
    k["angle"] = rng.uniform(0, 360, m + n_dis)
    depth = np.concatenate([z[ok], rng.uniform(2, 20, n_dis)]).astype(f32)
    desc = np.concatenate([_flip(rng, prev.desc[ok], flips), rng.integers(0, 256, (n_dis, 32), dtype=np.uint8)])
    k["x"][m:] = CX + (rng.uniform(8, 312, n_dis) - CX) * squeeze
    k["y"][m:] = CY + (rng.uniform(8, 232, n_dis) - CY) * squeeze
    k["octave"][m:] = rng.integers(0, max_octave + 1, n_dis)
    k["size"], k["class_id"] = 31, -1
    ur = np.where(rng.random(m + n_dis) < 0.2, -1.0, k["x"] - MBF / depth + rng.uniform(-1, 1, m + n_dis)).astype(f32)
    perm = rng.permutation(m + n_dis)
    fr.keys, fr.desc, fr.uright, fr.depth = k[perm], desc[perm], ur[perm], depth[perm]
    fr.Tcw = Tcw.astype(f32)
    return fr.unproject()


def make_chain(rng, motions, n=300, n_dis=60, **kw):
    first_kw = {k: kw[k] for k in ("squeeze", "max_octave", "similar") if k in kw}
    next_kw = {k: kw[k] for k in ("squeeze", "max_octave", "flips") if k in kw}
    frames = [first_frame(rng, n, **first_kw)]
    for D in motions:
        frames.append(next_frame(rng, frames[-1], D, n_dis, **next_kw))
    return frames


class LocalMap:
    """the map as arrays: the stereo points of the frames' own features (frame j's feature i is point base[j] + i), each with the normal, the distance
    interval and the descriptor its creating frame would give it -- so that the level PredictScale returns in that frame is the feature's octave"""

    def __init__(self, rng, frames, sf, obs_p=0.5, bad_p=0.1):
        self.base = np.concatenate([[0], np.cumsum([len(f.keys) for f in frames])]).astype(np.int64)
        PO = np.concatenate([f.mp_world.astype(np.float64) - f.Ow for f in frames])
        dist = np.linalg.norm(PO, axis=1)
        octv = np.concatenate([f.keys["octave"] for f in frames])
        nrm = PO / dist[:, None] + rng.normal(0, 0.05, PO.shape)
        self.world = np.ascontiguousarray(np.concatenate([f.mp_world for f in frames]), f32)
        self.normal = np.ascontiguousarray(nrm / np.linalg.norm(nrm, axis=1)[:, None], f32)
        self.maxd = (dist * sf[octv] * rng.uniform(0.88, 0.99, len(dist))).astype(f32)
        self.mind = (self.maxd / sf[-1]).astype(f32)
        self.desc = _flip(rng, np.concatenate([f.desc for f in frames]), 1)
        self.n = len(dist)
        self.obs = rng.random(self.n) < obs_p
        self.bad = rng.random(self.n) < bad_p

    def held(self, rng, frames, p):
        """mvpMapPoints of every frame: a share p of its features hold their own point"""
        return [np.where(rng.random(len(f.keys)) < p, self.base[j] + np.arange(len(f.keys)), -1).astype(np.int32) for j, f in enumerate(frames)]


# ---- the oracle, frame by frame -----------------------------------------------------------------------------------------------------------
def oracle_frustum(oracle, sf, fr, mp, frame_mp, order=None, n=None, cos_limit=0.5):
    """(inView, level, viewCos, proj3) over the frame's entries, with the skip rule applied; also the frame's view with mvpMapPoints set"""
    order = np.arange(mp.n) if order is None else np.asarray(order, np.int64)
    v = fr.view(sf, n)
    geom = ola.MapPointGeom(mp.world[order], mp.normal[order], mp.maxd[order], mp.mind[order], mp.desc[order], skip=mp.bad[order])
    inv, lvl, cosv, proj = oracle.is_in_frustum(v, geom, cos_limit)
    held = np.zeros(mp.n + 1, bool)
    if frame_mp is not None:
        fm = np.asarray(frame_mp[:v.N], np.int64)
        live = (fm >= 0) & (fm < mp.n)
        live[live] &= ~mp.bad[fm[live]]                      # a bad point is dropped from its feature (src/Tracking.cc:1885-1888)
        held[fm[live]] = True
        v.mp_valid[:] = live
        v.mp_obs[live] = mp.obs[fm[live]]
    inv = inv & ~mp.bad[order] & ~held[order]
    return (inv, lvl, cosv, proj), v, order


def oracle_frame(oracle, sf, fr, mp, frame_mp, th, nnratio, order=None, n=None):
    """(nmatches, matches as MAP indices, in-view count) of one frame"""
    (inv, lvl, cosv, proj), v, order = oracle_frustum(oracle, sf, fr, mp, frame_mp, order, n)
    mpv = ola.MapPointView(mp.desc[order], proj[:, 0], proj[:, 1], proj[:, 2], lvl * inv, cosv, mbTrackInView=inv, isBad=mp.bad[order], obs=mp.obs[order])
    if len(order) == 0:
        return 0, np.full(v.N, -1, np.int32), 0
    nm, m = oracle.search_local_map(v, mpv, th, nnratio)
    return nm, np.where(m >= 0, order[np.maximum(m, 0)], -1).astype(np.int32), int(inv.sum())


# ---- device side --------------------------------------------------------------------------------------------------------------------------
class DeviceBatch:
    """frames, map and (optionally) mvpMapPoints / per-frame lists as the device arrays of the two entries; counts may shorten or overstate a frame"""

    def __init__(self, ctx, frames, mp, frame_mp=None, lists=None, img_stride=1, counts=None):
        import torch
        self.ctx, self.n, self.st, cap = ctx, len(frames), img_stride, ctx.orb_capacity
        self.cap = cap
        nf, ni = self.n, max(self.n * img_stride, 1)
        rng = np.random.default_rng(5)
        kps = np.zeros((ni, cap), KEYPOINT_DTYPE)
        kps["octave"] = 99                                   # rows nothing may read: images between the frames, features past the count
        desc = rng.integers(0, 256, (ni, cap, 32), dtype=np.uint8)
        cnt = np.full(ni, 17, np.int32)
        ur, Tcw = np.full((max(nf, 1), cap), 5.0, f32), np.zeros((max(nf, 1), 4, 4), f32)
        fmp = np.full((max(nf, 1), cap), 3, np.int32)         # (past N: a live index nothing may read)
        for j, fr in enumerate(frames):
            m = len(fr.keys)
            assert m <= cap
            kps[j * img_stride, :m], desc[j * img_stride, :m] = fr.keys, fr.desc
            cnt[j * img_stride] = m if counts is None or counts[j] is None else counts[j]
            ur[j, :m], Tcw[j] = fr.uright, fr.Tcw
            if frame_mp is not None:
                fmp[j, :m] = frame_mp[j]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.kps, self.desc, self.counts = up(kps.view(np.uint8).reshape(ni, cap, 28)), up(desc), up(cnt)
        self.uright, self.Tcw = up(ur), up(Tcw)
        self.frame_mp = up(fmp) if frame_mp is not None else None
        u8 = lambda a: up(np.asarray(a, np.uint8))
        lo = li = None
        if lists is not None:
            lo = up(np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32))
            li = up(np.concatenate([np.asarray(x, np.int32) for x in lists] + [np.zeros(0, np.int32)]).astype(np.int32))
        self.map = matcher.LocalMapDev(up(mp.world), up(mp.normal), up(mp.maxd), up(mp.mind), up(mp.desc), u8(mp.obs), u8(mp.bad), lo, li, n_mp=mp.n)
        self.offs = torch.full((max(nf, 1), _lib.GRID_CELLS + 1), -5, dtype=torch.int32, device="cuda")
        self.idx = torch.full((max(nf, 1), cap), -5, dtype=torch.int32, device="cuda")
        if nf:
            with matcher._torch_stream() as s:
                _lib.check(lib().olf_frame_grid_dev(ctx.handle, nf, img_stride, self.kps.data_ptr(), self.counts.data_ptr(), *BOUNDS, self.offs.data_ptr(),
                                                    self.idx.data_ptr(), s), "olf_frame_grid_dev")

    def search(self, th=1.0, nnratio=0.8, **kw):
        return matcher.search_local_map_batch(self.n, self.kps, self.desc, self.counts, self.uright, self.offs, self.idx, self.Tcw, self.map, CAM, BOUNDS,
                                              th=th, nnratio=nnratio, frame_mp=self.frame_mp, img_stride=self.st, context=self.ctx, **kw)

    def frustum(self, cos_limit=0.5, **kw):
        return matcher.is_in_frustum_batch(self.n, self.Tcw, self.map, CAM, BOUNDS, cos_limit, frame_mp=self.frame_mp, counts=self.counts, img_stride=self.st,
                                           context=self.ctx, **kw)


def assert_frame(res, j, exp, cap):
    m, n = res
    n_o, m_o = exp[0], exp[1]
    N = len(m_o)
    row = m[j].cpu().numpy()
    assert int(n[j].item()) == n_o
    assert np.array_equal(row[:N], m_o) and np.all(row[N:] == -1) and len(row) == cap


def check_sf(ctx):
    sf = scale_factors(ctx)
    assert np.array_equal(sf, SF8)
    return sf


# ---- 1: the frustum alone -----------------------------------------------------------------------------------------------------------------
def frustum_case():
    rng = np.random.default_rng(101)
    sf = SF8
    poses = [pose(), pose(tx=0.4, ty=-0.2, tz=1.5, ry_deg=12.0, rx_deg=-7.0), pose(tx=-2.0, tz=-3.0, ry_deg=-25.0), pose(ty=0.3, rx_deg=15.0, ry_deg=170.0)]
    frames = []
    for T in poses:
        fr = SynthFrame()
        fr.keys, fr.desc, fr.uright = np.zeros(40, KEYPOINT_DTYPE), np.zeros((40, 32), np.uint8), np.zeros(40, f32)
        fr.Tcw = T.astype(f32)
        frames.append(fr)
    world, normal, maxd, mind, group = [], [], [], [], []

    def add(name, P, N=None, ratio=None, lo=None):
        """points P (camera 0 = world coordinates), seen from the origin unless N says otherwise; maxd = dist * ratio"""
        P = np.atleast_2d(np.asarray(P, np.float64))
        d = np.linalg.norm(P, axis=1)
        world.append(P); normal.append(P / d[:, None] if N is None else N)
        r = rng.uniform(1.0, 3.5, len(P)) if ratio is None else np.broadcast_to(ratio, (len(P),))
        maxd.append(d * r); mind.append(d * r / sf[-1] if lo is None else np.broadcast_to(lo, (len(P),)) * d)
        group.extend([name] * len(P))

    def spread(n):                                            # points across and around the image of camera 0, 1 .. 25 m deep
        z = rng.uniform(1, 25, n)
        return np.stack([(rng.uniform(-60, 380, n) - CX) * z / FX, (rng.uniform(-50, 290, n) - CY) * z / FY, z], 1)
    add("spread", spread(500))
    add("behind", spread(40) * [1, 1, -1])
    # u or v exactly on a bound (closed: in view), and one float outside it.  z = 0.5: invz = 2; z = 1.25: 150 * 0.8f rounds to 120
    on = np.array([[-0.4, 0, 0.5], [0.4, 0, 0.5], [0, -0.75, 1.25], [0, 0.75, 1.25]], f32)
    add("on_bound", on)
    def first_outside(p, axis, step):                         # the first float past p[axis] whose projection leaves the bound (the reference's float chain)
        p = p.copy()
        for _ in range(64):
            p[axis] = np.nextafter(p[axis], f32(step))
            w = f32(f32(f32(f32(FX) * p[axis]) * f32(f32(1.0) / p[2])) + f32(CX if axis == 0 else CY))
            if w < 0 or w > f32(BOUNDS[1] if axis == 0 else BOUNDS[3]):
                return p
        raise AssertionError("no float outside the bound")
    add("off_bound", np.stack([first_outside(on[0], 0, -1), first_outside(on[1], 0, 1), first_outside(on[2], 1, -1), first_outside(on[3], 1, 1)]))
    add("too_far", spread(30), ratio=rng.uniform(0.3, 0.83, 30))            # dist > 1.2 * maxd
    add("too_near", spread(30), lo=rng.uniform(1.26, 3.0, 30))              # dist < 0.8 * mind
    add("edge_far", spread(30), ratio=rng.uniform(0.8330, 0.8337, 30))     # either side of 1 / 1.2
    for k in range(8):                                                     # every level: ratio just below sf[k]
        add("level%d" % k, spread(12) * [0.3, 0.3, 1], ratio=float(sf[k]) * 0.97)
    # viewing angles either side of the two limits, for camera 0: the normal is the direction to the point turned by acos(c)
    for name, c in (("cos_lo", rng.uniform(0.4990, 0.5010, 60)), ("cos_hi", rng.uniform(0.9975, 0.9985, 60))):
        P = spread(60) * [0.3, 0.3, 1]
        d = P / np.linalg.norm(P, axis=1)[:, None]
        t = np.cross(d, [0.0, 1.0, 0.0])
        t /= np.linalg.norm(t, axis=1)[:, None]
        add(name, P, N=d * c[:, None] + t * np.sqrt(1 - c * c)[:, None])
    mp = LocalMap.__new__(LocalMap)
    mp.world, mp.normal = np.concatenate(world).astype(f32), np.concatenate(normal).astype(f32)
    mp.maxd, mp.mind = np.concatenate(maxd).astype(f32), np.concatenate(mind).astype(f32)
    mp.n = len(mp.world)
    mp.desc = rng.integers(0, 256, (mp.n, 32), dtype=np.uint8)
    mp.obs, mp.bad = rng.random(mp.n) < 0.5, (rng.random(mp.n) < 0.1) & (np.array(group) == "spread")
    frame_mp = [rng.choice(np.flatnonzero(np.array(group) == "spread"), 40, replace=False).astype(np.int32) for _ in frames]
    frame_mp[1][:5] = -1
    return frames, mp, frame_mp, np.array(group)


def test_frustum_alone(oracle, ctx):
    sf = check_sf(ctx)
    frames, mp, frame_mp, group = frustum_case()
    assert 500 <= mp.n <= 4000
    exp = [oracle_frustum(oracle, sf, fr, mp, frame_mp[j])[0] for j, fr in enumerate(frames)]
    # floors, on the oracle's outputs (camera 0 is the one the groups were built for)
    inv0, lvl0, cos0, proj0 = exp[0]
    g = lambda name: group == name
    assert not inv0[g("behind")].any() and not inv0[g("too_far")].any() and not inv0[g("too_near")].any() and not inv0[g("off_bound")].any()
    assert inv0[g("on_bound")].all()
    pb = proj0[g("on_bound")]
    assert pb[0, 0] == 0.0 and pb[1, 0] == 320.0 and pb[2, 1] == 0.0 and pb[3, 1] == 240.0
    assert 0 < inv0[g("edge_far")].sum() < g("edge_far").sum()
    for name, lim in (("cos_lo", 0.5), ("cos_hi", 0.998)):
        c = cos0[g(name) & inv0]
        assert 0 < inv0[g(name)].sum() and (c > lim).any() and abs(c - lim).min() < 3e-4
    assert 0 < inv0[g("cos_lo")].sum() < g("cos_lo").sum() and (cos0[g("cos_hi") & inv0] <= 0.998).any()
    for k in range(8):
        assert (lvl0[inv0] == k).any()
    for j in range(len(frames)):
        assert exp[j][0].sum() >= (100 if j < 3 else 0)
        fm = frame_mp[j][frame_mp[j] >= 0]
        assert not exp[j][0][fm].any() and not exp[j][0][mp.bad].any()
    assert exp[3][0].sum() < exp[0][0].sum()                  # (camera 3 looks the other way)
    import torch
    db = DeviceBatch(ctx, frames, mp, frame_mp)
    sent = (torch.full((4 * mp.n,), 9, dtype=torch.uint8, device="cuda"), torch.full((4 * mp.n,), -9, dtype=torch.int32, device="cuda"),
            torch.full((4 * mp.n,), -9.0, dtype=torch.float32, device="cuda"), torch.full((4 * mp.n, 3), -9.0, dtype=torch.float32, device="cuda"))
    inv_d, lvl_d, cos_d, proj_d = (t.cpu().numpy().reshape((4, mp.n) + tuple(t.shape[1:])) for t in db.frustum(out=sent))
    for j in range(len(frames)):
        inv, lvl, cosv, proj = exp[j]
        assert np.array_equal(inv_d[j], inv.astype(np.uint8))
        assert np.array_equal(lvl_d[j][inv], lvl[inv])
        assert np.array_equal(cos_d[j][inv].view(np.uint32), cosv[inv].view(np.uint32))
        assert np.array_equal(proj_d[j][inv].view(np.uint32), proj[inv].view(np.uint32))
        assert np.all(lvl_d[j][~inv] == -9) and np.all(cos_d[j][~inv] == -9.0) and np.all(proj_d[j][~inv] == -9.0)      # a failed gate writes in view alone
    ctx.poll_status()


# ---- 2: plain search ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_case():
    rng = np.random.default_rng(211)
    frames = make_chain(rng, [pose(tx=0.03), pose(tz=-0.3, ry_deg=1.0), pose(tx=-0.02, ty=0.02), pose(ry_deg=-1.5)])
    mp = LocalMap(rng, frames, SF8)
    return frames, mp, mp.held(rng, frames, 0.3)


@functools.lru_cache(maxsize=None)
def plain_expect(oracle, nnratio):
    frames, mp, frame_mp = plain_case()
    return [oracle_frame(oracle, SF8, fr, mp, frame_mp[j], th, nnratio) if th else None for j, (fr, th) in enumerate(zip(frames, PLAIN_TH))]


PLAIN_TH = [1.0, 3.0, 5.0, 0.0, 1.0]


@pytest.mark.parametrize("nnratio", [0.8, 0.6])
def test_plain_search(oracle, ctx, nnratio):
    import torch
    check_sf(ctx)
    frames, mp, frame_mp = plain_case()
    assert 3 <= len(frames) <= 6 and 500 <= mp.n <= 4000 and all(300 <= len(f.keys) <= 1400 for f in frames)
    exp = plain_expect(oracle, nnratio)
    cap = ctx.orb_capacity
    assert all(e[0] >= 100 and (e[1] >= 0).sum() >= 100 for e in exp if e is not None), [e and e[0] for e in exp]
    out = (torch.full((5, cap), 7, dtype=torch.int32, device="cuda"), torch.full((5,), 7, dtype=torch.int32, device="cuda"))
    DeviceBatch(ctx, frames, mp, frame_mp, img_stride=2).search(th=9.0, nnratio=nnratio, d_th=torch.tensor(PLAIN_TH, dtype=torch.float32, device="cuda"), out=out)
    for j, e in enumerate(exp):
        if e is None:
            assert bool((out[0][j] == 7).all()) and int(out[1][j].item()) == 7          # the skipped frame's rows keep the sentinel
            continue
        assert_frame(out, j, e, cap)
    if nnratio == 0.6:
        assert any(not np.array_equal(a[1], b[1]) for a, b in zip(exp, plain_expect(oracle, 0.8)) if a is not None)      # the ratio decides matches
    ctx.poll_status()


# ---- 3: crowded and blocked ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crowded_case(obs_all):
    """1000 + points squeezed to 15 % of the image area, similar descriptors; 92 % of the features hold their own point"""
    rng = np.random.default_rng(307)
    frames = make_chain(rng, [pose(), pose(tx=0.01)], n=1000, n_dis=100, squeeze=float(np.sqrt(0.15)), similar=True, flips=3)
    mp = LocalMap(rng, frames, SF8, obs_p=1.0 if obs_all else 0.0, bad_p=0.02)
    return frames, mp, mp.held(rng, frames, 0.92)


def window_stats(sf, fr, mp, frame_mp, fr_exp, th, stop=(200, 50)):
    """queries with >= 16 window candidates, and queries (with a window) of which at most one candidate is not blocked at the start"""
    (inv, lvl, cosv, proj), v, _ = fr_exp
    blocked = v.mp_valid & v.mp_obs
    big = few = 0
    for i in np.flatnonzero(inv):
        r = f32(f32(2.5 if cosv[i] > 0.998 else 4.0) * f32(th)) * sf[lvl[i]]
        cand = v.GetFeaturesInArea(proj[i, 0], proj[i, 1], r, lvl[i] - 1, lvl[i])
        big += len(cand) >= 16
        few += len(cand) >= 2 and (~blocked[cand]).sum() <= 1
        if big >= stop[0] and few >= stop[1]:
            break
    return big, few


@pytest.mark.parametrize("obs_all", [True, False])
def test_crowded_and_blocked(oracle, ctx, obs_all):
    sf = check_sf(ctx)
    frames, mp, frame_mp = crowded_case(obs_all)
    assert all(len(f.keys) <= 1400 for f in frames) and mp.n <= 4000
    th = 5.0
    exp = [oracle_frame(oracle, sf, fr, mp, frame_mp[j], th, 0.8) for j, fr in enumerate(frames)]
    if obs_all:
        for j, fr in enumerate(frames):
            fe = oracle_frustum(oracle, sf, fr, mp, frame_mp[j])
            assert (fe[1].mp_valid & fe[1].mp_obs).mean() > 0.8
            big, few = window_stats(sf, fr, mp, frame_mp[j], fe, th)
            assert big >= 200 and few >= 50, (j, big, few)
            assert exp[j][0] >= 20
    else:
        assert any(e[0] > (e[1] >= 0).sum() for e in exp)      # nothing blocks: features are reassigned, and nmatches counts every event
        assert all(e[0] >= 20 for e in exp)
    res = DeviceBatch(ctx, frames, mp, frame_mp).search(th=th)
    for j in range(len(frames)):
        assert_frame(res, j, exp[j], ctx.orb_capacity)


# ---- 4: order -----------------------------------------------------------------------------------------------------------------------------
def test_order_of_the_lists(oracle, ctx):
    sf = check_sf(ctx)
    rng = np.random.default_rng(401)
    # one scene seen twice: the map holds both frames' points, so two points -- descriptors 3 bits apart -- compete for every feature of the second frame
    chain = make_chain(rng, [pose()], n=450, n_dis=0, squeeze=float(np.sqrt(0.15)), similar=True, flips=3)
    fr = chain[1]
    mp = LocalMap(rng, chain, sf, obs_p=0.5, bad_p=0.05)
    frame_mp = [mp.held(rng, chain, 0.3)[1]] * 4
    a, b = np.arange(mp.n), rng.permutation(mp.n)
    sub = np.sort(rng.choice(mp.n, mp.n // 2, replace=False))
    lists = [a, b, np.zeros(0, np.int64), sub]
    exp = [oracle_frame(oracle, sf, fr, mp, frame_mp[0], 3.0, 0.8, order=o) for o in lists]
    assert exp[0][0] >= 100 and exp[1][0] >= 100 and not np.array_equal(exp[0][1], exp[1][1])      # the order decides matches
    assert exp[2][0] == 0 and 0 < exp[3][0]
    res = DeviceBatch(ctx, [fr] * 4, mp, frame_mp, lists=lists).search(th=3.0)
    for j in range(4):
        assert_frame(res, j, exp[j], ctx.orb_capacity)
    res = DeviceBatch(ctx, [fr] * 2, mp, frame_mp[:2]).search(th=3.0)             # list_offsets = NULL: every frame sees the map in index order
    for j in range(2):
        assert_frame(res, j, exp[0], ctx.orb_capacity)


# ---- 5: ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th,nnratio", [(1.0, 0.8), (3.0, 0.6), (3.0, 1.0)])
def test_ties(oracle, ctx, th, nnratio):
    """duplicated features, the copy 0 or 2 bits away on the same or a neighbouring octave: equal distances (the scan-order tie-break), and the ratio rule
    that holds between equal levels only"""
    sf = check_sf(ctx)
    rng = np.random.default_rng(503)
    frames = make_chain(rng, [pose(tx=0.02), pose()], n=300, n_dis=40)
    mp = LocalMap(rng, frames, sf, obs_p=0.5, bad_p=0.05)      # (the map: the features before they are doubled)
    for f in frames:
        _dup(f, rng)
    frame_mp = [np.where(rng.random(len(f.keys)) < 0.2, rng.integers(0, mp.n, len(f.keys)), -1).astype(np.int32) for f in frames]
    exp = [oracle_frame(oracle, sf, fr, mp, frame_mp[j], th, nnratio) for j, fr in enumerate(frames)]
    assert all(e[0] >= 100 for e in exp)
    res = DeviceBatch(ctx, frames, mp, frame_mp).search(th=th, nnratio=nnratio)
    for j in range(len(frames)):
        assert_frame(res, j, exp[j], ctx.orb_capacity)


# ---- 6: degenerate shapes and malformed indices -------------------------------------------------------------------------------------------
def empty_map():
    mp = LocalMap.__new__(LocalMap)
    mp.world, mp.normal, mp.maxd, mp.mind = np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros(0, f32)
    mp.desc, mp.obs, mp.bad, mp.n = np.zeros((0, 32), np.uint8), np.zeros(0, bool), np.zeros(0, bool), 0
    return mp


def test_no_map_points(ctx):
    import torch
    frames, _, _ = plain_case()
    cap = ctx.orb_capacity
    out = (torch.full((2, cap), 7, dtype=torch.int32, device="cuda"), torch.full((2,), 7, dtype=torch.int32, device="cuda"))
    DeviceBatch(ctx, frames[:2], empty_map()).search(out=out)
    assert bool((out[0] == -1).all()) and bool((out[1] == 0).all())
    out = (torch.full((2, cap), 7, dtype=torch.int32, device="cuda"), torch.full((2,), 7, dtype=torch.int32, device="cuda"))
    DeviceBatch(ctx, [], empty_map()).search(out=out)           # n_frames = 0: nothing is written
    torch.cuda.synchronize()
    assert bool((out[0] == 7).all()) and bool((out[1] == 7).all())


@pytest.mark.parametrize("shape", ["one_frame", "zero_keys", "count_above_capacity"])
def test_short_shapes(oracle, ctx, shape):
    sf = check_sf(ctx)
    frames, mp, frame_mp = plain_case()
    cap = ctx.orb_capacity
    if shape == "one_frame":
        res = DeviceBatch(ctx, frames[:1], mp, frame_mp[:1]).search()
        assert_frame(res, 0, plain_expect(oracle, 0.8)[0], cap)
        return
    if shape == "zero_keys":
        res = DeviceBatch(ctx, frames[:2], mp, frame_mp[:2], counts=[0, None]).search(th=3.0)
        assert int(res[1][0].item()) == 0 and bool((res[0][0] == -1).all())
        assert_frame(res, 1, plain_expect(oracle, 0.8)[1], cap)
        return
    # a count beyond the capacity is read as the capacity
    rng = np.random.default_rng(601)
    fr = first_frame(rng, cap)
    mp1 = LocalMap(rng, [fr], sf, bad_p=0.05)
    fm = mp1.held(rng, [fr], 0.3)
    exp = oracle_frame(oracle, sf, fr, mp1, fm[0], 1.0, 0.8)
    assert exp[0] >= 100
    res = DeviceBatch(ctx, [fr], mp1, fm, counts=[cap + 1000]).search()
    assert_frame(res, 0, exp, cap)


def test_malformed_indices(oracle, ctx):
    """a list index outside the map is left out, a mvpMapPoints value beyond the map counts as none; bit 512 reports either, nothing else changes"""
    sf = check_sf(ctx)
    frames, mp, frame_mp = plain_case()
    frames, frame_mp = frames[:2], [x.copy() for x in frame_mp[:2]]
    rng = np.random.default_rng(607)
    order = [rng.permutation(mp.n), rng.permutation(mp.n)]
    cap = ctx.orb_capacity
    ctx.poll_status()
    # lists: frame 0 carries two indices outside the map
    bad_list = np.concatenate([order[0][:50], [mp.n, -1], order[0][50:]])
    exp = [oracle_frame(oracle, sf, frames[j], mp, frame_mp[j], 1.0, 0.8, order=order[j]) for j in range(2)]
    assert all(e[0] >= 100 for e in exp)
    res = DeviceBatch(ctx, frames, mp, frame_mp, lists=[bad_list, order[1]]).search()
    for j in range(2):
        assert_frame(res, j, exp[j], cap)
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert e.value.code == OLF_ERR_CAPACITY and "flags=512" in str(e.value) and describes(e.value, 512)
    ctx.poll_status()
    # mvpMapPoints: a value beyond the map holds nothing
    hold = np.flatnonzero(frame_mp[1] >= 0)[:7]
    frame_mp[1][hold] = mp.n + np.arange(7) * 1000
    exp1 = oracle_frame(oracle, sf, frames[1], mp, frame_mp[1], 1.0, 0.8, order=order[1])
    assert not np.array_equal(exp1[1], exp[1][1])
    res = DeviceBatch(ctx, frames, mp, frame_mp, lists=order).search()
    assert_frame(res, 0, exp[0], cap)
    assert_frame(res, 1, exp1, cap)
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert "flags=512" in str(e.value) and describes(e.value, 512)


def test_error_codes(ctx):
    import torch
    frames, mp, frame_mp = plain_case()
    db = DeviceBatch(ctx, frames[:2], mp, frame_mp[:2])
    full = dict(kps=db.kps, desc=db.desc, counts=db.counts, uright=db.uright, cell_offsets=db.offs, cell_index=db.idx, Tcw=db.Tcw)
    m = torch.full((2, ctx.orb_capacity), -1, dtype=torch.int32, device="cuda")
    n = torch.zeros(2, dtype=torch.int32, device="cuda")
    v, l = torch.zeros(2 * mp.n, dtype=torch.uint8, device="cuda"), torch.zeros(2 * mp.n, dtype=torch.int32, device="cuda")
    c, p = torch.zeros(2 * mp.n, dtype=torch.float32, device="cuda"), torch.zeros((2 * mp.n, 3), dtype=torch.float32, device="cuda")

    def fill(skip=None, bounds=BOUNDS):
        t = _lib.TrackBatchC()
        for k, x in full.items():
            setattr(t, k, None if k == skip else x.data_ptr())
        t.img_stride = 1
        t.fx, t.fy, t.cx, t.cy, t.mbf = CAM
        t.minX, t.maxX, t.minY, t.maxY = bounds
        return t

    def lmap(skip=None):
        lm = db.map.c(2)
        if skip:
            setattr(lm, skip, None)
        return lm

    def search(t, lm, mm=m, nn=n, h=ctx.handle):
        return lib().olf_search_local_map_batch_dev(h, C.byref(t), 2, C.byref(lm), db.frame_mp.data_ptr(), 0.5, 1.0, None, 0.8,
                                                    mm.data_ptr() if mm is not None else None, nn.data_ptr() if nn is not None else None, None)

    def frustum(t, lm, vv=v):
        return lib().olf_is_in_frustum_batch_dev(ctx.handle, C.byref(t), 2, C.byref(lm), db.frame_mp.data_ptr(), 0.5, vv.data_ptr() if vv is not None else None,
                                                 l.data_ptr(), c.data_ptr(), p.data_ptr(), None)
    torch.cuda.synchronize()                                # (stream NULL = the context's own stream)
    assert search(fill(), lmap()) == 0 and frustum(fill(), lmap()) == 0
    for k in full:
        assert search(fill(skip=k), lmap()) == OLF_ERR_INVALID, k
    for k in ("world", "normal", "maxd", "mind", "desc", "obs", "bad"):
        assert search(fill(), lmap(skip=k)) == OLF_ERR_INVALID, k
    for k in ("world", "normal", "maxd", "mind", "bad"):
        assert frustum(fill(), lmap(skip=k)) == OLF_ERR_INVALID, k
    assert frustum(fill(skip="Tcw"), lmap()) == OLF_ERR_INVALID and frustum(fill(), lmap(), None) == OLF_ERR_INVALID
    assert search(fill(), lmap(), None) == OLF_ERR_INVALID and search(fill(), lmap(), m, None) == OLF_ERR_INVALID
    assert search(fill(), lmap(), h=None) == OLF_ERR_INVALID
    for b in ((320.0, 320.0, 0.0, 240.0), (0.0, 320.0, 240.0, 0.0)):
        assert search(fill(bounds=b), lmap()) == OLF_ERR_INVALID and frustum(fill(bounds=b), lmap()) == OLF_ERR_INVALID
    lm = lmap()
    lm.list_offsets, lm.list_index, lm.n_entries = db.offs.data_ptr(), None, 5       # lists without their indices
    assert search(fill(), lm) == OLF_ERR_INVALID
    ctx.synchronize()
    big_p = _lib.default_params()
    big_p.orb.nfeatures = _lib.GRID_MAX_KEYS + 1
    big = _lib.Context(big_p, W, H, 1)
    try:
        assert big.orb_capacity > _lib.GRID_MAX_KEYS
        assert search(fill(), lmap(), h=big.handle) == OLF_ERR_CAPACITY           # (refused before anything is read)
    finally:
        big.close()


# ---- 7: the loop of host entries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_grid", [False, True])
def test_equals_loop_of_host_entries(ctx, own_grid):
    """the batch entry against olf_is_in_frustum + olf_search_local_map, frame by frame, the host search walking a supplied grid or building its own"""
    sf = check_sf(ctx)
    frames, mp, frame_mp = plain_case()
    frames, frame_mp = frames[:3], frame_mp[:3]
    res = DeviceBatch(ctx, frames, mp, frame_mp).search(th=3.0)
    geom = ola.MapPointGeom(mp.world, mp.normal, mp.maxd, mp.mind, mp.desc, skip=mp.bad)
    for j, fr in enumerate(frames):
        v = fr.view(sf)
        if not own_grid:
            v.attach_grid(*ola.assign_features_to_grid(v.mvKeysUn, BOUNDS, context=ctx))
        mpv = ola.matcher.isInFrustum(v, geom, 0.5)
        fm = frame_mp[j].astype(np.int64)
        live = fm >= 0
        live[live] &= ~mp.bad[fm[live]]
        held = np.zeros(mp.n, bool)
        held[fm[live]] = True
        mpv.mbTrackInView &= ~mp.bad & ~held
        mpv.mnTrackScaleLevel[~mpv.mbTrackInView] = 0
        mpv.obs = mp.obs.copy()
        v.mp_valid[:] = live
        v.mp_obs[live] = mp.obs[fm[live]]
        n_h, m_h = ola.ORBmatcher(0.8, context=ctx).SearchByProjection(v, mpv, 3.0)
        assert n_h >= 100
        assert_frame(res, j, (n_h, m_h), ctx.orb_capacity)
