"""GPU parity: olf_search_for_triangulation_batch_dev -- ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:659-825) for a list of key-frame pairs of a
device-resident batch, Frame::ComputeBoW included -- against the CPU oracle's SearchForTriangulation on the oracle's own feature vectors, pair by pair.
Equality is exact.  The frames of tests 1 to 4 are fabricated (the entry takes arbitrary device arrays); every scenario_* function builds one case,
asserts from the oracle's output or a numpy count that the case occurs, and needs no GPU."""
import functools
import types
import numpy as np
import pytest
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, matcher
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, OLF_ERR_CAPACITY, lib
from status_text import describes

pytestmark = pytest.mark.gpu

W, H = 320, 240
FX = FY = 200.0
CX, CY = 160.0, 120.0
CAM = (FX, FY, CX, CY)
f32 = np.float32
COUNTS6 = (0, 1, 63, 64, 65, 300)


def scale_factors(n=8):
    """mvScaleFactor as ORBextractor builds it (src/ORBextractor.cc:423-428): sf[i] = float(sf[i - 1] * double(1.2f))"""
    sf = np.ones(n, f32)
    for i in range(1, n):
        sf[i] = f32(float(sf[i - 1]) * float(f32(1.2)))
    return sf


SF = scale_factors()


# ---- fabricated frames ----------------------------------------------------------------------------------------------------------------
def _flip(rng, d, max_bits):
    d = d.copy()
    for r in range(len(d)):
        for b in rng.choice(256, int(rng.integers(0, max_bits + 1)), replace=False):
            d[r, b // 8] ^= np.uint8(1 << (b % 8))
    return d


def make_frames(counts, seed, pool=320):
    """Frames that observe subsets of one pool of points: descriptors 0 to 12 bits from the point's, positions after a sideways translation of 0.05 m
    per frame (near-horizontal epipolar lines), vertical offsets from 0 to 12 px (the 3.84 sigma^2 gate is 1.96 to 7 px wide), octaves 0 to 7, 40 % mono,
    40 % with a map point; angles follow the point's, three in ten are random (those matches leave the three main rotation bins)."""
    rng = np.random.default_rng(seed)
    # (the pool's descriptors form 12 clusters, 40 bits around a centre each: two views of a point then mostly descend to the same vocabulary node)
    base = rng.integers(0, 256, (12, 32), dtype=np.uint8)[rng.integers(0, 12, pool)]
    for r in range(pool):
        for b in rng.choice(256, 40, replace=False):
            base[r, b // 8] ^= np.uint8(1 << (b % 8))
    bx, by, bz, bang = rng.uniform(40, 290, pool), rng.uniform(25, 215, pool), rng.uniform(2, 20, pool), rng.uniform(0, 360, pool)
    frames = []
    for j, n in enumerate(counts):
        fr = types.SimpleNamespace()
        fr.obs = rng.permutation(pool if n > 70 else 70)[:n]        # (the small frames share the first 70 points)
        o = fr.obs
        fr.desc = _flip(rng, base[o], 12)
        k = np.zeros(n, KEYPOINT_DTYPE)
        tx = 0.05 * j
        k["x"] = (bx[o] - FX * tx / bz[o]).astype(f32)
        k["y"] = (by[o] + rng.choice([0, 0, 0.3, 0.3, 0.8, 0.8, 1.5, 1.5, 2.5, 4.0, 7.0, 12.0], n) * rng.choice([-1.0, 1.0], n)).astype(f32)
        k["octave"] = rng.integers(0, 8, n)
        ang = ((bang[o] + np.where(rng.random(n) < 0.7, rng.normal(0, 3, n), rng.uniform(0, 360, n))) % 360).astype(f32)
        ang[ang >= 360] = 0
        k["angle"], k["size"], k["class_id"] = ang, 31, -1
        fr.keys = k
        fr.uright = np.where(rng.random(n) < 0.4, -1.0, k["x"] - 40.0 / bz[o]).astype(f32)
        fr.valid = rng.random(n) < 0.4
        fr.Tcw = np.eye(4, dtype=f32)
        fr.Tcw[0, 3], fr.Tcw[2, 3] = -tx, 0.004 * j
        frames.append(fr)
    return frames, base


def fundamental(T1, T2, cam=CAM):
    """LocalMapping::ComputeF12 (src/LocalMapping.cc:719-738): R12 = R1w R2w^T, t12 = -R12 t2w + t1w, F12 = K^-T [t12]x R12 K^-1, used as x1^T F12 x2"""
    T1, T2 = T1.astype(np.float64), T2.astype(np.float64)
    R12 = T1[:3, :3] @ T2[:3, :3].T
    t = -R12 @ T2[:3, 3] + T1[:3, 3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]], np.float64))
    return (Ki.T @ tx @ R12 @ Ki).astype(f32)


def camera_centre(T):
    """-Rcw.t() * tcw as cv::Mat forms it: double accumulation, one rounding"""
    out = np.zeros(3, f32)
    for r in range(3):
        acc = 0.0
        for k in range(3):
            acc += float(T[k, r]) * float(T[k, 3])
        out[r] = f32(-acc)
    return out


@functools.lru_cache(maxsize=None)
def _tree(k, L):
    import oracle_lib
    return oracle_lib.random_vocabulary(k, L, 31)


def make_voc(k, L, base, seed=5):
    """centroids drawn from the pool; every 7th word has weight 0 (its features are in no FeatureVector)"""
    import oracle_lib
    parent, leaf, vdesc, weight = _tree(k, L)
    rng = np.random.default_rng(seed)
    vdesc = vdesc.copy()
    vdesc[1:] = base[rng.integers(0, len(base), len(parent) - 1)]
    weight = weight.copy()
    weight[np.flatnonzero(leaf)[::7]] = 0.0
    return (k, L, parent, leaf, vdesc, weight), oracle_lib.OracleVoc.create(k, L, parent, leaf, vdesc, weight)


def view(fr, V, levelsup, cam=CAM, sf=SF):
    n = len(fr.keys)
    v = types.SimpleNamespace(N=n, mvKeysUn=fr.keys, mDescriptors=fr.desc, mvuRight=fr.uright, mp_valid=fr.valid, mvScaleFactors=sf, mTcw=fr.Tcw)
    v.fx, v.fy, v.cx, v.cy = (f32(c) for c in cam)
    v.mFeatVec = V.transform(fr.desc, levelsup)[1] if n else {}
    return v


def expected_row(n1, pairs):
    row = np.full(n1, -1, np.int32)
    for a, b in pairs:
        row[a] = b
    return row


def oracle_pairs(views, frames, pairs, only_stereo, check, Cw=None):
    import oracle_lib
    out = []
    for p, (a, b) in enumerate(pairs):
        cw = camera_centre(frames[a].Tcw) if Cw is None else Cw[p]
        n, mp = oracle_lib.search_for_triangulation(views[a], views[b], fundamental(frames[a].Tcw, frames[b].Tcw), only_stereo, cw, checkOri=check)
        out.append((n, expected_row(views[a].N, mp)))
    return out


def gated_minima(v1, v2, F12, Cw, only_stereo):
    """numpy mirror of the candidate gate in float32, for counting cases only: {idx1: [(position in key frame 2's list, chunk of 64 inside the node's
    segment, idx2) of every gated candidate at the minimum distance]}"""
    C2 = (v2.mTcw[:3, :3].astype(np.float64) @ np.asarray(Cw, np.float64) + v2.mTcw[:3, 3]).astype(f32)
    invz = f32(1.0) / C2[2]
    ex, ey = v2.fx * C2[0] * invz + v2.cx, v2.fy * C2[1] * invz + v2.cy
    F = np.asarray(F12, f32).reshape(9)
    pos0, at = {}, 0
    for node in sorted(v2.mFeatVec):
        pos0[node] = at
        at += len(v2.mFeatVec[node])
    res = {}
    for node, l1 in v1.mFeatVec.items():
        if node not in v2.mFeatVec:
            continue
        c = np.asarray(v2.mFeatVec[node])
        k2 = v2.mvKeysUn[c]
        st2 = v2.mvuRight[c] >= 0
        s = v2.mvScaleFactors[k2["octave"]]
        for i in l1:
            st1 = v1.mvuRight[i] >= 0
            if v1.mp_valid[i] or (only_stereo and not st1):
                continue
            ok = ~v2.mp_valid[c] & (st2 | (not only_stereo))
            dist = np.unpackbits(v1.mDescriptors[i][None] ^ v2.mDescriptors[c], axis=1).sum(1)
            ok &= dist <= 50
            dx, dy = ex - k2["x"], ey - k2["y"]
            if not st1:
                ok &= st2 | ~(dx * dx + dy * dy < f32(100) * s)
            x1, y1 = v1.mvKeysUn["x"][i], v1.mvKeysUn["y"][i]
            a, b, cc = x1 * F[0] + y1 * F[3] + F[6], x1 * F[1] + y1 * F[4] + F[7], x1 * F[2] + y1 * F[5] + F[8]
            num, den = a * k2["x"] + b * k2["y"] + cc, a * a + b * b
            ok &= (den != 0) & ((num * num / den).astype(np.float64) < 3.84 * (s * s).astype(np.float64)) if den != 0 else False
            if ok.any():
                best = dist[ok].min()
                res[i] = [(pos0[node] + int(r), int(r) // 64, int(c[r])) for r in np.flatnonzero(ok & (dist == best))]
    return res


# ---- scenarios (CPU only) ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames6():
    return make_frames(COUNTS6, 17)


ALL_PAIRS = [(i, j) for i in range(6) for j in range(6) if i != j]


@functools.lru_cache(maxsize=None)
def scenario_all_pairs(k, L, levelsup, only_stereo, check):
    frames, base = frames6()
    voc, V = make_voc(k, L, base)
    views = [view(fr, V, levelsup) for fr in frames]
    exp = oracle_pairs(views, frames, ALL_PAIRS, only_stereo, check)
    total = sum(n for n, _ in exp)
    assert total > 0
    if check:
        free = oracle_pairs(views, frames, ALL_PAIRS, only_stereo, False)
        assert sum(n for n, _ in free) > total              # the histogram drops matches somewhere
    return frames, voc, exp


@functools.lru_cache(maxsize=None)
def scenario_ties():
    """one node (the root) holds every feature; 40 features of key frame 2 exist twice, 150 list places apart, both on the epipolar line"""
    frames, base = make_frames((400, 400), 23, pool=400)
    f1, f2 = frames
    where1 = {int(p): i for i, p in enumerate(f1.obs)}
    for t in range(40):
        a, b, i1 = t, 150 + t, where1[int(f2.obs[t])]
        f1.valid[i1] = f2.valid[a] = False
        f2.keys["y"][a] = f1.keys["y"][i1]
        f2.keys[b], f2.desc[b], f2.uright[b], f2.valid[b] = f2.keys[a], f2.desc[a], f2.uright[a], False
        f2.keys["x"][b] += 5
    voc, V = make_voc(3, 2, base)
    views = [view(fr, V, 4) for fr in frames]
    assert list(views[1].mFeatVec) == [0] and len(views[1].mFeatVec[0]) > 4 * 64      # the root, and a query spans 5 chunks
    exp = oracle_pairs(views, frames, [(0, 1), (1, 0)], False, True)
    ties = {i: c for i, c in gated_minima(views[0], views[1], fundamental(f1.Tcw, f2.Tcw), camera_centre(f1.Tcw), False).items() if len(c) > 1}
    assert len(ties) >= 10
    assert sum(1 for c in ties.values() if len({chunk for _, chunk, _ in c}) > 1) >= 5
    free = oracle_pairs(views, frames, [(0, 1)], False, False)[0][1]
    for i, c in ties.items():
        assert free[i] == max(c)[2]                         # the oracle keeps the later one
    return frames, voc, exp


@functools.lru_cache(maxsize=None)
def scenario_epipole():
    """key frame 2 half a metre ahead of key frame 1: the epipole is the image centre; 60 mono features of key frame 2 lie within 1.5 px of it, where
    every epipolar line passes"""
    import oracle_lib
    frames, base = make_frames((300, 300), 29, pool=300)
    f1, f2 = frames
    rng = np.random.default_rng(3)
    c, s = np.cos(0.02), np.sin(0.02)
    f1.Tcw[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], f32)
    f1.Tcw[:3, 3] = (0.1, -0.05, 0.2)
    T21 = np.eye(4)
    T21[2, 3] = -0.5                                        # camera 2 = camera 1 moved 0.5 m along its optical axis
    f2.Tcw = (T21 @ f1.Tcw.astype(np.float64)).astype(f32)
    where1 = {int(p): i for i, p in enumerate(f1.obs)}
    for t in range(60):
        i1 = where1[int(f2.obs[t])]
        f1.valid[i1] = f2.valid[t] = False
        f1.uright[i1] = f2.uright[t] = -1.0
        f2.keys["x"][t], f2.keys["y"][t] = CX + rng.uniform(-1.5, 1.5), CY + rng.uniform(-1.5, 1.5)
        f2.keys["octave"][t] = rng.integers(2, 8)
    voc, V = make_voc(10, 3, base)
    views = [view(fr, V, 2) for fr in frames]
    Cw = camera_centre(f1.Tcw)[None]
    exp = oracle_pairs(views, frames, [(0, 1)], False, True, Cw)
    far = oracle_pairs(views, frames, [(0, 1)], False, True, np.array([[1000.0, 0.0, 0.0]], f32))
    assert exp[0][0] > 0 and not np.array_equal(exp[0][1], far[0][1])      # the epipole gate decides matches
    return frames, voc, exp, Cw


@functools.lru_cache(maxsize=None)
def scenario_edges():
    frames, base = frames6()
    frames = list(frames)
    voc, V = make_voc(10, 3, base)
    views = [view(fr, V, 2) for fr in frames]
    good = [(5, 3), (3, 5), (1, 5), (2, 4), (0, 5), (5, 0), (4, 5), (6, 4)]
    n45, row45 = oracle_pairs(views, frames, [(4, 5)], False, True)[0]
    assert n45 > 0
    bad = types.SimpleNamespace(**{k: np.copy(v) for k, v in vars(frames[5]).items()})
    bad.keys["octave"][row45[row45 >= 0][0]] = 9            # a feature of frame 5 that frame 4 matches: a candidate for certain
    frames.append(bad)
    views.append(view(bad, V, 2))
    exp = dict(zip(good, oracle_pairs(views, frames, good, False, True)))
    assert sum(exp[p][0] for p in good) > 0
    return frames, voc, exp


# ---- device side ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    p = _lib.default_params()
    p.orb.nfeatures = 400
    c = _lib.Context(p, W, H, 2)
    assert 400 <= c.orb_capacity <= 4096 and c.nlevels == 8
    sf = np.zeros(8, f32)
    lib().olf_orb_scale_tables(c.handle, sf.ctypes.data, None, None, None, None)
    assert np.array_equal(sf, SF)
    yield c
    c.close()


class DeviceFrames:
    """fabricated frames as the device arrays of olf_track_batch; rows nothing may read hold octave 99, random descriptors and no map point"""

    def __init__(self, ctx, frames, img_stride=1):
        import torch
        cap, nf = ctx.orb_capacity, len(frames)
        self.ctx, self.n, self.st, self.cap = ctx, nf, img_stride, cap
        rng = np.random.default_rng(5)
        kps = np.zeros((nf * img_stride, cap), KEYPOINT_DTYPE)
        kps["octave"] = 99
        desc = rng.integers(0, 256, (nf * img_stride, cap, 32), dtype=np.uint8)
        cnt = np.full(nf * img_stride, 17, np.int32)
        ur, valid, Tcw = np.full((nf, cap), 5.0, f32), np.zeros((nf, cap), np.uint8), np.zeros((nf, 4, 4), f32)
        for j, fr in enumerate(frames):
            m = len(fr.keys)
            assert m <= cap
            kps[j * img_stride, :m], desc[j * img_stride, :m], cnt[j * img_stride] = fr.keys, fr.desc, m
            ur[j, :m], valid[j, :m], Tcw[j] = fr.uright, fr.valid, fr.Tcw
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.kps, self.desc, self.counts = up(kps.view(np.uint8).reshape(nf * img_stride, cap, 28)), up(desc), up(cnt)
        self.uright, self.valid, self.Tcw = up(ur), up(valid), up(Tcw)
        self.F = lambda pairs: np.stack([fundamental(frames[a].Tcw, frames[b].Tcw) if 0 <= a < nf and 0 <= b < nf else np.zeros((3, 3), f32) for a, b in pairs])

    def search(self, G, pairs, levelsup, only_stereo=False, check=True, Cw=None, F12=None, valid=True, n_pairs=None):
        """(matches12 [len(pairs) + 1, cap], nmatches [len(pairs) + 1]) as numpy arrays: the outputs start as -7, the last row is a sentinel"""
        import torch
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
        P = len(pairs)
        d_pairs = up(np.asarray(pairs, np.int32).reshape(P, 2), np.int32)
        d_F = up(self.F(pairs) if F12 is None else F12, f32)
        if n_pairs is not None:
            d_pairs, d_F = d_pairs[:n_pairs], d_F[:n_pairs]
        out = (torch.full((P + 1, self.cap), -7, dtype=torch.int32, device="cuda"), torch.full((P + 1,), -7, dtype=torch.int32, device="cuda"))
        matcher.search_for_triangulation_batch(G, self.n, self.kps, self.desc, self.counts, self.uright, self.Tcw, d_pairs, d_F, CAM,
                                               Cw=None if Cw is None else up(Cw, f32), mp_valid=self.valid if valid else None,
                                               bOnlyStereo=only_stereo, checkOri=check, levelsup=levelsup, img_stride=self.st, out=out, context=self.ctx)
        torch.cuda.synchronize()
        return out[0].cpu().numpy(), out[1].cpu().numpy()


def assert_rows(m, nm, exp, at=None):
    for p, (n_o, row_o) in enumerate(exp):
        q = p if at is None else at[p]
        assert nm[q] == n_o, (q, nm[q], n_o)
        assert np.array_equal(m[q, :len(row_o)], row_o), (q, int(np.argmax(m[q, :len(row_o)] != row_o)))
        assert (m[q, len(row_o):] == -1).all()


# 1 -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [0, 1])
@pytest.mark.parametrize("only_stereo", [0, 1])
@pytest.mark.parametrize("k,L,levelsup", [(10, 3, 2), (10, 6, 4), (4, 4, 2)])
def test_all_ordered_pairs(ctx, k, L, levelsup, only_stereo, check):
    """every (i, j), i != j, of six frames with 0, 1, 63, 64, 65 and 300 features: each frame is key frame 1 five times and key frame 2 five times"""
    frames, voc, exp = scenario_all_pairs(k, L, levelsup, bool(only_stereo), bool(check))
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    m, nm = DeviceFrames(ctx, frames).search(G, ALL_PAIRS, levelsup, bool(only_stereo), bool(check))
    assert_rows(m, nm, exp)
    assert (m[-1] == -7).all() and nm[-1] == -7
    ctx.poll_status()
    G.clear()


# 2 -----------------------------------------------------------------------------------------------------------------------------------------
def test_ties_and_long_segments(ctx):
    """equal minima inside a chunk of 64 candidates and across chunks: the later list position wins, as `dist > bestDist -> continue` has it"""
    frames, voc, exp = scenario_ties()
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    m, nm = DeviceFrames(ctx, frames).search(G, [(0, 1), (1, 0)], 4)
    assert_rows(m, nm, exp)
    G.clear()


# 3 -----------------------------------------------------------------------------------------------------------------------------------------
def test_epipole_gate(ctx):
    """the epipole inside the image: with d_Cw given, and with d_Cw = NULL and the centre taken from key frame 1's Tcw"""
    frames, voc, exp, Cw = scenario_epipole()
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    dev = DeviceFrames(ctx, frames, img_stride=2)
    for cw in (Cw, None):
        m, nm = dev.search(G, [(0, 1)], 2, Cw=cw)
        assert_rows(m, nm, exp)
    G.clear()


# 4 -----------------------------------------------------------------------------------------------------------------------------------------
def test_edges_in_one_call(ctx):
    """F12 = 0, the empty frame on either side, pair indices out of range or equal, an octave outside the levels -- and the pairs beside them"""
    frames, voc, exp = scenario_edges()
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    dev = DeviceFrames(ctx, frames)
    good = list(exp)
    pairs = good[:3] + [(5, 4)] + good[3:5] + [(7, 1), (-1, 2), (3, 3)] + good[5:] + [(4, 6)]
    zero, refused_pair, refused_octave = 3, (6, 7, 8), len(pairs) - 1
    F12 = dev.F(pairs)
    F12[zero] = 0
    ctx.poll_status()
    m, nm = dev.search(G, pairs, 2, F12=F12)
    assert nm[zero] == 0 and (m[zero] == -1).all()
    for q in refused_pair + (refused_octave,):
        assert nm[q] == -1 and (m[q] == -7).all()
    at = [pairs.index(p) for p in good]
    assert_rows(m, nm, [exp[p] for p in good], at)
    assert (m[-1] == -7).all() and nm[-1] == -7            # nothing past either output array
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert e.value.code == OLF_ERR_CAPACITY and "flags=%d" % (256 | 2048) in str(e.value) and describes(e.value, 256, 2048)
    ctx.poll_status()                                       # reported once, then clear
    # each refusal alone sets its own bit
    m, nm = dev.search(G, [(7, 1)], 2)
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert nm[0] == -1 and "flags=2048" in str(e.value) and describes(e.value, 2048)
    m, nm = dev.search(G, [(4, 6)], 2)
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert nm[0] == -1 and "flags=256" in str(e.value) and describes(e.value, 256)
    # n_pairs = 0 writes nothing; mp_valid = NULL searches nothing
    m, nm = dev.search(G, [(5, 4)], 2, n_pairs=0)
    assert (m == -7).all() and (nm == -7).all()
    m, nm = dev.search(G, [(5, 4), (4, 5)], 2, valid=False)
    assert (m[:2] == -1).all() and (nm[:2] == 0).all() and (m[2] == -7).all() and nm[2] == -7
    ctx.poll_status()
    G.clear()


# 5, 6: extracted frames ------------------------------------------------------------------------------------------------------------------------
KITTI_CAM = (718.856, 718.856, 607.1928, 185.2157)
PAIRS4 = [(i, j) for i in range(4) for j in range(4) if i != j]


@pytest.fixture(scope="module")
def extracted(oracle):
    """4 stereo pairs at KITTI size, shifted copies of one scene; the host form's results for the 12 ordered pairs"""
    import torch
    from orb_line_slam_amd import synth
    w, h, B = 1242, 375, 4
    fe = ola.StereoFrontEnd(oracle.full_params(2000, 100), w, h, max_pairs=B)
    imgs = synth.stereo_batch(67, B, w, h)
    for i in range(1, B):
        imgs[2 * i:2 * i + 2] = np.roll(imgs[:2], 3 * i, axis=2)
    f = fe.frames(imgs)
    Tcw = np.stack([np.eye(4, dtype=f32)] * B)
    Tcw[:, 0, 3], Tcw[:, 2, 3] = -0.3 * np.arange(B), 0.004 * np.arange(B)
    F12 = np.stack([fundamental(Tcw[a], Tcw[b], KITTI_CAM) for a, b in PAIRS4])
    src = np.concatenate([f.pair(i)["mDescriptors"] for i in range(B)])
    parent, leaf, vdesc, weight = oracle.random_vocabulary(10, 3, 8)
    vdesc[1:] = src[np.random.default_rng(1).integers(0, len(src), len(parent) - 1)]
    G = ola.ORBVocabulary.from_arrays(10, 3, parent, leaf, vdesc, weight)
    mask = fe.stereo_points_mask()
    run = lambda: fe.search_for_triangulation_batch(G, Tcw, np.asarray(PAIRS4, np.int32), F12, KITTI_CAM, mp_valid=mask, levelsup=2)
    m, nm = run()
    torch.cuda.synchronize()
    kfs = []
    for i in range(B):
        g = f.pair(i)
        kf = ola.KeyFrameView(g["mvKeys"], g["mDescriptors"], g["mvuRight"], SF, bounds=(0.0, float(w), 0.0, float(h)), mTcw=Tcw[i])
        kf.mp_valid = g["mvDepth"] > 0
        _, kf.mFeatVec = G.transform(kf.mDescriptors, 2)
        kfs.append(kf)
    host = []
    for p, (a, b) in enumerate(PAIRS4):
        n, mp = ola.ORBmatcher(0.6, True).SearchForTriangulation(kfs[a], kfs[b], F12[p], False)
        host.append((n, expected_row(kfs[a].N, mp)))
    yield types.SimpleNamespace(fe=fe, G=G, mask=mask, run=run, m=m.cpu().numpy(), nm=nm.cpu().numpy(), host=host, B=B)
    G.clear()
    fe.ctx.close()


def test_extracted_frames_stride_2(extracted):
    """img_stride 2, mvuRight from the stereo matcher, mp_valid from olf_stereo_points_mask_dev: the batch equals the host form pair by pair"""
    e = extracted
    assert sum(n for n, _ in e.host) > 30 * len(PAIRS4)
    assert_rows(e.m, e.nm, e.host)


def test_shared_scratch_and_stage(extracted):
    """SearchByBoW, SearchForTriangulation, SearchByBoW on one stream: both share the FeatureVector stage and the context's batch scratch"""
    import torch
    e = extracted
    fb, B = e.fe._last_frames("test")
    cap, h = e.fe.ctx.orb_capacity, e.fe.ctx.handle
    bow = [(torch.full((B - 1, cap), -7, dtype=torch.int32, device="cuda"), torch.full((B - 1,), -7, dtype=torch.int32, device="cuda")) for _ in range(2)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        s = st.cuda_stream
        call = lambda o: _lib.check(lib().olf_search_by_bow_batch_dev(h, e.G._h, B, 2, fb.kps, fb.desc, fb.counts, e.mask.data_ptr(), None, 0.7, 1, 2,
                                                                      o[0].data_ptr(), o[1].data_ptr(), s), "olf_search_by_bow_batch_dev")
        call(bow[0])
        m, nm = e.run()
        call(bow[1])
    torch.cuda.synchronize()
    assert torch.equal(bow[0][0], bow[1][0]) and torch.equal(bow[0][1], bow[1][1]) and int(bow[0][1].sum()) > 0
    assert np.array_equal(m.cpu().numpy(), e.m) and np.array_equal(nm.cpu().numpy(), e.nm)
