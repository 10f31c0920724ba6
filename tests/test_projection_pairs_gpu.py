"""GPU parity: olf_search_by_projection_kf_pairs_dev -- ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
(src/ORBmatcher.cc:1620-1747, Tracking::Relocalization) for a list of (current frame, key frame) pairs -- and olf_search_by_projection_sim3_batch_dev --
SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:292-405, LoopClosing::ComputeSim3) for a batch of key frames.  Every expectation comes from the CPU
oracle pair by pair (oracle.search_by_projection_kf / search_by_projection_sim3, tests/projection_pairs_scenes.py); equality is exact on every row and
count.  The scenarios assert, without a GPU, that their cases really occur."""
import ctypes as C
import types
import numpy as np
import pytest
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, matcher
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, OLF_ERR_CAPACITY, lib
import projection_pairs_scenes as S
from projection_pairs_scenes import BOUNDS, CAM, FILL, f32
from status_text import describes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (the device tensors below)
    p = _lib.default_params()
    p.orb.nfeatures = 1400
    c = _lib.Context(p, S.W, S.H, 2)
    assert c.orb_capacity >= 1400
    sf = np.zeros(c.nlevels, np.float32)
    lib().olf_orb_scale_tables(c.handle, sf.ctypes.data_as(C.c_void_p), None, None, None, None)
    assert np.array_equal(sf, S.SF8)
    yield c
    c.close()


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(arrays, cap, fill, dtype):
    """per-pair (or per-frame) arrays over the capacity: positions past an array's length hold `fill`"""
    out = np.full((max(len(arrays), 1), cap), fill, dtype)
    for p, a in enumerate(arrays):
        out[p, :len(a)] = a
    return out


class Frames:
    """frames as the device arrays both entries read: key points, descriptors, counts and the grids; images between the frames and features past a count
    hold values that would change a result"""

    def __init__(self, ctx, kfs, img_stride=1, counts=None):
        import torch
        self.ctx, self.n, self.st, cap = ctx, len(kfs), img_stride, ctx.orb_capacity
        self.nf, ni = max(self.n, 1), max(self.n * img_stride, 1)
        rng = np.random.default_rng(5)
        kps = np.zeros((ni, cap), KEYPOINT_DTYPE)
        kps["x"], kps["y"], kps["octave"] = 160.0, 120.0, 3       # in the middle of every window
        desc = rng.integers(0, 256, (ni, cap, 32), dtype=np.uint8)
        cnt = np.full(ni, 17, np.int32)
        for j, kf in enumerate(kfs):
            assert kf.N <= cap
            kps[j * img_stride, :kf.N], desc[j * img_stride, :kf.N] = kf.mvKeysUn, kf.mDescriptors
            cnt[j * img_stride] = kf.N if counts is None or counts[j] is None else counts[j]
        self.kps, self.desc, self.counts = _up(kps.view(np.uint8).reshape(ni, cap, 28)), _up(desc), _up(cnt)
        self.offs = torch.full((self.nf, _lib.GRID_CELLS + 1), -5, dtype=torch.int32, device="cuda")
        self.idx = torch.full((self.nf, cap), -5, dtype=torch.int32, device="cuda")
        if self.n:
            with matcher._torch_stream() as s:
                _lib.check(lib().olf_frame_grid_dev(ctx.handle, self.n, img_stride, self.kps.data_ptr(), self.counts.data_ptr(), *BOUNDS, self.offs.data_ptr(),
                                                    self.idx.data_ptr(), s), "olf_frame_grid_dev")


class RelocBatch(Frames):
    """the frames of a relocalisation round: every one can stand on either side of a pair"""

    def __init__(self, ctx, kfs, img_stride=1, counts=None, own_desc=False):
        super().__init__(ctx, kfs, img_stride, counts)
        cap, nf = ctx.orb_capacity, self.nf
        rng = np.random.default_rng(6)
        Tcw = np.zeros((nf, 4, 4), f32)
        world, valid, bad = np.full((nf, cap, 3), 5.0, f32), np.ones((nf, cap), np.uint8), np.zeros((nf, cap), np.uint8)
        maxd, mind = np.full((nf, cap), 1e3, f32), np.full((nf, cap), 1e-3, f32)
        mdesc = rng.integers(0, 256, (nf, cap, 32), dtype=np.uint8)
        for j, kf in enumerate(kfs):
            m = kf.N
            Tcw[j] = kf.mTcw
            world[j, :m], valid[j, :m], bad[j, :m] = kf.mp_world, kf.mp_valid, kf.mp_bad
            maxd[j, :m], mind[j, :m], mdesc[j, :m] = kf.mp_maxd, kf.mp_mind, kf.mp_desc
        self.Tcw, self.world, self.valid, self.bad = _up(Tcw), _up(world), _up(valid), _up(bad)
        self.maxd, self.mind, self.mdesc = _up(maxd), _up(mind), None if own_desc else _up(mdesc)

    def search(self, pairs, poses, cur_valid, found, th, orb, ori, d_th=None, d_orb=None, n_frames=None):
        """(matches, nmatches) as numpy arrays; the outputs start from a fill no result equals.  poses None: the frames' own Tcw"""
        import torch
        cap, n = self.ctx.orb_capacity, len(pairs)
        m = torch.full((max(n, 1), cap), FILL, dtype=torch.int32, device="cuda")
        nm = torch.full((max(n, 1),), FILL, dtype=torch.int32, device="cuda")
        matcher.search_by_projection_kf_pairs(
            self.n if n_frames is None else n_frames, self.kps, self.desc, self.counts, self.offs, self.idx, self.world, self.maxd, self.mind,
            _up(np.asarray(pairs, np.int32).reshape(n, 2)), CAM, BOUNDS, th=th, ORBdist=orb, Tcw=self.Tcw,
            pair_Tcw=None if poses is None else _up(np.asarray(poses, f32).reshape(n, 4, 4)),
            cur_valid=None if cur_valid is None else _up(_rows(cur_valid, cap, 0, np.uint8)), already_found=None if found is None else _up(_rows(found, cap, 0, np.uint8)),
            d_th=None if d_th is None else _up(np.asarray(d_th, f32)), d_orb_dist=None if d_orb is None else _up(np.asarray(d_orb, np.int32)), checkOri=bool(ori),
            mp_valid=self.valid, mp_bad=self.bad, mp_desc=self.mdesc, img_stride=self.st, out=(m, nm), context=self.ctx)
        torch.cuda.synchronize()
        return m.cpu().numpy(), nm.cpu().numpy()

    def scene(self, s, th, ori, **kw):
        """the pairs of a scene with their per-pair poses, masks and ORBdist array"""
        return self.search(s.pairs, s.poses, s.cur_valid, s.found, th, 77, ori, d_orb=s.orbs, **kw)


class LoopBatch(Frames):
    """key frames and the map they are searched for"""

    def __init__(self, ctx, kfs, mp, img_stride=1, counts=None):
        super().__init__(ctx, kfs, img_stride, counts)
        self.mp = mp
        self.map = dict(world=_up(mp.world), normal=_up(mp.normal), maxd=_up(mp.maxd), mind=_up(mp.mind), desc=_up(mp.desc), bad=_up(mp.bad.astype(np.uint8)))

    def search(self, Scw, lists, fms, th, d_th=None, n_frames=None, n_mp=None):
        """(frame_matched after the call, nmatches) as numpy arrays.  lists None: every key frame sees the whole map in index order"""
        import torch
        cap, n = self.ctx.orb_capacity, len(Scw)
        offs = idx = None
        if lists is not None:
            offs = _up(np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32))
            idx = _up(np.concatenate([np.asarray(l, np.int32) for l in lists]))
        lm = matcher.LocalMapDev(self.map["world"], self.map["normal"], self.map["maxd"], self.map["mind"], self.map["desc"], None, self.map["bad"], offs, idx,
                                 n_mp=self.mp.n if n_mp is None else n_mp)
        fm = _up(_rows(fms, cap, FILL, np.int32))
        nm = torch.full((n,), FILL, dtype=torch.int32, device="cuda")
        matcher.search_by_projection_sim3_batch(self.n if n_frames is None else n_frames, self.kps, self.desc, self.counts, self.offs, self.idx, lm,
                                                _up(np.asarray(Scw, f32).reshape(n, 4, 4)), fm, CAM, BOUNDS, th=th, d_th=None if d_th is None else _up(np.asarray(d_th, f32)), img_stride=self.st, out=nm, context=self.ctx)
        torch.cuda.synchronize()
        return fm.cpu().numpy(), nm.cpu().numpy()


def assert_equal(res, exp, names=("rows", "nmatches")):
    for r, e, name in zip(res, exp, names):
        r = r[:len(e)]
        assert np.array_equal(r, e), (name, np.argwhere(r != e)[:10])


@pytest.fixture(scope="module")
def reloc(ctx):
    s = S.scenario_reloc_batch(ctx.orb_capacity)
    return s, RelocBatch(ctx, s.kfs)


@pytest.fixture(scope="module")
def loop(ctx):
    s = S.scenario_loop_batch(ctx.orb_capacity)
    return s, LoopBatch(ctx, s.kfs, s.mp)


# ---- the relocalisation form ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ori", [0, 1])
@pytest.mark.parametrize("th", S.RELOC_THS)
def test_reloc_batch_parity(ctx, reloc, th, ori):
    """1: seven frames of (0, 1, 63, 64, 65, 300, 900) key points, fourteen pairs each with its own pose, mvpMapPoints mask and sAlreadyFound, ORBdist
    100 / 64 per pair, one (frame, key frame) twice under two poses"""
    s, dev = reloc
    assert_equal(dev.scene(s, th, ori), s.exp[(th, ori)])
    ctx.poll_status()


@pytest.mark.parametrize("ori", [0, 1])
def test_reloc_hand_built(ctx, ori):
    """2: the order dependence both ways, the recompute path, a key point closed on entry, sAlreadyFound / a bad point / a feature without a point, the
    closed bounds, the distance interval to the ulp, the window's levels at level 0 and at the top, ORBdist and ORBdist + 1, the scan-order tie, a point
    behind the camera and a rejected rotation bin -- all cases as the pairs (2k, 2k + 1) of one call"""
    cases = S.scenario_reloc_gates(ctx.orb_capacity)
    kfs = [k for c in cases for k in (c.cur, c.kf)]
    pairs = [(2 * k, 2 * k + 1) for k in range(len(cases))]
    res = RelocBatch(ctx, kfs).search(pairs, None, [c.cur_valid for c in cases], [c.found for c in cases], 1.0, 1, ori, d_th=[c.th for c in cases],
                                      d_orb=[c.orb for c in cases])
    for k, c in enumerate(cases):
        want = c.want_ori if ori and c.want_ori else (c.want, c.want_n)
        assert (list(res[0][k, :c.cur.N]), res[1][k]) == want, c.name
        assert np.array_equal(res[0][k], c.exp[ori][0]) and res[1][k] == c.exp[ori][1], c.name
    ctx.poll_status()


def test_reloc_equals_the_host_form(ctx, reloc):
    """3: olf_search_by_projection_kf on the same views, with its own grid and with a supplied one, gives the rows of the entry"""
    s, dev = reloc
    res = dev.scene(s, 10.0, 1)
    m = ola.ORBmatcher(0.9, True, context=ctx)
    for p in (0, 1, 2, 3, 9, 12):
        a, b = s.pairs[p]
        for supplied in (False, True):
            cur = S.current_view(s.kfs[a], s.poses[p], s.cur_valid[p])
            cur.attach_grid(*(ola.assign_features_to_grid(cur.mvKeysUn, BOUNDS, context=ctx) if supplied and cur.N else (None, None)))
            n, row = m.SearchByProjection(cur, s.kfs[b], s.found[p], 10.0, s.orbs[p])
            assert n == res[1][p] and np.array_equal(row, res[0][p, :cur.N]), (p, supplied)
    ctx.poll_status()


def test_reloc_order_and_repetition(ctx, reloc):
    """4: the same call twice gives the same rows; the pair list permuted gives permuted rows"""
    s, dev = reloc
    first = dev.scene(s, 10.0, 1)
    assert_equal(first, s.exp[(10.0, 1)])
    assert_equal(dev.scene(s, 10.0, 1), first)
    perm = np.random.default_rng(4).permutation(len(s.pairs))
    pick = lambda a: [a[i] for i in perm]
    res = dev.search(pick(s.pairs), pick(s.poses), pick(s.cur_valid), pick(s.found), 10.0, 77, 1, d_orb=pick(s.orbs))
    assert_equal(res, tuple(e[perm] for e in s.exp[(10.0, 1)]))
    ctx.poll_status()


def test_reloc_malformed_and_skipped_pairs(ctx, reloc):
    """5: an index -1, an index n_frames and both indices equal give nmatches = -1, leave their rows as they were and set bit 2048; d_th <= 0 skips a
    pair, row and count untouched, no bit; the pairs beside them are not affected; n_pairs == 0 and n_frames == 0 write nothing"""
    s, dev = reloc
    bad = {2: (-1, 5), 5: (5, len(s.kfs)), 9: (6, 6)}
    skipped = (0, 7)
    pairs = [bad.get(p, ab) for p, ab in enumerate(s.pairs)]
    d_th = [0.0 if p == 0 else -1.0 if p == 7 else 10.0 for p in range(len(pairs))]
    res = dev.search(pairs, s.poses, s.cur_valid, s.found, 5.0, 77, 1, d_th=d_th, d_orb=s.orbs)
    good = [p for p in range(len(pairs)) if p not in bad and p not in skipped]
    assert_equal(tuple(r[good] for r in res), tuple(e[good] for e in s.exp[(10.0, 1)]))
    for p in bad:
        assert res[1][p] == -1 and (res[0][p] == FILL).all()
    for p in skipped:
        assert res[1][p] == FILL and (res[0][p] == FILL).all()
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert e.value.code == OLF_ERR_CAPACITY and "flags=2048" in str(e.value) and describes(e.value, 2048)
    ctx.poll_status()                                         # reported once, then clear
    res = dev.search([], [], [], [], 10.0, 100, 1)
    assert (res[0] == FILL).all() and (res[1] == FILL).all()
    res = dev.scene(s, 10.0, 1, n_frames=0)
    assert (res[0] == FILL).all() and (res[1] == FILL).all()
    ctx.poll_status()


def test_reloc_layout(ctx, reloc, oracle):
    """6: img_stride 1 and 2 give the same rows; a count above the capacity is read as the capacity and one below N cuts the frame; the frames' own
    descriptors stand in for a NULL mp_desc; without d_Tcw the current frame's own pose is used, without masks nothing is closed or found; a caller's stream"""
    import torch
    s, dev = reloc
    cap = ctx.orb_capacity
    assert_equal(RelocBatch(ctx, s.kfs, img_stride=2).scene(s, 10.0, 1), s.exp[(10.0, 1)])
    c = S.scenario_reloc_counts(cap)
    assert_equal(RelocBatch(ctx, c.kfs, img_stride=2, counts=c.counts).scene(c, 10.0, 1), c.exp)
    # mp_desc NULL: GetDescriptor() is the feature's own descriptor; no d_Tcw, no masks, the scalar ORBdist
    own = []
    for k in s.kfs:
        k = S.cut(k, k.N)
        k.mp_desc = k.mDescriptors.copy()
        own.append(k)
    sub = list(range(6))
    rows = [S.expect_reloc_pair(oracle, S.current_view(own[a], own[a].mTcw, np.zeros(own[a].N, bool)), own[b], np.zeros(own[b].N, bool), 10.0, 80, 1, cap)
            for a, b in (s.pairs[p] for p in sub)]
    exp_o = (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.int32))
    assert not np.array_equal(exp_o[0], s.exp[(10.0, 1)][0][sub])
    assert_equal(RelocBatch(ctx, own, own_desc=True).search([s.pairs[p] for p in sub], None, None, None, 10.0, 80, 1), exp_o)
    # a stream of the caller's
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        res = dev.scene(s, 10.0, 1)
    assert_equal(res, s.exp[(10.0, 1)])
    ctx.poll_status()


# ---- the loop form --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", S.LOOP_THS)
def test_loop_batch_parity(ctx, loop, th):
    """1: seven key frames of (0, 1, 63, 64, 65, 300, 900) key points under Sim3 poses of scale 0.5 .. 2, each with its own shuffled list of map points and
    a row of vpMatched that holds map points (closed, and in spAlreadyFound) and points outside the map (closed only)"""
    s, dev = loop
    assert_equal(dev.search(s.Scw, s.lists, s.fms, th), s.exp[th])
    ctx.poll_status()


def test_loop_hand_built(ctx):
    """2: the order dependence both ways, the recompute path, a key point closed on entry / spAlreadyFound / a bad point, the half-open bounds, the depth
    gate, the distance interval to the ulp, the level gate at level 0 (octave -1 passes) and at the top, TH_LOW and TH_LOW + 1, the scan-order tie -- the
    cases as the key frames of one call, their maps one after the other in one map"""
    cases = S.scenario_loop_gates(ctx.orb_capacity)
    base = np.concatenate([[0], np.cumsum([c.mp.n for c in cases])])
    mp = types.SimpleNamespace(n=int(base[-1]), **{k: np.concatenate([getattr(c.mp, k) for c in cases]) for k in ("world", "normal", "maxd", "mind", "desc", "bad")})
    shift = lambda a, o: np.where(np.asarray(a) >= 0, np.asarray(a) + o, np.asarray(a)).astype(np.int32)
    res = LoopBatch(ctx, [c.kf for c in cases], mp).search([c.Scw for c in cases], [base[k] + np.arange(c.mp.n) for k, c in enumerate(cases)],
                                                           [shift(c.fm, base[k]) for k, c in enumerate(cases)], 10.0)
    for k, c in enumerate(cases):
        assert list(res[0][k, :c.kf.N]) == list(shift(c.want, base[k])) and res[1][k] == c.want_n, c.name
        assert np.array_equal(res[0][k], shift(c.exp[0], base[k])) and res[1][k] == c.exp[1], c.name
    ctx.poll_status()


def test_loop_equals_the_host_form(ctx, loop):
    """3: olf_search_by_projection_sim3 on the same views, with its own grid and with a supplied one, gives the rows of the entry"""
    s, dev = loop
    rows, nm = dev.search(s.Scw, s.lists, s.fms, 10.0)
    m = ola.ORBmatcher(0.75, True, context=ctx)
    for j in (2, 4, 5, 6):
        kf, order, fm = s.kfs[j], s.lists[j].astype(np.int64), s.fms[j][:s.kfs[j].N]
        held = np.zeros(s.mp.n, bool)
        held[fm[fm >= 0]] = True
        for supplied in (False, True):
            kf.attach_grid(*(ola.assign_features_to_grid(kf.mvKeysUn, BOUNDS, context=ctx) if supplied else (None, None)))
            n, km = m.SearchByProjectionSim3(kf, s.Scw[j], S.loop_geom(s.mp, order, s.mp.bad[order] | held[order]), np.ascontiguousarray(fm != -1), 10)
            after = fm.copy()
            after[km >= 0] = order[km[km >= 0]]
            assert n == nm[j] and np.array_equal(after, rows[j, :kf.N]), (j, supplied)
        kf.attach_grid(None, None)
    ctx.poll_status()


def test_loop_order_and_repetition(ctx, loop, oracle):
    """4: the same call twice gives the same rows; the key frames in another order give their rows in that order; the lists of the other key frames
    permuted leave a key frame's row alone (and change their own: the order of a list matters)"""
    s, dev = loop
    cap = ctx.orb_capacity
    first = dev.search(s.Scw, s.lists, s.fms, 10.0)
    assert_equal(first, s.exp[10])
    assert_equal(dev.search(s.Scw, s.lists, s.fms, 10.0), first)
    perm = np.random.default_rng(4).permutation(len(s.kfs))
    pick = lambda a: [a[i] for i in perm]
    assert_equal(LoopBatch(ctx, pick(s.kfs), s.mp).search(pick(s.Scw), pick(s.lists), pick(s.fms), 10.0), tuple(e[perm] for e in s.exp[10]))
    rng = np.random.default_rng(8)
    lists = [l if j == 5 else rng.permutation(l) for j, l in enumerate(s.lists)]
    exp = S.expect_loop(oracle, s, 10, cap, lists=lists)
    assert np.array_equal(exp[0][5], s.exp[10][0][5]) and not np.array_equal(exp[0][6], s.exp[10][0][6])
    assert_equal(dev.search(s.Scw, lists, s.fms, 10.0), exp)
    ctx.poll_status()


def test_loop_malformed_indices_and_skipped_frames(ctx, loop, oracle):
    """5: a list index outside the map is left out and a held value >= n_mp only closes its key point, both set bit 512; d_th <= 0 skips a key frame, row
    and count untouched; the key frames beside them are not affected; n_frames == 0 writes nothing"""
    s, dev = loop
    cap = ctx.orb_capacity
    lists = [l.copy() for l in s.lists]
    took5 = s.exp[10][0][5][:300][s.exp[10][0][5][:300] != s.fms[5][:300]]      # the points key frame 5 received: two of them leave its list
    lists[5][np.flatnonzero(np.isin(lists[5], took5))[[0, 7]]] = (-1, s.mp.n + 5)
    fms = [f.copy() for f in s.fms]
    open6 = np.flatnonzero(s.exp[10][0][6][:900] != fms[6][:900])[:3]      # three key points that took a point: now they hold one outside the map
    fms[6][open6] = s.mp.n + 7
    t = types.SimpleNamespace(kfs=s.kfs, Scw=s.Scw, lists=lists, fms=fms, mp=s.mp)
    d_th = [10.0, 10.0, 0.0, 10.0, -2.0, 10.0, 10.0]
    exp = S.expect_loop(oracle, t, 10, cap)
    assert not np.array_equal(exp[0][5], s.exp[10][0][5]) and not np.array_equal(exp[0][6], s.exp[10][0][6])
    res = dev.search(s.Scw, lists, fms, 4.0, d_th=d_th)
    for j in range(7):
        if d_th[j] > 0:
            assert np.array_equal(res[0][j], exp[0][j]) and res[1][j] == exp[1][j], j
        else:
            assert np.array_equal(res[0][j], fms[j]) and res[1][j] == FILL, j
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert "flags=512" in str(e.value) and describes(e.value, 512)
    ctx.poll_status()
    res = dev.search(s.Scw, s.lists, s.fms, 10.0, n_frames=0)
    assert np.array_equal(res[0][:7], np.stack(s.fms)) and (res[1] == FILL).all()
    ctx.poll_status()


def test_loop_layout(ctx, loop, oracle):
    """6: img_stride 2; a count above the capacity is read as the capacity and one below N cuts the key frame; without lists every key frame sees the
    whole map in index order; a caller's stream"""
    import torch
    s, dev = loop
    cap = ctx.orb_capacity
    assert_equal(LoopBatch(ctx, s.kfs, s.mp, img_stride=2).search(s.Scw, s.lists, s.fms, 10.0), s.exp[10])
    # counts: the last key frame fills the capacity, so that the rows a count beyond it reaches are defined; key frame 4 is cut to 40
    c = S.scenario_loop_counts(cap)
    assert_equal(LoopBatch(ctx, c.full, c.mp, img_stride=2, counts=c.counts).search(c.Scw, c.lists, c.fms, 10.0), c.exp)
    # no lists: a map of the first 500 points, all of them for every key frame (what a key frame holds beyond them is a point outside the map: -2)
    sub = [2, 5, 6]
    t = types.SimpleNamespace(kfs=[s.kfs[j] for j in sub], Scw=[s.Scw[j] for j in sub], lists=[np.arange(500)] * 3,
                              fms=[np.where(s.fms[j] >= 500, -2, s.fms[j]).astype(np.int32) for j in sub], mp=s.mp)
    exp = S.expect_loop(oracle, t, 10, cap, n_mp=500)
    assert (exp[1] >= 10).all()
    assert_equal(LoopBatch(ctx, t.kfs, s.mp).search(t.Scw, None, t.fms, 10.0, n_mp=500), exp)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        res = dev.search(s.Scw, s.lists, s.fms, 10.0)
    assert_equal(res, s.exp[10])
    ctx.poll_status()


# ---- both -----------------------------------------------------------------------------------------------------------------------------------------------
def test_capacity(ctx, reloc, loop):
    """7: a context above OLF_GRID_MAX_KEYS is refused before anything is read"""
    s, dev = reloc
    t, ldev = loop
    p = _lib.default_params()
    p.orb.nfeatures = _lib.GRID_MAX_KEYS + 1
    big = _lib.Context(p, S.W, S.H, 1)
    try:
        assert big.orb_capacity > _lib.GRID_MAX_KEYS
        with pytest.raises(ola.OlfError) as e:
            matcher.search_by_projection_kf_pairs(dev.n, dev.kps, dev.desc, dev.counts, dev.offs, dev.idx, dev.world, dev.maxd, dev.mind,
                                                  _up(np.asarray(s.pairs[:1], np.int32)), CAM, BOUNDS, Tcw=dev.Tcw, img_stride=1,
                                                  out=(_up(np.full((1, 8), -1, np.int32)), _up(np.zeros(1, np.int32))), context=big)
        assert e.value.code == OLF_ERR_CAPACITY
        lm = matcher.LocalMapDev(*(ldev.map[k] for k in ("world", "normal", "maxd", "mind", "desc")), None, ldev.map["bad"])
        with pytest.raises(ola.OlfError) as e:
            matcher.search_by_projection_sim3_batch(1, ldev.kps, ldev.desc, ldev.counts, ldev.offs, ldev.idx, lm, _up(np.eye(4, dtype=f32)[None]),
                                                    _up(np.full((1, 8), -1, np.int32)), CAM, BOUNDS, img_stride=1, out=_up(np.zeros(1, np.int32)), context=big)
        assert e.value.code == OLF_ERR_CAPACITY
    finally:
        big.close()
    ctx.poll_status()
