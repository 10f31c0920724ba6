"""olf_compute_f12_pairs_dev, olf_create_new_map_points_batch_dev and olf_update_normal_and_depth_dev on the device against their host forms (bit for bit:
the same header, no contraction) and against the restatements by the rules of tests/test_newpoints_cpu.py: match rows of 0, 1, 63, 64, 65 and 300, pair
lists of 0, 1, 7 and 65 with a marked pair first, in the middle and last, img_stride 1 and 2, observation rows of 0, 1, 2, 63, 64, 65 and 300, a bad point,
a point list and NULL, outputs with 37 sentinel elements behind them, malformed input, and the chain F12 -> search -> create -> normal / depth -> frustum
on device buffers only."""
import copy
import numpy as np
import pytest
import newpoints_reference as R
import newpoints_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, newpoints
from orb_line_slam_amd._lib import OLF_ERR_CAPACITY
from status_text import describes
from test_newpoints_cpu import assert_und, cleaned_snapshot, host_create, host_und, malformed_snapshot

pytestmark = pytest.mark.gpu
F = np.float32
PAD = 37
KF_TEXT = "4096: a map-graph entry left out a key-frame index outside the graph"


@pytest.fixture(scope="module")
def ctx():
    p = _lib.default_params()
    p.orb.nfeatures = 500
    c = _lib.Context(p, S.W, S.H, 2)
    assert S.POOL <= c.orb_capacity <= 4096 and c.nlevels == 8
    sf = np.zeros(8, F)
    _lib.lib().olf_orb_scale_tables(c.handle, sf.ctypes.data, None, None, None, None)
    assert np.array_equal(sf, S.SF)
    yield c
    c.close()


def up(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


class DeviceBatch:
    def __init__(self, ctx, frames, img_stride=1):
        self.ctx, self.cap, self.st, self.n = ctx, ctx.orb_capacity, img_stride, len(frames)
        kps, cnt, ur, depth, Tcw = S.batch_arrays(frames, self.cap, img_stride)
        self.kps, self.counts = up(kps.view(np.uint8).reshape(self.n * img_stride, self.cap, 28)), up(cnt)
        self.uright, self.depth, self.Tcw = up(ur), up(depth), up(Tcw)

    def create(self, pairs, rows, monocular=False, mb=S.MB, n_pairs=None, fill=-1):
        """(x3D, code, nnew) as numpy arrays of the listed pairs; the outputs are PAD elements longer than the call needs and start as sentinels"""
        import torch
        P, cap = len(pairs), self.cap
        d_pairs, d_m12 = up(np.asarray(pairs, np.int32).reshape(P, 2)), up(S.match_rows(rows, cap, fill))
        if n_pairs is not None:
            d_pairs, d_m12 = d_pairs[:n_pairs], d_m12[:n_pairs]
        x3D = torch.full((P * cap * 3 + PAD,), -7.0, dtype=torch.float32, device="cuda")
        code = torch.full((P * cap + PAD,), 99, dtype=torch.uint8, device="cuda")
        nnew = torch.full((P + PAD,), -7, dtype=torch.int32, device="cuda")
        newpoints.create_new_map_points_batch(self.n, self.kps, self.counts, self.uright, self.depth, self.Tcw, S.CAM5, mb, d_pairs, d_m12, monocular, self.st,
                                              out=(x3D, code, nnew), context=self.ctx)
        torch.cuda.synchronize()
        x3D, code, nnew = x3D.cpu().numpy(), code.cpu().numpy(), nnew.cpu().numpy()
        assert (x3D[P * cap * 3:] == -7).all() and (code[P * cap:] == 99).all() and (nnew[P:] == -7).all()      # nothing past the batch
        return x3D[:P * cap * 3].reshape(P, cap, 3), code[:P * cap].reshape(P, cap), nnew[:P]


def same_as_host(dev, host):
    for a, b, what in zip(dev, host, ("x3D", "code", "nnew")):
        a, b = (S.bits(v) if v.dtype == np.float32 else v for v in (a, b))
        assert np.array_equal(a, b), (what, np.argwhere(a != b)[:6])


# ---- CreateNewMapPoints -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("img_stride", [1, 2])
def test_create_rows_of_every_length(ctx, img_stride):
    sc = S.scene_set()
    ctx.poll_status()
    got = DeviceBatch(ctx, sc.frames, img_stride).create(sc.pairs, sc.rows)
    ctx.poll_status()
    host = host_create(sc.frames, sc.pairs, sc.rows, img_stride=img_stride, cap=ctx.orb_capacity)
    assert host[3] == 0
    same_as_host(got, host[:3])
    worst = S.check_rows(*got, sc.refs)
    print("largest ratio of the tolerance rule, device against base:", worst)


@pytest.mark.parametrize("n_pairs", [0, 1, 7, 65])
def test_create_pair_lists_and_positions(ctx, n_pairs):
    """a marked pair (300 matches) first, in the middle and last among pairs of 63 matches: the same bits wherever it stands"""
    sc = S.scene_set()
    dev = DeviceBatch(ctx, sc.frames)
    if n_pairs == 0:
        x3D, code, nnew = dev.create([sc.pairs[5]], [sc.rows[5]], n_pairs=0)
        assert (x3D == -7).all() and (code == 99).all() and (nnew == -7).all()
        return
    marked = dev.create([sc.pairs[5]], [sc.rows[5]])
    filler = dev.create([sc.pairs[2]], [sc.rows[2]])
    for pos in sorted({0, n_pairs // 2, n_pairs - 1}):
        pairs = [sc.pairs[2]] * n_pairs
        rows = [sc.rows[2]] * n_pairs
        pairs[pos], rows[pos] = sc.pairs[5], sc.rows[5]
        got = dev.create(pairs, rows)
        for q in range(n_pairs):
            same_as_host([a[q] for a in got], [a[0] for a in (marked if q == pos else filler)])
    ctx.poll_status()


def test_create_malformed(ctx):
    sc = S.scene_set()
    dev = DeviceBatch(ctx, sc.frames)
    good = dev.create(sc.pairs, sc.rows)
    ctx.poll_status()
    pairs = [(0, 0), sc.pairs[3], (-1, 2), sc.pairs[5], (2, 6)]
    rows = [sc.rows[0], sc.rows[3], sc.rows[0], sc.rows[5], sc.rows[0]]
    x3D, code, nnew = dev.create(pairs, rows)
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert e.value.code == OLF_ERR_CAPACITY and "flags=2048" in str(e.value) and describes(e.value, 2048)
    for q in (0, 2, 4):
        assert nnew[q] == -1 and (code[q] == 99).all() and (x3D[q] == -7).all()      # rows untouched
    for q, p in ((1, 3), (3, 5)):
        same_as_host([a[q] for a in (x3D, code, nnew)], [a[p] for a in good])
    # an idx2 outside [0, N2), an octave outside the levels: the affected row equals the run without the element
    i_a, i_b = sorted(sc.refs[5])[:2]
    row = sc.rows[5].copy()
    row[i_a] = S.POOL + 3
    frames = list(sc.frames)
    frames[5] = copy.deepcopy(sc.frames[5])
    frames[5].keys["octave"][i_b] = 8
    got = DeviceBatch(ctx, frames).create([sc.pairs[5]], [row])
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert "flags=256" in str(e.value) and describes(e.value, 256)
    clean = sc.rows[5].copy()
    clean[[i_a, i_b]] = -1
    same_as_host(got, dev.create([sc.pairs[5]], [clean]))
    ctx.poll_status()
    # the baseline skip
    x3D, code, nnew = dev.create([sc.pairs[5]], [sc.rows[5]], mb=50.0)
    assert nnew[0] == 0 and not code.any() and not x3D.any()
    assert dev.create([sc.pairs[5]], [sc.rows[5]], mb=50.0, monocular=True)[2][0] > 0
    # rows full of values no feature has
    x3D, code, nnew = dev.create([sc.pairs[5]], [np.full(S.POOL, 1 << 30, np.int32)], fill=-(1 << 31))
    assert nnew[0] == 0 and not code.any()
    ctx.poll_status()


def test_create_row_across_steps_and_segments():
    """A first frame of more than 2049 key points in a context whose capacity exceeds a segment of the kernel's compaction (2048 idx1 slots), usable
    matches at both sides of the first step boundary (255, 256, 257), of the segment boundary (2046 to 2049), at slot 0 and at the frame's last key
    point, -1 everywhere else: the second turn of the segment loop runs.  The frame tiles the pool's key points -- a match's result depends on its own
    inputs only --, slot s of the nine holding the feature of one usable match of pair 5.  Equal to the host form bit for bit."""
    p = _lib.default_params()
    p.orb.nfeatures = 2100
    big = _lib.Context(p, S.W, S.H, 2)
    try:
        cap = big.orb_capacity
        assert 2049 + 5 < cap <= 4096
        sc = S.scene_set()
        (a, b), n1 = sc.pairs[5], cap - 5
        slots = [0, 255, 256, 257, 2046, 2047, 2048, 2049, n1 - 1]
        src = np.arange(n1) % S.POOL
        row = np.full(n1, -1, np.int32)
        for s, i1 in zip(slots, sorted(sc.refs[5])[::30]):
            src[s], row[s] = i1, sc.rows[5][i1]
        fr = copy.copy(sc.frames[a])
        fr.keys, fr.uright, fr.depth = sc.frames[a].keys[src], sc.frames[a].uright[src], sc.frames[a].depth[src]
        frames = list(sc.frames)
        frames[a] = fr
        big.poll_status()
        got = DeviceBatch(big, frames).create([(a, b)], [row])
        big.poll_status()
        host = host_create(frames, [(a, b)], [row], cap=cap)
        assert host[3] == 0
        same_as_host(got, host[:3])
        used = np.zeros(cap, bool)
        used[slots] = True
        assert (got[1][0][used] != 0).all() and not got[1][0][~used].any() and not got[0][0][~used].any()
        for s, i1 in zip(slots, sorted(sc.refs[5])[::30]):               # and the slot's result is that of the match where the pool has it
            assert got[1][0][s] == sc.refs[5][i1][0]
    finally:
        big.close()


# ---- ComputeF12 -----------------------------------------------------------------------------------------------------------------------------------------
def test_f12_pairs(ctx):
    import torch
    sc = S.scene_set()
    cam = (S.FX, S.FY, S.CX, S.CY)
    Tcw = up(np.stack([fr.Tcw for fr in sc.frames]))
    all_pairs = [(a, b) for a in range(6) for b in range(6) if a != b]
    host = {p: newpoints.ComputeF12(sc.frames[p[0]].Tcw, sc.frames[p[1]].Tcw, cam).reshape(-1) for p in all_pairs}
    for n in (0, 1, 7, 65):
        for pos in sorted({0, n // 2, max(n - 1, 0)}):
            pairs = [all_pairs[(3 * k) % 30] for k in range(n)]
            if n:
                pairs[pos] = (4, 1)
            out = torch.full((n * 9 + PAD,), -7.0, dtype=torch.float32, device="cuda")
            newpoints.compute_f12_pairs(Tcw, cam, up(np.asarray(pairs, np.int32).reshape(n, 2)), out=out, context=ctx)
            torch.cuda.synchronize()
            out = out.cpu().numpy()
            assert (out[n * 9:] == -7).all()
            for q, p in enumerate(pairs):
                assert np.array_equal(S.bits(out[9 * q:9 * q + 9]), S.bits(host[p])), (n, q, p)
    assert np.array_equal(S.bits(host[(4, 1)]), S.bits(R.compute_f12(sc.frames[4].Tcw, sc.frames[1].Tcw, cam).reshape(-1)))
    ctx.poll_status()
    pairs = [(0, 1), (2, 2), (1, 0), (6, 0), (3, -1), (5, 4)]
    out = torch.full((6 * 9,), -7.0, dtype=torch.float32, device="cuda")
    newpoints.compute_f12_pairs(Tcw, cam, up(np.asarray(pairs, np.int32)), out=out, context=ctx)
    torch.cuda.synchronize()
    out = out.cpu().numpy().reshape(6, 9)
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert "flags=2048" in str(e.value) and describes(e.value, 2048)
    for q, p in enumerate(pairs):
        assert (out[q] == -7).all() if p not in host else np.array_equal(S.bits(out[q]), S.bits(host[p]))


# ---- UpdateNormalAndDepth -----------------------------------------------------------------------------------------------------------------------------
def dev_und(ctx, s, graph, points=None, n_points=None):
    import torch
    g, v = graph
    normal = torch.full((s.n_mp * 3 + PAD,), -7.0, dtype=torch.float32, device="cuda")
    maxd = torch.full((s.n_mp + PAD,), -7.0, dtype=torch.float32, device="cuda")
    mind = torch.full((s.n_mp + PAD,), -7.0, dtype=torch.float32, device="cuda")
    newpoints.update_normal_and_depth(g, v, up(s.mp_world), up(s.ref_kf), up(s.kf_Ow), normal, maxd, mind, points=None if points is None else up(points, np.int32),
                                      n_points=n_points, context=ctx)
    torch.cuda.synchronize()
    normal, maxd, mind = normal.cpu().numpy(), maxd.cpu().numpy(), mind.cpu().numpy()
    assert (normal[s.n_mp * 3:] == -7).all() and (maxd[s.n_mp:] == -7).all() and (mind[s.n_mp:] == -7).all()
    return normal[:s.n_mp * 3].reshape(s.n_mp, 3), maxd[:s.n_mp], mind[:s.n_mp]


def test_normal_depth_rows_of_every_length(ctx):
    s = S.snapshot(3)
    graph = S.snapshot_graph(s)
    ctx.poll_status()
    got = dev_und(ctx, s, graph)
    ctx.poll_status()
    assert_und(got, host_und(s, graph=graph))
    assert_und(got, S.snapshot_expected(s))
    assert (got[1][[0, 3]] == -7).all()                              # the empty row and the bad point
    lst = [5, 1, 40, 5, 3, 0]
    got = dev_und(ctx, s, graph, points=lst)
    assert_und(got, S.snapshot_expected(s, points=lst))
    assert (dev_und(ctx, s, graph, points=lst, n_points=0)[1] == -7).all()
    # a list longer than a workgroup, every point several times
    lst = list(np.random.default_rng(1).integers(0, s.n_mp, 700))
    assert_und(dev_und(ctx, s, graph, points=lst), S.snapshot_expected(s, points=sorted(set(int(p) for p in lst))))
    ctx.poll_status()


def test_normal_depth_malformed(ctx):
    s = S.snapshot(4)
    for p, k in ((10, 1), (11, 0)):
        if s.mp_obs[p][k] == s.ref_kf[p]:
            s.ref_kf[p] = s.mp_obs[p][2]
    exp = list(S.snapshot_expected(cleaned_snapshot(s)))
    graph = S.snapshot_graph(s)
    malformed_snapshot(s, *graph)
    for a in exp:
        a[[12, 14]] = -7
    ctx.poll_status()
    got = dev_und(ctx, s, graph)
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert "flags=%d" % (256 | 4096) in str(e.value) and describes(e.value, 256) and KF_TEXT in str(e.value)
    assert_und(got, exp)
    got = dev_und(ctx, s, graph, points=[s.n_mp, 2, -1])
    with pytest.raises(ola.OlfError) as e:
        ctx.poll_status()
    assert "flags=512" in str(e.value) and describes(e.value, 512) and (got[1] != -7).sum() == 1


# ---- the chain --------------------------------------------------------------------------------------------------------------------------------------
def test_chain_on_device_buffers(ctx):
    """F12 -> SearchForTriangulation -> CreateNewMapPoints -> UpdateNormalAndDepth without a host copy of per-match data; the created points, as a local map,
    pass Frame::isInFrustum of key frame 1"""
    import torch
    import test_triangulation_batch_gpu as T
    from orb_line_slam_amd import CullView, MapGraph, matcher
    frames, base = T.make_frames((300, 300), 21)
    for fr in frames:                                                # no feature holds a point yet; mvDepth = mbf / disparity for the stereo ones
        fr.valid[:] = False
        fr.depth = np.where(fr.uright >= 0, F(40.0) / np.maximum(fr.keys["x"] - fr.uright, F(1e-3)), F(-1)).astype(F)
    voc, _ = T.make_voc(10, 3, base)
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    tdev = T.DeviceFrames(ctx, frames)
    cap = ctx.orb_capacity
    depth = np.full((2, cap), -1.0, F)
    for j, fr in enumerate(frames):
        depth[j, :len(fr.keys)] = fr.depth
    d_depth, d_pairs = up(depth), up(np.array([[0, 1]], np.int32))
    cam5 = T.CAM + (40.0,)
    F12 = newpoints.compute_f12_pairs(tdev.Tcw, T.CAM, d_pairs, context=ctx)
    m12, nm = matcher.search_for_triangulation_batch(G, 2, tdev.kps, tdev.desc, tdev.counts, tdev.uright, tdev.Tcw, d_pairs, F12, T.CAM, mp_valid=tdev.valid,
                                                     levelsup=2, img_stride=1, context=ctx)
    # (the frame builder's views are 0.05 m apart, less than mb: monocular = 1 leaves the baseline test out)
    x3D, code, nnew = newpoints.create_new_map_points_batch(2, tdev.kps, tdev.counts, tdev.uright, d_depth, tdev.Tcw, cam5, 0.2, d_pairs, m12, monocular=True,
                                                            img_stride=1, context=ctx)
    # the map: one point per idx1 slot of the pair, observed by key frame 0 at slot idx1 and by key frame 1 at slot idx2; the slots that created nothing are bad
    n_mp = cap
    made = (code[0] >= 1) & (code[0] <= 3)
    octave = np.zeros((2, cap), np.uint8)
    for j, fr in enumerate(frames):
        octave[j, :len(fr.keys)] = fr.keys["octave"]
    obs_off = torch.arange(0, 2 * n_mp + 1, 2, dtype=torch.int32, device="cuda")
    obs_kf = torch.tensor([0, 1], dtype=torch.int32, device="cuda").repeat(n_mp)
    obs_slot = torch.stack([torch.arange(n_mp, dtype=torch.int32, device="cuda"), torch.clamp(m12[0], min=0)], 1).reshape(-1).contiguous()
    g, v = _lib.MapGraphC(), _lib.CullViewC()
    g.n_kf, g.n_mp = 2, n_mp
    keep = [obs_off, obs_kf, obs_slot, (~made).to(torch.uint8), up(np.array([0, cap, 2 * cap], np.int32)), up(octave.reshape(-1))]
    g.mp_obs_offsets, g.mp_obs_kf, v.mp_obs_slot, g.mp_bad, g.kf_mp_offsets, v.kf_slot_octave = (t.data_ptr() for t in keep)
    Ow = up(np.stack([np.array(R.kf_pose(fr.Tcw)[2], F) for fr in frames]))
    normal, maxd, mind = (torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((n_mp, 3), (n_mp,), (n_mp,)))
    newpoints.update_normal_and_depth(g, v, x3D[0].contiguous(), torch.zeros(n_mp, dtype=torch.int32, device="cuda"), Ow, normal, maxd, mind, context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()
    n = int(nnew[0])
    print("chain: matches", int(nm[0]), "created", n)
    assert n >= 1 and int(made.sum()) == n
    # Frame::isInFrustum of key frame 1 (frame 0) for the created points
    idx = torch.nonzero(made).reshape(-1).cpu().numpy()
    w, nv, mx, mn = (t.cpu().numpy()[idx] for t in (x3D[0], normal, maxd, mind))
    assert np.isfinite(w).all() and np.isfinite(nv).all() and (mx > 0).all() and (mn > 0).all()
    fv = matcher.FrameView(frames[0].keys, frames[0].desc, frames[0].uright, T.SF, fx=T.FX, fy=T.FY, cx=T.CX, cy=T.CY, mbf=40.0,
                           bounds=(0.0, float(T.W), 0.0, float(T.H)), mTcw=frames[0].Tcw)
    seen = matcher.isInFrustum(fv, matcher.MapPointGeom(w, nv, mx, mn, np.zeros((len(idx), 32), np.uint8)), 0.5)
    assert seen.mbTrackInView.all()
    G.clear()


# ---- the adaptor and the host-pointer forms on the device -------------------------------------------------------------------------------------------------
def test_adaptor_on_the_device(tmp_path):
    """the same program with `device`: every call through the thread's context, and compared bit for bit with the host forms"""
    import subprocess
    from test_newpoints_cpu import build_adaptor
    exe = str(tmp_path / "adaptor_newpoints")
    build_adaptor(exe)
    out = subprocess.run([exe, "device"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_NEWPOINTS_OK" in out.stdout, out.stdout.decode()[-3000:]


def test_host_pointer_forms_on_the_device(ctx):
    """olf_compute_f12_pairs, olf_create_new_map_points_pairs and olf_update_normal_and_depth_points: staged, run, brought back; equal to the host forms,
    untouched rows come back as they went in, a status bit comes back as OLF_ERR_CAPACITY with the outputs complete"""
    import ctypes as C
    L, cap, sc = _lib.lib(), ctx.orb_capacity, S.scene_set()
    kps, cnt, ur, depth, Tcw = S.batch_arrays(sc.frames, cap)
    pairs = np.array([sc.pairs[5], (2, 2), sc.pairs[4]], np.int32)
    F12 = np.full((3, 9), -7.0, F)
    rc = L.olf_compute_f12_pairs(ctx.handle, _lib.ptr(Tcw), 6, S.FX, S.FY, S.CX, S.CY, 3, _lib.ptr(pairs), _lib.ptr(F12))
    assert rc == OLF_ERR_CAPACITY and "flags=2048" in _lib.last_error() and (F12[1] == -7).all()
    for q in (0, 2):
        a, b = pairs[q]
        assert np.array_equal(S.bits(F12[q]), S.bits(newpoints.ComputeF12(sc.frames[a].Tcw, sc.frames[b].Tcw, (S.FX, S.FY, S.CX, S.CY)).reshape(-1)))
    tb = _lib.TrackBatchC()
    tb.kps, tb.counts, tb.img_stride, tb.uright, tb.Tcw = _lib.ptr(kps), _lib.ptr(cnt), 1, _lib.ptr(ur), _lib.ptr(Tcw)
    tb.fx, tb.fy, tb.cx, tb.cy, tb.mbf = S.CAM5
    m12 = S.match_rows([sc.rows[5], sc.rows[0], sc.rows[4]], cap)
    x3D, code, nnew = np.full((3, cap, 3), -7.0, F), np.full((3, cap), 99, np.uint8), np.full(3, -7, np.int32)
    rc = L.olf_create_new_map_points_pairs(ctx.handle, C.byref(tb), 6, _lib.ptr(depth), S.MB, 3, _lib.ptr(pairs), _lib.ptr(m12), 0, _lib.ptr(x3D), _lib.ptr(code), _lib.ptr(nnew))
    assert rc == OLF_ERR_CAPACITY and "flags=2048" in _lib.last_error()
    assert nnew[1] == -1 and (code[1] == 99).all() and (x3D[1] == -7).all()
    host = host_create(sc.frames, [sc.pairs[5], sc.pairs[4]], [sc.rows[5], sc.rows[4]], cap=cap)
    same_as_host([a[[0, 2]] for a in (x3D, code, nnew)], host[:3])
    s = S.snapshot(3)
    g, v = S.snapshot_graph(s)
    gc, vc = g.c(), v.c()
    normal, maxd, mind = np.full((s.n_mp, 3), -7.0, F), np.full(s.n_mp, -7.0, F), np.full(s.n_mp, -7.0, F)
    w, r, ow = (np.ascontiguousarray(a) for a in (s.mp_world, s.ref_kf, s.kf_Ow))
    rc = L.olf_update_normal_and_depth_points(ctx.handle, C.byref(gc), C.byref(vc), s.n_mp, None, _lib.ptr(w), _lib.ptr(r), _lib.ptr(ow), _lib.ptr(normal), _lib.ptr(maxd),
                                              _lib.ptr(mind))
    assert rc == 0, _lib.last_error()
    assert_und((normal, maxd, mind), host_und(s, graph=(g, v)))
    assert L.olf_update_normal_and_depth_points(ctx.handle, C.byref(gc), None, s.n_mp, None, _lib.ptr(w), _lib.ptr(r), _lib.ptr(ow), _lib.ptr(normal), _lib.ptr(maxd),
                                                _lib.ptr(mind)) == -1
    ctx.poll_status()
