"""olf_pose_optimization_batch_dev on the device, against the host form and the restatement (posepoints_reference) under the tolerance rule
(posepoints_scenes.within_rule: 16 x the restatement's spread, floor 64 float ulp); flags, n_good, n_initial, passes and status exactly; iters not compared.
All scenes run as one batch.  Every output is allocated SLACK elements longer than the batch needs and filled with a sentinel: nothing may be written past
a count, a row or the batch.  Position independence, the pairs form and the scratch path are compared with that batch bit for bit.
The last test chains the entry between the PnP solver's two entries, the discard loop and the key-frame projection search on device pointers."""
import ctypes as C
import numpy as np
import pytest
import posepoints_scenes as S
from orb_line_slam_amd import _lib, posepoints
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, OLF_ERR_INVALID, OlfError, lib

pytestmark = pytest.mark.gpu

SLACK = 37
SENT = {np.float32: 777.0, np.uint8: 0xAB, np.int32: -777}
NAMES = S.NAMES
assert NAMES[-1] == "past_map"
WIDTH = dict(Tcw_out=16, n_good=1, n_initial=1, passes=1, iters=4, status=1)
TYPES = dict([(n, t) for n, t, _ in posepoints.OUTPUTS] + list(posepoints.ROWS))


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    p = _lib.default_params()
    p.orb.nfeatures = S.NFEATURES
    c = _lib.Context(p, S.W, S.H, 2)
    assert c.orb_capacity == S.CAP and c.nlevels == S.N_LEVELS
    sig = np.zeros(c.nlevels, np.float32)
    _lib.check(lib().olf_orb_scale_tables(c.handle, None, None, None, _lib.ptr(sig), None), "olf_orb_scale_tables")
    assert np.array_equal(sig, S.scene_of(NAMES[0])["inv_level_sigma2"])
    yield c
    lib().olf_debug_pose_points_lds_limit(0)


def settle(ctx, bits=0):
    """wait, then read the context's status word: exactly `bits` must be set"""
    import torch
    torch.cuda.synchronize()
    if bits:
        with pytest.raises(OlfError) as e:
            ctx.poll_status()
        assert "flags=%d " % bits in str(e.value), str(e.value)
    ctx.poll_status()


def run_rows(ctx, names, img_stride=1, pairs=False, active=None, refuse=()):
    """the scenes `names` as rows.  Frame form: row r reads frame r, its map is a slice of one concatenated map (mp_index_offset).  Pairs form: frame 2 r is
    the key frame whose plane of mp_world [n_frames, capacity, 3] holds row r's points, frame 2 r + 1 carries the features, pairs[r] = (2 r, 2 r + 1);
    rows in `refuse` get the pair (k, k).  Returns the outputs as numpy arrays with their SLACK tails."""
    import torch
    cap, n = ctx.orb_capacity, len(names)
    scenes = [S.scene_of(x) for x in names]
    n_frames = 2 * n if pairs else n
    m = max(n_frames, 1)
    kps, counts = np.zeros((m * img_stride, cap), KEYPOINT_DTYPE), np.full(m * img_stride, 5, np.int32)      # (the images between the frames are not read)
    ur, Tcw, fmp = np.full((m, cap), -1.0, np.float32), np.zeros((max(n, 1), 16), np.float32), np.full((max(n, 1), cap), -1, np.int32)
    offs, pr = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 2), np.int32)
    planes, flat, start = np.zeros((m, cap, 3), np.float32), [np.full((3, 3), 1e6, np.float32)], {}
    for x in NAMES:                                                  # one map for every batch, whatever its rows: past_map, the last scene, ends it
        start[x] = sum(len(w) for w in flat)
        flat.append(S.scene_of(x)["mp_world"])
    for r, s in enumerate(scenes):
        f = 2 * r + 1 if pairs else r
        k = len(s["keys"])
        kps[f * img_stride, :k], counts[f * img_stride], ur[f, :k] = s["keys"], k, s["uright"]
        Tcw[r], fmp[r, :k] = s["Tcw"].reshape(16), s["frame_mp"]
        if pairs:
            planes[2 * r, :len(s["mp_world"])] = s["mp_world"]
            pr[r] = (2 * r, 2 * r) if r in refuse else (2 * r, 2 * r + 1)
            counts[2 * r * img_stride] = 0
        else:
            offs[r] = start[names[r]]
    world = planes.reshape(-1, 3) if pairs else np.concatenate(flat)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    raw = lambda a: dev(a.view(np.uint8).reshape(-1))
    out = {k: torch.full((n * w + SLACK,), SENT[TYPES[k]], dtype=_dtype(TYPES[k]), device="cuda") for k, w in WIDTH.items()}
    for k, _ in posepoints.ROWS:
        out[k] = torch.full((n * cap + SLACK,), SENT[TYPES[k]], dtype=_dtype(TYPES[k]), device="cuda")
    posepoints.pose_optimization_batch(raw(kps), dev(counts), img_stride, dev(ur), S.CAMERA, dev(Tcw), dev(fmp), dev(world), n_frames=n_frames,
                                       mp_index_offset=None if pairs else dev(offs), pairs=dev(pr) if pairs else None,
                                       row_active=None if active is None else dev(np.asarray(active, np.int32)), out=out, context=ctx, n_rows=n)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _dtype(t):
    from orb_line_slam_amd.pose import _torch_dtype
    return _torch_dtype(t)


def row_of(res, r, scene, cap=S.CAP):
    k = len(scene["keys"])
    g = {name: res[name][r * w:(r + 1) * w].copy() if w > 1 else res[name][r].item() for name, w in WIDTH.items()}
    for name, _ in posepoints.ROWS:
        row = res[name][r * cap:(r + 1) * cap]
        assert not row[k:].any(), (name, "is 0 from the count on")
        g[name] = row[:k].copy()
    return g


def tails_untouched(res, n, cap=S.CAP):
    return all(np.all(res[k][n * w:] == SENT[TYPES[k]]) for k, w in WIDTH.items()) and all(np.all(res[k][n * cap:] == SENT[TYPES[k]]) for k, _ in posepoints.ROWS)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8) if isinstance(a[k], np.ndarray) else a[k], np.asarray(b[k]).view(np.uint8) if isinstance(b[k], np.ndarray) else b[k])
               for k in a)


@pytest.fixture(scope="module")
def all_rows(ctx):
    """every scene in one batch (fewer than 40 rows), the run the other tests compare bits with"""
    assert len(NAMES) < 40
    res = run_rows(ctx, NAMES)
    settle(ctx, 512)                                                 # past_map's index
    assert tails_untouched(res, len(NAMES))
    return {name: row_of(res, r, S.scene_of(name)) for r, name in enumerate(NAMES)}


@pytest.mark.parametrize("name", NAMES)
def test_device_against_restatement_and_host_form(all_rows, name):
    s, got = S.scene_of(name), all_rows[name]
    ref = S.reference_of(name)
    S.check_against(dict(got, status=got["status"] | (512 if name == "past_map" else 0)), ref, name)      # (the device raises 512 in the context's word)
    h = posepoints.pose_optimization_host(s["keys"], s["uright"], s["Tcw"], s["camera"], s["frame_mp"], s["mp_world"], s["inv_level_sigma2"])
    for k in ("outlier_out", "n_good", "n_initial", "passes"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(h[k])), (name, k)
    assert got["status"] == (h["status"] & ~512)
    print(name, "ratios", [round(S.within_rule(k, got[k], ref)[1], 3) for k in S.REAL_OUTPUTS], "iters", got["iters"], h["iters"])


@pytest.mark.parametrize("img_stride", [1, 2])
def test_rows_do_not_depend_on_their_position(ctx, all_rows, img_stride):
    rng = np.random.RandomState(11 + img_stride)
    names = [NAMES[i] for i in rng.permutation(len(NAMES))]
    names.insert(5, names[0])                                        # the same row twice
    names = names[:39]
    res = run_rows(ctx, names, img_stride=img_stride)
    settle(ctx, 512 if "past_map" in names else 0)
    assert tails_untouched(res, len(names))
    for r, name in enumerate(names):
        assert same_bits(row_of(res, r, S.scene_of(name)), all_rows[name]), (r, name)


def test_pairs_form(ctx, all_rows):
    names = [n for n in NAMES if n != "past_map"]
    active = np.ones(len(names), np.int32)
    active[4], active[9] = 0, -1
    res = run_rows(ctx, names, pairs=True, active=active, refuse=(7,))
    settle(ctx, 2048)
    assert tails_untouched(res, len(names))
    for r, name in enumerate(names):
        if r in (4, 7, 9):                                           # left untouched but for n_good = -1
            assert res["n_good"][r] == -1 and np.all(res["Tcw_out"][16 * r:16 * r + 16] == 777.0) and np.all(res["outlier_out"][r * S.CAP:(r + 1) * S.CAP] == 0xAB)
            assert res["status"][r] == -777 and np.all(res["chi2"][r * S.CAP:(r + 1) * S.CAP] == 777.0)
        else:
            assert same_bits(row_of(res, r, S.scene_of(name)), all_rows[name]), (r, name)


def test_forced_scratch_path(ctx, all_rows):
    assert lib().olf_debug_pose_points_lds_limit(1024) == 0           # 29 bytes per feature of the capacity no longer fit: the edges go to scratch
    try:
        res = run_rows(ctx, NAMES)
        settle(ctx, 512)
    finally:
        lib().olf_debug_pose_points_lds_limit(0)
    assert tails_untouched(res, len(NAMES))
    for r, name in enumerate(NAMES):
        assert same_bits(row_of(res, r, S.scene_of(name)), all_rows[name]), name


def test_edge_calls(ctx, all_rows):
    import torch
    res = run_rows(ctx, [])
    settle(ctx)
    assert tails_untouched(res, 0)
    b, o = _lib.PosePointsBatchC(), _lib.PosePointsOutputsC()
    b.img_stride = 1
    assert lib().olf_pose_optimization_batch_dev(ctx.handle, C.byref(b), 1, 1, C.byref(o), None) == OLF_ERR_INVALID
    assert lib().olf_pose_optimization_batch_dev(None, C.byref(b), 0, 0, C.byref(o), None) == OLF_ERR_INVALID
    assert lib().olf_pose_optimization_rows(ctx.handle, C.byref(b), 1, 1, C.byref(o)) == OLF_ERR_INVALID
    for name in ("out20_mix", "n257_mix", "n2_stereo", "depth0"):   # the host-pointer form: one frame staged through the context
        s = S.scene_of(name)
        r = posepoints.PoseOptimization(s["keys"], s["uright"], s["Tcw"], s["camera"], s["frame_mp"], s["mp_world"], context=ctx)
        assert same_bits({k: r[k] for k in all_rows[name]}, all_rows[name]), name
    s = S.scene_of("past_map")
    with pytest.raises(OlfError):
        posepoints.PoseOptimization(s["keys"], s["uright"], s["Tcw"], s["camera"], s["frame_mp"], s["mp_world"], context=ctx)
    settle(ctx)
    torch.cuda.synchronize()


def test_chain_on_device_pointers():
    """olf_pnp_solver_pairs_dev -> olf_pnp_apply_inliers_dev -> olf_pose_optimization_batch_dev -> olf_discard_outliers_batch_dev (mode 1, stereo) ->
    olf_search_by_projection_kf_pairs_dev on device pointers: the solver's pairs, Tcw and accepted and the inlier rows go into the optimiser as they lie.
    Against the same chain through the host forms: the optimiser's discrete outputs exactly, its pose within 64 float ulp, the discard loop exactly; the
    search gives what it gives on the optimiser's outputs brought up from the host."""
    import torch
    import pnpsolver_scenes as PS
    from test_pnpsolver_cpu import fresh_state, host_call, ransac
    from test_pnpsolver_gpu import up
    from orb_line_slam_amd import matcher, pnpsolver, pose
    p = _lib.default_params()
    p.orb.nfeatures = 440
    ctx = _lib.Context(p, PS.W, PS.H, 2)
    try:
        sc, rn = PS.scene_set(), ransac(False)
        assert ctx.orb_capacity == sc.cap
        P, cap, nf, lcap = len(sc.pairs), sc.cap, len(sc.frames), ctx.line_capacity
        kps, counts, world, v, b = sc.arrays
        d_kps, d_counts, d_world, d_v, d_b = (up(a) for a in sc.arrays)
        pairs = np.asarray(sc.pairs, np.int32)
        d_pairs, d_rows = up(pairs), up(np.stack(sc.rows))
        d = {k: up(val) for k, val in fresh_state(P, cap, rn.max_iterations).items()}
        cam = PS.CAM + (40.0,)
        # ---- on the device, nothing brought back in between
        pnpsolver.pnp_solver_batch(nf, d_kps, d_counts, d_world, PS.CAM, d_pairs, d_rows, up(sc.draws[:, :rn.max_iterations]), d, rn, mp_valid=d_v, mp_bad=d_b,
                                   img_stride=1, context=ctx)
        fmp = torch.full_like(d_rows, -1)
        cur = torch.zeros((P, cap), dtype=torch.uint8, device="cuda")
        fnd = torch.zeros((P, cap), dtype=torch.uint8, device="cuda")
        pnpsolver.pnp_apply_inliers(nf, d_counts, d_pairs, d_rows, d, out=fmp, cur_valid=cur, already_found=fnd, img_stride=1, context=ctx)
        d_ur = torch.full((nf, cap), -1.0, dtype=torch.float32, device="cuda")          # a monocular sensor
        po = posepoints.pose_optimization_batch(d_kps, d_counts, 1, d_ur, cam, d["Tcw"], fmp, d_world, n_frames=nf, pairs=d_pairs, row_active=d["accepted"], context=ctx)
        fed = fmp.clone()                                            # (what the optimiser read, for the host side below)
        row_counts = d_counts[d_pairs[:, 1].long()].contiguous()     # the discard loop's rows are the pairs: each reads its frame's count
        offs = (d_pairs[:, 0] * cap).contiguous()
        zl, fml, ol = torch.zeros(P, dtype=torch.int32, device="cuda"), torch.full((P, lcap), -1, dtype=torch.int32, device="cuda"), torch.zeros((P, lcap), dtype=torch.uint8, device="cuda")
        nm = pose.discard_outliers_batch(row_counts, zl, 1, fmp, fml, po["outlier_out"], ol, nf * cap, 0, 1, only_tracking=False, stereo=True, mp_index_offset=offs, context=ctx)
        torch.cuda.synchronize()
        ctx.poll_status()
        # ---- the same chain through the host forms
        host = fresh_state(P, cap, rn.max_iterations)
        assert host_call(sc, host, rn) == 0
        acc = np.flatnonzero(host["accepted"] == 1)
        assert len(acc) >= 12 and np.array_equal(d["accepted"].cpu().numpy(), host["accepted"])
        sig = S.scene_of(NAMES[0])["inv_level_sigma2"]
        got = {k: t.cpu().numpy() for k, t in po.items()}
        fed, left, nmh = fed.cpu().numpy(), fmp.cpu().numpy(), nm.cpu().numpy()
        flat = world.reshape(-1, 3)
        eps = float(np.finfo(np.float32).eps)
        for r in range(P):
            if r not in acc:
                assert got["n_good"][r] == -1 or host["accepted"][r] == 1
                continue
            kf, fr = pairs[r]
            n = int(counts[fr])
            h = posepoints.pose_optimization_host(kps[fr, :n], np.full(n, -1.0, np.float32), host["Tcw"][r], cam, fed[r, :n], flat, sig, mp_index_offset=int(kf) * cap)
            assert h["n_initial"] >= 10 and got["n_good"][r] == h["n_good"] and got["passes"][r] == h["passes"] and got["status"][r] == h["status"], r
            assert np.array_equal(got["outlier_out"][r, :n], h["outlier_out"]) and not got["outlier_out"][r, n:].any(), r
            assert np.max(np.abs(got["Tcw_out"][r].astype(np.float64) - h["Tcw_out"])) <= 64 * eps * np.max(np.abs(h["Tcw_out"])), r
            kept = np.where(h["outlier_out"] == 1, -1, fed[r, :n])                     # :2315-2317: a held outlier is dropped, its flag kept
            assert np.array_equal(left[r, :n], kept) and nmh[r, 0] == int(((fed[r, :n] >= 0) & (h["outlier_out"] == 0)).sum()) and nmh[r, 1] == 0, r
        # ---- the search on the optimiser's outputs: device pointers against the same arrays through the host
        rng = np.random.default_rng(5)
        bounds = (0.0, float(PS.W), 0.0, float(PS.H))
        d_desc = up(rng.integers(0, 256, (nf, cap, 32), dtype=np.uint8))
        d_maxd, d_mind = up(np.full((nf, cap), 1e3, np.float32)), up(np.full((nf, cap), 1e-3, np.float32))
        goffs = torch.zeros((nf, _lib.GRID_CELLS + 1), dtype=torch.int32, device="cuda")
        gidx = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
        with matcher._torch_stream() as s:
            _lib.check(lib().olf_frame_grid_dev(ctx.handle, nf, 1, d_kps.data_ptr(), d_counts.data_ptr(), *bounds, goffs.data_ptr(), gidx.data_ptr(), s), "olf_frame_grid_dev")
        sel = torch.from_numpy(acc).cuda()
        swapped = up(np.ascontiguousarray(pairs[acc][:, ::-1]))

        def search(T, cv, af):
            m, k = matcher.search_by_projection_kf_pairs(nf, d_kps, d_desc, d_counts, goffs, gidx, d_world, d_maxd, d_mind, swapped, cam, bounds, th=10.0, ORBdist=100,
                                                         pair_Tcw=T, cur_valid=cv, already_found=af, mp_valid=d_v, mp_bad=d_b, img_stride=1, context=ctx)
            torch.cuda.synchronize()
            return m.cpu().numpy(), k.cpu().numpy()

        chained = search(po["Tcw_out"][sel].contiguous(), (fmp[sel] >= 0).to(torch.uint8).contiguous(), fnd[sel].contiguous())
        again = search(up(got["Tcw_out"][acc]), up((left[acc] >= 0).astype(np.uint8)), up(fnd.cpu().numpy()[acc]))
        assert np.array_equal(chained[0], again[0]) and np.array_equal(chained[1], again[1]) and (chained[1] >= 0).all()
        ctx.poll_status()
    finally:
        ctx.close()
