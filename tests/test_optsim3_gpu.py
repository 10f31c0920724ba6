"""olf_optimize_sim3_pairs_dev on the device, against the host form and the restatement (optsim3_reference) under the tolerance rule
(optsim3_scenes.within_rule: 16 x the restatement's spread, floor 64 float ulp, for the double S12_out too); the match row, n_inliers, n_correspondences,
n_bad_first and status exactly; iters not compared.  The scenes run as two batches, one per scale mode (fix_scale belongs to the call).  Every output and
the match rows are allocated SLACK elements longer than the batch needs and filled with a sentinel: nothing may be written past a count, a row or the
batch.  Position independence, the scratch path and the staged form are compared with those batches bit for bit: between device runs bit equality is
promised, between device and host it is not (the device's exp / sin / cos, amplified by the numeric Jacobian's quotient by 2e-9).
The last test chains the entry behind the Sim3 solver, the filter and SearchBySim3 on device pointers and hands the winner's Scw to the projection search."""
import ctypes as C
import numpy as np
import pytest
import optsim3_scenes as S
import pose_scenes as PS
from orb_line_slam_amd import _lib, optsim3
from orb_line_slam_amd._lib import KEYPOINT_DTYPE, OLF_ERR_INVALID, OlfError, lib

pytestmark = pytest.mark.gpu

SLACK = 37
SENT = {np.float32: 777.0, np.float64: 777.0, np.uint8: 0xAB, np.int32: -777}
FREE = [n for n in S.NAMES if not S.scene_of(n)["fix_scale"]]
FIXED = [n for n in S.NAMES if S.scene_of(n)["fix_scale"]]
WIDTH = dict(S12_out=8, s12_out=1, R12_out=9, t12_out=3, Scw_out=16, n_inliers=1, n_correspondences=1, n_bad_first=1, iters=2, status=1, chi2=2 * S.CAP, matches=S.CAP)
TYPES = dict([(n, t) for n, t, _ in optsim3._OUT] + [("matches", np.int32)])


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401
    p = _lib.default_params()
    p.orb.nfeatures = S.NFEATURES
    c = _lib.Context(p, S.W, S.H, 2)
    assert c.orb_capacity == S.CAP and c.nlevels == S.N_LEVELS
    sig = np.zeros(c.nlevels, np.float32)
    _lib.check(lib().olf_orb_scale_tables(c.handle, None, None, None, _lib.ptr(sig), None), "olf_orb_scale_tables")
    assert np.array_equal(sig, S.scene_of(FREE[0])["inv_level_sigma2"])
    yield c
    lib().olf_debug_optimize_sim3_lds_limit(0)


def settle(ctx, bits=0):
    """wait, then read the context's status word: exactly `bits` must be set"""
    import torch
    torch.cuda.synchronize()
    if bits:
        with pytest.raises(OlfError) as e:
            ctx.poll_status()
        assert "flags=%d " % bits in str(e.value), str(e.value)
    ctx.poll_status()


def _dtype(t):
    from orb_line_slam_amd.pose import _torch_dtype
    return _torch_dtype(t)


def batch_of(names, img_stride=1, pairs=None):
    """the scenes `names` as pairs of one batch: scene r's key frames are frames 2 r and 2 r + 1 -- but `swapped` behind `clean64` reads clean64's two
    frames the other way round.  pairs: {row: (kf1, kf2)} replaces a row's pair.  Returns host arrays."""
    cap, n = S.CAP, len(names)
    m = max(2 * n, 1)
    kps, counts = np.zeros((m * img_stride, cap), KEYPOINT_DTYPE), np.full(m * img_stride, 5, np.int32)      # (the images between the frames are not read)
    Tcw, world = np.zeros((m, 16), np.float32), np.zeros((m, cap, 3), np.float32)
    valid, bad = np.zeros((m, cap), np.uint8), np.zeros((m, cap), np.uint8)
    pr, rows = np.zeros((max(n, 1), 2), np.int32), np.full((max(n, 1), cap), -1, np.int32)
    s12, R12, t12 = np.zeros(max(n, 1), np.float32), np.zeros((max(n, 1), 9), np.float32), np.zeros((max(n, 1), 3), np.float32)
    for r, name in enumerate(names):
        s = S.scene_of(name)
        for k in range(2):
            f = 2 * r + k
            kps[f * img_stride], counts[f * img_stride] = s["keys"][k], s["counts"][k]
            Tcw[f], world[f], valid[f], bad[f] = s["Tcw"][k].reshape(16), s["world"][k], s["valid"][k], s["bad"][k]
        pr[r] = (2 * r, 2 * r + 1)
        if name == "swapped" and "clean64" in names:
            q = names.index("clean64")
            pr[r] = (2 * q + 1, 2 * q)
        if pairs and r in pairs:
            pr[r] = pairs[r]
        rows[r], s12[r], R12[r], t12[r] = s["matches"], s["s12"], s["R12"], s["t12"]
    return dict(kps=kps, counts=counts, Tcw=Tcw, world=world, valid=valid, bad=bad, pairs=pr, rows=rows, s12=s12, R12=R12, t12=t12, n=n, n_frames=2 * n)


def run_pairs(ctx, names, fix_scale, img_stride=1, active=None, pairs=None):
    """the batch of `names` through olf_optimize_sim3_pairs_dev; returns the outputs and the match rows as numpy arrays with their SLACK tails"""
    import torch
    b = batch_of(names, img_stride, pairs)
    n = b["n"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    raw = lambda a: dev(a.view(np.uint8).reshape(-1))
    out = {k: torch.full((n * w + SLACK,), SENT[TYPES[k]], dtype=_dtype(TYPES[k]), device="cuda") for k, w in WIDTH.items()}
    if n:
        out["matches"][:n * S.CAP] = dev(b["rows"][:n].reshape(-1))
    optsim3.optimize_sim3_batch(b["n_frames"], raw(b["kps"]), dev(b["counts"]), dev(b["Tcw"]), dev(b["world"]), S.CAMERA, dev(b["pairs"][:n].reshape(n, 2)), out["matches"],
                                dev(b["s12"]), dev(b["R12"]), dev(b["t12"]), th2=S.TH2, fix_scale=fix_scale, row_active=None if active is None else dev(np.asarray(active, np.int32)),
                                mp_valid=dev(b["valid"]), mp_bad=dev(b["bad"]), img_stride=img_stride, out={k: v for k, v in out.items() if k != "matches"}, context=ctx)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def row_of(res, r):
    g = {name: res[name][r * w:(r + 1) * w].copy() if w > 1 else res[name][r].item() for name, w in WIDTH.items()}
    g["chi2"] = g["chi2"].reshape(S.CAP, 2)
    return g


def tails_untouched(res, n):
    return all(np.all(res[k][n * w:] == SENT[TYPES[k]]) for k, w in WIDTH.items())


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8) if isinstance(a[k], np.ndarray) else a[k], np.asarray(b[k]).view(np.uint8) if isinstance(b[k], np.ndarray) else b[k])
               for k in a)


def untouched_but_for_n_inliers(res, r):
    return res["n_inliers"][r] == -1 and all(np.all(res[k][r * w:(r + 1) * w] == SENT[TYPES[k]]) for k, w in WIDTH.items() if k not in ("n_inliers", "matches"))


@pytest.fixture(scope="module")
def all_rows(ctx):
    """every scene, one batch per scale mode (fewer than 40 pairs each): the runs the other tests compare bits with"""
    rows = {}
    for names, fix in ((FREE, False), (FIXED, True)):
        assert len(names) < 40
        res = run_pairs(ctx, names, fix)
        settle(ctx)
        assert tails_untouched(res, len(names))
        rows.update({name: row_of(res, r) for r, name in enumerate(names)})
    return rows


@pytest.mark.parametrize("name", S.NAMES)
def test_device_against_restatement_and_host_form(all_rows, name):
    from test_optsim3_cpu import host
    s, got, ref = S.scene_of(name), all_rows[name], S.reference_of(name)
    S.check_against(got, got["matches"], ref, name)
    h, hm = host(s)
    assert np.array_equal(got["matches"], hm)
    for k in S.DISCRETE:
        assert got[k] == h[k], (name, k)
    assert not got["chi2"][int(s["counts"][0]):].any()
    print(name, "ratios", [round(S.within_rule(k, got[k], ref)[1], 3) for k in S.REAL_OUTPUTS], "iters", got["iters"], h["iters"],
          "device - host S12", float(np.max(np.abs(got["S12_out"] - h["S12_out"]))))


@pytest.mark.parametrize("img_stride", [1, 2])
def test_pairs_do_not_depend_on_their_position(ctx, all_rows, img_stride):
    rng = np.random.RandomState(11 + img_stride)
    for base, fix in ((FREE, False), (FIXED, True)):
        names = [base[i] for i in rng.permutation(len(base))]
        names.insert(5, names[0])                                    # the same pair twice (on frames of its own)
        dup = {}
        if not fix:                                                  # ... and twice on the SAME frames; with `swapped` clean64's frames stand on both sides
            names.append("clean64")
            dup[len(names) - 1] = (2 * names.index("clean64"), 2 * names.index("clean64") + 1)
        res = run_pairs(ctx, names, fix, img_stride=img_stride, pairs=dup)
        settle(ctx)
        assert tails_untouched(res, len(names))
        for r, name in enumerate(names):
            assert same_bits(row_of(res, r), all_rows[name]), (r, name)


def test_refused_and_inactive_pairs(ctx, all_rows):
    names = FREE[:12]
    active = np.ones(len(names), np.int32)
    active[4], active[9] = 0, -1
    res = run_pairs(ctx, names, False, active=active, pairs={7: (14, 14), 2: (0, 2 * len(names)), 3: (-1, 6)})
    settle(ctx, 2048)
    assert tails_untouched(res, len(names))
    for r, name in enumerate(names):
        if r in (2, 3, 4, 7, 9):                                     # left untouched but for n_inliers = -1
            assert untouched_but_for_n_inliers(res, r) and np.array_equal(res["matches"][r * S.CAP:(r + 1) * S.CAP], S.scene_of(name)["matches"]), r
        else:
            assert same_bits(row_of(res, r), all_rows[name]), (r, name)


def test_forced_scratch_path(ctx, all_rows):
    assert lib().olf_debug_optimize_sim3_lds_limit(1024) == 0        # 69 bytes per feature of the capacity no longer fit: the correspondences go to scratch
    try:
        res = run_pairs(ctx, FREE, False)
        settle(ctx)
    finally:
        lib().olf_debug_optimize_sim3_lds_limit(0)
    assert tails_untouched(res, len(FREE))
    for r, name in enumerate(FREE):
        assert same_bits(row_of(res, r), all_rows[name]), name


def test_staged_form_equals_the_device_form(ctx, all_rows):
    names = ["out20", "n257_free", "gate12", "depth0", "n0_free", "skipped"]
    b = batch_of(names)
    rows = b["rows"].copy()
    out = optsim3.optimize_sim3_pairs(b["kps"], b["counts"], b["Tcw"].reshape(-1, 4, 4), b["world"], S.CAMERA, b["pairs"], rows, b["s12"], b["R12"], b["t12"], th2=S.TH2,
                                      fix_scale=False, mp_valid=b["valid"], mp_bad=b["bad"], context=ctx)
    for r, name in enumerate(names):
        got = {k: (out[k][r].copy() if out[k][r].ndim else out[k][r].item()) for k in out}
        got["matches"] = rows[r]
        assert same_bits(got, all_rows[name]), name
    refused = b["pairs"].copy()
    refused[1] = (3, 3)
    with pytest.raises(OlfError):                                    # bit 2048 of the context's word, the outputs complete
        optsim3.optimize_sim3_pairs(b["kps"], b["counts"], b["Tcw"].reshape(-1, 4, 4), b["world"], S.CAMERA, refused, b["rows"].copy(), b["s12"], b["R12"], b["t12"],
                                    mp_valid=b["valid"], mp_bad=b["bad"], context=ctx)
    settle(ctx)


def test_edge_calls(ctx, all_rows):
    res = run_pairs(ctx, [], False)
    settle(ctx)
    assert tails_untouched(res, 0)
    tb, io = _lib.TrackBatchC(), _lib.OptSim3IoC()
    tb.img_stride = 1
    one = np.zeros(16, np.float32)
    args = (None, 1, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), _lib.ptr(one))
    assert lib().olf_optimize_sim3_pairs_dev(ctx.handle, C.byref(tb), 2, *args, 10.0, 0, None, C.byref(io), None) == OLF_ERR_INVALID      # NULL planes and outputs
    assert lib().olf_optimize_sim3_pairs_dev(None, C.byref(tb), 2, None, 0, None, None, None, None, 10.0, 0, None, C.byref(io), None) == OLF_ERR_INVALID
    assert lib().olf_optimize_sim3_pairs_dev(ctx.handle, C.byref(tb), 2, None, 0, None, None, None, None, 0.0, 0, None, C.byref(io), None) == OLF_ERR_INVALID      # th2
    assert lib().olf_optimize_sim3_pairs_dev(ctx.handle, C.byref(tb), 2, None, -1, None, None, None, None, 10.0, 0, None, C.byref(io), None) == OLF_ERR_INVALID
    assert lib().olf_optimize_sim3_pairs(ctx.handle, C.byref(tb), 2, *args, 10.0, 0, None, C.byref(io)) == OLF_ERR_INVALID
    settle(ctx)


def test_adaptor_on_the_device(tmp_path):
    """tests/adaptor_opt_sim3.cpp with `device`: ORB_SLAM2::OptimizeSim3 on stand-in types through olf_optimize_sim3_pairs on a context of its own"""
    import subprocess
    from test_optsim3_cpu import build_adaptor
    exe = str(tmp_path / "adaptor_opt_sim3")
    build_adaptor(exe)
    out = subprocess.run([exe, "device"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_OPT_SIM3_OK" in out.stdout, out.stdout.decode()[-3000:]


CHAIN = ("clean64", "out20", "one_side", "n65_free", "n257_free")


def test_chain_on_device_pointers(ctx):
    """olf_sim3_solver_pairs_dev -> olf_sim3_filter_matches_dev -> olf_search_by_sim3_pairs_dev -> olf_optimize_sim3_pairs_dev on device pointers: the same
    pairs, the solver's best_s / best_R / best_t and accepted, and the rows the search wrote go into the optimiser as they lie, one synchronisation at the
    end.  Against the same chain through the host forms (olf_sim3_solver, numpy, ORBmatcher.SearchBySim3, olf_optimize_sim3) and the restatement on the
    host chain's rows, under the tolerance rule.  Then the first pair in candidate order with n_inliers >= 20 wins and its Scw_out goes into
    olf_search_by_projection_sim3_batch_dev, which gives what it gives on the same matrix brought up from the host."""
    import torch
    import orb_line_slam_amd as ola
    from orb_line_slam_amd import matcher, sim3solver
    from orb_line_slam_amd.matcher import LocalMapDev
    b = batch_of(list(CHAIN))
    P, cap, nf = b["n"], S.CAP, b["n_frames"]
    sf = PS.level_tables()[0]
    cam5, bounds = S.CAMERA + (40.0,), (0.0, float(S.W), 0.0, float(S.H))
    rng = np.random.default_rng(3)
    desc = rng.integers(0, 256, (nf, cap, 32), dtype=np.uint8)
    maxd, mind = np.full((nf, cap), 1e3, np.float32), np.full((nf, cap), 1e-3, np.float32)
    rn = sim3solver.sim3_ransac(False, 0.99, 20, 300, 300)
    draws = sim3solver.sim3_draws(P, 300, 5)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).cuda()
    d_kps = up(b["kps"].view(np.uint8).reshape(nf, -1))
    d_counts, d_T, d_world, d_v, d_b = (up(b[k]) for k in ("counts", "Tcw", "world", "valid", "bad"))
    d_desc, d_pairs, d_rows = up(desc), up(b["pairs"]), up(b["rows"])
    offs = torch.zeros((nf, _lib.GRID_CELLS + 1), dtype=torch.int32, device="cuda")
    idx = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
    with matcher._torch_stream() as s:
        _lib.check(lib().olf_frame_grid_dev(ctx.handle, nf, 1, d_kps.data_ptr(), d_counts.data_ptr(), *bounds, offs.data_ptr(), idx.data_ptr(), s), "olf_frame_grid_dev")
    d = sim3solver.sim3_state(P, cap, 300)
    ctx.poll_status()
    # ---- the chain: no host read between its stages
    sim3solver.sim3_solver_batch(nf, d_kps, d_counts, d_T, d_world, S.CAMERA, d_pairs, d_rows, up(draws), d, rn, mp_valid=d_v, mp_bad=d_b, img_stride=1, context=ctx)
    d_m = torch.full_like(d_rows, -9)
    sim3solver.sim3_filter_matches(d_rows, d["inliers"], d["n_inliers"], out=d_m, context=ctx)
    matcher.search_by_sim3_pairs(nf, d_kps, d_desc, d_counts, offs, idx, d_T, d_world, up(maxd), up(mind), d_pairs, d["best_s"], d["best_R"], d["best_t"], cam5, bounds,
                                 matches12=d_m, th=7.5, mp_valid=d_v, mp_bad=d_b, img_stride=1, context=ctx)
    d_fed = d_m.clone()                                              # (what the optimiser read, for the host side below)
    po = optsim3.optimize_sim3_batch(nf, d_kps, d_counts, d_T, d_world, S.CAMERA, d_pairs, d_m, d["best_s"], d["best_R"], d["best_t"], th2=S.TH2, fix_scale=False,
                                     row_active=d["accepted"], mp_valid=d_v, mp_bad=d_b, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()
    # ---- the same chain through the host forms
    st = sim3solver.sim3_state(P, cap, 300, device=False)
    m = ola.ORBmatcher(0.75, True, context=ctx)
    got, left, fed = {k: t.cpu().numpy() for k, t in po.items()}, d_m.cpu().numpy(), d_fed.cpu().numpy()
    winner = -1
    for p, name in enumerate(CHAIN):
        sc = S.scene_of(name)
        assert sim3solver.Sim3Solve(b["kps"], b["counts"], b["Tcw"].reshape(-1, 4, 4), b["world"], S.CAMERA, sf, b["pairs"][p], b["rows"][p], draws[p], st, rn, row=p,
                                    mp_valid=b["valid"], mp_bad=b["bad"]) == 0
        assert st["accepted"][p] == 1 == d["accepted"][p].item() and st["best_s"][p] == d["best_s"][p].item()
        row = np.where(st["inliers"][p] == 1, b["rows"][p], -1).astype(np.int32)
        kfs = []
        for f in b["pairs"][p]:
            n = int(b["counts"][f])
            kf = ola.KeyFrameView(b["kps"][f, :n], desc[f, :n], None, sf, *S.CAMERA, 40.0, bounds, mTcw=b["Tcw"][f].reshape(4, 4))
            kf.mp_valid[:], kf.mp_bad[:], kf.mp_world[:] = b["valid"][f, :n].astype(bool), b["bad"][f, :n].astype(bool), b["world"][f, :n]
            kf.mp_maxd[:], kf.mp_mind[:], kf.mp_desc = maxd[f, :n], mind[f, :n], kf.mDescriptors.copy()
            kfs.append(kf)
        n1 = int(sc["counts"][0])
        m12 = row[:n1].copy()
        m.SearchBySim3(kfs[0], kfs[1], m12, float(st["best_s"][p]), st["best_R"][p].reshape(3, 3), st["best_t"][p], 7.5)
        row[:n1] = m12
        assert np.array_equal(fed[p], row), p                        # the optimiser read the search's row as the search left it
        fed_scene = dict(sc, matches=row, s12=st["best_s"][p], R12=st["best_R"][p], t12=st["best_t"][p])
        ref = S.reference_for(fed_scene)
        assert all(np.array_equal(a["matches"], ref["base"]["matches"]) and all(a[k] == ref["base"][k] for k in S.DISCRETE) for a in ref["alts"]), name
        g = {k: (got[k][p].copy() if got[k][p].ndim else got[k][p].item()) for k in got}
        S.check_against(g, left[p], ref, "chain " + name)
        hm = row.copy()
        h = optsim3.OptimizeSim3(sc["keys"], sc["counts"], sc["Tcw"], sc["world"], S.CAMERA, sc["inv_level_sigma2"], (0, 1), hm, st["best_s"][p], st["best_R"][p],
                                 st["best_t"][p], th2=S.TH2, fix_scale=False, mp_valid=sc["valid"], mp_bad=sc["bad"])
        assert np.array_equal(left[p], hm) and all(g[k] == h[k] for k in S.DISCRETE), name
        if winner < 0 and g["n_inliers"] >= 20:
            winner = p
    assert winner == 0
    # ---- the winner's Scw_out into SearchByProjection(pKF, Scw, ...): the current key frame (kf1) against the candidate's points (kf2's, in the world frame)
    kf1, kf2 = (int(v) for v in b["pairs"][winner])
    n2 = int(b["counts"][kf2])
    T2 = b["Tcw"][kf2].reshape(4, 4).astype(np.float64)
    to_cam = -(T2[:3, :3].T @ T2[:3, 3]) - b["world"][kf2, :n2].astype(np.float64)             # the points' mean viewing directions: towards kf2's centre
    normal = (to_cam / np.linalg.norm(to_cam, axis=1, keepdims=True)).astype(np.float32)
    lm = LocalMapDev(d_world[kf2, :n2].contiguous(), up(normal), up(maxd[kf2, :n2]), up(mind[kf2, :n2]), d_desc[kf2, :n2].contiguous(), None, up(np.zeros(n2, np.uint8)))
    th = np.zeros(nf, np.float32)
    th[kf1] = 10.0

    def search(Scw_row):
        Scw = torch.zeros((nf, 4, 4), dtype=torch.float32, device="cuda")
        Scw[kf1] = Scw_row.reshape(4, 4)
        fm, nm = matcher.search_by_projection_sim3_batch(nf, d_kps, d_desc, d_counts, offs, idx, lm, Scw, torch.full((nf, cap), -1, dtype=torch.int32, device="cuda"),
                                                         cam5, bounds, th=10.0, d_th=up(th), img_stride=1, context=ctx)
        torch.cuda.synchronize()
        return fm.cpu().numpy(), nm.cpu().numpy()

    chained = search(po["Scw_out"][winner])
    again = search(up(got["Scw_out"][winner]))
    assert np.array_equal(chained[0], again[0]) and np.array_equal(chained[1], again[1]) and (chained[1] >= 0).all()
    ctx.poll_status()
