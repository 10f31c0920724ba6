"""olf_sim3_solver_pairs_dev and olf_sim3_filter_matches_dev on the device against the host form olf_sim3_solver, bit for bit (one header, no contraction),
over the scenes of tests/sim3solver_scenes.py at the context's capacity: every N of the table, both scale modes, img_stride 1 and 2, a shuffled pair
list, windows of 1, 5, 7 and 300 with carried state, the scratch-slot path against the LDS path, sentinels in everything the call must leave, malformed
pairs, an octave outside the levels, argument errors, the host-pointer form, the chain SearchByBoW -> solver -> filter -> SearchBySim3 on device pointers
with one synchronisation at its end, and the adaptor's batched function."""
import numpy as np
import pytest
import sim3solver_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, sim3solver
from test_sim3solver_cpu import SENTINEL, STATE_KEYS, fresh_state, host_call, ransac, same_state

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    p = _lib.default_params()
    p.orb.nfeatures = 440
    c = _lib.Context(p, S.W, S.H, 2)
    assert 300 < c.orb_capacity <= 1024 and c.nlevels == 8
    sf = np.zeros(8, F)
    _lib.lib().olf_orb_scale_tables(c.handle, sf.ctypes.data, None, None, None, None)
    assert np.array_equal(sf, S.SF)
    yield c
    _lib.lib().olf_debug_sim3_solver_lds_limit(0)
    c.close()


def up(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype.fields:
        a = a.view(np.uint8).reshape(a.shape + (-1,))
    return torch.from_numpy(a).cuda()


def device_call(ctx, sc, st, rn, order=None, img_stride=1, arrays=None, valid=True, bad=True, n_frames=None, pairs=None):
    """olf_sim3_solver_pairs_dev over the scene's pairs in `order`, on the rows of st in the same order (st: host arrays, changed in place)"""
    import torch
    P = len(sc.pairs)
    order = list(range(P)) if order is None else list(order)
    kps, counts, Tcw, world, v, b = arrays or S.batch_arrays(sc.frames, sc.cap, img_stride)
    d = {k: up(np.ascontiguousarray(st[k][order])) for k in STATE_KEYS}
    pr = np.asarray(sc.pairs if pairs is None else pairs, np.int32)[order]
    sim3solver.sim3_solver_batch(len(sc.frames) if n_frames is None else n_frames, up(kps), up(counts), up(Tcw), up(world), S.CAM, up(pr),
                                 up(np.stack(sc.rows)[order]), up(sc.draws[order][:, :rn.max_iterations]), d, rn, mp_valid=up(v) if valid else None,
                                 mp_bad=up(b) if bad else None, img_stride=img_stride, context=ctx)
    torch.cuda.synchronize()
    for k in STATE_KEYS:
        st[k][order] = d[k].cpu().numpy()
    return st


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("img_stride", [1, 2])
def test_device_equals_the_host_form(ctx, fix_scale, img_stride):
    sc = S.scene_set(fix_scale, ctx.orb_capacity)
    rn = ransac(sc)
    host = fresh_state(len(sc.pairs), sc.cap)
    assert host_call(sc, host, rn) == 0
    assert host["accepted"].sum() >= 8 and (host["n_correspondences"][:13] == [0, 2, 19, 20, 21, 63, 64, 65, 300, sc.cap, 40, 30, 60]).all()
    assert np.isnan(host["best_R"][11]).all() and host["best_inliers"][11] == 0          # the identity sample
    ctx.poll_status()
    dev = device_call(ctx, sc, fresh_state(len(sc.pairs), sc.cap), rn, img_stride=img_stride)
    ctx.poll_status()
    same_state(dev, host)
    # what the call must leave: rows past N1 and counts of iterations it did not evaluate (same_state compared them: the host form leaves them too)
    for p in range(len(sc.pairs)):
        N1 = sc.frames[sc.pairs[p][0]].n
        assert (dev["inliers"][p, N1:] == 99).all() and (dev["counts"][p, dev["iterations_done"][p]:] == SENTINEL).all()


def test_shuffled_pairs_and_windows(ctx):
    sc = S.scene_set(False, ctx.orb_capacity)
    P = len(sc.pairs)
    find = device_call(ctx, sc, fresh_state(P, sc.cap), ransac(sc))
    order = np.random.default_rng(3).permutation(P)
    same_state(device_call(ctx, sc, fresh_state(P, sc.cap), ransac(sc), order=order), find)
    for window in (1, 5, 7):
        rn = ransac(sc, n_iterations=window)
        st = fresh_state(P, sc.cap)
        for call in range(-(-S.MAX_ITS // window)):
            todo = [p for p in range(P) if not call or not (st["accepted"][p] or st["no_more"][p])]
            if not todo:
                break
            device_call(ctx, sc, st, rn, order=todo)
        same_state(st, find)
    ctx.poll_status()


def test_scratch_slot_path_equals_the_lds_path(ctx):
    sc = S.scene_set(False, ctx.orb_capacity)
    P = len(sc.pairs)
    lds = device_call(ctx, sc, fresh_state(P, sc.cap), ransac(sc))
    assert _lib.lib().olf_debug_sim3_solver_lds_limit(1024) == 0      # 52 bytes per feature of the capacity no longer fit: the state goes to scratch
    try:
        scratch = device_call(ctx, sc, fresh_state(P, sc.cap), ransac(sc))
    finally:
        _lib.lib().olf_debug_sim3_solver_lds_limit(0)
    same_state(scratch, lds)
    ctx.poll_status()


def test_malformed_pairs_and_octaves(ctx):
    sc = S.scene_set(False, ctx.orb_capacity)
    P, nf = len(sc.pairs), len(sc.frames)
    rn = ransac(sc)
    good = device_call(ctx, sc, fresh_state(P, sc.cap), rn)
    pairs = list(sc.pairs)
    refused = {0: (3, 3), 5: (-1, 2), 9: (4, nf), P - 1: (nf + 7, 0)}
    for p, pr in refused.items():
        pairs[p] = pr
    st = device_call(ctx, sc, fresh_state(P, sc.cap), rn, pairs=pairs)
    with pytest.raises(ola.OlfError, match="2048"):
        ctx.poll_status()
    fresh = fresh_state(P, sc.cap)
    for p in range(P):
        if p in refused:
            assert st["n_inliers"][p] == -1
            for k in STATE_KEYS:
                if k != "n_inliers":
                    assert np.array_equal(st[k][p], fresh[k][p]), (p, k)
        else:
            same_state({k: v[p:p + 1] for k, v in st.items()}, {k: v[p:p + 1] for k, v in good.items()})
    # an octave outside the levels: the correspondence is left out, bit 256, as the host form does
    arrays = [a.copy() for a in S.batch_arrays(sc.frames, sc.cap)]
    arrays[0][sc.pairs[6][0], 5]["octave"] = 8
    arrays[0][sc.pairs[8][1], 0]["octave"] = -1
    host = fresh_state(P, sc.cap)
    assert host_call(sc, host, rn, arrays=arrays) == 256
    dev = device_call(ctx, sc, fresh_state(P, sc.cap), rn, arrays=arrays)
    with pytest.raises(ola.OlfError, match="256"):
        ctx.poll_status()
    same_state(dev, host)
    assert dev["n_correspondences"][6] == 63


def test_optional_planes_and_no_pairs(ctx):
    """mp_valid and mp_bad NULL (every feature holds a good point), counts NULL, n_pairs == 0"""
    import torch
    sc = S.scene_set(False, ctx.orb_capacity)
    P = len(sc.pairs)
    rn = ransac(sc)
    host = fresh_state(P, sc.cap)
    host_call(sc, host, rn, valid=False, bad=False)
    dev = device_call(ctx, sc, fresh_state(P, sc.cap), rn, valid=False, bad=False)
    same_state(dev, host)
    assert dev["n_correspondences"][5] == 66                         # the bad, the unheld and the second bad feature count again
    kps, counts, Tcw, world, v, b = (up(a) for a in S.batch_arrays(sc.frames, sc.cap))
    d = {k: up(val) for k, val in fresh_state(P, sc.cap).items()}
    keep = {k: val.clone() for k, val in d.items()}
    sim3solver.sim3_solver_batch(len(sc.frames), kps, counts, Tcw, world, S.CAM, up(np.zeros((0, 2), np.int32)), up(np.stack(sc.rows))[:0], up(sc.draws)[:0], d, rn,
                                 img_stride=1, context=ctx)
    torch.cuda.synchronize()
    assert all(torch.equal(d[k], keep[k]) for k in d)
    d["counts"] = None
    sim3solver.sim3_solver_batch(len(sc.frames), kps, counts, Tcw, world, S.CAM, up(np.asarray(sc.pairs, np.int32)), up(np.stack(sc.rows)), up(sc.draws), d, rn,
                                 mp_valid=v, mp_bad=b, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    full = fresh_state(P, sc.cap)
    host_call(sc, full, rn)
    same_state({k: val.cpu().numpy() for k, val in d.items() if val is not None}, full, [k for k in STATE_KEYS if k != "counts"])
    ctx.poll_status()


def test_argument_errors(ctx):
    sc = S.scene_set(False, ctx.orb_capacity)
    P = len(sc.pairs)
    for kw in (dict(min_inliers=2), dict(max_iterations=0), dict(probability=0.0), dict(probability=1.5), dict(n_iterations=-1)):
        args = dict(fix_scale=False, probability=0.99, min_inliers=20, max_iterations=300, n_iterations=5)
        args.update(kw)
        with pytest.raises(ola.OlfError):
            device_call(ctx, sc, fresh_state(P, sc.cap), sim3solver.sim3_ransac(**args))
    st = fresh_state(P, sc.cap)
    import torch
    kps, counts, Tcw, world, v, b = (up(a) for a in S.batch_arrays(sc.frames, sc.cap))
    d = {k: up(val) for k, val in st.items()}
    d["best_t"] = None
    with pytest.raises(ola.OlfError):
        sim3solver.sim3_solver_batch(len(sc.frames), kps, counts, Tcw, world, S.CAM, up(np.asarray(sc.pairs, np.int32)), up(np.stack(sc.rows)), up(sc.draws), d,
                                     ransac(sc), img_stride=1, context=ctx)
    with pytest.raises(ola.OlfError):
        sim3solver.sim3_filter_matches(up(np.stack(sc.rows)), None, context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()


def test_host_pointer_form_equals_the_device_form(ctx):
    sc = S.scene_set(True, ctx.orb_capacity)
    P = len(sc.pairs)
    rn = ransac(sc)
    dev = device_call(ctx, sc, fresh_state(P, sc.cap), rn)
    kps, counts, Tcw, world, v, b = sc.arrays
    st = fresh_state(P, sc.cap)
    sim3solver.sim3_solver_pairs(kps, counts, Tcw, world, S.CAM, sc.pairs, np.stack(sc.rows), sc.draws, st, rn, mp_valid=v, mp_bad=b, context=ctx)
    same_state(st, dev)


def chain_descriptors(sc, seed=9):
    """descriptors consistent with the scenes' rows: the feature of key frame 2 a row names carries the descriptor of its feature of key frame 1 with up to
    8 bits flipped; every other feature a random one.  All angles are 0, so the rotation check keeps every match."""
    import bow_pairs_scenes as B
    rng = np.random.default_rng(seed)
    nf, cap = len(sc.frames), sc.cap
    desc = rng.integers(0, 256, (nf, cap, 32), dtype=np.uint8)
    for p in range(len(S.PAIR_SPECS)):
        a, b = sc.pairs[p]
        row, n1, n2 = sc.rows[p], sc.frames[a].n, sc.frames[b].n
        i1 = np.flatnonzero((row[:n1] >= 0) & (row[:n1] < n2))
        if len(i1):
            desc[b, row[i1]] = B._flip(rng, desc[a, i1], rng.integers(0, 9, len(i1)))
    return desc


def test_chain_bow_solver_filter_search_by_sim3(ctx):
    """olf_search_by_bow_pairs_dev (OLF_BOW_KF_KF) -> solver -> filter -> olf_search_by_sim3_pairs_dev on device pointers: the solver reads exactly the row
    the BoW entry writes, best_s / best_R / best_t are handed over without a copy, and the only synchronisation is at the end.  The same chain through
    the host forms (the oracle's SearchByBoW over the same vocabulary, olf_sim3_solver, numpy, ORBmatcher.SearchBySim3) gives the same rows."""
    import torch
    import bow_pairs_scenes as B
    from orb_line_slam_amd import matcher
    sc = S.scene_set(False, ctx.orb_capacity)
    P, cap, nf = len(sc.pairs), sc.cap, len(sc.frames)
    rn = ransac(sc)
    kps, counts, Tcw, world, v, b = sc.arrays
    desc = chain_descriptors(sc)
    levelsup = 2                                                     # the node level is the root: every feature is compared with every other
    voc, V, _ = B.make_voc(4, 2, np.concatenate([desc[f, :counts[f]] for f in range(0, nf, 2)]), stop_every=0)
    G = ola.ORBVocabulary.from_arrays(*voc, context=ctx)
    maxd, mind = np.full((nf, cap), 1e3, F), np.full((nf, cap), 1e-3, F)
    bounds = (0.0, float(S.W), 0.0, float(S.H))
    d_kps, d_counts, d_T, d_world, d_v, d_b, d_desc = (up(a) for a in (kps, counts, Tcw, world, v, b, desc))
    offs = torch.zeros((nf, _lib.GRID_CELLS + 1), dtype=torch.int32, device="cuda")
    idx = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
    with matcher._torch_stream() as s:
        _lib.check(_lib.lib().olf_frame_grid_dev(ctx.handle, nf, 1, d_kps.data_ptr(), d_counts.data_ptr(), *bounds, offs.data_ptr(), idx.data_ptr(), s),
                   "olf_frame_grid_dev")
    d_pairs, d_draws, d_maxd, d_mind = up(np.asarray(sc.pairs, np.int32)), up(sc.draws), up(maxd), up(mind)
    d = {k: up(val) for k, val in fresh_state(P, cap).items()}
    ctx.poll_status()
    # ---- the chain: no host read between its stages
    d_rows, d_nm = matcher.search_by_bow_pairs(G, nf, d_kps, d_desc, d_counts, d_pairs, mp_valid=d_v, mp_bad=d_b, form=matcher.BOW_KF_KF, nnratio=0.75,
                                               checkOri=True, levelsup=levelsup, img_stride=1, context=ctx)
    sim3solver.sim3_solver_batch(nf, d_kps, d_counts, d_T, d_world, S.CAM, d_pairs, d_rows, d_draws, d, rn, mp_valid=d_v, mp_bad=d_b, img_stride=1, context=ctx)
    d_filtered = torch.full_like(d_rows, -9)
    sim3solver.sim3_filter_matches(d_rows, d["inliers"], d["n_inliers"], out=d_filtered, context=ctx)
    res = matcher.search_by_sim3_pairs(nf, d_kps, d_desc, d_counts, offs, idx, d_T, d_world, d_maxd, d_mind, d_pairs, d["best_s"], d["best_R"], d["best_t"],
                                       S.CAM + (40.0,), bounds, matches12=d_filtered, th=7.5, mp_valid=d_v, mp_bad=d_b, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()
    # ---- the host chain
    views = []
    for f in range(nf):
        n = int(counts[f])
        fr = B.frame(desc[f, :n], None, v[f, :n].astype(bool), b[f, :n].astype(bool))
        fr.keys = kps[f, :n].copy()
        views.append(B.view(fr, V, levelsup))
    rows = np.full((P, cap), -1, np.int32)
    for p, (n_o, row_o) in enumerate(B.oracle_pairs(views, sc.pairs, B.KF_KF, 0.75, True)):
        rows[p, :len(row_o)] = row_o
    got_rows = d_rows.cpu().numpy()
    assert np.array_equal(got_rows, rows)                            # the BoW entry's row, at the context's capacity, -1 from N1 on
    # ... and it finds what the scenes planted: a true match differs in at most 16 bits, two random descriptors in about 128, so TH_LOW and the ratio test
    # pass every planted match and nothing else; the solver then sees the scenes' own numbers of correspondences
    for p in range(len(S.PAIR_SPECS)):
        fa, fb = sc.pairs[p]
        want = sc.rows[p][:sc.frames[fa].n]
        ok2 = (want >= 0) & (want < sc.frames[fb].n)
        planted = ok2 & (v[fa, :len(want)] == 1) & (b[fa, :len(want)] == 0)
        planted[ok2] &= (v[fb, want[ok2]] == 1) & (b[fb, want[ok2]] == 0)
        assert np.array_equal(rows[p, :len(want)], np.where(planted, want, -1)), p
    host = fresh_state(P, cap)
    host_call(sc, host, rn, rows=list(rows))
    same_state({k: val.cpu().numpy() for k, val in d.items()}, host)
    assert (host["n_correspondences"][:13] == [0, 2, 19, 20, 21, 63, 64, 65, 300, cap, 40, 30, 60]).all()
    filtered = np.where(host["inliers"] == 1, rows, -1).astype(np.int32)
    m = ola.ORBmatcher(0.75, True, context=ctx)
    got12, nfound = res[0].cpu().numpy(), res[3].cpu().numpy()
    checked = 0
    for p in range(P):
        a, bb = sc.pairs[p]
        if not host["accepted"][p]:
            continue
        kfs = []
        for f in (a, bb):
            n = int(counts[f])
            kf = ola.KeyFrameView(kps[f, :n], desc[f, :n], None, S.SF, *S.CAM, 40.0, bounds, mTcw=Tcw[f])
            kf.mp_valid[:], kf.mp_bad[:], kf.mp_world[:] = v[f, :n].astype(bool), b[f, :n].astype(bool), world[f, :n]
            kf.mp_maxd[:], kf.mp_mind[:], kf.mp_desc = maxd[f, :n], mind[f, :n], kf.mDescriptors.copy()
            kfs.append(kf)
        m12 = filtered[p, :counts[a]].copy()
        n, v1, v2 = m.SearchBySim3(kfs[0], kfs[1], m12, float(host["best_s"][p]), host["best_R"][p].reshape(3, 3), host["best_t"][p], 7.5)
        assert n == nfound[p] and np.array_equal(m12, got12[p, :counts[a]]), p
        checked += 1
    assert checked >= 6
    G.clear()


def test_adaptor_on_the_device(tmp_path):
    """tests/adaptor_sim3solver.cpp with `device`: a vector of solvers through Sim3SolversIterate on the thread's context, bit for bit the host form's"""
    import subprocess
    from test_sim3solver_cpu import build_adaptor
    exe = str(tmp_path / "adaptor_sim3solver")
    build_adaptor(exe)
    out = subprocess.run([exe, "device"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_SIM3SOLVER_OK" in out.stdout, out.stdout.decode()[-3000:]


def test_more_parameter_sets_than_the_table_cache_keeps(ctx):
    """Ten distinct (probability, min_inliers, max_iterations) through olf_sim3_solver_pairs_dev in one process, the first once more at the end: the host
    table cache keeps eight, so tables are evicted, their pinned buffers refilled and the first set's table built again.  Each call against the host form,
    on four small pairs; pair 10 (40 correspondences, never accepted) ends exactly at its set's cap, which is read from the table."""
    sc = S.scene_set(False, ctx.orb_capacity)
    P, order = len(sc.pairs), [3, 4, 5, 10]
    sets = [(0.99, 20, 300), (0.9, 20, 300), (0.99, 19, 300), (0.99, 20, 299), (0.5, 10, 64), (0.999, 21, 300), (0.95, 5, 7), (0.8, 30, 120), (0.99, 3, 1),
            (0.7, 12, 200)]
    assert len(set(sets)) == 10
    for pr, m, mx in sets + sets[:1]:
        rn = sim3solver.sim3_ransac(sc.fix_scale, pr, m, mx, mx)
        host = fresh_state(len(order), sc.cap, mx)
        host_call(sc, host, rn, pairs=[sc.pairs[p] for p in order], rows=[sc.rows[p] for p in order], draws=sc.draws[order])
        dev = device_call(ctx, sc, fresh_state(P, sc.cap, mx), rn, order=order)
        same_state({k: v[order] for k, v in dev.items()}, host)
    ctx.poll_status()
