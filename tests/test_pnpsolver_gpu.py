"""olf_pnp_solver_pairs_dev and olf_pnp_apply_inliers_dev on the device against the host form olf_pnp_solver, bit for bit on every field (one header, no
contraction; NaNs compared as one pattern), over the scenes of tests/pnpsolver_scenes.py at the context's capacity: every N of the table, both parameter
sets, img_stride 1 and 2, the pair list permuted and duplicated, windows of 1, 5, 7 and 300 with carried state (resumed after acceptances and beyond the
cap), the scratch-slot path against the LDS path, sentinels in everything the call must leave, malformed pairs, an octave outside the levels, the
optional planes, n_pairs == 0, the host-pointer form, and olf_pnp_apply_inliers_dev against numpy with its outputs fed to
olf_search_by_projection_kf_pairs_dev on device pointers, and the adaptor's batched function.  At most 18 pairs per call (the scenes' 18) -- there is no hook that makes the grid smaller
than the list, and a list longer than the 1024 resident workgroups would not stay within seconds, so the grid stride is not exercised here."""
import numpy as np
import pytest
import pnpsolver_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib, pnpsolver
from test_pnpsolver_cpu import SENTINEL, STATE_KEYS, fresh_state, host_call, prm, ransac, same_state

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def ctx():
    p = _lib.default_params()
    p.orb.nfeatures = 440
    c = _lib.Context(p, S.W, S.H, 2)
    assert c.orb_capacity == S.CAP and c.nlevels == 8
    sf = np.zeros(8, F)
    _lib.lib().olf_orb_scale_tables(c.handle, sf.ctypes.data, None, None, None, None)
    assert np.array_equal(sf, S.SF)
    yield c
    _lib.lib().olf_debug_pnp_solver_lds_limit(0)
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
    """olf_pnp_solver_pairs_dev over the scene's pairs in `order`, on the rows of st in the same order (st: host arrays, changed in place)"""
    import torch
    P = len(sc.pairs)
    order = list(range(P)) if order is None else list(order)
    kps, counts, world, v, b = arrays or S.batch_arrays(sc.frames, sc.cap, img_stride)
    d = {k: up(np.ascontiguousarray(st[k][order])) for k in STATE_KEYS}
    pr = np.asarray(sc.pairs if pairs is None else pairs, np.int32)[order]
    pnpsolver.pnp_solver_batch(len(sc.frames) if n_frames is None else n_frames, up(kps), up(counts), up(world), S.CAM, up(pr), up(np.stack(sc.rows)[order]),
                               up(sc.draws[order][:, :rn.max_iterations]), d, rn, mp_valid=up(v) if valid else None, mp_bad=up(b) if bad else None,
                               img_stride=img_stride, context=ctx)
    torch.cuda.synchronize()
    for k in STATE_KEYS:
        st[k][order] = d[k].cpu().numpy()
    return st


@pytest.fixture(scope="module")
def found(ctx):
    """find() of every pair under both parameter sets, by the host form and by the device: shared by the tests below and left unchanged"""
    sc = S.scene_set()
    P = len(sc.pairs)
    res = {}
    for alt in (False, True):
        rn = ransac(alt)
        host = fresh_state(P, sc.cap, rn.max_iterations)
        assert host_call(sc, host, rn) == 0
        ctx.poll_status()
        dev = device_call(ctx, sc, fresh_state(P, sc.cap, rn.max_iterations), rn)
        ctx.poll_status()
        res[alt] = (host, dev)
    return sc, res


@pytest.mark.parametrize("alt", [False, True])
def test_device_equals_the_host_form(ctx, found, alt):
    sc, res = found
    host, dev = res[alt]
    assert (host["n_correspondences"] == [0, 3, 4, 9, 10, 11, 19, 20, 21, 22, 63, 64, 65, 300, sc.cap, 41, 40, 30]).all()
    assert host["accepted"].sum() >= 12 and (host["no_more"][:3] == 1).all()
    same_state(dev, host)
    # what the call must leave: rows past the frame's count, the counts of iterations it did not evaluate, the pose of a call that returns none
    for p in range(len(sc.pairs)):
        Nf = sc.frames[sc.pairs[p][1]].n
        assert (dev["inliers"][p, Nf:] == 99).all() and (dev["counts"][p, dev["iterations_done"][p]:] == SENTINEL).all()
        if not dev["accepted"][p]:
            assert (dev["Tcw"][p] == 5.0).all()


def test_stride_two_batch(ctx, found):
    sc, res = found
    rn = ransac(False)
    same_state(device_call(ctx, sc, fresh_state(len(sc.pairs), sc.cap, rn.max_iterations), rn, img_stride=2), res[False][1])
    ctx.poll_status()


def test_permuted_and_duplicated_pairs(ctx, found):
    sc, res = found
    P = len(sc.pairs)
    rn = ransac(False)
    order = np.random.default_rng(3).permutation(P)
    same_state(device_call(ctx, sc, fresh_state(P, sc.cap, rn.max_iterations), rn, order=order), res[False][1])
    # duplicates: the same pair twice in one list, each on its own rows of the state
    import types
    twice = types.SimpleNamespace(frames=sc.frames, cap=sc.cap, pairs=[sc.pairs[k] for k in (13, 5, 13, 15, 5)], rows=[sc.rows[k] for k in (13, 5, 13, 15, 5)],
                                  draws=sc.draws[[13, 5, 13, 15, 5]])
    st = device_call(ctx, twice, fresh_state(5, sc.cap, rn.max_iterations), rn)
    for row, k in enumerate((13, 5, 13, 15, 5)):
        same_state({key: v[row:row + 1] for key, v in st.items()}, {key: v[k:k + 1] for key, v in res[False][1].items()})
    ctx.poll_status()


@pytest.mark.parametrize("window", [1, 5, 7, 300])
def test_windows_with_carried_state(ctx, found, window):
    """three calls of a window each, on the device and by the host form: resumed after an acceptance, and beyond the cap (the OR of :182); where the cap
    is at least the window, or Refine accepted, the first call is find()"""
    sc, res = found
    P = len(sc.pairs)
    alt = window == 300                                               # (max_iterations 300 in one parameter set only)
    rn = ransac(alt, n_iterations=window)
    host, dev = fresh_state(P, sc.cap, rn.max_iterations), fresh_state(P, sc.cap, rn.max_iterations)
    for call in range(3):
        host_call(sc, host, rn)
        device_call(ctx, sc, dev, rn)
        same_state(dev, host)
        if call == 0 and window <= 5:
            import ctypes as C
            f, m, c = res[alt][0], C.c_int32(0), C.c_int32(0)
            same = []
            for p in range(P):
                assert _lib.lib().olf_debug_pnp_solver_parameters(int(f["n_correspondences"][p]), C.byref(rn), C.addressof(m), C.addressof(c)) == 0
                if f["n_correspondences"][p] >= m.value and ((f["accepted"][p] and not f["no_more"][p]) or c.value >= window):
                    same.append(p)
            assert len(same) >= 12
            for p in same:
                same_state({k: v[p:p + 1] for k, v in dev.items()}, {k: v[p:p + 1] for k, v in res[alt][1].items()})
    assert (host["iterations_done"][[4, 16]] > [1, 35]).all()      # N == minimum (cap 1) and the pair that never accepts: beyond their caps
    ctx.poll_status()


def test_scratch_slot_path_equals_the_lds_path(ctx, found):
    sc, res = found
    rn = ransac(False)
    assert _lib.lib().olf_debug_pnp_solver_lds_limit(1024) == 0       # 32 bytes per feature of the capacity no longer fit: the planes go to scratch
    try:
        scratch = device_call(ctx, sc, fresh_state(len(sc.pairs), sc.cap, rn.max_iterations), rn)
    finally:
        _lib.lib().olf_debug_pnp_solver_lds_limit(0)
    same_state(scratch, res[False][1])
    ctx.poll_status()


def test_malformed_pairs_and_octaves(ctx, found):
    sc, res = found
    P, nf = len(sc.pairs), len(sc.frames)
    rn = ransac(False)
    good = res[False][1]
    pairs = list(sc.pairs)
    refused = {0: (3, 3), 5: (-1, 2), 9: (4, nf), P - 1: (nf + 7, 0)}
    for p, pr in refused.items():
        pairs[p] = pr
    st = device_call(ctx, sc, fresh_state(P, sc.cap, rn.max_iterations), rn, pairs=pairs)
    with pytest.raises(ola.OlfError, match="2048"):
        ctx.poll_status()
    fresh = fresh_state(P, sc.cap, rn.max_iterations)
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
    arrays[0][sc.pairs[11][1], 5]["octave"] = 8
    arrays[0][sc.pairs[13][1], 0]["octave"] = -1
    host = fresh_state(P, sc.cap, rn.max_iterations)
    assert host_call(sc, host, rn, arrays=arrays) == 256
    dev = device_call(ctx, sc, fresh_state(P, sc.cap, rn.max_iterations), rn, arrays=arrays)
    with pytest.raises(ola.OlfError, match="256"):
        ctx.poll_status()
    same_state(dev, host)
    assert dev["n_correspondences"][11] == 63 and dev["n_correspondences"][13] == 299


def test_optional_planes_no_pairs_and_argument_errors(ctx, found):
    """mp_valid and mp_bad NULL (every feature holds a good point), counts NULL, n_pairs == 0, the refused parameter sets"""
    import torch
    sc, res = found
    P = len(sc.pairs)
    rn = ransac(False)
    mi = rn.max_iterations
    host = fresh_state(P, sc.cap, mi)
    host_call(sc, host, rn, valid=False, bad=False)
    dev = device_call(ctx, sc, fresh_state(P, sc.cap, mi), rn, valid=False, bad=False)
    same_state(dev, host)
    assert dev["n_correspondences"][10] == 65                         # the unheld and the bad feature count again
    kps, counts, world, v, b = (up(a) for a in S.batch_arrays(sc.frames, sc.cap))
    d = {k: up(val) for k, val in fresh_state(P, sc.cap, mi).items()}
    keep = {k: val.clone() for k, val in d.items()}
    pnpsolver.pnp_solver_batch(len(sc.frames), kps, counts, world, S.CAM, up(np.zeros((0, 2), np.int32)), up(np.stack(sc.rows))[:0], up(sc.draws[:, :mi])[:0], d,
                               rn, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    assert all(torch.equal(d[k], keep[k]) for k in d)
    d["counts"] = None
    pnpsolver.pnp_solver_batch(len(sc.frames), kps, counts, world, S.CAM, up(np.asarray(sc.pairs, np.int32)), up(np.stack(sc.rows)), up(sc.draws[:, :mi]), d, rn,
                               mp_valid=v, mp_bad=b, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    same_state({k: val.cpu().numpy() for k, val in d.items() if val is not None}, res[False][0], [k for k in STATE_KEYS if k != "counts"])
    for kw in (dict(min_set=3), dict(epsilon=0.0), dict(epsilon=1.5), dict(th2=0.0), dict(min_inliers=0), dict(max_iterations=0), dict(probability=1.5),
               dict(n_iterations=-1)):
        with pytest.raises(ola.OlfError):
            device_call(ctx, sc, fresh_state(P, sc.cap, mi), ransac(False, **kw))
    d = {k: up(val) for k, val in fresh_state(P, sc.cap, mi).items()}
    d["refined_flags"] = None
    with pytest.raises(ola.OlfError):
        pnpsolver.pnp_solver_batch(len(sc.frames), kps, counts, world, S.CAM, up(np.asarray(sc.pairs, np.int32)), up(np.stack(sc.rows)), up(sc.draws[:, :mi]), d,
                                   rn, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()


def test_host_pointer_form_equals_the_device_form(ctx, found):
    sc, res = found
    rn = ransac(True)
    kps, counts, world, v, b = sc.arrays
    st = fresh_state(len(sc.pairs), sc.cap, rn.max_iterations)
    pnpsolver.pnp_solver_pairs(kps, counts, world, S.CAM, sc.pairs, np.stack(sc.rows), sc.draws[:, :rn.max_iterations], st, rn, mp_valid=v, mp_bad=b, context=ctx)
    same_state(st, res[True][1])


def test_apply_inliers_and_the_chain_into_search_by_projection(ctx, found):
    """olf_pnp_apply_inliers_dev against numpy; then its three outputs and the solver's Tcw go into olf_search_by_projection_kf_pairs_dev as device pointers,
    without a copy, and the search gives what it gives on the same arrays brought up from the host"""
    import torch
    from orb_line_slam_amd import matcher
    sc, res = found
    host = res[False][0]
    P, cap, nf = len(sc.pairs), sc.cap, len(sc.frames)
    rn = ransac(False)
    kps, counts, world, v, b = sc.arrays
    d_kps, d_counts, d_world, d_v, d_b = (up(a) for a in sc.arrays)
    d_pairs, d_rows = up(np.asarray(sc.pairs, np.int32)), up(np.stack(sc.rows))
    d = {k: up(val) for k, val in fresh_state(P, cap, rn.max_iterations).items()}
    pnpsolver.pnp_solver_batch(nf, d_kps, d_counts, d_world, S.CAM, d_pairs, d_rows, up(sc.draws[:, :rn.max_iterations]), d, rn, mp_valid=d_v, mp_bad=d_b,
                               img_stride=1, context=ctx)
    out = torch.full_like(d_rows, -9)
    cur = torch.full((P, cap), 7, dtype=torch.uint8, device="cuda")
    fnd = torch.full((P, cap), 7, dtype=torch.uint8, device="cuda")
    pnpsolver.pnp_apply_inliers(nf, d_counts, d_pairs, d_rows, d, out=out, cur_valid=cur, already_found=fnd, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    rows = np.stack(sc.rows)
    want_out, want_cur, want_fnd = np.full((P, cap), -9, np.int32), np.full((P, cap), 7, np.uint8), np.full((P, cap), 7, np.uint8)
    for p in range(P):
        if not host["accepted"][p]:
            continue
        Nf = sc.frames[sc.pairs[p][1]].n
        on = np.zeros(cap, bool)
        on[:Nf] = host["inliers"][p, :Nf] == 1
        want_out[p], want_cur[p] = np.where(on, rows[p], -1), on
        want_fnd[p] = 0
        want_fnd[p, rows[p][on]] = 1
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(cur.cpu().numpy(), want_cur) and np.array_equal(fnd.cpu().numpy(), want_fnd)
    assert host["accepted"].sum() >= 12
    # ---- the chain: the accepted pairs, ordered (current frame, key frame) for the projection search
    acc = np.flatnonzero(host["accepted"] == 1)
    rng = np.random.default_rng(5)
    desc = rng.integers(0, 256, (nf, cap, 32), dtype=np.uint8)
    bounds = (0.0, float(S.W), 0.0, float(S.H))
    maxd, mind = np.full((nf, cap), 1e3, F), np.full((nf, cap), 1e-3, F)
    d_desc, d_maxd, d_mind = up(desc), up(maxd), up(mind)
    offs = torch.zeros((nf, _lib.GRID_CELLS + 1), dtype=torch.int32, device="cuda")
    idx = torch.zeros((nf, cap), dtype=torch.int32, device="cuda")
    with matcher._torch_stream() as s:
        _lib.check(_lib.lib().olf_frame_grid_dev(ctx.handle, nf, 1, d_kps.data_ptr(), d_counts.data_ptr(), *bounds, offs.data_ptr(), idx.data_ptr(), s),
                   "olf_frame_grid_dev")
    sel = torch.from_numpy(acc).cuda()
    swapped = up(np.ascontiguousarray(np.asarray(sc.pairs, np.int32)[acc][:, ::-1]))

    def search(T, cv, af):
        m, n = matcher.search_by_projection_kf_pairs(nf, d_kps, d_desc, d_counts, offs, idx, d_world, d_maxd, d_mind, swapped, S.CAM + (40.0,), bounds, th=10.0,
                                                     ORBdist=100, pair_Tcw=T, cur_valid=cv, already_found=af, mp_valid=d_v, mp_bad=d_b, img_stride=1,
                                                     context=ctx)
        torch.cuda.synchronize()
        return m.cpu().numpy(), n.cpu().numpy()

    chained = search(d["Tcw"][sel].contiguous(), cur[sel].contiguous(), fnd[sel].contiguous())
    again = search(up(host["Tcw"][acc]), up(want_cur[acc]), up(want_fnd[acc]))
    assert np.array_equal(chained[0], again[0]) and np.array_equal(chained[1], again[1]) and (chained[1] >= 0).all()
    ctx.poll_status()


def test_adaptor_on_the_device(tmp_path):
    """tests/adaptor_pnpsolver.cpp with `device`: a vector of solvers through PnPsolversIterate on the thread's context, bit for bit the host form's"""
    import subprocess
    from test_pnpsolver_cpu import build_adaptor
    exe = str(tmp_path / "adaptor_pnpsolver")
    build_adaptor(exe)
    out = subprocess.run([exe, "device"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_PNPSOLVER_OK" in out.stdout, out.stdout.decode()[-3000:]


def test_more_parameter_sets_than_the_table_cache_keeps(ctx):
    """Ten distinct (probability, min_inliers, max_iterations) through olf_pnp_solver_pairs_dev in one process, the first once more at the end: the host
    table cache keeps eight, so tables are evicted, their pinned buffers refilled and the first set's table built again.  Each call against the host form,
    on four small pairs (11, 21, 63 and 40 correspondences); the effective min_inliers and the cap of a pair are read from the table."""
    sc = S.scene_set()
    P, order = len(sc.pairs), [5, 8, 10, 16]
    sets = [(0.99, 10, 40), (0.9, 10, 40), (0.99, 9, 40), (0.99, 10, 39), (0.5, 12, 16), (0.999, 11, 40), (0.95, 5, 7), (0.8, 20, 30), (0.99, 4, 1), (0.7, 12, 25)]
    assert len(set(sets)) == 10
    for pr, m, mx in sets + sets[:1]:
        rn = ransac(False, probability=pr, min_inliers=m, max_iterations=mx)
        host = fresh_state(P, sc.cap, mx)
        host_call(sc, host, rn, only=set(order))
        dev = device_call(ctx, sc, fresh_state(P, sc.cap, mx), rn, order=order)
        same_state({k: v[order] for k, v in dev.items()}, {k: v[order] for k, v in host.items()})
    ctx.poll_status()
